"""GPU tier of the speculative gunzip of ordinary .gz input: the cases of tests/_gunzip_stream_common.py (the ones
test_gunzip_stream_host.py runs on the CPU twin) through the gfx950 kernels -- ``HipBackend.gunzip_stream`` and
``device_gunzip="any"`` of the reader and the file drivers -- checked against ``zlib.decompressobj(-15)``, the
``device_gunzip=False`` reader and the twin."""
import pytest

from . import _gunzip_stream_common as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("writer", sorted(S.WRITERS))
def test_writers(hip_backend, writer):
    S.check_writer(hip_backend, writer)


def test_distance_32768(hip_backend):
    S.check_window_edge(hip_backend)


def test_ring_hazard(hip_backend):
    S.check_ring(hip_backend)


def test_sources_across_a_chunk_start(hip_backend):
    S.check_straddle(hip_backend)


def test_period_chain(hip_backend):
    S.check_period_chain(hip_backend)


def test_block_on_a_chunk_boundary_and_odd_start_bit(hip_backend):
    S.check_aligned_block(hip_backend)


def test_deflate_inside_stored_blocks(hip_backend):
    S.check_double(hip_backend)


def test_resume(hip_backend):
    S.check_resume(hip_backend)


def test_slab_cuts(hip_backend):
    S.check_slab_cuts(hip_backend)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 2049])
def test_launch(hip_backend, count):
    S.check_launch(hip_backend, count)


def test_empty_final_block(hip_backend):
    S.check_empty(hip_backend)


def test_corrupt_streams(hip_backend):
    S.check_corrupt(hip_backend)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_speculation_is_used(hip_backend, level):
    S.check_cap(hip_backend, level)


def test_same_result_words_as_the_twin(hip_backend):
    """The kernels and their CPU twin run one source (inflate_stream_core.hpp): every result word, the counters
    included, and the text -- for whole streams, a cut slab, a small room and the corrupt streams."""
    twin = S.StreamEmuBackend()
    calls = [dict(deflate=d, chunk_bytes=cb) for d, cb in S.agreement_streams()]
    d0 = calls[0]["deflate"]
    calls += [dict(deflate=d0, chunk_bytes=512, n_stream=len(d0) * 2 // 3), dict(deflate=d0, chunk_bytes=512, capacity=50000)]
    calls += [dict(deflate=s, chunk_bytes=1024, capacity=120000) for _, s in S.corrupt_streams()[::4]]
    for how in calls:
        a, b = S.run(hip_backend, **how), S.run(twin, **how)
        if a["status"] not in (0, S.NEED_INPUT, S.NEED_ROOM):
            assert a["status"] == b["status"]
        else:
            assert a == b, {k: (a[k], b[k]) for k in a if k != "text" and a[k] != b[k]}


# ---------------------------------------------------------------------------------------------- reader and drivers
def test_reader(hip_backend, tmp_path):
    S.check_reader(hip_backend, tmp_path)


def test_reader_small_chunks(hip_backend, tmp_path):
    S.check_reader(hip_backend, tmp_path, chunk_bytes=3000)


def test_trim_file(hip_backend, tmp_path):
    S.check_trim_file(tmp_path)


def test_trim_file_fasta(hip_backend, tmp_path):
    S.check_trim_file(tmp_path, fasta=True)


def test_trim_files_paired(hip_backend, tmp_path):
    S.check_trim_files(tmp_path)


def test_stats(hip_backend, tmp_path):
    S.check_stats(tmp_path)


def test_detect(hip_backend, tmp_path):
    S.check_detect(tmp_path)

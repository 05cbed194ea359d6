"""CPU tier of the speculative gunzip of ordinary .gz input (``gunzip_stream``, ``device_gunzip="any"``): the cases of
tests/_gunzip_stream_common.py through the CPU twin of the kernels (tests/emu/emu_gunzip_stream.cpp, built from the
product's inflate_stream_core.hpp), checked against ``zlib.decompressobj(-15)`` and the ``device_gunzip=False`` reader;
seeded bit flips, truncations and slab cuts through a stand-alone sanitized program (tests/emu/gunzip_stream_fuzz_main.cpp)."""
import struct
import subprocess
import zlib

import numpy as np
import pytest

from atropos_amd import _lib

from . import _gunzip_common as U
from . import _gunzip_stream_common as S


@pytest.fixture(scope="module")
def twin():
    return S.StreamEmuBackend()


@pytest.fixture()
def gz_backend(twin):
    prev = _lib.set_backend(twin, _test_double=True)
    yield twin
    _lib.set_backend(prev, _test_double=True)


@pytest.mark.parametrize("writer", sorted(S.WRITERS))
def test_writers(twin, writer):
    S.check_writer(twin, writer)


def test_distance_32768(twin):
    S.check_window_edge(twin)


def test_ring_hazard(twin):
    S.check_ring(twin)


def test_sources_across_a_chunk_start(twin):
    S.check_straddle(twin)


def test_period_chain(twin):
    S.check_period_chain(twin)


def test_block_on_a_chunk_boundary_and_odd_start_bit(twin):
    S.check_aligned_block(twin)


def test_deflate_inside_stored_blocks(twin):
    S.check_double(twin)


def test_resume(twin):
    S.check_resume(twin)


def test_slab_cuts(twin):
    S.check_slab_cuts(twin)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 2049])
def test_launch(twin, count):
    S.check_launch(twin, count)


def test_empty_final_block(twin):
    S.check_empty(twin)


def test_corrupt_streams(twin):
    S.check_corrupt(twin)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_speculation_is_used(twin, level):
    """The cap against a build that decodes everything serially: of the chunks in which a dynamic block starts, seven
    in eight are confirmed."""
    S.check_cap(twin, level)


@pytest.mark.parametrize("which", ["twin", "library"])
def test_abi_errors(twin, which):
    if which == "twin":
        call, work = twin._symbol("atr_gunzip_stream"), twin._symbol("atr_gunzip_stream_workspace")
        S.check_abi_errors(lambda *a: call(*a), work)
    else:
        lib = _lib.load_library()
        S.check_abi_errors(lib.atr_gunzip_stream, lib.atr_gunzip_stream_workspace)


def _fuzz_cases():
    """[(stream, n_stream, start_bit, window length, capacity, chunk_bytes)]: valid streams, their seeded bit flips,
    truncations and slab cuts, and calls that begin at a later block with the text before it as the window."""
    rng = np.random.default_rng(0x51ab)
    text = S.fastq_text(30000)
    valid = [U.raw_deflate(text[:9000], level=6), U.raw_deflate(text[:2000], level=0), U.raw_deflate(text[:3000], strategy=zlib.Z_FIXED),
             U.raw_deflate(text, level=1, mem=1), U.raw_deflate(text[:12000], flushes=((1, zlib.Z_FULL_FLUSH), (4000, zlib.Z_SYNC_FLUSH))),
             U.raw_deflate(U.CONTENTS["period_003"](9000), level=9), b"\x01\x00\x00\xff\xff"]
    valid += [S.deflate_of(m) for n, m in sorted(U.corrupt_corpus().items())]
    cases = []
    for d in valid:
        cbs = (64, 300, 1 << 16)
        cases.append((d, len(d), 0, 0, 40000, 256))
        for bit in sorted(set(int(b) for b in rng.integers(0, 8 * len(d), 120)) | set(range(min(40, 8 * len(d))))):
            cases.append((U._flip(d, bit), len(d), 0, 0, 40000, cbs[bit % 3]))
        for cut in sorted(set(int(c) for c in rng.integers(0, len(d) + 1, 30))):
            cases.append((d, cut, 0, 0, 40000, cbs[cut % 3]))
        for cap in (0, 1, 257, 5000):
            cases.append((d, len(d), 0, 0, cap, 128))
    for d in valid[:6]:
        for b in S.blocks_of(d)[1:8]:
            cases.append((d, len(d), b["start"], min(32768, b["text_at"]), 40000, 200))
            cases.append((d, len(d), b["start"], min(100, b["text_at"]), 40000, 200))      # (too short a window: far matches are errors)
    return cases


def _partial(data):
    """What zlib gives of a stream before it reports its error."""
    z, out = zlib.decompressobj(-15), b""
    try:
        for i in range(len(data)):
            out += z.decompress(data[i:i + 1])
    except zlib.error:
        pass
    return out


def test_fuzz_standalone(tmp_path):
    """The twin's code in a program of its own under the address and undefined-behaviour sanitizers, the stream, the
    window and the text in heap blocks of exactly their sizes: a zero exit, no report, and for every case zlib's
    verdict -- an error exactly when zlib reports one on the same bytes, else a prefix of zlib's text that ends on a
    block boundary, all of it when the final block lies inside the slab."""
    prog = S.build_fuzz()
    cases = _fuzz_cases()
    assert len(cases) > 3000
    with open(tmp_path / "cases.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for d, n, start, wlen, cap, cb in cases:
            before = b""
            if start:
                at = next(b["text_at"] for b in S.blocks_of(d) if b["start"] == start)
                before = zlib.decompressobj(-15).decompress(d)[:at]
            window = before[len(before) - wlen:] if wlen else b""
            fh.write(struct.pack("<IIIIII", n, start, len(window), zlib.crc32(before), cap, cb) + d[:n] + window)
    run = subprocess.run([prog, str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = run.stderr.decode("utf-8", "replace")
    assert run.returncode == 0, err[-2000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-2000:]
    raw = (tmp_path / "results.bin").read_bytes()
    at = errors = finals = 0
    for i, (d, n, start, wlen, cap, cb) in enumerate(cases):
        status, end_bit, final, crc, size = struct.unpack("<iIIII", raw[at:at + 20])
        got = raw[at + 20:at + 20 + size]
        at += 20 + size
        what = (i, n, start, wlen, cap, cb)
        if start:                                                            # zlib from the start of the stream is the oracle
            whole = S.oracle(d)
            assert whole is not None
            t0 = next(b["text_at"] for b in S.blocks_of(d) if b["start"] == start)
            far = any(dist > pos - t0 + wlen for b in S.blocks_of(d) if b["start"] >= start for pos, _, dist in b["matches"])
            if far:
                assert status == 11, what
                errors += 1
            else:
                assert status == 0 and final == 1 and got == whole[0][t0:] and crc == zlib.crc32(whole[0]), what
            continue
        want = S.oracle(d, n)
        if want is None and cap < 40000:                                     # (the room may end before the error is reached)
            assert status not in (0, S.NEED_INPUT) or _partial(d[:n]).startswith(got), (what, status)
            continue
        if want is None:
            assert status not in (0, S.NEED_INPUT, S.NEED_ROOM), (what, status)
            errors += 1
            continue
        assert status in (0, S.NEED_INPUT, S.NEED_ROOM), (what, status)
        if status:
            assert size == 0 and end_bit == 0, what
            continue
        assert want[0].startswith(got) and crc == zlib.crc32(got), what
        assert len(got) <= cap, what
        if final:
            assert want[1] and got == want[0], what
            finals += 1
        elif want[1]:
            assert len(want[0]) > cap or len(got) < len(want[0]), what
            assert len(want[0]) > cap, what                                  # (only the room keeps a whole stream from its end)
    assert at == len(raw) and errors >= 200 and finals >= 200, (errors, finals)


# ---------------------------------------------------------------------------------------------- reader and drivers
def test_reader(gz_backend, tmp_path):
    calls = gz_backend.stream_calls
    S.check_reader(gz_backend, tmp_path)
    assert gz_backend.stream_calls > calls + 20


def test_reader_small_chunks(gz_backend, tmp_path):
    S.check_reader(gz_backend, tmp_path, chunk_bytes=3000)


def test_trim_file(gz_backend, tmp_path):
    S.check_trim_file(tmp_path)


def test_trim_file_fasta(gz_backend, tmp_path):
    S.check_trim_file(tmp_path, fasta=True)


def test_trim_files_paired(gz_backend, tmp_path):
    S.check_trim_files(tmp_path)


def test_detect(gz_backend, tmp_path):
    S.check_detect(tmp_path)


def test_qc_and_error_rate_get_the_same_text(gz_backend, tmp_path, monkeypatch):
    """The statistics kernels have no CPU twin (tests/test_gpu_gunzip_stream.py compares their results): here the
    drivers run with the counting replaced by a recorder, and the file's records reach it as from the plain file."""
    from atropos_amd import stats
    seen = []

    def collect(self, *batches):
        seen.append([bytes(b.data[:int(b.line_ends[4 * len(b) - 1].item()) + 1].numpy().tobytes()) if len(b) else b"" for b in batches])

    for cls in (stats.ReadStatistics, stats.SingleEndReadStatistics, stats.PairedEndReadStatistics):
        monkeypatch.setattr(cls, "collect_batch", collect)
        monkeypatch.setattr(cls, "summarize", lambda self: None)
    monkeypatch.setattr(stats.ReadStatistics, "error_rate", lambda self, max_bases: (0.0, 0))
    plain, gz = S.stats_inputs(tmp_path)
    text = open(plain, "rb").read()

    def fed(call, path, **how):
        del seen[:]
        call(path, chunk_bytes=8000, **how)
        assert len(seen) > 10
        return b"".join(chunk[0] for chunk in seen)

    for call in (stats.qc_file, stats.error_rate_file):
        assert fed(call, gz, device_gunzip="any") == fed(call, plain) == text

"""The chunk boundaries of ``fastq.ChunkedFastqReader`` against a recording (tests/golden/reader_trace.json, written by
tests/golden/make_reader_trace_golden.py with the reader of the commit the fixture names): per reader and chunk
``(nbytes, consumed, final)``, and ``inflate_path``, for one seeded input per input road at two chunk sizes.  They decide
part-file contents and the bytes of device-gzip output.  Also: a constructor that fails leaves nothing open."""
import pytest

from tests import _reader_trace_common as T
from tests.conftest import load_golden


def check_trace(tmp_path, backends, only=None):
    want = load_golden("reader_trace.json")
    got = T.record(tmp_path, backends, only)
    assert got["inputs"] == want["inputs"]                  # (else: this zlib deflates differently, nothing is said about the reader)
    names = sorted(want["traces"]) if only is None else sorted(only)
    assert sorted(got["traces"]) == names
    for name in names:
        for size in T.CHUNK_SIZES:
            assert got["traces"][name][str(size)] == want["traces"][name][str(size)], (name, size)
    return len(names)


def test_chunk_trace_is_the_recorded_one(tmp_path):
    from tests import _bam_common as B
    from tests import _gunzip_stream_common as S
    assert len(load_golden("reader_trace.json")["commit"]) == 40
    assert check_trace(tmp_path, (S.StreamEmuBackend(), B.BamEmuBackend())) == 10


@pytest.mark.gpu
def test_chunk_trace_of_the_device_roads_on_the_gpu(hip_backend, tmp_path):
    assert check_trace(tmp_path, (hip_backend, hip_backend), T.DEVICE_ROADS) == 6


@pytest.mark.parametrize("fails_in,suffix,device_gunzip,npools,nbuf", [
    ("bgzf_scan", ".fastq.gz", True, 0, 0), ("empty", ".fastq.gz", "any", 2, 1), ("empty", ".fastq", False, 2, 4)])
def test_a_constructor_that_fails_leaves_nothing_open(tmp_path, monkeypatch, fails_in, suffix, device_gunzip, npools, nbuf):
    """Whatever fails after the file is open -- the look at the first member (``device_gunzip=True``: no source yet), the
    gzip-stream source's first allocation on the device (``"any"``), or the first upload of a plain file with its reads
    in flight -- closes the file, shuts both executors down and hands the staging buffers back."""
    from atropos_amd import fastq
    from tests import _gunzip_stream_common as S
    from tests import _gzip_common as G

    class Broken(S.StreamEmuBackend):
        def bgzf_scan(self, *a):
            if fails_in == "bgzf_scan":
                raise RuntimeError("the backend fails")
            return S.StreamEmuBackend.bgzf_scan(self, *a)

        def empty(self, *a):
            if fails_in == "empty":
                raise RuntimeError("the backend fails")
            return S.StreamEmuBackend.empty(self, *a)

    pools, buffers, made = [], [], []

    real_pool = fastq.ThreadPoolExecutor

    class Pool(real_pool):
        def __init__(self, *a, **k):
            real_pool.__init__(self, *a, **k)
            pools.append(self)

    class Reader(fastq.ChunkedFastqReader):
        def __init__(self, *a, **k):
            made.append(self)
            fastq.ChunkedFastqReader.__init__(self, *a, **k)

    real = fastq._staging
    monkeypatch.setattr(fastq, "ThreadPoolExecutor", Pool)
    monkeypatch.setattr(fastq, "_staging", lambda *a: (buffers.append(real(*a)), buffers[-1])[1])
    monkeypatch.setattr(fastq, "_STAGING_POOL", [])
    text = G.fastq_input(nrec=20)
    path = tmp_path / ("in" + suffix)
    path.write_bytes(S.gz_member(text) if suffix.endswith(".gz") else text)
    with pytest.raises(RuntimeError, match="the backend fails"):
        Reader(str(path), 4096, Broken(), device_gunzip=device_gunzip)
    assert made[0].file.closed and made[0].buf == []
    assert all(p._shutdown for p in pools) and len(pools) == npools
    assert len(buffers) == nbuf
    assert [id(t) for t in fastq._STAGING_POOL] == [id(t) for t in buffers]

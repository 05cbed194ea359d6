"""CPU tier of the device gunzip (``bgzf_scan``, ``gunzip_members``, ``device_gunzip=True`` of the file drivers): the
cases of tests/_gunzip_common.py through the CPU twin of the kernel (tests/emu/emu_gunzip.cpp, built from the product's
inflate_core.hpp), checked against ``zlib.decompress(member, 31)`` / ``gzip.decompress``; the corrupt corpus and seeded
bit flips and truncations through a stand-alone sanitized program (tests/emu/gunzip_fuzz_main.cpp)."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

from atropos_amd import _lib

from . import _gunzip_common as U
from . import _gzip_common as G
from .emu.backend import EmuBackend


@pytest.fixture(scope="module")
def twin():
    return EmuBackend()


@pytest.fixture()
def gz_backend(twin):
    prev = _lib.set_backend(twin, _test_double=True)
    yield twin
    _lib.set_backend(prev, _test_double=True)


def test_fixture_conditions(twin):
    """What a member case is named after is read from its parsed stream, not from how it was written."""
    U.fixture_conditions(twin)


@pytest.mark.parametrize("writer", sorted(U.WRITERS))
def test_members(twin, writer):
    cases = U.member_cases(writer, twin)
    assert len(cases) >= len(U.CONTENTS) + len(U.LENGTHS)
    U.check_members(twin, cases)


def test_subfield_before_bc(twin):
    text = U.CONTENTS["synth_fastq"](5000)
    cases = [("two subfields", U.member(text, before=b"XY\x03\x00abc" + b"Z\x00\x00\x00"), text)]
    U.check_members(twin, cases)


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 2049])
def test_launch(twin, count):
    U.check_launch(twin, count)


def test_members_are_independent(twin):
    U.check_independence(twin)


def test_placement(twin):
    """The stream and the text at 1, 2 and 3 bytes past an allocation."""
    cases = U.mixed_members(twin, 9)
    for off in (1, 2, 3):
        texts, status, bad = U.run_members(twin, [m for m, _ in cases], stream_off=off, text_off=4 - off, text_start=off)
        assert bad == 0 and texts == [t for _, t in cases]


def test_corrupt_corpus(twin):
    codes = U.check_corpus(twin)
    print("status per corrupt member:", codes)


def test_ranges_that_are_none(twin):
    U.check_ranges(twin)


def test_reader_names_the_offset(twin, tmp_path):
    U.check_reader_offsets(twin, tmp_path)


def _verdict(m):
    try:
        return zlib.decompress(m, 31)
    except zlib.error:
        return None


def _bgzf_header_ok(m):
    """The BGZF rules of a member's header, restated: magic, CM 8, FEXTRA and no flag that adds a field, a 'BC'
    subfield of SLEN 2 among the extra subfields, BSIZE + 1 the member's size."""
    if len(m) < 12 or m[:3] != b"\x1f\x8b\x08" or not m[3] & 4 or m[3] & 0xfa:
        return False
    end, at = 12 + struct.unpack("<H", m[10:12])[0], 12
    while at + 4 <= end <= len(m):
        slen = struct.unpack("<H", m[at + 2:at + 4])[0]
        if m[at:at + 2] == b"BC":
            return slen == 2 and at + 6 <= end and struct.unpack("<H", m[at + 4:at + 6])[0] + 1 == len(m) and end + 8 <= len(m)
        at += 4 + slen
    return False


def _fuzz_cases():
    """[(what, member, expected text or None)]: the corrupt corpus, valid members, and their seeded single-bit flips
    and truncations.  A changed member is judged by zlib, unless its header breaks a BGZF rule that zlib knows nothing
    of (FLG, the 'BC' subfield, BSIZE): then it must be refused."""
    rng = np.random.default_rng(0xb62f)
    text = U.CONTENTS["synth_fastq"](3000)
    valid = {
        "level6": U.member(text[:700], level=6), "level0": U.member(text[:300], level=0),
        "fixed": U.member(text[:500], strategy=zlib.Z_FIXED), "huffman_only": U.member(text[:2000], strategy=zlib.Z_HUFFMAN_ONLY),
        "flushed": U.member(text, flushes=((1, zlib.Z_FULL_FLUSH), (1000, zlib.Z_SYNC_FLUSH), (2500, zlib.Z_FULL_FLUSH))),
        "mem1": U.member(text, mem=1), "empty": G.EOF, "rebuilt": U.corrupt_corpus()["rebuilt"],
        "subfield": U.member(text[:400], before=b"XY\x01\x00q"),
    }
    cases = [("corpus " + n, m, None) for n, m in sorted(U.corrupt_corpus().items()) if n != "rebuilt"]
    for name, m in sorted(valid.items()):
        cases.append(("valid " + name, m, zlib.decompress(m, 31)))
        start = U.data_start(m)
        bits = set(int(b) for b in rng.integers(0, 8 * len(m), 160)) | set(range(8 * start, 8 * start + 48)) | set(range(8 * len(m) - 64, 8 * len(m)))
        for bit in sorted(bits):
            flipped = U._flip(m, bit)
            cases.append(("%s bit %d" % (name, bit), flipped, _verdict(flipped) if _bgzf_header_ok(flipped) else None))
        for cut in sorted(set(int(c) for c in rng.integers(0, len(m), 10)) | {len(m) - 1, len(m) - 8, start, 25, 26}):
            if 0 <= cut < len(m):
                cases.append(("%s cut at %d" % (name, cut), m[:cut], None))
    return cases


def test_fuzz_standalone(tmp_path):
    """The twin's per-member code in a program of its own under the address and undefined-behaviour sanitizers: a zero
    exit, no report, and for every case zlib's verdict -- and, where zlib takes a changed member, zlib's text."""
    prog = U.build_fuzz()
    cases = _fuzz_cases()
    assert len(cases) > 1500 and sum(1 for c in cases if "bit" in c[0] and c[2] is not None) >= 5
    with open(tmp_path / "cases.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _, m, _ in cases:
            fh.write(struct.pack("<I", len(m)) + m)
    run = subprocess.run([prog, str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE)
    err = run.stderr.decode("utf-8", "replace")
    assert run.returncode == 0, err[-2000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-2000:]
    raw = (tmp_path / "results.bin").read_bytes()
    at = 0
    for what, m, want in cases:
        status, size = struct.unpack("<iI", raw[at:at + 8])
        at += 8
        if want is None:
            assert status != 0, what
        else:
            assert status == 0 and raw[at:at + size] == want, (what, status)
        at += size
    assert at == len(raw)


def test_scan(twin):
    text = U.CONTENTS["synth_fastq"](10000)
    members = [U.member(text[:3000]), G.EOF, U.member(text[3000:3001], level=0), U.member(text[3001:], before=b"AB\x02\x00xy")]
    blob = b"".join(members)
    sizes = [len(m) for m in members]
    buf = torch.frombuffer(bytearray(b"pad" + blob + b"\0" * 32), dtype=torch.uint8)

    def scan(n, cap=10):
        m_at, t_at, k, covered, ok = twin.bgzf_scan(buf, 3, 3 + n, cap)
        return m_at[:k + 1].tolist(), t_at[:k + 1].tolist(), covered, ok

    assert scan(len(blob)) == (list(np.cumsum([0] + sizes)), [0, 3000, 3000, 3001, 10000], len(blob), True)
    assert scan(len(blob), cap=2) == ([0, sizes[0], sizes[0] + 28], [0, 3000, 3000], sizes[0] + 28, True)
    assert scan(len(blob), cap=0) == ([0], [0], 0, True)
    for short in (0, 5, 17, sizes[0] - 1):
        assert scan(short) == ([0], [0], 0, True)                          # (stops at a member that is not whole)
    assert scan(sizes[0] + 20)[2] == sizes[0] and scan(len(blob) - 1)[2] == len(blob) - sizes[3]
    # headers that are no BGZF member: magic, CM, no FEXTRA, no 'BC', SLEN other than 2, ISIZE above 65 536
    m = members[0]
    bad = [b"\x1e" + m[1:], m[:2] + b"\x07" + m[3:], m[:3] + b"\0" + m[4:], m[:12] + b"BD" + m[14:], m[:14] + b"\x03" + m[15:],
           m[:-4] + struct.pack("<I", 65537), gzip.compress(text)]
    for i, b in enumerate(bad):
        both = torch.frombuffer(bytearray(G.EOF + b + b"\0" * 16), dtype=torch.uint8)
        m_at, t_at, k, covered, ok = twin.bgzf_scan(both, 0, 28 + len(b), 10)
        assert (k, covered, ok) == (1, 28, False), i
    assert twin.bgzf_scan(torch.frombuffer(bytearray(m[:-4] + struct.pack("<I", 65536)), dtype=torch.uint8), 0, len(m), 4)[2] == 1


@pytest.mark.parametrize("which", ["twin", "library"])
def test_abi_errors(twin, which):
    """The refusals come before any pointer is looked at (the library's too: no device is needed for them)."""
    if which == "twin":
        scan, gunzip = twin._symbol("atr_bgzf_scan"), twin._symbol("atr_gunzip_members")
    else:
        lib = _lib.load_library()
        scan, gunzip = lib.atr_bgzf_scan, lib.atr_gunzip_members
    members = lambda *a: gunzip(*(a + (None,)))
    assert members(None, -1, None, None, 0, None, 0, None, None) == -1
    assert members(None, 100, None, None, -1, None, 0, None, None) == -1
    assert members(None, 100, None, None, 1, None, -1, None, None) == -1
    assert members(None, 1 << 32, None, None, 1, None, 10, None, None) == -2
    assert members(None, 100, None, None, 1, None, 1 << 32, None, None) == -2
    assert members(None, 1 << 31, None, None, (1 << 22) + 1, None, 10, None, None) == -2
    assert members(None, 100, None, None, 4, None, 10, None, None) == -1   # (100 bytes hold no four members)
    assert members(None, 100, None, None, 1, None, 10, None, None) == -1   # (no pointers)
    assert members(None, 0, None, None, 0, None, 0, None, None) == -1      # (d_bad is always needed)
    import ctypes as C
    k, covered = C.c_int64(), C.c_int64()
    one = (C.c_int64 * 2)()
    assert scan(None, C.c_int64(-1), C.c_int64(1), one, one, C.byref(k), C.byref(covered)) == -1
    assert scan(None, C.c_int64(10), C.c_int64(1), one, one, C.byref(k), C.byref(covered)) == -1
    assert scan(None, C.c_int64(0), C.c_int64(-1), one, one, C.byref(k), C.byref(covered)) == -1
    assert scan(None, C.c_int64(0), C.c_int64(1), None, one, C.byref(k), C.byref(covered)) == -1
    assert scan(None, C.c_int64(0), C.c_int64(1), one, one, C.byref(k), C.byref(covered)) == 0 and k.value == 0


# ---------------------------------------------------------------------------------------------- drivers
def test_trim_file(gz_backend, tmp_path):
    U.check_trim_file(tmp_path)
    assert gz_backend.inflate_calls > 10


def test_trim_files_paired(gz_backend, tmp_path):
    U.check_trim_files(tmp_path)


def test_detect(gz_backend, tmp_path):
    U.check_detect(tmp_path)


def test_qc_and_error_rate_get_the_same_text(gz_backend, tmp_path, monkeypatch):
    """The statistics kernels have no CPU twin (tests/test_gpu_gunzip.py compares their results): here the drivers
    run with the counting replaced by a recorder, and every file's records reach it as from the plain file."""
    from atropos_amd import stats
    seen = []

    def collect(self, *batches):
        seen.append([bytes(b.data[:int(b.line_ends[4 * len(b) - 1].item()) + 1].numpy().tobytes()) if len(b) else b"" for b in batches])

    for cls in (stats.ReadStatistics, stats.SingleEndReadStatistics, stats.PairedEndReadStatistics):
        monkeypatch.setattr(cls, "collect_batch", collect)
        monkeypatch.setattr(cls, "summarize", lambda self: None)
    monkeypatch.setattr(stats.ReadStatistics, "error_rate", lambda self, max_bases: (0.0, 0))
    plain, gz = U._stats_inputs(tmp_path)
    text = open(plain, "rb").read()

    def fed(call, *paths, **how):
        del seen[:]
        call(*paths, chunk_bytes=8000, **how)
        assert len(seen) > 10
        if call is stats.error_rate_file and len(paths) == 2:                 # (a recorder per file, called in turn)
            return [b"".join(chunk[0] for chunk in seen[i::2]) for i in range(2)]
        return [b"".join(chunk[i] for chunk in seen) for i in range(len(seen[0]))]

    for call, n in ((stats.qc_file, 1), (stats.qc_files, 2), (stats.error_rate_file, 1), (stats.error_rate_file, 2)):
        assert fed(call, *[gz] * n, device_gunzip=True) == fed(call, *[plain] * n) == [text] * n


def test_round_trip(gz_backend, tmp_path):
    U.check_round_trip(tmp_path)


def test_inputs_and_errors(gz_backend, tmp_path):
    U.check_inputs(gz_backend, tmp_path)


def test_default_flag_is_todays_path(gz_backend, tmp_path):
    from atropos_amd.trim import pipeline_from_args
    text = G.fastq_input(nrec=100)
    (tmp_path / "in.fastq.gz").write_bytes(U.bgzf_bytes(text))
    (tmp_path / "in.fastq").write_bytes(text)
    calls = gz_backend.inflate_calls
    assert U.read_all(tmp_path / "in.fastq.gz", gz_backend) == (text, "host")
    a = pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(str(tmp_path / "in.fastq.gz"), str(tmp_path / "a.fastq"), chunk_bytes=1 << 14)
    b = pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(str(tmp_path / "in.fastq"), str(tmp_path / "b.fastq"), chunk_bytes=1 << 14)
    assert a == b and (tmp_path / "a.fastq").read_bytes() == (tmp_path / "b.fastq").read_bytes()
    assert gz_backend.inflate_calls == calls

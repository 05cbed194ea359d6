"""Unaligned BAM input on the CPU twin (tests/emu/emu_bam.cpp over bam_core.hpp): the record walk and the decode at the
C ABI against the plain model of ``_bam_common``, the reader and the file drivers against the files the reference
writes for the same reads as FASTQ (tests/golden), and the twin as a sanitized program of its own over damaged
streams and byte soups."""
import os
import subprocess

import pytest

from atropos_amd import _lib, fastq
from tests import _bam_common as B


@pytest.fixture()
def bam_backend():
    """The CPU emulation with the BAM entry points served by their own twin library."""
    prev = _lib.set_backend(B.BamEmuBackend(), _test_double=True)
    yield _lib.get_backend()
    _lib.set_backend(prev, _test_double=True)


# ---------------------------------------------------------------------------------------------- header and format
def test_file_format_and_input_format():
    assert fastq.file_format("x.bam") == "bam" and fastq.file_format("dir/X.BAM") == "bam"
    assert fastq.file_format("x.fq.gz") == "fastq" and fastq.file_format("x.fa") == "fasta" and fastq.file_format("x") is None
    for name in ("x.sam", "x.bam.gz", "x.csfasta"):
        with pytest.raises(NotImplementedError):
            fastq.file_format(name)
    assert fastq.input_format("x.bam") == "bam" and fastq.input_format("reads", "bam") == "bam"
    with pytest.raises(ValueError):
        fastq.input_format("x.bam", "sam")


def test_header(bam_backend):
    refs = [(b"chr%d" % k, 10 * k) for k in range(7)]
    head = B.header(refs=refs)
    assert bam_backend.bam_header(head + b"rest") == (len(head), 7)
    assert bam_backend.bam_header(B.header()) == (len(B.header()), 0)
    for k in range(len(head)):
        assert bam_backend.bam_header(head[:k]) is None, k              # need more bytes
    with pytest.raises(ValueError):
        bam_backend.bam_header(b"BAM\2" + head[4:])
    with pytest.raises(ValueError):
        bam_backend.bam_header(b"@r\nACGT\n")


# ---------------------------------------------------------------------------------------------- the walk
def test_walk_boundary_sweep(bam_backend):
    assert B.check_sweep(bam_backend) == B.TILE


def test_walk_long_record(bam_backend):
    assert B.check_long_record(bam_backend) == 13


def test_walk_decoys_are_repaired(bam_backend):
    assert B.check_decoys(bam_backend) == 2


def test_walk_cut_at_every_byte(bam_backend):
    assert B.check_truncation(bam_backend) > 500


def test_walk_corruption_and_determinism(bam_backend):
    assert B.check_corruption(bam_backend) == 5


def test_walk_arguments(bam_backend):
    lib = B.load_twin()
    walk, decode = lib["atr_bam_walk"][0], lib["atr_bam_to_fastq"][0]
    assert walk(None, 1 << 32, 0, 0, 0, 256, B.CAP, None, 0, None, None, 0, None) == -2     # before any pointer
    assert walk(None, 10, 11, 0, 0, 256, B.CAP, None, 0, None, None, 0, None) == -1
    assert walk(None, 10, 0, 0, 0, 8, B.CAP, None, 0, None, None, 0, None) == -1
    assert decode(None, 1 << 31, None, 0, 0, None, None, None, None, None) == -2
    assert decode(None, 10, None, -1, 0, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- the decode
def test_decode(bam_backend):
    assert B.check_decode_all(bam_backend) == len(B.decode_records())


def test_decode_paired(bam_backend):
    assert B.check_decode_paired(bam_backend) == 12


# ---------------------------------------------------------------------------------------------- reader and drivers
def test_drivers_single_end(bam_backend, tmp_path):
    assert B.check_drivers_single(bam_backend, tmp_path) > 1000


def test_drivers_golden_single_end_cases(bam_backend, tmp_path):
    assert B.check_golden_single(bam_backend, tmp_path) >= 3


def test_drivers_paired(bam_backend, tmp_path):
    assert B.check_drivers_paired(bam_backend, tmp_path) > 1000


def test_golden_interleaved_names_are_refused_as_a_pair(bam_backend, tmp_path):
    assert B.check_golden_interleaved_names(bam_backend, tmp_path)


def test_refusals_and_errors(bam_backend, tmp_path):
    assert B.check_refusals(bam_backend, tmp_path)


# ---------------------------------------------------------------------------------------------- the stand-alone driver
def test_fuzz_driver_under_the_sanitizers(tmp_path):
    """tests/emu/bam_fuzz_main.cpp: the twin over damaged streams and byte soups, as a program of its own with
    -fsanitize=address,undefined (nothing of it is loaded into Python)."""
    from tests.emu import backend as emu
    exe = str(tmp_path / "bam_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DATR_HOST_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + emu._INC + [os.path.join(emu._HERE, "bam_fuzz_main.cpp"),
                                                                      os.path.join(emu._HERE, "emu_bam.cpp"), "-o", exe])
    out = subprocess.run([exe, "1500", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    assert b"ok: 1500 runs" in out.stdout and b" 0 repaired tiles" not in out.stdout


def test_qc_error_rate_and_detect_take_bam(bam_backend, tmp_path):
    assert B.check_other_drivers(bam_backend, tmp_path)

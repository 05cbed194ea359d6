"""Unaligned BAM input on the MI355X: the kernels of atropos_amd/csrc/bam_kernels.hip (record walk, decode to FASTQ
text) against the plain model of ``_bam_common`` and against their CPU twin, and the file drivers on BAM files made
here against the files the reference writes for the same reads as FASTQ (tests/golden).  The kernel-level cases use
tiles of 256 bytes, so every tile-edge case is reached within kilobytes."""
import pytest

from atropos_amd import _lib
from tests import _bam_common as B

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the walk
def test_walk_boundary_sweep(hip_backend):
    assert B.check_sweep(hip_backend) == B.TILE


def test_walk_long_record(hip_backend):
    assert B.check_long_record(hip_backend) == 13


def test_walk_decoys_are_repaired(hip_backend):
    twin = B.BamEmuBackend()
    for overshoot in (False, True):                                      # the inputs reach the repair path on the twin too
        assert B.run_walk(twin, B.decoy_stream(overshoot), final=True)[3] > 0
    assert B.check_decoys(hip_backend) == 2


def test_walk_cut_at_every_byte(hip_backend):
    assert B.check_truncation(hip_backend) > 500


def test_walk_corruption_and_determinism(hip_backend):
    assert B.check_corruption(hip_backend) == 5


def test_walk_arguments_without_pointers(hip_backend):
    lib = hip_backend.lib
    assert lib.atr_bam_walk(None, 1 << 32, 0, 0, 0, 256, B.CAP, None, 0, None, None, 0, None) == -2
    assert lib.atr_bam_to_fastq(None, 1 << 31, None, 0, 0, None, None, None, None, None) == -2
    assert lib.atr_bam_walk(None, 10, 11, 0, 0, 256, B.CAP, None, 0, None, None, 0, None) == -1


# ---------------------------------------------------------------------------------------------- the decode
def test_decode(hip_backend):
    assert B.check_decode_all(hip_backend) == len(B.decode_records())


def test_decode_paired(hip_backend):
    assert B.check_decode_paired(hip_backend) == 12


def test_device_against_the_twin(hip_backend):
    got, want = B.everything(hip_backend), B.everything(B.BamEmuBackend())
    assert len(got) == len(want) > 80
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, k                                                 # every returned word and byte


# ---------------------------------------------------------------------------------------------- reader and drivers
def test_drivers_single_end(hip_backend, tmp_path):
    assert B.check_drivers_single(hip_backend, tmp_path) > 1000


def test_drivers_golden_single_end_cases(hip_backend, tmp_path):
    assert B.check_golden_single(hip_backend, tmp_path) >= 3


def test_drivers_paired(hip_backend, tmp_path):
    assert B.check_drivers_paired(hip_backend, tmp_path) > 1000


def test_golden_interleaved_names_are_refused_as_a_pair(hip_backend, tmp_path):
    assert B.check_golden_interleaved_names(hip_backend, tmp_path)


def test_qc_error_rate_and_detect_take_bam(hip_backend, tmp_path):
    assert B.check_other_drivers(hip_backend, tmp_path)


def test_refusals_and_errors(hip_backend, tmp_path):
    assert B.check_refusals(hip_backend, tmp_path)
    assert _lib.BAM_MAX_BLOCK == 64 << 20                                # the cap is the reader's carry reserve

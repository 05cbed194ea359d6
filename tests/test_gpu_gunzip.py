"""GPU tier of the device gunzip: the cases of tests/_gunzip_common.py (the ones test_gunzip_host.py runs on the CPU
twin) through the gfx950 kernel -- ``HipBackend.gunzip_members``, ``HipBackend.bgzf_scan`` and ``device_gunzip=True`` of
the file drivers -- checked against ``zlib.decompress(member, 31)``, ``gzip.decompress`` and the twin; then the launch:
member counts around the wave size and above two thousand, members of unlike size, streams and texts at odd addresses;
then the named corrupt corpus (which the sanitized stand-alone program of the CPU tier has passed): refused, within
bounds."""
import pytest
import torch

from . import _gunzip_common as U
from . import _gzip_common as G

pytestmark = pytest.mark.gpu


def test_fixture_conditions(hip_backend):
    """The conditions that the project's own compressor meets are read from what the GPU compressor wrote."""
    U.fixture_conditions(hip_backend)


@pytest.mark.parametrize("writer", sorted(U.WRITERS))
def test_members(hip_backend, writer):
    cases = U.member_cases(writer, hip_backend)
    assert len(cases) >= len(U.CONTENTS) + len(U.LENGTHS)
    U.check_members(hip_backend, cases)


def test_subfield_before_bc(hip_backend):
    text = U.CONTENTS["synth_fastq"](5000)
    U.check_members(hip_backend, [("two subfields", U.member(text, before=b"XY\x03\x00abc" + b"Z\x00\x00\x00"), text)])


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 2049])
def test_launch(hip_backend, count):
    U.check_launch(hip_backend, count)


def test_members_are_independent(hip_backend):
    U.check_independence(hip_backend)


def test_placement_on_two_streams(hip_backend):
    """The stream and the text at 1, 2 and 3 bytes past an allocation, on two streams in turn."""
    cases = U.mixed_members(hip_backend, 9)
    streams = [torch.cuda.Stream(device=hip_backend.device) for _ in range(2)]
    for i, off in enumerate((1, 2, 3, 3, 2, 1)):
        streams[i % 2].wait_stream(torch.cuda.current_stream(hip_backend.device))
        with torch.cuda.stream(streams[i % 2]):
            texts, status, bad = U.run_members(hip_backend, [m for m, _ in cases], stream_off=off, text_off=4 - off, text_start=off)
        assert bad == 0 and texts == [t for _, t in cases], off


def test_same_status_and_text_as_the_twin(hip_backend):
    """The kernel and its CPU twin run one source (inflate_core.hpp): the corrupt corpus gets the same status codes."""
    from .emu.backend import EmuBackend
    twin = EmuBackend()
    assert U.check_corpus(hip_backend) == U.check_corpus(twin)


def test_ranges_that_are_none(hip_backend):
    U.check_ranges(hip_backend)


def test_reader_names_the_offset(hip_backend, tmp_path):
    U.check_reader_offsets(hip_backend, tmp_path)


def test_scan(hip_backend):
    text = U.CONTENTS["synth_fastq"](10000)
    blob = U.bgzf_bytes(text, size=3000)
    buf = torch.frombuffer(bytearray(blob + b"\0" * 16), dtype=torch.uint8)
    m_at, t_at, k, covered, ok = hip_backend.bgzf_scan(buf, 0, len(blob), 16)
    assert (k, covered, ok) == (5, len(blob), True) and t_at[:6].tolist() == [0, 3000, 6000, 9000, 10000, 10000]
    assert [m[0] for m in G.parse_members(blob)] == m_at[:5].tolist()


def test_abi_errors(hip_backend):
    lib = hip_backend.lib
    assert lib.atr_gunzip_members(None, -1, None, None, 0, None, 0, None, None, None) == -1
    assert lib.atr_gunzip_members(None, 1 << 32, None, None, 1, None, 10, None, None, None) == -2
    assert lib.atr_gunzip_members(None, 100, None, None, 4, None, 10, None, None, None) == -1
    assert lib.atr_gunzip_members(None, 100, None, None, 1, None, 10, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- drivers
def test_trim_file(hip_backend, tmp_path):
    U.check_trim_file(tmp_path)


def test_trim_files_paired(hip_backend, tmp_path):
    U.check_trim_files(tmp_path)


def test_qc_and_error_rate(hip_backend, tmp_path):
    U.check_stats(tmp_path)


def test_detect(hip_backend, tmp_path):
    U.check_detect(tmp_path)


def test_round_trip(hip_backend, tmp_path):
    U.check_round_trip(tmp_path)


def test_inputs_and_errors(hip_backend, tmp_path):
    U.check_inputs(hip_backend, tmp_path)

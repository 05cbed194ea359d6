"""The kernels of atropos_amd/csrc/detect_kernels.hip at the C ABI, with arguments of their own, against the plain Python
model of tests/_detect_kernels_common.py: per-read ``kept``, ``hashes`` and ``rep``, reads up to 320 bases, hand-built
runs for the collision branch of the distinct pass, every bit-set width and alphabet of the match pass, the largest
known lists the LDS holds.  Every comparison is exact.  tests/test_detect_kernels_host.py runs the same checks on the
CPU twin and asserts, from the model alone, that the cases are not hollow."""
import pytest

from . import _detect_common as DC
from . import _detect_kernels_common as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin():
    return DC.DetectEmuBackend()


@pytest.mark.parametrize("i", range(len(K.FILTER_HANDLES)))
def test_filter_kept_and_hashes_per_read(i, hip_backend, twin):
    rep = K.check_filter(hip_backend, i, twin)
    print(rep)
    assert rep["compared"] == sum(K.FILTER_SLICES) + rep["reads"] and rep["twin_compared"] == rep["reads"]


def test_filter_second_grid_trip_and_error_paths(hip_backend, twin):
    assert K.check_filter_grid(hip_backend, twin)["compared"] == 16385
    assert K.check_filter_errors(hip_backend) == dict(refused=3, overlong=2)


@pytest.mark.parametrize("m", K.MARK_SIZES)
def test_mark_hand_built_runs(m, hip_backend):
    rep = K.check_mark(hip_backend, m)
    print(rep)
    assert rep["compared"] == m
    if m >= 257:
        assert rep["longest_run"] == 257 and rep["crossing"] >= 1
    if m >= 63:
        assert rep["collided"] > 0 and rep["distinct"] < m


@pytest.mark.parametrize("name", sorted(K.MATCH_CASES))
def test_match_counters(name, hip_backend):
    rep = K.check_match(hip_backend, name)
    print({k: v for k, v in rep.items() if k != "lengths"})
    assert rep["compared"] == sum(K.match_case(name)["rep"])


def test_match_refused_k_invalid_read_and_second_grid_trip(hip_backend):
    assert K.check_refused_k(hip_backend) == 5
    assert K.check_invalid(hip_backend) == 1
    assert K.check_match_grid(hip_backend)["compared"] == 16385


@pytest.mark.parametrize("words", sorted(K.ENVELOPE))
def test_match_at_the_lds_envelope(words, hip_backend):
    rep = K.check_envelope(hip_backend, words)
    print(rep)
    assert rep["compared"] > 150 and rep["hits"] > 50 and rep["abundance"] > 20


def test_whole_chain_on_the_default_and_a_worker_stream(hip_backend):
    rep = K.check_chain(hip_backend)
    print(rep)
    assert rep["streams"] == 2 and rep["reads"] == 3000 and rep["distinct"] < rep["kept"] and rep["hits"] > 100

"""The kernels of atropos_amd/csrc/stats_kernels.hip (atr_read_stats_batch, atr_read_stats_merge) at the C ABI, with
arguments of their own, against the plain Python model of tests/_stats_kernels_common.py: whole blocks between guard
words, word for word, exact -- reads on the edges of the 64-position windows and of the 1 024 length bins kept in LDS,
every byte on both paths of the two tables, groups of 64 reads with fewer than four left, intervals, masks and
destinations, records without qualities, ties of both roundings, first reads at ``index_base`` beyond 2^32, the
grid-stride trips of both kernels, ``longest`` below the longest read, merges at an offset, 64-bit carries, a worker
stream.  tests/test_stats_kernels_host.py runs the same checks on the CPU twin and asserts, from the model alone, that
the cases are not hollow."""
import pytest

from . import _stats_kernels_common as S

pytestmark = pytest.mark.gpu


def test_length_edges(hip_backend):
    rep = S.check_length_edges(hip_backend)
    print({k: v for k, v in rep.items() if k != "groups"})
    assert rep["reads"] == 2 * 485 + 6 and rep["words"] == 4 * S.offsets(2049)["words"] + S.offsets(4096)["words"]
    assert rep["other_seq"] >= 5000 and rep["out_q"] >= 10000 and rep["long_bins"] >= 19 and {1, 2, 3, 5} <= set(rep["groups"])


def test_intervals_masks_destinations(hip_backend):
    rep = S.check_intervals(hip_backend)
    print(rep)
    assert rep["masked_inside"] >= 2000 and rep["gc_moved"] >= 100 and rep["reads"] >= 22 * 700


def test_records_without_qualities(hip_backend):
    rep = S.check_no_qualities(hip_backend)
    print(rep)
    assert rep["no_qual"] >= 100 and rep["withq"] >= 150


def test_rounding_ties(hip_backend):
    rep = S.check_rounding(hip_backend)
    print(rep)
    assert min(rep[k] for k in ("gc_down", "gc_up", "mq_down", "mq_up", "neg_down", "neg_up")) >= 8 and rep["non_ties"] >= 100


def test_first_seen_order(hip_backend):
    rep = S.check_first_seen(hip_backend)
    print(rep)
    assert rep["bins"] >= 80 and 4 * rep["many_groups"] >= 3 * rep["bins"] and 4 * rep["many_blocks"] >= 3 * rep["bins"]
    assert rep["late_first"] >= 40 and rep["reads"] == 12 * S.ORDER_READS


def test_grid_stride_many_reads(hip_backend):
    rep = S.check_stride_many_reads(hip_backend)
    print(rep)
    assert rep["reads"] == 786689 and rep["blocks"] == 3074


def test_grid_stride_long_reads(hip_backend):
    rep = S.check_stride_long_reads(hip_backend)
    print(rep)
    assert rep["reads"] == 16705 and rep["long"] == 40 and rep["second_trip"] == 20 and rep["windows"] == 49


def test_skipped_and_longest(hip_backend):
    rep = S.check_bounds(hip_backend)
    print(rep)
    assert all(rep["skipped"][b] >= 50 for b in S.LONGEST_BOUNDS if b < 120) and rep["skipped"][128] == 0
    assert all(rep["exact"][b] >= 5 for b in S.LONGEST_BOUNDS if b <= 120)


def test_merge(hip_backend):
    rep = S.check_merge(hip_backend)
    print(rep)
    assert min(rep["both"] + rep["src_only"] + rep["dst_only"]) >= 5 and rep["b_wins"] >= 5 and rep["reads"] == 6000


def test_wide_words(hip_backend):
    rep = S.check_wide_words(hip_backend)
    print(rep)
    assert rep["carried"] >= 200


def test_worker_stream_twice_into_one_block(hip_backend):
    rep = S.check_intervals(hip_backend, worker=True)
    print(rep)
    assert rep["stream"] == "worker" and rep["reads"] == 2 * 7 * 700

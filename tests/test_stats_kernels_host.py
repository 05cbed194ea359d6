"""The checks of tests/test_gpu_stats_kernels.py on the CPU twin (tests/emu/emu_stats.cpp): the twin restates the
kernels' counting, so here it is pinned, block for block, to the plain Python model of
tests/_stats_kernels_common.py, and the model and the case builders stay verified without a GPU.  What keeps a case from
being hollow is asserted here from the model alone, so it holds wherever the GPU tier runs."""
import os
import subprocess

import numpy as np
import pytest

from . import _pairtext_common as P
from . import _stats_kernels_common as S


@pytest.fixture(scope="module")
def twin():
    return P.PairTextEmuBackend()


def test_model_layout_and_rounding():
    """The restated layout against the library's block size; the restated division against Python's own round."""
    for L in (1, 4, 16, 128, 150, 256, 1024, 2049, 4096):
        assert S.offsets(L)["words"] == 8 + (L + 1) + 101 + 256 + 2 * 256 * L + (L + 1) + 101 + 256
        assert int(S.additive(L).sum()) == S.offsets(L)["words"] - 1 - (L + 1 + 101 + 256)
    assert [S.round_half_even(100 * g, 8) for g in (1, 3, 5, 7)] == [12, 38, 62, 88]
    assert [S.round_half_even(n, 2) for n in (-1, -3, -5)] == [0, -2, -2]
    for den in (1, 2, 3, 4, 7, 8, 200, 2049):
        for num in range(-3 * den, 3 * den + 1):
            assert S.round_half_even(num, den) == round(num / den), (num, den)
    # the model itself on two reads written out by hand: ACGN / "!I~\x7f" and an empty one, index_base 5
    block = S.model_batch(S.new_block(4), 4, 4, 33, b"ACGN!I~\x7f", [[0, 0, 0, 4, 4, 4, 0, 0], [0, 0, 0, 0, 4, 0, 0, 0]], index_base=5)
    o = S.offsets(4)
    assert block[:4] == [2, 4, 1, 0] and block[o["len"]:o["gc"]] == [1, 0, 0, 0, 1]
    assert block[o["gc"] + 50] == 1 and block[o["mq"] + 33 + round((0 + 40 + 93 + 94) / 4)] == 1
    assert [block[o["seq"] + 256 * p + c] for p, c in enumerate(b"ACGN")] == [1] * 4 and block[o["qual"] + 256 * 3 + 127] == 1
    assert block[o["first"] + 4] == 2 ** 64 - 1 - 5 and block[o["first"]] == 2 ** 64 - 1 - 6 and block[o["first_gc"] + 50] == 2 ** 64 - 6
    assert sum(block) == 2 + 4 + 1 + 2 + 1 + 1 + 4 + 4 + 2 * (2 ** 64 - 6) + 2 ** 64 - 7 + 2 ** 64 - 6


def test_length_edges(twin):
    rep = S.check_length_edges(twin)
    assert rep["reads"] == 2 * 485 + 6 and rep["words"] == 4 * S.offsets(2049)["words"] + S.offsets(4096)["words"]
    assert rep["other_seq"] >= 5000 and rep["out_q"] >= 10000 and rep["long_bins"] >= 19 and {1, 2, 3, 5} <= set(rep["groups"])


def test_intervals_masks_destinations(twin):
    rep = S.check_intervals(twin)
    assert rep["masked_inside"] >= 2000 and rep["gc_moved"] >= 100 and rep["reads"] >= 22 * 700
    assert {k for k in S.interval_case()["kinds"]} == set(S.MASK_KINDS)


def test_records_without_qualities(twin):
    rep = S.check_no_qualities(twin)
    assert rep["no_qual"] >= 100 and rep["withq"] >= 150


def test_rounding_ties(twin):
    rep = S.check_rounding(twin)
    assert min(rep[k] for k in ("gc_down", "gc_up", "mq_down", "mq_up", "neg_down", "neg_up")) >= 8 and rep["non_ties"] >= 100


def test_first_seen_order(twin):
    rep = S.check_first_seen(twin)
    assert rep["bins"] >= 80 and 4 * rep["many_groups"] >= 3 * rep["bins"] and 4 * rep["many_blocks"] >= 3 * rep["bins"]
    assert rep["late_first"] >= 40 and rep["reads"] == 12 * S.ORDER_READS


def test_grid_stride_many_reads(twin):
    rep = S.check_stride_many_reads(twin)
    assert rep["reads"] == 786689 and rep["blocks"] == 3074


def test_grid_stride_long_reads(twin):
    rep = S.check_stride_long_reads(twin)
    assert rep["reads"] == 16705 and rep["long"] == 40 and rep["second_trip"] == 20 and rep["windows"] == 49


def test_skipped_and_longest(twin):
    rep = S.check_bounds(twin)
    assert all(rep["skipped"][b] >= 50 for b in S.LONGEST_BOUNDS if b < 120) and rep["skipped"][128] == 0
    assert all(rep["exact"][b] >= 5 for b in S.LONGEST_BOUNDS if b <= 120)


def test_merge(twin):
    rep = S.check_merge(twin)
    assert min(rep["both"] + rep["src_only"] + rep["dst_only"]) >= 5 and rep["b_wins"] >= 5 and rep["reads"] == 6000


def test_wide_words(twin):
    assert S.check_wide_words(twin)["carried"] >= 200


def test_twice_into_one_block(twin):
    """The stream check's arithmetic on the twin (it has no streams): every call twice into its block."""
    rep = S.check_intervals(twin, worker=True)
    assert rep["stream"] == "default" and rep["reads"] == 2 * 7 * 700


def test_numpy_model_is_the_plain_model():
    """tests/test_stats_host.py's numpy model, which serves at size, on a ragged case with every byte."""
    from .test_stats_host import empty_counts, matrices, model_counts
    case = S.bound_case()
    reads = [(case["data"][r[2]:r[2] + r[3]], case["data"][r[4]:r[4] + r[5]]) for r in case["recs"]]
    acc = empty_counts(130)
    acc["next"] = 1 << 33
    got = S.block_of_counts(model_counts(*matrices(reads), quality_base=64, acc=acc), 130)
    assert np.array_equal(got, S.as_words(S.model_case(case, 130, 130, 64, intervals=False, index_base=1 << 33)))


# ---------------------------------------------------------------------------------------------- the stand-alone driver
def test_fuzz_driver_under_the_sanitizers(tmp_path):
    """tests/emu/stats_fuzz_main.cpp: the twin and stats_core.hpp over random records, intervals, masks and merges, as a
    program of its own with -fsanitize=address,undefined (nothing of it is loaded into Python)."""
    from tests.emu import backend as emu
    exe = str(tmp_path / "stats_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DATR_HOST_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + emu._INC + [os.path.join(emu._HERE, "stats_fuzz_main.cpp"),
                                                                      os.path.join(emu._HERE, "emu_stats.cpp"), "-o", exe])
    out = subprocess.run([exe, "150", "11"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    assert b"ok: 150 rounds" in out.stdout

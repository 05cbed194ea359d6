"""The checks of tests/test_gpu_detect_kernels.py on the CPU twin (tests/emu/emu_detect.cpp): the Python model and the
case builders of tests/_detect_kernels_common.py stay verified without a GPU, and what keeps a case from being hollow
is asserted here from the model alone, so it holds wherever the GPU tier runs."""
import os
import subprocess

import numpy as np
import pytest

from . import _detect_common as DC
from . import _detect_kernels_common as K


@pytest.fixture(scope="module")
def twin():
    return DC.DetectEmuBackend()


@pytest.mark.parametrize("i", range(len(K.FILTER_HANDLES)))
def test_filter_cases_are_not_hollow(i):
    case = K.filter_case(i)
    c = K.assert_filter_conditions(case)
    past, k, lens, max_len = K.FILTER_HANDLES[i]
    lengths = {len(s) for s in case["reads"]}
    assert {0, 1, k - 1, k, min(lens) - 1, min(lens), 63, 64, 65, max_len} <= lengths
    assert max(lengths) == max_len and (max_len < 320 or {127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320} <= lengths)
    assert 1400 <= c["reads"] <= 2000
    # a read on either side of the length tests that the complexity test let through; every run at every boundary
    rows = list(zip(case["reads"], case["kept"], case["how"]))
    assert any(len(s) == max(k, min(lens)) and kl == len(s) for s, kl, _ in rows)
    assert any(len(s) == max(k, min(lens)) - 1 and how != "low" for s, _, how in rows)
    for b in past:
        for run in K.RUNS:
            for bnd in K.BOUNDARIES:
                for o in range(9):                                  # the run starts o bases in front of the boundary
                    at = bnd - o
                    if at + run + 1 <= max_len:
                        assert any(s[at:at + run] == b * run and s[at - 1] != b and len(s) > at + run and s[at + run] != b
                                   for s in case["reads"]), (b, run, bnd, o)


@pytest.mark.parametrize("i", range(len(K.FILTER_HANDLES)))
def test_filter_kept_and_hashes_per_read(i, twin):
    rep = K.check_filter(twin, i)
    assert rep["compared"] == sum(K.FILTER_SLICES) + rep["reads"]


def test_filter_second_grid_trip_and_error_paths(twin):
    assert K.check_filter_grid(twin)["compared"] == 16385
    assert K.check_filter_errors(twin) == dict(refused=3, overlong=2)


@pytest.mark.parametrize("m", K.MARK_SIZES)
def test_mark_hand_built_runs(m, twin):
    rep = K.check_mark(twin, m)
    assert rep["compared"] == m
    if m >= 257:
        assert rep["longest_run"] == 257 and rep["crossing"] >= 1
    if m >= 63:
        assert rep["collided"] > 0 and rep["distinct"] < m


def test_mark_cases_cover_the_runs():
    case = K.mark_case(3000)
    assert {n for _, n in case["runs"]} >= set(K.MARK_RUNS)
    assert any(at % 256 and n == 257 for at, n in case["runs"]) and case["crossing"] >= 6
    assert sorted(case["order"]) != case["order"] and len(set(case["order"])) == 3000
    assert 0 < sum(case["rep"]) < 3000 and case["collided"] > 500
    # the model itself on a run written out by hand: head, copy, other, copy of other behind the cut, shorter, copy
    keys = ["ACGT", "ACGT", "ACGA", "ACGA", "ACG", "ACGT", "TTTT", "TTTT"]
    assert K.model_rep(keys, [0, 0, 0, 0, 0, 0, 6, 6]) == [1, 0, 1, 0, 1, 0, 1, 0]


@pytest.mark.parametrize("name", sorted(K.MATCH_CASES))
def test_match_counters(name, twin):
    rep = K.check_match(twin, name)
    k = K.MATCH_CASES[name][1]
    assert rep["compared"] == sum(K.match_case(name)["rep"]) and rep["lengths"][0] >= k
    if K.MATCH_CASES[name][3] == 257:
        assert rep["abundance"] > 0 and rep["lengths"][-1] == 320 and len(rep["lengths"]) > 20
        assert {63, 64, 65, 192, 256, 257, 319, 320} <= set(rep["lengths"])
    if name in ("w1_k12", "w4_k12", "k12_list_one", "iupac_k16", "mixed_k21"):
        assert rep["lost_abundance"] > 0              # a known sequence whose last base fell behind the past-end cut


def test_match_cases_cover_the_bit_set_widths_and_alphabets():
    assert [K.match_case(n)["words"] for n in ("w1_k12", "w2_k12_frac0", "w3_k12_frac1", "w4_k12")] == [1, 2, 3, 4]
    assert K.match_case("w3_k12_frac1")["thresholds"] == [-1] * 4 and -1 in K.match_case("k4_list_never")["thresholds"]
    assert sorted({K.MATCH_CASES[n][1] for n in K.MATCH_CASES if K.MATCH_CASES[n][0].startswith("w")}) == [4, 8, 12, 16, 32]
    assert sorted({K.MATCH_CASES[n][3] for n in K.MATCH_CASES}) == [1, 4, 5, 257]
    for name, letters in (("n", 6), ("mixed", 8), ("iupac", 15), ("w4", 4)):
        used = set("".join(K.KNOWN_SETS[name]))
        assert len(used | {K.COMP[c] for c in used if c in K.COMP}) == letters
    half = K.KNOWN_SETS["special"][0]
    assert half == K.revcomp(half) and K.KNOWN_SETS["special"][1][:20] == K.KNOWN_SETS["special"][2][:20]


def test_match_refused_k_invalid_read_and_second_grid_trip(twin):
    assert K.check_refused_k(twin) == 5
    assert K.check_invalid(twin) == 1
    assert K.check_match_grid(twin)["compared"] == 16385


@pytest.mark.parametrize("words", sorted(K.ENVELOPE))
def test_match_at_the_lds_envelope(words, twin):
    rep = K.check_envelope(twin, words)
    assert rep["compared"] > 150 and rep["hits"] > 50 and rep["abundance"] > 20


def test_whole_chain_twice_into_one_block(twin):
    rep = K.check_chain(twin)
    assert rep["reads"] == 3000 and rep["distinct"] < rep["kept"] and rep["hits"] > 100 and rep["abundance"] > 50


def test_python_counters_modes_agree():
    """The three ways to call the moved restatement give one answer where they overlap."""
    case = K.chain_case()
    items = [(s, None) for s in case["seqs"]]
    regexp = K.past_end_regexp(K.MATCH_PAST)
    kept = {r[:kl] for r in case["reads"] for kl in [K.model_kept(r, 12, 12, regexp)[0]] if kl}
    n, out, invalid = K.python_counters(None, items, 12, (), thresholds=case["thresholds"], representatives=sorted(kept),
                                        count_invalid=True)
    assert n == case["distinct"] and invalid == 0 and np.array_equal(out, case["want"])
    with pytest.raises(KeyError):
        K.python_counters(["ACGTTGCAGGATCCATXGACTGACCATGGTACA"], items, 12, ("A",), 0.5)
    assert K.python_counters(["ACGTTGCAGGATCCATGGACTGACCATGGTACAAA"], items, 12, (), 0.5)[0] == 1


# ---------------------------------------------------------------------------------------------- the stand-alone driver
def test_fuzz_driver_under_the_sanitizers(tmp_path):
    """tests/emu/detect_fuzz_main.cpp: the twin and detect_core.hpp over random handles and reads, as a program of its
    own with -fsanitize=address,undefined (nothing of it is loaded into Python)."""
    from tests.emu import backend as emu
    exe = str(tmp_path / "detect_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DATR_HOST_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + emu._INC + [os.path.join(emu._HERE, "detect_fuzz_main.cpp"),
                                                                      os.path.join(emu._HERE, "emu_detect.cpp"), "-o", exe])
    out = subprocess.run([exe, "120", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    assert b"ok: 120 rounds" in out.stdout

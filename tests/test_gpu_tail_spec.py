"""The run-time compiled DP tail (csrc/tail_filter.hpp, tail_spec.hip): ONE launch behind the specialised pre-pass --
window blocks first, band blocks behind them -- in place of the band_kernel || window_kernel pair.  Records with
ATR_TAIL_SPEC=1 == records with ATR_TAIL_SPEC=0 == the oracle, for every read: three aligners, equal-length (150 and
97 bases: a partial last word) and ragged (100 .. 150) plane64 batches of 65 536 reads from C2's generator and from
each of synth.HARD_KINDS (nearly every read a tail task, every band-width bin filled), a hand-built batch (window
reads, every band class, last-column bands of every width, and batches without any task), and 64 / 65 / 8 193 reads
(a partial last wave, the boundary of the tasks-per-wave rule)."""
import glob
import os
import random

import numpy as np
import pytest

from ._cases import rseq
from ._overlap_a_common import TRUSEQ

pytestmark = pytest.mark.gpu

NREADS = 65536
ALIGNERS = [(TRUSEQ, 0.1, 3),                 # C2's: k = 3
            (TRUSEQ, 0.12, 3),                # k = 4, 48-column windows
            (TRUSEQ[:20], 0.1, 3)]            # a 20-mer, indel cost 1, min_overlap 3
AIDS = ["truseq_e10", "truseq_e12", "mer20"]
SHAPES = ["n150", "n97", "ragged100_150"]
INPUTS = ["C2", "edits", "partial", "lowcomplex"]
_READS = {}
_COMPILED = set()


def shaped(mat, shape, seed):
    """150-base rows -> (matrix or list of rows, lens): the last 97 bases, or the last 100 .. 150."""
    if shape == "n150":
        return mat, np.full(len(mat), 150, np.int32)
    if shape == "n97":
        return np.ascontiguousarray(mat[:, -97:]), np.full(len(mat), 97, np.int32)
    lens = np.random.RandomState(seed).randint(100, 151, len(mat)).astype(np.int32)
    out = np.zeros_like(mat)
    for L in range(100, 151):
        rows = np.nonzero(lens == L)[0]
        out[rows, :L] = mat[rows, 150 - L:]
    return out, lens


def reads_of(ai, kind, shape, count=NREADS):
    from atropos_amd import synth
    key = (ALIGNERS[ai][0], kind, shape, count)
    if key not in _READS:
        if kind == "C2":
            mat = synth.workload("C2", 7 * NREADS, count)["reads"].numpy()
        else:
            mat = synth.hard_batch(kind, 3 * NREADS, count, adapter=ALIGNERS[ai][0]).numpy()
        _READS[key] = shaped(mat, shape, 17)
    return _READS[key]


def records(res):
    return res.numpy()[:, :6].astype(np.int32)


def check(monkeypatch, tmp_path, ai, mat, lens, ragged):
    """generic pair == specialised tail == oracle on (mat, lens); the pre-pass object must carry the tail kernel."""
    from atropos_amd.align import Aligner
    from oracle import oracle as O
    ref, e, mo = ALIGNERS[ai]
    n = mat.shape[1]
    exp = O.locate_many(ref, mat, lens, e, 14, False, False, mo, 1, max(2, min(16, os.cpu_count() or 2)))
    cache = tmp_path / "kcache"
    monkeypatch.setenv("ATR_KCACHE_DIR", str(cache))
    monkeypatch.setenv("ATR_JIT", "1")
    # a compile option of this module's own (part of the object's key): whatever the process has compiled for the same
    # adapter before, the first handle of a shape here compiles anew and leaves its object in `cache`
    monkeypatch.setenv("ATR_SPEC_FLAGS", "-DATR_TEST_TAIL_SPEC_OBJECTS=1")
    al = Aligner(ref, e, 14, False, False, mo, 1)
    rows = [bytes(mat[r, :lens[r]]).decode() for r in range(len(mat))] if ragged else mat
    planes = al.pack(rows, layout="plane64")
    assert planes.layout == "plane64" and (planes.lens is not None) == ragged
    assert al.prepare(n, ragged=ragged), "no specialised kernel (hiprtc?)"
    objs = glob.glob(str(cache / "*.hsaco"))
    if (ai, (n + 31) // 32, ragged) not in _COMPILED:       # (later handles find the object in the process's table)
        assert objs, "no code object in the cache directory"
        _COMPILED.add((ai, (n + 31) // 32, ragged))
    assert all(b"atr_tail_spec" in open(f, "rb").read() for f in objs), "a pre-pass object without its tail kernel"
    monkeypatch.setenv("ATR_TAIL_SPEC", "0")
    off = records(al.locate_batch(planes))
    monkeypatch.setenv("ATR_TAIL_SPEC", "1")
    on = records(al.locate_batch(planes))
    assert np.array_equal(off, exp), "generic band / window pair"
    bad = np.nonzero((on != exp).any(axis=1))[0]
    assert bad.size == 0, "specialised tail: %d reads differ, first %d: %s != %s" % (bad.size, bad[0], on[bad[0]], exp[bad[0]])
    return exp


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ai", range(len(ALIGNERS)), ids=AIDS)
def test_tail_equals_generic_and_oracle(hip_backend, oracle, tmp_path, monkeypatch, ai, shape, kind):
    mat, lens = reads_of(ai, kind, shape)
    exp = check(monkeypatch, tmp_path, ai, mat, lens, shape.startswith("ragged"))
    assert (exp[:, 1] >= 0).sum() > NREADS // 8


def hand_built(rng, ref, k, n=150):
    """Window reads, band reads of every width class, last-column bands of 4 .. 16 diagonals."""
    m = len(ref)
    other = lambda c: rng.choice([x for x in "ACGT" if x != c])
    reads = []

    def put(q):
        reads.append((rseq(rng, n) + q)[-n:])

    def edited(s, subs=0, ins=0, dels=0, lo=1, hi=None):
        s = list(s)
        for _ in range(subs):
            at = rng.randrange(lo, (hi or len(s)) - 1)
            s[at] = other(s[at])
        for _ in range(ins):
            s.insert(rng.randrange(lo, (hi or len(s)) - 1), rng.choice("ACGT"))
        for _ in range(dels):
            del s[rng.randrange(lo, min(hi or len(s), len(s)) - 1)]
        return "".join(s)

    for _ in range(40):
        # the window reads: the adapter ends 0 .. k columns before the read end, one error in it
        for t in range(k + 1):
            put(edited(ref, subs=1) + rseq(rng, t))
            put(edited(ref, ins=1) + rseq(rng, t))
            put(edited(ref, dels=1) + rseq(rng, t))
        # row-m band reads, 8 .. 16 diagonals: the whole adapter inside the read with 0 .. k edits of every kind, and a
        # second, shifted copy next to it (a wider span of candidate diagonals)
        for e in range(k + 1):
            for ins in range(e + 1):
                for dels in range(e + 1 - ins):
                    put(edited(ref, subs=e - ins - dels, ins=ins, dels=dels) + rseq(rng, rng.randint(k + 1, 60)))
        for shift in range(1, 9):
            put(ref + ref[-shift:] + rseq(rng, rng.randint(k + 1, 40)))
            put(edited(ref, subs=1) + ref[m - shift:] + rseq(rng, rng.randint(k + 1, 40)))
        # last-column band reads: a prefix of every length at the read end with 0 .. its allowed errors, indels included
        # (cost + 2 k' + 1 diagonals: 4 .. 16)
        for i in range(4, m):
            e = rng.randint(0, max(0, int(i * (k + 0.5) / m)))
            ins = rng.randint(0, e)
            dels = rng.randint(0, e - ins)
            if i > 6:
                put(edited(ref[:i], subs=e - ins - dels, ins=ins, dels=dels, lo=1, hi=i))
            else:
                put(ref[:i])
        # ... and with row-m candidates besides: the adapter up to k columns before the end, the read ending in its start
        for t in range(1, k + 1):
            put(edited(ref, subs=rng.randint(0, 1)) + ref[:t])
    rng.shuffle(reads)
    mat = np.zeros((len(reads), n), np.uint8)
    for r, q in enumerate(reads):
        mat[r] = np.frombuffer(q.encode(), np.uint8)
    return mat


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ai", range(len(ALIGNERS)), ids=AIDS)
def test_hand_built_classes(hip_backend, oracle, tmp_path, monkeypatch, ai, shape):
    ref, e, _ = ALIGNERS[ai]
    mat = hand_built(random.Random(41 + ai), ref, int(len(ref) * e))
    mat, lens = shaped(mat, shape, 5)
    exp = check(monkeypatch, tmp_path, ai, mat, lens, shape.startswith("ragged"))
    assert (exp[:, 1] >= 0).sum() > len(mat) // 2 and (exp[:, 5] > 0).sum() > len(mat) // 8


@pytest.mark.parametrize("ai", range(len(ALIGNERS)), ids=AIDS)
def test_no_tasks_at_all(hip_backend, oracle, tmp_path, monkeypatch, ai):
    """Every read resolved by the pre-pass (no base that matches anything): zero band tasks, zero window tasks."""
    mat = np.full((4096 + 11, 150), ord("N"), np.uint8)
    exp = check(monkeypatch, tmp_path, ai, mat, np.full(len(mat), 150, np.int32), False)
    assert (exp[:, 1] < 0).all()


@pytest.mark.parametrize("count", [64, 65, 8193])
@pytest.mark.parametrize("kind", ["C2", "edits", "partial"])
def test_small_batches(hip_backend, oracle, tmp_path, monkeypatch, kind, count):
    mat, lens = reads_of(0, kind, "n150", count)
    check(monkeypatch, tmp_path, 0, mat, lens, False)
    mat, lens = reads_of(0, kind, "ragged100_150", count)
    check(monkeypatch, tmp_path, 0, mat, lens, True)

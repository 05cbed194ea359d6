"""Pass A resolves a clean read-end overlap itself (piece_core.hpp: piece_overlap_word) -- the kernels.  The read
families of the CPU tier (tests/_overlap_a_common.py) in batches of 4096 + 37 reads (a partial last tile), at 3, 5 and 8
plane words and as a ragged batch, through the generic kernels and through a run-time compiled kernel per aligner, and
once through the fused ASCII entry: plane64 == tile64 path="full" == the oracle, for every read.

At this batch size the persistent grid gives every wave ONE tile, so a wave's queue fills only from a tile whose 64
reads all need pass B: the first two tiles of every batch are made of such reads (a substitution inside an overlap long
enough to allow one, chosen with the CPU twin: queued for pass B, not resolved by the rule), the others drain their
queue partially."""
import os
import random

import numpy as np
import pytest

from . import _overlap_a_common as X

pytestmark = pytest.mark.gpu

NREADS = 4096 + 37
ALIGNERS = [(X.TRUSEQ, 0.1, 3),                                    # C2's
            ("TCAGTTCAGTTCAGTTCCGTTCAGTTCA", 0.05, 3),             # periodic, one defect
            ("ATGAATCTCTGATTTACCCACTCTGCCAAACTCCA", 0.1, 5)]       # random, 35 bases: 32 swept rows + 3 tail rows
CASES = [(70, False), (150, False), (250, False), (150, True)]
_BATCHES = {}


def batch(ai, n, rg):
    """(reads, matrix or rows, oracle records), made once per aligner and shape."""
    key = (ai, n, rg)
    if key not in _BATCHES:
        from oracle import oracle as O
        ref, e, mo = ALIGNERS[ai]
        rng = random.Random(1000 * ai + n + rg)
        reads = X.overlap_reads(rng, ref, n, NREADS - 128)
        rng.shuffle(reads)
        cand = []
        for _ in range(600):                                      # pass-B reads: a substitution inside the overlap
            i = rng.randint(max(12, int(1 / e) + 2), len(ref) - 5)
            tail = list(ref[:i])
            at = rng.randrange(2, i - 2)
            tail[at] = rng.choice([c for c in "ACGT" if c != tail[at]])
            cand.append((X.rseq(rng, n) + "".join(tail))[-n:])
        if rg:                                                    # ragged: the last 100 .. 150 bases of every read
            cand = [q[len(q) - rng.randint(100, n):] for q in cand]
            reads = [q[len(q) - rng.randint(100, n):] for q in reads]
        _, _, ovl, st = X.scan(ref, e, 14, False, False, mo, 1, cand, n, rg, states=True)
        full = [q for q, i, s in zip(cand, ovl, st) if i == 0 and s & X.QUEUED][:128]
        assert len(full) == 128
        reads = full + reads
        lens = np.array([len(q) for q in reads], np.int32)
        mat = np.zeros((len(reads), n), np.uint8)
        for r, q in enumerate(reads):
            mat[r, :len(q)] = np.frombuffer(q.encode(), np.uint8)
        exp = O.locate_many(ref, mat, lens, e, 14, False, False, mo, 1, max(2, min(16, os.cpu_count() or 2)))
        _BATCHES[key] = (reads, reads if rg else mat, exp)
    return _BATCHES[key]


def records(res):
    return res.numpy()[:, :6].astype(np.int32)


@pytest.mark.parametrize("n,rg", CASES, ids=["n70", "n150", "n250", "ragged100_150"])
@pytest.mark.parametrize("ai", range(len(ALIGNERS)), ids=["truseq", "periodic", "random35"])
def test_generic_and_specialised(hip_backend, oracle, tmp_path, monkeypatch, ai, n, rg):
    from atropos_amd.align import Aligner
    ref, e, mo = ALIGNERS[ai]
    reads, mat, exp = batch(ai, n, rg)
    assert len(reads) == NREADS and (exp[:, 1] >= 0).sum() > 2000
    taken, word, ovl, st = X.scan(ref, e, 14, False, False, mo, 1, reads, n, rg, states=True)
    assert taken and word and (ovl > 0).sum() > 200               # (the rule has work in this batch; ~300 with the periodic adapter)
    # the first two tiles fill their wave's queue: 64 lanes queued for pass B each, none resolved in pass A
    assert not ovl[:128].any() and ((st[:128] & X.QUEUED) != 0).all() and (exp[:128, 1] >= 0).sum() > 100
    # ... and tiles behind them drain theirs partially
    q = ((st[128:4096] & X.QUEUED) != 0).reshape(-1, 64).sum(axis=1)
    assert ((q > 0) & (q < 64)).sum() > 50
    monkeypatch.setenv("ATR_KCACHE_DIR", str(tmp_path / "kcache"))
    al = Aligner(ref, e, 14, False, False, mo, 1)
    monkeypatch.setenv("ATR_JIT", "0")
    planes = al.pack(mat, layout="plane64")
    assert planes.layout == "plane64" and (planes.lens is not None) == rg
    gen = records(al.locate_batch(planes))
    tiles = al.pack(mat, layout="tile64")
    full = records(al.locate_batch(tiles, path="full"))
    assert np.array_equal(full, exp)
    assert np.array_equal(gen, exp), "generic kernel"
    monkeypatch.setenv("ATR_JIT", "1")
    assert al.prepare(n, ragged=rg), "no specialised kernel (hiprtc?)"
    got = records(al.locate_batch(planes))
    assert np.array_equal(got, exp), "run-time compiled kernel"


def test_fused_ascii_entry(hip_backend, oracle, tmp_path, monkeypatch):
    import torch
    from atropos_amd.align import Aligner
    ref, e, mo = ALIGNERS[0]
    reads, mat, exp = batch(0, 150, False)
    monkeypatch.setenv("ATR_KCACHE_DIR", str(tmp_path / "kcache"))
    monkeypatch.setenv("ATR_JIT", "1")
    al = Aligner(ref, e, 14, False, False, mo, 1)
    assert al.prepare(150), "no specialised kernel (hiprtc?)"
    res, left = al.locate_ascii(torch.from_numpy(mat).cuda(), None, 150)
    assert np.array_equal(records(res), exp)
    assert np.array_equal(records(al.locate_batch(left)), exp)                 # (the planes the fused kernel left behind)

"""Row-m band reads on the intersection of the hits' band and the pieces' band (filter_core.hpp: filter_decide_tm) and
pass A on two code planes (piece_core.hpp: piece_scan_spec) -- the kernels.  The read families of
tests/_band_planes_common.py in batches of 4096 + 37 reads (a partial last tile) at 3 and 5 plane words: the run-time
compiled kernel == the generic one (ATR_JIT=0) == tile64 path="full" == the oracle on every read, and the same with the
run-time compiled DP tail off (ATR_TAIL_SPEC=0) and with the four-mask pass A (ATR_SPEC_FLAGS=-DATR_PIECE_TWO_PLANES=0)."""
import os
import random

import numpy as np
import pytest

from . import _band_planes_common as X

pytestmark = pytest.mark.gpu

NREADS = 4096 + 37
_BATCHES = {}


def batch(ai, n):
    """(matrix, oracle records), made once per aligner and shape."""
    if (ai, n) not in _BATCHES:
        from oracle import oracle as O
        ref, e, mo = X.ALIGNERS[ai]
        rng = random.Random(500 * ai + n)
        mat = X.matrix(X.band_reads(rng, ref, int(len(ref) * e), n, NREADS), n)
        exp = O.locate_many(ref, mat, np.full(len(mat), n, np.int32), e, 14, False, False, mo, 1, max(2, min(16, os.cpu_count() or 2)))
        _BATCHES[(ai, n)] = (mat, exp)
    return _BATCHES[(ai, n)]


def records(res):
    return res.numpy()[:, :6].astype(np.int32)


@pytest.mark.parametrize("n", [70, 150], ids=["n70", "n150"])
@pytest.mark.parametrize("ai", range(len(X.ALIGNERS)), ids=X.IDS)
def test_specialised_generic_full_oracle(hip_backend, oracle, tmp_path, monkeypatch, ai, n):
    from atropos_amd.align import Aligner
    ref, e, mo = X.ALIGNERS[ai]
    mat, exp = batch(ai, n)
    assert len(mat) == NREADS and (exp[:, 1] >= 0).sum() > 2000
    monkeypatch.setenv("ATR_JIT", "0")
    al = Aligner(ref, e, 14, False, False, mo, 1)
    planes = al.pack(mat, layout="plane64")
    assert planes.layout == "plane64"
    assert np.array_equal(records(al.locate_batch(al.pack(mat, layout="tile64"), path="full")), exp), "tile64 full"
    assert np.array_equal(records(al.locate_batch(planes)), exp), "generic kernel"
    monkeypatch.setenv("ATR_JIT", "1")
    monkeypatch.setenv("ATR_KCACHE_DIR", str(tmp_path / "kcache"))
    monkeypatch.delenv("ATR_TAIL_SPEC", raising=False)
    # (the compile switches are part of the cache key: a fresh handle per build compiles its own kernel; ATR_TAIL_SPEC is
    #  read at every call and picks the generic band / window pair behind the same pre-pass)
    # (MINE: a define nothing reads.  The process keeps compiled kernels in memory under a key that includes the switches;
    #  with it these kernels stay apart from the ones a later test of the same process expects to compile and store itself)
    MINE = "-DATR_TEST_BAND_PLANES=1"
    for name, flags, tail in (("specialised", MINE, None), ("tail off", MINE, "0"), ("four masks", MINE + " -DATR_PIECE_TWO_PLANES=0", None)):
        monkeypatch.setenv("ATR_SPEC_FLAGS", flags)
        if tail is None:
            monkeypatch.delenv("ATR_TAIL_SPEC", raising=False)
        else:
            monkeypatch.setenv("ATR_TAIL_SPEC", tail)
        al2 = Aligner(ref, e, 14, False, False, mo, 1)
        assert al2.prepare(n), "no specialised kernel (hiprtc?)"
        got = records(al2.locate_batch(al2.pack(mat, layout="plane64")))
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert len(bad) == 0, (name, bad[:5], got[bad[:5]], exp[bad[:5]])

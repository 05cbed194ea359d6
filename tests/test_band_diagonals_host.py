"""The band of a row-m band read is the hits' band intersected with the pieces' band (filter_core.hpp: filter_decide_tm;
the pieces' diagonals travel with the pass-B task, piece_core.hpp: PieceTask) -- the CPU twin of the two-pass pre-pass
(tests/emu, the product's per-lane source) against the oracle on the read families of tests/_band_planes_common.py, and
the diagonal count the change is about on synthetic C2 reads."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from . import _band_planes_common as X

NREADS = 1500


def last_windows(be, n):
    win = np.zeros(n, np.uint32)
    be.lib.emu_piece_last_windows.restype = C.c_longlong
    assert be.lib.emu_piece_last_windows(win.ctypes.data_as(C.c_void_p), C.c_longlong(n)) == n
    return win


@pytest.mark.parametrize("n", [70, 150], ids=["n70", "n150"])
@pytest.mark.parametrize("ai", range(len(X.ALIGNERS)), ids=X.IDS)
def test_twin_equals_oracle(emu_backend, oracle, ai, n):
    from atropos_amd.align import Aligner
    ref, e, mo = X.ALIGNERS[ai]
    k = int(len(ref) * e)
    rng = random.Random(77 * ai + n)
    mat = X.matrix(X.band_reads(rng, ref, k, n, NREADS), n)
    exp = oracle.locate_many(ref, mat, np.full(len(mat), n, np.int32), e, 14, False, False, mo, 1, max(2, min(16, os.cpu_count() or 2)))
    al = Aligner(ref, e, 14, False, False, mo, 1)
    planes = al.pack(mat, layout="plane64")
    assert planes.layout == "plane64"
    got = al.locate_batch(planes).numpy()[:, :6].astype(np.int32)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], exp[bad[:5]], [bytes(mat[r]).decode() for r in bad[:2]])
    assert (exp[:, 1] >= 0).sum() > NREADS // 2
    # the batch has row-m band reads, some of them narrower than the 2 k + 1 + 2 (k - c) columns the hits alone give
    nd = X.band_diagonals(last_windows(emu_backend, len(mat)), len(ref), k)
    assert len(nd) > 50 and nd.min() >= 1 and nd.max() <= 16


def test_c2_row_m_bands_are_narrow(emu_backend):
    """20 000 synthetic C2 reads: the row-m band reads sweep 11.74 diagonals in the mean with the hits' band alone (the ND
    variant of band_locate their width selects: 8, 10, .. 16), 8.8 with the intersection.  The cap is a condition."""
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    n = 20000
    w = synth.workload("C2", 0, n)
    al = Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
    m = len(w["adapter"])
    k = int(m * w["max_error_rate"])
    al.locate_batch(al.pack(w["reads"], layout="plane64"))
    nd = X.band_diagonals(last_windows(emu_backend, n), m, k)
    variant = np.maximum(8, (nd + 1) // 2 * 2)
    print("row-m band reads %d of %d, mean diagonals %.2f, mean ND variant %.2f" % (len(nd), n, nd.mean(), variant.mean()))
    assert len(nd) > 500
    assert variant.mean() <= 9.5

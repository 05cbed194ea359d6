"""Pass A of the run-time compiled pre-pass on two code planes and one base mask (piece_core.hpp: piece_scan_spec) against
the generic pass A on four base masks (piece_scan), per read, on the CPU: tests/emu/emu_two_planes.cpp builds both from
the product's per-lane source under ATR_HOST_EMU, with the config header the library itself would generate for the aligner
(jit_config.hpp).  The form kept is the exact one -- a position without exactly one plane matches no code -- so the two
scans must be EQUAL on every read, clean or not (which is more than the superset relations a two-plane form with
aliasing would have to keep: flagged' >= flagged, ovl' in {ovl, 0}, j_exact' in {j_exact, 0}).  The same twin runs as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from . import _band_planes_common as X
from ._overlap_a_common import overlap_reads
from .conftest import ROOT

_SRC = os.path.join(ROOT, "tests", "emu", "emu_two_planes.cpp")
_FLAGS = ["-std=c++17", "-DATR_HOST_EMU", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "atropos_amd", "csrc")]
NREADS = 3000
J_EXACT, FLAGGED, OVL = 0, 3, 6


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    prog = str(tmp_path_factory.mktemp("two_gen") / "emu_two_gen")
    subprocess.check_call(["g++", "-O0", "-DEMU_TWO_GEN"] + _FLAGS + [_SRC, "-o", prog])
    return prog


def config_dir(gen, tmp_path, ref, e, mo, n):
    d = str(tmp_path)
    subprocess.check_call([gen, ref, repr(e), "14", str(mo), str(n), d])
    return d


@pytest.mark.parametrize("n", [70, 150, 160], ids=["n70", "n150", "n160"])
@pytest.mark.parametrize("ai", range(len(X.ALIGNERS)), ids=X.IDS)
def test_equals_four_masks(gen, tmp_path, ai, n):
    ref, e, mo = X.ALIGNERS[ai]
    k = int(len(ref) * e)
    cfg = config_dir(gen, tmp_path, ref, e, mo, n)
    so = str(tmp_path / "libemu_two_planes.so")
    subprocess.check_call(["g++", "-O1", "-fPIC", "-shared", "-DATR_SPEC=1", "-I" + cfg] + _FLAGS + [_SRC, "-o", so])
    lib = C.CDLL(so)
    lib.emu_two_planes_scan.restype = C.c_longlong
    lib.emu_two_planes_scan.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    assert lib.emu_two_planes_n() == n and lib.emu_two_planes_on() == 1
    rng = random.Random(31 * ai + n)
    reads = X.band_reads(rng, ref, k, n, NREADS) + overlap_reads(rng, ref, n, NREADS // 2)
    for a in range(10):                                             # A-runs at positions 0 .. 9 in front of the adapter verbatim
        for dirty in ("", "N", "R"):
            q = list(X.rseq(rng, n))
            q[:a + 1] = "A" * (a + 1)
            q[a + 1:a + 1 + len(ref)] = list(ref)
            for c in dirty:                                         # inside, next to, before and after the adapter
                for at in (a + 1 + rng.randrange(len(ref)), a, a + 1 + len(ref), rng.randrange(a + 1), n - 1):
                    qq = list(q)
                    qq[at] = c
                    reads.append("".join(qq[:n]))
            reads.append("".join(q[:n]))
    mat = X.matrix(reads, n)
    g, s = np.zeros((len(mat), 7), np.int32), np.zeros((len(mat), 7), np.int32)
    bad = lib.emu_two_planes_scan(ref.encode(), len(ref), e, 14, mo, mat.ctypes.data, n, len(mat), g.ctypes.data, s.ctypes.data)
    assert bad >= 0, "the twin was built for another aligner"
    dirty = np.array([any(c not in "ACGT" for c in q) for q in reads])
    diff = np.nonzero((g != s).any(axis=1))[0]
    assert len(diff) == 0 and bad == 0, (diff[:5], g[diff[:5]], s[diff[:5]], [reads[r] for r in diff[:2]])
    # the relations a two-plane form must keep on dirty reads at the least (implied by equality; said on their own)
    assert (s[dirty, FLAGGED] >= g[dirty, FLAGGED]).all()
    assert ((s[dirty, OVL] == g[dirty, OVL]) | (s[dirty, OVL] == 0)).all()
    assert ((s[dirty, J_EXACT] == g[dirty, J_EXACT]) | (s[dirty, J_EXACT] == 0)).all()
    # non-vacuity: verbatim, resolved-overlap, flagged and unflagged reads, clean and dirty
    assert dirty.sum() > 300 and (~dirty).sum() > 1000
    for sel in (dirty, ~dirty):
        assert (g[sel, J_EXACT] != 0).sum() > 20 and (g[sel, FLAGGED] != 0).sum() > 100 and (g[sel, FLAGGED] == 0).sum() > 20
    assert (g[:, OVL] != 0).sum() > 50


def test_standalone_under_sanitizers(gen, tmp_path):
    ref, e, mo = X.ALIGNERS[0]
    cfg = config_dir(gen, tmp_path, ref, e, mo, 150)
    prog = str(tmp_path / "emu_two_planes")
    subprocess.check_call(["g++", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DATR_SPEC=1",
                           "-DEMU_TWO_MAIN", "-I" + cfg] + _FLAGS + [_SRC, "-o", prog])
    run = subprocess.run([prog, ref, repr(e), "14", str(mo), "20000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = run.stderr.decode("utf-8", "replace")
    assert run.returncode == 0, (run.stdout.decode()[-500:], err[-2000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-2000:]
    assert "two planes on" in run.stdout.decode()

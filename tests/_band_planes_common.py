"""Shared by test_band_diagonals_host.py (the CPU twin of the two-pass pre-pass), test_two_planes_host.py (the twin of the
run-time compiled pass A) and test_gpu_band_planes.py (the kernels): the aligners and the read families that press on
the band of a row-m band read (filter_core.hpp: filter_decide_tm, the hits' band intersected with the pieces' band) and
on pass A's two code planes (piece_core.hpp: piece_scan_spec)."""
import numpy as np

from ._cases import rseq
from ._overlap_a_common import TRUSEQ

ALIGNERS = [(TRUSEQ, 0.1, 3),                                      # C2's
            ("TCAGTTCAGTTCAGTTCCGTTCAGTTCA", 0.05, 3),             # periodic, one defect
            ("ATGAATCTCTGATTTACCCACTCTGCCAAACTCCA", 0.1, 5)]       # random, 35 bases: 32 swept rows + 3 tail rows
IDS = ["truseq", "periodic", "random35"]
DIRTY = "NRYKMSWBDHVn."                                            # what a read may hold besides A C G T


def edited(rng, ref, errors):
    """The adapter with `errors` edit operations at distinct places: substitutions, insertions, deletions."""
    s = list(ref)
    for at in sorted(rng.sample(range(1, len(ref) - 1), errors), reverse=True):
        v = rng.random()
        if v < 0.5:
            s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
        elif v < 0.75:
            del s[at]
        else:
            s.insert(at, rng.choice("ACGT"))
    return "".join(s)


def band_reads(rng, ref, k, n, count):
    """Reads of n bases with the whole adapter: verbatim, one substitution, one insertion or deletion, two errors, three
    errors; anywhere, starting at columns 0 .. k (the clamped first diagonal), ending at n or within k of n (the window cut
    at the read end); with a chance second copy of a piece elsewhere (wide d_min .. d_max); with N or another code inside,
    next to, before and after the adapter; with runs of A at the read start."""
    m = len(ref)
    reads = []
    while len(reads) < count:
        t = len(reads)
        errors = (0, 1, 1, 2, 3)[t % 5]
        ad = edited(rng, ref, errors) if errors else ref
        if t % 5 == 2:                                             # one indel
            at = rng.randrange(1, m - 1)
            ad = ref[:at] + (rng.choice("ACGT") + ref[at:] if rng.random() < 0.5 else ref[at + 1:])
        where = (t // 5) % 4
        if where == 0:
            start = rng.randint(0, max(0, n - len(ad)))
        elif where == 1:
            start = rng.randint(0, k)                              # columns 0 .. k
        elif where == 2:
            start = n - len(ad) - rng.randint(0, k)                # ends at n, or within k of it
        else:
            start = n - len(ad) + rng.randint(1, 6)                # runs over the read end
        start = max(0, start)
        q = list(rseq(rng, n))
        q[start:start + len(ad)] = list(ad)
        q = q[:n]
        v = (t // 20) % 5
        if v == 1:                                                 # a chance second copy of a piece elsewhere
            L, a = rng.randint(8, 10), rng.randrange(0, m - 10)
            at = rng.choice([rng.randint(0, n - L), max(0, start - rng.randint(L, L + 12)), min(n - L, start + len(ad) + rng.randint(0, 12))])
            if at + L <= start or at >= start + len(ad):
                q[at:at + L] = list(ref[a:a + L])
        elif v == 2:                                               # N (or another code) inside / next to / before / after
            at = rng.choice([start + rng.randrange(len(ad)), start - 1, start + len(ad), rng.randrange(n), start - rng.randint(2, 9)])
            if 0 <= at < n:
                for x in range(at, min(n, at + rng.choice([1, 1, 2, 4]))):
                    q[x] = rng.choice(DIRTY)
        elif v == 3:                                               # a run of A at the read start
            for x in range(rng.randint(1, 10)):
                if x < start or rng.random() < 0.2:
                    q[x] = "A"
        reads.append("".join(q[:n]))
    return reads


def matrix(reads, n):
    mat = np.zeros((len(reads), n), np.uint8)
    for r, q in enumerate(reads):
        assert len(q) == n
        mat[r] = np.frombuffer(q.encode(), np.uint8)
    return mat


def band_diagonals(win, m, k):
    """The diagonal counts of the row-m band reads among the window words `win` (filter_core.hpp: window_word)."""
    win = np.asarray(win, np.uint32)
    sel = ((win >> 31) != 0) & (((win >> 28) & 1) != 0) & (((win >> 20) & 1) == 0)
    lo, hi = (win & 1023).astype(np.int64), ((win >> 10) & 1023).astype(np.int64)
    return (hi - lo - m + k + 1)[sel]

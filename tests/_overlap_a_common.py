"""Shared by test_overlap_pass_a_host.py (the CPU twin, tests/emu/emu_overlap_a.cpp) and test_gpu_overlap_pass_a.py (the
kernels): the adapters and the read families that press on the clean read-end overlap pass A resolves by itself
(piece_core.hpp: piece_overlap_word), and the loader of the twin."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

from ._cases import rseq
from .conftest import ROOT

_HERE = os.path.join(ROOT, "tests", "emu")
_SO = os.path.join(_HERE, "libemu_overlap_a.so")
_SRCS = [os.path.join(_HERE, "emu_overlap_a.cpp")] + [
    os.path.join(ROOT, "atropos_amd", "csrc", f) for f in ("piece_core.hpp", "filter_core.hpp", "locate_core.hpp", "aligner_host.hpp")] + [
    os.path.join(ROOT, "include", "atropos_hip.h")]
TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"

_twin = None


def twin():
    global _twin
    if _twin is None:
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU",
                                   "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "atropos_amd", "csrc"),
                                   _SRCS[0], "-o", _SO])
        _twin = C.CDLL(_SO)
        _twin.emu_overlap_a_scan.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return _twin


TAIL, FLAGGED, VERBATIM, QUEUED = 1, 2, 4, 8                 # bits of scan(..., states=True)'s third array


def scan(ref, e, flags, wr, wq, mo, ic, reads, n, ragged, states=False, force_off=False):
    """What pass A decides for every read: (taken, word, ovl) -- taken: the two-pass pre-pass takes the aligner at this
    length; word: PieceParams::ovl_a; ovl[r]: the overlap read r is resolved with, 0 for none.  states: a fourth value,
    per read TAIL | FLAGGED | VERBATIM | QUEUED (queued for pass B).  force_off: the scan with the word set to 0."""
    mat = np.zeros((len(reads), max(n, 1)), np.uint8)
    lens = np.zeros(len(reads), np.int32)
    for r, q in enumerate(reads):
        assert len(q) <= n and (ragged or len(q) == n)
        mat[r, :len(q)] = np.frombuffer(q.encode(), np.uint8)
        lens[r] = len(q)
    ovl = np.zeros(len(reads), np.int32)
    word = C.c_uint32(0)
    st = np.zeros(len(reads), np.int32)
    rc = twin().emu_overlap_a_scan(ref.encode(), len(ref), e, flags, int(wr), int(wq), mo, ic, mat.ctypes.data, mat.shape[1],
                                   lens.ctypes.data if ragged else None, len(reads), n, ovl.ctypes.data, C.byref(word),
                                   st.ctypes.data, int(force_off))
    assert rc in (0, 1), rc
    assert (ovl >= 0).all(), "a resolved read that is flagged or holds the adapter verbatim"
    return (rc == 0, word.value, ovl, st) if states else (rc == 0, word.value, ovl)


def adapter(rng, kind, m):
    """TruSeq; random; periodic (unit 1-5, with defects); repeated half; low complexity."""
    if kind == 0:
        return TRUSEQ[:m] if m <= 34 else TRUSEQ
    if kind == 1:
        return rseq(rng, m)
    if kind == 2:
        s = list((rseq(rng, rng.randint(1, 5)) * 80)[:m])
        for _ in range(rng.randint(0, 3)):
            s[rng.randrange(m)] = rng.choice("ACGT")
        return "".join(s)
    if kind == 3:
        half = rseq(rng, m // 2 + 1)
        return (half + half)[:m]
    return rseq(rng, m, rng.choice(["AC", "AG", "CT", "ACG"]))


def overlap_reads(rng, ref, n, count):
    """Reads of n bases around a perfect prefix of the adapter at the read end: every overlap length 1 .. m - 1 behind a
    random flank, a flank that continues the adapter's period backwards, a flank that repeats the adapter's start; one
    substitution or indel inside or just before the overlap; a second, shorter or longer, overlap candidate; a chance
    body piece elsewhere; the whole adapter earlier in the read; N runs."""
    m = len(ref)
    reads = []

    def flank(kind):
        if kind == 0:
            return rseq(rng, 24)
        if kind == 1:                                                          # the period of the adapter's start, backwards
            if rng.random() < 0.3:
                return (ref * 3)[2 * m - 24 + rng.randint(0, 3):][:24]        # (... or the adapter's own end)
            return (ref[:rng.randint(1, 5)] * 24)[-24:]
        return (ref[:rng.randint(1, 8)] * 24)[:24]

    def put(q):
        reads.append((rseq(rng, n) + q)[-n:] if n else "")

    for i in range(1, m):                                                      # every overlap length, the three flanks
        for kind in range(3):
            put(flank(kind) + ref[:i])
    while len(reads) < count:
        i = rng.randint(1, m - 1)
        w = rng.random()
        tail = list(ref[:i])
        if w < 0.2:                                                            # an edit inside or just before the overlap
            f = list(flank(rng.randrange(3)))
            s, at = (tail, rng.randrange(i)) if rng.random() < 0.6 else (f, len(f) - 1 - rng.randrange(3))
            v = rng.random()
            if v < 0.5:
                s[at] = rng.choice("ACGT")
            elif v < 0.75:
                del s[at]
            else:
                s.insert(at, rng.choice("ACGT"))
            put("".join(f) + "".join(tail))
        elif w < 0.4:                                                          # a second overlap candidate, shorter or longer
            j = rng.randint(1, m - 1)
            put(rseq(rng, 10) + ref[:j] + rseq(rng, rng.choice([0, 0, 1, 2, 3, 8])) + ref[:i])
        elif w < 0.55:                                                         # a chance body piece elsewhere
            L, a = rng.randint(5, 9), rng.randrange(0, m - 5)
            body = rseq(rng, rng.randint(0, n)) + ref[a:a + L] + rseq(rng, rng.choice([0, 1, 2, 5, 20, 60]))
            put(body + ref[:i])
        elif w < 0.7:                                                          # the whole adapter earlier in the read
            a = list(ref)
            if rng.random() < 0.5:
                a[rng.randrange(m)] = rng.choice("ACGT")
            put("".join(a) + rseq(rng, rng.choice([0, 1, 3, 10, 40])) + ref[:i])
        elif w < 0.85:                                                         # N runs
            q = list((rseq(rng, n) + flank(rng.randrange(3)) + ref[:i])[-n:]) if n else []
            if q:
                at = rng.choice([rng.randrange(len(q)), max(0, len(q) - i - rng.randint(0, 4)), len(q) - 1 - rng.randrange(min(i, len(q)))])
                for x in range(at, min(len(q), at + rng.randint(1, 6))):
                    q[x] = "N"
            reads.append("".join(q))
        else:
            put(flank(rng.randrange(3)) + ref[:i])
    return reads


def ragged(rng, reads, n, m):
    """The same reads cut to their last L bases, L from 0 to n -- shorter than the overlap included."""
    out = []
    for q in reads:
        L = rng.choice([n, rng.randint(0, n), rng.randint(0, m + 4), rng.randint(0, 8), rng.randint(max(0, n - 40), n)])
        out.append(q[len(q) - L:] if L else "")
    return out


def aligners(seed, rounds, mrange=(20, 40)):
    """(ref, e, flags, wr, wq, mo) -- the first is C2's own."""
    rng = random.Random(seed)
    yield TRUSEQ, 0.1, 14, False, False, 3
    for t in range(rounds - 1):
        m = rng.randint(*mrange)
        ref = adapter(rng, t % 5, m)
        wild = rng.random() < 0.25
        yield (ref, rng.choice([0.05, 0.1, 0.12]), rng.choice([14, 14, 14, 10]), wild and rng.random() < 0.5, wild,
               rng.choice([1, 3, 5, 12]))


def record(i, nr):
    return (0, i, nr - i, nr, i, 0)

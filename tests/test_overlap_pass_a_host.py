"""Pass A of the two-pass pre-pass resolves a clean read-end overlap itself (piece_core.hpp: piece_overlap_word).  CPU tier:
what the shared pass-A code decides, per read, through a small twin of its own (tests/emu/emu_overlap_a.cpp, the product's
per-lane source with -DATR_HOST_EMU) against the oracle; the complete two-pass pipeline through the existing twin
against the same oracle records; that the rule is not vacuous on C2's kind of read; and that it never fires where its
premises are off.  The kernels themselves: test_gpu_overlap_pass_a.py."""
import random

import numpy as np

from . import _overlap_a_common as X

LENGTHS = ((150, False), (100, True), (70, False), (250, True))


def test_exactness(emu_backend, oracle):
    """Every read on which the rule fires: its record is the oracle's.  Every read: the two-pass pipeline == the oracle."""
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    rng = random.Random(5)
    total = fired = piped = with_word = 0
    for t, (ref, e, flags, wr, wq, mo) in enumerate(X.aligners(7, 24)):
        n, rg = LENGTHS[t % len(LENGTHS)]
        reads = X.overlap_reads(rng, ref, n, 240)
        if rg:
            reads = X.ragged(rng, reads, n, len(ref))
        exp = [oracle.locate(ref, q, e, flags, wr, wq, mo, 1) for q in reads]
        taken, word, ovl, st = X.scan(ref, e, flags, wr, wq, mo, 1, reads, n, rg, states=True)
        with_word += bool(word)
        # the rest of pass A's answer with the rule on (the exact-overlap chain then runs over min(31, m) rows) against
        # the scan without it: the same read-end condition and verbatim adapter; a resolved read was flagged before
        _, _, off, st0 = X.scan(ref, e, flags, wr, wq, mo, 1, reads, n, rg, states=True, force_off=True)
        assert not off.any()
        keep = X.TAIL | X.VERBATIM
        assert ((st & keep) == (st0 & keep)).all()
        assert (((st & X.FLAGGED) != 0) == (((st0 & X.FLAGGED) != 0) & (ovl == 0))).all()
        assert ((st0[ovl > 0] & X.FLAGGED) != 0).all() and ((st0[ovl > 0] & X.VERBATIM) == 0).all()
        assert ((st & X.QUEUED)[ovl > 0] == 0).all()
        for q, i, x in zip(reads, ovl, exp):
            assert taken or i == 0
            if i:
                assert i <= len(q) and (word >> int(i)) & 1
                assert x == X.record(int(i), len(q)), (ref, q, e, flags, wr, wq, mo, int(i), x)
                fired += 1
        total += len(reads)
        al = Aligner(ref, e, flags, wr, wq, mo, 1)
        mat = reads if rg else np.frombuffer("".join(reads).encode(), np.uint8).reshape(len(reads), n).copy()
        try:
            planes = al.pack(mat, layout="plane64")
        except _lib.AtroposHipError:
            assert not taken
            continue
        assert taken
        got = al.locate_batch(planes).tuples()
        for q, g, x in zip(reads, got, exp):
            assert g == x, (ref, q, e, flags, wr, wq, mo, g, x)
        piped += len(reads)
    assert total > 5500 and piped > 4500 and with_word >= 12 and fired > 600, (total, piped, with_word, fired)


def test_not_vacuous():
    """C2's aligner, a random flank plus adapter[:i], 3 <= i <= 29: the rule fires on at least 90 % of the reads
    (a chance hit in the flank costs 1 - 3 %)."""
    rng = random.Random(11)
    reads = [X.rseq(rng, 150 - i) + X.TRUSEQ[:i] for i in range(3, 30) for _ in range(100)]
    taken, word, ovl = X.scan(X.TRUSEQ, 0.1, 14, False, False, 3, 1, reads, 150, False)
    assert taken and word == sum(1 << i for i in range(3, 30))
    share = float((ovl > 0).mean())
    print("rule fires on %.1f %% of %d reads" % (100 * share, len(reads)))
    assert share >= 0.90
    # ... and with the overlap it was given, unless the flank happens to lengthen it
    want = np.repeat(np.arange(3, 30), 100)
    assert ((ovl == 0) | (ovl >= want)).all() and (ovl == want).mean() > 0.6


def test_never_fires():
    """No firing on an aligner whose word is 0: START_WITHIN_SEQ1, indel cost != 1, more than 32 swept rows, flags
    without STOP_WITHIN_SEQ1."""
    rng = random.Random(13)
    cases = [(X.TRUSEQ, 0.1, 15, 1), (X.TRUSEQ, 0.1, 11, 1), (X.TRUSEQ, 0.1, 14, 2), (X.TRUSEQ, 0.1, 14, 100000),
             (X.TRUSEQ, 0.1, 10, 1), (X.rseq(rng, 48), 0.1, 14, 1), (X.rseq(rng, 64), 0.1, 14, 1), (X.rseq(rng, 41), 0.05, 14, 1)]
    seen = 0
    for ref, e, flags, ic in cases:
        for n, rg in ((150, False), (150, True)):
            reads = X.overlap_reads(rng, ref, n, 400)
            if rg:
                reads = X.ragged(rng, reads, n, len(ref))
            taken, word, ovl = X.scan(ref, e, flags, False, False, 3, ic, reads, n, rg)
            assert word == 0 and not ovl.any(), (ref, e, flags, ic, hex(word))
            seen += taken
    assert seen >= 12                                          # (the pre-pass takes most of them: the word is what keeps the rule off)

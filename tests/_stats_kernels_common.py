"""Shared by test_stats_kernels_host.py (the CPU twin, tests/emu/emu_stats.cpp) and test_gpu_stats_kernels.py (the
kernels of atropos_amd/csrc/stats_kernels.hip): a plain Python model of ``atr_read_stats_batch`` and
``atr_read_stats_merge`` -- one loop per read, one per base, over ``bytes`` -- the builders that put reads on the
kernels' edges (the 64-position windows, the 1 024 length bins kept in LDS, the quality bytes '!'..'~' of the LDS table,
the five register counters, groups of 64 reads with fewer than four reads left, the grid-stride passes), and the
``check_*`` functions that call the entry points at the C ABI with arguments of their own: ``longest`` below the
longest read, records without qualities, masks, destinations, ``index_base`` beyond 2^32, a worker stream.

The model restates the header comment of the two entry points (include/atropos_hip.h) and the layout comment of
stats_core.hpp, the layout offsets and the half-to-even floor division included; it shares no code with
stats_core.hpp, emu_stats.cpp or atropos_amd.stats.  numpy holds the finished block and builds tensors.  Every block
under test lies between guard words, and every comparison covers the whole block, word for word, exact.  A
``check_*`` takes a backend and returns the counts its test asserts on; the ``*_case`` builders are cached and assert,
from the model alone, the floors that keep a case from being hollow."""
import contextlib
import functools
import random

import numpy as np

from . import _fastq_kernels_common as K
from ._fastq_kernels_common import _dev, _i32, _sync, _u8, records_tensor, upload_text

# ---------------------------------------------------------------------------------------------- model: layout
MASK64 = (1 << 64) - 1
HDR = 8                                                     # header words: count, longest, withq, skipped, four unused
COUNT, LONGEST, WITHQ, SKIPPED = 0, 1, 2, 3
GC_BINS, MQ_BINS = 101, 256
GUARD_WORDS = 64
GUARD_PATTERN = 0xA5A5A5A5A5A5A5A5
WIN = 64                                                    # positions per window of the position kernel
LEN_LDS = 1024                                              # read lengths binned in LDS by the scalar kernel


def offsets(L):
    """Word offsets of a block for ``L`` positions: lengths (L + 1), gc (101), meanq (256), seq (L x 256), qual
    (L x 256), then the three first-read sections (L + 1, 101, 256), and the number of words."""
    len_off = HDR
    gc_off = len_off + L + 1
    mq_off = gc_off + GC_BINS
    seq_off = mq_off + MQ_BINS
    qual_off = seq_off + 256 * L
    first_off = qual_off + 256 * L
    return dict(len=len_off, gc=gc_off, mq=mq_off, seq=seq_off, qual=qual_off, first=first_off, first_gc=first_off + L + 1,
                first_mq=first_off + L + 1 + GC_BINS, words=first_off + L + 1 + GC_BINS + MQ_BINS)


def additive(L):
    """True for the words that a call adds into (everything but ``longest`` and the first-read sections)."""
    o = offsets(L)
    m = np.ones(o["words"], dtype=bool)
    m[LONGEST] = False
    m[o["first"]:] = False
    return m


def round_half_even(num, den):
    """round(num / den), ties to the even neighbour, by floor division: the remainder lies in [0, den) for a
    numerator of either sign."""
    q = num // den
    r = num - q * den
    if 2 * r > den or (2 * r == den and q % 2 == 1):
        q += 1
    return q


# ---------------------------------------------------------------------------------------------- model: the two calls
def new_block(L):
    return [0] * offsets(L)["words"]


def _ints(a):
    return None if a is None else [int(x) for x in a]


def model_batch(block, L, longest, quality_base, data, recs, begin=None, end=None, ubegin=None, uend=None, dest=None,
                which=0, index_base=0):
    """atr_read_stats_batch restated: adds the records into ``block`` (a list of ints, the words modulo 2^64)."""
    o = offsets(L)
    begin, end, ubegin, uend, dest = _ints(begin), _ints(end), _ints(ubegin), _ints(uend), _ints(dest)
    first = o["first"]
    for r, rec in enumerate(recs):
        if dest is not None and dest[r] != which:
            continue
        seq_at, seq_len, qual_at, qual_len = int(rec[2]), int(rec[3]), int(rec[4]), int(rec[5])
        a = begin[r] if begin is not None else 0
        b = max(a, end[r]) if begin is not None else seq_len
        n = b - a
        if n > longest:
            block[SKIPPED] = (block[SKIPPED] + 1) & MASK64
            continue
        tag = ~(index_base + r) & MASK64
        block[COUNT] = (block[COUNT] + 1) & MASK64
        block[o["len"] + n] = (block[o["len"] + n] + 1) & MASK64
        block[first + n] = max(block[first + n], tag)
        if n == 0:
            continue
        lo, hi = (ubegin[r], uend[r]) if ubegin is not None else (a, b)
        gc = total = 0
        for p in range(n):
            pos = a + p
            c = data[seq_at + pos] if lo <= pos < hi else 78
            if c == 67 or c == 71:
                gc += 1
            at = o["seq"] + 256 * p + c
            block[at] = (block[at] + 1) & MASK64
            if qual_len > 0:
                q = data[qual_at + pos]
                total += q - quality_base
                at = o["qual"] + 256 * p + q
                block[at] = (block[at] + 1) & MASK64
        block[LONGEST] = max(block[LONGEST], n)
        gb = round_half_even(100 * gc, n)
        block[o["gc"] + gb] = (block[o["gc"] + gb] + 1) & MASK64
        block[o["first_gc"] + gb] = max(block[o["first_gc"] + gb], tag)
        if qual_len > 0:
            block[WITHQ] = (block[WITHQ] + 1) & MASK64
            mb = round_half_even(total, n) + quality_base
            block[o["mq"] + mb] = (block[o["mq"] + mb] + 1) & MASK64
            block[o["first_mq"] + mb] = max(block[o["first_mq"] + mb], tag)
    return block


def model_merge(dst, dst_L, src, src_L, offset):
    """atr_read_stats_merge restated: dst += src; src's reads follow dst's, ``offset`` reads later."""
    d, s = offsets(dst_L), offsets(src_L)
    for i in range(HDR):
        dst[i] = max(dst[i], src[i]) if i == LONGEST else (dst[i] + src[i]) & MASK64
    for key, count in (("len", src_L + 1), ("gc", GC_BINS), ("mq", MQ_BINS), ("seq", 256 * src_L), ("qual", 256 * src_L)):
        for i in range(count):
            dst[d[key] + i] = (dst[d[key] + i] + src[s[key] + i]) & MASK64
    for key, count in (("first", src_L + 1), ("first_gc", GC_BINS), ("first_mq", MQ_BINS)):
        for i in range(count):
            tag = src[s[key] + i]
            if tag:                                                           # ~(index + offset) = ~index - offset
                dst[d[key] + i] = max(dst[d[key] + i], (tag - offset) & MASK64)
    return dst


def as_words(block):
    return np.array(block, dtype=np.uint64)


def model_case(case, L, longest, quality_base, lo=0, hi=None, masks=True, intervals=True, dest=True, which=0, index_base=0,
               block=None):
    """``model_batch`` over records [lo, hi) of a case, every per-record array passed from record ``lo`` on."""
    hi = len(case["recs"]) if hi is None else hi
    cut = lambda key, on: None if (not on or case.get(key) is None) else case[key][lo:hi]
    return model_batch(new_block(L) if block is None else block, L, longest, quality_base, case["data"], case["recs"][lo:hi],
                       cut("begin", intervals), cut("end", intervals), cut("ubegin", masks and intervals),
                       cut("uend", masks and intervals), cut("dest", dest), which, index_base)


# ---------------------------------------------------------------------------------------------- blocks on the backend
class Block(object):
    """A statistics block for ``L`` positions between GUARD_WORDS words of GUARD_PATTERN, cleared by
    atr_read_stats_clear or preloaded with ``words``."""

    def __init__(self, be, L, words=None):
        self.be, self.L = be, L
        self.words = be.read_stats_words(L)
        assert self.words == offsets(L)["words"], (self.words, offsets(L)["words"])
        pool = np.full(self.words + 2 * GUARD_WORDS, GUARD_PATTERN, dtype=np.uint64)
        if words is not None:
            pool[GUARD_WORDS:GUARD_WORDS + self.words] = words
        self.pool = _dev(be, pool.view(np.int64))
        self.view = self.pool[GUARD_WORDS:GUARD_WORDS + self.words]
        if words is None:
            be.read_stats_clear(self.view, L)

    def host(self):
        """The block's words (uint64 ndarray); the guards must be as they were."""
        _sync(self.be)
        h = self.pool.cpu().numpy().view(np.uint64)
        assert (h[:GUARD_WORDS] == GUARD_PATTERN).all(), "guard words in front of the block overwritten"
        assert (h[GUARD_WORDS + self.words:] == GUARD_PATTERN).all(), "guard words behind the block overwritten"
        return h[GUARD_WORDS:GUARD_WORDS + self.words].copy()


def _section(L, i):
    o = offsets(L)
    if i < HDR:
        return "header[%d]" % i
    for key, nxt, row in (("len", "gc", 1), ("gc", "mq", 1), ("mq", "seq", 1), ("seq", "qual", 256), ("qual", "first", 256),
                          ("first", "first_gc", 1), ("first_gc", "first_mq", 1), ("first_mq", "words", 1)):
        if i < o[nxt]:
            k = i - o[key]
            return "%s[%d]" % (key, k) if row == 1 else "%s[%d][%d]" % (key, k // 256, k % 256)
    return "?"


def assert_block(got, want, L, what=None):
    """The whole block, word for word; the table rows from the longest collected read on are zero."""
    want = as_words(want) if isinstance(want, list) else want
    assert got.shape == want.shape, (got.shape, want.shape, what)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s: %d words differ; first: %s" % (what, len(bad), [
            (_section(L, int(i)), int(got[i]), int(want[i])) for i in bad[:8]]))
    o = offsets(L)
    top = int(got[LONGEST])
    assert top <= L
    assert not got[o["seq"] + 256 * top:o["qual"]].any() and not got[o["qual"] + 256 * top:o["first"]].any(), what
    assert not got[4:HDR].any(), what
    return len(got)


class Upload(object):
    """A case in the backend's memory: the text (16-byte aligned, or a view ``misalign`` bytes into an aligned pool),
    the descriptors and the per-record arrays."""

    def __init__(self, be, case, misalign=0):
        self.be, self.case = be, case
        self.data = upload_text(be, case["data"], misalign)
        self.recs = records_tensor(be, case["recs"])
        opt = lambda key, make: None if case.get(key) is None else make(be, case[key])
        self.t = dict(begin=opt("begin", _i32), end=opt("end", _i32), ubegin=opt("ubegin", _i32), uend=opt("uend", _i32),
                      dest=opt("dest", _u8))

    def run(self, block, longest, quality_base, lo=0, hi=None, masks=True, intervals=True, dest=True, which=0, index_base=0):
        """atr_read_stats_batch over records [lo, hi), the arguments as ``model_case`` takes them."""
        hi = self.recs.shape[0] if hi is None else hi
        cut = lambda key, on: None if (not on or self.t[key] is None) else self.t[key][lo:hi]
        self.be.read_stats_batch(block.view, block.L, longest, quality_base, self.data, self.recs[lo:hi].contiguous(),
                                 cut("begin", intervals), cut("end", intervals), cut("ubegin", masks and intervals),
                                 cut("uend", masks and intervals), cut("dest", dest), which, index_base)


def once(be, case, L, longest, quality_base, up=None, **kw):
    """One call into a fresh guarded block against the model: returns (block words, words compared)."""
    up = Upload(be, case) if up is None else up
    blk = Block(be, L)
    up.run(blk, longest, quality_base, **kw)
    got = blk.host()
    return got, assert_block(got, model_case(case, L, longest, quality_base, **kw), L, (L, longest, quality_base, kw))


# ---------------------------------------------------------------------------------------------- builders
ACGTN = b"ACGTN"
LOWER = b"ACGTNacgtn"


def _seq(rng, n, style):
    if style == 0:
        return bytes(rng.choices(ACGTN, weights=(6, 6, 6, 6, 1), k=n))
    if style == 1:
        return bytes(rng.choices(LOWER, k=n))
    return bytes(rng.randrange(256) for _ in range(n))


def layout(reads):
    """(text, descriptors) of [(seq, qual or None)] laid out back to back with one byte between the lines, so that the
    lines start at every alignment; a record without qualities has qual_len 0 (and qual_off 0)."""
    text, recs = bytearray(b"@"), []
    for seq, qual in reads:
        so = len(text)
        text += seq + b"\n"
        if qual is None:
            recs.append([0, 0, so, len(seq), 0, 0, 0, 0])
        else:
            assert len(qual) == len(seq)
            recs.append([0, 0, so, len(seq), len(text), len(qual), 0, 0])
            text += qual + b"+"
    return bytes(text), recs


def kept(case, r, intervals=True):
    """(a, b) of record r."""
    if not intervals or case.get("begin") is None:
        return 0, int(case["recs"][r][3])
    a = int(case["begin"][r])
    return a, max(a, int(case["end"][r]))


def profile(case, longest, masks=True, dest=True, which=0):
    """What a case exercises, counted from the case alone: positions on the 'other byte' path of the sequence table
    (not A C G T N) and on the out-of-table path of the quality table (not '!'..'~'), reads binned at >= 1 024, masked
    positions inside a kept interval, reads whose mask changes their GC bin, skipped and collected reads."""
    out = dict(other_seq=0, out_q=0, q127=0, long_bins=0, masked_inside=0, gc_moved=0, skipped=0, collected=0, bases=0,
               empty=0, no_qual=0)
    data = case["data"]
    for r, rec in enumerate(case["recs"]):
        if dest and case.get("dest") is not None and int(case["dest"][r]) != which:
            continue
        a, b = kept(case, r)
        n = b - a
        if n > longest:
            out["skipped"] += 1
            continue
        out["collected"] += 1
        out["long_bins"] += n >= LEN_LDS
        out["empty"] += n == 0
        out["no_qual"] += n > 0 and rec[5] == 0
        out["bases"] += n
        raw = data[rec[2] + a:rec[2] + b]
        seen = raw
        if masks and case.get("ubegin") is not None:
            ub, ue = int(case["ubegin"][r]), int(case["uend"][r])
            seen = bytes(c if ub <= a + k < ue else 78 for k, c in enumerate(raw))
            out["masked_inside"] += sum(1 for k in range(n) if not ub <= a + k < ue)
            if n:
                gc = lambda s: round_half_even(100 * (s.count(b"C") + s.count(b"G")), n)
                out["gc_moved"] += gc(raw) != gc(seen)
        out["other_seq"] += sum(1 for c in seen if c not in ACGTN)
        if rec[5]:
            q = data[rec[4] + a:rec[4] + b]
            out["out_q"] += sum(1 for c in q if c < 33 or c > 126)
            out["q127"] += q.count(127)
    return out


# ---------------------------------------------------------------------------------------------- 1. length edges
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1022, 1023, 1024, 1025, 2047, 2048, 2049)
EDGE_QUALS = (32, 33, 126, 127)


def _edge_read(rng, n, i):
    """A read of n bases: the sequence in style i % 3; qualities 0..255 with 32, 33, 126, 127 in turn on the first and
    the last position of every window the read reaches."""
    seq = _seq(rng, n, i % 3)
    qual = bytearray(rng.randrange(256) for _ in range(n))
    k = i
    for p in range(n):
        if p % WIN in (0, WIN - 1):
            qual[p] = EDGE_QUALS[k % 4]
            k += 1
    return seq, bytes(qual)


@functools.lru_cache(maxsize=None)
def edge_case():
    """Three reads of every length of EDGE_LENGTHS and 130 of 0..70 bases, shuffled and filled up to three groups of 64;
    then four groups with 1, 2, 3 and 5 non-empty reads; then 37 reads of which three are non-empty."""
    rng = random.Random(1)
    lens = list(EDGE_LENGTHS) * 3 + [rng.randint(0, 70) for _ in range(192 - 3 * len(EDGE_LENGTHS))]
    rng.shuffle(lens)
    for some, size in ((1, 64), (2, 64), (3, 64), (5, 64), (3, 37)):
        group = [0] * size
        for slot, n in zip(rng.sample(range(size), some), (1025, 1, 129, 65, 64)):
            group[slot] = n
        lens += group
    reads = [_edge_read(rng, n, i) for i, n in enumerate(lens)]
    text, recs = layout(reads)
    case = dict(data=text, recs=recs, lens=lens)
    groups = [sum(n > 0 for n in lens[g:g + 64]) for g in range(0, len(lens), 64)]
    case["groups"] = groups
    case["profile"] = c = profile(case, 2049)
    assert len(lens) % 64 == 37 and {1, 2, 3, 5} <= set(groups) and all(lens.count(n) >= 3 for n in EDGE_LENGTHS)
    # every forced quality byte on the first and on the last position of a window; every path of both tables
    at = {(q[p], p % WIN) for _, q in reads for p in range(len(q)) if p % WIN in (0, WIN - 1)}
    assert at >= {(v, w) for v in EDGE_QUALS for w in (0, WIN - 1)}
    assert c["other_seq"] >= 5000 and c["out_q"] >= 10000 and c["q127"] >= 100 and c["long_bins"] >= 19, c
    assert c["bases"] - c["other_seq"] >= 10000 and c["skipped"] == 0
    return case


def check_length_edges(be):
    """The edge case with max_len == longest == 2 049 and with max_len == longest == 4 096 (a loose bound); its first 1,
    2, 3 non-empty reads alone."""
    case = edge_case()
    up = Upload(be, case)
    rep = dict(case["profile"], reads=0, words=0, groups=case["groups"])
    for L, longest in ((2049, 2049), (4096, 4096)):
        got, words = once(be, case, L, longest, 33, up)
        assert got[COUNT] == len(case["recs"]) and got[LONGEST] == 2049 and got[SKIPPED] == 0
        rep["reads"] += len(case["recs"])
        rep["words"] += words
    first = [r for r, n in enumerate(case["lens"]) if n > 0][:3]
    for n in (1, 2, 3):
        few = dict(data=case["data"], recs=[case["recs"][r] for r in first[:n]])
        got, words = once(be, few, 2049, 2049, 33)
        assert got[COUNT] == n
        rep["reads"] += n
        rep["words"] += words
    return rep


# ---------------------------------------------------------------------------------------------- 2. intervals, masks, dest
TEXT_SEQ = b"ACGT" * 5 + b"NNacgtnRY.-*"
MASK_KINDS = ("absent", "all", "empty", "left", "right", "inside", "outside")


@functools.lru_cache(maxsize=None)
def interval_case():
    """700 FASTQ records (names, '+name' lines, reads of 0..300 bases, qualities '!'..'~') with begin / end (the whole
    line, ``end == begin``, ``end < begin``, random) and a mask of every kind of MASK_KINDS in turn; dest in 0..3."""
    rng = random.Random(2)
    parts, begin, end, ubegin, uend, kinds = [], [], [], [], [], []
    for i in range(700):
        n = rng.choice((0, 1, 63, 64, 65, 150, 300)) if i % 7 == 0 else rng.randint(0, 160)
        name = b"r%d" % i
        seq = bytes(rng.choices(TEXT_SEQ, k=n))
        qual = bytes(rng.randint(33, 126) for _ in range(n))
        parts.append(b"@" + name + b"\n" + seq + b"\n+" + (name if i % 3 == 0 else b"") + b"\n" + qual + b"\n")
        how = i % 5
        if how == 0 or n == 0:
            a, b = 0, n
        elif how == 1:
            a = b = rng.randint(0, n)
        elif how == 2:
            a = rng.randint(1, n)
            b = rng.randint(0, a - 1)
        else:
            a = rng.randint(0, n // 2)
            b = rng.randint(a, n)
        kind = MASK_KINDS[(i // 5) % len(MASK_KINDS)]
        e = max(a, b)
        if kind in ("absent", "all"):
            ub, ue = (a, e) if kind == "absent" else (0, n)
        elif kind == "empty":
            ub = rng.randint(0, n)
            ue = rng.randint(0, ub)
        elif kind == "left":
            ub, ue = min(a + rng.randint(1, 9), e), n
        elif kind == "right":
            ub, ue = 0, max(e - rng.randint(1, 9), a)
        elif kind == "inside":
            ub = min(a + rng.randint(1, 9), e)
            ue = max(e - rng.randint(1, 9), ub)
        else:
            ub, ue = (0, a) if (i % 2 and a > 0) else (e, n)
        begin.append(a)
        end.append(b)
        ubegin.append(ub)
        uend.append(ue)
        kinds.append(kind)
    text = b"".join(parts)
    recs, _, err = K.model_index(text)
    assert err == K.INT64_MAX and len(recs) == 700
    dest = [rng.randrange(4) for _ in range(700)]
    case = dict(data=text, recs=recs, begin=np.asarray(begin), end=np.asarray(end), ubegin=np.asarray(ubegin),
                uend=np.asarray(uend), dest=np.asarray(dest), kinds=kinds)
    case["longest"] = max(kept(case, r)[1] - kept(case, r)[0] for r in range(700))
    case["profile"] = c = profile(case, case["longest"], dest=False)
    assert (case["end"] < case["begin"]).sum() >= 50 and (case["end"] == case["begin"]).sum() >= 50
    assert c["masked_inside"] >= 2000 and c["gc_moved"] >= 100 and c["other_seq"] >= 1000, c
    inside = lambda x: sum(1 for r in range(700) if begin[r] < x[r] < max(begin[r], end[r]))
    assert inside(ubegin) >= 100 and inside(uend) >= 100                      # a mask bound strictly inside the interval
    return case


def formatted_case(case, which):
    """The reads with ``dest == which`` as atr_fastq_emit writes them (``model_format``), indexed again: whole records."""
    text, _ = K.model_format(case["data"], case["recs"], case["begin"], case["end"], case["ubegin"], case["uend"], case["dest"],
                             which)
    recs, _, err = K.model_index(text)
    assert err == K.INT64_MAX and len(recs) == int((case["dest"] == which).sum())
    return dict(data=text, recs=recs)


def _sum_of_four(blocks, null, L):
    """The additive words of the four ``which`` blocks sum to those of the block collected with dest == NULL; its
    maxima are the maxima of the four."""
    add = additive(L)
    total = blocks[0].copy()
    for b in blocks[1:]:
        total += b
    assert np.array_equal(total[add], null[add])
    assert np.array_equal(np.maximum.reduce(blocks)[~add], null[~add])


def check_intervals(be, worker=False):
    """One block per ``which`` and one with d_dest == NULL; without masks; without intervals; the formatter cross-check
    for which == 1; the text 1..15 bytes off a 16-byte boundary.  ``worker``: everything on a stream of its own,
    every call twice into its block (the additive words double; the maxima and first reads stay)."""
    case = interval_case()
    L, longest = 320, case["longest"]
    rep = dict(case["profile"], reads=0, words=0, stream="default")
    context = contextlib.nullcontext
    if worker and hasattr(be, "worker_context"):
        context, rep["stream"] = be.worker_context, "worker"
    times = 2 if worker else 1
    add = additive(L)

    def call(up, blocks, **kw):
        blk = Block(be, L)
        for _ in range(times):
            up.run(blk, longest, 33, **kw)
        want = as_words(model_case(case, L, longest, 33, **kw))
        want[add] *= np.uint64(times)
        got = blk.host()
        rep["words"] += assert_block(got, want, L, kw)
        rep["reads"] += times * len(case["recs"])
        blocks.append(got)
        return got

    _sync(be)
    with context():
        up = Upload(be, case)
        four = []
        for which in range(4):
            call(up, four, which=which)
        null = call(up, [], dest=False)
        _sum_of_four(four, null, L)
        assert int(null[COUNT]) == times * 700 and int(null[SKIPPED]) == 0
        call(up, [], dest=False, masks=False)
        call(up, [], which=2, intervals=False)
        if not worker:
            # "as atr_fastq_emit would write them": the formatter model's text, indexed, collected as whole records
            emitted = formatted_case(case, 1)
            whole, words = once(be, emitted, L, longest, 33)
            same = add.copy()
            same[LONGEST] = True
            assert np.array_equal(whole[same], four[1][same])
            rep["words"] += words
            rep["reads"] += len(emitted["recs"])
            for mis in range(1, 16):
                call(Upload(be, case, misalign=mis), [], which=mis % 4)
    return rep


# ---------------------------------------------------------------------------------------------- 3. no qualities
@functools.lru_cache(maxsize=None)
def noqual_case():
    """330 records of 0..150 arbitrary bytes; two of five carry no quality line."""
    rng = random.Random(3)
    reads = []
    for i in range(330):
        n = rng.choice((0, 1, 64, 65, 150)) if i % 6 == 0 else rng.randint(0, 150)
        seq = _seq(rng, n, i % 3)
        reads.append((seq, None if i % 5 in (1, 3) else bytes(rng.randrange(256) for _ in range(n))))
    text, recs = layout(reads)
    case = dict(data=text, recs=recs, reads=reads)
    case["profile"] = c = profile(case, 150)
    assert c["no_qual"] >= 100 and c["collected"] - c["empty"] - c["no_qual"] >= 150, c
    return case


def check_no_qualities(be):
    case = noqual_case()
    L = 150
    got, words = once(be, case, L, 150, 33)
    o, c = offsets(L), case["profile"]
    withq = c["collected"] - c["empty"] - c["no_qual"]
    assert int(got[COUNT]) == 330 and int(got[WITHQ]) == withq < 330 - c["empty"]
    assert int(got[o["mq"]:o["seq"]].sum()) == withq and int(got[o["gc"]:o["mq"]].sum()) == 330 - c["empty"]
    # per position: every read that reaches it is in the sequence table, only those with qualities in the other
    for p in (0, 1, 63, 64, 100, 149):
        reach = [q is not None for s, q in case["reads"] if len(s) > p]
        assert int(got[o["seq"] + 256 * p:o["seq"] + 256 * (p + 1)].sum()) == len(reach)
        assert int(got[o["qual"] + 256 * p:o["qual"] + 256 * (p + 1)].sum()) == sum(reach)
    return dict(c, reads=330, words=words, withq=withq)


# ---------------------------------------------------------------------------------------------- 4. rounding
ROUNDING_BASES = (0, 33, 64, 255)


def _quals_for(total, n, base, rng):
    """n quality bytes with sum(q - base) == total, or None where no bytes 0..255 give it."""
    lo, hi = -base * n, (255 - base) * n
    if not lo <= total <= hi:
        return None
    vals = [total // n] * n                                                   # floor; hand out the remainder
    for k in range(total - sum(vals)):
        vals[k] += 1
    for _ in range(4):                                                        # move weight between two positions
        i, j = rng.randrange(n), rng.randrange(n)
        d = min(3, 255 - base - vals[i], vals[j] + base)
        if i != j and d > 0:
            vals[i] += d
            vals[j] -= d
    assert sum(vals) == total and all(0 <= v + base <= 255 for v in vals)
    return bytes(v + base for v in vals)


@functools.lru_cache(maxsize=None)
def rounding_case(base):
    """GC: 8 bases with 0..8 C/G (ties at 1, 3, 5, 7) and 200 bases with 0..8, 97..103, 196..200 C/G (ties at the odd
    counts).  Mean quality: 2 and 4 bases whose qualities sum to every numerator in -12..12 that the base allows (ties:
    odd over 2, 2 mod 4 over 4; below the base where the numerator is negative).  The expected bins come from Python's
    own ``round`` of the float quotient."""
    rng = random.Random(40 + base)
    reads, want_gc, want_mq = [], {}, {}
    ties = dict(gc_down=0, gc_up=0, mq_down=0, mq_up=0, neg_down=0, neg_up=0, non_ties=0)

    def note(kind, num, den, table, shift):
        exact = num / den
        b = round(exact)                                                      # Python: half to even
        table[b + shift] = table.get(b + shift, 0) + 1
        if kind is None:
            return
        if 2 * num % den == 0 and num % den:                                 # x.5
            up = b > exact
            ties[kind + ("_up" if up else "_down")] += 1
            if num < 0:
                ties["neg_up" if up else "neg_down"] += 1
        else:
            ties["non_ties"] += 1

    for n, counts in ((8, range(9)), (200, list(range(9)) + list(range(97, 104)) + list(range(196, 201)))):
        for g in counts:
            seq = [rng.choice(b"CG") for _ in range(g)] + [rng.choice(b"ATN") for _ in range(n - g)]
            rng.shuffle(seq)
            q = bytes([min(255, base + 7)]) * n
            reads.append((bytes(seq), q))
            note("gc", 100 * g, n, want_gc, 0)
            note(None, (q[0] - base) * n, n, want_mq, base)
    for n in (2, 4):
        for total in range(-12, 13):
            q = _quals_for(total, n, base, rng)
            if q is not None:
                reads.append((b"A" * n, q))
                note("mq", total, n, want_mq, base)
                note(None, 0, n, want_gc, 0)
    text, recs = layout(reads)
    return dict(data=text, recs=recs, want_gc=want_gc, want_mq=want_mq, ties=ties, base=base)


def rounding_ties():
    """The ties of the four cases together, and the floors that keep them from being hollow."""
    total = {}
    for base in ROUNDING_BASES:
        for k, v in rounding_case(base)["ties"].items():
            total[k] = total.get(k, 0) + v
    assert min(total[k] for k in ("gc_down", "gc_up", "mq_down", "mq_up", "neg_down", "neg_up")) >= 8, total
    assert total["non_ties"] >= 100
    assert {12, 38, 62, 88} <= set(rounding_case(33)["want_gc"])
    return total


def check_rounding(be):
    rep = dict(rounding_ties(), reads=0, words=0)
    for base in ROUNDING_BASES:
        case = rounding_case(base)
        got, words = once(be, case, 200, 200, base)
        o = offsets(200)
        gc = {b: int(v) for b, v in enumerate(got[o["gc"]:o["mq"]]) if v}
        mq = {b: int(v) for b, v in enumerate(got[o["mq"]:o["seq"]]) if v}
        assert gc == case["want_gc"], (base, gc, case["want_gc"])
        assert mq == case["want_mq"], (base, mq, case["want_mq"])
        if base in (33, 64):                                                  # -0.5 -> 0, -1.5 -> -2, -2.5 -> -2 of 2 bases
            assert {base, base - 2} <= set(mq) and base - 1 in mq and base - 3 in mq
        rep["reads"] += len(case["recs"])
        rep["words"] += words
    return rep


# ---------------------------------------------------------------------------------------------- 5. first-seen order
ORDER_BASES = (0, 12345, (1 << 32) - 100, 1 << 40)
ORDER_READS = 6037


@functools.lru_cache(maxsize=None)
def order_case():
    """6 037 reads of 0..12 bases.  The reads come in stages of 400: a stage draws from more lengths, GC contents and
    mean qualities than the one before it, so most bins get their first read somewhere in the middle and further reads
    from many later groups of 64 and blocks of 256."""
    rng = random.Random(5)
    reads, bins = [], []
    for r in range(ORDER_READS):
        stage = r // 400
        n = rng.randint(0, min(12, 1 + stage))
        gc = rng.randint(0, min(n, stage))
        seq = [rng.choice(b"CG") for _ in range(gc)] + [rng.choice(b"AT") for _ in range(n - gc)]
        rng.shuffle(seq)
        level = 40 + rng.randint(0, 2 * stage)
        qual = bytes(level + rng.randint(0, 1) for _ in range(n))
        reads.append((bytes(seq), qual))
        if n:
            bins.append((r, ("len", n), ("gc", round_half_even(100 * gc, n)), ("mq", round_half_even(sum(qual), n))))
        else:
            bins.append((r, ("len", 0)))
    text, recs = layout(reads)
    fed = {}
    for row in bins:
        for key in row[1:]:
            fed.setdefault(key, []).append(row[0])
    many_groups = sum(1 for v in fed.values() if len({r // 64 for r in v}) > 1)
    many_blocks = sum(1 for v in fed.values() if len({r // 256 for r in v}) > 1)
    late = sum(1 for v in fed.values() if min(v) >= 256)
    case = dict(data=text, recs=recs, bins=len(fed), many_groups=many_groups, many_blocks=many_blocks, late_first=late,
                first={k: min(v) for k, v in fed.items()})
    assert len(fed) >= 80 and 4 * many_groups >= 3 * len(fed) and 4 * many_blocks >= 3 * len(fed) and late >= 40, case
    return case


def check_first_seen(be):
    """Whole runs at every ORDER_BASES; then three calls into one block with advancing index_base, in order and
    last-first: the earliest read of every bin stays whatever came first."""
    case = order_case()
    up = Upload(be, case)
    L = 16
    o = offsets(L)
    rep = dict(bins=case["bins"], many_groups=case["many_groups"], many_blocks=case["many_blocks"],
               late_first=case["late_first"], reads=0, words=0)
    cuts = (0, 2000, 4100, ORDER_READS)
    for base in ORDER_BASES:
        got, words = once(be, case, L, 12, 0, up, index_base=base)
        for (kind, b), r in case["first"].items():                            # the tags, straight from the builder
            at = {"len": o["first"], "gc": o["first_gc"], "mq": o["first_mq"]}[kind] + b
            assert int(got[at]) == ~(base + r) & MASK64, (base, kind, b)
        assert np.count_nonzero(got[o["first"]:]) == case["bins"]
        rep["reads"] += ORDER_READS
        rep["words"] += words
        for order in ((0, 1, 2), (2, 1, 0)):
            blk = Block(be, L)
            for k in order:
                up.run(blk, 12, 0, lo=cuts[k], hi=cuts[k + 1], index_base=base + cuts[k])
            assert np.array_equal(blk.host(), got), (base, order)
            rep["reads"] += ORDER_READS
            rep["words"] += words
    return rep


# ---------------------------------------------------------------------------------------------- 6. grid-stride passes
STRIDE_READS = 786432 + 257                                # > 2 048 blocks of the scalar kernel, > 3 072 block columns
LONG_READS = 16384 + 321


def block_of_counts(c, L, index_base=0):
    """The block of a ``model_counts`` result of tests/test_stats_host.py (its first reads: index, -1 = none)."""
    o = offsets(L)
    block = np.zeros(o["words"], dtype=np.uint64)
    block[COUNT], block[LONGEST], block[WITHQ], block[SKIPPED] = c["count"], c["longest"], c["withq"], c["skipped"]
    block[o["len"]:o["gc"]] = c["lengths"]
    block[o["gc"]:o["mq"]] = c["gc"]
    block[o["mq"]:o["seq"]] = c["meanq"]
    block[o["seq"]:o["qual"]] = c["seq"].reshape(-1)
    block[o["qual"]:o["first"]] = c["qual"].reshape(-1)
    firsts = np.concatenate([c["first_len"], c["first_gc"], c["first_mq"]])
    tags = ~(firsts.astype(np.uint64) + np.uint64(index_base))
    block[o["first"]:] = np.where(firsts >= 0, tags, np.uint64(0))
    return block


@functools.lru_cache(maxsize=None)
def stride_case():
    """STRIDE_READS records of 0..4 bytes, eight bytes of text each (about 6 MB), built with numpy."""
    rng = np.random.RandomState(6)
    n = STRIDE_READS
    lens = rng.randint(0, 5, n).astype(np.int64)
    letters = np.frombuffer(b"ACGTACGTACGTNacgtn", np.uint8)
    S = letters[rng.randint(0, len(letters), (n, 4))]
    odd = rng.rand(n, 4) < 0.05
    S = np.where(odd, rng.randint(0, 256, (n, 4)), S).astype(np.uint8)
    Q = rng.randint(20, 140, (n, 4)).astype(np.uint8)
    at = 1 + 8 * np.arange(n, dtype=np.int64)
    recs = np.zeros((n, 8), dtype=np.int64)
    recs[:, 2], recs[:, 3], recs[:, 4], recs[:, 5] = at, lens, at + 4, lens
    data = b"@" + np.concatenate([S, Q], axis=1).tobytes()
    return dict(data=data, recs=recs, S=S, Q=Q, lens=lens)


def check_stride_many_reads(be):
    """6 (a): the numpy model of tests/test_stats_host.py, pinned to the plain model on the case's first 3 000 records."""
    from .test_stats_host import empty_counts, model_counts
    case = stride_case()
    L, base = 4, 12345
    small = dict(data=case["data"], recs=case["recs"][:3000].tolist())
    acc = empty_counts(L)
    acc["next"] = base
    pinned = block_of_counts(model_counts(case["S"][:3000], case["Q"][:3000], case["lens"][:3000], 33, acc=acc), L)
    assert np.array_equal(pinned, as_words(model_case(small, L, 4, 33, index_base=base)))
    acc = empty_counts(L)
    acc["next"] = base
    want = block_of_counts(model_counts(case["S"], case["Q"], case["lens"], 33, acc=acc), L)
    blk = Block(be, L)
    Upload(be, case).run(blk, 4, 33, index_base=base)
    got = blk.host()
    words = assert_block(got, want, L, "stride")
    blocks = (STRIDE_READS + 255) // 256
    assert blocks > 2048 and blocks > 3072 and int(got[COUNT]) == STRIDE_READS
    o = offsets(L)
    assert int(got[o["seq"]:o["seq"] + 256].sum()) == int((case["lens"] > 0).sum())
    return dict(reads=STRIDE_READS, words=words, blocks=blocks, pinned=3000)


@functools.lru_cache(maxsize=None)
def long_case():
    """LONG_READS reads of 0..40 bases, forty of them of 3 000..3 100: twenty among the first 16 384 reads (the first
    trip of the position kernel's 64 block columns of four waves) and twenty behind them (its second trip)."""
    rng = random.Random(7)
    lens = [rng.randint(0, 40) for _ in range(LONG_READS)]
    slots = rng.sample(range(16384), 20) + rng.sample(range(16384, LONG_READS), 20)
    for k, r in enumerate(slots):
        lens[r] = 3100 if k in (0, 39) else rng.randint(3000, 3100)
    reads = []
    for i, n in enumerate(lens):
        seq = bytes(rng.choices(LOWER, k=n)) if n > 40 else _seq(rng, n, 0 if i % 9 else 2)
        reads.append((seq, bytes(rng.choices(range(30, 131), k=n))))
    text, recs = layout(reads)
    windows = (3100 + WIN - 1) // WIN
    columns = max(64, 3072 // windows)
    assert windows == 49 and columns == 64 and (LONG_READS + 255) // 256 > columns
    assert sum(1 for r in slots if r >= columns * 256) == 20
    return dict(data=text, recs=recs, long=len(slots), second_trip=20, windows=windows)


def check_stride_long_reads(be):
    """6 (b), plain model."""
    case = long_case()
    got, words = once(be, case, 3100, 3100, 33)
    assert int(got[LONGEST]) == 3100
    o = offsets(3100)
    assert int(got[o["seq"] + 256 * 2999:o["seq"] + 256 * 3000].sum()) == 40  # all forty reach position 2 999
    return dict(reads=LONG_READS, words=words, long=case["long"], second_trip=case["second_trip"], windows=case["windows"])


# ---------------------------------------------------------------------------------------------- 7. skipped, longest
LONGEST_BOUNDS = (0, 1, 50, 63, 64, 65, 120, 128)


@functools.lru_cache(maxsize=None)
def bound_case():
    """320 reads whose kept lengths (a third of them cut by begin / end) run from 0 to 120, with several of exactly 0,
    1, 50, 63, 64, 65 and 120."""
    rng = random.Random(8)
    reads, begin, end = [], [], []
    for i in range(320):
        n = (0, 1, 50, 63, 64, 65, 120)[(i // 4) % 7] if i % 4 == 0 else rng.randint(0, 120)
        a, tail = (rng.randint(0, 5), rng.randint(0, 5)) if i % 3 == 1 else (0, 0)
        seq = _seq(rng, a + n + tail, i % 3)
        reads.append((seq, bytes(rng.randrange(256) for _ in range(len(seq)))))
        begin.append(a)
        end.append(a + n)
    text, recs = layout(reads)
    case = dict(data=text, recs=recs, begin=np.asarray(begin), end=np.asarray(end))
    lens = [e - a for a, e in zip(begin, end)]
    case["lens"] = lens
    for bound in LONGEST_BOUNDS:
        assert bound == 128 or lens.count(bound) >= 5
        assert bound >= 120 or sum(n > bound for n in lens) >= 50
    return case


def check_bounds(be):
    """``longest`` from 0 to max_len: a longer read adds one to ``skipped`` and nothing else; ``longest == 0`` counts
    the empty reads only and leaves the tables alone."""
    case = bound_case()
    up = Upload(be, case)
    L = 128
    o = offsets(L)
    rep = dict(reads=0, words=0, skipped={}, exact={})
    for bound in LONGEST_BOUNDS:
        got, words = once(be, case, L, bound, 33, up)
        skipped = sum(n > bound for n in case["lens"])
        assert int(got[SKIPPED]) == skipped and int(got[COUNT]) == 320 - skipped
        assert int(got[o["len"]:o["gc"]].sum()) == 320 - skipped and not got[o["len"] + bound + 1:o["gc"]].any()
        assert int(got[o["len"] + bound]) == case["lens"].count(bound)
        if bound == 0:
            assert not got[o["gc"]:o["first"]].any() and int(got[LONGEST]) == 0 and int(got[WITHQ]) == 0
            assert np.count_nonzero(got[o["first"]:]) == 1
        elif bound <= 120:                                                    # the reads of exactly `longest`: its last row
            row = got[o["seq"] + 256 * (bound - 1):o["seq"] + 256 * bound]
            assert int(row.sum()) == case["lens"].count(bound) and int(got[LONGEST]) == bound
        rep["skipped"][bound], rep["exact"][bound] = skipped, case["lens"].count(bound)
        rep["reads"] += 320
        rep["words"] += words
    return rep


# ---------------------------------------------------------------------------------------------- 8. merge
# (capacity of the destination, longest read of A, longest read of B, index of A's first read, offset of the merge)
MERGE_RUNS = ((1024, 900, 256, 0, 1000), (1024, 100, 256, (1 << 32) - 1000, 1 << 32), (256, 250, 200, 0, 0), (256, 100, 256, 0, 1000))
MERGE_SRC = 256


@functools.lru_cache(maxsize=None)
def merge_case(a_max, b_max):
    """A: 1 000 reads, B: 500 reads.  A's lengths are even (and a few up to ``a_max``), B's are multiples of three (and
    several of exactly ``b_max``): bins of every histogram on both sides, on one side only, on the other side only."""
    rng = random.Random(a_max * 1000 + b_max)

    def side(count, step, top, level):
        reads = []
        for i in range(count):
            n = top if i % 97 == 5 else (rng.randint(top // 2, top) if i % 50 == 7 else step * rng.randint(0, 60 // step))
            gc = rng.randint(0, n) if i % 2 else (n // 2 if step == 2 else n // 3)
            seq = [rng.choice(b"CG") for _ in range(gc)] + [rng.choice(b"ATN") for _ in range(n - gc)]
            rng.shuffle(seq)
            reads.append((bytes(seq), bytes(level + rng.randint(0, 12) for _ in range(n))))
        text, recs = layout(reads)
        return dict(data=text, recs=recs)

    return side(1000, 2, a_max, 40), side(500, 3, b_max, 48)


def _bins(block, L):
    return {(k, i) for k, n in (("first", L + 1), ("first_gc", GC_BINS), ("first_mq", MQ_BINS)) for i in range(n)
            if block[offsets(L)[k] + i]}


def check_merge(be):
    """Collect A; collect B at index_base 0 into a block of capacity 256; merge with ``offset``: the block that collected
    A and then B at index_base ``offset``.  The model computes both sides.  Then an all-zero source: nothing changes."""
    rep = dict(reads=0, words=0, both=[], src_only=[], dst_only=[], b_wins=0)
    for dst_L, a_max, b_max, a0, offset in MERGE_RUNS:
        A, B = merge_case(a_max, b_max)
        one_a = model_case(A, dst_L, a_max, 33, index_base=a0)
        one_b = model_case(B, MERGE_SRC, b_max, 33)
        bins_a, bins_b = _bins(one_a, dst_L), _bins(one_b, MERGE_SRC)
        rep["both"].append(len(bins_a & bins_b))
        rep["src_only"].append(len(bins_b - bins_a))
        rep["dst_only"].append(len(bins_a - bins_b))
        assert min(rep["both"][-1], rep["src_only"][-1], rep["dst_only"][-1]) >= 5
        assert (one_a[LONGEST] > one_b[LONGEST]) == (a_max > b_max) and one_b[LONGEST] == b_max and one_a[LONGEST] == a_max
        before = as_words(one_a)
        merged = model_merge(list(one_a), dst_L, one_b, MERGE_SRC, offset)
        both = model_case(B, dst_L, b_max, 33, index_base=offset, block=list(one_a))
        assert merged == both
        o = offsets(dst_L)
        rep["b_wins"] += sum(1 for i in range(o["first"], o["words"]) if before[i] and merged[i] != before[i])
        dst, src = Block(be, dst_L), Block(be, MERGE_SRC)
        Upload(be, A).run(dst, a_max, 33, index_base=a0)
        Upload(be, B).run(src, b_max, 33)
        assert_block(src.host(), one_b, MERGE_SRC, "merge source")
        be.read_stats_merge(dst.view, dst_L, src.view, MERGE_SRC, offset)
        got = dst.host()
        rep["words"] += assert_block(got, merged, dst_L, (dst_L, a_max, b_max, offset))
        assert_block(src.host(), one_b, MERGE_SRC, "merge source, after")
        zero = Block(be, MERGE_SRC)
        be.read_stats_merge(dst.view, dst_L, zero.view, MERGE_SRC, 7)
        assert np.array_equal(dst.host(), got) and not zero.host().any()
        rep["reads"] += 1500
    assert rep["b_wins"] >= 5                                                 # offset 0: some first reads are B's
    return rep


# ---------------------------------------------------------------------------------------------- 9. 64-bit words
PRELOAD = (1 << 32) - 3


def check_wide_words(be):
    """Every additive word starts at 2^32 - 3; what the call adds must carry into the upper half."""
    case = bound_case()
    L, bound = 128, 64
    add = additive(L)
    start = np.where(add, np.uint64(PRELOAD), np.uint64(0))
    blk = Block(be, L, start)
    Upload(be, case).run(blk, bound, 33)
    got = blk.host()
    carried = int((got[add] >= np.uint64(1 << 32)).sum())
    rest = got.copy()
    rest[add] -= np.uint64(PRELOAD)
    words = assert_block(rest, model_case(case, L, bound, 33), L, "preloaded")
    assert carried >= 200 and int(got[COUNT]) >> 32 == 1 and int(got[SKIPPED]) >> 32 == 1
    return dict(reads=320, words=words, carried=carried)

"""Shared by test_detect_kernels_host.py (the CPU twin, tests/emu/emu_detect.cpp) and test_gpu_detect_kernels.py (the
kernels of atropos_amd/csrc/detect_kernels.hip): a plain Python model of the three detect passes -- the read filter
(entropy, regular expression, length tests), the distinct pass (first read of every kept sequence inside a run) and
the match pass (``python_counters``: k-mer sets of strings) -- the builders that put reads on the kernels' edges, and
the ``check_*`` functions that call the passes at the C ABI with arguments of their own: per-read ``kept``, ``hashes``
and ``rep``, hand-built ``order`` / ``head``, handles that ``KnownContaminantDetector`` never creates.

The model works on ``str`` and shares no code with ``detect_core.hpp``; numpy only builds tensors.  Every comparison
is exact.  A ``check_*`` takes a backend and returns the counts its test asserts on; the ``*_case`` builders are
cached, so the model runs once per process however many tiers use it."""
import contextlib
import functools
import math
import random
import re

import numpy as np
import torch

from atropos_amd import _lib, detect

from ._fastq_kernels_common import _dev, _sync, padded, records_tensor

COMP = {a: b for a, b in zip("ACGTRYSWKMBDHVNacgtryswkmbdhvn", "TGCAYRSWMKVHDBNtgcayrswmkvhdbn")}
KEPT, DISTINCT, INVALID, OVERLONG = 0, 1, 2, 3               # header words of the counter block (detect_core.hpp)
HDR = _lib.DETECT_HDR
BOUNDARIES = (64, 128, 192, 256)                            # the ballot words of the filter kernel meet here
IUPAC = "ACGTRYSWKMBDHVN"


# ---------------------------------------------------------------------------------------------- model
def entropy_of_acgt(seq):
    """The reference's complexity measure, written out here so that the restatement below stands alone."""
    up = seq.upper()
    h = 0
    for b in ("A", "C", "G", "T"):
        c = up.count(b)
        if c > 0:
            p = c / float(len(up))
            h += p * math.log(p) / math.log(2)
    return -h


def past_end_regexp(past_end):
    return re.compile("|".join(b + "{8,}.*|" + b + "{2,}$" for b in past_end)) if past_end else None


def model_kept(seq, kmer_size, min_k, regexp):
    """(kept length, 0 = dropped; how: 'low' complexity, '' uncut, '8' cut by ``B{8,}.*``, '$' cut by ``B{2,}$``)."""
    if entropy_of_acgt(seq) <= 1.0:
        return 0, "low"
    how, n = "", len(seq)
    m = regexp.search(seq) if regexp is not None else None
    if m:
        n = m.start()
        how = "8" if m.end() - m.start() >= 8 and len(set(seq[n:n + 8])) == 1 else "$"
    return (0 if (n < kmer_size or n < min_k or n == 0) else n), how


def model_rep(keys, head):
    """rep[i] = 1 exactly when no earlier position of i's run (it starts at head[i]) holds the same kept bytes."""
    rep = []
    for i, key in enumerate(keys):
        rep.append(0 if any(keys[j] == key for j in range(head[i], i)) else 1)
    return rep


def python_counters(reads, items, kmer_size, past_end, frac=None, thresholds=None, representatives=None, count_invalid=False):
    """The contract restated in plain Python (not the twin): per known sequence (matches, hits, max_n, abundance).

    ``reads`` are filtered and made distinct here; ``representatives`` (kept sequences, taken as they are, twice if
    given twice) replaces them.  A hit is ``n / n_kmers > frac`` for a known sequence found in the read, or, with
    ``thresholds`` (what ``detect.hit_thresholds`` returns; -1 = never), ``n >= threshold``.  A read with a byte that
    has no complement raises KeyError as the reference does; with ``count_invalid`` it is left out and counted, and
    the count is returned as a third value."""
    if representatives is None:
        regexp = past_end_regexp(past_end)
        min_k = min(len(s) for s, _ in items)
        kept = set()
        for seq in reads:
            if entropy_of_acgt(seq) <= 1.0:
                continue
            m = regexp.search(seq) if regexp is not None else None
            if m:
                seq = seq[:m.start()]
            if len(seq) >= kmer_size and len(seq) >= min_k:
                kept.add(seq)
    else:
        kept = list(representatives)
    post = {}
    n_kmers = []
    for s, (seq, _) in enumerate(items):
        kmers = set(seq[i:i + kmer_size] for i in range(len(seq) - kmer_size + 1))
        n_kmers.append(len(kmers))
        for k in kmers:
            post.setdefault(k, []).append(s)
    out = np.zeros((4, len(items)), dtype=np.int64)
    invalid = 0
    for seq in kept:
        if count_invalid and any(c not in COMP for c in seq):
            invalid += 1
            continue
        rc = "".join(COMP[c] for c in reversed(seq))
        found = []
        for strand in (seq, rc):
            hit = {}
            for k in set(strand[i:i + kmer_size] for i in range(len(strand) - kmer_size + 1)):
                for s in post.get(k, ()):
                    hit[s] = hit.get(s, 0) + 1
            found.append(hit)
        for s in (range(len(items)) if thresholds is not None else set(found[0]) | set(found[1])):
            n = max(found[0].get(s, 0), found[1].get(s, 0))
            out[0, s] += n
            if (thresholds[s] >= 0 and n >= thresholds[s]) if thresholds is not None else n / n_kmers[s] > frac:
                out[1, s] += 1
                out[2, s] = max(out[2, s], n)
        for s, (known, _) in enumerate(items):
            if known in seq:
                out[3, s] += 1
    return (len(kept), out, invalid) if count_invalid else (len(kept), out)


# ---------------------------------------------------------------------------------------------- tensors
def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choices(alphabet, k=n)) if n > 0 else ""


def revcomp(seq):
    return "".join(COMP[c] for c in reversed(seq))


def upload_reads(be, reads):
    """The reads back to back, one byte between them (so the sequences start at every alignment), as a chunk in device
    memory and its record descriptors (only seq_off / seq_len are read by the detect passes)."""
    text, recs = bytearray(b"@"), []
    for seq in reads:
        recs.append([0, 0, len(text), len(seq), len(text), len(seq), 0, 0])
        text += seq.encode("latin-1") + b"\n"
    data = _dev(be, np.frombuffer(padded(bytes(text)), np.uint8).copy())
    return data, records_tensor(be, recs)


def create(be, seqs, kmer_size, past_end, thresholds, max_len=_lib.DETECT_MAX_READ):
    return be.detect_create([s.encode("latin-1") for s in seqs], kmer_size, "".join(past_end).encode("ascii"),
                            list(thresholds), detect.complexity_table(max_len), max_len)


def _host(t):
    return t.cpu().numpy()


def _i64(be, values):
    return _dev(be, np.asarray(values, dtype=np.int64).reshape(-1))


# ---------------------------------------------------------------------------------------------- filter pass
# (past-end bases, kmer_size, lengths of the known sequences, max_len)
FILTER_HANDLES = (
    ((), 4, (4,), 320),
    (("A",), 12, (30, 40), 320),
    (("A", "G"), 32, (32, 40), 320),
    (("N", "T", "A", "C"), 12, (12, 30, 40), 320),
    (("A", "G"), 4, (30,), 320),
    (("A",), 32, (40,), 320),
    (("A",), 4, (30,), 100),
)
FILTER_SLICES = (1, 63, 64, 65, 255, 256, 257)
RUNS = (1, 2, 7, 8, 9, 20)
GRID_READS = 4 * 4096 + 1                                   # one read past 4 waves x 4096 blocks: a second grid-stride trip


def filter_known(i):
    rng = random.Random(900 + i)
    return [rand_seq(rng, n) for n in FILTER_HANDLES[i][2]]


@functools.lru_cache(maxsize=None)
def filter_case(i):
    """The reads of filter handle ``i`` (about 1 500) and what the model says of them."""
    past, k, lens, max_len = FILTER_HANDLES[i]
    rng = random.Random(100 + i)
    min_k = min(lens)
    out = []
    edge = sorted(n for n in {0, 1, k - 1, k, min_k - 1, min_k, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320,
                              max_len - 1, max_len} if n <= max_len)
    for n in edge:
        out.append(rand_seq(rng, n))
        out.append(rand_seq(rng, n, "CGT"))
        for b in past[:2]:
            if n >= 3:
                out.append(rand_seq(rng, n - 2, "CGT".replace(b, "")) + b * 2)
    for b in past or ("A",):
        others = "".join(c for c in "ACGT" if c != b)
        for run in RUNS:
            for where in ["end", "start"] + [(bnd, o) for bnd in BOUNDARIES for o in range(9)]:
                if where == "end":
                    n = rng.randint(min(run + 40, max_len), max_len)
                    out.append(rand_seq(rng, n - run, others) + b * run)
                elif where == "start":
                    n = rng.randint(min(run + 40, max_len), max_len)
                    out.append(b * run + rand_seq(rng, n - run, others))
                else:
                    start = where[0] - where[1]
                    if start + run + 1 > max_len:
                        continue
                    n = start + run + 1 if rng.random() < 0.3 else rng.randint(start + run + 1, max_len)
                    out.append(rand_seq(rng, start, others) + b * run + rand_seq(rng, n - start - run, others))

    def cap(n):
        return min(n, max_len)

    for n in (50, 200, 320):
        out += [rand_seq(rng, cap(n), "acgt"), rand_seq(rng, cap(n), "ACGTacgt"), rand_seq(rng, cap(n), "ACGTN"),
                rand_seq(rng, cap(n) - 30, "cgt") + "a" * 10 + rand_seq(rng, 20, "cgt"),
                rand_seq(rng, cap(n) - 30, "cgt") + "A" * 10 + rand_seq(rng, 20, "cgt")]
    for c in "ACGTNa":
        out += [c * n for n in (1, 50, max_len)]
    for n in (2, 40, 64, 100, max_len):
        for two in ("AC", "GT", "aC", rng.sample("ACGT", 2)):
            half = [two[0]] * (n // 2) + [two[1]] * (n // 2)
            rng.shuffle(half)
            out.append("".join(half))                                         # exactly 1.0: dropped
            if n >= 40:
                third = [c for c in "ACGT" if c not in "".join(two).upper()][0]
                above = [two[0]] * (n // 2) + [two[1]] * (n // 2 - 1) + [third]
                below = [two[0]] * (n // 2 + 1) + [two[1]] * (n // 2 - 1)
                rng.shuffle(above)
                rng.shuffle(below)
                out += ["".join(above), "".join(below)]
    if max_len >= 80:
        quarter = list("A" * 20 + "C" * 20 + "N" * 40)                        # 25 / 25 of 80: exactly 1.0 again
        rng.shuffle(quarter)
        out.append("".join(quarter))
    for b in past:                                                            # equal up to the cut, different behind it
        base = rand_seq(rng, cap(150) - 40, "ACGT".replace(b, ""))
        out += [base + b * 8 + rand_seq(rng, 30), base + b * 9 + rand_seq(rng, 5), base, base[:-1]]
    out += [rng.choice(out) for _ in range(60)]                               # duplicates
    b = (past or ("A",))[0]
    while len(out) < 1500:
        n, kind = rng.randint(0, max_len), rng.random()
        if kind < 0.48:
            out.append(rand_seq(rng, n))
        elif kind < 0.70:
            out.append("".join(rng.choices("AC", weights=(9, 1), k=n)))
        elif kind < 0.85:
            run = rng.randint(1, min(12, n)) if n else 0
            at = rng.randint(0, n - run)
            out.append(rand_seq(rng, at) + b * run + rand_seq(rng, n - at - run))
        else:
            run = min(rng.randint(2, 5), n)
            out.append(rand_seq(rng, n - run) + rng.choice(past or ("A",)) * run)
    rng.shuffle(out)
    regexp = past_end_regexp(past)
    kept, how = zip(*(model_kept(s, k, min_k, regexp) for s in out))
    return dict(reads=out, kept=list(kept), how=list(how), k=k, min_k=min_k, past=past, max_len=max_len)


def filter_conditions(case):
    """What keeps a filter case from being hollow, from the model alone."""
    kept, how = case["kept"], case["how"]
    cuts = [(kl, h) for kl, h in zip(kept, how) if kl > 0 and h in ("8", "$")]
    return dict(reads=len(kept), kept=sum(kl > 0 for kl in kept), dropped=sum(kl == 0 for kl in kept),
                cut8=sum(h == "8" for _, h in cuts), cut_tail=sum(h == "$" for _, h in cuts),
                words=sorted({kl // 64 for kl, _ in cuts}))


def assert_filter_conditions(case):
    c = filter_conditions(case)
    assert 4 * c["kept"] >= c["reads"] and 10 * c["dropped"] >= c["reads"], c
    if case["past"]:
        assert c["cut8"] >= 20 and c["cut_tail"] >= 20, c
        assert c["words"] == list(range((case["max_len"] + 63) // 64 if case["max_len"] < 320 else 5)), c
    else:
        assert c["cut8"] == 0 and c["cut_tail"] == 0, c
    return c


def _check_hashes(reads, kept, hashes):
    """Equal kept bytes <=> equal hashes among the kept reads.  Returns the number of distinct kept sequences."""
    by_key, by_hash = {}, {}
    for seq, kl, h in zip(reads, kept, hashes):
        if kl > 0:
            key = seq[:kl]
            assert by_key.setdefault(key, h) == h, "equal kept bytes, different hashes"
            assert by_hash.setdefault(h, key) == key, "different kept bytes, one hash"
    return len(by_key)


def _filter_call(be, h, data, recs, longest):
    block = be.detect_counters(h)
    kept, hashes = be.detect_filter(h, data, recs, longest, block)
    _sync(be)
    return _host(kept).astype(np.int64), _host(hashes), be.detect_read(h, block)


def check_filter(be, i, twin=None):
    """Filter handle ``i``: the whole batch and its heads of FILTER_SLICES reads against the model; with ``twin``
    (a second backend) also ``kept`` and ``hashes`` of both, bit for bit."""
    case = filter_case(i)
    reads, want = case["reads"], np.asarray(case["kept"], dtype=np.int64)
    rep = dict(assert_filter_conditions(case), compared=0, twin_compared=0)
    longest = max(len(s) for s in reads)
    got = []
    for b in (be,) + ((twin,) if twin is not None else ()):
        h = create(b, filter_known(i), case["k"], case["past"], [1] * len(FILTER_HANDLES[i][2]), case["max_len"])
        try:
            data, recs = upload_reads(b, reads)
            for n in FILTER_SLICES + (len(reads),):
                kept, hashes, block = _filter_call(b, h, data, recs[:n].contiguous(), longest)
                assert np.array_equal(kept, want[:n]), (i, n, np.nonzero(kept != want[:n])[0][:10])
                assert block[KEPT] == int((want[:n] > 0).sum()) and not block[1:].any(), (i, n, block[:HDR])
                rep["distinct"] = _check_hashes(reads[:n], kept, hashes)
                if b is be:
                    rep["compared"] += n
            got.append((kept, hashes))
        finally:
            b.detect_destroy(h)
    if twin is not None:
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), i
        rep["twin_compared"] = len(reads)
    assert rep["distinct"] < rep["kept"]                                      # some kept reads were equal
    return rep


@functools.lru_cache(maxsize=None)
def grid_filter_case():
    """GRID_READS short reads for handle 1 (30 .. 48 bases)."""
    past, k, lens, _ = FILTER_HANDLES[1]
    rng = random.Random(77)
    reads = []
    for r in range(GRID_READS):
        n = rng.randint(28, 48)
        reads.append(rand_seq(rng, n - 9) + "A" * 9 if r % 5 == 0 else rand_seq(rng, n))
    reads[-1] = rand_seq(rng, 40, "CGT") + "AAA"                              # the read of the second trip is kept and cut
    regexp = past_end_regexp(past)
    kept, how = zip(*(model_kept(s, k, min(lens), regexp) for s in reads))
    return dict(reads=reads, kept=list(kept), how=list(how), k=k, past=past)


def check_filter_grid(be, twin=None):
    case = grid_filter_case()
    want = np.asarray(case["kept"], dtype=np.int64)
    assert want[-1] == 40 and 4 * int((want > 0).sum()) >= len(want) and 10 * int((want == 0).sum()) >= len(want)
    got = []
    for b in (be,) + ((twin,) if twin is not None else ()):
        h = create(b, filter_known(1), case["k"], case["past"], [1, 1])
        try:
            data, recs = upload_reads(b, case["reads"])
            kept, hashes, block = _filter_call(b, h, data, recs, 48)
            assert np.array_equal(kept, want), np.nonzero(kept != want)[0][:10]
            assert block[KEPT] == int((want > 0).sum()) and not block[1:].any()
            _check_hashes(case["reads"], kept, hashes)
            got.append((kept, hashes))
        finally:
            b.detect_destroy(h)
    if twin is not None:
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    return dict(compared=len(want), kept=int((want > 0).sum()))


def check_filter_errors(be):
    """``longest`` beyond the handle's max_len is refused with nothing counted; a record beyond max_len that the
    caller did not announce is dropped and counted as OVERLONG."""
    rng = random.Random(5)
    reads = [rand_seq(rng, 100, "CGT"), rand_seq(rng, 150, "CGT"), rand_seq(rng, 99, "CGT"), rand_seq(rng, 101, "CGT")]
    h = create(be, filter_known(6), 4, ("A",), [1], 100)
    try:
        data, recs = upload_reads(be, reads)
        block = be.detect_counters(h)
        for longest in (101, 150, 321):
            try:
                be.detect_filter(h, data, recs, longest, block)
            except _lib.AtroposUnsupported:
                continue
            raise AssertionError("longest = %d was accepted by a handle with max_len = 100" % longest)
        assert not be.detect_read(h, block).any()
        kept, hashes, block = _filter_call(be, h, data, recs, 100)
        assert kept.tolist() == [100, 0, 99, 0] and hashes[1] == 0 and hashes[3] == 0 and hashes[0] != 0
        assert block[:HDR].tolist() == [2, 0, 0, 2, 0, 0, 0, 0] and not block[HDR:].any()
    finally:
        be.detect_destroy(h)
    return dict(refused=3, overlong=2)


# ---------------------------------------------------------------------------------------------- distinct pass
MARK_RUNS = (1, 2, 3, 64, 65, 257)
MARK_SIZES = (1, 63, 64, 65, 256, 257, 3000)


def _mark_run(rng, length, c):
    """A run of ``length`` positions with ``c`` distinct kept sequences: [(read, kept)].  Every sequence comes once;
    of the copies, the first is the head's and sits right behind it, the last sits at the very end.  One sequence is
    the head's with a shorter kept length, one the head's with another last kept byte, and half of the reads have
    bytes of their own behind the cut."""
    head = rand_seq(rng, 60)
    kl = rng.randint(30, 60)
    kinds = [(head, kl)]
    if c >= 2:
        kinds.append((head, kl - rng.randint(1, 5)))                          # shared prefix, another kept length
    if c >= 3:
        last = rng.choice([x for x in "ACGT" if x != head[kl - 1]])
        kinds.append((head[:kl - 1] + last + head[kl:], kl))                  # only the last kept byte differs
    while len(kinds) < c:
        kinds.append((rand_seq(rng, 60), rng.randint(30, 60)))
    copies = length - c
    body = list(range(1, c)) + [rng.randrange(c) for _ in range(max(0, copies - 2))]
    rng.shuffle(body)
    slots = [0] + ([0] if copies >= 1 else []) + body + ([rng.randrange(c)] if copies >= 2 else [])
    assert len(slots) == length and set(slots) == set(range(c))
    out = []
    for sl in slots:
        seq, k = kinds[sl]
        out.append((seq[:k] + (seq[k:] if rng.random() < 0.5 else rand_seq(rng, rng.randint(0, 20))), k))
    return out


@functools.lru_cache(maxsize=None)
def mark_case(m):
    """Runs of MARK_RUNS positions back to back until ``m`` positions (the last run cut short), shuffled over the
    record array: reads, kept, order, head and the model's rep."""
    rng = random.Random(4000 + m)
    plan = []
    if m >= 3000:
        for length in MARK_RUNS:
            plan += [(length, c) for c in sorted({1, 2, 3, length // 2, length - 1, length} & set(range(1, length + 1)))]
        rng.shuffle(plan)
        plan.insert(0, (3, 3))                                                # the first 257 does not start a block
    else:
        plan = [(257, 5), (65, 65), (64, 2), (3, 2), (2, 1), (1, 1)] if m >= 257 else [(65, 3), (64, 64), (3, 3), (2, 2), (1, 1)]
        if m < 63:
            plan = [(m, 1)]
    entries, head, runs = [], [], []
    while len(entries) < m:
        for length, c in plan:
            run = _mark_run(rng, length, c)[:m - len(entries)]
            if not run:
                break
            runs.append((len(entries), len(run)))
            head += [len(entries)] * len(run)
            entries += run
    slots = list(range(len(entries) + 5))                                     # five records that no position names
    rng.shuffle(slots)
    order = slots[:len(entries)]
    reads = [rand_seq(rng, 50)] * len(slots)
    kept = [50] * len(slots)
    for pos, (seq, k) in zip(order, entries):
        reads[pos], kept[pos] = seq, k
    rep = model_rep([seq[:k] for seq, k in entries], head)
    crossing = sum(1 for at, n in runs if at // 256 != (at + n - 1) // 256)
    collided = sum(1 for i, (seq, k) in enumerate(entries) if head[i] != i and seq[:k] != entries[head[i]][0][:entries[head[i]][1]])
    return dict(reads=reads, kept=kept, order=order, head=head, rep=rep, runs=runs, crossing=crossing, collided=collided)


def check_mark(be, m):
    case = mark_case(m)
    h = create(be, ["ACGTTGCAGGATCCATGGACTGACC"], 12, ("A",), [1])
    try:
        data, recs = upload_reads(be, case["reads"])
        kept = _dev(be, np.asarray(case["kept"], dtype=np.int32))
        block = be.detect_counters(h)
        rep = be.detect_mark(h, data, recs, kept, _i64(be, case["order"]), _i64(be, case["head"]), block)
        _sync(be)
        got = _host(rep).astype(np.int64)
        want = np.asarray(case["rep"], dtype=np.int64)
        assert np.array_equal(got, want), (m, np.nonzero(got != want)[0][:10])
        host = be.detect_read(h, block)
        assert host[DISTINCT] == int(want.sum()) and not host[[0] + list(range(2, len(host)))].any()
        # m = 0: OK, nothing touched
        none = be.detect_mark(h, data, recs, kept, _i64(be, []), _i64(be, []), block)
        assert none.shape[0] == 0 and np.array_equal(be.detect_read(h, block), host)
    finally:
        be.detect_destroy(h)
    return dict(compared=m, distinct=int(want.sum()), crossing=case["crossing"], collided=case["collided"],
                longest_run=max(n for _, n in case["runs"]))


# ---------------------------------------------------------------------------------------------- match pass
def _known_sets():
    rng = random.Random(31)
    acgt = [rand_seq(rng, n - 2) + "CA" for n in (33, 60, 90, 130)]           # (they end in one A: see 'cutlast' below)
    half = rand_seq(rng, 20)
    stem = rand_seq(rng, 20)
    kmer = rand_seq(rng, 12)
    special = [half + revcomp(half), stem + rand_seq(rng, 25), stem + rand_seq(rng, 30),
               rand_seq(rng, 9) + kmer + rand_seq(rng, 7) + kmer + rand_seq(rng, 5), rand_seq(rng, 12)]
    with_n = [rand_seq(rng, 20) + "N" + rand_seq(rng, 19), rand_seq(rng, 15) + "NN" + rand_seq(rng, 30),
              rand_seq(rng, 18) + "X" + rand_seq(rng, 21), rand_seq(rng, 33)]
    iupac = ["".join(rng.sample(IUPAC, 15)) + rand_seq(rng, 25, IUPAC), rand_seq(rng, 50, IUPAC), rand_seq(rng, 33) + "CA"]
    mixed = [rand_seq(rng, 40, "ACGTacgt"), rand_seq(rng, 60, "acgt"), rand_seq(rng, 33) + "CA"]
    return dict(w1=acgt[:1], w2=acgt[:2], w3=acgt[:3], w4=acgt, special=special, n=with_n, iupac=iupac, mixed=mixed)


KNOWN_SETS = _known_sets()
# name: (known set, kmer_size, ('frac', f) or ('list', thresholds), m, a known sequence of exactly k bases is added)
MATCH_CASES = {
    "w1_k12": ("w1", 12, ("frac", 0.5), 257, False),
    "w2_k12_frac0": ("w2", 12, ("frac", 0.0), 257, True),
    "w3_k12_frac1": ("w3", 12, ("frac", 1.0), 5, True),
    "w4_k12": ("w4", 12, ("frac", 0.5), 257, True),
    "special_k12": ("special", 12, ("frac", 0.5), 257, False),
    "k4_list_never": ("w4", 4, ("list", [1, -1, 3, 40, 1]), 257, True),
    "k8_m4": ("w4", 8, ("frac", 0.5), 4, True),
    "k16_m1": ("w4", 16, ("frac", 0.5), 1, True),
    "k32": ("w4", 32, ("frac", 0.5), 257, True),
    "k12_list_one": ("w4", 12, ("list", [1, 1, 1, 1, 1]), 257, True),
    "n_k21": ("n", 21, ("frac", 0.5), 257, True),
    "iupac_k16": ("iupac", 16, ("frac", 0.5), 257, True),
    "mixed_k21": ("mixed", 21, ("frac", 0.0), 257, True),
}
REFUSED_K = (("w4", 33), ("n", 22), ("mixed", 22), ("iupac", 17), ("w4", 3))
MATCH_PAST = ("A",)


def _plant(bg, at, piece):
    piece = piece[:max(0, len(bg) - at)]
    return bg[:at] + piece + bg[at + len(piece):]


def _match_reads(rng, seqs, k, target):
    """Reads of every length of the issue's list with a known sequence planted in every way."""
    reads = [s + rand_seq(rng, 320 - len(s), "CGT") for s in seqs]            # whole at the start, no cut: the first reads
    reads.insert(1, rand_seq(rng, 320, "CGT"))                                # and one that holds nothing
    lengths = (k - 1, k, 63, 64, 65, 192, 256, 257, 319, 320)
    kinds = ("start", "end", "split", "revcomp", "lastkmer", "firstkmer", "cutlast", "cutbehind", "swapcase", "none")
    while len(reads) < target:
        for n in lengths:
            for kind in kinds:
                s = rng.choice(seqs)
                bg = rand_seq(rng, n, "CGT" if rng.random() < 0.5 else "ACGT")
                if kind == "start":
                    r = _plant(bg, 0, s)
                elif kind == "end":
                    r = _plant(bg, max(0, n - len(s)), s)
                elif kind == "split":
                    r = _plant(bg, rng.randint(0, max(0, n - len(s))), s[:len(s) // 2] + "N" + s[len(s) // 2:])
                elif kind == "revcomp":
                    r = _plant(bg, rng.randint(0, max(0, n - len(s))), "".join(COMP.get(c, "N") for c in reversed(s)))
                elif kind == "lastkmer":
                    r = _plant(bg, 0, s[-k:])
                elif kind == "firstkmer":
                    r = _plant(bg, max(0, n - k), s[:k])
                elif kind == "cutlast":                                       # B{8,} starts ON the last base of a known ...A
                    at = rng.randint(0, max(0, n - len(s) - 8))
                    r = _plant(rand_seq(rng, n, "CGT"), at, s + "A" * 7 + "C")
                elif kind == "cutbehind":                                     # ... and right behind a known sequence
                    at = rng.randint(0, max(0, n - len(s) - 9))
                    r = _plant(rand_seq(rng, n, "CGT"), at, s + "CAAAAAAAA")
                elif kind == "swapcase":
                    r = _plant(bg, 0, s.swapcase())
                else:
                    r = bg
                reads.append(r)
    return reads


@functools.lru_cache(maxsize=None)
def match_case(name):
    set_name, k, (mode, value), m, with_k = MATCH_CASES[name]
    rng = random.Random(sorted(MATCH_CASES).index(name) + 600)
    seqs = list(KNOWN_SETS[set_name]) + ([rand_seq(rng, k)] if with_k else [])
    n_kmers = [detect.distinct_kmers(s, k) for s in seqs]
    thresholds = detect.hit_thresholds(n_kmers, value) if mode == "frac" else list(value)[:len(seqs)]
    assert len(thresholds) == len(seqs)
    reads = _match_reads(rng, seqs, k, 420)
    return _finish_match_case(rng, seqs, k, thresholds, reads, m, keep_first=len(seqs) + 1)


def _finish_match_case(rng, seqs, k, thresholds, reads, m, keep_first=0):
    regexp = past_end_regexp(MATCH_PAST)
    min_k = min(len(s) for s in seqs)
    kept = [model_kept(r, k, min_k, regexp)[0] for r in reads]
    idx = [i for i, kl in enumerate(kept) if kl > 0]
    rest = idx[keep_first:]
    rng.shuffle(rest)
    order = (idx[:keep_first] + rest)[:m]
    assert len(order) == m, (len(order), m)
    rep = [0 if i % 7 == 6 else 1 for i in range(m)]
    reps = [reads[r][:kept[r]] for r, flag in zip(order, rep) if flag]
    _, want, invalid = python_counters(None, [(s, None) for s in seqs], k, MATCH_PAST, thresholds=thresholds,
                                       representatives=reps, count_invalid=True)
    lost = sum(1 for r in order if any(s in reads[r] and s not in reads[r][:kept[r]] for s in seqs))
    return dict(seqs=seqs, k=k, thresholds=thresholds, reads=reads, kept=kept, order=order, rep=rep, want=want,
                invalid=invalid, reps=len(reps), lost_abundance=lost, lengths=sorted({kept[r] for r in order}),
                words=(max(detect.distinct_kmers(s, k) for s in seqs) + 31) // 32)


def assert_match_conditions(case):
    hits, live = case["want"][1], [s for s, t in enumerate(case["thresholds"]) if t >= 0]
    if live:
        assert any(hits[s] > 0 for s in live) and any(hits[s] < case["reps"] for s in live), hits
    for s, t in enumerate(case["thresholds"]):
        if t < 0:
            assert hits[s] == 0 and case["want"][2][s] == 0


def run_match(be, case, h=None):
    """The match pass over ``case`` -> the counter block (host).  ``kept`` is the model's: this pass is on its own."""
    mine = h is None
    if mine:
        h = create(be, case["seqs"], case["k"], MATCH_PAST, case["thresholds"])
    try:
        data, recs = upload_reads(be, case["reads"])
        kept = _dev(be, np.asarray(case["kept"], dtype=np.int32))
        block = be.detect_counters(h)
        be.detect_match(h, data, recs, kept, _i64(be, case["order"]), _dev(be, np.asarray(case["rep"], dtype=np.uint8)), block)
        return be.detect_read(h, block)
    finally:
        if mine:
            be.detect_destroy(h)


def _assert_block(host, case, kept=0, distinct=0, times=1):
    nseq = len(case["seqs"])
    body = host[HDR:HDR + 4 * nseq].reshape(4, nseq)
    want = case["want"].copy()
    want[[0, 1, 3]] *= times
    assert np.array_equal(body, want), (body, want)
    assert host[:HDR].tolist() == [kept * times, distinct * times, case["invalid"] * times, 0, 0, 0, 0, 0], host[:HDR]


def check_match(be, name):
    case = match_case(name)
    assert_match_conditions(case)
    _assert_block(run_match(be, case), case)
    return dict(compared=case["reps"], invalid=case["invalid"], abundance=int(case["want"][3].sum()),
                lost_abundance=case["lost_abundance"], words=case["words"], lengths=case["lengths"])


def check_refused_k(be):
    for set_name, k in REFUSED_K:
        try:
            h = create(be, KNOWN_SETS[set_name], k, MATCH_PAST, [1] * len(KNOWN_SETS[set_name]))
        except _lib.AtroposUnsupported:
            continue
        be.detect_destroy(h)
        raise AssertionError("kmer_size %d was accepted for the known set %r" % (k, set_name))
    return len(REFUSED_K)


@functools.lru_cache(maxsize=None)
def invalid_case():
    """20 reads; one holds an X in what it keeps, one holds an X only behind the past-end cut."""
    rng = random.Random(8)
    seqs = KNOWN_SETS["w2"]
    reads = [_plant(rand_seq(rng, 150, "CGT"), rng.randint(0, 60), rng.choice(seqs)) for _ in range(20)]
    reads[3] = reads[3][:100] + "X" + reads[3][101:]
    reads[5] = reads[5][:120] + "AAAAAAAAX" + reads[5][129:]
    thresholds = detect.hit_thresholds([detect.distinct_kmers(s, 12) for s in seqs], 0.5)
    case = _finish_match_case(rng, seqs, 12, thresholds, reads, 20)
    case["rep"] = [1] * 20
    case["reps"] = 20
    reps = [reads[r][:case["kept"][r]] for r in case["order"]]
    _, case["want"], case["invalid"] = python_counters(None, [(s, None) for s in seqs], 12, MATCH_PAST, thresholds=thresholds,
                                                       representatives=reps, count_invalid=True)
    assert case["invalid"] == 1 and "X" in reads[5] and "X" not in reads[5][:case["kept"][5]] and case["want"][1].sum() >= 15
    return case


def check_invalid(be):
    case = invalid_case()
    _assert_block(run_match(be, case), case)
    return case["invalid"]


@functools.lru_cache(maxsize=None)
def grid_match_case():
    """GRID_READS representatives of 40 bases, k = 8, two known sequences: the grid-stride loop's second trip."""
    rng = random.Random(9)
    seqs = [rand_seq(rng, 24), rand_seq(rng, 30)]
    reads = []
    for r in range(GRID_READS + 40):
        bg = rand_seq(rng, 40, "CGT")
        reads.append(_plant(bg, rng.randint(0, 20), rng.choice(seqs)[rng.randint(0, 8):]) if r % 3 == 0 else bg)
    reads[-1] = seqs[1] + "CGTTGCCGTT"
    thresholds = detect.hit_thresholds([detect.distinct_kmers(s, 8) for s in seqs], 0.5)
    case = _finish_match_case(rng, seqs, 8, thresholds, reads, GRID_READS)
    assert case["kept"][-1] == 40
    case["order"] = case["order"][:GRID_READS - 1] + [len(reads) - 1]         # the last position is a whole known sequence
    case["rep"] = [1] * GRID_READS
    case["reps"] = GRID_READS
    reps = [reads[r][:case["kept"][r]] for r in case["order"]]
    _, case["want"], case["invalid"] = python_counters(None, [(s, None) for s in seqs], 8, MATCH_PAST, thresholds=thresholds,
                                                       representatives=reps, count_invalid=True)
    return case


def check_match_grid(be):
    case = grid_match_case()
    assert_match_conditions(case)
    assert case["want"][3][1] >= 1
    _assert_block(run_match(be, case), case)
    return dict(compared=case["reps"], hits=case["want"][1].tolist())


# the largest known lists det_build accepts, by words of the k-mer bit set: (sequences, bases each -> distinct 12-mers)
ENVELOPE = {1: (818, 32, 21), 2: (556, 60, 49), 3: (421, 90, 79), 4: (339, 130, 119)}


@functools.lru_cache(maxsize=None)
def envelope_case(words):
    count, length, n_kmers = ENVELOPE[words]
    rng = random.Random(50 + words)
    seqs = [rand_seq(rng, length) for _ in range(count + 1)]
    assert all(detect.distinct_kmers(s, 12) == n_kmers for s in seqs)
    reads = []
    for r in range(260):
        s = seqs[(r * 37) % count] if r % 2 else seqs[count - 1 - r % 3]
        bg = rand_seq(rng, rng.randint(140, 320), "CGT")
        reads.append(_plant(bg, rng.randint(0, 100), s if r % 4 else revcomp(s)))
    thresholds = detect.hit_thresholds([n_kmers] * count, 0.5)
    case = _finish_match_case(rng, seqs[:count], 12, thresholds, reads, 200)
    case["one_more"] = seqs
    return case


def check_envelope(be, words):
    case = envelope_case(words)
    assert case["words"] == words
    assert_match_conditions(case)
    _assert_block(run_match(be, case), case)
    try:
        h = create(be, case["one_more"], 12, MATCH_PAST, case["thresholds"] + [1])
    except _lib.AtroposUnsupported:
        return dict(compared=case["reps"], hits=int(case["want"][1].sum()), abundance=int(case["want"][3].sum()))
    be.detect_destroy(h)
    raise AssertionError("%d known sequences were accepted with %d words" % (len(case["one_more"]), words))


# ---------------------------------------------------------------------------------------------- the whole chain
@functools.lru_cache(maxsize=None)
def chain_case():
    """3 000 ragged reads up to 320 bases, a third of them copies: the model's kept, distinct and counters."""
    rng = random.Random(12)
    seqs = KNOWN_SETS["w4"] + KNOWN_SETS["special"]
    reads = _match_reads(rng, seqs, 12, 1500)[:1500]
    while len(reads) < 2400:
        n = rng.randint(0, 320)
        reads.append(rand_seq(rng, n) if rng.random() < 0.8 else "".join(rng.choices("AC", weights=(9, 1), k=n)))
    reads += [rng.choice(reads) for _ in range(600)]
    rng.shuffle(reads)
    thresholds = detect.hit_thresholds([detect.distinct_kmers(s, 12) for s in seqs], 0.5)
    regexp = past_end_regexp(MATCH_PAST)
    kept = sum(model_kept(r, 12, min(len(s) for s in seqs), regexp)[0] > 0 for r in reads)
    distinct, want = python_counters(reads, [(s, None) for s in seqs], 12, MATCH_PAST, 0.5)
    assert distinct < kept < len(reads) == 3000
    return dict(seqs=seqs, k=12, thresholds=thresholds, reads=reads, want=want, invalid=0, n_kept=kept, distinct=distinct)


def _chain_once(be, h, data, recs, longest, block):
    """filter, sort and run heads (as KnownContaminantDetector.counters builds them), mark, match."""
    kept, hashes = be.detect_filter(h, data, recs, longest, block)
    idx = torch.nonzero(kept > 0).squeeze(1)
    hs, o = torch.sort(hashes.index_select(0, idx))
    order = idx.index_select(0, o).contiguous()
    m = int(order.shape[0])
    pos = torch.arange(m, device=hs.device, dtype=torch.int64)
    start = torch.ones((m,), dtype=torch.bool, device=hs.device)
    start[1:] = hs[1:] != hs[:-1]
    head = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 0).values.contiguous()
    rep = be.detect_mark(h, data, recs, kept, order, head, block)
    be.detect_match(h, data, recs, kept, order, rep, block)
    return be.detect_read(h, block)


def check_chain(be):
    case = chain_case()
    h = create(be, case["seqs"], 12, MATCH_PAST, case["thresholds"])
    contexts = [contextlib.nullcontext]
    if hasattr(be, "worker_context"):
        contexts.append(be.worker_context)
    try:
        data, recs = upload_reads(be, case["reads"])
        _sync(be)
        for context in contexts:
            with context():
                block = be.detect_counters(h)
                once = _chain_once(be, h, data, recs, 320, block)
                twice = _chain_once(be, h, data, recs, 320, block)
            _assert_block(once, case, case["n_kept"], case["distinct"])
            _assert_block(twice, case, case["n_kept"], case["distinct"], times=2)
    finally:
        be.detect_destroy(h)
    return dict(streams=len(contexts), reads=len(case["reads"]), kept=case["n_kept"], distinct=case["distinct"],
                hits=int(case["want"][1].sum()), abundance=int(case["want"][3].sum()))

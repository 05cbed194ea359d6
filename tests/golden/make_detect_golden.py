#!/usr/bin/env python3
"""Generates tests/golden/detect_cases.json.gz: FASTQ texts, known-sequence lists, options and the REFERENCE's
KnownContaminantDetector results for them.  Run in the build container only (the reference is imported from a
scratch build, see make_golden.py --scratch); the committed file holds data only.

Per case and read file: ``n_distinct`` (size of the reference's set of filtered reads), ``full`` = its matches with
limit=None as [seq, kmer_freq, abundance, match_frac, sorted names] in its order, ``top`` = the same with its
default limit of 20, ``top_exact`` = no group of equal sort keys straddles that cut (only then is ``top`` a
defined list).  The known-sequence list of the reference (names and sequences, a data file) is stored once.

usage: python tests/golden/make_detect_golden.py [--scratch /tmp/atropos_ref_build] [--rate-reads 10000]
"""
import argparse
import math
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_SRC, build_reference, dump  # noqa: E402

COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s):
    return s.translate(COMP)[::-1]


class Rec(object):
    def __init__(self, seq):
        self.sequence = seq


def fastq(seqs):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs))


def rseq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def read_through(rng, adapters, n, length, frac=0.4, inserts=None):
    """n reads of `length` bases; `frac` of them are insert + adapter (+ random tail) cut to the length."""
    out = []
    for _ in range(n):
        if rng.random() < frac:
            ins = rng.choice(inserts) if inserts else rng.randint(length // 4, length - 5)
            s = rseq(rng, ins) + rng.choice(adapters) + rseq(rng, length)
            out.append(s[:length])
        else:
            out.append(rseq(rng, length))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/atropos_ref_build")
    ap.add_argument("--rate-reads", type=int, default=10000)
    args = ap.parse_args()
    build_reference(args.scratch)
    from atropos.adapters import AdapterCache
    from atropos.commands.detect import KnownContaminantDetector

    default_list = []
    cache = AdapterCache(path=None)
    cache.load_from_file(os.path.join(REF_SRC, "atropos", "adapters", "sequencing_adapters.fa"))
    for seq, names in cache.iter_sequences():
        for name in sorted(names):
            default_list.append([name, seq])
    seqs = cache.sequences
    truseq = [s for s in seqs if s.startswith("AGATCGGAAGAGC")][:2] or seqs[:2]
    adapters3 = truseq + [seqs[0]]

    def run_ref(known, reads, opts):
        c = AdapterCache(path=None)
        for name, seq in known:
            c.add(name, seq)
        det = KnownContaminantDetector(c, min_kmer_match_frac=opts["min_kmer_match_frac"], kmer_size=opts["kmer_size"],
                                       n_reads=opts["n_reads"], overrep_cutoff=opts["overrep_cutoff"],
                                       include=opts["include"], past_end_bases=tuple(opts["past_end_bases"]))
        if reads:
            det._read_length = len(reads[0])
        for s in reads:
            det.handle_reads(None, Rec(s))

        def rows(ms):
            return [[m.seq, m.count, m.abundance, m.match_frac, sorted(m.names)] for m in ms]
        full = det.matches(limit=None) if reads else []
        full = list(full)
        top = list(det.matches(limit=20)) if reads else []
        key = lambda m: len(m) * math.log(m.count)
        top_exact = len(full) <= 20 or key(full[19]) != key(full[20])
        return dict(n_distinct=len(det._read_sequences), full=rows(full), top=rows(top), top_exact=bool(top_exact))

    cases = []

    def add(name, read_sets, known=None, expect_empty=False, **opts):
        o = dict(kmer_size=12, n_reads=len(read_sets[0]), overrep_cutoff=100, include="all", past_end_bases=["A"],
                 min_kmer_match_frac=0.5)
        o.update(opts)
        t0 = time.time()
        results = [run_ref(known or default_list, reads, o) for reads in read_sets]
        if not expect_empty:
            assert all(r["full"] for r in results), "case %s reports no match" % name
        else:
            assert not any(r["full"] for r in results), "case %s was to be empty" % name
        cases.append(dict(name=name, fastq=[fastq(r) for r in read_sets], known=known, options=o, results=results))
        print("%-22s %5d reads %3d matches, top_exact=%s  (%.1f s)" % (
            name, len(read_sets[0]), len(results[0]["full"]), [r["top_exact"] for r in results], time.time() - t0))

    rng = random.Random(20261016)
    N = 300
    base = read_through(rng, adapters3, N, 100, inserts=[20, 35, 50, 64, 80, 90])
    add("read_through", [base])
    add("read_through_k8", [base], kmer_size=8)
    add("read_through_k16", [base], kmer_size=16)
    add("frac_0.3", [base], min_kmer_match_frac=0.3)
    # 33-base adapters have 22 distinct 12-mers: inserts that leave 11 + 11 bases of them give n / n_kmers == 0.5
    exact = read_through(rng, truseq[:1], N, 100, frac=0.8, inserts=[100 - 22, 100 - 23, 100 - 21, 40])
    add("frac_hit_exactly", [exact], min_kmer_match_frac=0.5)
    add("include_known", [base], include="known")
    with_n = ["".join("N" if rng.random() < 0.02 else c for c in s) for s in base]
    add("with_N", [with_n])
    lower = [s.lower() if i % 3 == 0 else (s[:50] + s[50:].lower() if i % 3 == 1 else s) for i, s in enumerate(base)]
    add("lower_case", [lower])
    rc = [revcomp(s) if i % 2 else s for i, s in enumerate(base)]
    add("reverse_complements", [rc])
    half = rseq(rng, 14)
    pal = half + revcomp(half)
    pal_known = [["pal", pal], ["plain", rseq(rng, 30)]]
    pal_reads = [rseq(rng, rng.randint(5, 40)) + pal + rseq(rng, 60) for _ in range(60)]
    pal_reads = [s[:90] for s in pal_reads] + [rseq(rng, 90) for _ in range(60)]
    add("palindrome", [pal_reads], known=pal_known, n_reads=10)
    dups = list(base[:120]) + list(base[:60]) + [s[:70] + "A" * 30 for s in base[:40]] + [s[:70] + "A" * 12 for s in base[:40]] \
        + [s[:70] + "AA" for s in base[:40]] + [s[:70] + "AAA" for s in base[:40]]
    add("duplicates", [dups])
    low = []
    for i in range(40):
        n = rng.choice([10, 20, 50])
        two = list("A" * n + "C" * n)
        rng.shuffle(two)
        low.append("".join(two))                                         # complexity exactly 1.0
        pad = list("G" * n + "T" * n + "N" * (2 * n))
        rng.shuffle(pad)
        low.append("".join(pad))                                         # 25 % / 25 % of a longer length: exactly 1.0
        three = list("A" * n + "C" * n + "G" * 2)
        rng.shuffle(three)
        low.append("".join(three))                                       # just above
        low.append(rng.choice("ACGT") * 40)
    add("low_complexity", [base[:150] + low])
    tails = []
    for i, s in enumerate(base[:200]):
        t = [1, 2, 7, 8, 9][i % 5]
        core = s[:100 - t]
        core = core[:-1] + ("C" if core[-1] == "A" else core[-1])
        tails.append(core + "A" * t)
    mid = [s[:60] + "A" * rng.randint(8, 12) + s[72:] for s in base[200:260]]
    mid7 = [s[:60] + "A" * 7 + "C" + s[68:] for s in base[260:]]
    add("poly_a", [tails + mid + mid7])
    ag = [s[:75] + rng.choice(["G" * 10 + rseq(rng, 15), rseq(rng, 23) + "GG", "A" * 9 + "G" * 16, rseq(rng, 25)]) for s in base]
    add("past_end_A_G", [ag], past_end_bases=["A", "G"])
    short = [rseq(rng, rng.randint(1, 18)) for _ in range(80)] + [s[:rng.randint(5, 30)] for s in base[:80]]
    add("short_reads", [base[:150] + short])
    varlen = [base[0][:40]] + [s[:rng.randint(30, 100)] for s in base[1:]]
    add("variable_lengths", [varlen])
    r2 = read_through(rng, [revcomp(truseq[0]), seqs[5]], N, 100)
    add("paired", [base, r2])
    add("no_contaminants", [[rseq(rng, 100) for _ in range(150)]], expect_empty=True)
    add("n_reads_scales_cutoff", [base], n_reads=10 ** 9)

    # more than 20 matches, so that the default limit cuts: many adapters of the default list (no tie at the cut) ...
    rng = random.Random(1)
    many = read_through(rng, rng.sample(seqs, 40), 500, 100, frac=0.8, inserts=[10, 20, 30, 40])
    add("limit_cuts", [many], kmer_size=8, min_kmer_match_frac=0.3)
    # ... and a list of 24 sequences of one length planted whole c times each: kmer_freq = c * n_kmers, the sort key
    # of ranks 19 .. 22 is the same, the group straddles the cut and the reference's top 20 is not a defined list
    rng = random.Random(2)
    tie_known = [["t%02d" % i, rseq(rng, 30)] for i in range(24)]
    copies = [40 - i for i in range(18)] + [12, 12, 12, 12] + [5, 4]
    tie_reads = []
    for (_, seq), c in zip(tie_known, copies):
        tie_reads += [rseq(rng, 30) + seq + rseq(rng, 30) for _ in range(c)]
    rng.shuffle(tie_reads)
    add("tie_at_the_cut", [tie_reads], known=tie_known, n_reads=10)
    # known sequences of 90 and 130 bases: 79 and 119 distinct 12-mers, bit sets of three and four words
    for name, size in (("long_known_3_words", 90), ("long_known_4_words", 130)):
        rng = random.Random(size)
        long_known = [["long", rseq(rng, size)], ["short", truseq[0]]]
        lr = []
        for i in range(200):
            a = rng.randint(0, size - 20)
            piece = long_known[0][1][a:a + rng.randint(20, size)]
            s = (rseq(rng, rng.randint(0, 60)) + piece + rseq(rng, 150))[:150]
            lr.append(revcomp(s) if i % 3 == 0 else s)
        lr += [(rseq(rng, 5) + long_known[0][1] + rseq(rng, 150))[:150] for _ in range(10)]
        lr += read_through(rng, truseq[:1], 60, 150)
        add(name, [lr], known=long_known, n_reads=10)

    by_name = {c["name"]: c for c in cases}
    assert any(len(c["results"][0]["full"]) > 20 and c["results"][0]["top_exact"] for c in cases), "no case the limit cuts"
    assert len(by_name["tie_at_the_cut"]["results"][0]["full"]) > 20 and not by_name["tie_at_the_cut"]["results"][0]["top_exact"]
    exact_cases = sum(all(r["top_exact"] for r in c["results"]) for c in cases)
    assert 2 * exact_cases >= len(cases), "too few cases with a defined top-20 list: %d of %d" % (exact_cases, len(cases))

    # the baseline users have today: the reference's own rate, one core
    reads = read_through(rng, adapters3, args.rate_reads, 150)
    t0 = time.time()
    run_ref(default_list, reads, dict(kmer_size=12, n_reads=10000, overrep_cutoff=100, include="all", past_end_bases=["A"],
                                      min_kmer_match_frac=0.5))
    dt = time.time() - t0
    print("reference KnownContaminantDetector: %d reads x 150 bp in %.1f s = %.0f reads/s (one core)"
          % (len(reads), dt, len(reads) / dt))
    dump("detect_cases.json.gz", dict(default_known=default_list, cases=cases))


if __name__ == "__main__":
    main()

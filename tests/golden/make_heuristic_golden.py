#!/usr/bin/env python3
"""Generates tests/golden/heuristic_cases.json.gz: reads, known-sequence lists, options and the REFERENCE's
HeuristicDetector results for them.  Run in the build container only (the reference is imported from a scratch build,
see make_golden.py --scratch); the committed file holds data only.

The reference's answer depends on the iteration order of sets of strings, which changes with the interpreter's hash
seed, so every case runs in child processes under PYTHONHASHSEED = 0 .. 7.  Per seed and read file: ``n_distinct``
(size of the reference's set of filtered reads) and ``full`` / ``top`` = the rows of ``matches(limit=None)`` and of the
default limit of 20: [seq, count, abundance, longest_match, is_known, sorted names, known_seqs sorted by repr,
match_frac, match_frac2].  A case is ``defined`` when the rows of all eight seeds agree, ``longest_match`` excepted.

Asserted here: at least three quarters of the cases are defined; every case that is not meant to be empty reports a
match; the case with a read that is a whole over-represented 20-mer (the reference's ``seq in cur``) loses a
candidate against the same reads without that read (its top count is smaller, though the read adds occurrences).

usage: python tests/golden/make_heuristic_golden.py [--scratch /tmp/atropos_ref_build] [--rate-reads 10000]
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_SRC, build_reference, dump  # noqa: E402
from make_detect_golden import Rec, read_through, rseq  # noqa: E402

SEEDS = range(8)


def run_ref(case, reads, once=False):
    from atropos.adapters import AdapterCache
    from atropos.commands.detect import HeuristicDetector
    o = case["options"]
    cache = None
    if case["known"]:
        cache = AdapterCache(path=None)
        for name, seq in case["known"]:
            cache.add(name, seq)

    def make():
        det = HeuristicDetector(min_frequency=o["min_frequency"], min_contaminant_match_frac=o["min_contaminant_match_frac"],
                                kmer_size=o["kmer_size"], n_reads=o["n_reads"], overrep_cutoff=o["overrep_cutoff"],
                                include=o["include"], known_contaminants=cache, past_end_bases=tuple(o["past_end_bases"]))
        if reads:
            det._read_length = len(reads[0])
        for s in reads:
            det.handle_reads(None, Rec(s))
        return det

    def rows(ms):
        out = []
        for m in ms:
            ks = None if m.known_seqs is None else [list(s) if isinstance(s, tuple) else s for s in sorted(m.known_seqs, key=repr)]
            out.append([m.seq, m.count, m.abundance, m.longest_match[0] if m.longest_match else None, m.is_known,
                        sorted(m.names) if m.names else None, ks, m.match_frac, m.match_frac2])
        return out
    det = make()
    full = rows(det.matches(limit=None)) if reads else []
    top = rows(make().matches(limit=20)) if reads and not once else []
    return dict(n_distinct=len(det._read_sequences), full=full, top=top)


def child(scratch, path):
    build_reference(scratch)
    cases = json.load(open(path))
    out = [[run_ref(c, reads) for reads in c["reads"]] for c in cases]
    json.dump(out, sys.stdout)


def without_longest(result):
    return [[r[:3] + r[4:] for r in result[key]] for key in ("full", "top")] + [result["n_distinct"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/atropos_ref_build")
    ap.add_argument("--rate-reads", type=int, default=10000)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.scratch, args.child)
    build_reference(args.scratch)
    from atropos.adapters import AdapterCache
    cache = AdapterCache(path=None)
    cache.load_from_file(os.path.join(REF_SRC, "atropos", "adapters", "sequencing_adapters.fa"))
    seqs = cache.sequences
    truseq = [s for s in seqs if s.startswith("AGATCGGAAGAGC")][:2] or seqs[:2]
    adapters3 = truseq + [seqs[0]]
    known_list = []
    for seq, names in cache.iter_sequences():
        if seq in adapters3 or len(known_list) < 12:
            known_list += [[name, seq] for name in sorted(names)]

    cases = []

    def add(name, read_sets, known=known_list, expect_empty=False, **opts):
        o = dict(kmer_size=12, n_reads=len(read_sets[0]), overrep_cutoff=100, include="all", past_end_bases=["A"],
                 min_frequency=0.001, min_contaminant_match_frac=0.9)
        o.update(opts)
        cases.append(dict(name=name, reads=read_sets, known=known, options=o, expect_empty=expect_empty))

    rng = random.Random(20261021)
    N = 300
    # free inserts: with a few fixed ones several reads hold an adapter at the smallest index, the reference's
    # longest_match is any of them, and through it match_frac2 of a known match changes with the hash seed
    base = read_through(rng, adapters3, N, 100)
    add("read_through", [base])
    add("fixed_inserts", [read_through(rng, adapters3, N, 100, inserts=[20, 35, 50, 64, 80, 90])])
    add("read_through_k8", [base], kmer_size=8)
    add("read_through_k16", [base], kmer_size=16)
    two = read_through(rng, truseq, N, 100)
    add("two_adapters", [two])
    add("three_adapters_free_inserts", [read_through(rng, adapters3, 400, 120, frac=0.5)])
    add("include_known", [base], include="known")
    decoys = [[n, q] for n, q in known_list if q not in adapters3]
    add("include_unknown", [base], known=decoys, include="unknown")
    add("include_unknown_all_known", [base], include="unknown", expect_empty=True)
    add("no_known_list", [base], known=None)
    add("include_unknown_no_list", [two], known=None, include="unknown")
    add("min_frequency_0.05", [base], min_frequency=0.05)
    add("n_reads_larger", [base], n_reads=2000)
    lower = [s.lower() if i % 3 == 0 else (s[:50] + s[50:].lower() if i % 3 == 1 else s) for i, s in enumerate(base)]
    add("lower_case", [lower])
    add("with_N", [["".join("N" if rng.random() < 0.02 else c for c in s) for s in base]])
    add("duplicates", [list(base[:120]) + list(base[:60]) + [s[:70] + "A" * 30 for s in base[:40]] + list(base[100:200])])
    varlen = [base[0][:60]] + [s[:rng.randint(60, 100)] for s in base[1:]]
    add("variable_lengths", [varlen])
    short = [rseq(rng, rng.randint(1, 18)) for _ in range(60)] + [s[:rng.randint(5, 30)] for s in base[:60]]
    add("short_reads", [base[:200] + short])
    # poly-A tails that the past-end cut shortens to an adapter prefix; one read is cut to exactly the first 20 bases of
    # the adapter, an over-represented 20-mer: the reference's `seq in cur` then drops its two 19-mers from the results
    ad = truseq[0]
    assert ad[19] != "A"
    tails = read_through(rng, [ad], 240, 100, frac=0.5, inserts=[20, 35, 50, 64])
    tails += [(rseq(rng, 30) + ad[:cut] + "A" * 100)[:100] for cut in (24, 28, 31) for _ in range(10)]
    quirk_read = ad[:20] + "A" * 9 + rseq(rng, 71)
    add("poly_a_quirk", [tails + [quirk_read]], known=None)           # (no list: fixed inserts, see above)
    add("poly_a_quirk_control", [tails], known=None)
    rep = rseq(rng, 25)
    twice = [(rseq(rng, rng.randint(5, 20)) + rep + rseq(rng, rng.randint(3, 15)) + rep + rseq(rng, 100))[:100] for _ in range(80)]
    add("kmer_twice_in_a_read", [twice + [rseq(rng, 100) for _ in range(120)]], known=None)
    add("no_contaminants", [[rseq(rng, 100) for _ in range(150)]], expect_empty=True)
    # the first record has 20 bases and min_frequency is 0: min_count(k) is 0 from k = 22 on, every k-mer is
    # over-represented and the loop ends because the reads run out (k reaches the longest read)
    run_out = [base[0][:20]] + [s[:80] for s in two[:80]]
    add("reads_run_out", [run_out], known=None, min_frequency=0.0, n_reads=10)
    r2 = read_through(rng, [truseq[1], seqs[5]], N, 100)
    add("paired", [base, r2])

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.json")
        json.dump(cases, open(path, "w"))
        t0 = time.time()
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--scratch", args.scratch, "--child", path],
                                  stdout=subprocess.PIPE, env=dict(os.environ, PYTHONHASHSEED=str(seed))) for seed in SEEDS]
        by_seed = [json.loads(p.communicate()[0]) for p in procs]
        assert all(p.returncode == 0 for p in procs)
        print("%d cases x %d seeds in %.1f s" % (len(cases), len(by_seed), time.time() - t0))
    defined = 0
    for i, case in enumerate(cases):
        case["results"] = [[by_seed[s][i][k] for s in SEEDS] for k in range(len(case["reads"]))]     # [file][seed]
        case["defined"] = all(without_longest(r) == without_longest(per_file[0]) for per_file in case["results"] for r in per_file)
        defined += case["defined"]
        full = case["results"][0][0]["full"]
        if case.pop("expect_empty"):
            assert not full, "case %s was to be empty" % case["name"]
        else:
            assert all(r["full"] for per_file in case["results"] for r in per_file), "case %s reports no match" % case["name"]
        varies = len({json.dumps([r[3] for r in res["full"]]) for res in case["results"][0]})
        print("%-28s %4d reads %3d matches defined=%s longest_match variants=%d" % (
            case["name"], len(case["reads"][0]), len(full), case["defined"], varies))
    assert 4 * defined >= 3 * len(cases), "too few defined cases: %d of %d" % (defined, len(cases))
    by_name = {c["name"]: c for c in cases}
    with_read = by_name["poly_a_quirk"]["results"][0][0]["full"][0]
    control = by_name["poly_a_quirk_control"]["results"][0][0]["full"][0]
    assert with_read[1] < control[1], "the quirk read drops no candidate: %r against %r" % (with_read[:2], control[:2])

    # the baseline users have today: the reference's own rate, one core
    reads = read_through(rng, adapters3, args.rate_reads, 150)
    t0 = time.time()
    run_ref(dict(known=known_list, options=dict(cases[0]["options"], n_reads=len(reads))), reads, once=True)
    dt = time.time() - t0
    print("reference HeuristicDetector: %d reads x 150 bp in %.1f s = %.0f reads/s (one core)"
          % (len(reads), dt, len(reads) / dt))
    dump("heuristic_cases.json.gz", dict(cases=cases))


if __name__ == "__main__":
    main()

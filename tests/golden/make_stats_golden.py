#!/usr/bin/env python3
"""Generates tests/golden/stats_fuzz.json.gz: FASTQ texts and the REFERENCE's read statistics of them
(SingleEndReadStatistics / PairedEndReadStatistics, BaseQualityErrorEstimator) plus `atropos trim --stats both`
summaries of inputs from trim_cases.json.gz.  Run in this container only (the reference is imported from a scratch
build, see make_golden.py --scratch); the committed file holds data only.

Histograms are stored as [[value, count], ...] in the reference's (first-seen) order with its mean, stdev,
median and modes as it returns them.

usage: python tests/golden/make_stats_golden.py [--scratch /tmp/atropos_ref_build]
"""
import argparse
import base64
import gzip
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import build_reference, dump  # noqa: E402

PE1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACACAGTGATCTCGTATGCCGTCTTCTGCTTG"
PE2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCTCGGTGGTCGCCGTATCATT"
TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def fuzz_fastq(rng, nreads, qb=33, maxlen=300, alphabet="ACGTN", eol="\n", qlo=None, qhi=None):
    qlo = 33 if qlo is None else qlo
    qhi = 126 if qhi is None else qhi
    out = []
    for i in range(nreads):
        r = rng.random()
        n = 0 if r < 0.05 else (rng.randint(1, 12) if r < 0.3 else rng.randint(1, maxlen))
        seq = "".join(rng.choice(alphabet) for _ in range(n))
        qual = "".join(chr(rng.randint(qlo, qhi)) for _ in range(n))
        out.append("@r%d%s%s%s+%s%s%s" % (i, eol, seq, eol, eol, qual, eol))
    return "".join(out)


def tie_fastq():
    """GC and mean-quality half-way ties: 8 bases with 1 G (12.5 -> 12), 8 with 3 C (37.5 -> 38), 2 with 1 C
    (50), quality sums that are x.5 above and below the base (mean -0.5 -> -0 / 0, -1.5 -> -2)."""
    recs = [("AAAAAAAG", "IIIIIIII"), ("CCCAAAAA", "IIIIIIIJ"), ("CA", "!\""), ("AT", " !"), ("TT", "\x1f "),
            ("GGGGGGGA", "########"), ("ACGTACGTAC", "!!!!!!!!!&"), ("G", "5"), ("", ""), ("NNNN", "&&&'")]
    return "".join("@t%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(recs))


def hist_json(summarized):
    items = [[k, v] for k, v in summarized["hist"].items()]
    s = summarized["summary"]
    return dict(hist=items, mean=s["mean"], stdev=s["stdev"], median=s["median"], modes=list(s["modes"]))


def table_json(table):
    t = table if isinstance(table, dict) else table.summarize()        # (trim's summary is summarised already)
    return dict(columns=list(t["columns"]), rows=[list(v) for v in t["rows"].values()])


def stats_json(rs):
    """One ReadStatistics.summarize() dict in JSON form."""
    out = dict(counts=rs["counts"], lengths=hist_json(rs["lengths"]), gc=hist_json(rs["gc"]), bases=table_json(rs["bases"]))
    if "qualities" in rs:
        q = rs["qualities"]
        out["qualities"] = hist_json(q if "summary" in q else q.summarize())
    if "base_qualities" in rs:
        out["base_qualities"] = table_json(rs["base_qualities"])
    return out


def reference_stats(texts, qb):
    from atropos.commands.error import BaseQualityErrorEstimator
    from atropos.commands.stats import PairedEndReadStatistics, SingleEndReadStatistics
    from atropos.io._seqio import FastqReader
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k, t in enumerate(texts):
            paths.append(os.path.join(tmp, "in%d.fastq" % k))
            open(paths[-1], "wb").write(t.encode("latin-1"))
        reads = [list(FastqReader(p)) for p in paths]
    if len(texts) == 1:
        st = SingleEndReadStatistics(qualities=True, quality_base=qb)
        for r in reads[0]:
            st.collect(r)
    else:
        st = PairedEndReadStatistics(qualities=True, quality_base=qb)
        for r1, r2 in zip(*reads):
            st.collect(r1, r2)
    summary = {k: stats_json(v) for k, v in st.summarize().items()}
    errors = []
    for max_bases in (None, 1, 40, 100):
        est, lens = [], []
        for rs in reads:
            e = BaseQualityErrorEstimator(max_read_len=max_bases)
            for r in rs:
                e.handle_reads(None, r)
            est.append(e.estimate()[0] if e.total_len else None)
            lens.append(e.total_len)
        errors.append(dict(max_bases=max_bases, estimate=est, total_len=lens))
    return summary, errors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/atropos_ref_build")
    args = ap.parse_args()
    build_reference(args.scratch)
    from atropos.commands import get_command
    rng = random.Random(20261015)
    cases = []

    def add(name, texts, qb=33):
        summary, errors = reference_stats(texts, qb)
        cases.append(dict(name=name, fastq=texts, quality_base=qb, summary=summary, errors=errors))
        print("%-28s %6d bytes" % (name, sum(len(t) for t in texts)))

    add("plain", [fuzz_fastq(rng, 300)])
    add("crlf", [fuzz_fastq(rng, 150, eol="\r\n")])
    add("ties", [tie_fastq()])
    add("ties_base64", [tie_fastq()], qb=64)
    add("iupac_lower", [fuzz_fastq(rng, 200, alphabet="ACGTNacgtnRYKMSWBDHV.-*")])
    add("any_bytes", [fuzz_fastq(rng, 120, alphabet="".join(chr(c) for c in range(33, 127) if chr(c) not in "@+"))])
    add("base64", [fuzz_fastq(rng, 200, qb=64, qlo=59, qhi=126)], qb=64)
    add("long", [fuzz_fastq(rng, 12, maxlen=3000)])
    add("all_empty_but_one", ["@a\n\n+\n\n@b\nACGT\n+\nIIII\n@c\n\n+\n\n"])
    add("paired", [fuzz_fastq(random.Random(5), 150), fuzz_fastq(random.Random(6), 150)])

    # atropos trim --stats both on inputs of trim_cases.json.gz
    with gzip.open(os.path.join(HERE, "trim_cases.json.gz")) as fh:
        inputs = {k: base64.b64decode(v) for k, v in json.load(fh)["inputs"].items()}
    trim_single = [
        ("synth.fastq", "-a " + TRUSEQ + " -q 20 -m 20"),
        ("synth.fastq", "-a " + TRUSEQ + " -q 15,25 --trim-n -m 30 -M 90"),
        ("synth.fastq", "-a " + TRUSEQ + " --mask-adapter --trim-n"),
        ("synth.fastq", "-a " + TRUSEQ + " --mask-adapter --max-n 0.3"),
        ("synth.fastq", "--max-n 2 --trim-n"),
        ("synth.fastq", "-a " + TRUSEQ + " --zero-cap -q 10 -m 10"),
        ("illumina64.fastq", "-q 10 --quality-base 64 -a XXXXXX"),
    ]
    trim_paired = [
        ("synth_pe.1.fastq", "synth_pe.2.fastq", "--aligner insert -a %s -A %s -q 20 -m 30" % (PE1, PE2)),
        ("synth_pe.1.fastq", "synth_pe.2.fastq",
         "--aligner insert -a %s -A %s --correct-mismatches liberal -m 30" % (PE1, PE2)),
    ]
    trims = []
    with tempfile.TemporaryDirectory() as tmp:
        for idx, (name, argstr) in enumerate(trim_single):
            src, dst = os.path.join(tmp, "in%d.fastq" % idx), os.path.join(tmp, "out%d.fastq" % idx)
            open(src, "wb").write(inputs[name])
            params = argstr.split() + ["-se", src, "-o", dst, "--quiet", "--no-default-adapters", "--no-cache-adapters",
                                       "--stats", "both"]
            retcode, summary = get_command("trim").execute(params)
            assert retcode == 0, argstr
            trims.append(dict(inputs=[name], args=argstr, pre={k: stats_json(v) for k, v in summary["pre"][0].items()},
                              post={d: {k: stats_json(v) for k, v in s[0].items()} for d, s in summary["post"].items()}))
            print("trim %-60s post: %s" % (argstr[:60], sorted(summary["post"])))
        for idx, (n1, n2, argstr) in enumerate(trim_paired):
            paths = [os.path.join(tmp, "pe%d_%s.fastq" % (idx, t)) for t in ("in1", "in2", "out1", "out2")]
            open(paths[0], "wb").write(inputs[n1])
            open(paths[1], "wb").write(inputs[n2])
            params = argstr.split() + ["-pe1", paths[0], "-pe2", paths[1], "-o", paths[2], "-p", paths[3], "--quiet",
                                       "--no-default-adapters", "--no-cache-adapters", "--stats", "both"]
            retcode, summary = get_command("trim").execute(params)
            assert retcode == 0, argstr
            trims.append(dict(inputs=[n1, n2], args=argstr, pre={k: stats_json(v) for k, v in summary["pre"][0].items()},
                              post={d: {k: stats_json(v) for k, v in s[0].items()} for d, s in summary["post"].items()}))
            print("trim %-60s post: %s" % (argstr[:60], sorted(summary["post"])))
    dump("stats_fuzz.json.gz", dict(cases=cases, trim=trims))


if __name__ == "__main__":
    main()

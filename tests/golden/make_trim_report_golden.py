#!/usr/bin/env python3
"""Generates tests/golden/trim_report.json.gz: the REFERENCE's ``summary['trim']`` (RecordHandler.summarize,
commands/trim/__init__.py:129-137) and the input totals ``Pipeline.finish`` writes (commands/base.py:98-110) for
every command line of make_trim_golden.py that lies inside the envelope of the device trim report, plus synthetic
lines that fill what those leave out.  Run in the build container only (the reference is imported from a scratch
build, see make_golden.py --scratch); the committed file holds data only and names its inputs, whose text is in
trim_cases.json.gz.

Normalisation: MergingDict, Const and the counting dicts become plain JSON (tuples become lists, integer keys
strings), the running number that names an adapter without a name becomes its position ("#1").  The reference keys ``record_counts`` / ``bp_counts`` by its source index, 0 (one input per run).

usage: python tests/golden/make_trim_report_golden.py [--scratch /tmp/oracle_ref]
"""
import argparse
import base64
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_trim_golden import CASES, PAIRED_CASES, PE1, PE2, TRUSEQ, synth_fastq, synth_pairs      # noqa: E402

# what the device report refuses (linked adapters, the insert aligner, merging, bisulfite trimmers) and the inputs the
# reference's reader rejects
def in_envelope(names, argstr):
    words = argstr.split()
    if any(n.startswith("bad_") for n in names):
        return False
    if "..." in argstr or "--bisulfite" in words or "-R" in words or "--merge-overlapping" in words:
        return False
    return not ("--aligner" in words and words[words.index("--aligner") + 1] == "insert")


# synthetic lines: what the conditions on the fixture ask for and the lines above do not reach
EXTRA = [
    ("synth.fastq", "-a first=ACGTTGCAAC -a second=" + TRUSEQ),                     # two adapters, the second wins
    ("synth.fastq", "-a first=ACGTTGCAAC -a second=" + TRUSEQ + " -b third=" + TRUSEQ[:18] + " -n 3 --mask-adapter"),
    ("synth.fastq", "-g " + TRUSEQ[:20] + " -e 0.2 -O 4 --no-trim"),
    ("synth.fastq", "-b " + TRUSEQ + " -n 2 --mask-adapter -q 20 --op-order CAGQW --nextseq-trim 15"),
    ("synth.fastq", "-a " + TRUSEQ + " -u 7 -u -9 --cut-min 12 --cut-min -15 -m 25 --too-short-output {too_short}"),
    ("synth.fastq", "-a " + TRUSEQ + " -u 120"),                                    # a cut longer than most reads
    ("synth.fastq", "-a " + TRUSEQ + " -M 60 --too-long-output {too_long} --max-n 1 --trim-n"),
    ("synth.fastq", "-a " + TRUSEQ + " --discard-trimmed -m 30 -q 10,10"),
]
EXTRA_PAIRED = [
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-a %s -A %s --pair-filter both -m 60 -q 20" % (PE1, PE2)),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-a %s -A %s -G %s -n 2 --mask-adapter --trim-n --max-n 0.2" % (PE1, PE2, PE1[:20])),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-a %s -A %s --no-trim --discard-untrimmed" % (PE1, PE2)),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-b %s -B %s -u 3 -U -4 -U 2 --nextseq-trim 18" % (PE1[:30], PE2[:30])),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-a %s -A %s -M 120 --too-long-output {too_long} --too-long-paired-output {too_long2} -m 50" % (PE1, PE2)),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-a %s -m 30 --discard-trimmed" % PE1),                        # legacy mode
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-g %s -e 0.2 -u 4 --max-n 2" % PE1[:16]),                     # legacy mode
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-a %s -A %s --cut-min 8 --cut-min2 -6 --cut-min2 3 --pair-filter both -m 40" % (PE1, PE2)),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-U 5 --trim-n -m 20"),
    ("synth_pe.1.fastq", "synth_pe.2.fastq", "-A %s -q 15,15 --max-n 0.1 --pair-filter both" % PE2),
    ("paired.1.fastq", "paired.2.fastq", "-a TTAGACATAT -A CAGTGGAGTA -n 2 --mask-adapter"),
    ("paired.1.fastq", "paired.2.fastq", "-g ^TTAGACATAT -A CAGTGGAGTA$ --no-indels -e 0.2"),
]

KINDS = ("info", "rest", "wildcard", "too_short", "too_short2", "too_long", "too_long2", "untrimmed", "untrimmed2")

# the conditions on the fixture: (label, paired?, test on the argument words)
TALLY = [
    ("-g", False, lambda w: "-g" in w), ("-b", False, lambda w: "-b" in w),
    ("anchored", False, lambda w: any(x.startswith("^") or x.endswith("$") for x in w)),
    ("second wins", False, lambda w: "first=ACGTTGCAAC" in w),
    ("--times 2", False, lambda w: any(a in ("--times", "-n") and b == "2" for a, b in zip(w, w[1:]))),
    ("--mask-adapter", False, lambda w: "--mask-adapter" in w), ("--no-trim", False, lambda w: "--no-trim" in w),
    ("-q", False, lambda w: "-q" in w), ("--nextseq-trim", False, lambda w: "--nextseq-trim" in w),
    ("--trim-n", False, lambda w: "--trim-n" in w), ("-u twice", False, lambda w: w.count("-u") == 2),
    ("--cut-min", False, lambda w: "--cut-min" in w), ("-m", False, lambda w: "-m" in w), ("-M", False, lambda w: "-M" in w),
    ("--max-n", False, lambda w: "--max-n" in w),
    ("--discard-trimmed", False, lambda w: "--discard-trimmed" in w or "--discard" in w),
    ("--too-short-output", False, lambda w: "--too-short-output" in w),
    ("legacy", True, lambda w: not any(x in w for x in ("-A", "-G", "-B", "-U", "-q", "--trim-n", "--pair-filter", "--cut-min2"))),
    ("--pair-filter both", True, lambda w: "both" in w),
]


def plain(obj, key=None):
    """The summary as plain JSON data.  An adapter without a name of its own carries a running number of the process
    that made it: such a name becomes "#<position in its cutter>"."""
    if type(obj).__name__ == "Const":
        obj = obj.value
    if isinstance(obj, dict):
        if key == "adapters":
            return {("#%d" % pos if str(k).isdigit() else str(k)): plain(v) for pos, (k, v) in enumerate(obj.items(), 1)}
        return {str(k): plain(v, k) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [plain(v, key) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    raise TypeError("summary value of type %s" % type(obj).__name__)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/oracle_ref")
    args = ap.parse_args()
    sys.path.insert(0, args.scratch)
    from atropos.commands import get_command
    from atropos.commands.base import Summary
    # the dicts as RecordHandler.summarize and Pipeline.finish leave them: without the report layer's post-processing
    # (Summary.finish: fractions, totals, the errors tables flattened to columns / rows)
    Summary.finish = lambda self: None
    with gzip.open(os.path.join(HERE, "trim_cases.json.gz"), "rb") as fh:
        inputs = {k: base64.b64decode(v) for k, v in json.loads(fh.read().decode())["inputs"].items()}
    assert inputs["synth.fastq"] == synth_fastq(1200, 11).encode()           # (the builders still make the stored text)
    assert [inputs["synth_pe.1.fastq"], inputs["synth_pe.2.fastq"]] == synth_pairs(500, 21)

    single = [c for c in CASES if in_envelope(c[:1], c[1])] + EXTRA
    paired = [c for c in PAIRED_CASES if in_envelope(c[:2], c[2])] + EXTRA_PAIRED
    doc = dict(cases=[], paired=[])
    with tempfile.TemporaryDirectory() as tmp:
        for idx, case in enumerate(single + paired):
            names, argstr = case[:-1], case[-1]
            ins = [os.path.join(tmp, "in%d_%d.fastq" % (idx, k)) for k in range(len(names))]
            for path, name in zip(ins, names):
                open(path, "wb").write(inputs[name])
            filled = argstr
            for kind in KINDS:
                filled = filled.replace("{%s}" % kind, os.path.join(tmp, "%s_%d.txt" % (kind, idx)))
            outs = [os.path.join(tmp, "out%d_%d.fastq" % (idx, k)) for k in range(len(names))]
            params = filled.split() + (["-se", ins[0], "-o", outs[0]] if len(names) == 1 else
                                       ["-pe1", ins[0], "-pe2", ins[1], "-o", outs[0], "-p", outs[1]])
            retcode, summary = get_command("trim").execute(params + ["--quiet", "--no-default-adapters", "--no-cache-adapters"])
            assert retcode == 0 and "exception" not in summary, (argstr, summary.get("exception"))
            entry = dict(args=argstr, trim=plain(summary["trim"]))
            entry.update(("input" if len(names) == 1 else "input%d" % (k + 1), n) for k, n in enumerate(names))
            for key in ("record_counts", "total_record_count", "bp_counts", "total_bp_counts", "sum_total_bp_count"):
                entry[key] = plain(summary[key])
            doc["paired" if len(names) == 2 else "cases"].append(entry)
            print("%-16s %-100s -> %d records" % (names[0], argstr[:100], entry["total_record_count"]))
    print("tally: %d single-end, %d paired cases" % (len(doc["cases"]), len(doc["paired"])))
    assert len(doc["cases"]) >= 40 and len(doc["paired"]) >= 15
    for label, is_paired, test in TALLY:
        count = sum(1 for c in doc["paired" if is_paired else "cases"] if test(c["args"].split()))
        print("  %-20s %d" % (label, count))
        assert count >= 1, label
    out = os.path.join(HERE, "trim_report.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, sort_keys=True).encode())
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()

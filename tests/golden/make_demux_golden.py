#!/usr/bin/env python3
"""Generates tests/golden/trim_demux.json.gz: every file the REFERENCE's ``atropos trim`` leaves when the output path
holds ``{name}`` (demultiplexing by adapter name: commands/trim/writers.py:95, :119-128, :147-154;
commands/trim/__init__.py:605-630), for a list of single-end command lines over the inputs of trim_cases.json.gz.
Run in the build container only (the reference is imported from a scratch build, see make_golden.py --scratch); the
committed file holds data only and names its inputs.

Per case: ``args`` (the output files of the filters as {too_short} / {too_long} / {untrimmed}), ``input``, ``head``
(the run read the first ``head`` records of the input; null: all of them -- that keeps the file below 1 MiB) and
``files`` = {file name: base64 text} of everything the run left next to its input, empty files included.  The run
writes to ``out.{name}.fastq``.  An adapter without a name of its own is named by a running number of the process
that parsed it: the generator restarts the reference's numbering before every case, so such an adapter's file is
``out.<position>.fastq``, stored as ``out.#<position>.fastq`` (cases name all of their adapters or none).

usage: python tests/golden/make_demux_golden.py [--scratch /tmp/oracle_ref]
"""
import argparse
import base64
import gzip
import itertools
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_trim_golden import TRUSEQ      # noqa: E402

SMALL = "TTAGACATATCTCCGTCG"
SHORT = "ACGTTGCAAC"
# twelve 5' barcodes of three bases, anchored
BARCODES = ["ACG", "CAT", "GTA", "TGC", "AAC", "CCA", "GGT", "TTG", "AGA", "CTC", "GAG", "TCT"]
TWELVE_G = " ".join("-g bc%02d=^%s" % (k + 1, b) for k, b in enumerate(BARCODES))
# twelve 3' adapters: the two the synthetic reads were made with or resemble, and ten prefixes / windows of the long one
TWELVE_A = " ".join("-a ad%02d=%s" % (k + 1, s) for k, s in enumerate(
    [TRUSEQ, SHORT] + [TRUSEQ[k:k + 12 + k] for k in range(1, 11)]))

CASES = [
    ("synth.fastq", "-a first=%s -a second=%s" % (SHORT, TRUSEQ)),                                  # 2 named
    ("synth.fastq", "-a first=%s -a second=%s -b third=%s" % (SHORT, TRUSEQ, TRUSEQ[:18])),          # 3 named
    ("synth.fastq", TWELVE_G + " --no-indels -e 0"),                                                # 12 barcodes
    ("synth.fastq", TWELVE_A),                                                                      # 12 named
    ("synth.fastq", "-a %s -a %s" % (SHORT, TRUSEQ)),                                               # unnamed
    ("small.fastq", "-b %s -b CAAGAT" % SMALL),                                                     # unnamed, -b
    ("small.fastq", "-g one=^CCTA -g two=^GGTC -g three=^TACG -e 0.3"),                             # -g ^ barcodes
    ("synth.fastq", "-g bA=^A -g bC=^C -a tru=%s -n 2 -O 1" % TRUSEQ),                              # round 2 differs from round 1
    ("synth.fastq", "-a first=%s -b second=%s --no-trim" % (SHORT, TRUSEQ)),
    ("synth.fastq", "-a first=%s -b second=%s -n 2 --mask-adapter" % (SHORT, TRUSEQ)),
    ("synth.fastq", "-a first=%s -a second=%s --untrimmed-output {untrimmed}" % (SHORT, TRUSEQ)),
    ("synth.fastq", "-a first=%s -a second=%s --discard-untrimmed" % (SHORT, TRUSEQ)),
    ("synth.fastq", "-a first=%s -a second=%s -m 40 --too-short-output {too_short}" % (SHORT, TRUSEQ)),
    ("synth.fastq", "-a first=%s -a second=%s --max-n 1 -M 80 --too-long-output {too_long}" % (SHORT, TRUSEQ)),
    ("synth.fastq", "-a first=%s -a second=%s -q 20 --trim-n -m 30 --untrimmed-output {untrimmed}" % (SHORT, TRUSEQ)),
    ("small.fastq", "-a nope=GGGGGGGGGGCCCCCCCCCCGGGGGGGGGG -O 20"),                                 # no read matches
    ("small.fastq", "-a nope=GGGGGGGGGGCCCCCCCCCCGGGGGGGGGG -O 20 --discard-untrimmed"),            # ... and nothing is written
    ("small.fastq", "-g every=^N -a ad=%s" % SMALL),                                                # every read matches
    ("small.fastq", "-a ad=%s -m 30" % SMALL),                                                      # -m without an output
]
KINDS = ("too_short", "too_long", "untrimmed")
HEAD = 300                               # records of synth.fastq every case but the first reads

# the conditions on the fixture: (label, test on the case)
def _words(c):
    return c["args"].split()


def _names(c):
    return [w.split("=")[0] for a, w in zip(_words(c), _words(c)[1:]) if a in ("-a", "-b", "-g") and "=" in w]


TALLY = [
    ("2 named", lambda c: len(_names(c)) == 2), ("3 named", lambda c: len(_names(c)) == 3),
    ("12 named", lambda c: len(_names(c)) == 12),
    ("unnamed", lambda c: not _names(c)), ("-g ^", lambda c: any(w.split("=")[-1].startswith("^") for w in _words(c))),
    ("-b", lambda c: "-b" in _words(c)), ("--times 2", lambda c: "-n" in _words(c)),
    ("--no-trim", lambda c: "--no-trim" in _words(c)), ("--mask-adapter", lambda c: "--mask-adapter" in _words(c)),
    ("--untrimmed-output", lambda c: "--untrimmed-output" in _words(c)),
    ("--discard-untrimmed", lambda c: "--discard-untrimmed" in _words(c)),
    ("-m with --too-short-output", lambda c: "--too-short-output" in _words(c)), ("--max-n", lambda c: "--max-n" in _words(c)),
    ("no read matches", lambda c: "nope=" in c["args"] and "out.nope.fastq" not in c["files"]),
    ("every read matches", lambda c: "every=" in c["args"] and "out.unknown.fastq" not in c["files"]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/oracle_ref")
    args = ap.parse_args()
    sys.path.insert(0, args.scratch)
    from atropos.commands import get_command
    import atropos.adapters as ref_adapters
    with gzip.open(os.path.join(HERE, "trim_cases.json.gz"), "rb") as fh:
        inputs = {k: base64.b64decode(v) for k, v in json.loads(fh.read().decode())["inputs"].items()}
    doc = dict(cases=[])
    for idx, (name, argstr) in enumerate(CASES):
        head = HEAD if (idx and name == "synth.fastq") else None
        text = inputs[name] if head is None else b"".join(inputs[name].splitlines(True)[:4 * head])
        named = [w for a, w in zip(argstr.split(), argstr.split()[1:]) if a in ("-a", "-b", "-g")]
        assert all("=" in w for w in named) or not any("=" in w for w in named), argstr
        ref_adapters.ADAPTER_ID_GENERATOR = itertools.count(1)
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, "in.fastq")
            open(src, "wb").write(text)
            filled = argstr
            for kind in KINDS:
                filled = filled.replace("{%s}" % kind, os.path.join(tmp, kind + ".txt"))
            params = filled.split() + ["-se", src, "-o", os.path.join(tmp, "out.{name}.fastq")]
            retcode, summary = get_command("trim").execute(params + ["--quiet", "--no-default-adapters", "--no-cache-adapters"])
            assert retcode == 0 and "exception" not in summary, (argstr, summary.get("exception"))
            files = {}
            for fname in sorted(os.listdir(tmp)):
                if fname == "in.fastq":
                    continue
                key = re.sub(r"^out\.(\d+)\.fastq$", r"out.#\1.fastq", fname)
                files[key] = base64.b64encode(open(os.path.join(tmp, fname), "rb").read()).decode()
        doc["cases"].append(dict(args=argstr, input=name, head=head, files=files))
        print("%-12s %-90s -> %s" % (name, argstr[:90], " ".join(
            "%s:%d" % (k, base64.b64decode(v).count(b"\n") // 4) for k, v in files.items())))
    assert len(doc["cases"]) >= 15
    for label, test in TALLY:
        count = sum(1 for c in doc["cases"] if test(c))
        print("  %-28s %d" % (label, count))
        assert count >= 1, label
    every = next(c for c in doc["cases"] if "every=" in c["args"])
    assert sum(base64.b64decode(v).count(b"\n") for v in every["files"].values()) == inputs[every["input"]].count(b"\n") and every["head"] is None
    assert any(c["input"] == "synth.fastq" for c in doc["cases"]) and any(c["input"] == "small.fastq" for c in doc["cases"])
    out = os.path.join(HERE, "trim_demux.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, sort_keys=True).encode())
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()

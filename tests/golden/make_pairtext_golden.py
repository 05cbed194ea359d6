#!/usr/bin/env python3
"""Generates tests/golden/pairtext.json.gz: every file the REFERENCE's ``atropos trim`` leaves for paired-end runs
that read an interleaved file (``-l``), write one (``-L``), or both -- FastqReader's interleaved mode
(io/seqio.py:470-510) and InterleavedFormatter (io/seqio.py:740-749).  Run in the build container only (the
reference is imported from a scratch build, see make_golden.py --scratch); the committed file holds data only.

The input is made here from a seed and stored in the fixture: ``inputs`` = {"r1", "r2": the two files, "il": the same
pairs interleaved, "il64", "r1_64", "r2_64": with qualities from base 64, "odd": "il" without its last record}, base64.
About 220 pairs of up to 2 x 100 bp named ``.../1`` and ``.../2``; some carry an adapter, some mates are shorter
than their partner, a few reads are very short, a few pairs have low-quality ends and N ends.

Per case: ``args`` (the trimming options), ``input`` ("pair" | "il" and the quality base), ``output`` ("pair" | "il"),
``files`` = {file name: base64 text} of everything the run left next to its inputs.  A paired output is ``out.1.fastq``
and ``out.2.fastq``, an interleaved one ``out.il.fastq``.  ``error``: the message of the exception the run ended
with (the odd file), else null.

``overwrite_read``: the reference's ``OverwriteRead`` modifier (commands/trim/modifiers.py:511-563) called directly on 200
generated pairs (``direct_calls``): its arguments, both reads before and after, or the error it raised.

usage: python tests/golden/make_pairtext_golden.py [--scratch /tmp/oracle_ref]
"""
import argparse
import base64
import gzip
import json
import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
AD1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"
AD2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}

# (trimming options, input kind, output kind, quality base of the input)
BOTH = "-a %s -A %s" % (AD1, AD2)
CASES = [
    (BOTH, "il", "pair", 33),
    (BOTH, "pair", "il", 33),
    (BOTH, "il", "il", 33),
    ("-a %s" % AD1, "il", "pair", 33),                          # -l switches the legacy mode off: read 2 is modified too
    ("-a %s -q 20" % AD1, "il", "il", 33),
    ("-a %s" % AD1, "pair", "il", 33),                          # legacy mode (read 1 alone is modified) with -L
    (BOTH + " --aligner insert", "il", "il", 33),
    (BOTH + " -q 20", "il", "il", 33),
    (BOTH + " --trim-n -m 30", "il", "il", 33),
    (BOTH + " --trim-n -m 30", "pair", "il", 33),
    (BOTH + " --discard-trimmed", "il", "il", 33),
    (BOTH + " --discard-untrimmed", "pair", "il", 33),
    (BOTH + " --discard-untrimmed --pair-filter both", "il", "pair", 33),
    (BOTH + " --mask-adapter", "il", "il", 33),
    (BOTH + " --mask-adapter --trim-n", "pair", "il", 33),
    ("-a first=%s -A second=%s -x pre_{name}_ -y _{name} --length-tag length=" % (AD1, AD2), "il", "il", 33),
    (BOTH + " --length-tag length=", "pair", "il", 33),
    (BOTH + " -q 20 --quality-base 64", "il", "il", 64),
    (BOTH + " -u 3 -U -2 -M 90", "il", "il", 33),
    (BOTH, "odd", "il", 33),
    # --overwrite-low-quality LOWQ,HIGHQ,WINDOW (OverwriteRead, the W of --op-order CGQAW)
    (BOTH + " -w 10,20,20", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --op-order WCGQA -u 5 -U 5", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --aligner insert", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 -q 20", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --trim-n -m 30", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --discard-trimmed", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --discard-untrimmed", "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --mask-adapter", "pair", "pair", 33),
    ("-a first=%s -A second=%s -w 10,20,20 -x pre_{name}_ -y _{name} --length-tag length=" % (AD1, AD2), "pair", "pair", 33),
    (BOTH + " -w 10,20,20 --quality-base 64", "pair", "pair", 64),
    (BOTH + " -w 15,15,20", "pair", "pair", 33),
    (BOTH + " -w 10,20,150", "pair", "pair", 33),
    (BOTH + " -w 10,20,20", "il", "il", 33),
]


def revcomp(seq):
    return "".join(COMP[c] for c in reversed(seq))


def make_pairs(seed=20240611, npairs=220):
    """[(name, seq1, qual1, seq2, qual2)]: inserts of 30 .. 260 bases read from both ends, up to 100 bases each."""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(npairs):
        insert_len = int(rng.integers(30, 261))
        insert = "".join("ACGT"[k] for k in rng.integers(0, 4, insert_len))
        len1 = 100 if i % 7 else int(rng.integers(60, 100))    # mates of different lengths
        len2 = 100 if i % 5 else int(rng.integers(60, 100))
        if i % 41 == 7:
            len1 = int(rng.integers(0, 12))                    # a few very short reads (an empty one among them)
        if i % 43 == 9:
            len2 = int(rng.integers(1, 12))
        filler = lambda n: "".join("ACGT"[k] for k in rng.integers(0, 4, n))
        seq1 = (insert + AD1 + filler(100))[:len1]
        seq2 = (revcomp(insert) + AD2 + filler(100))[:len2]
        reads = []
        for seq in (seq1, seq2):
            seq = list(seq)
            for p in range(len(seq)):
                if rng.random() < 0.01:
                    seq[p] = "ACGT"[int(rng.integers(0, 4))]    # sequencing errors
            if rng.random() < 0.1:
                for p in range(max(len(seq) - int(rng.integers(1, 6)), 0), len(seq)):
                    seq[p] = "N"                               # N ends
            # (mostly one value: the fixture stores ~25 copies of the qualities, and random ones do not compress)
            qual = np.where(rng.random(len(seq)) < 0.1, rng.integers(25, 41, len(seq)), 38)
            if rng.random() < 0.3:
                tail = int(rng.integers(1, 30))
                qual[max(len(seq) - tail, 0):] = rng.integers(2, 15, min(tail, len(seq)))
            reads.append(("".join(seq), qual))
        # a quarter of the pairs: the first 20 qualities of read 1, of read 2 or (some) of both are low
        if i % 4 == 1:
            for k in ((0,), (1,), (0, 1))[(i // 4) % 5 % 3 if (i // 4) % 5 else 2]:
                head = min(20, len(reads[k][1]))
                reads[k][1][:head] = rng.integers(2, 9, head)
        plus = "pair%03d extra" % i if i % 9 == 0 else ""       # some '+' lines repeat the name
        pairs.append(("pair%03d extra" % i, plus, reads[0], reads[1]))
    return pairs


def render(pairs, base, which):
    """FASTQ text of read 1 (which = 1), read 2 (2) or both in turn (0)."""
    out = []
    for name, plus, r1, r2 in pairs:
        for k, (seq, qual) in ((1, r1), (2, r2)):
            if which in (0, k):
                head = name.replace(" ", "/%d " % k)
                two = plus.replace(" ", "/%d " % k)
                out.append("@%s\n%s\n+%s\n%s\n" % (head, seq, two, "".join(chr(int(q) + base) for q in qual)))
    return "".join(out).encode("ascii")


def quals_with_sum(rng, n, window, total, base):
    """n quality characters whose first ``window`` values sum to ``total`` exactly (values 0 .. 41)."""
    vals = np.full(window, total // window)
    vals[:total % window] += 1
    rng.shuffle(vals)
    assert vals.sum() == total and vals.min() >= 0 and vals.max() <= 41
    vals = np.concatenate([vals, rng.integers(2, 41, n - window)])
    return "".join(chr(int(v) + base) for v in vals)


def direct_calls(OverwriteRead, Sequence, seed=77, npairs=200):
    """``OverwriteRead`` called on generated pairs: [{args, before, after, error}]; a read is [name, sequence,
    qualities, name2, corrected].  The window sums sit on lowq * window and highq * window exactly, one below each,
    and far from both; some reads are shorter than the window, the mates' lengths differ, bases are upper- and
    lower-case IUPAC; a few reads hold a base without a complement (the reference's KeyError)."""
    rng = np.random.default_rng(seed)
    out = []
    letters = "ACGT" * 8 + "acgtNnRYSWKMBDHVryswkmbdhv"
    for i in range(npairs):
        lowq, highq, window = [(10, 20, 20), (15, 15, 10), (5, 30, 1), (10, 20, 150)][i % 4 if i % 11 else 3]
        base = 64 if i % 5 == 0 else 33
        sums = (lowq * window - 1, lowq * window, highq * window - 1, highq * window, 2 * window, min(38, highq + 8) * window)
        reads = []
        for k in (1, 2):
            n = int(rng.integers(max(window, 1), max(window, 1) + 80))
            if i % 13 == k:
                n = max(window - 1, 0)                          # shorter than the window
            seq = "".join(letters[j] for j in rng.integers(0, len(letters), n))
            if i % 29 == 3 * k and n:
                seq = seq[:n // 2] + "." + seq[n // 2 + 1:]      # no complement
            total = sums[int(rng.integers(0, len(sums)))]
            qual = quals_with_sum(rng, n, window, total, base) if n >= window else "".join(
                chr(int(v) + base) for v in rng.integers(2, 41, n))
            name = "d%03d/%d tail" % (i, k)
            reads.append(Sequence(name, seq, qual, name if i % 3 == 0 else ""))
        show = lambda r: [r.name, r.sequence, r.qualities, r.name2, int(r.corrected)]
        before = [show(r) for r in reads]
        try:
            got = OverwriteRead(lowq, highq, window, base=base)(*reads)
            after, error = [show(r) for r in got], None
        except KeyError as exc:
            after, error = None, "KeyError"
        out.append(dict(args=[lowq, highq, window, base], before=before, after=after, error=error))
    over1 = sum(1 for c in out if c["after"] and c["after"][0][0] != c["before"][0][0])
    over2 = sum(1 for c in out if c["after"] and c["after"][1][0] != c["before"][1][0])
    longer = sum(1 for c in out if c["after"] and any(a[0] != b[0] and len(a[1]) > len(b[1]) for a, b in zip(c["after"], c["before"])))
    errors = sum(1 for c in out if c["error"])
    print("direct OverwriteRead calls: %d, read 1 overwritten %d, read 2 overwritten %d, clone longer %d, KeyError %d" % (
        len(out), over1, over2, longer, errors))
    assert over1 >= 5 and over2 >= 5 and longer >= 1 and errors >= 1
    assert sum(1 for c in out if c["after"] == c["before"]) >= 20
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/oracle_ref")
    args = ap.parse_args()
    sys.path.insert(0, args.scratch)
    from atropos.commands import get_command
    pairs = make_pairs()
    inputs = dict(r1=render(pairs, 33, 1), r2=render(pairs, 33, 2), il=render(pairs, 33, 0),
                  r1_64=render(pairs, 64, 1), r2_64=render(pairs, 64, 2), il64=render(pairs, 64, 0))
    inputs["odd"] = b"".join(inputs["il"].splitlines(True)[:-4])
    assert inputs["il"].count(b"\n") == 8 * len(pairs) and inputs["odd"].count(b"\n") == 8 * len(pairs) - 4
    doc = dict(inputs={k: base64.b64encode(v).decode() for k, v in inputs.items()}, cases=[])
    from atropos.commands.trim.modifiers import OverwriteRead
    from atropos.io.seqio import Sequence
    doc["overwrite_read"] = direct_calls(OverwriteRead, Sequence)
    for argstr, kind_in, kind_out, base in CASES:
        sfx = "_64" if base == 64 else ""
        with tempfile.TemporaryDirectory() as tmp:
            params = argstr.split()
            if kind_in == "pair":
                for flag, key in (("-pe1", "r1" + sfx), ("-pe2", "r2" + sfx)):
                    path = os.path.join(tmp, "in.%s.fastq" % key)
                    open(path, "wb").write(inputs[key])
                    params += [flag, path]
            else:
                key = "odd" if kind_in == "odd" else ("il64" if base == 64 else "il")
                path = os.path.join(tmp, "in.il.fastq")
                open(path, "wb").write(inputs[key])
                params += ["-l", path]
            if kind_out == "pair":
                params += ["-o", os.path.join(tmp, "out.1.fastq"), "-p", os.path.join(tmp, "out.2.fastq")]
            else:
                params += ["-L", os.path.join(tmp, "out.il.fastq")]
            seen = []
            catch = logging.Handler()
            catch.emit = seen.append                           # (the runner logs the exception that ends a run)
            logging.getLogger().addHandler(catch)
            try:
                retcode, summary = get_command("trim").execute(params + ["--quiet", "--no-default-adapters", "--no-cache-adapters"])
            finally:
                logging.getLogger().removeHandler(catch)
            error = summary["exception"]["message"] if "exception" in summary else None
            if error is None and retcode != 0:
                error = next(str(rec.exc_info[1]) for rec in seen if rec.exc_info)
            assert (retcode == 0) == (error is None), (argstr, error)
            assert (error is not None) == (kind_in == "odd"), (argstr, error)
            files = {f: base64.b64encode(open(os.path.join(tmp, f), "rb").read()).decode()
                     for f in sorted(os.listdir(tmp)) if f.startswith("out.")}
        doc["cases"].append(dict(args=argstr, input=kind_in, output=kind_out, base=base, files=files, error=error))
        print("%-4s -> %-4s %-100s %s %s" % (kind_in, kind_out, argstr[:100], " ".join(
            "%s:%d" % (k, base64.b64decode(v).count(b"\n") // 4) for k, v in files.items()), error or ""))
    # what the fixture must contain: OverwriteRead
    def names(c, f):
        return [l.split()[0] for l in base64.b64decode(c["files"][f]).decode().splitlines()[0::4]]
    wcase = lambda extra: next(c for c in doc["cases"] if c["args"] == BOTH + " -w 10,20,20" + extra and c["input"] == "pair")
    plainw = wcase("")
    over = [{n[1:8] for n in names(plainw, f) if not n.endswith("/%d" % k)} for k, f in ((1, "out.1.fastq"), (2, "out.2.fastq"))]
    print("overwritten in the default -w case: read 1 %d, read 2 %d" % (len(over[0]), len(over[1])))
    assert len(over[0]) >= 5 and len(over[1]) >= 5 and not over[0] & over[1]
    kept = {n[1:8] for n in names(wcase(" --trim-n -m 30"), "out.1.fastq")} | {n[1:8] for n in names(wcase(" --discard-trimmed"), "out.1.fastq")}
    assert (over[0] | over[1]) - {n[1:8] for n in names(wcase(" --discard-trimmed"), "out.1.fastq")}, "an overwritten read a filter drops"
    by_name = {}
    for name, plus, r1, r2 in pairs:
        by_name[name.split()[0]] = (len(r1[0]), len(r2[0]))
    assert any(by_name["pair" + p[4:]][1] > by_name["pair" + p[4:]][0] for p in over[0]) or any(
        by_name["pair" + p[4:]][0] > by_name["pair" + p[4:]][1] for p in over[1]), "a clone longer than the read it replaces"
    assert names(wcase(""), "out.1.fastq") != names(next(c for c in doc["cases"] if "-w 10,20,150" in c["args"]), "out.1.fastq")
    # ... and the interleaved files
    text = lambda c, f: base64.b64decode(c["files"][f])
    plain = next(c for c in doc["cases"] if c["args"] == BOTH and c["input"] == "il" and c["output"] == "il")
    split = next(c for c in doc["cases"] if c["args"] == BOTH and c["input"] == "il" and c["output"] == "pair")
    lines = text(plain, "out.il.fastq").splitlines(True)
    assert len(lines) == 8 * len(pairs)
    assert b"".join(l for k, l in enumerate(lines) if k % 8 < 4) == text(split, "out.1.fastq")       # -L is -o and -p in turn
    assert b"".join(l for k, l in enumerate(lines) if k % 8 >= 4) == text(split, "out.2.fastq")
    assert text(plain, "out.il.fastq") != inputs["il"]                                              # something was trimmed
    assert any(b"\n\n" in text(c, f) for c in doc["cases"] for f in c["files"])                     # an empty read is written
    dropped = [c for c in doc["cases"] if c["output"] == "il" and c["error"] is None and
               0 < text(c, "out.il.fastq").count(b"\n") < 8 * len(pairs)]
    assert len(dropped) >= 4, len(dropped)                                                          # filters drop whole pairs
    masked = next(c for c in doc["cases"] if "--mask-adapter" in c["args"] and c["output"] == "il")
    assert text(masked, "out.il.fastq").count(b"NNNNNNNN") > 15
    assert sum(c["error"] is not None for c in doc["cases"]) == 1
    out = os.path.join(HERE, "pairtext.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, sort_keys=True).encode())
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()

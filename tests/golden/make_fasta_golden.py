#!/usr/bin/env python3
"""Generates tests/golden/fasta.json.gz: every file the REFERENCE's ``atropos trim`` leaves for runs that read FASTA
(FastaReader, io/seqio.py:233-280) or write it (FastaFormat, io/seqio.py:1008-1067), and the message of the runs it
ends with an error.  Run in the build container only (the reference is imported from a scratch build, see
make_golden.py --scratch); the committed file holds data only.

The inputs are made here from a seed and stored in the fixture (``inputs``, base64), about 200 reads of up to 100 bp,
some with an adapter, N ends, very short ones, empty ones, one with an empty name, one with a blank inside:
  two    two-line FASTA;
  wrap   the same reads wrapped at 7, 60 and 70, mixed per record;
  messy  the same reads with CRLF and lone CR line ends, blank lines and '#' lines between sequence lines, leading and
         trailing blanks and tabs, ' >' headers, header-only records (the last one among them), no final line end;
  fq     the same reads as FASTQ;
  r1, r2 the paired cases' two files (two-line FASTA), r2w = r2 wrapped;
  bad    text in front of the first header, behind a blank line and a '#' line.

Per case: ``args`` (the trimming options; a token that begins with ``out.`` is a file next to the inputs), ``input``
(the key of the input, or two keys), ``files`` = {file name: base64 text} of everything the run left, ``error`` =
[exception type, message] or null.  The main output is ``out.fasta`` (``out.1.fasta`` / ``out.2.fasta`` for pairs)
unless ``output`` names it otherwise.

usage: python tests/golden/make_fasta_golden.py [--scratch /tmp/oracle_ref]
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
FRONT = "TTAGGCATCGGA"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
SIDE = " --info-file out.info --rest-file out.rest --wildcard-file out.wild"

# (trimming options, input key or (key 1, key 2), main output or (output 1, output 2))
SINGLE = [
    ("-a %s" % AD1,),
    ("-a %s -n 2 -e 0.2 -O 5" % AD1,),
    ("-g %s -a %s" % (FRONT, AD1),),
    ("-b %s --no-indels" % AD1,),
    ("-a %s -N" % AD1[:13].replace("G", "N", 1),),
    ("-a wild=AGATCGGNNGAGC --match-read-wildcards" + SIDE,),      # (named: the reference numbers unnamed adapters per process)
    ("-a ^%s...%s" % (FRONT, AD1[:13]),),
    ("-g ^%s" % FRONT,),
    ("-a %s$" % AD1[:13],),
    ("-a %s --no-trim" % AD1,),
    ("-a %s --mask-adapter --trim-n" % AD1,),
    ("-a %s -u 3 -u -2 --trim-n" % AD1,),
    ("-a %s --cut-min 5" % AD1,),
    ("-a %s --bisulfite rrbs" % AD1,),
    ("-a %s -m 30 -M 90 --max-n 2" % AD1,),
    ("-a %s --discard-trimmed" % AD1,),
    ("-a %s --discard-untrimmed" % AD1,),
    ("-a first=%s -x pre_{name}_ -y _{name} --length-tag length= --strip-suffix extra" % AD1,),
    ("-a %s -z" % AD1,),
    ("-a ad=%s" % AD1 + SIDE,),
    ("-a %s -m 30 -M 90 --too-short-output out.short.fasta --too-long-output out.long.fasta --untrimmed-output out.untrimmed.fasta" % AD1,),
    ("-a %s -m 30 --too-short-output out.short" % AD1, None, "out.reads"),              # names that say nothing: FASTA
]
PAIRED = [
    ("-a %s -A %s" % (AD1, AD2),),
    ("-a %s -A %s --aligner insert" % (AD1, AD2),),
    ("-a %s -A %s -U 2 --trim-n -m 30 --pair-filter both" % (AD1, AD2),),
    ("-a %s -A %s -m 40 --too-short-output out.short.1.fasta --too-short-paired-output out.short.2.fasta" % (AD1, AD2),),
    ("-a %s" % AD1,),                                                                  # legacy mode
]


def revcomp(seq):
    return "".join(COMP[c] for c in reversed(seq))


def make_reads(seed=20241020, n=200):
    """[(name, sequence)]"""
    rng = np.random.default_rng(seed)
    fill = lambda k: "".join("ACGT"[j] for j in rng.integers(0, 4, k))
    reads = []
    for i in range(n):
        insert = fill(int(rng.integers(10, 120)))
        seq = (insert + AD1 + fill(100))[:100 if i % 6 else int(rng.integers(40, 100))]
        if i % 10 == 3:
            seq = FRONT + seq[:-len(FRONT)]
        seq = list(seq)
        for p in range(len(seq)):
            if rng.random() < 0.01:
                seq[p] = "ACGT"[int(rng.integers(0, 4))]
        if rng.random() < 0.15:
            for p in range(max(len(seq) - int(rng.integers(1, 6)), 0), len(seq)):
                seq[p] = "N"
        if i % 17 == 5:
            seq[:2] = "NN"
        seq = "".join(seq)
        if i % 37 == 11:
            seq = seq[:int(rng.integers(1, 9))]                  # very short
        if i % 53 == 20:
            seq = ""                                            # empty
        if i % 29 == 9:
            seq = seq.lower()
        name = "read%03d extra" % i if i % 3 else "read%03d" % i
        if i == 77:
            name = ""
        if i == 120:
            seq = "NNACGT acgt"                                 # a blank inside the line stays
        reads.append((name, seq))
    reads[-1] = (reads[-1][0], "")                              # the last record is a header alone
    return reads


def make_pairs(seed=20241021, n=200):
    rng = np.random.default_rng(seed)
    fill = lambda k: "".join("ACGT"[j] for j in rng.integers(0, 4, k))
    r1, r2 = [], []
    for i in range(n):
        insert = fill(int(rng.integers(30, 200)))
        len1 = 100 if i % 7 else int(rng.integers(60, 100))
        len2 = 100 if i % 5 else int(rng.integers(60, 100))
        if i % 41 == 7:
            len1 = int(rng.integers(0, 12))
        s1 = list((insert + AD1 + fill(100))[:len1])
        s2 = list((revcomp(insert) + AD2 + fill(100))[:len2])
        for s in (s1, s2):
            for p in range(len(s)):
                if rng.random() < 0.01:
                    s[p] = "ACGT"[int(rng.integers(0, 4))]
            if rng.random() < 0.1:
                for p in range(max(len(s) - int(rng.integers(1, 6)), 0), len(s)):
                    s[p] = "N"
        r1.append(("pair%03d/1 extra" % i, "".join(s1)))
        r2.append(("pair%03d/2 extra" % i, "".join(s2)))
    return r1, r2


def two_line(reads):
    return "".join(">%s\n%s\n" % r for r in reads).encode("ascii")


def wrapped(reads):
    out = []
    for i, (name, seq) in enumerate(reads):
        width = (7, 60, 70, 1000)[i % 4] if " " not in seq else 1000
        out.append(">%s\n" % name)
        out.extend(seq[k:k + width] + "\n" for k in range(0, len(seq), width))
        if not seq and i % 2:
            out.append("\n")
    return "".join(out).encode("ascii")


def messy(reads, seed=5):
    rng = np.random.default_rng(seed)
    out = ["\n", "# a comment in front of the first record\r\n", "  \t\n"]
    for i, (name, seq) in enumerate(reads):
        end = ("\n", "\r\n", "\r")[i % 3]
        head = (">", " >", "\t>", ">")[i % 4] + name + ("", " ", "\t ", "")[(i // 4) % 4]
        out.append(head + end)
        width = int(rng.integers(5, 80)) if " " not in seq else 1000
        pieces = [seq[k:k + width] for k in range(0, len(seq), width)]
        for k, piece in enumerate(pieces):
            if i % 5 == 1 and k:
                out.append(("\n", "#skipped\n", " \t \r\n", "\x0b\x0c\n")[(i + k) % 4])
            out.append(("", " ", "\t", "\x1c\x1f")[(i + k) % 4] + piece + ("", "  ", "\t", "\x1d ")[(i // 2 + k) % 4] + end)
        if i % 11 == 2:
            out.append("\n#tail comment\n")
    # (a lone "\r" in front of an inserted blank line reads as one "\r\n": a line end less, the same records)
    return "".join(out).rstrip("\r\n").encode("ascii")          # no final line end (the last record is a header alone)


def fastq(reads):
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in reads).encode("ascii")


def run(get_command, inputs, argstr, keys, outs):
    with tempfile.TemporaryDirectory() as tmp:
        params = [os.path.join(tmp, t) if t.startswith("out.") else t for t in argstr.split()]
        flags = ("-se",) if len(keys) == 1 else ("-pe1", "-pe2")
        for flag, key in zip(flags, keys):
            path = os.path.join(tmp, "in.%s.%s" % (key, "fastq" if key == "fq" else "fasta"))
            open(path, "wb").write(inputs[key])
            params += [flag, path]
        for flag, name in zip(("-o", "-p"), outs):
            params += [flag, os.path.join(tmp, name)]
        seen = []
        catch = logging.Handler()
        catch.emit = seen.append                               # (the runner logs the exception that ends a run)
        logging.getLogger().addHandler(catch)
        error = None
        try:
            retcode, summary = get_command("trim").execute(params + ["--quiet", "--no-default-adapters", "--no-cache-adapters"])
            if "exception" in summary:
                error = [summary["exception"]["details"][0].__name__, summary["exception"]["message"]]
            elif retcode != 0:
                exc = next(rec.exc_info[1] for rec in seen if rec.exc_info)
                error = [type(exc).__name__, str(exc)]
        except Exception as exc:                               # (raised while the command was put together)
            error = [type(exc).__name__, str(exc)]
        finally:
            logging.getLogger().removeHandler(catch)
        files = {f: base64.b64encode(open(os.path.join(tmp, f), "rb").read()).decode()
                 for f in sorted(os.listdir(tmp)) if f.startswith("out.")}
    return files, error


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/oracle_ref")
    args = ap.parse_args()
    sys.path.insert(0, args.scratch)
    from atropos.commands import get_command
    reads = make_reads()
    r1, r2 = make_pairs()
    inputs = dict(two=two_line(reads), wrap=wrapped(reads), messy=messy(reads), fq=fastq(reads), r1=two_line(r1),
                  r2=two_line(r2), r2w=wrapped(r2),
                  bad=b"\n#comment\nACGTACGT\n>r1\nACGT\n")
    doc = dict(inputs={k: base64.b64encode(v).decode() for k, v in inputs.items()}, cases=[])

    def add(argstr, keys, outs):
        files, error = run(get_command, inputs, argstr, keys, outs)
        doc["cases"].append(dict(args=argstr, input=list(keys), output=list(outs), files=files, error=error))
        print("%-10s %-90s %s %s" % ("+".join(keys), argstr[:90], " ".join(
            "%s:%d" % (k, len(base64.b64decode(v))) for k, v in files.items()), error or ""))
        return files

    for case in SINGLE:
        argstr = case[0]
        out = case[2] if len(case) > 2 else "out.fasta"
        same = [add(argstr, (key,), (out,)) for key in ("two", "wrap", "messy")]
        assert same[0] == same[1] == same[2], argstr            # the same reads however they are written
        assert same[0], argstr
    for case in PAIRED:
        a = add(case[0], ("r1", "r2"), ("out.1.fasta", "out.2.fasta"))
        b = add(case[0], ("r1", "r2w"), ("out.1.fasta", "out.2.fasta"))
        assert a == b and a
    # FASTQ in, FASTA out (by the output's name), with a FASTA side file; and FASTA in, FASTQ-named out
    add("-a %s -m 30 --too-short-output out.short.fa" % AD1, ("fq",), ("out.fna",))
    add("-a %s --mask-adapter" % AD1, ("fq",), ("out.fasta",))
    add("-a %s" % AD1, ("two",), ("out.fastq",))
    add("-a %s" % AD1, ("bad",), ("out.fasta",))
    errors = [c for c in doc["cases"] if c["error"]]
    assert len(errors) == 2, errors
    assert errors[0]["error"][1] == "Output format cannot be FASTQ since no quality values are available."
    assert errors[1]["error"][1] == "At line 3: Expected '>' at beginning of FASTA record, but got 'ACGTACGT'."
    text = lambda c, f: base64.b64decode(c["files"][f])
    plain = doc["cases"][0]
    assert text(plain, "out.fasta").count(b">") == len(reads) and text(plain, "out.fasta") != inputs["two"]
    assert b">\n" in text(plain, "out.fasta") and b"\n\n" in text(plain, "out.fasta")        # empty name, empty read
    assert b"NNACGT acgt\n" in text(plain, "out.fasta")
    masked = next(c for c in doc["cases"] if c["args"].endswith("--mask-adapter"))
    assert text(masked, "out.fasta").count(b"NNNNNNNN") > 15
    fq_case = next(c for c in doc["cases"] if c["input"] == ["fq"] and "--mask" not in c["args"])
    assert text(fq_case, "out.fna").startswith(b">") and text(fq_case, "out.short.fa").startswith(b">")
    info = next(c for c in doc["cases"] if c["args"].endswith(SIDE) and c["input"] == ["two"])
    assert any(line.endswith(b"\t\t\t") for line in text(info, "out.info").splitlines())      # empty quality columns
    out = os.path.join(HERE, "fasta.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as fh:
        fh.write(json.dumps(doc, sort_keys=True).encode())
    print("wrote", out, os.path.getsize(out), "bytes,", len(doc["cases"]), "cases")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()

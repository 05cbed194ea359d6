#!/usr/bin/env python3
"""Known-contaminant detection on one MI355X: reads/s of the three passes (filter, distinct, match) and of the whole
``add_batch`` + counters on a resident batch, of ``atr_read_stats_batch`` on the same batch (a kernel that also
reads every base once), and of ``detect_file`` file to result.  Prints one JSON line.

``--detector heuristic``: the de-novo discovery instead (no list is needed; without one two Illumina adapters are
planted): reads/s of ``discover`` + ``matches`` on a resident batch and the seconds of each stage -- filter, distinct,
rank (the rounds up to kmer_size), levels (the level loop), gather, support and host (merge, known matching, report).

usage: python tools/bench_detect.py --known LIST.fa [--reads 10000000] [--length 150] [--steps 5] [--warmup 2] [--file]
       python tools/bench_detect.py --detector heuristic [--known LIST.fa] [--reads 10000] ...
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from atropos_amd import _lib, detect, stats, synth  # noqa: E402
from atropos_amd.fastq import FastqBatch  # noqa: E402


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


PLANTED = ("AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCACGATCTCGTATGCCGTCTTCTGCTTG",
           "CTGTCTCTTATACACATCTCCGAGCCCACGAGACTAAGGCGAATCTCGTATGCCGTCTTCTGCTTG")


def heuristic(args):
    known = detect.KnownContaminants.from_fasta(args.known) if args.known else None
    planted = [s for s in known.sequences if len(s) >= 30] if known else list(PLANTED)
    rec = synth.contaminated_fastq(args.reads, 1, planted, args.length)
    be = _lib.get_backend()
    batch, _ = FastqBatch.from_bytes(rec.tobytes(), backend=be)
    n = len(batch)
    names = ("filter", "distinct", "rank", "levels", "gather", "support", "host")
    stages, whole = {k: [] for k in names}, []
    for step in range(args.warmup + args.steps):
        det = detect.HeuristicDetector(known, n_reads=n, backend=be)
        det.add_batch(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        matches = det.matches()
        dt = time.perf_counter() - t0
        found = det.discover(timed=True)
        seconds = dict(det.timings)
        t0 = time.perf_counter()
        merged = detect.merge_candidates(list(det.candidates().items()))
        t1 = time.perf_counter()
        det.support([x[0] for x in merged])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        det.matches()
        seconds["support"] = t2 - t1
        seconds["host"] = (t1 - t0) + max(0.0, (time.perf_counter() - t2) - (t2 - t0))
        if step >= args.warmup:
            whole.append(n / dt)
            for k in names:
                stages[k].append(seconds.get(k, 0.0))
        det.close()
    print(json.dumps(dict(detector="heuristic", reads=n, length=args.length, kept=found["kept"], distinct=found["distinct"],
                          levels=found["levels"], candidates=int(found["rows"].shape[0]),
                          matches=[[m.seq, m.count, m.abundance] for m in matches[:4]],
                          matches_reads_per_s=spread(whole), stage_seconds={k: spread(v) for k, v in stages.items()},
                          steps=args.steps, warmup=args.warmup)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--known", default=None, help="FASTA file of known contaminants (optional with --detector heuristic)")
    ap.add_argument("--detector", default="known", choices=("known", "heuristic"))
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--file", action="store_true", help="also time detect_file on a temporary file")
    args = ap.parse_args()
    if args.detector == "heuristic":
        return heuristic(args)
    if not args.known:
        ap.error("--known is required with --detector known")
    known = detect.KnownContaminants.from_fasta(args.known)
    rec = synth.contaminated_fastq(args.reads, 1, [s for s in known.sequences if len(s) >= 30], args.length)
    be = _lib.get_backend()
    batch, _ = FastqBatch.from_bytes(rec.tobytes(), backend=be)
    n = len(batch)
    passes, whole, st_times = {"filter": [], "distinct": [], "match": []}, [], []
    for step in range(args.warmup + args.steps):
        det = detect.KnownContaminantDetector(known, n_reads=n, backend=be)
        det.add_batch(batch)
        if step == 0:
            det.counters()                                    # (builds the tables: not part of a step)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = det.counters(recompute=True)
        dt = time.perf_counter() - t0
        det.counters(timed=True)
        rs = stats.ReadStatistics(qualities=True, backend=be)
        if step == 0:
            rs.collect_batch(batch)                           # (allocates the block)
            rs = stats.ReadStatistics(qualities=True, backend=be)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rs.collect_batch(batch)
        torch.cuda.synchronize()
        ds = time.perf_counter() - t0
        if step >= args.warmup:
            whole.append(n / dt)
            st_times.append(n / ds)
            for k in passes:
                passes[k].append(n / det.timings[k])
        det.close()
    out = dict(reads=n, length=args.length, kept=c["kept"], distinct=c["distinct"], hits=int(c["hits"].sum()),
               add_batch_reads_per_s=spread(whole), read_stats_reads_per_s=spread(st_times),
               passes_reads_per_s={k: spread(v) for k, v in passes.items()}, steps=args.steps, warmup=args.warmup)
    if args.file:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "reads.fastq")
            with open(path, "wb") as fh:
                fh.write(rec.tobytes())
            times = []
            for step in range(1 + min(args.steps, 3)):
                t0 = time.perf_counter()
                detect.detect_file(path, known, max_reads=None, n_reads=n)
                if step:
                    times.append(n / (time.perf_counter() - t0))
            out["detect_file_reads_per_s"] = spread(times)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Known-contaminant detection on one MI355X: reads/s of the three passes (filter, distinct, match) and of the whole
``add_batch`` + counters on a resident batch, of ``atr_read_stats_batch`` on the same batch (a kernel that also
reads every base once), and of ``detect_file`` file to result.  Prints one JSON line.

usage: python tools/bench_detect.py --known LIST.fa [--reads 10000000] [--length 150] [--steps 5] [--warmup 2] [--file]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--known", required=True, help="FASTA file of known contaminants")
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--file", action="store_true", help="also time detect_file on a temporary file")
    args = ap.parse_args()
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

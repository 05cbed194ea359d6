#!/usr/bin/env python3
"""Read statistics rates (atropos_amd.stats): (a) a resident, indexed chunk of C2-like 150 bp reads with
qualities, device events around each repetition -- "kernels": the atr_read_stats_batch call alone (the two
kernels), "collect_batch": ReadStatistics.collect_batch (adds the host's read of the longest kept length, one
device sync); (b) qc_file, file to summary; (c) trim_file with stats=("pre", "post") against without, on the same
file.  Prints one JSON line.

usage: tools/bench_stats.py [nreads] [reps] [--ref-qc-rate READS_PER_S]
  --ref-qc-rate: the reference's `atropos qc` rate on one CPU core, measured separately (it is not run here), for
  the ratio; --ref-qc-note: how it was measured."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from atropos_amd import stats as S                     # noqa: E402
from atropos_amd.fastq import FastqBatch               # noqa: E402
from atropos_amd.trim import pipeline_from_args        # noqa: E402
from bench_fastq import device_fastq                   # noqa: E402

HBM_BPS = 6.29e12                                      # bytes read per second at the roofline (ADVICE / DESIGN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nreads", nargs="?", type=int, default=10_000_000)
    ap.add_argument("reps", nargs="?", type=int, default=20)
    ap.add_argument("--file-reads", type=int, default=4_000_000)
    ap.add_argument("--ref-qc-rate", type=float, default=None)
    ap.add_argument("--ref-qc-note", default=None)
    args = ap.parse_args()
    out = {}
    # (a) device-resident
    data, nbytes = device_fastq(args.nreads)
    batch, _ = FastqBatch.from_device(data, nbytes)
    st = S.ReadStatistics(qualities=True)
    st.collect_batch(batch)                             # warm-up; sizes the block
    be = st.backend
    lens = batch.seq_lens
    longest = int(lens.max().item())
    read_bytes = int(2 * lens.to(torch.int64).sum().item())          # sequence + quality bytes, each read twice

    def timed(call):
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        ms = times[len(times) // 2]
        return dict(ms_median=ms, ms_min=times[0], ms_max=times[-1], reads_per_s=args.nreads / ms * 1e3,
                    roofline_fraction_one_pass=read_bytes / (ms * 1e-3) / HBM_BPS)

    out["resident"] = dict(reads=args.nreads, reps=args.reps, bytes_per_pass=read_bytes,
                           kernels=timed(lambda: be.read_stats_batch(st._block, st._cap, longest, 33, batch.data,
                                                                     batch.records, index_base=st.reads)),
                           collect_batch=timed(lambda: st.collect_batch(batch)))
    assert st.counts()["count"] == args.nreads * (2 * args.reps + 1)
    # (b) / (c) file based, on the same C2-like text
    text = bytes(data[:nbytes].cpu().numpy().tobytes()) if args.file_reads == args.nreads else None
    del batch, data, st
    if text is None:
        d, nb = device_fastq(args.file_reads)
        text = bytes(d[:nb].cpu().numpy().tobytes())
        del d
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "out.fastq")
        with open(src, "wb") as fh:
            fh.write(text)
        S.qc_file(src)                                  # warm-up
        t0 = time.perf_counter()
        S.qc_file(src)
        sec = time.perf_counter() - t0
        out["qc_file"] = dict(reads=args.file_reads, seconds=sec, reads_per_s=args.file_reads / sec,
                              file_bytes=len(text))
        if args.ref_qc_rate:
            out["qc_file"]["reference_qc_one_core_reads_per_s"] = args.ref_qc_rate
            out["qc_file"]["speedup_vs_reference_one_core"] = args.file_reads / sec / args.ref_qc_rate
            if args.ref_qc_note:
                out["qc_file"]["reference_note"] = args.ref_qc_note
        trim = {}
        for label, stats in (("without", None), ("pre_post", ("pre", "post"))):
            pipe = pipeline_from_args("-a AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC -q 20 --trim-n -m 20")
            pipe.stats = stats or ()
            pipe.trim_file(src, dst)                    # warm-up
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                pipe.trim_file(src, dst)
                sec = time.perf_counter() - t0
                best = sec if best is None else min(best, sec)
            trim[label] = dict(seconds_best_of_3=best, reads_per_s=args.file_reads / best)
        trim["overhead"] = trim["pre_post"]["seconds_best_of_3"] / trim["without"]["seconds_best_of_3"] - 1
        out["trim_file"] = trim
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

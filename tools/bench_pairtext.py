#!/usr/bin/env python3
"""Interleaved output on one MI355X: N pairs of 2 x 150 bp as FASTQ text in HBM (tools/bench_fastq.py's generator),
after the paired adapter stage (-a / -A), formatted

  (a) pairs : one call pair of atr_fastq_emit_pairs (sizing + writing) -- what ``-L`` does per chunk
  (b) two   : the two call pairs of atr_fastq_emit that a two-file output makes on the same batches

once with the two reads in two chunks (two input files) and once with both in one chunk (an interleaved input).
Both as the backend methods run them (work and output buffers allocated per call, the total read back between the
two calls).  The two sides ALTERNATE, run by run, inside one process; every run sits between device
synchronisations; warm-up runs first.  Prints the median and the spread (min .. max) in milliseconds per side.

Then the paired pipeline's ``run`` with and without ``-w 10,20,20`` (the overwrite stage) on the same two chunks, a
tenth of the pairs overwritten, alternating as above.

``--files``: also ``trim_files`` file to file, ``-l`` in and ``-L`` out against two files in and two out on the
same reads (files under --dir, page cache warm, alternating): an I/O-bound figure.
usage: tools/bench_pairtext.py [npairs] [runs] [warmup] [--files] [--dir DIR]"""
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from atropos_amd import _lib                           # noqa: E402
from atropos_amd.fastq import FastqBatch               # noqa: E402
from atropos_amd.trim import pipeline_from_args        # noqa: E402
from bench_fastq import device_fastq                   # noqa: E402

ARGS = "-a AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC -A AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"


def alternate(fns, runs, warmup):
    """{name: [ms]}: the functions in turn, run after run, each between device synchronisations."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def bench_formatter(be, layout, b1, b2, runs, warmup):
    res = pipeline_from_args(ARGS, paired_input=True).run(b1, b2)
    reads = (res.read1, res.read2)

    def pairs():
        return res.device_text_interleaved(_lib.DEST_KEEP)

    def two():
        return [be.fastq_emit(r.batch.data, r.batch.records, r.begin, r.end, r.ubegin, r.uend, r.dest, _lib.DEST_KEEP)
                for r in reads]

    text, parts = pairs(), two()                                # the two sides move the same bytes
    out_bytes = int(text.numel())
    assert out_bytes == sum(int(p.numel()) for p in parts)
    del text, parts
    ms = alternate(dict(pairs=pairs, two=two), runs, warmup)
    row = dict(what="formatter", layout=layout, npairs=len(b1), out_bytes=out_bytes, runs=runs,
               pairs_ms=summary(ms["pairs"]), two_ms=summary(ms["two"]))
    row["pairs_GBps_out"] = out_bytes / row["pairs_ms"]["median"] / 1e6
    row["two_GBps_out"] = out_bytes / row["two_ms"]["median"] / 1e6
    print(json.dumps(row), flush=True)
    return row


def bench_overwrite(be, npairs, runs, warmup):
    """The paired pipeline (adapter stage and filters, no formatting) with and without -w 10,20,20 on the same two
    chunks; every tenth pair has the first 20 qualities of one read (read 1 and read 2 in turn) set low."""
    data1, n1 = device_fastq(npairs)
    data2 = data1.clone()
    width = n1 // npairs
    qual_at = width - 151                                         # (fixed-width records: the quality line is last)
    low = torch.arange(0, npairs, 20, device=data1.device)
    data1[:n1].view(npairs, width)[low, qual_at:qual_at + 20] = 35
    data2[:n1].view(npairs, width)[low + 10, qual_at:qual_at + 20] = 35
    b1, _ = FastqBatch.from_device(data1, n1, True, be)
    b2, _ = FastqBatch.from_device(data2, n1, True, be)
    plain = pipeline_from_args(ARGS, paired_input=True)
    over = pipeline_from_args(ARGS + " -w 10,20,20", paired_input=True)
    over.run(b1, b2)
    share = sum(over.overwritten) / float(npairs)
    ms = alternate(dict(plain=lambda: plain.run(b1, b2), overwrite=lambda: over.run(b1, b2)), runs, warmup)
    row = dict(what="overwrite_stage", npairs=npairs, runs=runs, overwritten_share=share, plain_ms=summary(ms["plain"]),
               overwrite_ms=summary(ms["overwrite"]))
    print(json.dumps(row), flush=True)
    return row


def bench_files(be, npairs, runs, warmup, where):
    data1, n1 = device_fastq(npairs)
    b1, _ = FastqBatch.from_device(data1, n1, True, be)
    width = n1 // npairs
    host = data1[:n1].cpu()
    il = host.view(npairs, width).repeat_interleave(2, dim=0).contiguous().view(-1)
    paths = {k: os.path.join(where, "pairtext_bench." + k) for k in ("r1", "r2", "il", "o1", "o2", "oil")}
    for key, t in (("r1", host), ("r2", host), ("il", il)):
        with open(paths[key], "wb") as fh:
            fh.write(t.numpy().tobytes())
    del data1, b1, host, il
    pipe = pipeline_from_args(ARGS, paired_input=True)
    ms = alternate(dict(interleaved=lambda: pipe.trim_files(paths["il"], None, paths["oil"], keep_output=True),
                        two_files=lambda: pipe.trim_files(paths["r1"], paths["r2"], paths["o1"], paths["o2"], keep_output=True)),
                   runs, warmup)
    assert os.path.getsize(paths["oil"]) == os.path.getsize(paths["o1"]) + os.path.getsize(paths["o2"])
    row = dict(what="file_to_file", npairs=npairs, runs=runs, in_bytes=2 * n1, interleaved_ms=summary(ms["interleaved"]),
               two_files_ms=summary(ms["two_files"]))
    print(json.dumps(row), flush=True)
    for p in paths.values():
        os.unlink(p)
    return row


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    where = None
    if "--dir" in sys.argv:
        where = sys.argv[sys.argv.index("--dir") + 1]
        argv.remove(where)
    npairs = int(argv[0]) if len(argv) > 0 else 4_000_000
    runs = int(argv[1]) if len(argv) > 1 else 9
    warmup = int(argv[2]) if len(argv) > 2 else 2
    be = _lib.get_backend()
    data1, n1 = device_fastq(npairs)
    b1, _ = FastqBatch.from_device(data1, n1, True, be)
    b2, _ = FastqBatch.from_device(data1.clone(), n1, True, be)
    rows = [bench_formatter(be, "two chunks", b1, b2, runs, warmup)]
    del data1, b1, b2
    data, n = device_fastq(2 * npairs)
    m1, m2 = FastqBatch.from_device(data, n, True, be)[0].mates()
    rows.append(bench_formatter(be, "one interleaved chunk", m1, m2, runs, warmup))
    del data, m1, m2
    print("| layout | pairs | atr_fastq_emit_pairs: median (min .. max) ms | 2 x atr_fastq_emit: median (min .. max) ms | pairs / two |")
    print("|---|---|---|---|---|")
    for r in rows:
        a, b = r["pairs_ms"], r["two_ms"]
        print("| %s | %d | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.2f |" % (
            r["layout"], r["npairs"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"], a["median"] / b["median"]))
    torch.cuda.empty_cache()
    r = bench_overwrite(be, npairs, runs, warmup)
    a, b = r["plain_ms"], r["overwrite_ms"]
    print("| paired pipeline, %d pairs, %.1f %% overwritten | without -w: %.2f (%.2f .. %.2f) ms | with -w 10,20,20: %.2f (%.2f .. %.2f) ms |" % (
        r["npairs"], 100 * r["overwritten_share"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"]))
    if "--files" in sys.argv:
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory(dir=where) as tmp:
            r = bench_files(be, npairs, max(runs // 2, 3), 1, tmp)
        a, b = r["interleaved_ms"], r["two_files_ms"]
        print("| file to file, %d pairs | -l in, -L out: %.0f (%.0f .. %.0f) ms | two in, two out: %.0f (%.0f .. %.0f) ms |" % (
            r["npairs"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"]))


if __name__ == "__main__":
    main()

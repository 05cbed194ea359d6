#!/usr/bin/env python3
"""Demultiplexed output of one resident chunk on one MI355X: N reads x 150 bp as FASTQ text in HBM
(tools/bench_fastq.py's generator), every record with a uniformly random output of G, for G in 2, 8, 96, 384:

  (a) grouped : one call pair of atr_fastq_emit_grouped (sizing + writing)
  (b) loop    : G call pairs of atr_fastq_emit over the same chunk with dest = the group -- what there was before
                the grouped formatter.  dest is a byte, so beyond 255 outputs the codes are split over arrays of
                255 (made outside the timed region).

Both as the backend methods run them (work and output buffers allocated per call, the sizes read back between
the two calls).  Per variant: warm-up runs, then `runs` timed runs, each between device synchronisations; the
median and the spread (min .. max) in milliseconds.  Prints one JSON line per G and a markdown table.
usage: tools/bench_demux.py [nreads] [runs] [warmup]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from atropos_amd import _lib                           # noqa: E402
from atropos_amd.fastq import FastqBatch               # noqa: E402
from bench_fastq import device_fastq                   # noqa: E402

GROUPS = (2, 8, 96, 384)


def timed_runs(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    nreads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    be = _lib.get_backend()
    data, nbytes = device_fastq(nreads)
    batch, _ = FastqBatch.from_device(data, nbytes, True, be)
    n = len(batch)
    begin = torch.zeros((n,), dtype=torch.int32, device=data.device)
    end = batch.seq_lens.clone()
    gen = torch.Generator(device=data.device)
    gen.manual_seed(11)
    rows = []
    for G in GROUPS:
        group = torch.randint(0, G, (n,), device=data.device, generator=gen, dtype=torch.int32)
        dests = [torch.where(torch.div(group, 255, rounding_mode="floor") == k, group % 255,
                             torch.full_like(group, 255)).to(torch.uint8) for k in range((G + 254) // 255)]

        def grouped():
            return be.fastq_emit_grouped(batch.data, batch.records, begin, end, None, None, group, G)

        def loop():
            return [be.fastq_emit(batch.data, batch.records, begin, end, None, None, dests[g // 255], g % 255)
                    for g in range(G)]

        text, edges = grouped()                                 # the two agree before they are timed
        parts = loop()
        assert [int(p.numel()) for p in parts] == [edges[g + 1] - edges[g] for g in range(G)]
        for g in (0, G - 1):
            assert torch.equal(text[edges[g]:edges[g + 1]], parts[g])
        del parts, text
        a = timed_runs(grouped, runs, warmup)
        b = timed_runs(loop, runs, warmup)
        row = dict(groups=G, nreads=n, out_bytes=edges[-1], runs=runs,
                   grouped_ms=dict(median=statistics.median(a), min=min(a), max=max(a)),
                   loop_ms=dict(median=statistics.median(b), min=min(b), max=max(b)))
        print(json.dumps(row), flush=True)
        rows.append(row)
    print("| G | grouped: median (min .. max) ms | loop of G emits: median (min .. max) ms | loop / grouped |")
    print("|---|---|---|---|")
    for r in rows:
        a, b = r["grouped_ms"], r["loop_ms"]
        print("| %d | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.1f |" % (
            r["groups"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"], b["median"] / a["median"]))


if __name__ == "__main__":
    main()

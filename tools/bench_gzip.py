#!/usr/bin/env python3
"""The .gz output path on one MI355X:

  (a) kernel : HipBackend.gzip_blocks on a resident chunk of FASTQ text (tools/bench_fastq.py's generator over
               atropos_amd.synth reads), GB/s of plain text, with the compressed size
  (b) file   : TrimPipeline.trim_file of that text as a file into out.fastq.gz with device_gzip=True, the same run with
               device_gzip=False (one host thread of zlib at level 6), and the run into a plain file
  (c) sizes  : the device stream against zlib levels 1 and 6 over the same text (a sample of it for speed)

Per timed variant: warm-up runs, then `runs` runs; the median and the spread (min .. max).  One JSON line.
usage: tools/bench_gzip.py [nreads] [runs] [warmup] [host_reads]   (host_reads: reads of the device_gzip=False run)"""
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from atropos_amd import _lib                           # noqa: E402
from atropos_amd.trim import pipeline_from_args        # noqa: E402
from bench_fastq import device_fastq                   # noqa: E402

ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def main():
    nreads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    host_reads = int(sys.argv[4]) if len(sys.argv) > 4 else min(nreads, 200_000)
    be = _lib.get_backend()
    data, nbytes = device_fastq(nreads)
    text = data[:nbytes]
    # (a) the kernels alone
    ms = []
    for k in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, total = be.gzip_blocks(text)
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    kernel = dict(text_bytes=nbytes, compressed_bytes=total, ratio=nbytes / total, ms=spread(ms),
                  gb_per_s=nbytes / (statistics.median(ms) * 1e-3) / 1e9)
    # (c) sizes on a sample of whole blocks
    sample = bytes(text[:64 * 65280].cpu().numpy().tobytes())
    dev_sample = be.gzip_blocks(text[:len(sample)])[1]
    sizes = dict(sample_bytes=len(sample), device=dev_sample, zlib1=len(zlib.compress(sample, 1)),
                 zlib6=len(zlib.compress(sample, 6)))
    # (b) file to file
    host = bytes(text.cpu().numpy().tobytes())
    width = nbytes // nreads
    rates = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, small = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "in_small.fastq")
        with open(src, "wb") as fh:
            fh.write(host)
        with open(small, "wb") as fh:
            fh.write(host[:host_reads * width])
        for name, path_in, reads, path_out, flag, nrun in (("plain", src, nreads, "out.fastq", False, runs),
                                                           ("device_gzip", src, nreads, "out.fastq.gz", True, runs),
                                                           ("host_gzip", small, host_reads, "host.fastq.gz", False, max(1, min(runs, 3)))):
            secs = []
            for k in range((warmup if name != "host_gzip" else 0) + nrun):
                pipe = pipeline_from_args("-a %s -m 20" % ADAPTER)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.trim_file(path_in, os.path.join(tmp, path_out), device_gzip=flag)
                torch.cuda.synchronize()
                if name == "host_gzip" or k >= warmup:
                    secs.append(time.perf_counter() - t0)
            rates[name] = dict(reads=reads, seconds=spread(secs), mreads_per_s=reads / statistics.median(secs) / 1e6,
                               out_bytes=os.path.getsize(os.path.join(tmp, path_out)))
    print(json.dumps(dict(kernel=kernel, sizes=sizes, file_to_file=rates, runs=runs, warmup=warmup)), flush=True)


if __name__ == "__main__":
    main()

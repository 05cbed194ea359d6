#!/usr/bin/env python3
"""The .gz input path on one MI355X.  Two inputs hold the text of tools/bench_fastq.py's generator: the BGZF file that
``trim_file(..., device_gzip=True)`` writes (a pass-through pipeline), and an ordinary gzip file: ONE member written by
zlib at level 6, what a sequencer or an archive hands out.

  (a) kernel : HipBackend.gunzip_members on the resident BGZF file ("kernel"), and HipBackend.gunzip_stream -- the
               speculative inflater of device_gunzip="any" -- on the resident deflate data of the ordinary member
               ("stream_kernel", with its chunks / confirmed / redecoded counts), GB/s of plain text
  (b) file   : TrimPipeline.trim_file into a plain file from the BGZF file with device_gunzip=True, from the ordinary
               file with device_gunzip="any", the same two runs with device_gunzip=False (one host thread of zlib: the
               path before the flags, over fewer reads), and the run from the plain file (the ceiling).  The variants
               alternate, run after run.

Per timed variant: warm-up runs, then `runs` runs; the median and the spread (min .. max).  One JSON line.
usage: tools/bench_gunzip.py [nreads] [runs] [warmup] [host_reads]   (host_reads: reads of the device_gunzip=False run)"""
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


def scan_all(be, buf, n):
    member_at, text_at, at = [0], [0], 0
    while at < n:
        m_at, t_at, k, covered, ok = be.bgzf_scan(buf, at, n, 4096)
        assert ok and k, "the input is not BGZF throughout"
        member_at += [at + v for v in m_at[1:k + 1].tolist()]
        text_at += [text_at[-1] + v for v in t_at[1:k + 1].tolist()]
        at += covered
    return member_at, text_at


def main():
    nreads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    runs = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    host_reads = int(sys.argv[4]) if len(sys.argv) > 4 else min(nreads, 200_000)
    be = _lib.get_backend()
    data, nbytes = device_fastq(nreads)
    host = bytes(data[:nbytes].cpu().numpy().tobytes())
    width = nbytes // nreads
    with tempfile.TemporaryDirectory() as tmp:
        plain, small = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "small.fastq")
        with open(plain, "wb") as fh:
            fh.write(host)
        with open(small, "wb") as fh:
            fh.write(host[:host_reads * width])
        gz, small_gz = os.path.join(tmp, "in.fastq.gz"), os.path.join(tmp, "small.fastq.gz")
        for src, dst in ((plain, gz), (small, small_gz)):                  # (no adapter, no filter: the text as it is)
            pipeline_from_args("-m 1").trim_file(src, dst, device_gzip=True)
        # (a) the kernel alone, on the whole file resident
        raw = open(gz, "rb").read()
        n = len(raw)
        buf = torch.zeros(((n + 15) // 16 * 16,), dtype=torch.uint8)
        buf[:n] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        member_at, text_at = scan_all(be, buf, n)
        assert text_at[-1] == nbytes
        stream = buf.to(be.device)
        offsets = torch.tensor([member_at, text_at], dtype=torch.int64).to(be.device)
        text = be.empty((nbytes + 16,), torch.uint8)
        ms = []
        for k in range(warmup + runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status, bad = be.gunzip_members(stream, n, offsets[0], offsets[1], len(member_at) - 1, text, nbytes)
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        assert int(bad.item()) == 0 and bool((text[:nbytes] == data[:nbytes]).all()), "the inflated text is not the input"
        kernel = dict(text_bytes=nbytes, compressed_bytes=n, members=len(member_at) - 1, ms=spread(ms),
                      gb_per_s=nbytes / (statistics.median(ms) * 1e-3) / 1e9)
        # the ordinary gzip files: one zlib level 6 member each
        ordinary, small_ordinary = os.path.join(tmp, "ordinary.fastq.gz"), os.path.join(tmp, "small_ordinary.fastq.gz")
        for text_bytes, dst in ((host, ordinary), (host[:host_reads * width], small_ordinary)):
            co = zlib.compressobj(6, zlib.DEFLATED, 31)
            with open(dst, "wb") as fh:
                fh.write(co.compress(text_bytes) + co.flush())
        # (a) the stream entry point alone: the member's deflate data resident (behind the 10-byte header), one call
        raw = open(ordinary, "rb").read()
        n = len(raw) - 10 - 8
        assert n <= _lib.GUNZIP_STREAM_MAX and nbytes < (1 << 31) - 64, "fewer reads: one call takes a slab below 256 MiB"
        buf = torch.zeros(((n + 15) // 16 * 16 + 16,), dtype=torch.uint8)
        buf[:n] = torch.frombuffer(bytearray(raw[10:10 + n]), dtype=torch.uint8)
        stream = buf.to(be.device)
        window = be.empty((16,), torch.uint8)
        spacing = 131072                                   # (ChunkedFastqReader.STREAM_SPACING: what fastq._GzipStreamSource spaces its starts by)
        work = be.empty((be.gunzip_stream_workspace(n, spacing, nbytes + 64),), torch.uint8)
        text.zero_()
        ms = []
        for k in range(warmup + runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = be.gunzip_stream(stream, n, 0, window, 0, 0, text, nbytes + 16, spacing, work=work)
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        words = dict(zip(_lib.GUNZIP_STREAM_WORDS, res.cpu().tolist()))
        assert words["status"] == 0 and words["final_seen"] == 1 and words["text_len"] == nbytes and words["crc_out"] == zlib.crc32(host)
        assert bool((text[:nbytes] == data[:nbytes]).all()), "the inflated text is not the input"
        stream_kernel = dict(text_bytes=nbytes, compressed_bytes=n, spacing=spacing, chunks=words["chunks"], confirmed=words["confirmed"],
                             redecoded=words["redecoded"], ms=spread(ms), gb_per_s=nbytes / (statistics.median(ms) * 1e-3) / 1e9)
        del work
        # (b) file to file, the variants in turn
        variants = (("plain", plain, nreads, False), ("device_gunzip", gz, nreads, True), ("host_gunzip", small_gz, host_reads, False),
                    ("any_gunzip", ordinary, nreads, "any"), ("host_gunzip_ordinary", small_ordinary, host_reads, False))
        secs = {name: [] for name, _, _, _ in variants}
        for k in range(warmup + runs):
            for name, path_in, reads, flag in variants:
                pipe = pipeline_from_args("-a %s -m 20" % ADAPTER)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.trim_file(path_in, os.path.join(tmp, name + ".out"), device_gunzip=flag)
                torch.cuda.synchronize()
                if k >= warmup:
                    secs[name].append(time.perf_counter() - t0)
        outs = {name: open(os.path.join(tmp, name + ".out"), "rb").read() for name in ("plain", "device_gunzip", "any_gunzip")}
        assert outs["plain"] == outs["device_gunzip"], "device_gunzip changes the output"
        assert outs["plain"] == outs["any_gunzip"], "device_gunzip='any' changes the output"
        rates = {name: dict(reads=reads, seconds=spread(secs[name]), mreads_per_s=reads / statistics.median(secs[name]) / 1e6)
                 for name, _, reads, _ in variants}
    print(json.dumps(dict(kernel=kernel, stream_kernel=stream_kernel, file_to_file=rates, runs=runs, warmup=warmup)), flush=True)


if __name__ == "__main__":
    main()

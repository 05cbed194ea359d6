#!/usr/bin/env python3
"""Unaligned BAM input on one MI355X.  The reads (150 bp, names of 8 letters, an adapter in a third of them) are made
here, and so is their BAM file, with numpy, ``struct`` and ``zlib`` (BGZF members of 65 280 bytes at level 1).

  (a) kernels : on ONE resident chunk -- the whole file -- ``HipBackend.gunzip_members`` (compressed bytes -> BAM bytes),
                ``HipBackend.bam_walk`` (BAM bytes -> record table) and ``HipBackend.bam_to_fastq`` (records -> FASTQ text;
                both of its calls and the read-back of the text size between them), ms and GB/s of BAM bytes, for
                records without tags and with three tags; the repaired tiles of the walk
  (b) file    : ``TrimPipeline.trim_file`` into a plain file from the uBAM, from the same reads as BGZF ``.fastq.gz`` with
                ``device_gunzip=True`` and as plain ``.fastq``.  The variants alternate, run after run; the three
                outputs must be equal.

Per timed variant: warm-up runs, then `runs` runs; the median and the spread (min .. max).  One JSON line.
usage: tools/bench_bam.py [nreads] [runs] [warmup]"""
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atropos_amd import _lib                           # noqa: E402
from atropos_amd.trim import pipeline_from_args        # noqa: E402

ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
READ_LEN = 150
TAGS = b"RGZgrp1\0" + b"NMC\0" + b"ASC\x2a"            # "a few tags": 16 bytes


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def make_reads(n, seed=1):
    """(names uint8 [n, 8], bases uint8 [n, 150] of ACGT, qualities uint8 [n, 150] raw)."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, READ_LEN))]
    ad = np.frombuffer(ADAPTER.encode(), np.uint8)
    for at in (100, 120, 140):                             # an adapter at three offsets, each in a ninth of the reads
        rows = np.arange(at % 9, n, 9)
        take = min(len(ad), READ_LEN - at)
        bases[rows, at:at + take] = ad[:take]
    quals = rng.integers(2, 41, (n, READ_LEN), dtype=np.uint8)
    idx = np.arange(n)
    names = np.empty((n, 8), np.uint8)
    names[:, 0] = ord("r")
    for k in range(7):
        names[:, 7 - k] = 48 + (idx // 10 ** k) % 10
    return names, bases, quals


def fastq_text(names, bases, quals):
    n = len(names)
    rec = np.empty((n, 1 + 8 + 1 + READ_LEN + 3 + READ_LEN + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:9] = names
    rec[:, 9] = 10
    rec[:, 10:10 + READ_LEN] = bases
    rec[:, 10 + READ_LEN:13 + READ_LEN] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 13 + READ_LEN:13 + 2 * READ_LEN] = quals + 33
    rec[:, -1] = 10
    return rec.tobytes()


def bam_stream(names, bases, quals, tags=b""):
    """Header + records (one fixed length), not yet BGZF."""
    n = len(names)
    code = np.zeros(256, np.uint8)
    for k, c in enumerate(b"=ACMGRSVTWYHKDBN"):
        code[c] = k
    nib = code[bases]
    body = 32 + 9 + READ_LEN // 2 + READ_LEN + len(tags)
    rec = np.empty((n, 4 + body), np.uint8)
    fixed = struct.pack("<iiiBBHHHiiii", body, -1, -1, 9, 0, 4680, 0, 4, READ_LEN, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, np.uint8)
    rec[:, 36:44] = names
    rec[:, 44] = 0
    rec[:, 45:45 + READ_LEN // 2] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    rec[:, 45 + READ_LEN // 2:45 + READ_LEN // 2 + READ_LEN] = quals
    if tags:
        rec[:, -len(tags):] = np.frombuffer(tags, np.uint8)
    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0) + rec.tobytes()


def bgzf(payload):
    out = []
    for at in range(0, len(payload), 65280):
        data = payload[at:at + 65280]
        comp = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = comp.compress(data) + comp.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    out.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(out)


def scan_all(be, buf, n):
    member_at, text_at, at = [0], [0], 0
    while at < n:
        m_at, t_at, k, covered, ok = be.bgzf_scan(buf, at, n, 4096)
        assert ok and k, "the input is not BGZF throughout"
        member_at += [at + v for v in m_at[1:k + 1].tolist()]
        text_at += [text_at[-1] + v for v in t_at[1:k + 1].tolist()]
        at += covered
    return member_at, text_at


def timed(fn, runs, warmup):
    ms, last = [], None
    for k in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, last


def kernels(be, raw, stream_bytes, want_text, nreads, runs, warmup):
    n = len(raw)
    buf = torch.zeros(((n + 15) // 16 * 16,), dtype=torch.uint8)
    buf[:n] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    member_at, text_at = scan_all(be, buf, n)
    nbam = text_at[-1]
    assert nbam == stream_bytes
    comp = buf.to(be.device)
    offsets = torch.tensor([member_at, text_at], dtype=torch.int64).to(be.device)
    bam = be.empty(((nbam + 15) // 16 * 16 + 16,), torch.uint8)
    bam.zero_()
    ms_inflate, (status, bad) = timed(lambda: be.gunzip_members(comp, n, offsets[0], offsets[1], len(member_at) - 1, bam, nbam),
                                      runs, warmup)
    assert int(bad.item()) == 0
    entry, n_ref = be.bam_header(bytes(bam[:1 << 16].cpu().numpy().tobytes()))
    work = be.empty((be._host("atr_bam_walk_workspace", nbam, _lib.BAM_TILE),), torch.uint8)
    ms_walk, (starts, result) = timed(lambda: be.bam_walk(bam, nbam, entry, n_ref, True, work=work), runs, warmup)
    count, consumed, err, repaired = (int(v) for v in result.cpu().tolist())
    assert count == nreads and consumed == nbam and err == _lib.INT64_MAX
    ms_decode, (text, total, used, err, _) = timed(lambda: be.bam_to_fastq(bam, nbam, starts, count), runs, warmup)
    assert used == nreads and err == _lib.INT64_MAX
    assert bytes(text[:total].cpu().numpy().tobytes()) == want_text, "the decoded text is not the reads"

    def row(ms):
        return dict(ms=spread(ms), gb_per_s=nbam / (statistics.median(ms) * 1e-3) / 1e9)
    return dict(bam_bytes=nbam, compressed_bytes=n, members=len(member_at) - 1, records=count, tile_bytes=_lib.BAM_TILE,
                tiles=(nbam + _lib.BAM_TILE - 1) // _lib.BAM_TILE, repaired_tiles=repaired, gunzip_members=row(ms_inflate),
                bam_walk=row(ms_walk), bam_to_fastq=row(ms_decode),
                walk_plus_decode_over_inflate=(statistics.median(ms_walk) + statistics.median(ms_decode)) / statistics.median(ms_inflate))


def main():
    nreads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    runs = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    be = _lib.get_backend()
    names, bases, quals = make_reads(nreads)
    text = fastq_text(names, bases, quals)
    with tempfile.TemporaryDirectory() as tmp:
        result = {}
        paths = {}
        for label, tags in (("no_tags", b""), ("tags", TAGS)):
            stream = bam_stream(names, bases, quals, tags)
            raw = bgzf(stream)
            paths[label] = os.path.join(tmp, label + ".bam")
            with open(paths[label], "wb") as fh:
                fh.write(raw)
            result["kernels_" + label] = kernels(be, raw, len(stream), text, nreads, runs, warmup)
            del stream, raw
        plain, gz = os.path.join(tmp, "in.fastq"), os.path.join(tmp, "in.fastq.gz")
        with open(plain, "wb") as fh:
            fh.write(text)
        pipeline_from_args("-m 1").trim_file(plain, gz, device_gzip=True)       # (no adapter, no filter: the text as it is)
        variants = (("plain_fastq", plain, False), ("bgzf_fastq_device_gunzip", gz, True), ("ubam", paths["no_tags"], False),
                    ("ubam_tags", paths["tags"], False))
        secs = {name: [] for name, _, _ in variants}
        for k in range(warmup + runs):
            for name, path_in, flag in variants:
                pipe = pipeline_from_args("-a %s -m 20" % ADAPTER)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.trim_file(path_in, os.path.join(tmp, name + ".out"), device_gunzip=flag)
                torch.cuda.synchronize()
                if k >= warmup:
                    secs[name].append(time.perf_counter() - t0)
        outs = {name: open(os.path.join(tmp, name + ".out"), "rb").read() for name, _, _ in variants}
        assert all(o == outs["plain_fastq"] for o in outs.values()), "the input container changes the output"
        result["file_to_file"] = {name: dict(reads=nreads, seconds=spread(secs[name]),
                                             mreads_per_s=nreads / statistics.median(secs[name]) / 1e6) for name, _, _ in variants}
    result.update(reads=nreads, read_len=READ_LEN, runs=runs, warmup=warmup)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/reader_trace.json: the chunk trace of ``fastq.read_chunks`` -- per reader and chunk
``[nbytes, consumed, final]``, and the reader's ``inflate_path`` -- for the seeded inputs of
tests/_reader_trace_common.py (one per input road, at chunk sizes 3000 and 16384), on the CPU twins of the kernels.

The trace pins the chunk boundaries across a change of the reader's inside, so it is recorded with the code BEFORE that
change: check that commit out, run this, and commit the file with the change.  ``commit`` in the fixture is the hash of
the commit whose code wrote it (``--commit``, default: ``git rev-parse HEAD``); ``inputs`` are SHA-256 digests of the
input files, so that a zlib that deflates differently is told from a reader that cuts differently.  Every case is
recorded twice and the two must agree.

usage: python tests/golden/make_reader_trace_golden.py [--commit HASH] [--out FILE] [--hip]
(--hip: on the GPU instead of the twins, for a comparison by hand; the committed file is the twins')
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "reader_trace.json"))
    ap.add_argument("--hip", action="store_true")
    args = ap.parse_args()
    from tests import _reader_trace_common as T
    if args.hip:
        from atropos_amd import _lib
        _lib.set_backend(None)
        hip = _lib.get_backend()
        backends, only = (hip, hip), T.DEVICE_ROADS
    else:
        from tests import _bam_common as B
        from tests import _gunzip_stream_common as S
        backends, only = (S.StreamEmuBackend(), B.BamEmuBackend()), None
    with tempfile.TemporaryDirectory() as tmp:
        doc = T.record(tmp, backends, only)
        again = T.record(tmp, backends, only)
    assert doc == again, "the trace is not deterministic"
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    doc["commit"] = commit
    for name, by_size in sorted(doc["traces"].items()):
        print("%-20s %s" % (name, "  ".join("%s: %s" % (cb, "+".join("%d chunks (%s)" % (len(r["chunks"]), r["inflate_path"])
                                                                     for r in readers)) for cb, readers in sorted(by_size.items()))))
    with open(args.out, "w") as fh:
        json.dump(doc, fh, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes, commit", commit)


if __name__ == "__main__":
    main()

"""Shared by tests/test_reader_trace.py and tests/golden/make_reader_trace_golden.py: the chunk trace of
``fastq.read_chunks`` -- per reader and chunk ``(nbytes, consumed, final)``, and the reader's ``inflate_path`` -- over
small seeded inputs, one per input road of ``fastq.ChunkedFastqReader``.  The chunk boundaries decide part-file contents
and the bytes of device-gzip output, so they are pinned against a recording (tests/golden/reader_trace.json)."""
import hashlib
import os

from tests import _bam_common as B
from tests import _gunzip_common as U
from tests import _gunzip_stream_common as S
from tests import _gzip_common as G

CHUNK_SIZES = (3000, 1 << 14)
DEVICE_ROADS = ("bgzf", "ordinary_any", "bgzf_then_ordinary", "ubam_single", "ubam_paired", "lockstep_any")


def _mates():
    """Two files whose records differ in size: mate 2 has 100 bases (``_gunzip_common.check_trim_files``)."""
    r1 = G.fastq_input(nrec=300, seed=5)
    lines = G.fastq_input(nrec=300, seed=6).split(b"\n")
    for r in range(300):
        lines[4 * r + 1] = lines[4 * r + 1][:100]
        lines[4 * r + 3] = lines[4 * r + 3][:100]
    return r1, b"\n".join(lines)


def _members_taken(sizes, budget):
    """How many of the members ahead (``sizes``: their bytes of text) a BGZF slab takes: while their text fits, one at least."""
    k = len(sizes)
    while k > 1 and sum(sizes[:k]) > budget:
        k -= 1
    return k


def _member_size(n, eof, first):
    """The text of ``n`` bytes in BGZF members of how many bytes each (``first`` or a little more; ``eof``: the empty
    end marker follows).  A BGZF slab is cut on the read-ahead thread, by a budget of the chunk size less the carry
    that thread last saw, and which carry that is depends on how far ahead the thread is: with members of a few
    hundred bytes the trace differs from run to run (so it did with the reader the fixture was recorded with).  So the
    size is one at which the carry cannot decide: wherever a slab starts, it takes the same members at a carry of 0 and
    at one of 399 bytes -- more than a record, or a pair, of these inputs has."""
    for size in range(first, first + 500, 10):
        sizes = [size] * (n // size) + [n % size] * bool(n % size) + [0] * bool(eof)
        if all(_members_taken(sizes[s:], c - 399) == _members_taken(sizes[s:], c) for c in CHUNK_SIZES for s in range(len(sizes))):
            return size
    raise AssertionError("no member size for %d bytes" % n)


def _bam(stream):
    size = _member_size(len(stream), True, 1300)
    return B.bgzf(stream, list(range(size, len(stream), size)))


def make_cases(tmp):
    """{name: (paths, keyword arguments of ``read_chunks``, needs the BAM backend)}; the files are written under ``tmp``."""
    from atropos_amd.shard import fastq_shard_ranges
    tmp = str(tmp)
    text = G.fastq_input(nrec=300)
    assert text.endswith(b"\n")
    half = len(text) // 2
    r1, r2 = _mates()
    pairs = B.pair_fastq(n=150)
    single = B.fastq_to_bam(text)
    paired = B.fastq_to_bam(pairs, paired=True, swap=(3, 17, 39))
    files = {
        "no_newline.fastq": text[:-1],
        "whole.fastq": text,
        "host.fastq.gz": S.gz_member(text),
        "bgzf.fastq.gz": U.bgzf_bytes(text, size=_member_size(len(text), True, 3000)),
        "ordinary.fastq.gz": S.gz_member(text[:half], flags=8, mem=1) + S.gz_member(text[half:], level=1),   # (mem=1: small blocks)
        "bgzf_then_ordinary.fastq.gz": U.bgzf_bytes(text[:half], size=_member_size(half, False, 3000), eof=False) + S.gz_member(text[half:]),
        "single.bam": _bam(single),
        "paired.bam": _bam(paired),
        "r1.fastq": r1, "r2.fastq": r2,
        "r1.fastq.gz": S.gz_member(r1, mem=1), "r2.fastq.gz": S.gz_member(r2, level=9, mem=2),
    }
    for name, data in files.items():
        with open(os.path.join(tmp, name), "wb") as fh:
            fh.write(data)
    at = lambda *names: [os.path.join(tmp, n) for n in names]
    ranges = fastq_shard_ranges(at("whole.fastq")[0], 3)
    cases = {
        "plain_no_newline": (at("no_newline.fastq"), {}, False),
        "plain_byte_range": (at("whole.fastq"), dict(byte_ranges=[ranges[1]]), False),
        "host_gz": (at("host.fastq.gz"), dict(device_gunzip=False), False),
        "bgzf": (at("bgzf.fastq.gz"), dict(device_gunzip=True), False),
        "ordinary_any": (at("ordinary.fastq.gz"), dict(device_gunzip="any"), False),
        "bgzf_then_ordinary": (at("bgzf_then_ordinary.fastq.gz"), dict(device_gunzip="any"), False),
        "ubam_single": (at("single.bam"), {}, True),
        "ubam_paired": (at("paired.bam"), dict(interleaved=True), True),
        "lockstep_plain": (at("r1.fastq", "r2.fastq"), {}, False),
        "lockstep_any": (at("r1.fastq.gz", "r2.fastq.gz"), dict(device_gunzip="any"), False),
    }
    digest = {n: hashlib.sha256(d).hexdigest() for n, d in sorted(files.items())}
    return cases, digest


def trace(paths, chunk_bytes, backend, **how):
    """[{"inflate_path": ..., "chunks": [[nbytes, consumed, final], ...]} per path] of one ``read_chunks`` run."""
    from atropos_amd import fastq
    made = []
    real = fastq.ChunkedFastqReader

    class Traced(real):
        def __init__(self, *a, **k):
            real.__init__(self, *a, **k)
            self.chunks = []
            made.append(self)

        def advance(self, consumed=None):
            self.chunks.append([int(self.nbytes), int(self.consumed if consumed is None else consumed), bool(self.final)])
            return real.advance(self, consumed)

    fastq.ChunkedFastqReader = Traced
    try:
        for _ in fastq.read_chunks(paths, chunk_bytes, backend, **how):
            pass
    finally:
        fastq.ChunkedFastqReader = real
    return [dict(inflate_path=r.inflate_path, chunks=r.chunks) for r in made]


def record(tmp, backends, only=None):
    """{"inputs": digests, "traces": {case: {chunk size: trace}}}; ``backends``: (for text, for BAM)."""
    from atropos_amd import _lib
    cases, digest = make_cases(tmp)
    out = {}
    for name, (paths, how, bam) in sorted(cases.items()):
        if only is not None and name not in only:
            continue
        be = backends[1] if bam else backends[0]
        prev = _lib.set_backend(be, _test_double=True)
        try:
            out[name] = {str(cb): trace(paths, cb, be, **how) for cb in CHUNK_SIZES}
        finally:
            _lib.set_backend(prev, _test_double=True)
    return dict(inputs=digest, traces=out)

"""Shared by test_gunzip_stream_host.py (the CPU twin, tests/emu/emu_gunzip_stream.cpp) and test_gpu_gunzip_stream.py
(the kernels of atropos_amd/csrc/gunzip_stream_kernels.hip): the speculative inflater of ordinary deflate streams
(``gunzip_stream``) at the C ABI, and ``device_gunzip="any"`` of the reader and the file drivers.

The oracle for text is ``zlib.decompressobj(-15)``; block boundaries come from the block walker of
tests/_gunzip_common.py (``walk``), which reads the bits itself.  Nothing here includes or calls the inflater under test
except through a backend.  Also builds and loads the twin library and defines the backend that serves it."""
import ctypes as C
import functools
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import torch

from atropos_amd import _lib
from tests import _fasta_common as F
from tests import _gunzip_common as U
from tests import _gzip_common as G
from tests.emu import backend as emu

ENTRY_POINTS = ("atr_gunzip_stream_workspace", "atr_gunzip_stream")
FILL = 0xa5
NEED_INPUT, NEED_ROOM = 101, 102
_twin = []


# ---------------------------------------------------------------------------------------------- the twin
def _deps():
    cpp = os.path.join(emu._HERE, "emu_gunzip_stream.cpp")
    return cpp, [cpp, os.path.join(emu._HERE, "emu_abi.hpp"), os.path.join(emu._ROOT, "include", "atropos_hip.h")] + [
        os.path.join(emu._CSRC, f) for f in ("inflate_stream_core.hpp", "inflate_core.hpp", "deflate_core.hpp")]


def build_twin():
    """tests/emu/libemu_gunzip_stream.so from emu_gunzip_stream.cpp and the product's per-wave code."""
    so = os.path.join(emu._HERE, "libemu_gunzip_stream.so")
    cpp, deps = _deps()
    if emu.stale(so, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU"] + emu._INC + [cpp, "-o", so])
    return so


def build_fuzz():
    """The stand-alone sanitized program (its own ``main``): address and undefined-behaviour sanitizers over the twin."""
    main = os.path.join(emu._HERE, "gunzip_stream_fuzz_main.cpp")
    prog = os.path.join(emu._HERE, "gunzip_stream_fuzz")
    cpp, deps = _deps()
    if emu.stale(prog, deps + [main]):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-DATR_HOST_EMU"] + emu._INC + [main, cpp, "-o", prog])
    return prog


def load_twin():
    if not _twin:
        _twin.append(_lib.attach_prototypes(C.CDLL(build_twin()), "emu_", ENTRY_POINTS))
    return _twin[0]


class StreamEmuBackend(F.FastaEmuBackend, _lib.GunzipStreamCalls):
    """The CPU stand-in with the stream entry points, which go to a twin library of their own (emu_gunzip_stream.cpp);
    above the one with the FASTA entry points, for the drivers' ``.fasta.gz`` case."""

    def __init__(self):
        F.FastaEmuBackend.__init__(self)
        self.stream_calls = 0

    def _call(self, name, *args):
        if name not in ENTRY_POINTS:
            return super()._call(name, *args)
        fn, at = load_twin()[name]
        return _lib._check(None, fn(*args) if at is None else fn(*args[:at], None, *args[at:]), name)

    _host = _call

    def _symbol(self, name):
        return load_twin()[name][0] if name in ENTRY_POINTS else super()._symbol(name)

    def gunzip_stream(self, *args, **how):
        self.stream_calls += 1
        return super().gunzip_stream(*args, **how)


# ---------------------------------------------------------------------------------------------- streams
def deflate_of(member):
    """The deflate data of a gzip member written by tests/_gunzip_common.py or the project's compressor."""
    return member[U.data_start(member):-8]


def framed(deflate, text):
    """``deflate`` in a gzip member that ``walk`` reads (an empty extra field), of any size."""
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\0\0" + deflate + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


@functools.lru_cache(maxsize=None)
def blocks_of(deflate):
    """``walk`` over a whole deflate stream, bit positions counted from the stream's first bit."""
    text = zlib.decompressobj(-15).decompress(deflate)
    blocks = U.walk(framed(deflate, text))
    for b in blocks:
        b["start"] -= 96
        b["end"] -= 96
    return blocks


def oracle(deflate, n_stream=None):
    """What zlib makes of ``deflate[:n_stream]`` -> (text, eof) or None for an error."""
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(deflate if n_stream is None else deflate[:n_stream]), d.eof
    except zlib.error:
        return None


def fastq_text(n):
    return G.ratio_fixture("uniform")[:n]


def mutated_period(period=20000, copies=5, seed=7):
    """Text over 64 letters of period ``period`` whose every copy renews 20 bytes in 60: matches of 40 at the distance
    of a period between literals, so that every stretch of it is worth a dynamic block."""
    rng = np.random.default_rng(seed)
    letters = np.arange(48, 112, dtype=np.uint8)
    base = rng.choice(letters, size=period)
    out = [base]
    for _ in range(copies - 1):
        nxt = out[-1].copy()
        for lo in range(40, period, 60):
            nxt[lo:lo + 20] = rng.choice(letters, size=len(nxt[lo:lo + 20]))
        out.append(nxt)
    return np.concatenate(out).tobytes()


TEXTS = {"fastq": lambda: fastq_text(150000)}
TEXTS.update({"period_%03d" % p: (lambda p=p: U.CONTENTS["period_%03d" % p](40000)) for p in (1, 3, 63, 64, 65, 258, 259)})
CHUNKS = (256, 1024, 4096, 1 << 20)
WRITERS = {k: v for k, v in U.WRITERS.items() if v is not None}


# ---------------------------------------------------------------------------------------------- one call
def run(backend, deflate, n_stream=None, start_bit=0, window=b"", crc_in=0, capacity=None, chunk_bytes=1024, want_text=None):
    """One ``gunzip_stream`` call over ``deflate[:n_stream]`` with the stream, the window, the text and the workspace
    inside buffers filled with FILL.  -> dict of the result words and ``text``; asserts that nothing outside
    text[0 .. capacity) and the workspace was stored to."""
    n = len(deflate) if n_stream is None else n_stream
    if capacity is None:
        capacity = (len(want_text) if want_text is not None else 4 * n) + 300
    dev = backend.device
    pad = 64
    host = np.full((pad + (n + 15) // 16 * 16 + 16,), 0, dtype=np.uint8)
    host[:pad] = FILL
    host[pad:pad + n] = np.frombuffer(deflate[:n], dtype=np.uint8)
    stream = torch.from_numpy(host).to(dev)
    win = torch.from_numpy(np.frombuffer(bytes(window) + b"\0", dtype=np.uint8).copy()).to(dev)
    text = torch.full((pad + capacity + pad,), FILL, dtype=torch.uint8).to(dev)
    need = backend.gunzip_stream_workspace(n, chunk_bytes, capacity)
    work = torch.full((pad + need + pad,), FILL, dtype=torch.uint8).to(dev)
    res = backend.gunzip_stream(stream[pad:], n, start_bit, win, len(window), crc_in, text[pad:], capacity, chunk_bytes,
                                work=work[pad:pad + need])
    out = dict(zip(_lib.GUNZIP_STREAM_WORDS, res.cpu().tolist()))
    raw, w, s = text.cpu().numpy(), work.cpu().numpy(), stream.cpu().numpy()
    assert (raw[:pad] == FILL).all() and (raw[pad + capacity:] == FILL).all(), "a store outside the text's capacity"
    assert (w[:pad] == FILL).all() and (w[pad + need:] == FILL).all(), "a store outside the workspace"
    assert (s == host).all(), "a store into the stream"
    assert 0 <= out["text_len"] <= capacity
    out["text"] = raw[pad:pad + out["text_len"]].tobytes()
    return out


def check_whole(backend, deflate, text, chunk_bytes, what=""):
    """A whole stream in one call: the text, the bit behind the final block, the CRC."""
    r = run(backend, deflate, chunk_bytes=chunk_bytes, want_text=text)
    assert r["status"] == 0, (what, chunk_bytes, r["status"])
    assert r["text"] == text, (what, chunk_bytes)
    assert r["final_seen"] == 1 and (r["end_bit"] + 7) // 8 == len(deflate) and r["end_bit"] == blocks_of(deflate)[-1]["end"], (what, chunk_bytes)
    assert r["crc_out"] == zlib.crc32(text), (what, chunk_bytes)
    assert r["chunks"] == max(1, -(-len(deflate) // chunk_bytes)) and 1 <= r["confirmed"] <= r["chunks"], (what, chunk_bytes, r["chunks"], r["confirmed"])
    return r


def check_writer(backend, writer):
    for name in sorted(TEXTS):
        text = TEXTS[name]()
        deflate = U.raw_deflate(text, **WRITERS[writer])
        for cb in CHUNKS:
            check_whole(backend, deflate, text, cb, "%s/%s" % (writer, name))


# ---------------------------------------------------------------------------------------------- the window
def check_window_edge(backend):
    """A match at distance exactly 32 768, from the project's own compressor (zlib stops at 32 506)."""
    text = U.CONTENTS["window_edge"](U.FULL)
    deflate = deflate_of(U.written("own", text, backend))
    assert any(d == 32768 for b in blocks_of(deflate) for _, _, d in b["matches"])
    for cb in CHUNKS:
        check_whole(backend, deflate, text, cb, "window_edge")


def _stored(data, final=False):
    return bytes([1 if final else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data


def _fixed_matches(matches, final=True):
    """A fixed block of length-258 matches at ``matches`` distances (24 577 .. 32 768), from a byte boundary."""
    w = U._BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    for d in matches:
        U._fixed_code(w, 285)
        w.code(29, 5)
        w.put(d - 24577, 13)
    U._fixed_code(w, 256)
    return w.bytes()


def check_ring(backend):
    """Length 258 at distances up to 32 768 behind 32 768 bytes of text: a ring of exactly 32 768 slots would read what
    the same match writes.  With one chunk the speculative decode takes it, with small chunks the decode from known state."""
    rng = np.random.default_rng(11)
    head = rng.integers(0, 256, 33000, dtype=np.uint8).tobytes()
    dists = (32768, 32767, 32700, 32511, 32768 - 257, 32768 - 258, 32768 - 64, 32768)
    deflate = _stored(head) + _fixed_matches(dists)
    text = zlib.decompressobj(-15).decompress(deflate)
    assert len(text) == 33000 + 258 * len(dists)
    for cb in CHUNKS:
        r = check_whole(backend, deflate, text, cb, "ring")
        assert r["confirmed"] == 1
    # the same behind an unknown window: the call starts at the fixed block, the head is the window
    bit = 8 * len(_stored(head))
    r = run(backend, deflate, start_bit=bit, window=head[-32768:], crc_in=zlib.crc32(head), want_text=text)
    assert r["status"] == 0 and r["text"] == text[33000:] and r["crc_out"] == zlib.crc32(text) and r["final_seen"] == 1


def candidate_blocks(deflate, chunk_bytes):
    """The blocks the finder can name: per chunk (not chunk 0) the first non-final dynamic block that starts in it."""
    first = {}
    for b in blocks_of(deflate):
        i = b["start"] // (8 * chunk_bytes)
        if i and b["btype"] == 2 and not b["bfinal"] and i not in first:
            first[i] = b
    return first


def check_straddle(backend):
    """Matches whose source straddles a chunk's start (part marker, part own text), and overlapping ones (distance below
    length) whose source lies before it: read from the walked stream, then the text compared."""
    # FASTQ text, then a periodic run in whose middle a block ends (Z_BLOCK): the next block opens with a copy of the run
    text, flushes = b"", []
    for i, p in enumerate((3, 63, 65, 127, 7, 31, 255, 1)):
        text += fastq_text(60000)[i * 4000:(i + 1) * 4000] + U.CONTENTS["period_%03d" % p](900)
        flushes.append((len(text) - 500, zlib.Z_BLOCK))
    text += fastq_text(4000)
    deflate = U.raw_deflate(text, level=6, flushes=tuple(flushes))
    cb = 256
    straddle = overlap = 0
    for b in candidate_blocks(deflate, cb).values():
        for pos, n, d in b["matches"]:
            straddle += pos - d < b["text_at"] < pos - d + n
            overlap += d < n and pos - d < b["text_at"]
    assert straddle >= 3 and overlap >= 1, (straddle, overlap)
    r = check_whole(backend, deflate, text, cb, "straddle")
    assert r["confirmed"] >= 8


def check_period_chain(backend):
    """Text of period 20 000 in blocks of 10 000 bytes: every chunk refers into its predecessors, and a chunk shorter
    than the window hands on part of the older window."""
    text = mutated_period()
    deflate = U.raw_deflate(text, level=6, flushes=tuple((lo, zlib.Z_SYNC_FLUSH) for lo in range(10000, len(text), 10000)))
    blocks = [b for b in blocks_of(deflate) if b["size"]]
    assert len(blocks) >= 9 and all(b["btype"] == 2 for b in blocks)
    assert all(any(d > pos - b["text_at"] + 10000 for pos, _, d in b["matches"]) for b in blocks[3:])
    sizes = [(b["end"] - b["start"]) // 8 for b in blocks[2:]]
    cb = min(sizes) - 16                                                     # (every block from the third on opens a chunk)
    assert cb >= 256
    r = check_whole(backend, deflate, text, cb, "period chain")
    assert r["confirmed"] >= 4, r
    for other in (256, 1024):
        check_whole(backend, deflate, text, other, "period chain")


# ---------------------------------------------------------------------------------------------- chunks
def check_aligned_block(backend):
    """A call that begins at a block inside the stream (a bit that is no byte's first) with chunk_bytes such that a later
    block starts exactly on a chunk's first bit -- and the block before it ends on a chunk's last bit."""
    text = fastq_text(150000)
    deflate = U.raw_deflate(text, level=6, mem=1)
    blocks = [b for b in blocks_of(deflate) if b["btype"] == 2 and not b["bfinal"]]
    pair = next((a, b) for i, a in enumerate(blocks) for b in blocks[i + 1:i + 40]
                if a["start"] % 8 and (b["start"] - a["start"]) % 8 == 0 and b["start"] - a["start"] >= 8 * 256)
    a, b = pair
    cb = (b["start"] - a["start"]) // 8
    before = text[:a["text_at"]]
    r = run(backend, deflate, start_bit=a["start"], window=before[-32768:], crc_in=zlib.crc32(before), chunk_bytes=cb, want_text=text)
    assert r["status"] == 0 and r["text"] == text[a["text_at"]:] and r["crc_out"] == zlib.crc32(text) and r["final_seen"] == 1
    assert r["confirmed"] >= 2
    # a window shorter than the text before it: a match that reaches beyond it is zlib's "invalid distance too far back"
    far = min(pos - d for blk in blocks_of(deflate) if blk["start"] >= a["start"] for pos, _, d in blk["matches"])
    assert far < a["text_at"]
    short = a["text_at"] - far - 1
    r = run(backend, deflate, start_bit=a["start"], window=before[len(before) - short:], crc_in=zlib.crc32(before), chunk_bytes=cb, want_text=text)
    assert r["status"] == 11, r["status"]


def check_double(backend):
    """Stored blocks whose bytes are a real deflate stream: every candidate inside is false."""
    text = fastq_text(600000)
    inner = U.raw_deflate(text, level=6)
    outer = U.raw_deflate(inner, level=0)
    assert len(candidate_blocks(inner, 1024)) >= 8 and all(b["btype"] == 0 for b in blocks_of(outer))
    for cb in (256, 1024, 4096):
        r = check_whole(backend, outer, inner, cb, "double")
        assert r["confirmed"] == 1, r


# ---------------------------------------------------------------------------------------------- resuming
def boundaries(deflate):
    """{bit behind a block: bytes of text before it}."""
    return {b["end"]: b["text_at"] + b["size"] for b in blocks_of(deflate)}


def inflate_in_calls(backend, deflate, slab, capacity, chunk_bytes, grow=True):
    """The whole stream as a reader takes it: slabs of ``slab`` bytes from the byte of the last boundary, ``capacity``
    bytes of text a call; a slab or a room in which no block ends is doubled.  -> (text, calls, the statuses seen)."""
    ends = boundaries(deflate)
    text, bit, crc, calls, seen = b"", 0, 0, 0, set()
    while True:
        at = bit // 8
        piece = deflate[at:at + slab]
        r = run(backend, piece, start_bit=bit - 8 * at, window=text[-32768:], crc_in=crc, capacity=capacity, chunk_bytes=chunk_bytes)
        calls += 1
        seen.add(r["status"])
        assert calls < 5000
        if r["status"] == NEED_INPUT:
            assert at + slab < len(deflate), "more input asked for at the stream's end"
            assert r["end_bit"] == bit - 8 * at and r["text_len"] == 0
            slab *= 2
            continue
        if r["status"] == NEED_ROOM:
            assert r["end_bit"] == bit - 8 * at and r["text_len"] == 0
            capacity *= 2
            continue
        assert r["status"] == 0, r["status"]
        bit = 8 * at + r["end_bit"]
        text += r["text"]
        crc = r["crc_out"]
        assert ends.get(bit) == len(text), "end_bit is no block boundary, or the text is not the text before it"
        assert crc == zlib.crc32(text)
        if r["final_seen"]:
            return text, calls, seen


def check_resume(backend):
    text = fastq_text(120000)
    for how in (dict(level=6), dict(level=1, mem=1), dict(level=0), dict(strategy=zlib.Z_FIXED, flushes=((40000, zlib.Z_SYNC_FLUSH), (90000, zlib.Z_FULL_FLUSH)))):
        deflate = U.raw_deflate(text, **how)
        # small room: more calls than one
        got, calls, seen = inflate_in_calls(backend, deflate, len(deflate), 70000, 1024)
        assert got == text and calls >= 2, (how, calls)
        # small slabs and small room
        got, calls, seen = inflate_in_calls(backend, deflate, 9000, 50000, 512)
        assert got == text and calls >= 3, (how, calls)
    # the statuses of no progress
    deflate = U.raw_deflate(text, level=6)
    first = blocks_of(deflate)[0]
    r = run(backend, deflate, n_stream=first["end"] // 8 - 1, capacity=first["size"] + 100)
    assert r["status"] == NEED_INPUT and r["end_bit"] == 0 and r["text_len"] == 0
    r = run(backend, deflate, capacity=first["size"] - 1)
    assert r["status"] == NEED_ROOM and r["end_bit"] == 0 and r["text_len"] == 0
    r = run(backend, deflate, capacity=first["size"])
    assert r["status"] == 0 and r["end_bit"] == first["end"] and r["text"] == text[:first["size"]]
    r = run(backend, deflate, n_stream=0, capacity=10)
    assert r["status"] == NEED_INPUT


def check_slab_cuts(backend):
    """Slabs cut at every byte offset of a short stretch: inside a block header, a code, a stored length."""
    text = fastq_text(20000)
    deflate = U.raw_deflate(text, level=6, flushes=((3000, zlib.Z_SYNC_FLUSH), (3100, zlib.Z_FULL_FLUSH), (9000, zlib.Z_SYNC_FLUSH)))
    ends = boundaries(deflate)
    blocks = blocks_of(deflate)
    assert {b["btype"] for b in blocks} >= {0, 2}
    cuts = set()
    for b in blocks[:6]:
        cuts |= set(range(max(0, b["start"] // 8 - 3), min(len(deflate), b["start"] // 8 + 12)))
    cuts |= set(range(0, 80)) | set(range(len(deflate) - 12, len(deflate) + 1))
    for cut in sorted(cuts):
        r = run(backend, deflate, n_stream=cut, chunk_bytes=256, want_text=text)
        done = [e for e in ends if (e + 7) // 8 <= cut]
        if not done:
            assert r["status"] == NEED_INPUT, cut
            continue
        assert r["status"] == 0 and r["end_bit"] == max(done), (cut, r["end_bit"], max(done))
        assert r["text"] == text[:ends[max(done)]] and r["final_seen"] == (max(done) == blocks[-1]["end"]), cut


# ---------------------------------------------------------------------------------------------- launch
def check_launch(backend, count):
    text = fastq_text(600000)
    deflate = U.raw_deflate(text, level=6)
    if count == 1:
        n, cb = len(deflate), len(deflate) + 5
    else:
        cb = max(64, len(deflate) // count)
        n = cb * count - cb // 2
    assert n <= len(deflate)
    r = run(backend, deflate, n_stream=n, chunk_bytes=cb, want_text=text)
    ends = boundaries(deflate)
    last = max(e for e in ends if (e + 7) // 8 <= n)
    assert r["status"] == 0 and r["chunks"] == count and r["end_bit"] == last and r["text"] == text[:ends[last]], (count, r["chunks"])
    return r


def check_empty(backend):
    for cb in (64, 256):
        r = run(backend, b"\x01\x00\x00\xff\xff", chunk_bytes=cb, capacity=0)
        assert (r["status"], r["end_bit"], r["text_len"], r["final_seen"], r["crc_out"], r["chunks"]) == (0, 40, 0, 1, 0, 1)
    r = run(backend, b"\x03\x00", chunk_bytes=64, capacity=16)                # an empty fixed block
    assert (r["status"], r["end_bit"], r["text_len"], r["final_seen"]) == (0, 10, 0, 1)


# ---------------------------------------------------------------------------------------------- corrupt streams
def corrupt_streams():
    """[(name, stream)]: the deflate data of every member of ``corrupt_corpus`` behind valid blocks that end on a byte
    (a sync flush), so that it lies in the first, a middle and the last chunk of 1 024 bytes -- in the middle with more
    valid-looking data behind it."""
    text = fastq_text(40000)
    out = []
    for name, m in sorted(U.corrupt_corpus().items()):
        bad = deflate_of(m)
        for where, n in (("first", 0), ("middle", 9000), ("last", 30000)):
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            pre = (co.compress(text[:n]) + co.flush(zlib.Z_SYNC_FLUSH)) if n else b""
            tail = U.raw_deflate(text[:9000]) if where == "middle" else b""
            out.append(("%s/%s" % (name, where), pre + bad + tail))
    return out


def check_corrupt(backend):
    """Every one terminates, reports an error exactly when zlib does (and zlib's text and end where it does not), and
    stores nowhere else (``run``)."""
    errors = 0
    for name, stream in corrupt_streams():
        want = oracle(stream)
        for cb in (1024, 1 << 20):
            r = run(backend, stream, chunk_bytes=cb, capacity=120000)
            if want is None:
                assert r["status"] not in (0, NEED_INPUT, NEED_ROOM), (name, cb, r["status"])
                errors += 1
            else:
                assert r["status"] == 0 and r["final_seen"] == int(want[1]), (name, cb, r["status"])
                if want[1]:
                    assert r["text"] == want[0], (name, cb)
                else:
                    assert want[0].startswith(r["text"]), (name, cb)
    assert errors >= 60
    # the rule a member breaks is the status, as for a BGZF member (the rules of the trailer are the reader's)
    for name, code in sorted(U.CORPUS_STATUS.items()):
        if code in (4, 12, 13, 14):
            continue
        r = run(backend, deflate_of(U.corrupt_corpus()[name]), chunk_bytes=1024, capacity=10000)
        assert r["status"] == code, (name, r["status"], code)


# ---------------------------------------------------------------------------------------------- the cap
def cap_counts(backend, level):
    """(W, confirmed, redecoded) of FASTQ text written by zlib at ``level``, 4 096-byte chunks: W = chunks (not chunk 0)
    in whose bit range a dynamic block starts."""
    text = G.ratio_fixture("uniform")
    deflate = U.raw_deflate(text, level=level)
    w = len({b["start"] // (8 * 4096) for b in blocks_of(deflate) if b["btype"] == 2} - {0})
    r = check_whole(backend, deflate, text, 4096, "cap level %d" % level)
    return w, r["confirmed"], r["redecoded"]


def check_cap(backend, level):
    w, confirmed, redecoded = cap_counts(backend, level)
    print("level %d: W %d confirmed %d redecoded %d" % (level, w, confirmed, redecoded))
    assert w >= 8, "lengthen the text"
    assert 8 * (confirmed - 1) >= 7 * w, (w, confirmed, redecoded)


def agreement_streams():
    text = fastq_text(150000)
    return [(U.raw_deflate(text, level=6), 1024), (U.raw_deflate(text, level=1, mem=1), 256), (U.raw_deflate(text, level=0), 4096),
            (U.raw_deflate(U.raw_deflate(text, level=6), level=0), 1024), (U.raw_deflate(mutated_period(), level=9), 512)]


def check_abi_errors(call, workspace):
    """The refusals come before any pointer is looked at."""
    ok = (None, 100, 0, None, 0, 0, None, 0, 256, None, 0, None)
    def with_(**k):
        names = ("s", "n", "bit", "w", "wl", "crc", "t", "cap", "cb", "work", "wb", "res")
        return tuple(k.get(a, v) for a, v in zip(names, ok)) + (None,)
    assert call(*with_(n=-1)) == -1 and call(*with_(bit=-1)) == -1 and call(*with_(bit=801)) == -1
    assert call(*with_(wl=-1)) == -1 and call(*with_(wl=32769)) == -1 and call(*with_(cap=-1)) == -1 and call(*with_(cb=63)) == -1
    assert call(*with_(n=1 << 28)) == -2 and call(*with_(cap=1 << 31)) == -2 and call(*with_(cb=(1 << 24) + 1)) == -2
    assert call(*with_()) == -1                                               # (no pointers)
    assert workspace(-1, 256, 10) == -1 and workspace(10, 0, 10) == -1 and workspace(100, 256, 1000) > 0


# ---------------------------------------------------------------------------------------------- reader and drivers
def gz_member(text, level=6, flags=0, mtime=0, mem=8):
    """An ordinary gzip member; ``flags``: FTEXT 1, FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16."""
    head = b"\x1f\x8b\x08" + bytes([flags]) + struct.pack("<I", mtime) + b"\x00\x03"
    if flags & 4:
        head += struct.pack("<H", 7) + b"XY\x03\x00abc"
    if flags & 8:
        head += b"reads.fastq\0"
    if flags & 16:
        head += b"a comment\0"
    if flags & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + U.raw_deflate(text, level=level, mem=mem) + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def host_verdict(path, backend, chunk_bytes):
    try:
        return U.read_all(path, backend, chunk_bytes, device_gunzip=False)[0]
    except Exception as e:                                                     # noqa: BLE001
        return type(e)


def check_reader(backend, tmp_path, chunk_bytes=1 << 14):
    """Path selection and the files a user has: the same text, or the same exception type, as ``device_gunzip=False``."""
    text = G.fastq_input(nrec=500)
    half = len(text) // 2
    plain = gz_member(text)
    files = {
        "ordinary": (plain, "stream"),
        "python": (gzip.compress(text), "stream"),
        "all_fields": (gz_member(text, flags=31, mtime=12345), "stream"),
        "cat": (gz_member(text[:half], level=1) + gz_member(text[half:], level=9, flags=8), "stream"),
        "empty_members": (gz_member(b"") + gz_member(text) + gz_member(b""), "stream"),
        "bgzf_then_ordinary": (U.bgzf_bytes(text[:half], eof=False) + gz_member(text[half:]), "device"),
        "ordinary_then_bgzf": (gz_member(text[:half]) + U.bgzf_bytes(text[half:]), "stream"),
        "bgzf": (U.bgzf_bytes(text), "device"),
        "stored": (gz_member(text, level=0), "stream"),
        "no_newline": (gz_member(text[:-1]), "stream"),
        "zero_padding": (plain + b"\0" * 100, "stream"),
    }
    for name, (data, road) in sorted(files.items()):
        path = tmp_path / (name + ".fastq.gz")
        path.write_bytes(data)
        want = host_verdict(path, backend, chunk_bytes)
        whole = gzip.decompress(data)
        assert want == whole + (b"" if whole.endswith(b"\n") else b"\n"), name       # (a missing last newline is supplied)
        got = U.read_all(path, backend, chunk_bytes, device_gunzip="any")
        assert got == (want, road), (name, got[1], len(got[0]), len(want))
    # today's paths stay
    (tmp_path / "t.fastq").write_bytes(text)
    assert U.read_all(tmp_path / "t.fastq", backend, chunk_bytes, device_gunzip="any") == (text, None)
    assert U.read_all(tmp_path / "ordinary.fastq.gz", backend, chunk_bytes, device_gunzip=True) == (text, "host")
    assert U.read_all(tmp_path / "ordinary.fastq.gz", backend, chunk_bytes) == (text, "host")
    assert U.read_all(tmp_path / "bgzf.fastq.gz", backend, chunk_bytes, device_gunzip=True) == (text, "device")
    from atropos_amd import fastq
    try:
        fastq.ChunkedFastqReader(str(tmp_path / "ordinary.fastq.gz"), 1 << 16, backend, byte_range=(0, 10), device_gunzip="any")
    except ValueError:
        pass
    else:
        raise AssertionError("a byte range of compressed input was taken")
    # errors: the same exception type as the host path; BadGzipFile names the member's file offset
    first = gz_member(text[:half])
    second = gz_member(text[half:])
    n = len(first) + len(second)
    bad = {
        "crc": first + second[:-8] + bytes([second[-8] ^ 0x10]) + second[-7:],
        "isize": first + second[:-4] + bytes([second[-4] ^ 1]) + second[-3:],
        "cut_data": (first + second)[:n - 300],
        "cut_trailer": (first + second)[:n - 3],
        "cut_header": first + second[:5],
        "garbage_behind": first + b"garbage that is no member",
        "bad_block": first + second[:10] + b"\x07" + second[11:],
        "not_gzip": b"plain text, no gzip at all\n" * 10,
    }
    for name, data in sorted(bad.items()):
        path = tmp_path / ("bad_" + name + ".fastq.gz")
        path.write_bytes(data)
        want = host_verdict(path, backend, chunk_bytes)
        try:
            got = U.read_all(path, backend, chunk_bytes, device_gunzip="any")[0]
        except Exception as e:                                                 # noqa: BLE001
            got = type(e)
            if name in ("crc", "isize"):
                assert isinstance(e, gzip.BadGzipFile) and "offset %d " % len(first) in str(e), (name, str(e))
            if name in ("cut_data", "cut_trailer"):
                assert isinstance(e, EOFError), (name, e)
        if isinstance(want, type) and isinstance(got, type):
            assert issubclass(got, want) or issubclass(want, got), (name, got, want)
        else:
            assert got == want, (name, got if isinstance(got, type) else len(got), want if isinstance(want, type) else len(want))


def check_trim_file(tmp_path, backend=None, fasta=False):
    from atropos_amd.trim import pipeline_from_args
    args = "-a %s -m 30" % G.TRUSEQ
    text = G.fastq_input(nrec=400)
    if fasta:
        lines = text.split(b"\n")
        text = b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 3, 4))
    ext = "fasta" if fasta else "fastq"
    (tmp_path / ("in." + ext)).write_bytes(text)
    (tmp_path / ("in.%s.gz" % ext)).write_bytes(gz_member(text[:30000], flags=8, mem=1) + gz_member(text[30000:], level=1))
    runs = {}
    for name, src, how in (("plain", "in." + ext, {}), ("host", "in.%s.gz" % ext, dict(device_gunzip=False)),
                           ("any", "in.%s.gz" % ext, dict(device_gunzip="any"))):
        runs[name] = pipeline_from_args(args).trim_file(str(tmp_path / src), str(tmp_path / (name + ".out." + ext)), chunk_bytes=7000, **how)
    out = (tmp_path / ("plain.out." + ext)).read_bytes()
    assert runs["plain"]["keep"] > 200 and len(text) // 7000 > 6
    assert runs["any"] == runs["host"] == runs["plain"]
    assert (tmp_path / ("any.out." + ext)).read_bytes() == out and (tmp_path / ("host.out." + ext)).read_bytes() == out


def check_trim_files(tmp_path):
    """Mate 1 an ordinary gzip file, mate 2 BGZF."""
    from atropos_amd.trim import pipeline_from_args
    r1 = G.fastq_input(nrec=300, seed=5)
    lines = G.fastq_input(nrec=300, seed=6).split(b"\n")
    for r in range(300):                                                    # mate 2: 100 bases
        lines[4 * r + 1] = lines[4 * r + 1][:100]
        lines[4 * r + 3] = lines[4 * r + 3][:100]
    r2 = b"\n".join(lines)
    outs = {}
    for name, gz, how in (("plain", False, {}), ("any", True, dict(device_gunzip="any"))):
        ins = []
        for k, text in enumerate((r1, r2)):
            p = tmp_path / ("%s.%d.fastq%s" % (name, k + 1, ".gz" if gz else ""))
            p.write_bytes((gz_member(text) if k == 0 else U.bgzf_bytes(text, size=5000)) if gz else text)
            ins.append(str(p))
        pipe = pipeline_from_args("-a %s -A %s -m 30" % (G.TRUSEQ, G.TRUSEQ), paired_input=True)
        counts = pipe.trim_files(ins[0], ins[1], str(tmp_path / (name + ".o1")), str(tmp_path / (name + ".o2")), chunk_bytes=9000, **how)
        outs[name] = (counts, (tmp_path / (name + ".o1")).read_bytes(), (tmp_path / (name + ".o2")).read_bytes())
    assert outs["any"] == outs["plain"] and outs["plain"][0]["keep"] > 100


def stats_inputs(tmp_path):
    text = G.fastq_input(nrec=300)
    (tmp_path / "q.fastq").write_bytes(text)
    (tmp_path / "q.fastq.gz").write_bytes(gz_member(text, mem=1))             # (blocks far smaller than a chunk)
    return str(tmp_path / "q.fastq"), str(tmp_path / "q.fastq.gz")


def check_stats(tmp_path):
    from atropos_amd import stats
    plain, gz = stats_inputs(tmp_path)
    assert stats.qc_file(gz, chunk_bytes=8000, device_gunzip="any") == stats.qc_file(plain, chunk_bytes=8000)
    assert stats.error_rate_file(gz, chunk_bytes=8000, device_gunzip="any") == stats.error_rate_file(plain, chunk_bytes=8000)


def check_detect(tmp_path):
    from atropos_amd import detect
    plain, gz = stats_inputs(tmp_path)
    known = detect.KnownContaminants()
    known.add("truseq", G.TRUSEQ)
    assert (detect.detect_file(gz, known, max_reads=250, chunk_bytes=8000, device_gunzip="any") ==
            detect.detect_file(plain, known, max_reads=250, chunk_bytes=8000))

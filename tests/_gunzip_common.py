"""Shared by test_gunzip_host.py (the CPU twin, tests/emu/emu_gunzip.cpp) and test_gpu_gunzip.py (the kernel): the BGZF
writer, the block walker, the member cases, the corrupt corpus and the checks of the device gunzip (``bgzf_scan``,
``gunzip_members``, ``device_gunzip=True``).  The oracle for text is ``zlib.decompress(member, 31)`` /
``gzip.decompress``; the members come from ``zlib.compressobj`` (raw deflate, framed here) and from the project's own
compressor.  Nothing here includes or calls the inflater under test except through a backend."""
import functools
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import torch

from . import _deflate_ref as R
from . import _gzip_common as G
from .conftest import ROOT
from .emu.backend import stale, twin_sources

FILL = 0xa5


def build_fuzz():
    """The stand-alone sanitized program (its own ``main``): address and undefined-behaviour sanitizers over the twin."""
    main = os.path.join(ROOT, "tests", "emu", "gunzip_fuzz_main.cpp")
    prog = os.path.join(ROOT, "tests", "emu", "gunzip_fuzz")
    cpps, deps = twin_sources("gunzip")
    if stale(prog, deps + [main]):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-DATR_HOST_EMU", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "atropos_amd", "csrc"), main] + cpps + ["-o", prog])
    return prog


# ---------------------------------------------------------------------------------------------- the BGZF writer
def frame(deflate, crc, isize, before=b""):
    """Raw deflate data inside the BGZF header (extra subfields ``before`` the 'BC' one) and the trailer."""
    size = 12 + len(before) + 6 + len(deflate) + 8
    assert size <= 65536, "a BGZF member holds at most 64 KiB"
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(before) + 6) + before + b"BC\x02\x00" +
            struct.pack("<H", size - 1) + deflate + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff))


def raw_deflate(text, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """``flushes``: (offset in the text, flush mode), in order."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    out, at = [], 0
    for upto, mode in flushes:
        upto = min(upto, len(text))
        out.append(co.compress(text[at:upto]))
        out.append(co.flush(mode))
        at = upto
    out.append(co.compress(text[at:]))
    out.append(co.flush())
    return b"".join(out)


def member(text, before=b"", **how):
    return frame(raw_deflate(text, **how), zlib.crc32(text), len(text), before)


WRITERS = {
    "level0": dict(level=0),
    "level1": dict(level=1),
    "level6": dict(level=6),
    "level9": dict(level=9),
    "fixed": dict(strategy=zlib.Z_FIXED),
    "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(strategy=zlib.Z_RLE),
    "full_flush": dict(flushes=((1, zlib.Z_FULL_FLUSH), (1000, zlib.Z_FULL_FLUSH), (1000, zlib.Z_FULL_FLUSH), (40000, zlib.Z_FULL_FLUSH))),
    "sync_flush": dict(flushes=((777, zlib.Z_SYNC_FLUSH),)),
    "mem1": dict(mem=1),
    "own": None,                      # the project's own compressor: gzip_blocks of the backend under test
}
PERIODS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259)
LENGTHS = (0, 1, 2, 3, 257, 258, 259, 32767, 32768, 32769, 65279, 65280)
FULL = 65280


def _period(p):
    base = np.random.default_rng(1000 + p).permutation(256).astype(np.uint8).tobytes()
    base = (base + base[::-1])[:p]                                          # (p bytes, no shorter period: 256 distinct first)
    return lambda n: G._cycle(base, n)


CONTENTS = dict(G.CONTENTS)
CONTENTS.update({"period_%03d" % p: _period(p) for p in PERIODS})
CONTENTS["quiet"] = lambda n: G._cycle(G._quiet(), n)                      # coded, and no match anywhere


def written(writer, text, backend):
    """One member holding ``text`` (cut down until it fits 64 KiB where the writer does not compress it)."""
    if writer == "own":
        assert len(text) <= FULL
        return G.compress(backend, text) if text else G.EOF
    while True:
        data = raw_deflate(text, **WRITERS[writer])
        if len(data) + 26 <= 65536:
            return frame(data, zlib.crc32(text), len(text))
        text = text[:len(text) * 7 // 8]


_CASES = {}


def member_cases(writer, backend):
    """[(name, member, text)] of one writer: every content at a full block, every length of FASTQ text, for level 6
    every content at every length, and 65 536 bytes of compressible text (the format's largest ISIZE)."""
    key = (writer, backend.name)
    if key not in _CASES:
        picks = [(c, FULL) for c in sorted(CONTENTS)] + [("synth_fastq", n) for n in LENGTHS]
        if writer == "level6":
            picks += [(c, n) for c in sorted(CONTENTS) for n in LENGTHS]
        if writer not in ("own", "level0"):
            picks.append(("synth_fastq", 65536))
        cases = []
        for content, n in picks:
            m = written(writer, CONTENTS[content](n), backend)
            text = zlib.decompress(m, 31)
            assert text == CONTENTS[content](n)[:len(text)] and len(text) >= min(n, 32768)
            cases.append(("%s/%s/%d" % (writer, content, n), m, text))
        _CASES[key] = cases
    return _CASES[key]


# ---------------------------------------------------------------------------------------------- running members
def run_members(backend, members, text_sizes=None, text_start=37, tail=51, stream_off=0, text_off=0):
    """``members`` (bytes each) in one ``gunzip_members`` call.  The text of member m lands where the running sum of
    ``text_sizes`` (default: every member's ISIZE) says, from ``text_start`` on, in a buffer filled with FILL.
    -> (texts, statuses, bad); asserts that every byte outside [text_at[0], text_at[n]) kept the fill."""
    sizes = [struct.unpack("<I", m[-4:])[0] for m in members] if text_sizes is None else list(text_sizes)
    member_at = np.cumsum([0] + [len(m) for m in members]).astype(np.int64)
    text_at = (np.cumsum([0] + sizes) + text_start).astype(np.int64)
    n = int(member_at[-1])
    host = np.zeros(((stream_off + n + 15) // 16 * 16 + 16,), dtype=np.uint8)
    host[stream_off:stream_off + n] = np.frombuffer(b"".join(members), dtype=np.uint8)
    dev = backend.device
    stream = torch.from_numpy(host).to(dev)
    cap = int(text_at[-1]) + tail
    buf = torch.full((text_off + cap,), FILL, dtype=torch.uint8).to(dev)
    status, bad = backend.gunzip_members(stream[stream_off:], n, torch.from_numpy(member_at).to(dev), torch.from_numpy(text_at).to(dev),
                                         len(members), buf[text_off:], cap)
    raw = buf.cpu().numpy()
    lo, hi = text_off + text_start, text_off + int(text_at[-1])
    assert (raw[:lo] == FILL).all() and (raw[hi:] == FILL).all(), "a store outside the members' text"
    texts = [raw[text_off + int(a):text_off + int(b)].tobytes() for a, b in zip(text_at[:-1], text_at[1:])]
    return texts, status.cpu().tolist()[:len(members)], int(bad.item())


def check_members(backend, cases):
    texts, status, bad = run_members(backend, [c[1] for c in cases])
    for (name, _, want), got, st in zip(cases, texts, status):
        assert st == 0, (name, st)
        assert got == want, name
    assert bad == 0


# ---------------------------------------------------------------------------------------------- the block walker
_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def data_start(m):
    return 12 + struct.unpack("<H", m[10:12])[0]


def walk(m):
    """The deflate blocks of one member, read from its bits: [dict(btype, bfinal, start, end (bit positions; end is
    behind the end-of-block code or the stored bytes), text_at, size, matches [(pos, length, distance)], ll_lens,
    d_lens)].  Checks itself against zlib."""
    bits = R._Bits(m, data_start(m))
    text, blocks = bytearray(), []
    while True:
        b = dict(start=bits.pos, bfinal=bits.take(1), btype=bits.take(2), text_at=len(text), matches=[], ll_lens=None, d_lens=None)
        assert b["btype"] != 3
        if b["btype"] == 0:
            bits.pos = (bits.pos + 7) // 8 * 8
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xffff
            text += m[bits.pos // 8:bits.pos // 8 + n]
            bits.pos += 8 * n
        else:
            if b["btype"] == 1:
                ll_lens, d_lens = _FIXED_LL, [5] * 32
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[R.CL_ORDER[i]] = bits.take(3)
                cl_table, cl_max = R._decode_table(cl_lens)
                lens = []
                while len(lens) < hlit + hdist:
                    sym, _ = R._symbol(bits, cl_table, cl_max)
                    if sym < 16:
                        lens.append(sym)
                    elif sym == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    else:
                        lens += [0] * ((3 if sym == 17 else 11) + bits.take(3 if sym == 17 else 7))
                assert len(lens) == hlit + hdist
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
            b["ll_lens"], b["d_lens"] = ll_lens, d_lens
            ll_table, ll_max = R._decode_table(ll_lens)
            d_table, d_max = R._decode_table(d_lens)
            while True:
                sym, _ = R._symbol(bits, ll_table, ll_max)
                if sym < 256:
                    text.append(sym)
                elif sym == 256:
                    break
                else:
                    length = R.LEN_BASE[sym - 257] + bits.take(R.LEN_EXTRA[sym - 257])
                    dsym, _ = R._symbol(bits, d_table, d_max)
                    dist = R.DIST_BASE[dsym] + bits.take(R.DIST_EXTRA[dsym])
                    b["matches"].append((len(text), length, dist))
                    for _ in range(length):
                        text.append(text[-dist])
        b["end"], b["size"] = bits.pos, len(text) - b["text_at"]
        blocks.append(b)
        if b["bfinal"]:
            break
    assert bytes(text) == zlib.decompress(m, 31) and (bits.pos + 7) // 8 == len(m) - 8
    return blocks


def fixture_conditions(backend):
    """What the member cases are named after, read from the parsed streams.  zlib never writes a distance above
    32 506 (its window less its look-ahead) and always sends two distance codes, so the match at 32 768, the block
    with exactly one distance code and the block without any come from the project's own compressor."""
    text = G.ratio_fixture("uniform")[:FULL]
    seen = set()
    walks = {w: walk(written(w, text, backend)) for w in ("level0", "level6", "fixed", "huffman_only", "rle", "full_flush", "sync_flush", "mem1")}
    for blocks in walks.values():
        seen |= {b["btype"] for b in blocks}
    assert seen == {0, 1, 2}
    assert [b["btype"] for b in walks["level0"]] == [0, 0] and walks["level0"][1]["size"] == 0
    assert all(b["btype"] == 1 for b in walks["fixed"])
    assert len(walks["level6"]) >= 2 and len(walks["mem1"]) >= 64
    assert any(len(b) >= 3 for b in walks.values())
    assert len(walks["huffman_only"]) >= 3 and all(b["btype"] == 2 and not b["matches"] for b in walks["huffman_only"])
    assert all(d == 1 for b in walks["rle"] for _, _, d in b["matches"]) and any(b["matches"] for b in walks["rle"])
    ff = walks["full_flush"]
    assert [b["btype"] for b in ff[:3]] == [1, 0, 2] and ff[1]["size"] == 0
    # an empty stored block between coded blocks; a coded block that ends inside a byte before a stored one
    between = [i for i in range(1, len(ff) - 1) if ff[i]["btype"] == 0 and ff[i]["size"] == 0 and ff[i - 1]["btype"] and ff[i + 1]["btype"]]
    assert between and any(ff[i - 1]["end"] % 8 for i in between)
    sf = walks["sync_flush"]
    assert sf[0]["btype"] != 0 and sf[1]["btype"] == 0 and sf[1]["size"] == 0 and sf[0]["size"] == 777
    # a match whose source lies in an earlier block
    assert any(pos - d < b["text_at"] for b in sf[2:] for pos, _, d in b["matches"])
    # a 15-bit literal/length code
    fib = walk(written("huffman_only", CONTENTS["fibonacci"](FULL), backend))
    assert max(max(b["ll_lens"]) for b in fib) == 15
    # the largest member
    big = written("level6", CONTENTS["random"](FULL), backend)
    assert len(big) > 65300 and all(b["btype"] == 0 for b in walk(big))
    assert struct.unpack("<I", written("level6", CONTENTS["synth_fastq"](65536), backend)[-4:])[0] == 65536
    # the project's own compressor: distance 32 768, exactly one distance code, no distance code at all
    edge = walk(written("own", CONTENTS["window_edge"](FULL), backend))
    assert any(d == 32768 for b in edge for _, _, d in b["matches"])
    one = walk(written("own", CONTENTS["one_byte"](FULL), backend))
    assert [sum(1 for l in b["d_lens"] if l) for b in one] == [1] and one[0]["matches"]
    none = walk(written("own", CONTENTS["quiet"](FULL), backend))
    assert none[0]["btype"] == 2 and not any(none[0]["d_lens"]) and not none[0]["matches"]
    # overlapping copies (distance below the length) around the lane count, the longest match among them
    lengths = {l for p in (1, 63, 64, 65, 258, 259) for b in walk(written("level6", CONTENTS["period_%03d" % p](FULL), backend))
               for _, l, d in b["matches"] if d < l}
    assert 258 in lengths and len(lengths) >= 2


# ---------------------------------------------------------------------------------------------- launch
def mixed_members(backend, count):
    """``count`` members of unlike text sizes, a few hundred bytes to a full block, empty ones interleaved."""
    pool = []
    src = CONTENTS["synth_fastq"](FULL)
    for i, n in enumerate((301, 0, 1023, 4099, 777, 0, 65280, 513, 12345, 2, 33001, 0, 999, 257, 5000, 611)):
        w = ("level6", "level1", "fixed", "level0", "own", "huffman_only")[i % 6]
        text = src[i * 97:i * 97 + n]
        pool.append((written(w, text, backend), text))
    return [pool[i % len(pool)] for i in range(count)]


def check_launch(backend, count):
    cases = mixed_members(backend, count)
    if count == 0:
        texts, status, bad = run_members(backend, [])
        assert texts == [] and bad == 0
        return
    texts, status, bad = run_members(backend, [m for m, _ in cases])
    assert bad == 0 and not any(status)
    for i, ((_, want), got) in enumerate(zip(cases, texts)):
        assert got == want, "member %d" % i


def check_independence(backend):
    """A member coded with short tables behind a member with 15-bit codes (and the other way round, and behind a
    stored and an empty one): every member's text is what that member gives alone."""
    deep = written("huffman_only", CONTENTS["fibonacci"](FULL), backend)
    flat = written("own", CONTENTS["one_byte"](4000), backend)
    stored = written("level0", CONTENTS["random"](3000), backend)
    seq = [deep, flat, G.EOF, deep, stored, flat, deep, flat]
    texts, status, bad = run_members(backend, seq)
    assert bad == 0 and not any(status)
    for m, got in zip(seq, texts):
        assert got == zlib.decompress(m, 31)
        assert run_members(backend, [m])[0][0] == got


# ---------------------------------------------------------------------------------------------- the corrupt corpus
class _BitWriter(object):
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):                     # least significant bit first
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def code(self, code, nbits):                     # a Huffman code: most significant bit first
        self.put(int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _canonical(lens):
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for sym, l in enumerate(lens):
        if l:
            out[sym] = (nxt[l], l)
            nxt[l] += 1
    return out


_CL_LENS = [4] * 13 + [5] * 6                        # a complete code over the 19 code-length symbols


def _fixed_code(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xc0 + sym - 280, 8)


def _fixed_member(symbols, isize):
    """BFINAL, BTYPE 01, then ``symbols``: an int is a literal/length symbol, a ("d", code) a 5-bit distance code."""
    w = _BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    for s in symbols:
        if isinstance(s, tuple):
            w.code(s[1], 5)
        else:
            _fixed_code(w, s)
    return frame(w.bytes(), zlib.crc32(b"A"), isize)


def _rebuilt(base, ll_lens, d_lens, cl_syms=None):
    """The single dynamic block of ``base`` with its header written anew: HCLEN 19, the fixed code-length code, the
    code lengths ``ll_lens`` + ``d_lens`` one symbol each (or ``cl_syms``: [(symbol, extra value)]), then the
    block's own token bits."""
    (b,) = walk(base)
    w = _BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(len(ll_lens) - 257, 5)
    w.put(len(d_lens) - 1, 5)
    w.put(15, 4)
    for s in R.CL_ORDER:
        w.put(_CL_LENS[s], 3)
    codes = _canonical(_CL_LENS)
    for sym, extra in (cl_syms if cl_syms is not None else [(l, 0) for l in list(ll_lens) + list(d_lens)]):
        w.code(*codes[sym])
        w.put(extra, {16: 2, 17: 3, 18: 7}.get(sym, 0))
    # the tokens: from behind the original header to the end-of-block code
    first = _header_end(base)
    stream = int.from_bytes(base, "little")
    w.put(stream >> first, b["end"] - first)
    return frame(w.bytes(), struct.unpack("<I", base[-8:-4])[0], struct.unpack("<I", base[-4:])[0])


def _header_end(m):
    """Bit position of the first token of the single dynamic block of ``m``."""
    bits = R._Bits(m, data_start(m))
    assert bits.take(3) == 5
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    cl_lens = [0] * 19
    for i in range(hclen):
        cl_lens[R.CL_ORDER[i]] = bits.take(3)
    table, mx = R._decode_table(cl_lens)
    n = 0
    while n < hlit + hdist:
        sym, _ = R._symbol(bits, table, mx)
        n += 1 if sym < 16 else 3 + bits.take(2) if sym == 16 else 3 + bits.take(3) if sym == 17 else 11 + bits.take(7)
    return bits.pos


def _flip(m, bit):
    out = bytearray(m)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def corrupt_corpus():
    """{name: member}: one member per rule of the inflater, each made from a valid member by editing its bits or its
    trailer, each rejected by ``zlib.decompress(member, 31)``.  Also "rebuilt": the valid member the header cases
    are edits of, with the same rewritten header -- so that what is rejected is the edit."""
    text = CONTENTS["synth_fastq"](3000)
    base = member(text, level=6)
    (b,) = walk(base)
    assert b["btype"] == 2
    ll, d = list(b["ll_lens"]), list(b["d_lens"])
    at = 8 * data_start(base)
    out = {"rebuilt": _rebuilt(base, ll, d)}
    assert zlib.decompress(out["rebuilt"], 31) == text
    out["btype_11"] = _flip(base, at + 1)
    stored = member(text, level=0)
    out["len_nlen"] = _flip(stored, at + 8 + 16 + 3)
    used = max(s for s in range(256) if ll[s] and ll[s] < 15)
    assert ll[used] >= 2
    out["oversubscribed"] = _rebuilt(base, ll[:used] + [ll[used] - 1] + ll[used + 1:], d)
    out["incomplete"] = _rebuilt(base, ll[:used] + [ll[used] + 1] + ll[used + 1:], d)
    out["no_end_of_block"] = _rebuilt(base, ll[:256] + [0] + ll[257:], d)
    plain = [(l, 0) for l in ll + d]
    out["repeat_first"] = _rebuilt(base, ll, d, [(16, 0)] + plain[3:])
    out["repeat_past_end"] = _rebuilt(base, ll, d, plain[:-5] + [(18, 127)])
    A = ord("A")
    out["symbol_286"] = _fixed_member([A, 286, 256], 1)
    out["symbol_287"] = _fixed_member([A, 287, 256], 1)
    out["distance_30"] = _fixed_member([A, 257, ("d", 30), 256], 4)
    out["distance_31"] = _fixed_member([A, 257, ("d", 31), 256], 4)
    out["distance_before_start"] = _fixed_member([A, 257, ("d", 1), 256], 4)
    n = len(text)
    out["output_past_isize"] = base[:-4] + struct.pack("<I", n - 1)
    out["output_short_of_isize"] = base[:-4] + struct.pack("<I", n + 1)
    out["input_into_trailer"] = _flip(base, b["start"])                       # BFINAL cleared: the next header is the trailer
    out["crc"] = _flip(base, 8 * (len(base) - 8) + 5)
    for name, m in out.items():
        if name == "rebuilt":
            continue
        try:
            zlib.decompress(m, 31)
        except zlib.error:
            continue
        raise AssertionError("zlib takes the corrupt member %r" % name)
    return out


# the rule each corrupt member breaks, as the status of inflate_core.hpp (INF_E_*) that names it
CORPUS_STATUS = {
    "btype_11": 5, "len_nlen": 6, "oversubscribed": 7, "incomplete": 7, "no_end_of_block": 8, "repeat_first": 9,
    "repeat_past_end": 9, "symbol_286": 10, "symbol_287": 10, "distance_30": 10, "distance_31": 10,
    "distance_before_start": 11, "output_past_isize": 12, "output_short_of_isize": 4, "input_into_trailer": 13, "crc": 14,
}


def check_ranges(backend):
    """Ranges that are none -- member offsets that run backwards or beyond the stream, text offsets that run backwards
    or beyond the capacity -- are status 1 for that member, before anything of it is read; the other member is right."""
    good = [member(CONTENTS["synth_fastq"](1500 + 700 * i), level=6) for i in range(2)]
    sizes = [len(g) for g in good]
    texts = [zlib.decompress(g, 31) for g in good]
    n = sum(sizes)
    host = np.zeros(((n + 15) // 16 * 16,), dtype=np.uint8)
    host[:n] = np.frombuffer(b"".join(good), dtype=np.uint8)
    dev = backend.device
    t = [len(x) for x in texts]
    cap = 40 + t[0] + t[1] + 40
    at, tt = [0, sizes[0], n], [40, 40 + t[0], 40 + t[0] + t[1]]
    # (member_at, text_at, capacity, the member that is refused)
    cases = [([0, sizes[0], sizes[0] - 5], tt, cap, 1),                       # member offsets run backwards
             ([0, sizes[0], n + 16], tt, cap, 1),                             # ... beyond the stream
             (at, [40, 40 + t[0], 39], cap, 1),                               # text offsets run backwards
             (at, tt, tt[2] - 1, 1),                                          # ... beyond the capacity
             (at, [-1, t[0] - 1, t[0] - 1 + t[1]], cap, 0)]                   # ... before the text
    for member_at, text_at, capacity, refused in cases:
        buf = torch.full((cap,), FILL, dtype=torch.uint8).to(dev)
        status, bad = backend.gunzip_members(torch.from_numpy(host).to(dev), n, torch.tensor(member_at, dtype=torch.int64).to(dev),
                                             torch.tensor(text_at, dtype=torch.int64).to(dev), 2, buf, capacity)
        status, raw = status.cpu().tolist()[:2], buf.cpu().numpy()
        assert int(bad.item()) == 1 and status[refused] == 1 and status[1 - refused] == 0, (member_at, text_at, status)
        k = 1 - refused
        a, b = text_at[k], text_at[k + 1]
        assert raw[a:b].tobytes() == texts[k], (member_at, text_at)
        assert (raw[:a] == FILL).all() and (raw[b:] == FILL).all(), "a store outside the one good member's text"


def check_corpus(backend):
    """Every corrupt member between two valid ones: a nonzero status exactly for the corrupt ones, the neighbours'
    text right, nothing outside the text ranges touched."""
    corpus = corrupt_corpus()
    names = [n for n in sorted(corpus) if n != "rebuilt"]
    good = [member(CONTENTS["synth_fastq"](2000 + 13 * i), level=(1, 6, 0)[i % 3]) for i in range(len(names) + 1)]
    seq = [good[0]]
    for i, n in enumerate(names):
        seq += [corpus[n], good[i + 1]]
    texts, status, bad = run_members(backend, seq)
    assert bad == len(names)
    for i, m in enumerate(seq):
        if i % 2:
            assert status[i] == CORPUS_STATUS[names[i // 2]], (names[i // 2], status[i])
        else:
            assert status[i] == 0 and texts[i] == zlib.decompress(m, 31), i
    assert run_members(backend, [corpus["rebuilt"]])[1] == [0]
    # a text range that is not the member's ISIZE (ranges that are none: check_ranges)
    base = good[1]
    n = struct.unpack("<I", base[-4:])[0]
    for sizes in ([n - 1], [n + 1], [0]):
        assert run_members(backend, [base], text_sizes=sizes)[1] != [0]
    return dict(zip(names, [status[2 * i + 1] for i in range(len(names))]))


def check_reader_offsets(backend, tmp_path):
    """Through the reader: ``BadGzipFile`` names the file offset of the member that fails."""
    from atropos_amd import fastq
    corpus = corrupt_corpus()
    text = G.fastq_input(nrec=12)
    good = member(text, level=6)
    for name in sorted(corpus):
        if name == "rebuilt":
            continue
        path = tmp_path / ("bad_%s.fastq.gz" % name)
        path.write_bytes(good + good + corpus[name] + good + G.EOF)
        try:
            for _ in fastq.read_chunks([str(path)], 1 << 16, backend, device_gunzip=True):
                pass
        except gzip.BadGzipFile as e:
            assert "offset %d " % (2 * len(good)) in str(e), (name, str(e))
        else:
            raise AssertionError("no BadGzipFile for %r" % name)


# ---------------------------------------------------------------------------------------------- drivers
def bgzf_bytes(text, size=3000, level=6, eof=True):
    """``text`` as a BGZF file of members of ``size`` bytes of text."""
    return b"".join(member(text[lo:lo + size], level=level) for lo in range(0, len(text), size)) + (G.EOF if eof else b"")


def read_all(path, backend, chunk_bytes=1 << 14, **how):
    """The text of every chunk of ``read_chunks`` (whole records only), and the reader's ``inflate_path``."""
    from atropos_amd import fastq
    out, seen = [], []
    real = fastq.ChunkedFastqReader

    class Spy(real):
        def __init__(self, *a, **k):
            real.__init__(self, *a, **k)
            seen.append(self.inflate_path)

    fastq.ChunkedFastqReader = Spy
    try:
        for (b,) in fastq.read_chunks([str(path)], chunk_bytes, backend, **how):
            if len(b):                                                        # (a chunk's whole records stand at its front)
                out.append(bytes(b.data[:int(b.line_ends[4 * len(b) - 1].item()) + 1].cpu().numpy().tobytes()))
    finally:
        fastq.ChunkedFastqReader = real
    return b"".join(out), seen[0]


def check_trim_file(tmp_path, args="-a %s -m 30" % G.TRUSEQ):
    from atropos_amd.trim import pipeline_from_args
    text = G.fastq_input(nrec=400)
    (tmp_path / "in.fastq").write_bytes(text)
    (tmp_path / "in.fastq.gz").write_bytes(bgzf_bytes(text, size=5000))
    runs = {}
    for name, src, how in (("plain", "in.fastq", {}), ("host", "in.fastq.gz", dict(device_gunzip=False)),
                           ("device", "in.fastq.gz", dict(device_gunzip=True))):
        runs[name] = pipeline_from_args(args).trim_file(str(tmp_path / src), str(tmp_path / (name + ".out")), chunk_bytes=7000, **how)
    out = (tmp_path / "plain.out").read_bytes()
    assert runs["plain"]["keep"] > 200 and len(text) // 7000 > 10
    assert runs["device"] == runs["host"] == runs["plain"]
    assert (tmp_path / "device.out").read_bytes() == out and (tmp_path / "host.out").read_bytes() == out


def check_trim_files(tmp_path):
    """Mates of different record sizes: the file with the smaller records carries its surplus over every chunk."""
    from atropos_amd.trim import pipeline_from_args
    r1 = G.fastq_input(nrec=300, seed=5)
    lines = G.fastq_input(nrec=300, seed=6).split(b"\n")
    for r in range(300):                                                    # mate 2: 100 bases
        lines[4 * r + 1] = lines[4 * r + 1][:100]
        lines[4 * r + 3] = lines[4 * r + 3][:100]
    r2 = b"\n".join(lines)
    outs = {}
    for name, gz, how in (("plain", False, {}), ("device", True, dict(device_gunzip=True))):
        ins = []
        for k, text in enumerate((r1, r2)):
            p = tmp_path / ("%s.%d.fastq%s" % (name, k + 1, ".gz" if gz else ""))
            p.write_bytes(bgzf_bytes(text, size=4000 + 1000 * k) if gz else text)
            ins.append(str(p))
        pipe = pipeline_from_args("-a %s -A %s -m 30" % (G.TRUSEQ, G.TRUSEQ), paired_input=True)
        counts = pipe.trim_files(ins[0], ins[1], str(tmp_path / (name + ".o1")), str(tmp_path / (name + ".o2")), chunk_bytes=9000, **how)
        outs[name] = (counts, (tmp_path / (name + ".o1")).read_bytes(), (tmp_path / (name + ".o2")).read_bytes())
    assert outs["device"] == outs["plain"] and outs["plain"][0]["keep"] > 100


def _stats_inputs(tmp_path):
    text = G.fastq_input(nrec=300)
    (tmp_path / "q.fastq").write_bytes(text)
    (tmp_path / "q.fastq.gz").write_bytes(bgzf_bytes(text, size=6000))
    return str(tmp_path / "q.fastq"), str(tmp_path / "q.fastq.gz")


def check_stats(tmp_path):
    from atropos_amd import stats
    plain, gz = _stats_inputs(tmp_path)
    assert stats.qc_file(gz, chunk_bytes=8000, device_gunzip=True) == stats.qc_file(plain, chunk_bytes=8000)
    assert stats.qc_files(gz, gz, chunk_bytes=8000, device_gunzip=True) == stats.qc_files(plain, plain, chunk_bytes=8000)
    assert stats.error_rate_file(gz, chunk_bytes=8000, device_gunzip=True) == stats.error_rate_file(plain, chunk_bytes=8000)
    assert stats.error_rate_file(gz, gz, chunk_bytes=8000, device_gunzip=True) == stats.error_rate_file(plain, plain, chunk_bytes=8000)


def check_detect(tmp_path):
    from atropos_amd import detect
    plain, gz = _stats_inputs(tmp_path)
    known = detect.KnownContaminants()
    known.add("truseq", G.TRUSEQ)
    assert (detect.detect_file(gz, known, max_reads=250, chunk_bytes=8000, device_gunzip=True) ==
            detect.detect_file(plain, known, max_reads=250, chunk_bytes=8000))
    assert (detect.detect_files(gz, gz, known, max_reads=250, chunk_bytes=8000, device_gunzip=True) ==
            detect.detect_files(plain, plain, known, max_reads=250, chunk_bytes=8000))


def check_round_trip(tmp_path):
    """What ``device_gzip=True`` writes, read back with ``device_gunzip=True``."""
    from atropos_amd.trim import pipeline_from_args
    args = "-a %s -m 30" % G.TRUSEQ
    (tmp_path / "in.fastq").write_bytes(G.fastq_input(nrec=500))
    pipeline_from_args(args).trim_file(str(tmp_path / "in.fastq"), str(tmp_path / "a.fastq"), chunk_bytes=1 << 16)
    pipeline_from_args(args).trim_file(str(tmp_path / "in.fastq"), str(tmp_path / "a.fastq.gz"), chunk_bytes=1 << 16, device_gzip=True)
    for out, how in (("b.fastq", {}), ("b.fastq.gz", dict(device_gzip=True))):
        pipeline_from_args("-m 1").trim_file(str(tmp_path / "a.fastq.gz"), str(tmp_path / out), chunk_bytes=1 << 15,
                                             device_gunzip=True, **how)
    want = (tmp_path / "a.fastq").read_bytes()
    assert len(want) > 50000 and (tmp_path / "b.fastq").read_bytes() == want
    assert gzip.decompress((tmp_path / "b.fastq.gz").read_bytes()) == want


def check_inputs(backend, tmp_path):
    """Path selection, empty members, the missing end marker, the missing last newline, and the three errors."""
    text = G.fastq_input(nrec=120)
    # not BGZF: the host path, the same text
    (tmp_path / "plain.fastq.gz").write_bytes(gzip.compress(text))
    assert read_all(tmp_path / "plain.fastq.gz", backend, device_gunzip=True) == (text, "host")
    (tmp_path / "t.fastq").write_bytes(text)
    assert read_all(tmp_path / "t.fastq", backend, device_gunzip=True) == (text, None)
    # the default: today's path
    bg = bgzf_bytes(text)
    (tmp_path / "b.fastq.gz").write_bytes(bg)
    assert read_all(tmp_path / "b.fastq.gz", backend) == (text, "host")
    assert read_all(tmp_path / "b.fastq.gz", backend, device_gunzip=True) == (text, "device")
    # cat a.gz b.gz: an end marker in the middle, empty members anywhere, no end marker at the end, a subfield before 'BC'
    half = len(text) // 2
    cat = (G.EOF + bgzf_bytes(text[:half]) + G.EOF + G.EOF + member(text[half:half + 100], before=b"XY\x03\x00abc") +
           bgzf_bytes(text[half + 100:], size=1500, eof=False))
    (tmp_path / "cat.fastq.gz").write_bytes(cat)
    assert gzip.decompress(cat) == text
    assert read_all(tmp_path / "cat.fastq.gz", backend, device_gunzip=True) == (text, "device")
    (tmp_path / "only_eof.fastq.gz").write_bytes(G.EOF)
    assert read_all(tmp_path / "only_eof.fastq.gz", backend, device_gunzip=True) == (b"", "device")
    # errors: cut inside the last member, a flipped CRC byte, a plain gzip member behind BGZF members
    cases = (("cut", bg[:-28 - 11], EOFError), ("crc", bg[:-28 - 7] + bytes([bg[-28 - 7] ^ 0x10]) + bg[-28 - 6:], gzip.BadGzipFile),
             ("mixed", bgzf_bytes(text, eof=False) + gzip.compress(text), gzip.BadGzipFile))
    for name, data, error in cases:
        path = tmp_path / (name + ".fastq.gz")
        path.write_bytes(data)
        for how in (dict(device_gunzip=True), {}):
            try:
                read_all(path, backend, **how)
            except error:
                continue
            except Exception as e:                                             # noqa: BLE001
                raise AssertionError("%s: %r instead of %s" % (name, e, error.__name__))
            if how or name != "mixed":                                         # (the host path reads on through any gzip member)
                raise AssertionError("%s: no %s" % (name, error.__name__))
    from atropos_amd import fastq
    try:
        fastq.ChunkedFastqReader(str(tmp_path / "b.fastq.gz"), 1 << 16, backend, byte_range=(0, 10), device_gunzip=True)
    except ValueError:
        pass
    else:
        raise AssertionError("a byte range of compressed input was taken")

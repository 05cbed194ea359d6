"""Shared by test_pairtext_host.py (the CPU twin, tests/emu/emu_pairtext.cpp) and test_gpu_pairtext.py (the kernels of
atropos_amd/csrc/pairtext_kernels.hip): the pair formatter ``atr_fastq_emit_pairs`` at the C ABI against the plain
Python model of ``_fastq_kernels_common`` (``model_format`` of the interleaved record list), and the interleaved
file drivers against the reference's files (tests/golden/pairtext.json.gz).

Also builds and loads the twin libraries of the paired-text and of the read-statistics entry points (emu_pairtext.cpp,
emu_stats.cpp) and defines the backend that serves them (``PairTextEmuBackend``); the test module installs it in a
fixture of its own."""
import base64
import ctypes as C
import os
import subprocess

import numpy as np
import torch

from atropos_amd import _lib
from tests import _fastq_kernels_common as K
from tests.emu import backend as emu

PAIR_ENTRY_POINTS = ("atr_fastq_emit_pairs_work_bytes", "atr_fastq_emit_pairs", "atr_overwrite_work_bytes",
                     "atr_overwrite_plan_batch", "atr_overwrite_apply_batch")
STATS_ENTRY_POINTS = ("atr_read_stats_bytes", "atr_read_stats_clear", "atr_read_stats_batch", "atr_read_stats_merge")
# twin library -> (its source, the product headers it is built from, the entry points it stands in for)
NEW_TWINS = {"pairtext": ("emu_pairtext.cpp", ("pairtext_core.hpp", "fastq_core.hpp"), PAIR_ENTRY_POINTS),
             "stats": ("emu_stats.cpp", ("stats_core.hpp", "fastq_core.hpp"), STATS_ENTRY_POINTS)}
# atr_fastq_emit_pairs' staged instantiations: pair_bytes_hint -> (pairs per tile, bytes per stage)
PAIR_VARIANTS = ((0, 8, 13312), (700, 4, 3328), (780, 8, 6656))
_twins = {}


# ---------------------------------------------------------------------------------------------- the twins
def build_new_twin(name):
    """tests/emu/libemu_<name>.so from its .cpp and the product's per-lane code, by ``build_twin``'s g++ line."""
    src, headers, _ = NEW_TWINS[name]
    so = os.path.join(emu._HERE, "libemu_%s.so" % name)
    cpp = os.path.join(emu._HERE, src)
    deps = [cpp, os.path.join(emu._HERE, "emu_abi.hpp"), os.path.join(emu._ROOT, "include", "atropos_hip.h")] + [
        os.path.join(emu._CSRC, f) for f in headers]
    if emu.stale(so, deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU"] + emu._INC + [cpp, "-o", so])
    return so


def load_new_twin(name):
    if name not in _twins:
        lib = C.CDLL(build_new_twin(name))
        _twins[name] = _lib.attach_prototypes(lib, "emu_", NEW_TWINS[name][2])
    return _twins[name]


class PairTextEmuBackend(emu.EmuBackend, _lib.PairTextCalls, _lib.StatsCalls):
    """The CPU stand-in with the paired-text and the read-statistics entry points: those go to twin libraries of
    their own (emu_pairtext.cpp, emu_stats.cpp)."""

    def _call(self, name, *args):
        twin = next((t for t, row in NEW_TWINS.items() if name in row[2]), None)
        if twin is None:
            return super()._call(name, *args)
        fn, at = load_new_twin(twin)[name]
        return _lib._check(None, fn(*args) if at is None else fn(*args[:at], None, *args[at:]), name)

    _host = _call

    def _symbol_of(self, name):
        """The bare ctypes function of one of the new twins' entry points."""
        twin = next(t for t, row in NEW_TWINS.items() if name in row[2])
        return load_new_twin(twin)[name][0]


# ---------------------------------------------------------------------------------------------- formatter: cases
def _take(case, idx):
    """The records ``idx`` of a formatter case as one mate: descriptors and per-record arrays."""
    out = dict(data=case["data"], recs=[case["recs"][i] for i in idx])
    for key in ("begin", "end", "ubegin", "uend"):
        out[key] = None if case[key] is None else np.asarray(case[key])[idx]
    return out


def pair_cases():
    """{layout: (mate 1, mate 2, dest per pair, which)} over ``formatter_case`` texts (names of 0..40 bytes, reads of
    0..2 900 bases, LF and CRLF, '+name' lines, random intervals and masks):
    'interleaved' -- one chunk, the even records are read 1 and the odd ones read 2 (what ``-l`` hands over);
    'halves' -- one chunk, its first half read 1 and its second half read 2 (one buffer, two far spans);
    'two' -- two chunks."""
    if not _CASES:
        one = K.formatter_case(nrec=600, seed=5)
        a, b = K.formatter_case(nrec=300, seed=7), K.formatter_case(nrec=300, seed=8)
        rng = np.random.default_rng(41)
        dest = rng.integers(0, 3, 300)
        every = np.arange(600)
        _CASES.update(interleaved=(_take(one, every[0::2]), _take(one, every[1::2]), dest, 1),
                      halves=(_take(one, every[:300]), _take(one, every[300:]), dest, 1),
                      two=(_take(a, np.arange(300)), _take(b, np.arange(300)), dest, 1))
    return _CASES


_CASES = {}


def model_pairs(m1, m2, dest, which, lo, hi, masks=True, use_dest=True):
    """(text, offsets[n + 1]) of the pairs [lo, hi): ``model_format`` over the interleaved record list.  Two chunks
    are modelled as one text, the second behind the first."""
    same = m1["data"] is m2["data"]
    data = m1["data"] if same else m1["data"] + m2["data"]
    shift = 0 if same else len(m1["data"])
    recs, begin, end, ubegin, uend, dst = [], [], [], [], [], []
    for p in range(lo, hi):
        for m, off in ((m1, 0), (m2, shift)):
            no, nl, so, sl, qo, ql, fl, rs = m["recs"][p]
            recs.append([no + off, nl, so + off, sl, qo + off, ql, fl, rs + off if fl & 2 else rs])
            begin.append(m["begin"][p])
            end.append(m["end"][p])
            masked = masks and m["ubegin"] is not None
            ubegin.append(m["ubegin"][p] if masked else m["begin"][p])
            uend.append(m["uend"][p] if masked else max(m["begin"][p], m["end"][p]))
            dst.append(dest[p] if use_dest else which)
    text, offs = K.model_format(data, recs, begin, end, ubegin, uend, dst, which)
    return text, offs[0::2]


def pair_tile_report(m1, m2, offsets, tile, stage, addr1, addr2, addr_out):
    """Which way emit_pairs_staged_kernel<tile, stage> takes every tile, from the descriptors, the model's offsets
    and the three base addresses (mod 16): 'one' (both reads staged as one span), 'two' (side by side),
    'overflow' (stageable but beyond the stage), 'unordered', 'empty'."""
    rep = dict(one=0, two=0, overflow=0, unordered=0, empty=0)
    n = len(offsets) - 1

    def stageable(m, p, lo, hi):
        no, nl, so, sl, qo, ql, fl, _ = m["recs"][p]
        a = int(m["begin"][p])
        b = max(a, int(m["end"][p]))
        return (no - 1 >= lo and qo + ql <= hi and so >= no - 1 and no + nl <= so and so + sl <= qo and not fl & 2 and a >= 0 and
                b <= sl and (b == a or b <= ql))

    for t0 in range(0, n, tile):
        t1 = min(t0 + tile, n)
        out_lo, out_hi = offsets[t0], offsets[t1]
        if out_hi == out_lo:
            rep["empty"] += 1
            continue
        span = [(m["recs"][t0][0] - 1, m["recs"][t1 - 1][4] + m["recs"][t1 - 1][5]) for m in (m1, m2)]
        if not all(stageable(m, p, *span[k]) for k, m in enumerate((m1, m2)) for p in range(t0, t1)):
            rep["unordered"] += 1
            continue
        (lo1, hi1), (lo2, hi2) = span
        mis1, mis2 = (addr1 + lo1) & 15, (addr2 + lo2) & 15
        ulo, uhi = min(lo1, lo2), max(hi1, hi2)
        umis = (addr1 + ulo) & 15
        one = m1["data"] is m2["data"] and addr1 == addr2 and (uhi - ulo) + umis + 16 <= stage
        side2 = (mis1 + (hi1 - lo1) + 15) & ~15
        need_in = (uhi - ulo) + umis if one else side2 + mis2 + (hi2 - lo2)
        mis_out = (addr_out + out_lo) & 15
        if need_in + 16 <= stage and (out_hi - out_lo) + mis_out + 16 <= stage:
            rep["one" if one else "two"] += 1
        else:
            rep["overflow"] += 1
    return rep


# ---------------------------------------------------------------------------------------------- formatter: calls
def emit_pairs_call(be, dev, n, dest, which, hint, out_misalign=0):
    """atr_fastq_emit_pairs (or the twin's) called directly: the sizing call, then the write into a view of a 0xEE
    pool with GUARD bytes in front of it and behind ``total``.  ``dev``: the twelve per-mate tensors.  Returns
    (offsets list, text bytes, guards untouched)."""
    ptr = _lib._ptr
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=be.device)
    work = be.empty((max(be._host("atr_fastq_emit_pairs_work_bytes", n), 16),), torch.uint8)

    def call(out_ptr):
        be._call("atr_fastq_emit_pairs", *[ptr(t) for t in dev], ptr(dest), which, n, hint, ptr(offsets), ptr(work), out_ptr)
    call(None)
    K._sync(be)
    offs = offsets.cpu().tolist()
    total = offs[n]
    pool = torch.full((K.GUARD + 16 + total + K.GUARD,), 0xEE, dtype=torch.uint8, device=be.device)
    assert pool.data_ptr() % 16 == 0 and 0 <= out_misalign < 16
    start = K.GUARD + out_misalign
    call(C.c_void_p(pool.data_ptr() + start))
    K._sync(be)
    host = pool.cpu().numpy()
    intact = bool((host[:start] == 0xEE).all() and (host[start + total:] == 0xEE).all())
    return offs, host[start:start + total].tobytes(), intact


class PairRun(object):
    """One pair case on the device (the chunks 16-byte aligned, or views ``mis1`` / ``mis2`` bytes into a pool),
    formatted under any launch variant / slice / output offset and compared with the model."""

    def __init__(self, be, m1, m2, dest, which, mis1=0, mis2=0):
        self.be, self.m1, self.m2, self.dest, self.which = be, m1, m2, dest, which
        self.same = m1["data"] is m2["data"]
        assert not self.same or mis1 == mis2
        self.mis = (mis1, mis2)
        data1 = K.upload_text(be, m1["data"], mis1)
        data2 = data1 if self.same else K.upload_text(be, m2["data"], mis2)
        self.sides = []
        for m, data in ((m1, data1), (m2, data2)):
            opt = lambda key: None if m[key] is None else K._i32(be, m[key])
            self.sides.append(dict(data=data, recs=K.records_tensor(be, m["recs"]), begin=K._i32(be, m["begin"]),
                                   end=K._i32(be, m["end"]), ubegin=opt("ubegin"), uend=opt("uend")))
        self.d_dest = K._u8(be, dest)
        self.calls = 0

    def check(self, hint, tile, stage, lo=0, hi=None, out_misalign=0, masks=True, dest=True, report=None):
        hi = len(self.m1["recs"]) if hi is None else hi
        dev = []
        for side in self.sides:
            dev += [side["data"], side["recs"][lo:hi], side["begin"][lo:hi], side["end"][lo:hi],
                    side["ubegin"][lo:hi] if (masks and side["ubegin"] is not None) else None,
                    side["uend"][lo:hi] if (masks and side["uend"] is not None) else None]
        offs, text, intact = emit_pairs_call(self.be, dev, hi - lo, self.d_dest[lo:hi] if dest else None, self.which, hint,
                                             out_misalign)
        want, want_offs = model_pairs(self.m1, self.m2, self.dest, self.which, lo, hi, masks, dest)
        what = (hint, lo, hi, self.mis, out_misalign, masks, dest)
        assert offs == want_offs, what
        assert intact, ("guard bytes overwritten", what)
        assert text == want, what
        self.calls += 1
        sub = lambda m: dict(m, recs=m["recs"][lo:hi], begin=m["begin"][lo:hi], end=m["end"][lo:hi])
        s1, s2 = sub(self.m1), sub(self.m2)
        if self.same:
            s2["data"] = s1["data"]
        rep = pair_tile_report(s1, s2, want_offs, tile, stage, self.mis[0], self.mis[1], out_misalign)
        if report is not None:
            for key, v in rep.items():
                report[key] = report.get(key, 0) + v
        return rep


def pair_variants(be):
    """The launch variants to loop over: the three staged instantiations on the GPU; the twin has one formatter."""
    return PAIR_VARIANTS if be.name == "hip" else PAIR_VARIANTS[:1]


def check_pairs_layouts(be):
    """Every layout under every variant, with and without masks and dest; then both, one and neither chunk
    unaligned (views 1, 7, 15 bytes into a pool) with an aligned and an unaligned output.  Returns {layout: tile
    report} and the number of calls."""
    out, calls = {}, 0
    for layout, (m1, m2, dest, which) in pair_cases().items():
        run = PairRun(be, m1, m2, dest, which)
        rep = out[layout] = {}
        for hint, tile, stage in pair_variants(be):
            run.check(hint, tile, stage, report=rep)
            run.check(hint, tile, stage, masks=False, report=rep)
            run.check(hint, tile, stage, dest=False, report=rep)
        calls += run.calls
    hint, tile, stage = pair_variants(be)[-1]
    shifted = out["shifted"] = {}
    m1, m2, dest, which = pair_cases()["two"]
    for off in (1, 7, 15):
        for mis1, mis2 in ((off, 0), (0, off), (off, 16 - off)):
            run = PairRun(be, m1, m2, dest, which, mis1, mis2)
            run.check(hint, tile, stage, report=shifted)
            run.check(hint, tile, stage, out_misalign=off, report=shifted)
            calls += run.calls
    m1, m2, dest, which = pair_cases()["interleaved"]
    for off in (1, 7, 15):
        run = PairRun(be, m1, m2, dest, which, off, off)
        run.check(hint, tile, stage, report=shifted)
        run.check(hint, tile, stage, out_misalign=16 - off, report=shifted)
        calls += run.calls
    run = PairRun(be, m1, m2, dest, which)
    for off in (1, 7, 15):
        run.check(hint, tile, stage, out_misalign=off, report=shifted)
    return out, calls + run.calls


def check_pairs_tiles(be):
    """Per variant: n in {0, 1, TILE - 1, TILE, TILE + 1, 4 TILE + 3}; the arrays passed from pair k in {1, 2, 3, 5} on; a
    whole tile with ``dest != which``; a random permutation of the pair order; renamed records (flag bit 1).
    Returns {hint: report}."""
    m1, m2, dest, which = pair_cases()["interleaved"]
    n = len(dest)
    perm = np.random.default_rng(43).permutation(n)
    runs = dict(plain=PairRun(be, m1, m2, dest, which), permuted=PairRun(be, _take(m1, perm), _take(m2, perm), dest[perm], which))
    one = K.renamed_case(K.formatter_case(nrec=600, seed=5))
    every = np.arange(600)
    r1, r2 = _take(one, every[0::2]), _take(one, every[1::2])
    r2["data"] = r1["data"]
    runs["renamed"] = PairRun(be, r1, r2, dest, which)
    out = {}
    for hint, tile, stage in pair_variants(be):
        rep = out[hint] = dict(edge_calls=0)
        for count in (0, 1, tile - 1, tile, tile + 1, 4 * tile + 3):
            runs["plain"].check(hint, tile, stage, hi=count, report=rep)
            rep["edge_calls"] += 1
        for k in (1, 2, 3, 5):
            runs["plain"].check(hint, tile, stage, lo=k, report=rep)
            runs["plain"].check(hint, tile, stage, lo=k, hi=k + 4 * tile + 3, dest=False, report=rep)
        hollow = dest.copy()
        hollow[tile:2 * tile] = 3                               # tile 1 writes nothing
        before = rep.get("empty", 0)
        PairRun(be, m1, m2, hollow, which).check(hint, tile, stage, report=rep)
        rep["empty_tile"] = rep["empty"] - before
        rep["permuted_unordered"] = runs["permuted"].check(hint, tile, stage)["unordered"]
        ren = runs["renamed"].check(hint, tile, stage)
        rep["renamed_unordered"], rep["renamed_staged"] = ren["unordered"], ren["one"] + ren["two"]
    return out


def check_pairs_stage_limit(be):
    """Per variant two tiles on either side of the stage size (``stage_limit_case`` with 2 TILE records per tile, read
    as interleaved pairs): tile 0 needs the stage exactly, tile 1 one byte more.  Returns {hint: report}."""
    out = {}
    for hint, tile, stage in pair_variants(be):
        case = K.stage_limit_case(2 * tile, stage)
        every = np.arange(4 * tile)
        m1, m2 = _take(case, every[0::2]), _take(case, every[1::2])
        m2["data"] = m1["data"]
        out[hint] = PairRun(be, m1, m2, np.zeros(2 * tile, dtype=np.int64), 0).check(hint, tile, stage, dest=False)
    return out


# ---------------------------------------------------------------------------------------------- overwrite: plan, apply
OVER_LETTERS = np.frombuffer(b"ACGT" * 8 + b"acgtNnRYSWKMBDHVryswkmbdhv", np.uint8)


def overwrite_case(n, window, base, seed, lowq=10, highq=20, bad=()):
    """n pairs in two chunks (sizes no multiple of 16): reads of up to 300 bases with ``begin > 0`` and ``end < len``;
    kept lengths 0, window - 1, window, window + 1 and up to 300 in both reads, so that the mates' lengths differ in
    both directions; the window sums of the kept qualities on lowq * window and highq * window exactly, one below
    each, and far from both; upper-, lower-case and IUPAC bases; the pairs ``bad`` hold a base without a complement
    in the read that would be cloned."""
    rng = np.random.default_rng(seed)
    sums = (lowq * window - 1, lowq * window, highq * window - 1, highq * window, 2 * window, min(40, highq + 9) * window)
    lens = (0, window - 1, window, window + 1, window + 37, 300)
    texts, metas = [b"", b""], [[], []]
    for p in range(n):
        pick = (0, 5) if p in bad else (int(rng.integers(0, 6)), int(rng.integers(0, 6)))      # (read 1 low, read 2 high)
        for k in (0, 1):
            kept = max(lens[int(rng.integers(0, 6))] if p not in bad else window + 5, 0)
            a, tail = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            total = a + kept + tail
            seq = bytearray(OVER_LETTERS[rng.integers(0, len(OVER_LETTERS), total)].tobytes())
            if p in bad and k == 1:
                seq[a + kept // 2] = ord(".")
            q = rng.integers(2, 41, total)
            if kept >= window > 0:
                vals = np.full(window, sums[pick[k]] // window)
                vals[:sums[pick[k]] % window] += 1
                rng.shuffle(vals)
                q[a:a + window] = vals
            name = b"p%d/%d x" % (p, k + 1)
            plus = b"+" + name if p % 3 == 0 else b"+"
            rec = b"@" + name + b"\n" + bytes(seq) + b"\n" + plus + b"\n" + bytes((q + base).astype(np.uint8)) + b"\n"
            metas[k].append((a, a + kept))
            texts[k] += rec
    return texts, metas


def check_overwrite(be, n, window, base, seed, bad=()):
    """atr_overwrite_plan_batch + atr_overwrite_apply_batch against ``modifiers.OverwriteRead`` on the kept intervals: the
    ``which`` bytes, the growth offsets, every appended byte, the re-pointed descriptors and intervals, and that
    nothing outside the appended tails changed.  Returns (pairs overwritten per read, the error word)."""
    from atropos_amd.modifiers import COMP_TABLE, OverwriteRead
    from atropos_amd.reads import Read
    lowq, highq = 10, 20
    texts, metas = overwrite_case(n, window, base, seed, lowq, highq, bad)
    sides = []
    for k in (0, 1):
        recs, _, err = K.model_index(texts[k])
        assert err == K.INT64_MAX and len(recs) == n
        raw = texts[k] + b"\0" * (17 + k)                        # readable, and no multiple of 16 long
        raw += b"\0" * ((5 - len(raw)) % 16)
        assert len(raw) % 16 == 5
        sides.append(dict(raw=raw, recs=recs, data=K._u8(be, np.frombuffer(raw, np.uint8).copy()), d_recs=K.records_tensor(be, recs),
                          begin=K._i32(be, [m[0] for m in metas[k]]), end=K._i32(be, [m[1] for m in metas[k]])))
    s1, s2 = sides

    class Chunk(object):
        def __init__(self, side):
            self.data, self.records = side["data"], side["d_recs"]
    which, grow1, grow2 = be.overwrite_plan(Chunk(s1), s1["begin"], s1["end"], Chunk(s2), s2["begin"], s2["end"], lowq, highq,
                                            window, base)
    K._sync(be)
    # the model
    want_which, clones, failed = [], [[], []], []
    for p in range(n):
        reads = []
        for k, side in enumerate(sides):
            no, nl, so, sl, qo, ql, fl, _ = side["recs"][p]
            a, b = metas[k][p]
            name = side["raw"][no:no + nl].decode()
            reads.append(Read(name, side["raw"][so + a:so + b].decode(), side["raw"][qo + a:qo + b].decode(), name if fl & 1 else ""))
        try:
            got = OverwriteRead(lowq, highq, window, base=base)(*reads)
        except KeyError:
            failed.append(p)
            got = None
        w = 0
        if got is None:
            w = 1                                               # (the bad pairs are made so that read 1 is overwritten)
        elif got[0] is not reads[0]:
            w = 1
        elif got[1] is not reads[1]:
            w = 2
        want_which.append(w)
        if w:
            src = reads[2 - w]
            text = None
            if got is not None:
                clone = got[w - 1]
                assert clone.name == src.name and len(clone) == len(src)
                text = clone.name.encode() + clone.sequence.encode() + clone.qualities.encode()
            clones[w - 1].append((p, len(src.name) + 2 * len(src), text, src))
    assert which.cpu().tolist() == want_which, (n, window, base)
    grows = (grow1.cpu().tolist(), grow2.cpu().tolist())
    tails, datas, new_recs = [], [], []
    for k, side in enumerate(sides):
        at, want_grow, it = 0, [], iter(clones[k])
        nxt = next(it, None)
        for p in range(n):
            want_grow.append(at)
            if nxt is not None and nxt[0] == p:
                at += (nxt[1] + 15) // 16 * 16
                nxt = next(it, None)
        assert grows[k] == want_grow + [at], (k, n, window)
        base_at = (len(side["raw"]) + 15) // 16 * 16
        tails.append(base_at)
        datas.append(torch.cat([side["data"], torch.full((base_at - len(side["raw"]) + at + 16,), 0xEE, dtype=torch.uint8,
                                                          device=side["data"].device)]))
        new_recs.append(side["d_recs"].clone())
    err = be.overwrite_apply(datas[0], new_recs[0], s1["begin"], s1["end"], datas[1], new_recs[1], s2["begin"], s2["end"], which,
                             grow1, grow2, tails[0], tails[1], COMP_TABLE)
    K._sync(be)
    assert err == (failed[0] * 8 + 1 if failed else K.INT64_MAX), (err, failed)
    for k, side in enumerate(sides):
        host = datas[k].cpu().numpy().tobytes()
        assert host[:len(side["raw"])] == side["raw"]           # nothing in front of the tail changed
        got_recs = K._host_u32(new_recs[k]).reshape(-1, 8).tolist()
        begin, end = sides[k]["begin"].cpu().tolist(), sides[k]["end"].cpu().tolist()
        written = bytearray(b"\xee" * (len(host) - len(side["raw"])))
        cloned = {c[0]: c for c in clones[k]}
        for p in range(n):
            if p not in cloned:
                assert got_recs[p] == side["recs"][p] and (begin[p], end[p]) == metas[k][p]
                continue
            _, size, text, src = cloned[p]
            at = tails[k] + grows[k][p]
            kept = len(src)
            assert got_recs[p] == [at, len(src.name), at + len(src.name), kept, at + len(src.name) + kept, kept,
                                   1 if src.name2 else 0, 0], p
            assert (begin[p], end[p]) == (0, kept)
            if text is not None:
                assert host[at:at + size] == text, p
            written[at - len(side["raw"]):at - len(side["raw"]) + size] = host[at:at + size]
        assert host[len(side["raw"]):] == bytes(written)        # ... and nothing in the tail but the clones
    return [len(clones[0]), len(clones[1])], err


def check_overwrite_matrix(be):
    """n in {1, 63, 64, 65, 257} x windows 1, 10, 150 x bases 33 and 64; then a base without a complement in pairs 70 and
    200: the error word is pair 70's.  Returns the pairs overwritten per read, summed."""
    total = [0, 0]
    for i, n in enumerate((1, 63, 64, 65, 257)):
        for window in (1, 10, 150):
            over, err = check_overwrite(be, n, window, 64 if (i + window) % 2 else 33, 100 * n + window)
            assert err == K.INT64_MAX
            total = [total[0] + over[0], total[1] + over[1]]
    over, err = check_overwrite(be, 257, 10, 33, 9, bad=(70, 200))
    assert err == 70 * 8 + 1
    try:
        check_overwrite(be, 5, 0, 33, 1)
    except ValueError:
        pass
    else:
        raise AssertionError("window 0 was not refused")
    return total


# ---------------------------------------------------------------------------------------------- the reference's files
def fixture_files(doc):
    return {k: base64.b64decode(v) for k, v in doc["inputs"].items()}


def write_inputs(doc, tmp):
    """The fixture's inputs as files under ``tmp``: {key: path}."""
    paths = {}
    for key, blob in fixture_files(doc).items():
        paths[key] = os.path.join(str(tmp), "in.%s.fastq" % key)
        with open(paths[key], "wb") as fh:
            fh.write(blob)
    return paths


def case_paths(case, paths, tmp, tag):
    """(the pipeline's argv, in1, in2, out1, out2) of a fixture case: the interleaved paths go through -l / -L."""
    sfx = "_64" if case["base"] == 64 else ""
    argv = case["args"].split()
    if case["input"] == "pair":
        in1, in2 = paths["r1" + sfx], paths["r2" + sfx]
    else:
        in1, in2 = paths["odd" if case["input"] == "odd" else ("il64" if sfx else "il")], None
        argv += ["-l", in1]
    stem = os.path.join(str(tmp), "got.%s" % tag)
    if case["output"] == "pair":
        out1, out2 = stem + ".1.fastq", stem + ".2.fastq"
    else:
        out1, out2 = stem + ".il.fastq", None
        argv += ["-L", out1]
    return argv, in1, in2, out1, out2


def run_case_files(case, paths, tmp, tag, chunk_bytes):
    """The case through ``pipeline_from_args`` + ``trim_files``: {reference file name: bytes written}."""
    from atropos_amd.trim import pipeline_from_args
    argv, in1, in2, out1, out2 = case_paths(case, paths, tmp, tag)
    pipe = pipeline_from_args(argv, paired_input=case["input"] == "pair")
    assert pipe.interleaved_input == (in1 if in2 is None else None)
    assert pipe.interleaved_output == (out1 if out2 is None else None)
    pipe.trim_files(in1, in2, out1, out2, chunk_bytes=chunk_bytes)
    names = ("out.il.fastq",) if out2 is None else ("out.1.fastq", "out.2.fastq")
    return {name: open(path, "rb").read() for name, path in zip(names, (out1, out2))}


def run_case_bytes(case, doc):
    """The case on one batch through ``run`` and ``text`` / ``text_interleaved``: {reference file name: bytes}."""
    from atropos_amd.fastq import FastqBatch
    from atropos_amd.trim import pipeline_from_args
    blobs = fixture_files(doc)
    sfx = "_64" if case["base"] == 64 else ""
    argv = case["args"].split()
    if case["input"] == "pair":
        b1 = FastqBatch.from_bytes(blobs["r1" + sfx])[0]
        b2 = FastqBatch.from_bytes(blobs["r2" + sfx])[0]
    else:
        argv += ["-l", "in.fastq"]
        b1, b2 = FastqBatch.from_bytes(blobs["il64" if sfx else "il"])[0].mates()
    res = pipeline_from_args(argv, paired_input=case["input"] == "pair").run(b1, b2)
    if case["output"] == "il":
        return {"out.il.fastq": res.text_interleaved()}
    t1, t2 = res.text()
    return {"out.1.fastq": t1, "out.2.fastq": t2}


AD1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"                       # the adapters the fixture's reads were made with
AD2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"


def check_detect_interleaved(doc, tmp):
    """``detect_files`` of the interleaved file against the two files, ``max_reads`` ending inside the first and inside
    a later chunk (the cut goes through ``FastqBatch.head`` of both mates).  Returns the comparisons made."""
    from atropos_amd import detect
    paths = write_inputs(doc, tmp)
    size = odd_first_chunk(fixture_files(doc)["il"])
    known = detect.KnownContaminants()
    known.add("ad1", AD1)
    known.add("ad2", AD2)
    done = 0
    for max_reads in (50, 137):
        one = detect.detect_files(paths["il"], None, known, max_reads=max_reads, chunk_bytes=size)
        two = detect.detect_files(paths["r1"], paths["r2"], known, max_reads=max_reads, chunk_bytes=size)
        assert one == two and one["matches"][0] and one["matches"][1]
        done += 1
    return done


def check_stats_interleaved(doc, tmp):
    """``qc_files`` and ``error_rate_file`` of the interleaved file against the two files, cut into chunks (an odd
    first chunk) and as one chunk.  Returns what the interleaved runs gave, for a comparison across backends."""
    from atropos_amd.stats import error_rate_file, qc_files
    paths = write_inputs(doc, tmp)
    out = []
    for size in (odd_first_chunk(fixture_files(doc)["il"]), 1 << 22):
        qc = qc_files(paths["il"], chunk_bytes=size)
        assert qc == qc_files(paths["r1"], paths["r2"], chunk_bytes=size)
        assert qc["pre"][0]["read1"]["counts"] == 220 and qc["pre"][0]["read2"]["counts"] == 220, "220 pairs, a summary per read"
        err = error_rate_file(paths["il"], interleaved=True, chunk_bytes=size)
        assert err == error_rate_file(paths["r1"], paths["r2"], chunk_bytes=size)
        assert len(err[0]) == 2 and len(err[1]) == 2            # one estimate and one total per read
        assert err != error_rate_file(paths["il"], chunk_bytes=size)       # ... not the one of a single-end file
        out.append((qc, err))
    assert out[0] == out[1]
    with pytest_raises(ValueError):
        error_rate_file(paths["r1"], paths["r2"], interleaved=True)
    return out[0]


def pytest_raises(exc):
    import pytest
    return pytest.raises(exc)


def want_files(case):
    return {k: base64.b64decode(v) for k, v in case["files"].items()}


def odd_first_chunk(text, lo=30000, hi=60000, step=97):
    """A chunk size at which the first chunk of ``text`` indexes to an odd number of records (its last record is
    carried over) and the file is cut into at least three chunks."""
    for size in range(lo, hi, step):
        head = text[:size]
        if head.count(b"\n") // 4 % 2 == 1 and len(text) >= 3 * size:
            return size
    raise AssertionError("no chunk size with an odd first chunk")

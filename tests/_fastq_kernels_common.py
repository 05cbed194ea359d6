"""Shared by test_fastq_kernels_host.py (the CPU twin, tests/emu/emu_fastq.cpp) and test_gpu_fastq_kernels.py (the
kernels of atropos_amd/csrc/fastq_kernels.hip and fastq_emit_kernels.hip): a plain Python model of the FASTQ text kernels -- line index, record
descriptors, formatter, interval modifiers, filters, the pack from records -- the case builders that put the inputs
on the kernels' edges, and the ``check_*`` functions that call the kernels at the C ABI with those inputs.

The model works on ``bytes`` and lists and shares no code with ``*_core.hpp``; numpy only builds tensors.  Every
comparison is exact (bytes or integers).  A ``check_*`` takes a backend and returns the counts its test asserts on."""
import ctypes as C

import numpy as np
import torch

from atropos_amd import _lib

INT64_MAX = (1 << 63) - 1
ERR_AT, ERR_PLUS, ERR_NAME2, ERR_LENGTH = 1, 2, 3, 4            # ATR_FASTQ_ERR_* (include/atropos_hip.h)
LF, CRLF, CR = b"\n", b"\r\n", b"\r"
GUARD = 64                                                      # bytes of 0xEE in front of and behind every formatter output
# atr_fastq_emit's staged instantiations: record_bytes_hint -> (records per tile, bytes per stage).  The stage sizes
# are EMIT_STAGE = 13 * 1024 of fastq_device.hpp: <32> whole, <8> EMIT_STAGE / 4, <16> EMIT_STAGE / 2, <16> whole.
EMIT_VARIANTS = ((0, 32, 13312), (300, 8, 3328), (390, 16, 6656), (500, 16, 13312))
NAME_LETTERS = np.frombuffer(b"abcXYZ019:/_-.# @+", np.uint8)
SEQ_LETTERS = np.frombuffer(b"ACGT" * 6 + b"Nacgtn", np.uint8)


# ---------------------------------------------------------------------------------------------- tensors
def _sync(be):
    if be.name == "hip":
        torch.cuda.synchronize(be.device)


def _dev(be, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(be.device)


def _i32(be, values):
    return _dev(be, np.asarray(values, dtype=np.int64).astype(np.int32))


def _u8(be, values):
    return _dev(be, np.asarray(values, dtype=np.uint8))


def padded(text):
    """The chunk as FastqBatch.from_bytes hands it over: zero-padded to a multiple of 16, plus 16."""
    text = bytes(text)
    return text + b"\0" * ((len(text) + 15) // 16 * 16 + 16 - len(text))


def upload_text(be, text, misalign=0):
    """The padded chunk in device memory, 16-byte aligned -- or, with ``misalign``, a view that many bytes into an
    aligned pool (descriptors index the view, so they stay as they are)."""
    raw = np.frombuffer(padded(text), np.uint8)
    pool = torch.zeros((len(raw) + 16,), dtype=torch.uint8, device=be.device)
    assert pool.data_ptr() % 16 == 0
    view = pool[misalign:misalign + len(raw)]
    view.copy_(torch.from_numpy(raw.copy()))
    assert view.data_ptr() % 16 == misalign
    return view


def records_tensor(be, recs):
    arr = np.asarray(recs, dtype=np.int64).reshape(len(recs), 8)
    return _dev(be, arr.astype(np.uint32).view(np.int32))


def _host_u32(tensor):
    return tensor.cpu().numpy().view(np.uint32).astype(np.int64)


# ---------------------------------------------------------------------------------------------- model: index
def model_lines(text):
    """[(start, content length, position of the terminator's last byte)] of every terminated line: universal
    newlines, i.e. what ``bytes.splitlines`` splits on ("\\n", "\\r\\n", a lone "\\r")."""
    out, pos = [], 0
    for piece in bytes(text).splitlines(True):
        if piece.endswith(CRLF):
            term = 2
        elif piece.endswith(LF) or piece.endswith(CR):
            term = 1
        else:
            break                                               # the text's last line has no line end: not a line yet
        out.append((pos, len(piece) - term, pos + len(piece) - 1))
        pos += len(piece)
    return out


def model_index(text):
    """(record descriptors as lists of 8 ints, line_ends, error word) as atr_fastq_index leaves them: the error
    word is ``record * 8 + code`` of the first record that fails (the first failing check of that record)."""
    text = bytes(text)
    lines = model_lines(text)
    recs, err = [], INT64_MAX
    for r in range(len(lines) // 4):
        (s0, c0, _), (s1, c1, _), (s2, c2, _), (s3, c3, _) = lines[4 * r:4 * r + 4]
        head, plus = text[s0:s0 + c0], text[s2:s2 + c2]
        name = head[1:]
        failed, flags = [], 0
        if not head.startswith(b"@"):
            failed.append(ERR_AT)
        if not plus.startswith(b"+"):
            failed.append(ERR_PLUS)
        elif len(plus) > 1:
            if plus[1:] == name:
                flags = 1
            else:
                failed.append(ERR_NAME2)
        if c3 != c1:
            failed.append(ERR_LENGTH)
        recs.append([s0 + 1, len(name), s1, c1, s3, c3, flags, 0])
        if failed:
            err = min(err, r * 8 + failed[0])
    return recs, [end for _, _, end in lines], err


def model_records(text):
    """[(name, seq, has_name2, qual)] with the line ends stripped, and the error word."""
    text = bytes(text)
    recs, _, err = model_index(text)
    return [(text[no:no + nl], text[so:so + sl], bool(fl & 1), text[qo:qo + ql]) for no, nl, so, sl, qo, ql, fl, _ in recs], err


# ---------------------------------------------------------------------------------------------- model: format
def model_format(data, recs, begin, end, ubegin, uend, dest, which):
    """(text, offsets[n + 1]) of atr_fastq_emit: ``@name\\nSEQ\\n+[name2]\\nQUAL\\n`` over [begin, max(begin, end)) of
    the records with ``dest[r] == which`` in record-array order; bases outside [ubegin, uend) read ``N``; name2 is
    the name, or -- flag bit 1 -- the ``flags >> 8`` bytes at ``reserved``."""
    data = bytes(data)
    out, offsets, total = [], [0], 0
    for r, (no, nl, so, sl, qo, ql, fl, rs) in enumerate(recs):
        if dest is None or dest[r] == which:
            a = int(begin[r])
            b = max(a, int(end[r]))
            seq = bytearray(data[so + a:so + b])
            if ubegin is not None:
                for k in range(b - a):
                    if not int(ubegin[r]) <= a + k < int(uend[r]):
                        seq[k] = ord("N")
            name2 = b""
            if fl & 1:
                name2 = data[rs:rs + (fl >> 8)] if fl & 2 else data[no:no + nl]
            piece = b"@" + data[no:no + nl] + b"\n" + bytes(seq) + b"\n+" + name2 + b"\n" + data[qo + a:qo + b] + b"\n"
            out.append(piece)
            total += len(piece)
        offsets.append(total)
    return b"".join(out), offsets


def tile_report(recs, offsets, tile, stage):
    """Which way emit_staged_kernel<tile, stage> takes every tile of a call, from the descriptors and the model's
    offsets: 'staged' (through LDS), 'overflow' (in file order but beyond the stage), 'unordered', 'empty'; the
    span misalignments of the staged tiles and ``need_in`` = (in_hi - in_lo) + mis_in + 16 of the ordered ones."""
    rep = dict(staged=0, overflow=0, unordered=0, empty=0, mis_in=set(), mis_out=set(), need_in=[])
    n = len(recs)
    for t0 in range(0, n, tile):
        sub = recs[t0:t0 + tile]
        in_lo, in_hi = sub[0][0] - 1, sub[-1][4] + sub[-1][5]
        out_lo, out_hi = offsets[t0], offsets[t0 + len(sub)]
        if out_hi == out_lo:
            rep["empty"] += 1
            continue
        ordered = all(no - 1 >= in_lo and qo + ql <= in_hi and so >= no - 1 and so + sl <= qo and no + nl <= so and not fl & 2
                      for no, nl, so, sl, qo, ql, fl, _ in sub)
        if not ordered:
            rep["unordered"] += 1
            continue
        need_in = (in_hi - in_lo) + (in_lo & 15) + 16
        need_out = (out_hi - out_lo) + (out_lo & 15) + 16
        rep["need_in"].append(need_in)
        if need_in <= stage and need_out <= stage:
            rep["staged"] += 1
            rep["mis_in"].add(in_lo & 15)
            rep["mis_out"].add(out_lo & 15)
        else:
            rep["overflow"] += 1
    return rep


# ---------------------------------------------------------------------------------------------- formatter: cases
def _letters(rng, alphabet, n):
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


def formatter_case(nrec=600, seed=5):
    """~600 records: names of 0..40 bytes, reads of 0..160 bases, every ninth read one of 0, 1, 3, 17, 150, 151, 400,
    2 900 bases (and three of 2 900 in a row), ~30 % ``+name`` lines, LF and CRLF records mixed; random begin / end (``end < begin`` and empty
    intervals included), random mask intervals (``ubegin >= uend`` included), dest in {0, 1, 2}."""
    rng = np.random.default_rng(seed)
    special = (0, 1, 3, 17, 150, 151, 400, 2900)
    parts, lens = [], []
    for i in range(nrec):
        name = _letters(rng, NAME_LETTERS, int(rng.integers(0, 41)))
        n = special[(i // 9) % 8] if i % 9 == 4 else int(rng.integers(0, 161))
        if 100 <= i < 103:
            n = 2900                                            # three in a row: beyond the largest stage, whatever the tile
        seq = _letters(rng, SEQ_LETTERS, n)
        qual = bytes(rng.integers(33, 75, n).astype(np.uint8))
        eol = CRLF if rng.random() < 0.3 else LF
        plus = b"+" + name if rng.random() < 0.3 else b"+"
        parts.append(eol.join([b"@" + name, seq, plus, qual, b""]))
        lens.append(n)
    text = b"".join(parts)
    recs, _, err = model_index(text)
    assert err == INT64_MAX and len(recs) == nrec and [r[3] for r in recs] == lens
    lens = np.asarray(lens)
    whole = rng.random(nrec) < 0.4                              # untouched reads: the formatter's plain copies
    begin = np.where(whole, 0, rng.integers(0, lens + 1))
    end = np.where(whole, lens, rng.integers(0, lens + 1))
    unmasked = rng.random(nrec) < 0.6
    ubegin = np.where(unmasked, 0, rng.integers(0, lens + 1))
    uend = np.where(unmasked, lens, rng.integers(0, lens + 1))
    dest = rng.integers(0, 3, nrec)
    assert (end < begin).any() and (end == begin).any() and (ubegin >= uend).any()
    assert any(r[6] & 1 for r in recs) and CRLF in text
    return dict(data=padded(text), recs=recs, begin=begin, end=end, ubegin=ubegin, uend=uend, dest=dest, which=1)


def renamed_case(case, seed=9):
    """The case with a tenth of its names rewritten as TrimPipeline._rewrite_names does it: the new names sit behind
    the (16-byte padded) chunk, the records point at them, and a record whose ``+`` line repeats the name keeps
    the old one: ``flags = 1 | 2 | old_len << 8``, ``reserved`` = the old ``name_off``."""
    rng = np.random.default_rng(seed)
    data = case["data"]
    base = (len(data) + 15) // 16 * 16
    extra, recs = b"", []
    for rec in case["recs"]:
        rec = list(rec)
        if rng.random() < 0.1:
            new = b"new:" + _letters(rng, NAME_LETTERS, int(rng.integers(0, 30)))
            if rec[6] & 1:
                rec[7] = rec[0]
                rec[6] = 1 | 2 | (rec[1] << 8)
            rec[0], rec[1] = base + len(extra), len(new)
            extra += new
        recs.append(rec)
    assert any(r[6] & 2 for r in recs) and any(r[0] >= base and not r[6] & 2 for r in recs)
    out = dict(case)
    out.update(data=padded(data + b"\0" * (base - len(data)) + extra), recs=recs)
    return out


def stage_limit_case(tile, stage):
    """Two tiles of ``tile`` LF records, every tile stage - 15 bytes of text: tile 0 starts at byte 0 (mis_in 0) and
    needs (in_hi - in_lo) + mis_in + 16 = stage exactly; tile 1 starts at stage - 15 (mis_in 1) and needs one byte
    more.  One read per tile is as long as that takes; its kept interval is 40 bases short, so that the output
    side is not what decides."""
    parts, lens = [], []
    for t in range(2):
        small = [(b"s%03d" % i, 10 + i % 3) for i in range(tile - 1)]
        rest = (stage - 15) - sum(len(nm) + 2 * n + 6 for nm, n in small)
        name = b"long" if (rest - 6 - 4) % 2 == 0 else b"long."
        big = (rest - 6 - len(name)) // 2
        for nm, n in [(name, big)] + small:
            parts.append(b"@" + nm + b"\n" + b"ACGT" * (n // 4) + b"A" * (n % 4) + b"\n+\n" + b"I" * n + b"\n")
            lens.append(n)
    text = b"".join(parts)
    assert len(text) == 2 * (stage - 15)
    recs, _, err = model_index(text)
    assert err == INT64_MAX and len(recs) == 2 * tile
    lens = np.asarray(lens)
    end = lens.copy()
    end[0] -= 40
    end[tile] -= 40
    return dict(data=padded(text), recs=recs, begin=np.zeros_like(lens), end=end, ubegin=None, uend=None, dest=None, which=0)


# ---------------------------------------------------------------------------------------------- formatter: calls
def emit_variants(be):
    """The launch variants to loop over: the four staged instantiations on the GPU; the twin has one formatter."""
    return EMIT_VARIANTS if be.name == "hip" else EMIT_VARIANTS[:1]


def emit_call(be, data, recs, begin, end, ubegin, uend, dest, which, hint, out_misalign=0):
    """atr_fastq_emit (or the twin's) called directly: sizing call, then the write into a view of a 0xEE pool
    with GUARD bytes in front of it and behind ``total``.  Returns (offsets list, text bytes, guards untouched)."""
    n = recs.shape[0]
    ptr = _lib._ptr
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=be.device)
    work = be.empty((max(be._host("atr_fastq_emit_work_bytes", n), 16),), torch.uint8)

    def call(out_ptr):
        be._call("atr_fastq_emit", ptr(data), ptr(recs), ptr(begin), ptr(end), ptr(ubegin), ptr(uend), ptr(dest), which, n, hint,
                 ptr(offsets), ptr(work), out_ptr)
    call(None)
    _sync(be)
    offs = offsets.cpu().tolist()
    total = offs[n]
    pool = torch.full((GUARD + 16 + total + GUARD,), 0xEE, dtype=torch.uint8, device=be.device)
    assert pool.data_ptr() % 16 == 0 and 0 <= out_misalign < 16
    start = GUARD + out_misalign
    call(C.c_void_p(pool.data_ptr() + start))
    _sync(be)
    host = pool.cpu().numpy()
    intact = bool((host[:start] == 0xEE).all() and (host[start + total:] == 0xEE).all())
    return offs, host[start:start + total].tobytes(), intact


class EmitRun(object):
    """One case on the device, formatted under any launch variant / slice / pointer offset and compared with the
    model; collects what the formatter tests assert on."""

    def __init__(self, be, case, in_misalign=0):
        self.be, self.case = be, case
        self.data = upload_text(be, case["data"], in_misalign)
        self.recs = records_tensor(be, case["recs"])
        opt = lambda key, make: None if case[key] is None else make(be, case[key])
        self.begin, self.end = _i32(be, case["begin"]), _i32(be, case["end"])
        self.ubegin, self.uend = opt("ubegin", _i32), opt("uend", _i32)
        self.dest = opt("dest", _u8)
        self.calls = 0

    def check(self, hint, tile, stage, lo=0, hi=None, out_misalign=0, masks=True, dest=True, report=None):
        """Records [lo, hi) of the case (all arrays passed from record ``lo`` on); returns the tile report."""
        c = self.case
        hi = len(c["recs"]) if hi is None else hi
        cut = lambda t, on=True: None if (t is None or not on) else t[lo:hi]
        sub = lambda a, on=True: None if (a is None or not on) else a[lo:hi]
        offs, text, intact = emit_call(self.be, self.data, self.recs[lo:hi], cut(self.begin), cut(self.end),
                                       cut(self.ubegin, masks), cut(self.uend, masks), cut(self.dest, dest), c["which"], hint,
                                       out_misalign)
        want, want_offs = model_format(c["data"], c["recs"][lo:hi], c["begin"][lo:hi], c["end"][lo:hi], sub(c["ubegin"], masks),
                                       sub(c["uend"], masks), sub(c["dest"], dest), c["which"])
        what = (hint, lo, hi, out_misalign, masks, dest)
        assert offs == want_offs, what
        assert intact, ("guard bytes overwritten", what)
        assert text == want, what                               # the whole output
        self.calls += 1                                         # (every call is a guarded one)
        rep = tile_report(c["recs"][lo:hi], want_offs, tile, stage)
        if report is not None:
            for key in ("staged", "overflow", "unordered", "empty"):
                report[key] = report.get(key, 0) + rep[key]
            for key in ("mis_in", "mis_out"):
                report.setdefault(key, set()).update(rep[key])
            report.setdefault("need_in", []).extend(rep["need_in"])
        return rep


_FORMATTER_CASE = []


def shared_formatter_case():
    if not _FORMATTER_CASE:
        _FORMATTER_CASE.append(formatter_case())
    return _FORMATTER_CASE[0]


def check_emit_variants(be):
    """The generated text under every staged instantiation (hints 0, 300, 390, 500), with and without masks and
    dest, and through the byte-per-lane kernel: unaligned input (a view 1, 7, 15 bytes into a pool), unaligned
    output, both.  Returns {hint: tile report} and the byte-per-lane calls per kind."""
    case = shared_formatter_case()
    run = EmitRun(be, case)
    staged = {}
    for hint, tile, stage in emit_variants(be):
        rep = staged[hint] = {}
        run.check(hint, tile, stage, report=rep)
        run.check(hint, tile, stage, masks=False, report=rep)
        run.check(hint, tile, stage, dest=False, report=rep)
    lanes = dict(input=0, output=0, both=0)
    for off in (1, 7, 15):
        shifted = EmitRun(be, case, in_misalign=off)
        shifted.check(300, 8, 3328)
        run.check(300, 8, 3328, out_misalign=off)
        shifted.check(300, 8, 3328, out_misalign=16 - off)
        lanes["input"] += 1
        lanes["output"] += 1
        lanes["both"] += 1
        run.calls += shifted.calls
    return dict(staged=staged, lanes=lanes, calls=run.calls)


def check_emit_tiles(be):
    """For every staged variant: n in {1, TILE - 1, TILE, TILE + 1, 4 TILE + 3}; the record / begin / end / mask / dest
    arrays passed from record k in {1, 2, 3, 5} on (tile 0 starts at an arbitrary in_lo); a whole tile with
    ``dest != which``; a random permutation of the record array; renamed records.  Returns {hint: report}."""
    case = shared_formatter_case()
    n = len(case["recs"])
    rng = np.random.default_rng(21)
    perm = rng.permutation(n)
    permuted = dict(case)
    permuted["recs"] = [case["recs"][i] for i in perm]
    for key in ("begin", "end", "ubegin", "uend", "dest"):
        permuted[key] = case[key][perm]
    renamed = renamed_case(case)
    runs = dict(plain=EmitRun(be, case), permuted=EmitRun(be, permuted), renamed=EmitRun(be, renamed))
    out = {}
    for hint, tile, stage in emit_variants(be):
        rep = out[hint] = dict(edge_calls=0, offset_calls=0)
        for count in (1, tile - 1, tile, tile + 1, 4 * tile + 3):
            runs["plain"].check(hint, tile, stage, hi=count, report=rep)
            rep["edge_calls"] += 1
        for k in (1, 2, 3, 5):
            runs["plain"].check(hint, tile, stage, lo=k, report=rep)
            runs["plain"].check(hint, tile, stage, lo=k, hi=k + 4 * tile + 3, dest=False, report=rep)
            rep["offset_calls"] += 2
        hollow = dict(case)
        hollow["dest"] = case["dest"].copy()
        hollow["dest"][tile:2 * tile] = 3                      # tile 1 writes nothing: out_hi == out_lo
        before = rep.get("empty", 0)
        EmitRun(be, hollow).check(hint, tile, stage, report=rep)
        rep["empty_tile"] = rep["empty"] - before
        rep["permuted_unordered"] = runs["permuted"].check(hint, tile, stage)["unordered"]
        ren = runs["renamed"].check(hint, tile, stage)
        rep["renamed_unordered"], rep["renamed_staged"] = ren["unordered"], ren["staged"]
    return out


def check_emit_stage_limit(be):
    """Per staged variant two tiles on either side of the stage size; returns {hint: (tiles that fit, tiles
    that overflow, need_in values)}."""
    out = {}
    for hint, tile, stage in emit_variants(be):
        rep = EmitRun(be, stage_limit_case(tile, stage)).check(hint, tile, stage)
        out[hint] = (rep["staged"], rep["overflow"], rep["need_in"])
    return out


# ---------------------------------------------------------------------------------------------- index: cases
# n records through the shared "sizes -> offsets -> total" step (device_scan of scan_kernels.hpp): one block, the block
# edge, two and three blocks, and 1026 blocks -- there every thread of scan_sums_kernel owns a run of two block totals,
# threads 0 .. 512 are busy and the rest are empty.
OFFSET_COUNTS = (0, 1, 1023, 1024, 1025, 2048, 2049, 1048576 + 1025)


def offsets_case(n, seed=41):
    """(text, record texts, dest) of n records with hexadecimal names and 1 to 3 bases: record sizes that are no
    multiple of anything, and a dest mask that keeps about half of the records."""
    rng = np.random.default_rng(seed + n)
    lens = rng.integers(1, 4, size=n).tolist()
    bases = SEQ_LETTERS[rng.integers(0, len(SEQ_LETTERS), size=n + 3)].tobytes()
    quals = rng.integers(33, 74, size=n + 3).astype(np.uint8).tobytes()
    pieces = [b"@%x\n%s\n+\n%s\n" % (r, bases[r:r + k], quals[r:r + k]) for r, k in enumerate(lens)]
    return b"".join(pieces), pieces, rng.integers(0, 2, size=n).astype(np.uint8)


def check_emit_offsets(be):
    """atr_fastq_emit over OFFSET_COUNTS records, indexed on the device, half of them kept by ``dest``: the text byte
    for byte against a ``bytes.join`` over the kept records, every offset and the total against the running sum of
    their lengths.  Returns {n: total}."""
    out = {}
    for n in OFFSET_COUNTS:
        text, pieces, dest = offsets_case(n)
        data = upload_text(be, text)
        recs, _, nlines, err = be.fastq_index(data, len(text))
        _sync(be)
        assert nlines == 4 * n and recs.shape[0] == n and err == INT64_MAX, n
        want = b"".join(p for p, keep in zip(pieces, dest.tolist()) if keep)
        sizes = np.asarray([len(p) for p in pieces], dtype=np.int64) * dest
        want_offs = np.concatenate((np.zeros(1, np.int64), np.cumsum(sizes)))
        begin = torch.zeros((n,), dtype=torch.int32, device=be.device)
        end = recs[:, 3].to(torch.int32).contiguous()                           # the whole sequence: seq_len
        offs, got, intact = emit_call(be, data, recs, begin, end, None, None, _u8(be, dest), 1, 0)
        assert offs[n] == len(want), (n, offs[n], len(want))                   # the total
        assert np.array_equal(np.asarray(offs, dtype=np.int64), want_offs), n
        assert intact, ("guard bytes overwritten", n)
        assert got == want, n
        out[n] = offs[n]
    return out


def _render(lines):
    """[(content, eol)] -> text.  A lone "\\r" followed by an empty line that ends in "\\n" would read as one
    "\\r\\n": such a line gets "\\r\\n" of its own."""
    out, last = [], None
    for content, eol in lines:
        if last == CR and not content and eol == LF:
            eol = CRLF
        out.append(content + eol)
        last = eol
    return b"".join(out)


INDEX_PLACEMENTS = (
    # (offset of the terminator's first byte, kind) -- 'crlf': "\r\n" there; 'cr': a lone "\r"; 'cr_crlf': a lone
    # "\r" directly followed by "\r\n".  Offsets = 15 (mod 16) put the "\n" (or what follows) in the next 16-byte
    # block, offsets 4096 k - 1 in the next thread block; 14 (mod 16) puts the second "\r" of "\r\r\n" on byte 15.
    (1007, "crlf"), (2047, "cr"), (4095, "A"), (8191, "A"), (12287, "B"), (16383, "B"), (20479, "cr_crlf"),
    (24590, "cr_crlf"), (28671, "crlf"), (32766, "cr_crlf"), (36863, "cr"))


def index_placements(swap):
    """'A' offsets hold "\\r\\n" and 'B' offsets a lone "\\r" -- or, with ``swap``, the other way round: both texts
    together put each of the two on 4095 | 4096, 8191 | 8192, 12287 | 12288 and 16383 | 16384."""
    pick = {"A": "cr" if swap else "crlf", "B": "crlf" if swap else "cr"}
    return [(off, pick.get(kind, kind)) for off, kind in INDEX_PLACEMENTS]


def placement_present(text, off, kind):
    if kind == "crlf":
        return text[off:off + 2] == CRLF
    if kind == "cr":
        return text[off:off + 1] == CR and text[off + 1:off + 2] not in (LF, CR)
    return text[off:off + 3] == CR + CRLF


def index_records(swap=False, tail_mod=0, seed=3, size=40000):
    """[[(content, eol) x 4] per record] of a ~40 KB text with LF, CRLF and lone-CR line ends, the placements of
    ``index_placements(swap)`` and a length = tail_mod (mod 16)."""
    rng = np.random.default_rng(seed)
    records, cur = [], [0]

    def add(name, n, eols, repeat):
        seq = _letters(rng, SEQ_LETTERS, n)
        qual = bytes(rng.integers(33, 75, n).astype(np.uint8))
        rec = list(zip([b"@" + name, seq, b"+" + (name if repeat else b""), qual], eols))
        records.append(rec)
        cur[0] += len(_render(rec))

    def filler(limit):
        while cur[0] + 700 < limit:
            style = rng.integers(0, 4)
            eols = [(LF, CRLF, CR)[int(k)] for k in rng.integers(0, 3, 4)] if style == 3 else [(LF, CRLF, CR)[int(style)]] * 4
            add(_letters(rng, NAME_LETTERS, int(rng.integers(0, 41))), int(rng.integers(0, 121)), eols, rng.random() < 0.3)

    for off, kind in index_placements(swap):
        filler(off)
        gap = off - cur[0] - 1                                  # '@' + gap bytes of name, then the terminator at `off`
        assert 0 <= gap <= 700
        name = _letters(rng, NAME_LETTERS, gap)
        if kind == "cr_crlf":
            add(name, 0, [CR, CRLF, CR, CRLF], False)           # an empty read: "\r" + "\r\n", twice
        else:
            add(name, int(rng.integers(1, 60)), [CRLF if kind == "crlf" else CR, LF, CRLF, LF], rng.random() < 0.5)
    filler(size)
    n = 33
    fixed = len(b"@") + 1 + n + 1 + 2 + n + 1
    add(_letters(rng, NAME_LETTERS, (tail_mod - cur[0] - fixed) % 16), n, [LF] * 4, False)
    return records


def index_text(records):
    return _render([line for rec in records for line in rec])


def malform(records, r, code):
    """A copy of the records with record r broken so that it fails with ``code`` (and with nothing before it)."""
    out = [list(rec) for rec in records]
    (head, e0), (seq, e1), (plus, e2), (qual, e3) = out[r]
    if code == ERR_AT:
        head = b"X" + head[1:]
    elif code == ERR_PLUS:
        plus = b"-" + plus[1:]
    elif code == ERR_NAME2:
        plus = b"+" + head[1:] + b"x"
    else:
        qual = qual + b"I"
    out[r] = [(head, e0), (seq, e1), (plus, e2), (qual, e3)]
    return out


def check_index_text(be, text):
    """atr_fastq_count_lines + atr_fastq_index over ``text`` against the model: number of lines, line_ends, every
    descriptor word, the error word.  Returns (lines, records, error word)."""
    recs, ends, err = model_index(text)
    data = upload_text(be, text)
    got_recs, got_ends, nlines, got_err = be.fastq_index(data, len(text))
    _sync(be)
    assert nlines == len(ends)
    assert _host_u32(got_ends)[:nlines].tolist() == ends
    assert got_recs.shape[0] == len(recs)
    assert _host_u32(got_recs).reshape(-1, 8).tolist() == recs
    assert got_err == err, (got_err, err)
    return nlines, len(recs), err


def check_index(be):
    """The placement texts (both assignments of "\\r\\n" / lone "\\r" to the block boundaries) at lengths = 0, 1, 15
    (mod 16); then two malformed records in different 4096-byte blocks, once per error code: the smaller record
    index wins.  Returns counts."""
    out = dict(texts=0, lines=0, records=0, errors=[])
    for swap in (False, True):
        for tail_mod in (0, 1, 15):
            records = index_records(swap, tail_mod)
            text = index_text(records)
            assert len(text) % 16 == tail_mod and len(text) > 9 * 4096
            for off, kind in index_placements(swap):
                assert placement_present(text, off, kind), (off, kind)
            for eol in (LF, CRLF, CR):
                assert sum(e == eol for rec in records for _, e in rec) > 50
            nlines, nrec, err = check_index_text(be, text)
            assert err == INT64_MAX and nrec == len(records) and nlines == 4 * nrec
            out["texts"] += 1
            out["lines"] += nlines
            out["records"] += nrec
    records = index_records(False, 0)
    starts = np.cumsum([0] + [len(_render(rec)) for rec in records])
    first = int(np.searchsorted(starts, 2 * 4096 + 100))
    second = int(np.searchsorted(starts, 6 * 4096 + 100))
    assert starts[first] // 4096 == 2 and starts[second] // 4096 == 6
    for code in (ERR_AT, ERR_PLUS, ERR_NAME2, ERR_LENGTH):
        other = code % 4 + 1
        text = index_text(malform(malform(records, first, code), second, other))
        _, _, err = check_index_text(be, text)
        assert err == first * 8 + code                          # (the model agrees with how the text was broken)
        text = index_text(malform(records, second, code))      # ... and the later record alone
        _, _, err = check_index_text(be, text)
        assert err == second * 8 + code
        out["errors"].append(code)
    return out


# ---------------------------------------------------------------------------------------------- pack from records
PACK_MAX_LENS = (1, 31, 32, 33, 150, 249, 250, 505, 506, 736)
PACK_LETTERS = np.frombuffer(b"ACGT" * 12 + b"acgtnNRYSWKMBDHV" + b".-*X", np.uint8)


def pack_waves(max_len):
    """Waves per block of atr_pack_records' launch: 4 up to max_len 249, 2 up to 505, otherwise 1."""
    return 4 if max_len <= 249 else (2 if max_len <= 505 else 1)


def pack_nreads(max_len):
    """1, 63, 64, 65 and 64 waves -+ 1 reads, ``waves`` the launch's waves per block."""
    waves = pack_waves(max_len)
    return sorted({1, 63, 64, 65, 64 * waves - 1, 64 * waves + 1})


def pack_case(max_len, seed):
    """64 waves + 1 records for one max_len: reads of 0 bases, around max_len and beyond it (truncation), for the
    long rows reads of >= 253 bases (more than 64 dwords per line); names sized so that seq_off & 3 takes every
    value; begin / end before, inside and beyond the line."""
    rng = np.random.default_rng(seed)
    nrec = 64 * pack_waves(max_len) + 1
    parts, lens = [], []
    for i in range(nrec):
        pick = i % 8
        if pick == 0:
            n = 0
        elif pick == 1:
            n = max_len + int(rng.integers(-1, 2))
        elif pick == 2:
            n = max_len + int(rng.integers(2, 41))
        elif pick == 3 and max_len >= 505:
            n = int(rng.integers(253, max_len + 1))
        else:
            n = int(rng.integers(0, max_len + 9))
        n = max(n, 0)
        name = b"r" * int(rng.integers(0, 8))
        parts.append(b"@" + name + b"\n" + _letters(rng, PACK_LETTERS, n) + b"\n+\n" + b"I" * n + b"\n")
        lens.append(n)
    text = b"".join(parts)
    recs, _, err = model_index(text)
    assert err == INT64_MAX and [r[3] for r in recs] == lens
    lens = np.asarray(lens)
    kind = rng.integers(0, 4, nrec)
    begin = np.select([kind == 0, kind == 1, kind == 2], [0, rng.integers(-3, 1, nrec), rng.integers(0, lens + 1)], lens + rng.integers(0, 4, nrec))
    kind = rng.integers(0, 4, nrec)
    end = np.select([kind == 0, kind == 1, kind == 2], [lens, lens + rng.integers(1, 5, nrec), rng.integers(0, lens + 1)], rng.integers(-2, 1, nrec))
    return dict(text=text, recs=recs, begin=begin, end=end)


def _packed_rows(packed, nreads, max_len):
    """The packed words of every read as a row (tile64 / plane64: [tile][chunk][lane] x 16 bytes)."""
    nch, nt = (max_len + 31) // 32, (nreads + 63) // 64
    words = packed.cpu().numpy().view(np.uint32)[:nt * nch * 64 * 4]
    return words.reshape(nt, nch, 64, 4).transpose(0, 2, 1, 3).reshape(nt * 64, nch * 4)[:nreads]


def check_pack_records(be):
    """atr_pack_records against atr_pack_reads over a byte matrix built in Python from seq[a:b][:max_len] (same
    table, planes and max_len): packed words of every read, lens, the invalid count.  Returns counts."""
    kinds = (_lib.TABLE_DNA15, _lib.TABLE_IUPAC, _lib.TABLE_ACGT)
    tables = [be.translate_table(k) for k in kinds]
    out = dict(cases=0, reads=0, shifts=set(), long_lines=0, truncated=0, invalid=0, tables=set())
    case_no = 0
    for max_len in PACK_MAX_LENS:
        case = pack_case(max_len, 100 + max_len)
        text = case["text"]
        data = upload_text(be, text)
        for nreads in pack_nreads(max_len):
            recs = case["recs"][:nreads]
            begin, end = case["begin"][:nreads], case["end"][:nreads]
            rows = []
            for (no, nl, so, sl, qo, ql, fl, _), a, b in zip(recs, begin, end):
                a = min(max(int(a), 0), sl)
                b = max(a, min(int(b), sl))
                rows.append(text[so + a:so + b][:max_len])
                out["shifts"].add((so + a) & 3)
                out["long_lines"] += len(rows[-1]) + ((so + a) & 3) > 256
                out["truncated"] += b - a > max_len
            mat = np.full((nreads, max_len), ord("A"), np.uint8)
            for i, row in enumerate(rows):
                mat[i, :len(row)] = np.frombuffer(row, np.uint8)
            lens = np.asarray([len(row) for row in rows], np.int32)
            d_recs, d_mat, d_lens = records_tensor(be, recs), _dev(be, mat), _dev(be, lens)
            for planes in (False, True):
                for nulls in ((False,) if nreads != 65 else (False, True)):
                    table = tables[case_no % 3]
                    out["tables"].add((kinds[case_no % 3], planes))
                    case_no += 1
                    if nulls:                                   # begin == NULL, end == NULL: the whole line
                        full = [text[r[2]:r[2] + r[3]][:max_len] for r in recs]
                        fmat = np.full((nreads, max_len), ord("A"), np.uint8)
                        for i, row in enumerate(full):
                            fmat[i, :len(row)] = np.frombuffer(row, np.uint8)
                        want_lens = np.asarray([len(row) for row in full], np.int32)
                        ref, ref_bad = be.pack_reads(_dev(be, fmat), _dev(be, want_lens), max_len, table, count_invalid=True, planes=planes)
                        got, got_lens, got_bad = be.pack_records(data, d_recs, None, None, max_len, table, count_invalid=True, planes=planes)
                    else:
                        want_lens = lens
                        ref, ref_bad = be.pack_reads(d_mat, d_lens, max_len, table, count_invalid=True, planes=planes)
                        got, got_lens, got_bad = be.pack_records(data, d_recs, _i32(be, begin), _i32(be, end), max_len, table,
                                                                 count_invalid=True, planes=planes)
                    _sync(be)
                    what = (max_len, nreads, planes, nulls)
                    assert got_lens.cpu().tolist() == want_lens.tolist(), what
                    assert got_bad == ref_bad, what
                    assert np.array_equal(_packed_rows(got, nreads, max_len), _packed_rows(ref, nreads, max_len)), what
                    out["cases"] += 1
                    out["reads"] += nreads
                    out["invalid"] += got_bad
    return out


# ---------------------------------------------------------------------------------------------- interval modifiers
def model_quality_trim(oracle, qual, cutoff_front, cutoff_back, base):
    return oracle.quality_trim_index(bytes(qual), cutoff_front, cutoff_back, base)


def model_nextseq_trim(oracle, seq, qual, cutoff, base):
    return oracle.nextseq_trim_index(bytes(seq), bytes(qual), cutoff, base)


def model_masked(seq, a, ubegin, uend):
    """seq = read[a:b]; positions (of the line) outside [ubegin, uend) read N."""
    return bytes(c if ubegin <= a + k < uend else ord("N") for k, c in enumerate(seq))


def model_n_end_trim(oracle, seq):
    """(start, stop) of the read without its N ends, ``read[start:stop]`` (empty when stop <= start)."""
    start, stop = oracle.n_end_trim(bytes(seq))
    return start, max(start, stop)


def quality_case(base, seed=17):
    """16 x 40 records in which (qual_off + begin) & 15 takes every value at every length 0..39, then records of
    150 and 700 bases; qualities in four styles -- all above the cutoffs (the scans stop at their first base), all
    below (they never stop), a bad head and tail around a good middle (they stop in a later block), random."""
    rng = np.random.default_rng(seed + base)
    parts, begin, end, cur = [], [], [], 0
    shapes = [(t, n) for t in range(16) for n in range(40)] + [(int(rng.integers(0, 16)), n) for n in (150, 700) * 8]
    for i, (target, n) in enumerate(shapes):
        a = min(i % 4, n)
        style = (i // 16 + i) % 4
        if style == 0:
            q = rng.integers(41, 42, n)
        elif style == 1:
            q = rng.integers(0, 3, n)
        elif style == 2:
            q = np.full(n, 41)
            edge = int(rng.integers(0, n // 2 + 1))
            q[:edge] = rng.integers(0, 12, edge)
            q[n - edge:] = rng.integers(0, 12, edge)
        else:
            q = rng.integers(0, 42, n)
        seq = bytearray(_letters(rng, np.frombuffer(b"ACGT", np.uint8), n))
        tail = int(rng.integers(0, 8))
        seq[max(n - tail, 0):] = b"G" * min(tail, n)            # --nextseq-trim: G counts as bad
        qual = bytes((q + base).astype(np.uint8))
        nl = (target - a - (cur + n + 5)) % 16                  # qual_off = cur + 1 + nl + 1 + n + 1 + 2
        parts.append(b"@" + b"n" * nl + b"\n" + bytes(seq) + b"\n+\n" + qual + b"\n")
        cur += len(parts[-1])
        begin.append(a)
        end.append(n if i % 5 else max(a, n - 1))
    text = b"".join(parts)
    recs, _, err = model_index(text)
    assert err == INT64_MAX
    for (target, n), rec, a in zip(shapes, recs, begin):
        assert (rec[4] + a) & 15 == target
    assert {((rec[4] + a) & 15, rec[3]) for rec, a in zip(recs[:640], begin)} == {(t, n) for t in range(16) for n in range(40)}
    return dict(text=text, recs=recs, begin=np.asarray(begin), end=np.asarray(end))


QUALITY_CUTOFFS = ((0, 20), (15, 0), (15, 20), (40, 40))


def check_quality_trim(be, oracle):
    """atr_quality_trim_batch for ``-q cf,cb`` and ``--nextseq-trim 20``, bases 33 and 64, against the oracle's
    quality_trim_index / nextseq_trim_index on the read's own text.  Returns counts (records checked; scans of
    the 5' and 3' ends that stop at the first base, later, or run over the whole read)."""
    out = dict(records=0, stop_first=0, stop_later=0, stop_never=0, changed=0)
    for base in (33, 64):
        case = quality_case(base)
        text, recs = case["text"], case["recs"]
        data, d_recs = upload_text(be, text), records_tensor(be, recs)
        for cf, cb, nextseq in [(cf, cb, False) for cf, cb in QUALITY_CUTOFFS] + [(0, 20, True)]:
            begin, end = _i32(be, case["begin"]), _i32(be, case["end"])
            be.quality_trim_batch(data, d_recs, begin, end, cf, cb, base, nextseq)
            _sync(be)
            want_b, want_e = [], []
            for (no, nl, so, sl, qo, ql, fl, _), a, b in zip(recs, case["begin"].tolist(), case["end"].tolist()):
                if b > a:
                    seq, qual = text[so + a:so + b], text[qo + a:qo + b]
                    if nextseq:
                        a, b = a, a + model_nextseq_trim(oracle, seq, qual, cb, base)
                    else:
                        s, e = model_quality_trim(oracle, qual, cf, cb, base)
                        n = b - a
                        out["stop_first"] += (s == 0 and cf > 0) + (e == n and cb > 0 and e > s)
                        out["stop_never"] += (s == 0 and e == 0 and n > 16)
                        out["stop_later"] += (s > 16) + (0 < e < n - 16)
                        a, b = a + s, a + e
                want_b.append(a)
                want_e.append(b)
            assert begin.cpu().tolist() == want_b, (base, cf, cb, nextseq)
            assert end.cpu().tolist() == want_e, (base, cf, cb, nextseq)
            out["records"] += len(recs)
            out["changed"] += sum(x != y for x, y in zip(want_e, case["end"].tolist()))
    return out


def check_nend_trim(be, oracle):
    """atr_nend_trim_batch: reads that are all N, with N only inside, N (and lower-case n, which stays) at the
    ends, and a mask that turns the ends into N -- against the oracle's n_end_trim on the masked sequence."""
    rng = np.random.default_rng(23)
    seqs = [b"", b"N", b"NN", b"N" * 40, b"ACGNNNTA", b"NACGT", b"ACGTN", b"NNACNNGTNNN", b"nnACGTnn", b"NnACGTnN", b"A", b"ANA"]
    for _ in range(300):
        n = int(rng.integers(0, 80))
        seq = bytearray(_letters(rng, np.frombuffer(b"ACGTNn", np.uint8), n))
        head, tail = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        seq[:head] = b"N" * min(head, n)
        seq[max(n - tail, 0):] = b"N" * min(tail, n)
        seqs.append(bytes(seq))
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    recs, _, err = model_index(text)
    assert err == INT64_MAX
    lens = np.asarray([len(s) for s in seqs])
    begin0 = np.minimum(rng.integers(0, 3, len(seqs)), lens)
    end0 = np.maximum(begin0, lens - rng.integers(0, 3, len(seqs)))
    ubegin = rng.integers(0, lens + 1)
    uend = rng.integers(0, lens + 1)
    keep = rng.random(len(seqs)) < 0.3
    ubegin, uend = np.where(keep, 0, ubegin), np.where(keep, lens, uend)
    data, d_recs = upload_text(be, text), records_tensor(be, recs)
    out = dict(records=0, emptied=0, inner_only=0, by_mask=0)
    for masked in (False, True):
        begin, end = _i32(be, begin0), _i32(be, end0)
        if masked:
            be.nend_trim_batch(data, d_recs, begin, end, _i32(be, ubegin), _i32(be, uend))
        else:
            be.nend_trim_batch(data, d_recs, begin, end)
        _sync(be)
        want_b, want_e = [], []
        for r, rec in enumerate(recs):
            a, b = int(begin0[r]), int(end0[r])
            if b > a:
                raw = text[rec[2] + a:rec[2] + b]
                seq = model_masked(raw, a, int(ubegin[r]), int(uend[r])) if masked else raw
                s, e = model_n_end_trim(oracle, seq)
                out["emptied"] += e == s
                out["inner_only"] += (s, e) == (0, b - a) and b"N" in seq
                out["by_mask"] += masked and (s, e) != model_n_end_trim(oracle, raw)
                a, b = a + s, a + e
            want_b.append(a)
            want_e.append(b)
        assert begin.cpu().tolist() == want_b and end.cpu().tolist() == want_e, masked
        out["records"] += len(recs)
    return out


def check_clip(be):
    """atr_clip_batch: front and back each in {0, 1, 5, -1, -5}; the ABI refuses front < 0 and back > 0; Python
    slicing ``read[front:back]`` / ``read[front:]`` otherwise, empty reads left alone."""
    lens = list(range(0, 13)) * 2
    begin0 = np.asarray([0] * 13 + [2] * 13)
    end0 = begin0 + np.asarray(lens)
    end0[5] = begin0[5] - 1                                     # end < begin: an empty read as well
    out = dict(run=0, refused=0, shorter_than_cut=0)
    for front in (0, 1, 5, -1, -5):
        for back in (0, 1, 5, -1, -5):
            begin, end = _i32(be, begin0), _i32(be, end0)
            if front < 0 or back > 0:
                try:
                    be.clip_batch(None, begin, end, front, back)
                except ValueError:
                    out["refused"] += 1
                else:
                    raise AssertionError("clip %d,%d was not refused" % (front, back))
                continue
            be.clip_batch(None, begin, end, front, back)
            _sync(be)
            want_b, want_e = [], []
            for a, b in zip(begin0.tolist(), end0.tolist()):
                if b > a and (front or back):
                    kept = range(a, b)[front:back] if back else range(a, b)[front:]
                    out["shorter_than_cut"] += b - a < front - back
                    a, b = kept.start, max(kept.start, kept.stop)
                want_b.append(a)
                want_e.append(b)
            assert begin.cpu().tolist() == want_b and end.cpu().tolist() == want_e, (front, back)
            out["run"] += 1
    return out


def check_match_trim(be):
    """atr_match_trim_batch: ``read[:rstart]`` / ``read[rstop:]``, the front guessed from ``rstart == 0`` when the
    code is > 1, records without a match, the ``active`` and ``matched`` bytes (given or NULL)."""
    rng = np.random.default_rng(29)
    n = 600
    lens = rng.integers(0, 60, n)
    begin0 = rng.integers(0, 4, n)
    end0 = begin0 + lens
    matches = np.zeros((n, 8), np.int16)
    rstart = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 70, n))
    matches[:, 2] = rstart
    matches[:, 3] = rstart + rng.integers(0, 20, n)
    matches[:, 1] = np.where(rng.random(n) < 0.3, -1, 5)
    front = rng.integers(0, 4, n).astype(np.uint8)
    active0 = (rng.random(n) < 0.8).astype(np.uint8)
    matched0 = (rng.random(n) < 0.2).astype(np.uint8)
    out = dict(run=0, guessed_front=0, trimmed=0)
    for use_front, default_front, use_active, use_matched in ((True, 0, True, True), (False, 0, True, True), (False, 1, False, True),
                                                              (False, 2, True, False), (True, 1, False, False)):
        begin, end = _i32(be, begin0), _i32(be, end0)
        active = _u8(be, active0) if use_active else None
        matched = _u8(be, matched0) if use_matched else None
        be.match_trim_batch(_dev(be, matches), _u8(be, front) if use_front else None, default_front, begin, end, active, matched)
        _sync(be)
        want_b, want_e, want_a, want_m = [], [], active0.tolist(), matched0.tolist()
        for r in range(n):
            a, b = int(begin0[r]), int(end0[r])
            if not use_active or active0[r]:
                if matches[r, 1] < 0:
                    want_a[r] = 0
                else:
                    f = int(front[r]) if use_front else default_front
                    if f > 1:
                        f = 1 if matches[r, 2] == 0 else 0
                        out["guessed_front"] += 1
                    kept = range(a, b)[int(matches[r, 3]):] if f else range(a, b)[:int(matches[r, 2])]
                    out["trimmed"] += len(kept) < b - a
                    a, b = kept.start, kept.stop
                    want_m[r] = 1
            want_b.append(a)
            want_e.append(b)
        assert begin.cpu().tolist() == want_b and end.cpu().tolist() == want_e
        if use_active:
            assert active.cpu().tolist() == want_a
        if use_matched:
            assert matched.cpu().tolist() == want_m
        out["run"] += 1
    return out


# ---------------------------------------------------------------------------------------------- filters
FILTER_ORDER = (1, 2, 3, 4, 5)     # ATR_DEST_*: too short, too long, too many N, discard trimmed, discard untrimmed


def model_filter_mask(seq, matched, min_len, max_len, max_n, discard_trimmed, discard_untrimmed):
    n = len(seq)
    fires = set()
    if min_len > 0 and n < min_len:
        fires.add(1)
    if max_len >= 0 and n > max_len:
        fires.add(2)
    if max_n >= 0:
        count = seq.count(b"N") + seq.count(b"n")
        if max_n < 1:
            if n and count / n > max_n:                         # a fraction of the length; a length of 0 never fires
                fires.add(3)
        elif count > max_n:
            fires.add(3)
    if discard_trimmed and matched:
        fires.add(4)
    if discard_untrimmed and not matched:
        fires.add(5)
    return fires


def model_destination(fires1, fires2=None, min_affected=1):
    for d in FILTER_ORDER:
        hits = (d in fires1) + (fires2 is not None and d in fires2)
        if hits >= (min_affected if fires2 is not None else 1):
            return d
    return 0


def filter_case(seed=31):
    """1 025 records whose kept lengths straddle 0 | 1, 19 | 20 | 21 and 99 | 100 | 101, with N counts (n included) on
    both sides of 0, 0.2, 0.999, 1 and 3."""
    rng = np.random.default_rng(seed)
    nrec = 1025
    edge = (0, 1, 2, 19, 20, 21, 99, 100, 101, 5, 10)
    seqs = []
    for i in range(nrec):
        n = edge[i % len(edge)] if i % 3 else int(rng.integers(0, 130))
        seq = bytearray(_letters(rng, np.frombuffer(b"ACGT", np.uint8), n))
        pick = (i // 3) % 8
        count = (0, 1, 2, 3, 4, n // 5, n // 5 + 1, n)[pick]    # n // 5: the fraction 0.2 exactly (when 5 | n), then one more
        if pick == 7 and i % 2:
            count = max(n - 1, 0)                               # one base that is no N: below 0.999 from 1 000 bases on only
        for p in rng.permutation(n)[:min(count, n)]:
            seq[p] = ord("N") if rng.random() < 0.7 else ord("n")
        seqs.append(bytes(seq))
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    recs, _, err = model_index(text)
    assert err == INT64_MAX
    lens = np.asarray([len(s) for s in seqs])
    cut = rng.random(nrec) < 0.25
    begin = np.where(cut, np.minimum(1, lens), 0)
    end = np.where(cut, np.maximum(begin, lens - 1), lens)
    end[7] = begin[7] - 1                                       # end < begin: length 0
    unmasked = rng.random(nrec) < 0.5
    ubegin = np.where(unmasked, 0, np.minimum(rng.integers(0, 3, nrec), lens))
    uend = np.where(unmasked, lens, np.maximum(lens - rng.integers(0, 3, nrec), 0))
    matched = (rng.random(nrec) < 0.5).astype(np.uint8)
    return dict(text=text, recs=recs, begin=begin, end=end, ubegin=ubegin, uend=uend, matched=matched)


def check_read_filter(be):
    """atr_read_filter_batch: the ``dest`` byte and the ``fail_mask`` byte of 1 025 records under min_len x max_len x
    max_n, the discard switches with random ``matched``, with and without a mask.  Returns counts per destination."""
    case = filter_case()
    text, recs = case["text"], case["recs"]
    data, d_recs = upload_text(be, text), records_tensor(be, recs)
    begin, end = _i32(be, case["begin"]), _i32(be, case["end"])
    ubegin, uend, matched = _i32(be, case["ubegin"]), _i32(be, case["uend"]), _u8(be, case["matched"])
    plain, masked = [], []
    for r, rec in enumerate(recs):
        a = int(case["begin"][r])
        b = max(a, int(case["end"][r]))
        raw = text[rec[2] + a:rec[2] + b]
        plain.append(raw)
        masked.append(model_masked(raw, a, int(case["ubegin"][r]), int(case["uend"][r])))
    switches = ((0, 0), (1, 0), (0, 1), (1, 1))
    configs = []
    for min_len in (0, 1, 20):
        for max_len in (-1, 0, 100):
            for max_n in (-1, 0, 0.2, 0.999, 1, 3):
                configs.append((min_len, max_len, max_n) + switches[len(configs) % 4] + (len(configs) % 3 == 0,))
    configs += [(20, 100, 0.2) + sw + (True,) for sw in switches] + [(0, -1, -1) + sw + (False,) for sw in switches]
    out = dict(configs=0, records=0, dests={d: 0 for d in range(6)}, n_fired_by_mask=0, sides={})
    for min_len, max_len, max_n, d_trim, d_untrim, use_mask in configs:
        args = (data, d_recs, begin, end, ubegin if use_mask else None, uend if use_mask else None, matched, min_len, max_len,
                float(max_n), d_trim, d_untrim)
        got_dest = be.read_filter_batch(*args).cpu().tolist()
        got_mask = be.read_filter_batch(*args, masks=True).cpu().tolist()
        _sync(be)
        want_dest, want_mask = [], []
        for r in range(len(recs)):
            fires = model_filter_mask(masked[r] if use_mask else plain[r], bool(case["matched"][r]), min_len, max_len, max_n,
                                      d_trim, d_untrim)
            want_dest.append(model_destination(fires))
            want_mask.append(sum(1 << d for d in fires))
            if use_mask and 3 in fires:
                out["n_fired_by_mask"] += 3 not in model_filter_mask(plain[r], False, min_len, max_len, max_n, 0, 0)
            out["sides"].setdefault(max_n, set()).add(3 in fires)
        what = (min_len, max_len, max_n, d_trim, d_untrim, use_mask)
        assert got_dest == want_dest, what
        assert got_mask == want_mask, what
        for d in want_dest:
            out["dests"][d] += 1
        out["configs"] += 1
        out["records"] += len(recs)
    return out


def check_pair_filter(be):
    """atr_pair_filter_batch over all 64 x 64 pairs of fail masks, min_affected 1 and 2."""
    m1 = np.repeat(np.arange(64), 64).astype(np.uint8)
    m2 = np.tile(np.arange(64), 64).astype(np.uint8)
    bits = lambda m: {d for d in FILTER_ORDER if m >> d & 1}
    out = dict(pairs=0, differ=0)
    got = {}
    for min_affected in (1, 2):
        got[min_affected] = be.pair_filter_batch(_u8(be, m1), _u8(be, m2), min_affected).cpu().tolist()
        _sync(be)
        want = [model_destination(bits(int(a)), bits(int(b)), min_affected) for a, b in zip(m1, m2)]
        assert got[min_affected] == want, min_affected
        out["pairs"] += len(want)
    out["differ"] = sum(a != b for a, b in zip(got[1], got[2]))
    return out

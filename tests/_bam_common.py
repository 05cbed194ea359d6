"""Shared by test_bam_host.py (the CPU twin, tests/emu/emu_bam.cpp) and test_gpu_bam.py (the kernels of
atropos_amd/csrc/bam_kernels.hip): unaligned BAM input -- the record walk (``atr_bam_walk``) and the decode to FASTQ
text (``atr_bam_to_fastq``) at the C ABI against a plain Python model written from the SAM/BAM specification (section
4.2) and taken from nowhere, and the file drivers against the files the reference writes for the same reads as FASTQ
(tests/golden): ``pysam`` is not needed, the BAM files are made here with ``struct`` and ``zlib``.

A record is ``block_size`` i32, then refID i32, pos i32, l_read_name u8, mapq u8, bin u16, n_cigar_op u16, flag u16,
l_seq i32, next_refID i32, next_pos i32, tlen i32, the NUL-terminated name, the cigar, the bases (4 bits each, high
nibble first, through "=ACMGRSVTWYHKDBN"), the qualities and the tags.  The serial walk goes ``at += 4 + block_size``.

Also builds and loads the twin library and defines the backend that serves it (``BamEmuBackend``)."""
import base64
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import torch

from atropos_amd import _lib, fastq
from tests import _fasta_common as F
from tests import _fastq_kernels_common as K
from tests.emu import backend as emu

BAM_ENTRY_POINTS = ("atr_bam_header", "atr_bam_walk_workspace", "atr_bam_walk", "atr_bam_to_fastq_work_bytes", "atr_bam_to_fastq")
CODES = "=ACMGRSVTWYHKDBN"
CAP = _lib.BAM_MAX_BLOCK
NONE = _lib.INT64_MAX
TILE = 256                                                          # the kernel-level tests: every edge within kilobytes
_twin = []


# ---------------------------------------------------------------------------------------------- the twin
def twin_sources():
    cpp = os.path.join(emu._HERE, "emu_bam.cpp")
    return cpp, [cpp, os.path.join(emu._HERE, "emu_abi.hpp"), os.path.join(emu._ROOT, "include", "atropos_hip.h")] + [
        os.path.join(emu._CSRC, f) for f in ("bam_core.hpp", "fastq_core.hpp")]


def build_twin():
    """tests/emu/libemu_bam.so from emu_bam.cpp and the product's per-record code, by ``build_new_twin``'s g++ line."""
    so = os.path.join(emu._HERE, "libemu_bam.so")
    cpp, deps = twin_sources()
    if emu.stale(so, deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU"] + emu._INC + [cpp, "-o", so])
    return so


def load_twin():
    if not _twin:
        _twin.append(_lib.attach_prototypes(C.CDLL(build_twin()), "emu_", BAM_ENTRY_POINTS))
    return _twin[0]


class BamEmuBackend(F.FastaEmuBackend, _lib.BamCalls):
    """The CPU stand-in with the BAM entry points, which go to a twin library of their own (emu_bam.cpp)."""

    def _call(self, name, *args):
        if name not in BAM_ENTRY_POINTS:
            return super()._call(name, *args)
        fn, at = load_twin()[name]
        return _lib._check(None, fn(*args) if at is None else fn(*args[:at], None, *args[at:]), name)

    _host = _call


# ---------------------------------------------------------------------------------------------- the writer
def record(name, seq, qual, flag=4, cigar=(), tags=b"", ref=-1, mate_ref=-1, l_seq=None, block_size=None, l_name=None):
    """One BAM record.  ``name``: bytes without the NUL; ``seq``: letters of CODES; ``qual``: raw values (a list or
    bytes).  ``l_seq`` / ``block_size`` / ``l_name``: a field that lies about the record."""
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i // 2] |= CODES.index(chr(c) if isinstance(c, int) else c) << (0 if i % 2 else 4)
    name_z = bytes(name) + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref, -1, len(name_z) if l_name is None else l_name, 0, 4680, len(cigar), flag,
                       len(seq) if l_seq is None else l_seq, mate_ref, -1, 0)
    body += name_z + b"".join(struct.pack("<I", c) for c in cigar) + bytes(packed) + bytes(qual) + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def member(data, stored=False):
    """One BGZF member holding ``data`` (at most 65 280 bytes); ``stored``: a stored block, not a compressed one."""
    assert len(data) <= 65280
    comp = zlib.compressobj(0 if stored else 6, zlib.DEFLATED, -15)
    body = comp.compress(data) + comp.flush()
    size = 12 + 6 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + body +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


EOF = member(b"")


def bgzf(payload, cuts=None, eof=True, stored=()):
    """``payload`` as BGZF members cut at the offsets ``cuts`` (default: every 65 280 bytes); member k of ``stored`` is a
    stored block."""
    if cuts is None:
        cuts = list(range(65280, len(payload), 65280))
    edges = [0] + [c for c in cuts if 0 < c < len(payload)] + [len(payload)]
    out = b"".join(member(payload[a:b], k in stored) for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])))
    return out + (EOF if eof else b"")


def fastq_records(text):
    lines = text.split(b"\n")
    return [(lines[k][1:], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def fastq_to_bam(text, paired=False, refs=(), swap=()):
    """The BAM stream (header + records, not yet BGZF) of FASTQ ``text``; ``paired``: records 2i / 2i + 1 get the flags
    of read 1 / read 2 and, like every name-sorted pair, ONE name -- the pair's read 1 name, which the caller's FASTQ
    must use for both; pairs in ``swap`` are stored read 2 first."""
    out = [header(refs=refs)]
    recs = fastq_records(text)
    for i, (name, seq, qual) in enumerate(recs):
        flag = 4
        if paired:
            flag = 77 if i % 2 == 0 else 141
            if i // 2 in swap:
                name, seq, qual = recs[i ^ 1]
                flag = 141 if i % 2 == 0 else 77
        out.append(record(name, seq.upper().replace(b".", b"N"), bytes(q - 33 for q in qual), flag))
    return b"".join(out)


def write_bam(path, stream, cuts=None, eof=True, stored=()):
    with open(str(path), "wb") as fh:
        fh.write(bgzf(stream, cuts, eof, stored))
    return str(path)


# ---------------------------------------------------------------------------------------------- the model
def i32(b, at):
    return struct.unpack_from("<i", b, at)[0]


def model_walk(b, entry=0, final=False, cap=CAP):
    """The serial walk: (starts, consumed, error word)."""
    b = bytes(b)
    n, at, starts, kind = len(b), entry, [], 0
    while True:
        if n - at < 4:
            break
        bs = i32(b, at)
        if bs < 32:
            kind = _lib.BAM_ERR_SMALL
            break
        if bs > cap:
            kind = _lib.BAM_ERR_BIG
            break
        if at + 4 + bs > n:
            break
        l_name, n_cigar, l_seq = b[at + 12], struct.unpack_from("<H", b, at + 16)[0], i32(b, at + 20)
        if l_seq < 0:
            kind = _lib.BAM_ERR_LSEQ
            break
        if bs < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
            kind = _lib.BAM_ERR_SMALL
            break
        starts.append(at)
        at += 4 + bs
    if not kind and final and at != n:
        kind = _lib.BAM_ERR_TRUNCATED
    return starts, at, (at * 8 + kind if kind else NONE)


def model_record(b, at):
    l_name, n_cigar, flag, l_seq = b[at + 12], struct.unpack_from("<H", b, at + 16)[0], struct.unpack_from("<H", b, at + 18)[0], i32(b, at + 20)
    name = at + 36
    seq = name + l_name + 4 * n_cigar
    qual = seq + (l_seq + 1) // 2
    bases = "".join(CODES[(b[seq + i // 2] >> (0 if i % 2 else 4)) & 15] for i in range(l_seq)).encode()
    return dict(name=b[name:name + max(l_name - 1, 0)], name_z=b[name:name + l_name], l_name=l_name, flag=flag, seq=bases,
                qual=b[qual:qual + l_seq])


def model_decode(b, starts, paired=False):
    """(text, error word, records written, offsets)."""
    b = bytes(b)
    recs = [model_record(b, at) for at in starts]
    used = len(recs) - (len(recs) % 2 if paired else 0)
    order, errors = list(range(used)), []
    if paired:
        for i in range(0, used, 2):
            first, second = recs[i], recs[i + 1]
            if first["name_z"] != second["name_z"]:
                errors.append(i * 8 + _lib.BAM_REC_PAIR_NAME)
            elif not second["flag"] & (0x80 if first["flag"] & 0x40 else 0x40):
                errors.append(i * 8 + _lib.BAM_REC_PAIR_FLAGS)
            if not first["flag"] & 0x40:
                order[i], order[i + 1] = i + 1, i
    out, offs = [], [0]
    for r in order:
        rec = recs[r]
        if not rec["seq"]:
            errors.append(r * 8 + _lib.BAM_REC_LSEQ0)
        elif rec["l_name"] == 0:
            errors.append(r * 8 + _lib.BAM_REC_NAME)
        out.append(b"@" + rec["name"] + b"\n" + rec["seq"] + b"\n+\n" + bytes((q + 33) & 255 for q in rec["qual"]) + b"\n")
        offs.append(offs[-1] + len(out[-1]))
    if not errors:                                                     # (the second call runs only behind a clean first)
        for r in order:
            rec = recs[r]
            if any(q > 93 for q in rec["qual"]):
                errors.append(r * 8 + _lib.BAM_REC_QUAL)
            elif b"\n" in rec["name"] or b"\r" in rec["name"]:
                errors.append(r * 8 + _lib.BAM_REC_NAME)
    return b"".join(out), (min(errors) if errors else NONE), used, offs


# ---------------------------------------------------------------------------------------------- inputs
def random_records(n, seed, lens=None, tags=False, names=None):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        l_seq = int(lens[i % len(lens)]) if lens is not None else int(rng.integers(1, 200))
        seq = bytes(np.frombuffer(CODES.encode(), np.uint8)[rng.integers(0, 16, l_seq)])
        qual = bytes(rng.integers(0, 94, l_seq, dtype=np.uint8))
        name = names[i % len(names)] if names is not None else b"r%d" % i + b"x" * int(rng.integers(0, 9))
        extra = b"RGZgroup%d\0" % (i % 3) + b"NMC" + bytes([i % 7]) if tags and i % 2 else b""
        out.append(record(name, seq, qual, tags=extra, cigar=(l_seq << 4,) if i % 5 == 3 else ()))
    return out


def sweep_stream(tile=TILE):
    """``tile`` records of tile + 1 bytes each: record i starts at i modulo ``tile``, so a start falls on every offset
    of a tile -- block_size split 1/3, 2/2 and 3/1 across an edge and the 36 fixed bytes split everywhere among them."""
    out = []
    for i in range(tile):
        room = tile + 1 - 36 - 2                                        # behind a one-letter name
        l_seq = room * 2 // 3 - (i % 3) * 2
        rest = room - l_seq - (l_seq + 1) // 2
        out.append(record(b"abcdefgh"[i % 8:i % 8 + 1], b"ACGTN"[i % 5:i % 5 + 1] * l_seq, bytes([i % 94]) * l_seq, tags=b"t" * rest))
        assert len(out[-1]) == tile + 1
    return out


def decoy_stream(overshoot, tile=TILE):
    """A real record whose B:C tag payload is a well-formed chain of fake records that begins right after a tile edge,
    while the true next start lies later in that tile.  ``overshoot``: the chain's last block_size reaches into the
    middle of a later record; else it ends exactly at the real record's end."""
    lead = random_records(3, 41, lens=(20,))
    at = sum(len(r) for r in lead)
    fixed = len(record(b"host", b"ACGTACGT", b"\7" * 8)) + 3 + 1 + 4      # ... + tag "XB" 'B' + 'C' + count
    pad = (-(at + fixed)) % tile                                          # the fakes begin on a tile edge + 0
    fakes = [record(b"f", b"AC", b"\1\1") for k in range(4)]           # (41 bytes each: the chain stays inside one tile)
    if overshoot:
        fakes[-1] = record(b"f", b"AC", b"\1\1", block_size=len(fakes[-1]) - 4 + 70)
    payload = b"\0" * pad + b"".join(fakes)
    host = record(b"host", b"ACGTACGT", b"\7" * 8, tags=b"XBBC" + struct.pack("<I", len(payload)) + payload)
    fake_at = at + len(host) - len(b"".join(fakes))
    assert fake_at % tile == 0 and (at + len(host)) // tile == fake_at // tile     # the true next start: same tile, later
    tail = random_records(6, 43, lens=(30, 31))
    return b"".join(lead) + host + b"".join(tail)


def decode_records():
    """Everything the decode must get right, in one stream."""
    recs = []
    for l_seq in (1, 2, 63, 64, 65, 127, 128, 129, 301):
        recs += random_records(2, 100 + l_seq, lens=(l_seq,), tags=True)
    recs.append(record(b"codes", CODES.encode(), bytes(range(16))))
    recs.append(record(b"q", b"ACGTN", bytes([0, 93, 0, 93, 93])))
    recs.append(record(b"", b"ACG", b"\1\2\3"))                          # l_read_name 1: an empty name
    recs.append(record(b"n" * 254, b"ACGT", b"\1\2\3\4"))                # l_read_name 255
    recs.append(record(b"cig", b"ACGTA", b"\1\2\3\4\5", cigar=(5 << 4, 3 << 4 | 4)))
    recs.append(record(b"tagged", b"AC", b"\11\12", tags=b"RGZx\0"))
    return recs


# ---------------------------------------------------------------------------------------------- calls and checks
def run_walk(be, b, entry=0, n_ref=0, final=False, tile=TILE, cap=CAP):
    """``atr_bam_walk`` (or the twin's) over ``b``: (starts, consumed, error word, repaired tiles)."""
    data = K.upload_text(be, bytes(b))
    starts, result = be.bam_walk(data, len(b), entry, n_ref, final, tile, cap)
    K._sync(be)
    count, consumed, err, repaired = (int(v) for v in result.cpu().tolist())
    assert count <= starts.numel()
    return [int(v) & 0xFFFFFFFF for v in starts[:count].cpu().tolist()], consumed, err, repaired


def check_walk(be, b, entry=0, n_ref=0, final=False, tile=TILE, cap=CAP):
    got = run_walk(be, b, entry, n_ref, final, tile, cap)
    want = model_walk(b, entry, final, cap)
    assert got[0] == want[0] and got[1:3] == want[1:], (got[1:], want[1:], len(got[0]), len(want[0]))
    return got


def run_decode(be, b, starts, paired=False):
    """``atr_bam_to_fastq`` through ``BamCalls.bam_to_fastq``: (text, error word, records written, offsets)."""
    data = K.upload_text(be, bytes(b))
    table = torch.tensor([s - (1 << 32) if s >= (1 << 31) else s for s in starts] or [0], dtype=torch.int32).to(be.device)
    text, total, used, err, offsets = be.bam_to_fastq(data, len(b), table, len(starts), paired)
    K._sync(be)
    host = text.cpu().numpy().tobytes()
    assert len(host) == (total + 15) // 16 * 16 + 16 and not any(host[total:])
    # (behind an error word of the first call nothing is written: the text is then unspecified)
    return (host[:total] if err == NONE else b""), err, used, [int(v) for v in offsets.cpu().tolist()]


def check_decode(be, b, paired=False):
    starts = model_walk(b)[0]
    got, want = run_decode(be, b, starts, paired), model_decode(b, starts, paired)
    assert got[1:] == want[1:], (got[1:3], want[1:3])
    if want[1] == NONE:
        assert got[0] == want[0]
    return got


# ---------------------------------------------------------------------------------------------- the file drivers
AD = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"


def golden_fq():
    """(FASTQ text, cases): the FASTQ input of tests/golden/fasta.json.gz and the cases the reference ran on it, WITHOUT
    the few of its 200 reads that no BAM reader takes (lower-case bases, a blank inside the sequence, no bases at all): they are taken
    out of the input and, by name, out of the reference's recorded FASTA files; every other byte is the reference's."""
    doc = F.load_doc()
    recs = fastq_records(F.fixture_inputs(doc)["fq"])
    odd = {name for name, seq, _ in recs if not seq or set(seq.decode()) - set(CODES)}
    assert len(recs) == 200 and len(odd) < 20
    text = b"".join(b"@%s\n%s\n+\n%s\n" % r for r in recs if r[0] not in odd)
    cases = []
    for case in doc["cases"]:
        if case["input"] == ["fq"] and not case["error"]:
            files = {}
            for f, blob in case["files"].items():
                lines = base64.b64decode(blob).split(b"\n")
                kept = [lines[k] + b"\n" + lines[k + 1] + b"\n" for k in range(0, len(lines) - 1, 2) if lines[k][1:] not in odd]
                files[f] = base64.b64encode(b"".join(kept)).decode()
            cases.append(dict(case, files=files))
    assert len(cases) >= 2
    return text, cases


def uneven_cuts(n, seed=5):
    """Member boundaries every few hundred bytes, at odd places: records, pairs and block_size fields straddle them."""
    rng = np.random.default_rng(seed)
    cuts, at = [], 0
    while at < n:
        at += int(rng.integers(150, 900))
        cuts.append(at)
    return cuts


# ---------------------------------------------------------------------------------------------- the checks both suites run
def check_sweep(be):
    recs = sweep_stream()
    stream = b"".join(recs)
    starts = check_walk(be, stream)[0]
    assert sorted(s % TILE for s in starts) == list(range(TILE)) and len(starts) == TILE
    assert check_walk(be, stream, final=True)[2] == NONE
    assert check_walk(be, stream, tile=_lib.BAM_TILE)[0] == starts           # the product's tile size
    lead = header(refs=[(b"chr1", 1000)])                                     # an entry inside a tile, n_ref > 0
    assert [s - len(lead) for s in check_walk(be, lead + stream, entry=len(lead), n_ref=1)[0]] == starts
    return len(starts)


def check_long_record(be):
    short = random_records(12, 11, lens=(30, 45, 61))
    big = record(b"long", b"ACGT" * 5000, bytes(range(80)) * 250)
    stream = b"".join(short[:6]) + big + b"".join(short[6:])
    starts = check_walk(be, stream, final=True)[0]
    with_start = {s // TILE for s in starts}
    assert len(starts) == 13 and len(set(range(len(stream) // TILE)) - with_start) > 100     # tiles without a start
    check_walk(be, stream, tile=_lib.BAM_TILE)
    return len(starts)


def check_decoys(be):
    for overshoot in (False, True):
        stream = decoy_stream(overshoot)
        starts, _, err, repaired = check_walk(be, stream, final=True)
        assert err == NONE and len(starts) == 10
        assert repaired > 0, "the decoy did not mislead the speculative pass: the test shows nothing"
    return 2


def truncation_stream():
    return b"".join(random_records(7, 23, lens=(17, 40, 33), tags=True))


def check_truncation(be):
    stream = truncation_stream()
    ends = set(model_walk(stream)[0]) | {len(stream)}
    for k in range(len(stream) + 1):
        cut = stream[:k]
        starts, consumed, err, _ = check_walk(be, cut)
        assert err == NONE and consumed == max(e for e in ends if e <= k)
        _, consumed, err, _ = check_walk(be, cut, final=True)
        assert (err == NONE) == (k in ends) and (err == NONE or err == consumed * 8 + _lib.BAM_ERR_TRUNCATED)
    return len(stream) + 1


def corrupt_streams():
    """[(label, stream, the error kind, the offending record)] -- record 5 of 9 is damaged."""
    recs = random_records(9, 31, lens=(50, 64, 77), tags=True)
    at = sum(len(r) for r in recs[:5])
    out = []
    for label, kind, patch in (("31", _lib.BAM_ERR_SMALL, struct.pack("<i", 31)), ("-1", _lib.BAM_ERR_SMALL, struct.pack("<i", -1)),
                               ("cap", _lib.BAM_ERR_BIG, struct.pack("<i", CAP + 1)), ("fields", _lib.BAM_ERR_SMALL, struct.pack("<i", 40))):
        out.append((label, b"".join(recs[:5]) + patch + b"".join(recs)[at + 4:], kind, at))
    stream = bytearray(b"".join(recs))
    stream[at + 20:at + 24] = struct.pack("<i", -5)
    out.append(("l_seq", bytes(stream), _lib.BAM_ERR_LSEQ, at))
    return out


def check_corruption(be):
    for label, stream, kind, at in corrupt_streams():
        for final in (False, True):
            a, b = check_walk(be, stream, final=final), check_walk(be, stream, final=final)
            assert a == b, label                                            # the same twice
            assert a[2] == at * 8 + kind and a[1] == at and len(a[0]) == 5, label
    return 5


def check_decode_all(be):
    stream = b"".join(decode_records())
    text, err, used, offs = check_decode(be, stream)
    assert err == NONE and used == len(decode_records()) and b"@codes\n" + CODES.encode() + b"\n+\n" in text
    assert b"@\nACG\n+\n\"#$\n" in text and b"@q\nACGTN\n+\n!~!~~\n" in text
    batch, _ = fastq.FastqBatch.from_device(K.upload_text(be, text), len(text), True, be)   # the existing index takes the text
    want = [(r["name"].decode(), r["seq"].decode(), bytes(q + 33 for q in r["qual"]).decode(), "")
            for r in (model_record(stream, at) for at in model_walk(stream)[0])]
    assert batch.to_records() == want
    assert check_decode(be, b"")[2] == 0                                  # zero records
    good = random_records(5, 3, lens=(10,))
    for bad, kind in ((record(b"e", b"", b""), _lib.BAM_REC_LSEQ0), (record(b"e", b"ACGT", bytes([1, 94, 2, 3])), _lib.BAM_REC_QUAL),
                      (record(b"e", b"ACGT", b"\xff" * 4), _lib.BAM_REC_QUAL), (record(b"a\nb", b"ACGT", b"\1\2\3\4"), _lib.BAM_REC_NAME)):
        assert check_decode(be, b"".join(good[:3]) + bad + b"".join(good[3:]))[1] == 3 * 8 + kind
    return used


def pair_records(n, seed, swap=(), names=None):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pair = [record((names or {}).get((i, k), b"p%d" % i), bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20 + k)]),
                       bytes(rng.integers(0, 94, 20 + k, dtype=np.uint8)), flag) for k, flag in ((0, 77), (1, 141))]
        out += pair[::-1] if i in swap else pair
    return out


def check_decode_paired(be):
    recs = pair_records(6, 9, swap=(1, 4))
    stream = b"".join(recs)
    text, err, used, _ = check_decode(be, stream, paired=True)
    assert err == NONE and used == 12
    plain = check_decode(be, b"".join(pair_records(6, 9)))[0]
    assert text == plain                                                 # read 2 stored first is swapped back
    assert check_decode(be, b"".join(pair_records(4, 9, names={(2, 1): b"other"})), paired=True)[1] == 4 * 8 + _lib.BAM_REC_PAIR_NAME
    twice = pair_records(4, 9)
    twice[3] = record(b"p1", b"ACGT", b"\1\2\3\4", 77)                   # 0x40 | 0x40
    assert check_decode(be, b"".join(twice), paired=True)[1] == 2 * 8 + _lib.BAM_REC_PAIR_FLAGS
    neither = pair_records(4, 9)
    neither[4] = record(b"p2", b"ACGT", b"\1\2\3\4", 4)                  # the first is no read 1, the second no read 1 either
    assert check_decode(be, b"".join(neither), paired=True)[1] == 4 * 8 + _lib.BAM_REC_PAIR_FLAGS
    odd = check_decode(be, b"".join(recs[:7]), paired=True)              # an odd count: the last one is left out
    assert odd[2] == 6 and odd[0] == check_decode(be, b"".join(recs[:6]), paired=True)[0]
    return used


def everything(be):
    """Every word and byte the entry points return for the inputs above -- what device and twin must agree on."""
    out = []
    streams = [b"".join(sweep_stream()), decoy_stream(False), decoy_stream(True), truncation_stream()[:-7], b"", b"".join(decode_records())]
    streams += [s for _, s, _, _ in corrupt_streams()]
    for stream in streams:
        for tile in (TILE, 64, _lib.BAM_TILE):
            for final in (False, True):
                out.append(run_walk(be, stream, final=final, tile=tile))
        starts = model_walk(stream)[0]
        for paired in (False, True):
            out.append(run_decode(be, stream, starts, paired))
    for recs in (pair_records(6, 9, swap=(1, 4)), pair_records(4, 9, names={(2, 1): b"other"})):
        stream = b"".join(recs)
        out.append(run_decode(be, stream, model_walk(stream)[0], True))
    return out


# ---- drivers
def pair_fastq(n=40, seed=2):
    """Interleaved FASTQ whose two reads of a pair carry ONE name (what a name-sorted BAM holds), adapters in some."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        for k in (1, 2):
            m = int(rng.integers(20, 70))
            seq = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, m)]) + (AD[:int(rng.integers(0, 30))].encode() if i % 3 else b"")
            out.append(b"@pair%03d\n%s\n+\n%s\n" % (i, seq, bytes(rng.integers(35, 74, len(seq), dtype=np.uint8))))
    return b"".join(out)


def run_trim(argv, src, out_names, tmp, paired=False, **how):
    from atropos_amd.trim import pipeline_from_args
    os.makedirs(str(tmp), exist_ok=True)
    outs = [os.path.join(str(tmp), o) for o in out_names]
    pipe = pipeline_from_args(argv, paired_input=paired)
    if paired:
        pipe.trim_files(src, None, outs[0], outs[1] if len(outs) > 1 else None, **how)
    else:
        pipe.trim_file(src, outs[0], **how)
    got = []
    for o in outs:
        with open(o, "rb") as fh:
            got.append(fh.read())
    return got


def check_drivers_single(be, tmp):
    """The golden FASTQ input as BAM, whole and in 4 KiB chunks over odd member boundaries: the reference's output."""
    import gzip
    text, cases = golden_fq()
    stream = fastq_to_bam(text)
    bam = write_bam(os.path.join(str(tmp), "in.bam"), stream, uneven_cuts(len(stream)), stored=(2, 5))
    fq = os.path.join(str(tmp), "in.fastq")
    with open(fq, "wb") as fh:
        fh.write(text)
    for k, case in enumerate(cases):                                    # the reference's recorded files
        F.check_case(case, {"fq": bam}, os.path.join(str(tmp), "whole%d" % k))
        F.check_case(case, {"fq": bam}, os.path.join(str(tmp), "chunked%d" % k), chunk_bytes=4096)
    want = run_trim(["-a", AD], fq, ["plain.fastq"], tmp, chunk_bytes=4096)[0]
    assert want.count(b"\n") == 4 * len(fastq_records(text)) and len(want) < len(text)
    assert run_trim(["-a", AD], bam, ["whole.fastq"], tmp) == [want]
    assert run_trim(["-a", AD], bam, ["chunked.fastq"], tmp, chunk_bytes=4096) == [want]
    refs = [(b"chromosome_with_a_long_name_%03d" % k, 1000 + k) for k in range(200)]              # a header longer than a 4 KiB chunk; no EOF member
    long_header = fastq_to_bam(text, refs=refs)
    assert len(header(refs=refs)) > 4096
    bam2 = write_bam(os.path.join(str(tmp), "refs.BAM"), long_header, uneven_cuts(len(long_header), 6), eof=False)
    assert run_trim(["-a", AD], bam2, ["refs.fastq"], tmp, chunk_bytes=4096) == [want]
    gz = run_trim(["-a", AD], bam, ["dev.fastq.gz"], tmp, chunk_bytes=4096, device_gzip=True)[0]
    assert gzip.decompress(gz) == want
    assert run_trim(["-a", AD], bam, ["out.fasta"], tmp, chunk_bytes=4096)[0].count(b">") == want.count(b"\n+\n")
    reader = fastq.ChunkedFastqReader(bam, 4096, be)
    try:
        assert reader.fmt == "bam" and reader.inflate_path == "device"
    finally:
        reader.close()
    assert sum(1 for _ in fastq.read_chunks([bam], 4096, be)) > 5
    return len(want)


def check_drivers_paired(be, tmp):
    text = pair_fastq()
    il = os.path.join(str(tmp), "il.fastq")
    with open(il, "wb") as fh:
        fh.write(text)
    stream = fastq_to_bam(text, paired=True, swap=(3, 17, 39))
    bam = write_bam(os.path.join(str(tmp), "il.bam"), stream, uneven_cuts(len(stream), 8))
    argv = ["-a", AD, "-A", AD, "-m", "10"]
    want = run_trim(argv, il, ["w1.fastq", "w2.fastq"], tmp, paired=True)
    assert want[0].count(b"\n") > 40
    assert run_trim(argv, bam, ["o1.fastq", "o2.fastq"], tmp, paired=True) == want
    assert run_trim(argv, bam, ["c1.fastq", "c2.fastq"], tmp, paired=True, chunk_bytes=4096) == want
    assert (run_trim(argv, bam, ["L.fastq"], tmp, paired=True, chunk_bytes=4096) == run_trim(argv, il, ["wL.fastq"], tmp, paired=True))
    odd = write_bam(os.path.join(str(tmp), "odd.bam"), stream + record(b"single", b"ACGT", b"\1\2\3\4", 77), uneven_cuts(len(stream), 8))
    assert run_trim(argv, odd, ["d1.fastq", "d2.fastq"], tmp, paired=True, chunk_bytes=4096) == want   # zip(sam, sam) drops it
    return len(want[0])


def golden_interleaved(tmp):
    """The interleaved cases of tests/golden/pairtext.json.gz as BAM.  The two reads of a pair are named differently
    there ("pair000/1", "pair000/2"), which a paired BAM reader refuses, as the reference does: they go in as they are
    and the error is what is demanded; the single-end road takes the same file and gives the reference's text of
    the reads."""
    from tests.conftest import load_golden
    doc = load_golden("pairtext.json.gz")
    text = base64.b64decode(doc["inputs"]["il"])
    return text, write_bam(os.path.join(str(tmp), "golden_il.bam"), fastq_to_bam(text), uneven_cuts(len(text), 3))


def check_other_drivers(be, tmp):
    from atropos_amd import detect, stats
    text = golden_fq()[0]
    stream = fastq_to_bam(text)
    bam = write_bam(os.path.join(str(tmp), "q.bam"), stream, uneven_cuts(len(stream)))
    fq = os.path.join(str(tmp), "q.fastq")
    with open(fq, "wb") as fh:
        fh.write(text)
    known = detect.KnownContaminants()
    known.add("adapter", AD)
    assert (detect.detect_file(bam, known, max_reads=None, n_reads=200, chunk_bytes=4096) ==
            detect.detect_file(fq, known, max_reads=None, n_reads=200, chunk_bytes=4096))
    assert stats.qc_file(bam, chunk_bytes=4096) == stats.qc_file(fq, chunk_bytes=4096)
    assert stats.error_rate_file(bam, chunk_bytes=4096) == stats.error_rate_file(fq, chunk_bytes=4096)
    ptext = pair_fastq()
    il = os.path.join(str(tmp), "p.fastq")
    with open(il, "wb") as fh:
        fh.write(ptext)
    pstream = fastq_to_bam(ptext, paired=True, swap=(1,))
    pbam = write_bam(os.path.join(str(tmp), "p.bam"), pstream, uneven_cuts(len(pstream)))
    assert stats.qc_files(pbam, chunk_bytes=4096) == stats.qc_files(il, chunk_bytes=4096)
    assert (stats.error_rate_file(pbam, interleaved=True, chunk_bytes=4096) ==
            stats.error_rate_file(il, interleaved=True, chunk_bytes=4096))
    assert (detect.detect_files(pbam, None, known, max_reads=None, n_reads=200, chunk_bytes=4096) ==
            detect.detect_files(il, None, known, max_reads=None, n_reads=200, chunk_bytes=4096))
    return True


def check_refusals(be, tmp):
    import gzip
    import pytest
    from atropos_amd.trim import pipeline_from_args
    inputs = os.path.join(str(tmp), "inputs")
    outdir = os.path.join(str(tmp), "outputs")
    os.makedirs(inputs)
    os.makedirs(outdir)
    text = golden_fq()[0]
    stream = fastq_to_bam(text)
    bam = write_bam(os.path.join(inputs, "a.bam"), stream, uneven_cuts(len(stream)))
    fq = os.path.join(inputs, "a.fastq")
    with open(fq, "wb") as fh:
        fh.write(text)
    sam = os.path.join(inputs, "a.sam")
    with open(sam, "wb") as fh:
        fh.write(b"@HD\tVN:1.6\n")
    out = os.path.join(outdir, "out.fastq")
    pipe, pair = pipeline_from_args(["-a", AD]), pipeline_from_args(["-a", AD, "-A", AD])
    for call in (lambda: pair.trim_files(bam, bam, out, os.path.join(outdir, "out2.fastq")),
                 lambda: pipe.trim_file(bam, os.path.join(outdir, "out.bam")),
                 lambda: pipe.trim_file(bam, os.path.join(outdir, "out.sam")),
                 lambda: pipe.trim_file(sam, out),
                 lambda: pipe.trim_file(os.path.join(inputs, "a.bam.gz"), out),
                 lambda: pipeline_from_args(["-a", AD, "--input-read", "1"]),
                 lambda: next(fastq.read_chunks([bam], 4096, be, byte_ranges=[(0, 100)])),
                 lambda: next(fastq.read_chunks([bam, bam], 4096, be))):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="different formats"):
        pair.trim_files(bam, fq, out, os.path.join(outdir, "out2.fastq"))
    assert os.listdir(outdir) == []
    # a corrupt member; a bad record names its ordinal
    blob = bytearray(open(bam, "rb").read())
    blob[len(blob) // 2] ^= 0x55
    broken = os.path.join(inputs, "broken.bam")
    with open(broken, "wb") as fh:
        fh.write(bytes(blob))
    with pytest.raises(gzip.BadGzipFile):
        pipe.trim_file(broken, out, chunk_bytes=4096)
    recs = random_records(30, 77, lens=(40,))
    recs[20] = record(b"noqual", b"ACGT", b"\xff" * 4)
    bad = write_bam(os.path.join(inputs, "bad.bam"), header() + b"".join(recs), uneven_cuts(2000))
    with pytest.raises(fastq.FormatError, match=r"BAM record 21 \('noqual'\)"):
        pipe.trim_file(bad, out, chunk_bytes=1024)
    recs[20] = record(b"cut", b"ACGT", b"\1\2\3\4", block_size=20)
    bad = write_bam(os.path.join(inputs, "bad2.bam"), header() + b"".join(recs), uneven_cuts(2000))
    with pytest.raises(fastq.FormatError, match="BAM record 21 .*block_size"):
        pipe.trim_file(bad, out, chunk_bytes=1024)
    cut = write_bam(os.path.join(inputs, "cut.bam"), (header() + b"".join(recs[:20]))[:-9], uneven_cuts(2000))
    with pytest.raises(fastq.FormatError, match="BAM record 20 .*ends inside"):
        pipe.trim_file(cut, out, chunk_bytes=1024)
    ptext = pair_fastq(10)
    mixed = fastq_records(ptext)
    mixed[5] = (b"stranger",) + mixed[5][1:]
    renamed = b"".join(b"@%s\n%s\n+\n%s\n" % r for r in mixed)
    pbad = write_bam(os.path.join(inputs, "pbad.bam"), fastq_to_bam(renamed, paired=True))
    with pytest.raises(fastq.FormatError, match="Consecutive reads pair002, stranger in paired-end SAM/BAM file do not have the same name"):
        pair.trim_files(pbad, None, out, os.path.join(outdir, "out2.fastq"))
    with open(os.path.join(inputs, "not.bam"), "wb") as fh:
        fh.write(bgzf(b"@r\nACGT\n+\nIIII\n"))
    with pytest.raises(fastq.FormatError, match="not a BAM file"):
        pipe.trim_file(os.path.join(inputs, "not.bam"), out)
    return True


def golden_single_cases(limit=6):
    """A few single-end cases of tests/golden/trim_cases.json.gz whose reads a BAM file can hold as they are: names
    without a blank, a plain '+' line, bases among the sixteen codes; with the reference's whole output recorded."""
    from tests.conftest import load_golden
    doc = load_golden("trim_cases.json.gz")
    picked = []
    for case in doc["cases"]:
        if case["error"] or "aux" in case or case["input"] not in ("small.fastq", "longad.fastq", "anchor.fastq") or "size" not in case:
            continue
        text = base64.b64decode(doc["inputs"][case["input"]])
        want = base64.b64decode(case["output"])
        recs = fastq_records(text)
        if (len(want) != case["size"] or b"\n+\n" not in text or text.count(b"\n+\n") != len(recs) or
                any(b" " in name or set(seq.decode()) - set(CODES) for name, seq, _ in recs)):
            continue
        picked.append((case["args"], text, want))
    by_input = {}
    for row in picked:
        by_input.setdefault(row[1], []).append(row)
    out = [row for rows in by_input.values() for row in rows[:max(2, limit // max(len(by_input), 1))]]
    return out[:limit]


def check_golden_single(be, tmp):
    cases = golden_single_cases()
    assert len(cases) >= 3
    for k, (args, text, want) in enumerate(cases):
        stream = fastq_to_bam(text)
        bam = write_bam(os.path.join(str(tmp), "case%d.bam" % k), stream, uneven_cuts(len(stream), k))
        assert run_trim(args.split(), bam, ["whole%d.fastq" % k], tmp) == [want], args
        assert run_trim(args.split(), bam, ["chunked%d.fastq" % k], tmp, chunk_bytes=4096) == [want], args
    return len(cases)


def check_golden_interleaved_names(be, tmp):
    """tests/golden/pairtext.json.gz "il": the reads of a pair are named "pair000/1 extra" and "pair000/2 extra", which
    the reference's paired BAM reader refuses; so does this one, with its sentence.  Read single-end, the same file
    gives the same reads as the FASTQ."""
    import pytest
    from atropos_amd.trim import pipeline_from_args
    text, bam = golden_interleaved(tmp)
    with pytest.raises(fastq.FormatError, match="Consecutive reads pair000/1 extra, pair000/2 extra in paired-end SAM/BAM file"):
        pipeline_from_args(["-a", AD, "-A", AD]).trim_files(bam, None, os.path.join(str(tmp), "x1.fastq"), os.path.join(str(tmp), "x2.fastq"))
    plain = b"".join(b"@%s\n%s\n+\n%s\n" % r for r in fastq_records(text))
    fq = os.path.join(str(tmp), "il_plain.fastq")
    with open(fq, "wb") as fh:
        fh.write(plain)
    assert (run_trim(["-a", AD, "-q", "20"], bam, ["se.fastq"], tmp, chunk_bytes=4096) ==
            run_trim(["-a", AD, "-q", "20"], fq, ["se_want.fastq"], tmp, chunk_bytes=4096))
    return True

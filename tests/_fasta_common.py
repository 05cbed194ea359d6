"""Shared by test_fasta_host.py (the CPU twin, tests/emu/emu_fasta.cpp) and test_gpu_fasta.py (the kernels of
atropos_amd/csrc/fasta_kernels.hip): the FASTA index (``atr_fasta_scan`` /
``atr_fasta_index``) and formatter (``atr_fasta_emit``) at the C ABI against a plain Python model of the reader and the
formatter, written from the rules of the format and not taken from anywhere; and the file drivers against the files the
reference writes (tests/golden/fasta.json.gz).

The rules: a line ends at "\\n", "\\r\\n" or a lone "\\r"; every line is stripped of " \\t\\n\\r\\x0b\\x0c\\x1c\\x1d\\x1e\\x1f";
blank lines and lines that begin with '#' are skipped; a line that begins with '>' opens a record named by the rest of
the line; every other line is a piece of the open record's sequence, and text in front of the first record is an
error.  A record of at most one piece is used where it stands, the pieces of any other are joined in a tail behind the
text.  ``final=False`` takes the records in front of the LAST header.

Also builds and loads the twin library and defines the backend that serves it (``FastaEmuBackend``)."""
import base64
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import torch

from atropos_amd import _lib, fastq
from tests import _fastq_kernels_common as K
from tests import _pairtext_common as P
from tests.emu import backend as emu

FASTA_ENTRY_POINTS = ("atr_fasta_work_bytes", "atr_fasta_scan", "atr_fasta_index",
                      "atr_fasta_emit_work_bytes", "atr_fasta_emit")
SPACE = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"
_twin = []


# ---------------------------------------------------------------------------------------------- the twin
def build_twin():
    """tests/emu/libemu_fasta.so from emu_fasta.cpp and the product's per-line code, by ``build_new_twin``'s g++ line."""
    so = os.path.join(emu._HERE, "libemu_fasta.so")
    cpp = os.path.join(emu._HERE, "emu_fasta.cpp")
    deps = [cpp, os.path.join(emu._HERE, "emu_abi.hpp"), os.path.join(emu._ROOT, "include", "atropos_hip.h")] + [
        os.path.join(emu._CSRC, f) for f in ("fasta_core.hpp", "fastq_core.hpp")]
    if emu.stale(so, deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU"] + emu._INC + [cpp, "-o", so])
    return so


def load_twin():
    if not _twin:
        _twin.append(_lib.attach_prototypes(C.CDLL(build_twin()), "emu_", FASTA_ENTRY_POINTS))
    return _twin[0]


class FastaEmuBackend(P.PairTextEmuBackend, _lib.FastaCalls):
    """The CPU stand-in with the FASTA entry points, which go to a twin library of their own (emu_fasta.cpp)."""

    def _call(self, name, *args):
        if name not in FASTA_ENTRY_POINTS:
            return super()._call(name, *args)
        fn, at = load_twin()[name]
        return _lib._check(None, fn(*args) if at is None else fn(*args[:at], None, *args[at:]), name)

    _host = _call


# ---------------------------------------------------------------------------------------------- the model
def model_lines(text):
    """[(first byte, last byte of the line end)] of the complete lines of ``text``."""
    lines, start = [], 0
    for i, c in enumerate(text):
        if c == 10 or (c == 13 and not (i + 1 < len(text) and text[i + 1] == 10)):
            lines.append((start, i))
            start = i + 1
    return lines


def model_index(text, final=True):
    """The records of ``text``: dict(records=[dict(name, seq, name_off, name_len, pieces=[(off, len)], end)], error=None or
    (line number, stripped text), consumed, nlines).  ``final``: a missing last line end is supplied."""
    text = bytes(text)
    if final and text and text[-1] not in (10, 13):
        text += b"\n"
    records, error, heads = [], None, []
    lines = model_lines(text)
    for number, (start, end) in enumerate(lines, 1):
        lo, hi = start, end + 1
        while lo < hi and text[lo] in SPACE:
            lo += 1
        while hi > lo and text[hi - 1] in SPACE:
            hi -= 1
        if lo == hi or text[lo:lo + 1] == b"#":
            pass
        elif text[lo:lo + 1] == b">":
            records.append(dict(name_off=lo + 1, name_len=hi - lo - 1, pieces=[]))
            heads.append(start)
        elif records:
            records[-1]["pieces"].append((lo, hi - lo))
        elif error is None:
            error = (number, text[lo:hi])
        if records:
            records[-1]["end"] = end
    consumed = len(text)
    if not final:
        consumed = heads[-1] if len(heads) > 1 else 0
        records = records[:-1]
    for rec in records:
        rec["name"] = text[rec["name_off"]:rec["name_off"] + rec["name_len"]]
        rec["seq"] = b"".join(text[o:o + n] for o, n in rec["pieces"])
    return dict(records=records, error=error, consumed=consumed, nlines=len(lines), text=text)


def model_descriptors(records, nbytes):
    """(descriptor rows, tail offset, tail bytes) as ``atr_fasta_index`` lays them out for ``records`` -- ALL records of
    a chunk of ``nbytes`` bytes, also the last one that ``final=False`` leaves out: the tail holds its sequence too."""
    tail_off = (nbytes + 15) // 16 * 16 + 16
    rows, tail = [], b""
    for rec in records:
        if len(rec["pieces"]) > 1:
            seq_off = tail_off + len(tail)
            tail += rec["seq"]
        elif rec["pieces"]:
            seq_off = rec["pieces"][0][0]
        else:
            seq_off = rec["name_off"] + rec["name_len"]
        rows.append([rec["name_off"], rec["name_len"], seq_off, len(rec["seq"]), 0, 0, 0, 0])
    return rows, tail_off, tail


def model_format(names_seqs, begin, end, ubegin, uend, dest, which):
    """(text, offsets[n + 1]) of '>' name '\\n' sequence[begin:end] '\\n' for the records with dest == which; bases
    outside [ubegin, uend) read 'N'."""
    out, offs = [], [0]
    for i, (name, seq) in enumerate(names_seqs):
        if dest is None or dest[i] == which:
            a = begin[i]
            b = max(a, end[i])
            ub, ue = (a, b) if ubegin is None else (ubegin[i], uend[i])
            kept = bytes(seq[p] if ub <= p < ue else 78 for p in range(a, b))
            out.append(b">" + name + b"\n" + kept + b"\n")
        offs.append(offs[-1] + (len(out[-1]) if (dest is None or dest[i] == which) else 0))
    return b"".join(out), offs


# ---------------------------------------------------------------------------------------------- inputs
def load_doc():
    from tests.conftest import load_golden
    return load_golden("fasta.json.gz")


def fixture_inputs(doc):
    return {k: base64.b64decode(v) for k, v in doc["inputs"].items()}


def generated(nrec, width, seed, long_at=None):
    """``nrec`` records of 0 .. 3 * width + 2 bases wrapped at ``width``, names of 0 .. 12 bytes; record ``long_at`` has
    70 000 bases (wrapped at 60: it spans many blocks of lines)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nrec):
        n = 70000 if i == long_at else int(rng.integers(0, 3 * width + 3))
        w = 60 if i == long_at else width
        seq = bytes(K.SEQ_LETTERS[rng.integers(0, len(K.SEQ_LETTERS), n)])
        name = bytes(K.NAME_LETTERS[rng.integers(0, 12, int(rng.integers(0, 13)))]).strip(SPACE)
        out.append(b">" + name + b"\n" + b"".join(seq[k:k + w] + b"\n" for k in range(0, n, w)))
    return b"".join(out)


def index_texts(doc):
    """{label: text} of everything the index is checked on."""
    texts = {k: v for k, v in fixture_inputs(doc).items() if k in ("two", "wrap", "messy")}
    for nrec in (0, 1, 2, 63, 64, 65, 257, 4097):
        texts["n%d" % nrec] = generated(nrec, 16, nrec)
    for width in (1, 15, 16, 17):
        texts["w%d" % width] = generated(40, width, 100 + width)
    texts["long"] = generated(4098, 20, 7, long_at=2000)
    texts["header_only"] = b">alone\n"
    texts["empty"] = b""
    texts["blank"] = b"\n \n#x\n"
    texts["crlf_end"] = b">a\r\nAC\r\nGT\r\n>b\rAC\r"
    return texts


# ---------------------------------------------------------------------------------------------- index
def run_index(be, text, final=True):
    """``FastaBatch.from_bytes`` and what it left on the device: (batch, consumed, descriptor rows, record ends, the
    bytes behind the padded text)."""
    batch, consumed = fastq.FastaBatch.from_bytes(text, final=final, backend=be)
    K._sync(be)
    rows = K._host_u32(batch.records).tolist()
    ends = K._host_u32(batch.record_ends).tolist()
    data = batch.data.cpu().numpy().tobytes()
    return batch, consumed, rows, ends, data


def check_index(be, text, final=True):
    """The index of ``text`` against the model: descriptors, record ends, tail bytes, consumed; returns the number of
    records and of tail bytes."""
    model = model_index(text, final)
    assert model["error"] is None
    chunk = model if final else _whole_chunk(text)
    batch, consumed, rows, ends, data = run_index(be, text, final)
    all_rows, tail_off, tail = model_descriptors(chunk["records"], len(model["text"]))
    n = len(model["records"])
    assert consumed == model["consumed"], (consumed, model["consumed"])
    assert rows == all_rows[:n]
    assert ends[:n] == [rec["end"] for rec in model["records"]]
    assert data[:len(model["text"])] == model["text"]
    assert data[tail_off:tail_off + len(tail)] == tail
    assert isinstance(batch, fastq.FastaBatch) and batch.fmt == "fasta" and len(batch) == n
    assert batch.to_records() == [(r["name"].decode("ascii", "replace"), r["seq"].decode("ascii", "replace"), None, "")
                                  for r in model["records"]]
    return n, len(tail)


def _whole_chunk(text):
    """The model of every record whose header line is complete in ``text`` (what the index sees of a chunk that is cut
    anywhere): the text up to its last line end, read as final."""
    lines = model_lines(text)
    return model_index(text[:lines[-1][1] + 1] if lines else b"", True)


def check_cut_everywhere(be, text, lo, hi):
    """``final=False`` on ``text[:k]`` for every k in [lo, hi]: consumed and the records match the model."""
    for k in range(lo, hi + 1):
        check_index(be, text[:k], final=False)
    return hi - lo + 1


def check_head(be, text):
    """``head(k)`` consumes up to the end of record k - 1, whatever k."""
    model = model_index(text, True)
    batch, _ = fastq.FastaBatch.from_bytes(text, backend=be)
    n = len(model["records"])
    for k in sorted({0, 1, n // 2, n - 1, n, n + 5}):
        if k < 0:
            continue
        head, consumed = batch.head(k)
        k = min(k, n)
        assert len(head) == k and consumed == (model["records"][k - 1]["end"] + 1 if k else 0)
    return n


# ---------------------------------------------------------------------------------------------- emit
def emit_call(be, batch, begin, end, ubegin, uend, dest, which, out_misalign=0):
    """atr_fasta_emit (or the twin's) called directly: the sizing call, then the write into a view of a 0xEE pool with
    GUARD bytes around it.  Returns (offsets, text, guards untouched)."""
    ptr = _lib._ptr
    n = len(batch)
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=be.device)
    work = be.empty((max(be._host("atr_fasta_emit_work_bytes", n), 16),), torch.uint8)
    dev = [None if t is None else K._i32(be, t) for t in (begin, end, ubegin, uend)]
    d_dest = None if dest is None else K._u8(be, dest)

    def call(out_ptr):
        be._call("atr_fasta_emit", ptr(batch.data), ptr(batch.records), *[ptr(t) for t in dev], ptr(d_dest), which, n, 0,
                 ptr(offsets), ptr(work), out_ptr)
    call(None)
    K._sync(be)
    offs = offsets.cpu().tolist()
    total = offs[n]
    pool = torch.full((K.GUARD + 16 + total + K.GUARD,), 0xEE, dtype=torch.uint8, device=be.device)
    start = K.GUARD + out_misalign
    if total:
        call(C.c_void_p(pool.data_ptr() + start))
    K._sync(be)
    host = pool.cpu().numpy()
    intact = bool((host[:start] == 0xEE).all() and (host[start + total:] == 0xEE).all())
    return offs, host[start:start + total].tobytes(), intact


def check_emit(be, text, seed=3, fastq_text=None):
    """The formatter over the batch of ``text`` (FASTA) or of ``fastq_text``: every destination, no destination array,
    random intervals (empty ones among them), masks; returns the number of calls."""
    rng = np.random.default_rng(seed)
    if fastq_text is None:
        batch, _ = fastq.FastaBatch.from_bytes(text, backend=be)
        recs = [(r["name"], r["seq"]) for r in model_index(text)["records"]]
    else:
        batch, _ = fastq.FastqBatch.from_bytes(fastq_text, backend=be)
        lines = fastq_text.split(b"\n")
        recs = [(lines[k][1:], lines[k + 1]) for k in range(0, len(lines) - 1, 4)]
    n = len(recs)
    assert len(batch) == n
    lens = np.array([len(s) for _, s in recs], dtype=np.int64)
    full = (np.zeros(n, dtype=np.int64), lens)
    begin = (rng.random(n) * (lens + 1)).astype(np.int64)
    end = begin + (rng.random(n) * (lens - begin + 1)).astype(np.int64)
    end[::7] = begin[::7]                                               # empty kept intervals
    end[3::11] = begin[3::11] - 2                                       # end < begin reads as empty too
    ubegin = begin + (rng.random(n) * (end - begin + 1)).clip(0).astype(np.int64)
    uend = np.maximum(ubegin, end - (rng.random(n) * 4).astype(np.int64))
    dest = rng.integers(0, 4, n)
    calls = 0
    for b, e, ub, ue in (full + (None, None), (begin, end, None, None), (begin, end, ubegin, uend)):
        for d, which in [(None, 0)] + [(dest, w) for w in range(5)]:
            exp_text, exp_offs = model_format(recs, b, e, ub, ue, d, which)
            for mis in (0, 5):
                offs, got, intact = emit_call(be, batch, b, e, ub, ue, d, which, mis)
                assert intact and offs == exp_offs and got == exp_text, (which, mis)
                calls += 1
    return calls


# ---------------------------------------------------------------------------------------------- the file drivers
def write_inputs(doc, tmp):
    paths = {}
    for key, blob in fixture_inputs(doc).items():
        paths[key] = os.path.join(str(tmp), "in.%s.%s" % (key, "fastq" if key == "fq" else "fasta"))
        with open(paths[key], "wb") as fh:
            fh.write(blob)
    return paths


ERRORS = {"ValueError": ValueError, "FormatError": fastq.FormatError}


def run_case(case, paths, tmp, chunk_bytes, **how):
    """One fixture case through ``pipeline_from_args`` and ``trim_file`` / ``trim_files`` in a directory of its own;
    returns ({file name: bytes} of what the run left, the exception it raised or None)."""
    from atropos_amd.trim import pipeline_from_args
    os.makedirs(str(tmp))
    argv = [os.path.join(str(tmp), t) if t.startswith("out.") else t for t in case["args"].split()]
    ins = [paths[k] for k in case["input"]]
    outs = [os.path.join(str(tmp), o) for o in case["output"]]
    error = None
    try:
        pipe = pipeline_from_args(argv, paired_input=len(ins) == 2)
        if len(ins) == 2:
            pipe.trim_files(ins[0], ins[1], outs[0], outs[1], chunk_bytes=chunk_bytes, **how)
        else:
            pipe.trim_file(ins[0], outs[0], chunk_bytes=chunk_bytes, **how)
    except Exception as exc:
        error = exc
    files = {}
    for f in sorted(os.listdir(str(tmp))):
        with open(os.path.join(str(tmp), f), "rb") as fh:
            files[f] = fh.read()
    return files, error


def check_case(case, paths, tmp, chunk_bytes=1 << 20):
    files, error = run_case(case, paths, tmp, chunk_bytes)
    if case["error"]:
        assert type(error) is ERRORS[case["error"][0]] and str(error) == case["error"][1], (case["args"], error)
        return 0
    if error is not None:
        raise error
    want = {f: base64.b64decode(v) for f, v in case["files"].items()}
    assert sorted(files) == sorted(want), case["args"]
    for f in want:
        assert files[f] == want[f], (case["args"], case["input"], f)
    return len(want)


def count_chunks(path, chunk_bytes, be):
    return sum(1 for _ in fastq.read_chunks([path], chunk_bytes, be))


def bgzf(text, be, tmp, name):
    """``text`` as a BGZF file made by the project's own device (or twin) encoder; returns its path."""
    path = os.path.join(str(tmp), name)
    sink = fastq.make_sink(path, 1, len(text) + 4096, be, device_gzip=True)
    sink.write(torch.frombuffer(bytearray(text), dtype=torch.uint8).to(be.device))
    sink.close()
    with gzip.open(path, "rb") as fh:
        assert fh.read() == text
    return path

"""Device-resident FASTQ batches: the MI355X replacement for the reference's per-record
``FastqReader`` / ``Sequence`` / ``FastqFormat`` path (atropos/io/_seqio.pyx:163-245,
atropos/io/seqio.py:686-700).

A chunk of the file is uploaded as raw bytes; the library finds and validates the records
(``atr_fastq_index``), every trimming step is an update of a kept interval per read, and the
surviving records are formatted on the device (``atr_fastq_emit``).  No per-read Python
object exists anywhere on this path.
"""
import collections
import importlib
import os
import struct
import time
from concurrent.futures import Future, ThreadPoolExecutor
from contextlib import ExitStack

import torch

from . import _lib


class FormatError(Exception):
    """Malformed input file (atropos/io/seqio.py FormatError)."""


def _universal_newlines(raw):
    """What Python's text mode (the reference's xopen(..., 'r')) makes of a line's bytes."""
    return raw.replace(b"\r\n", b"\n").replace(b"\r", b"\n")


def _text(b):
    return bytes(b).decode("utf-8", "replace")


class FastqBatch(object):
    """Whole FASTQ records in device memory.

    Attributes:
        data: uint8 tensor with the chunk's bytes (padded to a multiple of 16).
        nbytes: bytes of text in ``data``.
        records: int32 [n, 8] descriptors (``atr_fastq_record``): name_off, name_len,
            seq_off, seq_len, qual_off, qual_len, flags, reserved.
        line_ends: uint32 positions of the line terminators (kept for ``head``).

    Line ends follow Python's universal newlines ("\\n", "\\r\\n", lone "\\r"), which is how
    the reference reads its input.
    """

    def __init__(self, data, nbytes, records, backend, line_ends=None, stride=1):
        self.data, self.nbytes, self.records, self.backend = data, nbytes, records, backend
        self.line_ends = line_ends
        # records of the chunk per record of this batch: 2 for the mates of an interleaved chunk (``mates``), whose
        # ``records`` are every other descriptor of the chunk while ``line_ends`` are the chunk's
        self.stride = int(stride)

    def head(self, nrec):
        """The first ``nrec`` records as a batch of their own, and the number of bytes of text
        they occupy (paired files are consumed in lock step: the shorter chunk decides).  For a mate of an interleaved
        chunk that is the text of the first ``nrec`` PAIRS."""
        nrec = min(int(nrec), len(self))
        consumed = int(self.line_ends[4 * nrec * self.stride - 1].item()) + 1 if nrec else 0
        return FastqBatch(self.data, self.nbytes, self.records[:nrec], self.backend, self.line_ends, self.stride), consumed

    def mates(self):
        """The even and the odd records of an interleaved chunk (an even number of records) as two batches, read 1 and
        read 2 of the pairs: strided views of the descriptors made contiguous, over the one ``data`` tensor."""
        if len(self) % 2 or self.stride != 1:
            raise ValueError("mates(): a whole chunk with an even number of records is needed")
        return [FastqBatch(self.data, self.nbytes, self.records[k::2].contiguous(), self.backend, self.line_ends, 2)
                for k in (0, 1)]

    def __len__(self):
        return self.records.shape[0]

    @property
    def seq_lens(self):
        return self.records[:, 3].contiguous()

    @classmethod
    def from_matrix(cls, ascii_2d, lens=None, backend=None):
        """A batch over a uint8 [n, width] matrix of sequences already on the device (no names,
        no qualities): lets the record-based packer and the compacting adapter stages run on
        reads that did not come from a FASTQ file."""
        be = backend or _lib.get_backend()
        n, width = ascii_2d.shape
        nbytes = n * width
        if nbytes >= (1 << 32) - 16:
            raise ValueError("the matrix must be smaller than 4 GiB")
        data = be.empty(((nbytes + 15) // 16 * 16 + 16,), torch.uint8)
        data[:nbytes].view(n, width).copy_(ascii_2d)
        data[nbytes:].zero_()
        records = torch.zeros((n, 8), dtype=torch.int32, device=data.device)
        off = torch.arange(n, device=data.device, dtype=torch.int64) * width
        records[:, 2] = off.to(torch.int32) if nbytes < (1 << 31) else (off - (off >= (1 << 31)) * (1 << 32)).to(torch.int32)
        records[:, 3] = width if lens is None else lens.to(torch.int32)
        return cls(data, nbytes, records, be)

    @classmethod
    def from_bytes(cls, buf, final=True, backend=None):
        """Index ``buf`` (bytes-like FASTQ text that starts at a record boundary).

        final=True: ``buf`` is the rest of the file -- a missing last newline is tolerated
        and leftover lines raise "FASTQ file ended prematurely" (_seqio.pyx:244-245).
        final=False: only whole records are taken; the number of bytes consumed is returned
        so that the caller can prepend the remainder to its next chunk.
        Returns (batch, consumed_bytes)."""
        be = backend or _lib.get_backend()
        buf = bytes(buf) if not isinstance(buf, (bytes, bytearray)) else buf
        unterminated = bool(final and len(buf) and not buf.endswith((b"\n", b"\r")))
        if unterminated:
            buf = bytes(buf) + b"\n"
        nbytes = len(buf)
        if nbytes >= (1 << 32) - 16:
            raise ValueError("a FASTQ batch must be smaller than 4 GiB; read the file in chunks")
        padded = (nbytes + 15) // 16 * 16 + 16
        host = torch.zeros((padded,), dtype=torch.uint8)
        if nbytes:
            host[:nbytes] = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        data = be.empty((padded,), torch.uint8)
        data.copy_(host)
        return cls.from_device(data, nbytes, final, be, host_text=buf, unterminated=unterminated)

    @classmethod
    def from_device(cls, data, nbytes, final=True, backend=None, host_text=None, unterminated=False):
        """Index FASTQ text that already sits in device memory: ``data`` is a uint8 tensor,
        16-byte aligned, readable up to the next multiple of 16 beyond ``nbytes`` plus one
        byte, whose text ends in a line end.  Returns (batch, consumed_bytes)."""
        be = backend or _lib.get_backend()
        records, line_ends, nlines, err = be.fastq_index(data, nbytes)
        nrec = nlines // 4
        if err != _lib.INT64_MAX:
            if host_text is None:
                host_text = bytes(data[:nbytes].cpu().numpy().tobytes())
            cls._raise_format_error(host_text, line_ends, err)
        if final and nlines % 4 != 0:
            # the reference validates the lines of the incomplete last record as it reads them
            # (_seqio.pyx:208-238) before it runs out of input (:244-245)
            tail = [int(v) for v in line_ends[max(4 * nrec - 1, 0):nlines].cpu().tolist()]
            if nrec == 0:
                tail = [-1] + tail
            if host_text is None:
                host_text = bytes(data[:nbytes].cpu().numpy().tobytes())
            lines = [_universal_newlines(bytes(host_text[tail[i] + 1:tail[i + 1] + 1])) for i in range(len(tail) - 1)]
            if unterminated:
                # the file's last line had no line end: the reference still drops its last
                # character (line[:strip]); give the line a "\n" in place of that character
                lines[-1] = lines[-1][:-2] + b"\n" if len(lines[-1]) > 1 else lines[-1]
            if not lines[0].startswith(b"@"):
                raise FormatError("Line {0} in FASTQ file is expected to start with '@', but found {1!r}".format(
                    1, _text(lines[0])[:10]))
            if len(lines) >= 3 and lines[2] != b"+\n":
                plus, name = lines[2][:-1], lines[0][1:-1]
                if not plus.startswith(b"+"):
                    raise FormatError("Line {0} in FASTQ file is expected to start with '+', but found {1!r}".format(
                        3, _text(plus)[:10]))
                if len(plus) > 1 and plus[1:] != name:
                    raise FormatError(
                        "At line {0}: Sequence descriptions in the FASTQ file don't match "
                        "({1!r} != {2!r}).\n"
                        "The second sequence description must be either empty "
                        "or equal to the first description.".format(3, _text(name), _text(plus[1:])))
            raise FormatError("FASTQ file ended prematurely")
        consumed = nbytes
        if not final:
            consumed = int(line_ends[4 * nrec - 1].item()) + 1 if nrec else 0
        return cls(data, nbytes, records[:nrec], be, line_ends), consumed

    @staticmethod
    def _raise_format_error(buf, line_ends, err):
        """Re-create the reference's message for the first invalid record."""
        r, code = err // 8, err % 8
        ends = [int(v) for v in line_ends[max(4 * r - 1, 0):4 * r + 4].cpu().tolist()]
        if r == 0:
            ends = [-1] + ends
        # the lines as the reference sees them: newline-translated, each ending in "\n"
        lines = [_universal_newlines(bytes(buf[ends[i] + 1:ends[i + 1] + 1])) for i in range(4)]
        name = _text(lines[0][1:-1])
        if code == _lib.FASTQ_ERR_AT:                                      # _seqio.pyx:209-211 / :199-201
            raise FormatError("Line {0} in FASTQ file is expected to start with '@', but found {1!r}".format(
                1, _text(lines[0])[:10]))
        if code == _lib.FASTQ_ERR_PLUS:                                    # :224-227
            raise FormatError("Line {0} in FASTQ file is expected to start with '+', but found {1!r}".format(
                3, _text(lines[2][:-1])[:10]))
        if code == _lib.FASTQ_ERR_NAME2:                                   # :229-235
            raise FormatError(
                "At line {0}: Sequence descriptions in the FASTQ file don't match "
                "({1!r} != {2!r}).\n"
                "The second sequence description must be either empty "
                "or equal to the first description.".format(3, name, _text(lines[2][:-1])[1:]))
        seq, qual = lines[1][:-1], lines[3][:-1]
        rname = name if len(name) <= 100 else name[:97] + "..."            # util.truncate_string
        cause = FormatError(
            "In read named {0!r}: length of quality sequence ({1}) and "
            "length  of read ({2}) do not match".format(rname, len(qual), len(seq)))
        raise FormatError("Error creating sequence record at line {}".format(4)) from cause

    # ------------------------------------------------------------------ views for tests / small batches
    def to_records(self, begin=None, end=None):
        """Host copies [(name, sequence, qualities, name2), ...] -- test helper, not a product path."""
        raw = bytes(self.data[:self.nbytes].cpu().numpy().tobytes())
        out = []
        rec = self.records.cpu().tolist()
        b0 = None if begin is None else begin.cpu().tolist()
        e0 = None if end is None else end.cpu().tolist()
        for i, (no, nl, so, sl, qo, ql, fl, _) in enumerate(rec):
            a = 0 if b0 is None else b0[i]
            b = sl if e0 is None else max(a, e0[i])
            name = raw[no:no + nl].decode("ascii", "replace")
            out.append((name, raw[so + a:so + b].decode("ascii", "replace"),
                        raw[qo + a:qo + b].decode("ascii", "replace"), name if fl & 1 else ""))
        return out


FASTA_SPACE = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"        # what the FASTA index strips (fasta_core.hpp): str.strip() below 0x80
_COMPRESSED = (".gz", ".bz2", ".xz")


def _codec(path):
    """The module that reads and writes a compressed file, by the name's suffix as the reference's xopen chooses it;
    None for any other name."""
    name = str(path)
    for sfx, module in zip(_COMPRESSED, ("gzip", "bz2", "lzma")):
        if name.endswith(sfx):
            return importlib.import_module(module)
    return None


def open_compressed(path, file=None):
    """The decompressed bytes of a ``.gz`` / ``.bz2`` / ``.xz`` file for reading (``file``: the open file to read them
    from), None for any other name."""
    mod = _codec(path)
    return mod.open(file if file is not None else str(path), "rb") if mod else None


def guess_format(path):
    """"fasta", "fastq" or None (unknown) from a file name, its compression suffix aside: the reference's
    ``guess_format_from_name`` over ``splitext_compressed`` (io/seqio.py:958-989).  The formats it knows and this
    project does not read (colorspace FASTA, SAM / BAM) are a NotImplementedError."""
    name = os.path.basename(str(path))
    for sfx in _COMPRESSED:
        if name.lower().endswith(sfx):
            name = name[:-len(sfx)]
            break
    stem, ext = os.path.splitext(name)
    ext = ext.lower()
    if ext in (".fasta", ".fa", ".fna"):
        return "fasta"
    if ext in (".fastq", ".fq") or (ext == ".txt" and stem.endswith("_sequence")):
        return "fastq"
    if ext in (".csfasta", ".csfa", ".sam", ".bam"):
        raise NotImplementedError("%s input / output (%r) is not provided" % (ext[1:], str(path)))
    return None


def file_format(path):
    """"bam" for a name that ends in ``.bam`` (any letter case, no compression suffix: BAM is BGZF inside), else what
    ``guess_format`` says -- ``.sam``, ``.bam.gz`` and colorspace FASTA stay its NotImplementedError."""
    if str(path).lower().endswith(".bam"):
        return "bam"
    return guess_format(path)


def sniff_format(head):
    """"fasta" if the first line of ``head`` (bytes) that is neither blank nor a '#' line begins with '>', else
    "fastq" -- what every input was before FASTA was read (a FASTQ file that begins with '>' is a FormatError either
    way)."""
    for line in _universal_newlines(bytes(head)).split(b"\n"):
        line = line.strip(FASTA_SPACE)
        if line and not line.startswith(b"#"):
            return "fasta" if line.startswith(b">") else "fastq"
    return "fastq"


def input_format(path, explicit=None):
    """The format a file is read as: ``explicit`` ("fasta" | "fastq" | "bam"), else what its name says
    (``file_format``), else what its first byte says once it is decompressed and blank and '#' lines are passed
    (``sniff_format``; the reference raises UnknownFileType for every name it does not know)."""
    if explicit is not None:
        if explicit not in ("fasta", "fastq", "bam"):
            raise ValueError("input_format must be 'fasta', 'fastq' or 'bam'")
        return explicit
    fmt = file_format(path)
    if fmt is not None:
        return fmt
    with (open_compressed(path) or open(str(path), "rb")) as fh:
        return sniff_format(fh.read(1 << 16))


class FastaBatch(FastqBatch):
    """Whole FASTA records in device memory, the reference's FastaReader (io/seqio.py:233-280) over a chunk: the same
    descriptors as a FastqBatch with ``qual_off = qual_len = flags = 0``, so every stage that reads names and bases
    takes it as it is.  A record whose sequence is wrapped over several lines has it in one piece in a tail behind
    the text (``atr_fasta_index``); ``data`` is then longer than the chunk and ``nbytes`` covers the tail.

    ``record_ends``: per record of the CHUNK the last byte of the line end of its last line (kept for ``head``).
    One difference from the reference: whitespace is ASCII (``FASTA_SPACE``); it decodes the file as UTF-8, where
    U+0085 and U+00A0 are stripped too."""

    fmt = "fasta"

    def __init__(self, data, nbytes, records, backend, record_ends=None):
        FastqBatch.__init__(self, data, nbytes, records, backend, None)
        self.record_ends = record_ends

    def head(self, nrec):
        nrec = min(int(nrec), len(self))
        consumed = int(self.record_ends[nrec - 1].item()) + 1 if nrec else 0
        return FastaBatch(self.data, self.nbytes, self.records[:nrec], self.backend, self.record_ends), consumed

    def mates(self):
        raise NotImplementedError("interleaved FASTA is not provided")

    @classmethod
    def from_bytes(cls, buf, final=True, backend=None):
        """Index ``buf`` (bytes-like FASTA text that starts at a header, or at the top of the file).
        final=True: ``buf`` is the rest of the file, a missing last line end is tolerated.  final=False: the records
        in front of the chunk's LAST header are taken -- that record may go on in the next chunk -- and the number
        of bytes consumed, the first byte of that header's line, is returned with them.  Returns (batch, consumed)."""
        be = backend or _lib.get_backend()
        buf = bytes(buf)
        if final and len(buf) and not buf.endswith((b"\n", b"\r")):
            buf += b"\n"
        nbytes = len(buf)
        if nbytes >= (1 << 32) - 32:
            raise ValueError("a FASTA batch must be smaller than 4 GiB; read the file in chunks")
        padded = (nbytes + 15) // 16 * 16 + 16
        host = torch.zeros((padded,), dtype=torch.uint8)
        if nbytes:
            host[:nbytes] = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        data = be.empty((padded,), torch.uint8)
        data.copy_(host)
        return cls.from_device(data, nbytes, final, be, host_text=buf)

    @classmethod
    def from_device(cls, data, nbytes, final=True, backend=None, host_text=None, unterminated=False):
        """Index FASTA text that already sits in device memory (the conditions of ``FastqBatch.from_device``; the
        tensor must be zero-padded to the next multiple of 16 and 16 bytes more).  Returns (batch, consumed)."""
        be = backend or _lib.get_backend()
        grown, records, record_ends, end, _nlines, err = be.fasta_index(data, nbytes)
        if err != _lib.INT64_MAX:
            if host_text is None:
                host_text = bytes(data[:nbytes].cpu().numpy().tobytes())
            cls._raise_format_error(host_text, err)
        nrec, consumed = records.shape[0], nbytes
        if not final:
            nrec = max(nrec - 1, 0)
            consumed = int(record_ends[nrec - 1].item()) + 1 if nrec else 0
        return cls(grown, max(nbytes, end), records[:nrec], be, record_ends), consumed

    @staticmethod
    def _raise_format_error(buf, err):
        """The reference's message for text in front of the first header (io/seqio.py:273-275)."""
        line = _text(_universal_newlines(bytes(buf)).split(b"\n")[err // 8 - 1].strip(FASTA_SPACE))
        shown = line if len(line) <= 100 else line[:97] + "..."             # util.truncate_string
        raise FormatError("At line {0}: Expected '>' at beginning of FASTA record, but got {1!r}.".format(err // 8, shown))

    def to_records(self, begin=None, end=None):
        """Host copies [(name, sequence, None, ""), ...] -- test helper, not a product path."""
        return [(name, seq, None, "") for name, seq, _, _ in FastqBatch.to_records(self, begin, end)]


class RecordSource(object):
    """Read source of the device-resident adapter matchers (``Adapter.match_source``) over the
    kept intervals of a FastqBatch: packs ``sequence[begin:end]`` once per translate table."""

    def __init__(self, batch, begin, end):
        self.fq, self.begin, self.end = batch, begin, end
        self.n = len(batch)
        self._batches = {}

    def max_len(self):
        if getattr(self, "_max_len", None) is None:
            self._max_len = int((self.end - self.begin).clamp_(min=0).max().item()) if self.n else 0
        return self._max_len

    def split_long(self):
        """(source of the reads with the over-long ones emptied, their indices, an AsciiSource of the over-long
        reads): one record beyond the batch pipelines' length does not abort the chunk -- the adapter matcher sends
        those through the long-read sweep (the reference has no length limit, _align.pyx:266-291)."""
        from .adapters import AsciiSource
        lens = (self.end - self.begin).clamp_(min=0)
        long_idx = torch.nonzero(lens > _lib.MAX_READ_LEN).squeeze(1)
        long_lens = lens.index_select(0, long_idx).to(torch.int32)
        width = (int(long_lens.max().item()) + 3) // 4 * 4
        if width > _lib.MAX_LONG_READ_LEN:
            raise ValueError("reads longer than %d bases are outside the device kernels' envelope" % _lib.MAX_LONG_READ_LEN)
        rec = self.fq.records.index_select(0, long_idx)
        off = (rec[:, 2].to(torch.int64) & 0xFFFFFFFF) + self.begin.index_select(0, long_idx).to(torch.int64)
        pos = off[:, None] + torch.arange(width, device=off.device, dtype=torch.int64)[None, :]
        mat = self.fq.data[pos.clamp_(max=self.fq.data.numel() - 1)]
        mat = torch.where((mat >= 97) & (mat <= 122), mat - 32, mat)          # match_to upper-cases the read (:349)
        mat = torch.where(torch.arange(width, device=off.device)[None, :] < long_lens[:, None], mat, torch.zeros_like(mat))
        short = RecordSource(self.fq, self.begin, torch.where(lens > _lib.MAX_READ_LEN, self.begin, self.end))
        return short, long_idx, AsciiSource(mat.contiguous(), long_lens.contiguous())

    def batch_for(self, aligner):
        """The batch ``aligner.locate_batch`` is fastest on: bit planes when the two-pass pre-pass takes the
        aligner on a (ragged) batch of this size, else 4-bit codes."""
        planes = aligner._wants_planes("auto", self.n, self.max_len(), ragged=True)
        return self.batch(aligner.table_kind, aligner._table, planes=planes)

    def batch(self, table_kind, table, planes=False):
        from .batch import ReadBatch
        key = (table_kind, bytes(table), bool(planes))
        if key not in self._batches:
            be = self.fq.backend
            max_len = self.max_len()
            if max_len > _lib.MAX_READ_LEN:
                raise ValueError("reads longer than %d bases are outside the device kernels' envelope"
                                 % _lib.MAX_READ_LEN)
            # Adapter.match_to upper-cases the read first (adapters/__init__.py:349): fold that
            # into the translate table instead of touching the bytes
            folded = bytearray(table)
            for c in range(ord("a"), ord("z") + 1):
                folded[c] = table[c - 32]
            packed, lens = be.pack_records(self.fq.data, self.fq.records, self.begin, self.end, max_len, bytes(folded),
                                           planes=bool(planes))
            self._batches[key] = ReadBatch(packed, lens, self.n, max_len, table_kind, table,
                                           layout="plane64" if planes else "tile64")
        return self._batches[key]

    def sliced(self, starts):
        """The source of the reads ``read[start:]`` (start relative to the kept interval)."""
        begin = self.begin + starts.to(self.begin.dtype)
        return RecordSource(self.fq, begin, torch.maximum(self.end, begin))

    def planes(self, max_len, table_kind, table, check=False, count=False):
        """plane64 pack (insert aligner) of the kept intervals with a given max_len; no case
        folding (InsertAligner compares the reads as they are).  check: every base must have a code;
        count: leave the number of reads with an uncoded character in ``.uncoded_reads``."""
        from .batch import ReadBatch
        be = self.fq.backend
        if count:
            packed, lens, bad = be.pack_records(self.fq.data, self.fq.records, self.begin, self.end, max_len, bytes(table),
                                                count_invalid=True, planes=True)
            batch = ReadBatch(packed, lens, self.n, max_len, table_kind, table, layout="plane64")
            batch.uncoded_reads = bad
            return batch
        if check:
            packed, lens, bad = be.pack_records(self.fq.data, self.fq.records, self.begin, self.end, max_len, bytes(table),
                                                count_invalid=True, planes=True)
            if bad:
                raise ValueError("%d read(s) contain bases without an upper-case IUPAC code; the device insert "
                                 "aligner cannot reverse-complement them" % bad)
        else:
            packed, lens = be.pack_records(self.fq.data, self.fq.records, self.begin, self.end, max_len, bytes(table),
                                           planes=True)
        return ReadBatch(packed, lens, self.n, max_len, table_kind, table, layout="plane64")


# ---------------------------------------------------------------------------------------------
# file streaming: page-locked staging, threaded reads, read-ahead and write-behind
_STAGING_POOL = []           # page-locked buffers are expensive to create: released ones are kept for reuse


def _staging(nbytes, pinned):
    for i, t in enumerate(_STAGING_POOL):
        if t.numel() >= nbytes and t.is_pinned() == bool(pinned):
            return _STAGING_POOL.pop(i)
    t = torch.empty((nbytes,), dtype=torch.uint8)
    return t.pin_memory() if pinned else t


STAGING_POOL_BYTES = 4 << 30  # page-locked memory the pool keeps between runs (more starves other processes of a shared node);
if os.environ.get("ATR_STAGING_POOL_GB"):     # ATR_STAGING_POOL_GB: a host that runs file after file with many part files keeps more
    STAGING_POOL_BYTES = int(float(os.environ["ATR_STAGING_POOL_GB"]) * (1 << 30))


def _release(buffers):
    _STAGING_POOL.extend(buffers)
    del _STAGING_POOL[:-64]                                   # at most 64 (a paired run with merging into eight parts holds 56)
    total = 0
    for i in range(len(_STAGING_POOL) - 1, -1, -1):           # ... and at most STAGING_POOL_BYTES, the newest first
        total += _STAGING_POOL[i].numel()
        if total > STAGING_POOL_BYTES:
            del _STAGING_POOL[:i + 1]
            break


IO_THREADS = 8              # pread slices per chunk (a page-cached file scales to ~6 GB/s per thread); ATR_IO_THREADS
if os.environ.get("ATR_IO_THREADS"):
    IO_THREADS = max(1, int(os.environ["ATR_IO_THREADS"]))


class StageClock(object):
    """Seconds the streaming loop spent WAITING per stage (what bounds file -> file)."""

    def __init__(self):
        self.seconds = {}

    def add(self, stage, t0):
        self.seconds[stage] = self.seconds.get(stage, 0.0) + (time.perf_counter() - t0)


class _NotBgzf(Exception):
    """(inside the reader) The BGZF walk met a member that is none, at this file offset."""

    def __init__(self, offset):
        Exception.__init__(self, offset)
        self.offset = offset


# What a source hands out.  ``data``: the device tensor (zero behind ``nbytes``, padded to 16 bytes and 16 more);
# ``host``: the same bytes in the staging buffer, on the roads whose text passes through it; ``unterminated``: the
# file's last newline was missing and has been supplied; ``ready`` / ``keep``: the event behind the upload and the
# tensors the upload stream allocated (``_ChunkIO.claim``).
Chunk = collections.namedtuple("Chunk", "data nbytes final host unterminated ready keep")


def _settled(result=None, error=None):
    """A future that is done: a source's ``pending`` is a future of a Chunk on every road, and a failure met while the
    chunk was put together is raised by its ``result()``, when the chunk is asked for."""
    fut = Future()
    if error is not None:
        fut.set_exception(error)
    else:
        fut.set_result(result)
    return fut


class _ChunkIO(object):
    """What the input roads of a reader share, each written once: the file and its size, the page-locked staging
    buffers and whose turn it is, the ``pread`` pool and the read-ahead thread, the upload stream, the clock."""

    def __init__(self, path, backend, clock, chunk_bytes, limits):
        self.file = open(path, "rb")
        self.fd, self.size = self.file.fileno(), os.fstat(self.file.fileno()).st_size
        self.be, self.clock, self.chunk_bytes = backend, clock, chunk_bytes
        self.limits = limits                                  # the reader: READ_AHEAD, RESERVE, BGZF_SCAN, STREAM_SPACING
        self.pinned = getattr(backend, "name", "") == "hip"
        self.buf, self.uploaded, self.next_slot = [], [], 0
        self.readers = self.ahead = self.upload_stream = None

    def allocate(self, nbuf):
        """The staging buffers (a chunk and the reserve for the carry in front of it) and the threads of a road."""
        for _ in range(nbuf):
            self.buf.append(_staging(self.chunk_bytes + self.limits.RESERVE + 32, self.pinned))
        self.uploaded = [None] * nbuf                         # per staging buffer: the event behind its last upload
        self.readers = ThreadPoolExecutor(IO_THREADS)
        self.ahead = ThreadPoolExecutor(1)
        # the host -> device copy of a chunk runs on its own stream: it overlaps the GPU work on the chunk before
        self.upload_stream = torch.cuda.Stream(device=self.be.device) if self.pinned else None

    def read(self, view, offset, want):
        """Starts reading the file's bytes [offset, offset + want) into ``view``, a slice per thread of the pool;
        ``finish`` waits for them."""
        step = ((want + IO_THREADS - 1) // IO_THREADS + 4095) & ~4095
        jobs = []
        for t in range(IO_THREADS):
            lo, hi = t * step, min(want, (t + 1) * step)
            if hi > lo:
                jobs.append(self.readers.submit(os.preadv, self.fd, [view[lo:hi]], offset + lo))
        return jobs, want

    def finish(self, read):
        jobs, want = read
        if sum(j.result() for j in jobs) != want:
            raise IOError("short read: the input file changed while it was being read")
        return want

    def take_slot(self):
        """The staging buffer whose turn it is, once the upload that last read it has landed (chunks ago: long gone)."""
        slot = self.next_slot
        self.next_slot = (slot + 1) % len(self.buf)
        if self.uploaded[slot] is not None:
            self.uploaded[slot].synchronize()
            self.uploaded[slot] = None
        return slot

    def on_upload_stream(self):
        """A context: the upload stream, where the run has one (the CPU twins have none)."""
        stack = ExitStack()
        if self.upload_stream is not None:
            stack.enter_context(torch.cuda.device(self.be.device))
            stack.enter_context(torch.cuda.stream(self.upload_stream))
        return stack

    def to_device(self, host, n, pad=16):
        """``host[:n]`` in a new device tensor of ``n`` rounded up to 16, and ``pad``, bytes: zero behind ``n``."""
        data = self.be.empty(((n + 15) // 16 * 16 + pad,), torch.uint8)
        data[:n].copy_(host[:n], non_blocking=True)
        data[n:].zero_()
        return data

    def mark(self, slot):
        """(on the upload stream) The event behind what was queued so far: staging buffer ``slot`` is free after it."""
        ready = None
        if self.upload_stream is not None:
            ready = torch.cuda.Event()
            ready.record()
        self.uploaded[slot] = ready
        return ready

    def host_chunk(self, slot, host, nbytes, final, lines):
        """The chunk of [carry | new bytes] as they stand in ``host``, a view of staging buffer ``slot``: its upload is
        started; a missing last newline of the file is tolerated (_seqio.pyx:240-243) where the decoder reads ``lines``."""
        unterminated = bool(lines and final and nbytes and int(host[nbytes - 1]) not in (10, 13))
        if unterminated:
            host[nbytes] = 10
            nbytes += 1
        with self.on_upload_stream():
            data, ready = self.to_device(host, nbytes), self.mark(slot)
        return Chunk(data, nbytes, final, host, unterminated, ready, (data,))

    def starts_with_bgzf(self):
        head = torch.frombuffer(bytearray(os.pread(self.fd, 65536, 0)), dtype=torch.uint8) if self.size else None
        return head is not None and self.be.bgzf_scan(head, 0, head.numel(), 1)[4]

    def claim(self, chunk):
        """The caller's stream waits for the chunk's upload and takes over the tensors the upload stream allocated."""
        if chunk.ready is not None:
            with torch.cuda.device(self.be.device):
                cur = torch.cuda.current_stream()
                cur.wait_event(chunk.ready)
                for t in chunk.keep:
                    if t is not None:
                        t.record_stream(cur)

    def close(self):
        for pool in (self.readers, self.ahead):
            if pool is not None:
                pool.shutdown()                               # (waits: reads and slabs still in flight own their buffers)
        for ev in self.uploaded:
            if ev is not None:
                ev.synchronize()
        self.file.close()
        _release(self.buf)
        self.buf = []


def _end_last_line_on_device(io, chunk, lines):
    """A missing last newline is tolerated (_seqio.pyx:240-243) in a chunk inflated on the device as well (in a staging
    buffer: ``_ChunkIO.host_chunk``), on the caller's stream, where the decoder reads ``lines``."""
    data, nbytes = chunk.data, chunk.nbytes
    if not (lines and chunk.final and nbytes and int(data[nbytes - 1].item()) not in (10, 13)):
        return chunk
    data[nbytes] = 10
    if chunk.ready is not None:                               # (the carry is copied on the upload stream)
        io.upload_stream.wait_stream(torch.cuda.current_stream(io.be.device))
    return chunk._replace(nbytes=nbytes + 1, unterminated=True)


class _Source(object):
    """One input road of a reader.  ``pending`` is a future of the next Chunk (``_settled``); ``take`` makes it the
    current one on the caller's stream; ``advance`` puts the one after it together behind what the caller left;
    ``close`` drains what the source has in flight on the read-ahead thread (``_ChunkIO.close`` then waits for the
    ``pread`` pool and the uploads).  ``lines``: the decoder reads lines of text, so a missing last newline is
    supplied."""

    inflate_path = None

    def __init__(self, io, lines):
        self.io, self.lines = io, lines
        self.pending = self.chunk = None

    def carry(self, consumed):
        """What the caller left of the current chunk, to stand in front of the next one (None at the start: nothing):
        ``bytes`` on the roads that put a chunk together in a staging buffer."""
        return bytes(self.chunk.host[consumed:self.chunk.nbytes].numpy().tobytes())

    def take(self, chunk):
        self.io.claim(chunk)
        self.chunk = chunk
        return chunk

    def advance(self, consumed):
        """-> the source of the next chunk: this one, one that takes over from it, or None: the file is exhausted and
        nothing is carried over."""
        if self.chunk.final and consumed == self.chunk.nbytes:
            return None
        return self.prepare(self.carry(consumed))

    def close(self):
        pass


class _DeviceSource(_Source):
    """The roads that put a chunk together on the device: the carry is (tensor, lo, hi), a slice of the current chunk
    that is copied device to device -- the text never visits the host."""

    def carry(self, consumed):
        return self.chunk.data, consumed, self.chunk.nbytes


class _PlainSource(_Source):
    """Plain files: ``READ_AHEAD`` chunks are being READ while the GPU works on the current one.  What a chunk
    carries over from the one before it (its unfinished last record; in a paired run the surplus records of the
    file with the smaller records) is known only once that chunk has been indexed on the device, but the file
    READ does not depend on it: the new bytes land behind a reserve at the front of the staging buffer, the
    carried-over tail is copied in front of them when it is known, and the host -> device copy (its own
    stream) covers both.  Rounds 2-5 read chunk i + 1 only after chunk i was indexed -- read + upload in one
    chain, the upload engine idle during every read (the "upload_and_index" wait of ``trim_file``): 16 M x 150 bp
    into eight part files 64 -> 107 M reads/s.  (A producer thread that also INDEXES each chunk on the upload stream, so
    that the next upload starts a record count after the last, was measured next: 96 M -- its index kernels and its
    Python run against the caller's -- and is not kept.)  ``byte_range``: only these bytes of the file."""

    def __init__(self, io, lines, byte_range):
        _Source.__init__(self, io, lines)
        self.pos, self.end = byte_range or (0, io.size)       # the next pread, the end
        self.reads = collections.deque()                      # (slot, pread jobs and bytes asked for, last chunk of the file)
        self.read_done = False
        self.carry_est = 0
        io.allocate(io.limits.READ_AHEAD + 1)
        for _ in range(io.limits.READ_AHEAD):
            self._issue_read()

    def _issue_read(self):
        if self.read_done:
            return
        io = self.io
        slot = io.take_slot()                                 # (three chunks ago: long gone)
        # a chunk is carry + new bytes ~ chunk_bytes in all: in a paired run the file with the smaller records
        # carries its surplus records over every time, and reading a full chunk on top of it would let that
        # surplus grow without bound (1 % of a chunk per step for records 1 % apart).  The carry of the chunk
        # this read will follow is not known yet; the last one seen stands in for it (it drifts slowly).
        want = max(io.chunk_bytes - self.carry_est, io.chunk_bytes // 4)
        want = min(want, self.end - self.pos)
        read = io.read(memoryview(io.buf[slot].numpy())[io.limits.RESERVE:], self.pos, want)
        self.pos += want
        self.read_done = self.pos >= self.end
        self.reads.append((slot, read, self.read_done))

    def prepare(self, carry):
        """The next chunk: its carried-over head in front of the bytes read for it, and its upload."""
        io, reserve = self.io, self.io.limits.RESERVE
        t0 = time.perf_counter()
        if self.reads:
            slot, read, final = self.reads.popleft()
            got = io.finish(read)
        else:                                                 # the file is read; records carried over are left
            slot, got, final = io.take_slot(), 0, True
        io.clock.add("wait_file_read", t0)
        n0 = len(carry or b"")
        if n0 > reserve:
            raise ValueError("%d bytes carried over from one chunk to the next (a FASTQ record, or the surplus records of "
                             "one file of a pair, of more than %d bytes)" % (n0, reserve))
        host = io.buf[slot][reserve - n0:]
        if n0:
            memoryview(host.numpy())[:n0] = carry
        self.carry_est = n0
        self.pending = _settled(io.host_chunk(slot, host, n0 + got, final, self.lines))
        self._issue_read()                                    # the buffer of the chunk before this one is free again
        return self


class _DecompressedSource(_Source):
    """``.gz`` / ``.bz2`` / ``.xz`` input (what the reference's xopen opens by extension) is decompressed by one
    read-ahead thread straight into the staging buffer, one chunk ahead: the decompressor then sets the pace."""

    def __init__(self, io, lines, stream, inflate_path):
        _Source.__init__(self, io, lines)
        self.stream, self.inflate_path = stream, inflate_path
        io.allocate(2)

    def prepare(self, carry):
        self.pending = self.io.ahead.submit(self._fill, carry)
        return self

    def _fill(self, carry):
        io = self.io
        slot = io.take_slot()
        host = io.buf[slot]
        view = memoryview(host.numpy())
        n0 = len(carry or b"")
        if n0:
            view[:n0] = carry
        room = host.numel() - 32 - n0
        want = max(io.chunk_bytes - n0, min(io.chunk_bytes // 4, room))
        if want <= 0:
            raise ValueError("FASTQ record of more than %d bytes" % host.numel())
        want, got = min(want, room), 0
        while got < want:
            n = self.stream.readinto(view[n0 + got:n0 + want])
            if not n:
                break
            got += n
        return io.host_chunk(slot, host, n0 + got, got < want, self.lines)


class _BgzfSource(_DeviceSource):
    """BGZF input (what ``bgzip``, htslib and ``device_gzip=True`` write: members of at most 64 KiB that carry their own
    size): the COMPRESSED bytes take the plain-file road -- slabs read ahead with the ``pread`` pool and walked member by
    member on the host (``bgzf_scan``), a job that never waits for the GPU -- and are inflated on the device
    (``gunzip_members``, a wave per member) straight into the chunk's text tensor behind the carried-over tail, which is
    a device-to-device copy.  A member that fails its checks is a ``gzip.BadGzipFile`` naming its file offset, a file
    that ends inside a member an ``EOFError``; a member that is not BGZF is a ``BadGzipFile`` too, unless ``any_gzip``:
    then a ``_GzipStreamSource`` takes over at its offset."""

    inflate_path = "device"

    def __init__(self, io, lines, any_gzip):
        _Source.__init__(self, io, lines)
        self.any_gzip = any_gzip
        self.pos = 0                                          # the next slab's file offset
        self.reads = collections.deque()                      # futures of _read_slab
        self.carry_est = 0
        self.ratio = 1.0                                      # compressed bytes per byte of text, as last seen
        self.members = None                                   # of the pending chunk: status, bad, file offset, member offsets
        io.allocate(io.limits.READ_AHEAD + 1)
        for _ in range(io.limits.READ_AHEAD):
            self.reads.append(io.ahead.submit(self._read_slab))

    def _read_slab(self):
        """(read-ahead thread) The next slab of compressed bytes and its whole members, as many as hold the text of
        a chunk.  Nothing here waits for the GPU but the reuse of a staging buffer three chunks later."""
        io, scan = self.io, self.io.limits.BGZF_SCAN
        slot = io.take_slot()
        host = io.buf[slot]
        budget = max(io.chunk_bytes - self.carry_est, io.chunk_bytes // 4)
        want = min(io.size - self.pos, host.numel() - 32, max(int(budget * self.ratio * 1.25) + (128 << 10), 1 << 17))
        io.finish(io.read(memoryview(host.numpy()), self.pos, want))
        at_end = self.pos + want >= io.size
        member_at, text_at, k, covered, error = [0], [0], 0, 0, None
        while covered < want and text_at[-1] <= budget and k + scan <= _lib.GUNZIP_MAX_MEMBERS:
            m_at, t_at, n, took, ok = io.be.bgzf_scan(host, covered, want, scan)
            member_at += [covered + v for v in m_at[1:n + 1].tolist()]
            text_at += [text_at[-1] + v for v in t_at[1:n + 1].tolist()]
            k += n
            covered += took
            if not ok and self.any_gzip:
                error = _NotBgzf(self.pos + covered)          # (device_gunzip="any": the stream road goes on from here)
            elif not ok:
                import gzip
                error = gzip.BadGzipFile("not a BGZF member at file offset %d (device_gunzip wants BGZF throughout)" % (self.pos + covered))
            if not ok or n < scan:
                break
        while k > 1 and text_at[k] > budget:                  # (members are taken while their text fits)
            k -= 1
        if k:
            error = None                                      # (the member behind these opens the next slab)
        elif error is None and at_end and want:
            error = EOFError("Compressed file ended before the end-of-stream marker was reached")
        elif error is None and want:
            raise IOError("no whole BGZF member in %d bytes at file offset %d" % (want, self.pos))
        covered = member_at[k]
        if text_at[k]:
            self.ratio = covered / float(text_at[k])
        pos = self.pos
        self.pos += covered
        return slot, pos, covered, member_at[:k + 1], text_at[:k + 1], self.pos >= io.size, error

    def prepare(self, carry):
        """The next chunk: [carried-over text | the text of the next slab's members], both put there on the device."""
        io, be = self.io, self.io.be
        n0 = carry[2] - carry[1] if carry else 0
        self.carry_est = n0
        t0 = time.perf_counter()
        slot, pos, n, member_at, text_at, final, error = self.reads.popleft().result()
        io.clock.add("wait_file_read", t0)
        if isinstance(error, _NotBgzf):                       # an ordinary member behind BGZF members
            self.close()
            self.reads.clear()
            return _GzipStreamSource(io, self.lines, error.offset, self.ratio).prepare(carry)
        if error is not None:
            self.pending = _settled(error=error)              # (raised when this chunk is asked for)
            return self
        k, total = len(member_at) - 1, text_at[-1]
        nbytes = n0 + total
        status = bad = None
        with io.on_upload_stream():
            data = be.empty(((nbytes + 15) // 16 * 16 + 16,), torch.uint8)
            if n0:
                data[:n0].copy_(carry[0][carry[1]:carry[2]])
            if k:
                comp = io.to_device(io.buf[slot], n, pad=0)
                offsets = torch.tensor([member_at, text_at], dtype=torch.int64).to(be.device)
                status, bad = be.gunzip_members(comp, n, offsets[0], offsets[1], k, data[n0:], total)
            data[nbytes:].zero_()
            ready = io.mark(slot)
        self.reads.append(io.ahead.submit(self._read_slab))   # (past the end of the file: an empty, final slab)
        self.members = status, bad, pos, member_at
        self.pending = _settled(Chunk(data, nbytes, final, None, False, ready, (data, status, bad)))
        return self

    def take(self, chunk):
        _Source.take(self, chunk)
        status, bad, pos, member_at = self.members
        if bad is not None and int(bad.item()):
            import gzip
            first = int(torch.nonzero(status)[0].item())
            raise gzip.BadGzipFile("BGZF member at file offset %d fails its checks (status %d of inflate_core.hpp)"
                                   % (pos + member_at[first], int(status[first].item())))
        self.chunk = _end_last_line_on_device(self.io, chunk, self.lines)
        return self.chunk

    def close(self):
        for fut in self.reads:
            fut.exception()                                   # (a slab still being read owns its buffer)


class _GzipStreamSource(_DeviceSource):
    """Any other ``.gz`` member (``device_gunzip="any"``): an ordinary gzip file, or the rest of a file from an ordinary
    member behind BGZF ones on (then the BGZF source's staging buffers, pools and last compression ratio are taken
    over), inflated on the device member by member, slab by slab (``gunzip_stream``: the deflate stream split
    speculatively).  The host parses the member headers, issues one call per slab of compressed bytes into
    the chunk's text tensor, reads the call's eight result words back (the next call starts at their ``end_bit``), keeps
    the last 32 KiB of text as the next call's window and checks CRC-32 and ISIZE at a member's end.  A chunk holds at
    least one deflate block.  The slab is staging buffer 0; ``offset``: where a member's header stands (or the file
    ends)."""

    inflate_path = "stream"

    def __init__(self, io, lines, offset, ratio):
        _Source.__init__(self, io, lines)
        if not io.buf:                                        # (else: taken over from a BGZF source, whose uploads have landed)
            io.allocate(1)
        self.ratio = ratio                                    # compressed bytes per byte of text, as last seen
        self.pos = offset                                     # file offset of slab byte 0
        self.n = 0                                            # bytes of the slab
        self.at = 0                                           # next byte of the slab: a header, or (in a member) unused
        self.dev = None                                       # the slab on the device
        self.member = None                                    # file offset of the member being inflated
        self.bit = 0                                          # ... and the bit of the slab its next block starts at
        self.crc = self.isize = 0
        self.window = io.be.empty((32768,), torch.uint8)
        self.wlen = 0
        self.work = None
        self.done = False
        # compressed bytes per speculative start: see ChunkedFastqReader.STREAM_SPACING
        self.spacing = min(io.limits.STREAM_SPACING, max(256, io.chunk_bytes // 64))

    def _load(self, start, want):
        """Slab := the file's bytes [start, start + want), as far as the file goes."""
        io = self.io
        want = max(0, min(want, io.buf[0].numel() - 32, _lib.GUNZIP_STREAM_MAX, io.size - start))
        io.finish(io.read(memoryview(io.buf[0].numpy()), start, want))
        self.bit -= 8 * (start - self.pos)
        self.at -= start - self.pos
        self.pos, self.n, self.dev = start, want, None

    def _more(self, keep_from, budget):
        """A slab that begins at slab byte ``keep_from`` and is larger than what is left behind it; -> False at the file's end."""
        if self.pos + self.n >= self.io.size:
            return False
        left = self.n - keep_from
        self._load(self.pos + keep_from, max(2 * left, int(budget * self.ratio * 1.25) + (128 << 10)))
        if self.n <= left:
            raise ValueError("a deflate block or a gzip header of more than %d bytes at file offset %d" % (left, self.pos))
        return True

    def _header(self, buf, at, end, at_eof):
        """The gzip member header at slab byte ``at``: -> the byte its deflate data starts at, or None: not all there.
        What Python's gzip module refuses is refused with its exception."""
        import gzip

        def short():
            if at_eof:
                raise EOFError("Compressed file ended before the end-of-stream marker was reached")

        if end - at < 2:
            if at_eof:
                raise gzip.BadGzipFile("Not a gzipped file (%r)" % bytes(buf[at:end]))
            return None
        if buf[at] != 0x1f or buf[at + 1] != 0x8b:
            raise gzip.BadGzipFile("Not a gzipped file (%r) at file offset %d " % (bytes(buf[at:at + 2]), self.pos + at))
        if end - at < 10:
            return short()
        if buf[at + 2] != 8:
            raise gzip.BadGzipFile("Unknown compression method at file offset %d " % (self.pos + at))
        flags, p = int(buf[at + 3]), at + 10
        if flags & 4:                                         # FEXTRA
            if end - p < 2:
                return short()
            p += 2 + int(buf[p]) + 256 * int(buf[p + 1])
        for bit in (8, 16):                                   # FNAME, FCOMMENT: zero-terminated
            if flags & bit:
                while p < end and buf[p]:
                    p += 1
                p += 1
        if flags & 2:                                         # FHCRC
            p += 2
        return p if p <= end else short()

    def prepare(self, carry):
        """The next chunk: [carried-over text | text of the members' blocks, as much as the chunk takes]."""
        try:
            self.pending = _settled(self._inflate(carry))
        except Exception as e:                                # noqa: BLE001 (raised when this chunk is asked for)
            self.pending = _settled(error=e)
        return self

    def _inflate(self, carry):
        import gzip
        import zlib
        io, be = self.io, self.io.be
        n0 = carry[2] - carry[1] if carry else 0
        budget = max(io.chunk_bytes - n0, io.chunk_bytes // 4)
        data = be.empty(((n0 + budget + 15) // 16 * 16 + 32,), torch.uint8)
        if n0:
            data[:n0].copy_(carry[0][carry[1]:carry[2]])
        filled = 0
        buf = io.buf[0].numpy()
        while not self.done and filled < budget:
            t0 = time.perf_counter()
            at_eof = self.pos + self.n >= io.size
            if self.member is None:                           # between members: zero padding, the end, or a header
                while self.at < self.n and buf[self.at] == 0 and self.pos + self.at > 0:
                    self.at += 1
                if self.at >= self.n:
                    if at_eof:
                        self.done = True
                        break
                    self._load(self.pos + self.at, int(budget * self.ratio * 1.25) + (128 << 10))
                    io.clock.add("wait_file_read", t0)
                    continue
                start = self._header(buf, self.at, self.n, at_eof)
                if start is None:
                    self._more(self.at, budget)
                    io.clock.add("wait_file_read", t0)
                    continue
                self.member, self.bit = self.pos + self.at, 8 * start
                self.crc = self.isize = self.wlen = 0
            if self.dev is None:
                self.dev = io.to_device(io.buf[0], self.n)
            io.clock.add("wait_file_read", t0)
            byte = self.bit // 8
            room = budget - filled
            need = be.gunzip_stream_workspace(self.n - byte, self.spacing, room)
            if self.work is None or self.work.numel() < need:
                self.work = be.empty((need,), torch.uint8)
            res = be.gunzip_stream(self.dev[byte:], self.n - byte, self.bit - 8 * byte, self.window, self.wlen, self.crc,
                                   data[n0 + filled:], room, self.spacing, work=self.work)
            status, end_bit, got, final, crc = res.cpu().tolist()[:5]   # (the next call's first bit: the one wait of a call)
            if status == _lib.GUNZIP_NEED_INPUT:
                if not self._more(byte, budget):
                    raise EOFError("Compressed file ended before the end-of-stream marker was reached")
                continue
            if status == _lib.GUNZIP_NEED_ROOM:
                if filled:
                    break                                     # (the next chunk has all its room for this block)
                budget *= 2                                   # a block of more text than a chunk: this chunk grows
                grown = be.empty(((n0 + budget + 15) // 16 * 16 + 32,), torch.uint8)
                grown[:n0].copy_(data[:n0])
                data = grown
                continue
            if status:                                        # (what the host road's decompressor raises for bad deflate data)
                raise zlib.error("Error -3 while decompressing data: the gzip member at file offset %d breaks rule %d of "
                                 "inflate_core.hpp" % (self.member, status))
            if got:
                lo = n0 + filled
                if got >= 32768:
                    self.window.copy_(data[lo + got - 32768:lo + got])
                    self.wlen = 32768
                else:
                    both = torch.cat([self.window[:self.wlen], data[lo:lo + got]])[-32768:]
                    self.wlen = both.numel()
                    self.window[:self.wlen].copy_(both)
                self.ratio = max(end_bit / 8.0 / got, 0.001)
            filled += got
            self.crc, self.isize = crc, (self.isize + got) & 0xffffffff
            self.bit = 8 * byte + end_bit
            if not final:
                # the slab ended inside a block, or the next block's text does not fit: the next call says which, at
                # the price of decoding the rest of the slab once more -- so a chunk that is half full ends here
                if got < room and 2 * filled >= budget:
                    break
                if got < room and self.pos + self.n < io.size:
                    self._more(self.bit // 8, budget)
                continue
            trailer = (self.bit + 7) // 8
            if trailer + 8 > self.n:
                if not self._more(self.bit // 8, budget):
                    raise EOFError("Compressed file ended before the end-of-stream marker was reached")
                trailer = (self.bit + 7) // 8
                if trailer + 8 > self.n:
                    raise EOFError("Compressed file ended before the end-of-stream marker was reached")
            want_crc, want_size = struct.unpack("<II", bytes(buf[trailer:trailer + 8]))
            if want_crc != self.crc:
                raise gzip.BadGzipFile("CRC check failed for the gzip member at file offset %d (%#x != %#x)" % (self.member, want_crc, self.crc))
            if want_size != self.isize:
                raise gzip.BadGzipFile("Incorrect length of data produced by the gzip member at file offset %d " % self.member)
            self.member, self.at = None, trailer + 8
        nbytes = n0 + filled
        data[nbytes:nbytes + 32].zero_()
        return Chunk(data[:(nbytes + 15) // 16 * 16 + 16], nbytes, self.done, None, False, None, ())

    def take(self, chunk):
        self.chunk = _end_last_line_on_device(self.io, chunk, self.lines)
        return self.chunk


# ---- decoders: a chunk -> (the batch of its whole records, the bytes of the chunk they take)
class _TextDecoder(object):
    """FASTQ or FASTA text; the first chunk decides a format that neither the caller nor the file's name gave."""

    lines = True

    def __init__(self, fmt, byte_range, backend):
        self.fmt, self.byte_range, self.be = fmt, byte_range, backend

    def __call__(self, chunk):
        if self.fmt is None:
            n = min(chunk.nbytes, 1 << 16)
            head = chunk.host[:n] if chunk.host is not None else chunk.data[:n].cpu()
            self.fmt = sniff_format(head.numpy().tobytes())
            if self.fmt == "fasta" and self.byte_range:
                raise NotImplementedError("a byte range of FASTA input is not provided")
        cls = FastaBatch if self.fmt == "fasta" else FastqBatch
        return cls.from_device(chunk.data, chunk.nbytes, chunk.final, self.be, unterminated=chunk.unterminated)


class _BamDecoder(object):
    """Unaligned BAM over the chunks of a ``_BgzfSource``, which then hold BAM bytes: the header, parsed once on the
    host, is skipped, the records are found by ``bam_walk`` and decoded to FASTQ text by ``bam_to_fastq`` (DESIGN
    3.8i), and the batch is ``FastqBatch.from_device`` over that text.  ``consumed`` and the carry are BAM bytes.
    ``paired``: records 2i and 2i + 1 are the reads of a pair (one name, read 1 / read 2 flags, read 2 first is
    swapped); a chunk's last record without partner waits in the carry, the file's is dropped.  A record the reference
    fails on is a ``FormatError`` naming its number in the file and its name."""

    fmt = "bam"
    lines = False

    def __init__(self, io, paired):
        self.be, self.paired = io.be, paired
        self.skip, self.n_ref = self._header(io)              # header bytes not yet passed; references of the header
        self.records = 0                                      # records handed out so far (error messages count from 1)

    def _header(self, io):
        """The header, inflated from the file's first members with zlib and parsed (``bam_header``): its bytes are
        skipped in the chunks that hold them (it may be longer than a chunk)."""
        import gzip
        import zlib
        text, pos, need = b"", 0, 12
        while True:
            raw = os.pread(io.fd, 1 << 20, pos)
            head = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else None
            m_at, _, k, covered, ok = self.be.bgzf_scan(head, 0, len(raw), io.limits.BGZF_SCAN) if raw else (None, None, 0, 0, True)
            if not k:
                if not ok:
                    raise gzip.BadGzipFile("not a BGZF member at file offset %d (BAM is a BGZF stream)" % pos)
                raise FormatError("the BAM file ends inside its header" if text else "not a BAM file: no BGZF member")
            at = [int(v) for v in m_at[:k + 1].tolist()]
            for m in range(k):
                try:
                    text += zlib.decompress(raw[at[m]:at[m + 1]], 31)
                except zlib.error as exc:
                    raise gzip.BadGzipFile("BGZF member at file offset %d fails its checks (%s)" % (pos + at[m], exc))
                if len(text) >= 8 and need == 12:
                    if text[:4] != b"BAM\1":
                        raise FormatError("not a BAM file: it begins with %r" % text[:4])
                    need = 12 + max(int.from_bytes(text[4:8], "little", signed=True), 0)
                if len(text) < need:
                    continue
                try:
                    parsed = self.be.bam_header(text)
                except ValueError:
                    raise FormatError("not a BAM file: its header is malformed")
                if parsed is not None:
                    return parsed
            pos += covered

    def _name(self, data, at, nbytes):
        at = int(at)
        if at + 36 > nbytes:
            return "?"
        end = min(at + 36 + max(int(data[at + 12].item()) - 1, 0), nbytes)
        return _text(bytes(data[at + 36:end].cpu().numpy().tobytes()))

    def __call__(self, chunk):
        """Walk + decode of a chunk of BAM bytes: the batch over the decoded FASTQ text, and the BAM bytes consumed."""
        be, data, nbytes = self.be, chunk.data, chunk.nbytes
        entry = min(self.skip, nbytes)
        self.skip -= entry
        if self.skip and chunk.final:
            raise FormatError("the BAM file ends inside its header")
        starts, result = be.bam_walk(data, nbytes, entry, self.n_ref, chunk.final)
        count, consumed, err, _repaired = (int(v) for v in result.cpu().tolist())
        if err != _lib.INT64_MAX:
            at, kind = err // 8, err % 8
            what = {_lib.BAM_ERR_SMALL: "its block_size is smaller than its own fields need",
                    _lib.BAM_ERR_BIG: "its block_size is above %d" % _lib.BAM_MAX_BLOCK,
                    _lib.BAM_ERR_LSEQ: "its l_seq is negative",
                    _lib.BAM_ERR_TRUNCATED: "the file ends inside it"}[kind]
            name = "?" if kind in (_lib.BAM_ERR_SMALL, _lib.BAM_ERR_BIG) else self._name(data, at, nbytes)
            raise FormatError("BAM record %d (%r): %s" % (self.records + count + 1, name, what))
        if self.paired and count % 2:
            count -= 1                                        # the file's last record without partner is dropped (zip(sam, sam))
            if not chunk.final:
                consumed = int(starts[count].item()) & 0xFFFFFFFF     # (a chunk's: it waits for its partner in the carry)
        text, total, used, err, _ = be.bam_to_fastq(data, nbytes, starts, count, self.paired)
        if err != _lib.INT64_MAX:
            j, kind = err // 8, err % 8
            number = self.records + j + 1
            name = self._name(data, int(starts[j].item()) & 0xFFFFFFFF, nbytes)
            if kind == _lib.BAM_REC_PAIR_NAME:                # io/seqio.py:627-632
                other = self._name(data, int(starts[j + 1].item()) & 0xFFFFFFFF, nbytes)
                raise FormatError("BAM records %d and %d: Consecutive reads %s, %s in paired-end SAM/BAM file do not have the same "
                                  "name; make sure your file is name-sorted and does not contain any secondary/supplementary "
                                  "alignments." % (number, number + 1, name, other))
            what = {_lib.BAM_REC_LSEQ0: "it has no sequence", _lib.BAM_REC_QUAL: "it has no qualities, or one above 93",
                    _lib.BAM_REC_NAME: "its name holds a line end, or it has none",
                    _lib.BAM_REC_PAIR_FLAGS: "it and the record behind it are not flagged as read 1 and read 2 of a pair"}[kind]
            raise FormatError("BAM record %d (%r): %s" % (number, name, what))
        self.records += used
        return FastqBatch.from_device(text, total, True, be)[0], consumed


class ChunkedFastqReader(object):
    """Feeds a FASTQ, FASTA or unaligned BAM file to the GPU in chunks of whole records.  The file is read straight into
    page-locked staging buffers (``IO_THREADS`` ``pread`` slices per chunk, no intermediate bytes objects).

    The reader picks a SOURCE, which puts the chunks together, and a DECODER, which makes the batch of a chunk's whole
    records; ``_ChunkIO`` holds what the sources share.  The sources, by the file's name and ``device_gunzip``:

    ``_PlainSource``: plain files, read ``READ_AHEAD`` chunks ahead of the carry.  ``byte_range`` = (lo, hi): only
    these bytes, which must be whole records (a rank's shard, ``shard.fastq_shard_ranges``).

    ``_DecompressedSource``: ``.gz`` / ``.bz2`` / ``.xz`` through a host decompressor thread.

    ``_BgzfSource``: ``device_gunzip=True`` and a ``.gz`` file whose first member is BGZF: the compressed slabs are read
    ahead and inflated on the device; the text never visits the host.  The flag wants BGZF throughout: a later member
    that is not BGZF, or one that fails its checks, is a ``gzip.BadGzipFile`` naming the member's file offset; a file
    that ends inside a member is an ``EOFError``.

    ``_GzipStreamSource``: ``device_gunzip="any"``: every other ``.gz`` member -- an ordinary gzip file, and an ordinary
    member behind BGZF ones, which ``True`` refuses: there the BGZF source hands the rest of the file over to a stream
    source -- is inflated on the device as well.

    ``inflate_path`` says which source a reader STARTED with: "device" (BGZF), "stream", "host" (any other ``.gz``), or
    None.

    The decoders: ``_TextDecoder`` (FASTQ / FASTA; ``fmt`` is None until the first chunk has been sniffed, where neither
    the caller nor the name says it) and ``_BamDecoder`` (``fmt == "bam"``: a name ending in ``.bam``, or
    ``input_format="bam"``), which always sits on a ``_BgzfSource``, whatever ``device_gunzip`` says; ``paired`` tells
    it that records 2i and 2i + 1 are the reads of a pair.

    The loop that drives a reader -- ``next_batch``, ``advance``, ``close``, and two readers in lock step -- is
    ``read_chunks``; nothing else constructs one."""

    READ_AHEAD = 3
    RESERVE = 64 << 20                                       # room for the carried-over tail of the previous chunk

    BGZF_SCAN = 4096                                         # members per bgzf_scan call

    # compressed bytes per speculative start (atr_gunzip_stream): the one serial wave resolves 32 KiB of text per
    # confirmed chunk, so a chunk should hold many times that; 128 KiB is some 300 - 600 KB of FASTQ
    STREAM_SPACING = 131072

    def __init__(self, path, chunk_bytes, backend=None, clock=None, byte_range=None, device_gunzip=False, input_format=None,
                 paired=False):
        name = str(path)
        # "fasta" | "fastq" | "bam": given, else by the file's name, else (None until the first chunk is there) by its
        # first byte
        fmt = input_format if input_format is not None else file_format(name)
        if fmt not in ("fasta", "fastq", "bam", None):
            raise ValueError("input_format must be 'fasta', 'fastq' or 'bam'")
        if fmt == "fasta" and byte_range is not None:
            raise NotImplementedError("a byte range of FASTA input is not provided")
        if fmt == "bam" and byte_range is not None:
            raise NotImplementedError("a byte range of BAM input is not provided")
        self.paired = bool(paired)                            # (BAM: records 2i, 2i + 1 are decoded as the reads of a pair)
        if byte_range is not None and _codec(name):
            raise ValueError("a byte range of compressed input: the offsets are those of the plain text")
        be = backend or _lib.get_backend()
        self.clock = clock or StageClock()
        self.nbytes, self.final = 0, False
        self.source = self.decoder = None
        io = self.io = _ChunkIO(path, be, self.clock, int(chunk_bytes), self)
        try:                                                  # (nobody else holds the file, the thread pools and the buffers yet)
            self.decoder = _BamDecoder(io, self.paired) if fmt == "bam" else _TextDecoder(fmt, byte_range, be)
            lines, gz = self.decoder.lines, name.endswith(".gz")
            # BAM is BGZF by definition and always takes the device road: device_gunzip is about .gz
            if fmt == "bam" or (device_gunzip and gz and io.starts_with_bgzf()):
                source = _BgzfSource(io, lines, device_gunzip == "any" and fmt != "bam")
            elif device_gunzip == "any" and gz:
                source = _GzipStreamSource(io, lines, 0, 1.0)
            elif _codec(name):
                source = _DecompressedSource(io, lines, open_compressed(name, io.file), "host" if gz else None)
            else:
                source = _PlainSource(io, lines, byte_range)
            self.inflate_path = source.inflate_path
            self.source = source.prepare(None)
        except BaseException:
            self.close()
            raise

    fmt = property(lambda self: self.decoder.fmt)
    buf = property(lambda self: self.io.buf)                 # the staging buffers; [] after close
    file = property(lambda self: self.io.file)

    def next_batch(self):
        """Upload and index the next chunk; returns the FastqBatch (FastaBatch) of its whole records."""
        t0 = time.perf_counter()
        chunk = self.source.pending.result()                  # (raises what was met while it was put together)
        self.clock.add("wait_file_read", t0)                  # the decompressor thread's chunk; every other is there already
        t0 = time.perf_counter()
        chunk = self.source.take(chunk)
        self.nbytes, self.final = chunk.nbytes, chunk.final
        batch, self.consumed = self.decoder(chunk)
        self.clock.add("upload_and_index", t0)
        return batch

    def advance(self, consumed=None):
        """The caller took ``consumed`` bytes of the current chunk (default: all whole records);
        the rest is carried over and the next chunk is put together (plain files: its bytes are in the staging
        buffer already, its upload starts here).  Returns True when the file is exhausted and nothing is
        carried over."""
        source = self.source.advance(self.consumed if consumed is None else consumed)
        self.source = source or self.source                   # (an ordinary member behind BGZF ones: another source goes on)
        return source is None

    def close(self):
        if self.source is not None:
            self.source.close()
        self.io.close()


def read_chunks(paths, chunk_bytes, backend=None, clock=None, byte_ranges=None, device_gunzip=False, interleaved=False,
                input_formats=None):
    """THE chunk loop of every file driver (trim, qc, error rate, detect, a rank's shard): yields a list of
    FastqBatch, one per path, chunk after chunk of whole records.  Several paths are read in lock step: every
    batch of a list holds the same number of records (the file whose chunk holds fewer decides, the surplus of the
    others is carried over), and files that do not hold the same number of records are a ValueError.

    The next chunk is put together, and its upload started, BEFORE a chunk is handed out: that copy runs while the
    consumer works.  A chunk may hold no whole record; it is yielded all the same.  The readers are closed when the
    loop ends, however it ends -- a consumer that has enough just leaves its ``for`` loop.  ``byte_ranges``: one
    (lo, hi) or None per path (``ChunkedFastqReader``).  ``device_gunzip``: BGZF ``.gz`` input (``True``), or any ``.gz`` input (``"any"``), is inflated on the GPU
    (``ChunkedFastqReader``); every other input is read as without it.

    ``interleaved``: the one path holds pairs, read 1 and read 2 in turn (the reference's ``-l``): every list holds TWO
    batches, the even and the odd records of the chunk (``FastqBatch.mates``: one ``data`` tensor).  A chunk with an
    odd number of records hands out all but the last, which is carried over like the surplus of a two-file run; an
    odd number of records in the whole file is the reference's FormatError (io/seqio.py:499-502).  The names of the
    two reads are not compared -- the two-file readers do not compare them either.  With ``byte_ranges`` it is a
    ValueError: a range may begin at a read 2.

    ``input_formats``: "fasta" | "fastq" | "bam" | None per path; None is the file's name, else its first byte
    (``input_format``).  FASTA paths yield ``FastaBatch``es; two paths of different formats are a ValueError, FASTA with
    ``byte_ranges`` or ``interleaved`` a NotImplementedError.  A BAM path yields ``FastqBatch``es over the decoded text;
    with ``interleaved`` the reader pairs the records itself (names and flags are checked, a last record without partner is
    dropped: ``PairedEndSAMReader``); two BAM paths and BAM with ``byte_ranges`` are a NotImplementedError."""
    mismatch = "the two input files hold different numbers of records"
    if interleaved:
        if len(paths) != 1:
            raise ValueError("interleaved input is one file")
        if byte_ranges is not None and any(r is not None for r in byte_ranges):
            raise ValueError("byte ranges of an interleaved file are not provided (a range may begin at a read 2)")
    readers = []
    try:
        for path, byte_range, fmt in zip(paths, byte_ranges or [None] * len(paths), input_formats or [None] * len(paths)):
            readers.append(ChunkedFastqReader(path, chunk_bytes, backend, clock, byte_range, device_gunzip, fmt, interleaved))
        if len(readers) > 1 and all(r.fmt == "bam" for r in readers):
            raise NotImplementedError("two BAM files as the reads of a pair are not provided: one name-sorted BAM file "
                                      "holds both (interleaved)")
        while True:
            batches = [r.next_batch() for r in readers]
            if len({r.fmt for r in readers}) > 1:
                raise ValueError("the two input files are of different formats (%s)" % " and ".join(r.fmt for r in readers))
            if interleaved and readers[0].fmt == "fasta":
                raise NotImplementedError("interleaved FASTA input is not provided")
            if interleaved:
                reader, batch = readers[0], batches[0]
                if len(batch) % 2:
                    if reader.final:
                        raise FormatError("Interleaved input file incomplete: Last record has no partner.")
                    batch, consumed = batch.head(len(batch) - 1)
                    done = [reader.advance(consumed)]
                else:
                    done = [reader.advance()]
                batches = batch.mates()
            elif len(readers) == 1:
                done = [readers[0].advance()]                 # (all whole records: no head(), no device sync)
            else:
                nrec = min(len(b) for b in batches)
                heads = [b.head(nrec) for b in batches]
                done = [r.advance(h[1]) for r, h in zip(readers, heads)]
                if all(r.final for r in readers) and any(len(b) != nrec for b in batches):
                    raise ValueError(mismatch)
                batches = [h[0] for h in heads]
            yield batches
            if all(done):
                return
            if any(done):
                raise ValueError(mismatch)
    finally:
        for r in readers:
            r.close()


class FastqSink(object):
    """Writes device text to a file through three page-locked buffers.  ``write`` only queues: the
    device -> host copy runs on its own stream behind an event (the caller's stream goes on with the
    next chunk) and a writer thread puts the buffer into the file once the copy has landed -- in
    order, one ``pwrite`` at a time (writes to one file are serialised by the kernel anyway).

    Every ``pwrite`` covers whole 4 KiB blocks of a block-aligned staging buffer at a block-aligned
    offset; the odd bytes at the end of a chunk are carried to the front of the next buffer (the next
    device -> host copy lands right behind them) and the last few go out in ``close``.  That makes
    ``direct=True`` (O_DIRECT, page-cache bypass) possible where the file system allows it -- off by
    default: a lone 1 GB ``pwrite`` into a new file runs at 14 GB/s that way against 6-7 GB/s through the
    page cache on the measured host, but inside the pipeline the synchronous direct writes were no faster
    than the buffered ones (110 vs 100 ms per 4 M reads) and slower than overwriting in place.
    ``keep``: do not truncate an existing file first (overwriting cached pages is about twice as fast as
    allocating new ones); the file is cut to the written length at the end."""

    BLOCK = 4096

    WRITERS = 1                                               # threads a buffer's pwrite is split over (set_writers)

    @classmethod
    def set_writers(cls, n):
        """Split every buffer's ``pwrite`` into n block-aligned ranges written by n threads (one file, disjoint
        ranges: pays where the file system does not serialise writers of one file -- tools/micro/write_parts.py)."""
        cls.WRITERS = max(1, int(n))

    def __init__(self, path, capacity, backend=None, clock=None, keep=False, direct=False, nbuf=3):
        be = backend or _lib.get_backend()
        self.clock = clock or StageClock()
        self.gpu = getattr(be, "name", "") == "hip"
        self.path = path
        self.nbuf = max(2, int(nbuf))
        self.buf = [_staging(capacity + self.BLOCK, self.gpu) for _ in range(self.nbuf)]
        flags = os.O_WRONLY | os.O_CREAT | (0 if keep else os.O_TRUNC)
        self.direct = False
        self.fd = -1
        if direct and hasattr(os, "O_DIRECT") and all(t.data_ptr() % self.BLOCK == 0 for t in self.buf):
            try:
                self.fd = os.open(path, flags | os.O_DIRECT, 0o644)
                self.direct = True
            except OSError:
                self.fd = -1
        if self.fd < 0:
            self.fd = os.open(path, flags, 0o644)
        self.offset = 0                                       # bytes handed to pwrite so far (a multiple of BLOCK)
        self.rem = 0                                          # carried bytes at the front of the next buffer
        self.pool = ThreadPoolExecutor(1)
        self.writers = int(self.WRITERS)                      # (fixed for this sink's life: set_writers() applies to later sinks)
        self.wpool = ThreadPoolExecutor(self.writers - 1) if self.writers > 1 else None
        self.pending = [None] * self.nbuf
        self.k = 0
        self.copy_stream = torch.cuda.Stream(device=be.device) if self.gpu else None

    def _put(self, k, rem, n, offset, done, text):
        if done is not None:
            done.synchronize()                                # the device -> host copy has landed
        del text
        host = self.buf[k]
        total = rem + n
        whole = total - total % self.BLOCK
        view = memoryview(host.numpy())
        at = 0
        if self.wpool is not None and not self.direct and whole >= (16 << 20):
            # disjoint block-aligned ranges of the same buffer and file, one thread each
            per = (whole // self.writers) // self.BLOCK * self.BLOCK

            def piece(lo, hi):
                while lo < hi:
                    lo += os.pwrite(self.fd, view[lo:hi], offset + lo)
            jobs = [self.wpool.submit(piece, i * per, (i + 1) * per) for i in range(1, self.writers - 1)]
            jobs.append(self.wpool.submit(piece, (self.writers - 1) * per, whole))
            piece(0, per)
            for job in jobs:
                job.result()
            at = whole
        while at < whole:
            try:
                at += os.pwrite(self.fd, view[at:whole], offset + at)
            except OSError:
                if not self.direct:
                    raise
                os.close(self.fd)                             # the file system refused the direct write: go on buffered
                self.fd = os.open(self.path, os.O_WRONLY)
                self.direct = False
        if total > whole:                                     # the odd bytes travel to the front of the next buffer
            self.buf[(k + 1) % self.nbuf][:total - whole].copy_(host[whole:total])

    def write(self, text):
        n = int(text.numel())
        room = self.buf[self.k].numel() - self.BLOCK           # (a staging buffer also holds up to BLOCK - 1 carried bytes)
        if n > room:
            # text that outgrew its chunk (read-name prefixes / suffixes / length tags on short records): in pieces
            for lo in range(0, n, room):
                self.write(text[lo:lo + room])
            return
        t0 = time.perf_counter()
        if self.pending[self.k] is not None:
            self.pending[self.k].result()                     # this buffer is free again after its write
        self.clock.add("wait_file_write", t0)
        rem = self.rem
        if rem + n > self.buf[self.k].numel():
            raise ValueError("FastqSink: a chunk of %d bytes does not fit the staging buffers" % n)
        host = self.buf[self.k]
        done = None
        if self.gpu and n:
            ready = torch.cuda.Event()
            ready.record()                                    # the text is complete on the caller's stream here
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                host[rem:rem + n].copy_(text, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
            text.record_stream(self.copy_stream)
        elif n:
            host[rem:rem + n].copy_(text)
        self.pending[self.k] = self.pool.submit(self._put, self.k, rem, n, self.offset, done, text)
        total = rem + n
        self.offset += total - total % self.BLOCK
        self.rem = total % self.BLOCK
        self.k = (self.k + 1) % self.nbuf

    def close(self):
        t0 = time.perf_counter()
        try:
            for job in self.pending:
                if job is not None:
                    job.result()
            if self.rem:                                      # the last odd bytes: an ordinary write
                tail = bytes(self.buf[self.k][:self.rem].numpy().tobytes())
                fd = os.open(self.path, os.O_WRONLY) if self.direct else self.fd
                try:
                    os.pwrite(fd, tail, self.offset)
                finally:
                    if self.direct:
                        os.close(fd)
        finally:
            self.clock.add("wait_file_write", t0)
            self.pool.shutdown()
            if self.wpool is not None:
                self.wpool.shutdown()
            os.ftruncate(self.fd, self.offset + self.rem)
            os.close(self.fd)
            _release(self.buf)
            self.buf = []


class PartSink(object):
    """The output as N part files ``<path>.part0 .. <path>.part<N-1>``, one ``FastqSink`` -- writer thread, staging
    buffers, file -- each: chunk k of the stream goes to part k mod N, records keep their order inside a part.
    Ordering contract: the parts concatenated are NOT the input order; part i holds the chunks i, i + N, i + 2N, ...
    of the stream in that order (an empty chunk is written as nothing and still takes its turn).
    For hosts whose file system serialises the writers of ONE file (measured on the MI355X box: 11.8 GB/s into a
    fresh file from one thread or from eight, 75 GB/s into eight files; putting the parts together again by
    copy_file_range costs as much as writing them, tools/micro/write_parts.py).  What the reference's
    ``--no-writer-process`` does with its worker processes: every worker writes a file of its own."""

    def __init__(self, path, parts, capacity, backend=None, clock=None, keep=False):
        # parts of an earlier run with more of them must not survive next to this run's (`out.part*` would mix them in)
        import glob
        import re
        for old in glob.glob(glob.escape(str(path)) + ".part*"):
            tail = old[len(str(path)) + 5:]
            if re.fullmatch(r"[0-9]+", tail) and int(tail) >= int(parts):
                os.unlink(old)
        self.paths = ["%s.part%d" % (path, i) for i in range(int(parts))]
        self.sinks = [FastqSink(p, capacity, backend, clock, keep=keep, nbuf=2) for p in self.paths]
        self.k = 0

    def write(self, text):
        self.sinks[self.k % len(self.sinks)].write(text)
        self.k += 1

    def close(self):
        first = None
        for s in self.sinks:
            try:
                s.close()
            except Exception as exc:                          # close every part, report the first failure
                first = first or exc
        if first is not None:
            raise first


class CompressedSink(object):
    """The output through a host compressor (``.gz`` / ``.bz2`` / ``.xz`` by extension, as the reference's xopen):
    a writer thread takes the chunks in order, so that the GPU goes on with the next chunk while one is compressed.
    One host thread compresses -- it sets the pace of the whole run.  This is the default for every compressed
    output, and the only path for ``.bz2`` / ``.xz``, side files and demultiplexed outputs; for the main ``.gz``
    outputs ``make_sink(..., device_gzip=True)`` compresses on the GPU instead (``DeviceGzipSink``)."""

    def __init__(self, path, clock=None):
        self.fh = open_by_extension(path)
        self.clock = clock or StageClock()
        self.writer = ThreadPoolExecutor(1)
        self.pending = []

    def write(self, text):
        t0 = time.perf_counter()
        while len(self.pending) > 2:                          # (bounded: at most three chunks in flight)
            self.pending.pop(0).result()
        self.clock.add("wait_file_write", t0)
        host = text.cpu() if torch.is_tensor(text) else text  # the device -> host copy, then the compressor's turn
        self.pending.append(self.writer.submit(lambda h: self.fh.write(bytes(h.numpy().tobytes()) if torch.is_tensor(h) else h), host))

    def close(self):
        try:
            for job in self.pending:
                job.result()
        finally:
            self.writer.shutdown()
            self.fh.close()


class DeviceGzipSink(object):
    """``.gz`` output compressed on the device: every chunk of text becomes a stream of BGZF members
    (``backend.gzip_blocks``: a gzip member per 65 280 bytes, dynamic Huffman over an LZ77 parse) on the caller's
    stream, and the compressed tensor -- a half to a quarter of the text -- goes the way plain text goes: the
    ``FastqSink`` machinery (page-locked staging buffers, copy stream, writer thread).  ``write`` reads the
    compressed length, so the text has been consumed when it returns; the compressed tensor is kept alive by
    the sink until its copy has landed.  An empty chunk writes nothing; ``close`` appends the 28-byte BGZF
    end-of-file member, which alone is the file of a run that keeps no read.  The file's bytes depend on the
    text and on where the chunks end, not on time or scheduling; decompressed it is the plain file."""

    def __init__(self, path, capacity, backend=None, clock=None, keep=False):
        self.be = backend or _lib.get_backend()
        # compressed text is rarely more than half the text; what is goes out in pieces (FastqSink.write)
        self.sink = FastqSink(path, int(capacity) // 2 + (1 << 20), self.be, clock, keep=keep)

    def write(self, text):
        if not int(text.numel()):
            return
        stream, total = self.be.gzip_blocks(text)
        self.sink.write(stream[:total])

    def close(self):
        try:
            eof = torch.frombuffer(bytearray(_lib.GZIP_EOF), dtype=torch.uint8)
            self.sink.write(eof.to(self.be.device))
        finally:
            self.sink.close()


def open_by_extension(path):
    """A binary file object for writing; ``.gz`` / ``.bz2`` / ``.xz`` compress (the reference's xopen does so for EVERY
    output, the side files -- too-short, untrimmed, info, rest, wildcard -- included)."""
    mod = _codec(path)
    if mod is None:
        return open(str(path), "wb")
    return mod.open(str(path), "wb", **(dict(compresslevel=6) if mod.__name__ == "gzip" else {}))


def make_sink(path, parts, capacity, backend=None, clock=None, keep=False, device_gzip=False):
    """One file, or ``parts`` > 1 part files (PartSink); a compressed file by its extension (CompressedSink).
    ``device_gzip``: a ``.gz`` file compressed on the GPU (DeviceGzipSink); any other path is a ValueError with it."""
    if device_gzip:
        if not str(path).endswith(".gz"):
            raise ValueError("device_gzip: the output path must end in .gz (%r)" % str(path))
        if parts and int(parts) > 1:
            raise ValueError("part files of a compressed output are not provided")
        return DeviceGzipSink(path, capacity, backend, clock, keep)
    if str(path).endswith((".gz", ".bz2", ".xz")):
        if parts and int(parts) > 1:
            raise ValueError("part files of a compressed output are not provided")
        return CompressedSink(path, clock)
    if parts and int(parts) > 1:
        return PartSink(path, parts, capacity, backend, clock, keep)
    return FastqSink(path, capacity, backend, clock, keep=keep)

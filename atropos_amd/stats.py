"""Read statistics on the GPU: the device twin of the reference's ``atropos.commands.stats`` (``atropos qc``,
``atropos trim --stats pre|post|both``) and of ``BaseQualityErrorEstimator`` (``atropos error -a quality``).

The reference counts one dict entry per base and per quality character (``ReadStatistics.collect_record``,
commands/stats.py:194-255).  Here a FASTQ chunk that is already in device memory (``FastqBatch``, or the kept
intervals of a ``TrimResult``) is histogrammed by ``atr_read_stats_batch`` into a block of uint64 counters that
stays on the device across chunks; the host copies the block once and derives the summary (mean, stdev, median,
modes over a few hundred bins) from it.

The reference's histograms are dicts in the order values were first seen, and its ``median`` (a weighted median
walked in that order) and the float sum of ``stdev`` follow it.  The kernels keep,
for every bin, the stream index of the first read that landed in it, so the summary walks the bins in the
reference's order.  The one remaining difference: the non-ACGTN columns of ``bases`` (a set's iteration order in
the reference, which varies between runs) are sorted.  Tile statistics are not supported (out of scope).
"""
import math

import numpy as np
import torch

from . import _lib
from .fastq import FastqBatch, read_chunks

HDR = 8                                     # stats_core.hpp
COUNT, LONGEST, WITHQ, SKIPPED = range(4)
GC_BINS, MQ_BINS = 101, 256


def layout(cap):
    """Word offsets of the block sections for a capacity of ``cap`` positions (stats_core.hpp)."""
    gc = HDR + cap + 1
    mq = gc + GC_BINS
    seq = mq + MQ_BINS
    qual = seq + 256 * cap
    first = qual + 256 * cap
    return dict(len=HDR, gc=gc, mq=mq, seq=seq, qual=qual, first=first, words=first + cap + 1 + GC_BINS + MQ_BINS)


def div_round_even(num, den):
    """Python's ``round(num / den)`` in integers (half to even, floor division for a negative ``num``): the rule
    the kernels apply to GC% and mean quality (stats_core.hpp, st_div_round_even)."""
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    return q


# ---------------------------------------------------------------------------------------------- summaries
def hist_summary(hist, first=None):
    """``Histogram.summarize()`` (util/__init__.py:328-347) of {value: count} (counts > 0).  ``first``: {value: index
    of the first read with it}; the statistics walk the values in that order, as the reference walks its dict
    (default: ascending values)."""
    if not hist:
        raise ValueError("Cannot summarize an empty histogram")
    values = sorted(hist, key=(lambda v: first[v]) if first is not None else None)
    counts = [hist[v] for v in values]
    total = sum(counts)
    mean = sum(v * c for v, c in zip(values, counts)) / total
    if len(values) == 1:
        stdev, modes = 0, [values[0]]
    else:
        stdev = math.sqrt(sum(((v - mean) ** 2) * c for v, c in zip(values, counts)) / total)
        top = max(counts)
        modes = sorted(v for v, c in zip(values, counts) if c == top)
    # weighted median over the values in that order: the mean of the values where the running count reaches
    # total // 2 + 1 and (total + 1) // 2
    mid2 = total // 2 + 1
    mid1 = mid2 - 1 if total % 2 == 0 else mid2
    cum, val1, val2 = 0, None, None
    for v, c in zip(values, counts):
        cum += c
        if val1 is None and mid1 <= cum:
            val1 = v
        if mid2 <= cum:
            val2 = v
            break
    median = float(val1 + val2) / 2
    return dict(hist={v: hist[v] for v in sorted(values)},
                summary=dict(mean=mean, stdev=stdev, median=median, modes=modes))


def _table_summary(table, is_qualities, quality_base):
    """``BaseCountingDicts.summarize()`` (commands/stats.py:51-79) of a [positions, 256] count table."""
    used = [b for b in range(256) if table[:, b].any()] if table.shape[0] else []
    if is_qualities:
        keys = used
        columns = tuple(b - quality_base for b in keys)
    else:
        acgtn = [ord(c) for c in "ACGTN"]
        keys = acgtn[:4] + [b for b in used if b not in acgtn] + acgtn[4:]
        columns = tuple(chr(b) for b in keys)
    sub = table[:, keys] if keys else np.zeros((table.shape[0], 0), dtype=table.dtype)
    rows = {i + 1: tuple(int(v) for v in sub[i]) for i in range(table.shape[0])}
    return dict(columns=columns, rows=rows)


def summarize_counts(c, quality_base=33, qualities=None):
    """The reference's ``ReadStatistics.summarize()`` dict from the counters of a block (``ReadStatistics.counts``),
    with ``lengths`` / ``gc`` / ``qualities`` as {"hist", "summary"} and ``bases`` / ``base_qualities`` in
    ``BaseCountingDicts.summarize()`` form.  ``qualities``: None -- quality statistics exist once a non-empty read
    with qualities was seen; True -- always."""
    if c["skipped"]:
        raise RuntimeError("%d reads were longer than the bound the statistics were collected with" % c["skipped"])
    nz = lambda arr, shift=0: {i - shift: int(v) for i, v in enumerate(arr.tolist()) if v}
    summary = dict(counts=int(c["count"]), lengths=hist_summary(nz(c["lengths"]), nz(c["first_len"] + 1)),
                   gc=hist_summary(nz(c["gc"]), nz(c["first_gc"] + 1)),
                   bases=_table_summary(c["seq"], False, quality_base))
    if qualities or (qualities is None and c["withq"]):
        mq = nz(c["meanq"], quality_base)
        if mq:
            summary["qualities"] = hist_summary(mq, nz(c["first_mq"] + 1, quality_base))
        summary["base_qualities"] = _table_summary(c["qual"], True, quality_base)
    return summary


def error_rate_from_counts(c, max_bases=None):
    """``BaseQualityErrorEstimator`` (commands/error/__init__.py:62-82) from the per-position quality table:
    (estimate, total_len).  Every read is cut to ``max_bases`` (falsy: no limit); ``qual2prob`` is base 33
    whatever the quality base."""
    q = c["qual"]
    if max_bases:
        q = q[:max_bases]
    per_char = q.sum(axis=0)
    total_len = int(per_char.sum())
    total_qual = 0.0
    for b in np.nonzero(per_char)[0].tolist():
        total_qual += int(per_char[b]) * 10 ** (-(b - 33) / 10)
    return total_qual / total_len, total_len


# ---------------------------------------------------------------------------------------------- accumulators
class ReadStatistics(object):
    """Statistics of one read stream (``atropos.commands.stats.ReadStatistics``), accumulated on the device.

    ``collect_batch`` adds the records of a FastqBatch -- optionally their kept intervals ``begin`` / ``end``,
    the adapter mask ``ubegin`` / ``uend`` and only those with ``dest == which`` -- as ``atr_fastq_emit`` would
    write them.  ``collect_record`` (and ``collect`` of the subclasses) queues single reads and sends them to the
    device in batches; there is no host computation of the statistics.
    """

    FLUSH_RECORDS = 65536

    def __init__(self, qualities=None, quality_base=33, tiles=None, backend=None):
        if tiles:
            raise NotImplementedError("tile statistics (the tile key is a regular expression over read names)")
        if not 0 <= int(quality_base) <= 255:
            raise ValueError("quality_base must lie in 0 .. 255")
        self.qualities, self.quality_base = qualities, int(quality_base)
        self._be = backend
        self._block, self._cap = None, 0
        self._pending = []
        self.reads = 0                         # records offered so far: the stream index of the next one

    @property
    def backend(self):
        if self._be is None:
            self._be = _lib.get_backend()
        return self._be

    def _reserve(self, longest):
        """A block whose tables reach ``longest`` positions (grown by doubling; old counts carried over)."""
        if longest > _lib.MAX_LONG_READ_LEN:
            raise _lib.AtroposUnsupported("read statistics: a read of %d bases (at most %d)"
                                          % (longest, _lib.MAX_LONG_READ_LEN))
        if self._block is not None and longest <= self._cap:
            return
        cap = max(256, self._cap)
        while cap < longest:
            cap *= 2
        cap = min(cap, _lib.MAX_LONG_READ_LEN)
        be = self.backend
        block = be.empty((be.read_stats_words(cap),), torch.int64)
        be.read_stats_clear(block, cap)
        if self._block is not None:
            be.read_stats_merge(block, cap, self._block, self._cap)
        self._block, self._cap = block, cap

    def collect_batch(self, batch, begin=None, end=None, ubegin=None, uend=None, dest=None, which=None):
        """Add the records of ``batch`` (see the class doc)."""
        self._flush()
        self._collect(batch, begin, end, ubegin, uend, dest, which)

    def _collect(self, batch, begin, end, ubegin, uend, dest, which):
        if (begin is None) != (end is None) or (ubegin is None) != (uend is None) or (ubegin is not None and begin is None):
            raise ValueError("begin / end and ubegin / uend come in pairs, and a mask needs the interval")
        if dest is not None and which is None:
            raise ValueError("dest needs which")
        n = len(batch)
        if n == 0:
            return
        lens = batch.seq_lens if begin is None else (end - begin).clamp(min=0)
        if dest is not None:
            lens = torch.where(dest == which, lens, torch.zeros_like(lens))
        longest = int(lens.max().item())
        if self.qualities is False and longest > 0:
            raise NotImplementedError("qualities=False with non-empty reads (the reference fails on them too)")
        self._reserve(longest)
        self.backend.read_stats_batch(self._block, self._cap, longest, self.quality_base, batch.data, batch.records,
                                      begin, end, ubegin, uend, dest, 0 if which is None else int(which), self.reads)
        self.reads += n

    def collect_record(self, record):
        """Queue one read (any object with ``sequence`` and ``qualities`` strings)."""
        seq, qual = record.sequence or "", record.qualities or ""
        if seq and len(qual) != len(seq):
            raise NotImplementedError("reads without qualities (the reference fails on them too)")
        self._pending.append(b"@\n" + seq.encode("latin-1") + b"\n+\n" + qual.encode("latin-1") + b"\n")
        if len(self._pending) >= self.FLUSH_RECORDS:
            self._flush()

    def collect(self, read1, read2=None):
        raise NotImplementedError()

    def _flush(self):
        if self._pending:
            text, self._pending = b"".join(self._pending), []
            batch, _ = FastqBatch.from_bytes(text, final=True, backend=self.backend)
            self._collect(batch, None, None, None, None, None, None)

    def merge(self, other):
        """Add the counts of ``other`` (same quality base) into this one; other's reads count as read after this
        one's (CountingDict.merge appends the new keys)."""
        if not isinstance(other, ReadStatistics):
            raise ValueError("Cannot merge object of type {}".format(type(other)))
        if other.quality_base != self.quality_base:
            raise ValueError("Cannot merge statistics of different quality bases")
        other._flush()
        self._flush()
        if other._block is not None:
            self._reserve(other._cap)
            self.backend.read_stats_merge(self._block, self._cap, other._block, other._cap, self.reads)
        self.reads += other.reads
        if other.qualities and self.qualities is None:
            self.qualities = True
        return self

    def counts(self):
        """The counters as host arrays: count, longest, withq, skipped; lengths [longest + 1], gc [101],
        meanq [256] (bin = mean + quality_base), seq / qual [longest, 256]; first_len / first_gc / first_mq: per
        bin the stream index of the first read in it, -1 for an empty bin."""
        self._flush()
        if self._block is None:
            z = np.zeros((0, 256), dtype=np.int64)
            none = lambda k: np.full(k, -1, np.int64)
            return dict(count=0, longest=0, withq=0, skipped=0, lengths=np.zeros(1, np.int64),
                        gc=np.zeros(GC_BINS, np.int64), meanq=np.zeros(MQ_BINS, np.int64), seq=z, qual=z,
                        first_len=none(1), first_gc=none(GC_BINS), first_mq=none(MQ_BINS))
        host = self._block.cpu().numpy()
        lay = layout(self._cap)
        longest = int(host[LONGEST])
        nlen = int(np.nonzero(host[lay["len"]:lay["gc"]])[0].max()) + 1 if host[COUNT] else 1
        # ~index in the block, 0 = none: as int64, ~x is -1 - x, so -1 - stored gives the index and -1 for none
        first = -1 - host[lay["first"]:lay["words"]]
        f_gc = first[self._cap + 1:self._cap + 1 + GC_BINS]
        return dict(count=int(host[COUNT]), longest=longest, withq=int(host[WITHQ]), skipped=int(host[SKIPPED]),
                    lengths=host[lay["len"]:lay["len"] + nlen], gc=host[lay["gc"]:lay["mq"]],
                    meanq=host[lay["mq"]:lay["seq"]],
                    seq=host[lay["seq"]:lay["qual"]].reshape(self._cap, 256)[:longest],
                    qual=host[lay["qual"]:lay["first"]].reshape(self._cap, 256)[:longest],
                    first_len=first[:nlen], first_gc=f_gc, first_mq=first[self._cap + 1 + GC_BINS:])

    def summarize(self):
        return summarize_counts(self.counts(), self.quality_base, self.qualities)

    def error_rate(self, max_bases=None):
        """(estimate, total_len) of ``BaseQualityErrorEstimator`` over the collected reads."""
        return error_rate_from_counts(self.counts(), max_bases)


class SingleEndReadStatistics(ReadStatistics):
    """``SingleEndReadStatistics``: summary {"read1": ...}."""

    def collect(self, read1, read2=None):
        self.collect_record(read1)

    def summarize(self):
        return dict(read1=super().summarize())


class PairedEndReadStatistics(object):
    """``PairedEndReadStatistics``: one ReadStatistics per read, summary {"read1": ..., "read2": ...}."""

    def __init__(self, **kwargs):
        self.read1 = ReadStatistics(**kwargs)
        self.read2 = ReadStatistics(**kwargs)

    def collect(self, read1, read2):
        self.read1.collect_record(read1)
        self.read2.collect_record(read2)

    def collect_batch(self, batch1, batch2, begin1=None, end1=None, begin2=None, end2=None, ubegin1=None, uend1=None,
                      ubegin2=None, uend2=None, dest=None, which=None):
        self.read1.collect_batch(batch1, begin1, end1, ubegin1, uend1, dest, which)
        self.read2.collect_batch(batch2, begin2, end2, ubegin2, uend2, dest, which)

    def merge(self, other):
        self.read1.merge(other.read1)
        self.read2.merge(other.read2)
        return self

    def summarize(self):
        return dict(read1=self.read1.summarize(), read2=self.read2.summarize())


# ---------------------------------------------------------------------------------------------- file drivers
# (every chunk of ``fastq.read_chunks`` into the counters: one file, or two in lock step)
def _need_qualities(batches):
    """FASTA input has no qualities to count: a clear ValueError (the reference's qc and error commands fail on it)."""
    if any(getattr(b, "fmt", "fastq") == "fasta" for b in batches):
        raise ValueError("read statistics and error rates need quality values: the input is FASTA")


def qc_file(path, chunk_bytes=64 << 20, quality_base=33, qualities=True, device_gunzip=False):
    """``atropos qc`` of one FASTQ file: {"pre": {0: {"read1": summary}}} (QcPipeline.finish).  ``device_gunzip``
    (here and in the drivers below): BGZF ``.gz`` input is inflated on the GPU (``fastq.ChunkedFastqReader``)."""
    st = SingleEndReadStatistics(qualities=qualities, quality_base=quality_base)
    for batches in read_chunks([path], chunk_bytes, device_gunzip=device_gunzip):
        _need_qualities(batches)
        st.collect_batch(*batches)
    return {"pre": {0: st.summarize()}}


def qc_files(path1, path2=None, chunk_bytes=64 << 20, quality_base=33, qualities=True, device_gunzip=False):
    """``atropos qc`` of paired files: {"pre": {0: {"read1": ..., "read2": ...}}}.  ``path2=None``: ``path1`` is an
    interleaved file (the reference's ``-l``; ``fastq.read_chunks(interleaved=True)``)."""
    st = PairedEndReadStatistics(qualities=qualities, quality_base=quality_base)
    paths = [path1] if path2 is None else [path1, path2]
    for batches in read_chunks(paths, chunk_bytes, device_gunzip=device_gunzip, interleaved=path2 is None):
        _need_qualities(batches)
        st.collect_batch(*batches)
    return {"pre": {0: st.summarize()}}


def error_rate_file(path, path2=None, max_bases=None, chunk_bytes=64 << 20, device_gunzip=False, interleaved=False):
    """``atropos error -a quality``: (estimates, total_lens), one entry per input file, as
    BaseQualityErrorEstimator / PairedErrorEstimator put them in the summary.  ``interleaved``: ``path`` alone holds
    the pairs (the reference's ``-l``); one entry per read, as for two files."""
    if interleaved and path2 is not None:
        raise ValueError("interleaved input is one file")
    paths = [path] if path2 is None else [path, path2]
    sts = [ReadStatistics(qualities=True) for _ in range(2 if interleaved else len(paths))]
    for batches in read_chunks(paths, chunk_bytes, device_gunzip=device_gunzip, interleaved=interleaved):
        _need_qualities(batches)
        for st, batch in zip(sts, batches):
            st.collect_batch(batch)
    res = [s.error_rate(max_bases) for s in sts]
    return tuple(r[0] for r in res), tuple(r[1] for r in res)

"""Known-contaminant detection on the GPU: the device twin of the reference's ``atropos detect --detector known``
(``KnownContaminantDetector``, commands/detect/__init__.py:495-549) -- "which adapters are in these reads?", the
step before ``trim``.

The reference keeps the *set* of filtered read sequences and intersects, per distinct read and both strands, the
read's k-mer set with the k-mer set of every known sequence, in Python sets; that is why it samples 10 000 reads.
Here the reads of a ``FastqBatch`` stay in device memory and three passes run over them (detect_kernels.hip): the
read filter (complexity <= 1.0, past-end cut, length tests), the exact distinct pass (hash, ``torch.sort``, byte
compare of reads that share a hash) and the match pass over one representative of every distinct sequence, which
leaves four integers per known sequence in a device counter block: the sum of matching k-mers, the number of
distinct reads over ``min_kmer_match_frac``, the largest match among those, and the number of distinct reads that
hold the whole known sequence.  Everything else (thresholds, fractions, filters, the sort) is host arithmetic on
those integers; all floating point of the per-read decisions is hoisted into host tables built with the
reference's own expressions (``complexity_table``, ``hit_thresholds``).

Distinctness is over the whole run: ``add_batch`` keeps the chunks resident and the passes run once over all of them
put together, so the reads looked at must fit one batch (< 4 GiB of FASTQ text; ``ValueError`` beyond).

Differences from the reference, both where its result is unspecified:

* Matches with an equal sort key (``len(seq) * log(count)``) come in the order of the known sequences in the input
  list; the reference leaves them in the insertion order of a dict filled while walking a set of reads.
* ``known_names`` is sorted; the reference's is a set's iteration order.

A read that holds a byte without a complement makes the reference raise ``KeyError``; here it is a ``ValueError``
with the number of such reads.  Reads are at most 320 bases (``AtroposUnsupported`` beyond, nothing is counted).

Out of scope (``NotImplementedError`` at the interface): the heuristic detector (k grows until nothing is
over-represented, so keys outgrow a machine word, and its merge step walks candidates in dict / set order), the
khmer detector (a third-party probabilistic counter), ``--past-end-bases`` given as a regular expression, fetching
the default contaminant list from a URL, the adapter cache file.  No contaminant list ships with the package: the
caller passes a FASTA file or ``name=SEQ`` pairs.
"""
import math

import numpy as np
import torch

from . import _lib
from .fastq import FastqBatch, read_chunks

LOG2 = math.log(2)
MAX_READ = _lib.DETECT_MAX_READ


# ---------------------------------------------------------------------------------------------- host tables
def sequence_complexity(seq):
    """``atropos.util.sequence_complexity``: entropy in bits over the counts of A, C, G, T after ``upper()``,
    each divided by the whole length."""
    upper = seq.upper()
    whole = float(len(upper))
    total = 0
    for present in (upper.count(b) for b in "ACGT"):
        if present:
            share = present / whole
            total += share * math.log(share) / LOG2
    return -total


def complexity_table(max_len=MAX_READ):
    """f[len][count] = (count / len) * log(count / len) / LOG2 with the reference's expression, for every
    count <= len <= max_len (0 elsewhere).  The device adds the entries of A, C, G, T in that order."""
    f = np.zeros((max_len + 1, max_len + 1), dtype=np.float64)
    log = math.log
    for n in range(1, max_len + 1):
        seqlen = float(n)
        row = f[n]
        for count in range(1, n + 1):
            frac = count / seqlen
            row[count] = frac * log(frac) / LOG2
    return f


_TABLES = {}


def _complexity_table(max_len):
    if max_len not in _TABLES:
        _TABLES[max_len] = complexity_table(max_len)
    return _TABLES[max_len]


def distinct_kmers(seq, kmer_size):
    """Number of distinct k-mers of ``seq`` (ContaminantMatcher.n_kmers)."""
    return len({seq[at:at + kmer_size] for at in range(0, len(seq) + 1 - kmer_size)})


def hit_thresholds(n_kmers, min_kmer_match_frac):
    """Per known sequence the smallest n with ``n / n_kmers > min_kmer_match_frac`` in Python floats (-1: none, or
    no k-mers): what the match pass compares its integer n with."""
    out = []
    for nk in n_kmers:
        thr = -1
        for n in range(nk + 1 if nk > 0 else 0):
            if float(n) / nk > min_kmer_match_frac:
                thr = n
                break
        out.append(thr)
    return out


# ---------------------------------------------------------------------------------------------- known sequences
class KnownContaminants(object):
    """The known sequences with their names (the reference's ``AdapterCache`` without file cache and URL):
    distinct sequences in first-seen order, every one with the set of names it was given."""

    def __init__(self):
        self._names_of = {}                    # sequence -> its names, in first-seen order of the sequences
        self._seq_of = {}                      # name -> sequence (the last one given that name)

    def add(self, name, seq):
        self._names_of.setdefault(seq, set()).add(name)
        self._seq_of[name] = seq

    @classmethod
    def from_fasta(cls, path_or_lines):
        """From a FASTA file (a path) or its lines: the first word of a header is the name, sequence lines are
        joined, blank lines and lines that start with '#' are skipped (FastaReader, io/seqio.py:251-280)."""
        self = cls()
        self.load_from_fasta(path_or_lines)
        return self

    def load_from_fasta(self, path_or_lines):
        if isinstance(path_or_lines, str):
            with open(path_or_lines, "rt") as fh:
                return self.load_from_fasta(fh.readlines())
        header, pieces, count = None, [], 0
        for number, raw in enumerate(path_or_lines, 1):
            text = raw.strip()
            if text == "" or (text[0] == "#"):
                continue
            if text[0] != ">":
                if header is None:
                    raise ValueError("line %d: a FASTA record starts with '>', found %r" % (number, text[:100]))
                pieces.append(text)
                continue
            if header is not None:
                self.add(header.split(None, 1)[0], "".join(pieces))
                count += 1
            header, pieces = text[1:], []
        if header is not None:
            self.add(header.split(None, 1)[0], "".join(pieces))
            count += 1
        return count

    names = property(lambda self: list(self._seq_of))
    sequences = property(lambda self: list(self._names_of))

    def iter_sequences(self):
        """(sequence, set of names) pairs in first-seen order."""
        return self._names_of.items()

    def __len__(self):
        return len(self._names_of)

    def summarize(self):
        counts = {"num_adapter_names": len(self._seq_of), "num_adapter_seqs": len(self._names_of)}
        return dict(counts, path=None, auto_reverse_complement=False)


class Match(object):
    """A contaminant match: the fields and ``summarize()`` keys of the reference's ``Match`` for a known
    contaminant (``match_frac2`` and ``longest_match`` stay None for this detector, as there)."""

    match_frac2 = None
    longest_match = None
    is_known = True
    count_is_frequency = False                 # the count is an integer number of k-mers

    def __init__(self, seq, count=0, names=None, match_frac=None, abundance=None):
        self.seq, self.known_seqs = seq, [seq]
        self.names = tuple(names) if names else None
        self.count, self.match_frac, self.abundance = count, match_frac, abundance

    def __len__(self):
        return len(self.seq)

    def __repr__(self):
        return "%s => %s" % (self.seq, self.names)

    @property
    def seq_complexity(self):
        return sequence_complexity(self.seq)

    def summarize(self):
        pairs = [("longest_kmer", self.seq), ("kmer_freq", self.count), ("kmer_freq_type", "count"),
                 ("abundance", self.abundance), ("is_known", True),
                 ("known_to_contaminant_match_frac", self.match_frac), ("contaminant_to_known_match_frac", None),
                 ("longest_match", None), ("known_names", self.names), ("known_seqs", self.known_seqs)]
        return dict(pairs)


# ---------------------------------------------------------------------------------------------- the detector
def _check_past_end(past_end_bases):
    bases = tuple(past_end_bases or ())
    for b in bases:
        if len(b) != 1:
            raise NotImplementedError("--past-end-bases given as a regular expression (only single bases)")
        if not (b.isalnum() and ord(b) < 128):
            raise NotImplementedError("a past-end base that is not a letter or digit (it would be regular-expression syntax)")
    return bases


def _concat(batches):
    """The batches as one: their texts back to back, the records' offsets shifted."""
    if len(batches) == 1:
        return batches[0]
    be = batches[0].backend
    total = sum(b.nbytes for b in batches)
    if total >= (1 << 32) - 16:
        raise ValueError("detect: the reads looked at must fit one batch (< 4 GiB of FASTQ text); use max_reads")
    data = be.empty(((total + 15) // 16 * 16 + 16,), torch.uint8)
    recs, base = [], 0
    for b in batches:
        data[base:base + b.nbytes].copy_(b.data[:b.nbytes])
        r = b.records.to(torch.int64)
        # name, sequence and quality offsets; `reserved` too: it is an offset only for records whose flags say so
        # (fastq_core.hpp) and is not read otherwise, so shifting it everywhere is harmless
        for col in (0, 2, 4, 7):
            r[:, col] = ((r[:, col] & 0xFFFFFFFF) + base) & 0xFFFFFFFF
        r = torch.where(r >= (1 << 31), r - (1 << 32), r)
        recs.append(r.to(torch.int32))
        base += b.nbytes
    data[total:].zero_()
    return FastqBatch(data, total, torch.cat(recs).contiguous(), be)


class KnownContaminantDetector(object):
    """``KnownContaminantDetector`` over device-resident reads.

    ``add_batch`` takes FastqBatches; ``matches`` / ``summarize`` run the device passes over all of them and apply
    the reference's thresholds, filters and sort.  ``n_reads`` is the configured maximum the reference scales its
    minimum hit count with (not the number of reads seen); ``None``: the number of reads added.
    """

    def __init__(self, known_contaminants, kmer_size=12, n_reads=10000, overrep_cutoff=100, include="all",
                 past_end_bases=("A",), min_kmer_match_frac=0.5, backend=None):
        if not len(known_contaminants):
            raise ValueError("no known contaminant sequences")
        if include not in ("all", "known", "unknown"):
            raise ValueError("include must be 'all', 'known' or 'unknown'")
        self.known_contaminants = known_contaminants
        self.kmer_size, self.n_reads, self.overrep_cutoff = int(kmer_size), n_reads, overrep_cutoff
        self.include = include
        self.past_end_bases = _check_past_end(past_end_bases)
        if not 0 <= min_kmer_match_frac <= 1:
            raise ValueError("min_kmer_match_frac must lie in 0 .. 1")
        self.min_kmer_match_frac = min_kmer_match_frac
        self._items = [(seq, names) for seq, names in known_contaminants.iter_sequences()]
        self._min_k = min(len(s) for s, _ in self._items)
        self._n_kmers = [distinct_kmers(s, self.kmer_size) for s, _ in self._items]
        self._be = backend
        self._handle = None
        self._batches = []
        self._resident = 0                     # bytes of FASTQ text added so far
        self._read_length = None
        self._counts = None
        self.reads = 0
        self.timings = {}

    @property
    def backend(self):
        if self._be is None:
            self._be = _lib.get_backend()
        return self._be

    def _create(self):
        if self._handle is None:
            seqs = []
            for s, _ in self._items:
                try:
                    seqs.append(s.encode("latin-1"))
                except UnicodeEncodeError:
                    raise ValueError("known sequence %r holds characters beyond one byte" % s)
            self._handle = self.backend.detect_create(
                seqs, self.kmer_size, "".join(self.past_end_bases).encode("ascii"),
                hit_thresholds(self._n_kmers, self.min_kmer_match_frac), _complexity_table(MAX_READ), MAX_READ)
        return self._handle

    def close(self):
        if self._handle is not None:
            self.backend.detect_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_batch(self, batch):
        """Add the records of a FastqBatch (kept resident until the detector is dropped)."""
        if len(batch) == 0:
            return
        if self._resident + batch.nbytes >= (1 << 32) - 16:
            raise ValueError("detect: the reads looked at must fit one batch (< 4 GiB of FASTQ text); use max_reads")
        if self._read_length is None:
            self._read_length = int(batch.records[0, 3].item())
        self._batches.append(batch)
        self._resident += batch.nbytes
        self.reads += len(batch)
        self._counts = None

    def counters(self, recompute=False, timed=False):
        """The device passes over everything added so far.  Returns dict(kept, distinct, matches, hits, max_n,
        abundance): two integers and four int64 arrays in the order of the known sequences.  The result is kept
        until reads are added; ``recompute`` runs the passes again, ``timed`` also leaves the seconds of each pass
        (with a device synchronisation around it) in ``timings``."""
        if self._counts is not None and not (timed or recompute):
            return self._counts
        be = self.backend
        h = self._create()
        nseq = len(self._items)
        if not self._batches:
            z = np.zeros(nseq, np.int64)
            self._counts = dict(kept=0, distinct=0, matches=z, hits=z.copy(), max_n=z.copy(), abundance=z.copy())
            return self._counts
        batch = _concat(self._batches)
        self._batches = [batch]
        longest = int(batch.seq_lens.max().item())
        if longest > MAX_READ:
            raise _lib.AtroposUnsupported("detect: a read of %d bases (at most %d)" % (longest, MAX_READ))
        clock = _Clock(be, timed)
        block = be.detect_counters(h)
        clock.start()
        kept, hashes = be.detect_filter(h, batch.data, batch.records, longest, block)
        clock.stop("filter")
        idx = torch.nonzero(kept > 0).squeeze(1)
        hs, o = torch.sort(hashes.index_select(0, idx))
        order = idx.index_select(0, o).contiguous()
        m = int(order.shape[0])
        if m:
            pos = torch.arange(m, device=hs.device, dtype=torch.int64)
            start = torch.ones((m,), dtype=torch.bool, device=hs.device)
            start[1:] = hs[1:] != hs[:-1]
            head = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 0).values.contiguous()
            rep = be.detect_mark(h, batch.data, batch.records, kept, order, head, block)
            clock.stop("distinct")
            be.detect_match(h, batch.data, batch.records, kept, order, rep, block)
            clock.stop("match")
        host = be.detect_read(h, block)
        self.timings = clock.seconds
        hdr = _lib.DETECT_HDR
        if int(host[3]):
            raise _lib.AtroposUnsupported("detect: %d read(s) longer than %d bases" % (int(host[3]), MAX_READ))
        if int(host[2]):
            raise ValueError("%d read(s) contain bases without a complement (the reference raises KeyError on them)"
                             % int(host[2]))
        body = host[hdr:hdr + 4 * nseq].reshape(4, nseq)
        self._counts = dict(kept=int(host[0]), distinct=int(host[1]), matches=body[0].copy(), hits=body[1].copy(),
                            max_n=body[2].copy(), abundance=body[3].copy())
        return self._counts

    def min_count(self):
        """The reference's minimum number of hits (``_get_contaminants``)."""
        n_reads = self.reads if self.n_reads is None else self.n_reads
        positions = self._read_length - self._min_k + 1
        scaled = n_reads * positions * self.overrep_cutoff
        return math.ceil(scaled / float(4 ** self._min_k))

    def matches(self, min_len=None, min_complexity=1.1, min_match_frac=0.1, limit=20):
        """``Detector.matches``: the contaminants over the thresholds, filtered and sorted (ties in list order)."""
        min_len = self.kmer_size if min_len is None else min_len
        c = self.counters()
        if self._read_length is None:
            return []
        min_count = self.min_count()
        found = []
        for s, (seq, names) in enumerate(self._items):
            hits = int(c["hits"][s])
            if hits < 1 or hits < min_count:
                continue
            found.append(Match(seq, count=int(c["matches"][s]), names=sorted(names),
                               match_frac=int(c["max_n"][s]) / self._n_kmers[s], abundance=int(c["abundance"][s])))

        def keep(m):
            if m.count < 0.1:
                return False
            if min_len and len(m) < min_len:
                return False
            if min_complexity and m.seq_complexity < min_complexity:
                return False
            if self.include == "unknown":
                return False
            if min_match_frac and m.match_frac < min_match_frac:
                return False
            return True

        found = [m for m in found if keep(m)]
        found.sort(key=_sort_key, reverse=True)
        return found if limit is None else found[:limit]

    def _args_summary(self):
        return dict(kmer_size=self.kmer_size, n_reads=self.reads if self.n_reads is None else self.n_reads,
                    overrep_cutoff=self.overrep_cutoff, include=self.include, past_end_bases=self.past_end_bases,
                    known_contaminants=self.known_contaminants.summarize())

    def summarize(self, **kwargs):
        """The reference's ``summary['detect']``."""
        out = self._args_summary()
        out["matches"] = ([m.summarize() for m in self.matches(**kwargs)],)
        return out


def _sort_key(match):
    return len(match.seq) * math.log(match.count)


class _Clock(object):
    """Seconds per pass, with a device synchronisation around each (only when asked for)."""

    def __init__(self, backend, on):
        self.on = bool(on) and getattr(backend, "name", "") == "hip"
        self.be = backend
        self.seconds = {}

    def _sync(self):
        torch.cuda.synchronize(self.be.device)

    def start(self):
        if self.on:
            import time
            self._sync()
            self.t0 = time.perf_counter()

    def stop(self, name):
        if self.on:
            import time
            self._sync()
            t = time.perf_counter()
            self.seconds[name] = t - self.t0
            self.t0 = t


class PairedDetector(object):
    """Two independent detectors, one per read of the pair (``PairedDetector``, :461-492)."""

    def __init__(self, known_contaminants, **kwargs):
        self.read1_detector = KnownContaminantDetector(known_contaminants, **kwargs)
        self.read2_detector = KnownContaminantDetector(known_contaminants, **kwargs)

    def add_batch(self, batch1, batch2):
        if len(batch1) != len(batch2):
            raise ValueError("the two batches hold different numbers of records")
        self.read1_detector.add_batch(batch1)
        self.read2_detector.add_batch(batch2)

    def close(self):
        self.read1_detector.close()
        self.read2_detector.close()

    def matches(self, **kwargs):
        return self.read1_detector.matches(**kwargs), self.read2_detector.matches(**kwargs)

    def summarize(self, **kwargs):
        out = self.read1_detector._args_summary()
        out["matches"] = tuple([m.summarize() for m in ms] for ms in self.matches(**kwargs))
        return out


# ---------------------------------------------------------------------------------------------- file drivers
def _detect_paths(paths, detector_class, known_contaminants, max_reads, chunk_bytes, kwargs, interleaved=False):
    """The chunks of ``fastq.read_chunks`` into a detector until ``max_reads`` records went in; its summary."""
    report = {k: kwargs.pop(k) for k in ("min_len", "min_complexity", "min_match_frac", "limit") if k in kwargs}
    device_gunzip = kwargs.pop("device_gunzip", False)        # (BGZF .gz input inflated on the GPU: fastq.ChunkedFastqReader)
    kwargs.setdefault("n_reads", max_reads)
    det = detector_class(known_contaminants, **kwargs)
    try:
        left = max_reads
        for batches in read_chunks(paths, chunk_bytes, device_gunzip=device_gunzip, interleaved=interleaved):
            if left is not None:
                batches = [b.head(left)[0] for b in batches]
                left -= len(batches[0])
            det.add_batch(*batches)
            if left is not None and left <= 0:
                break
        return det.summarize(**report)
    finally:
        det.close()


def detect_file(path, known_contaminants, max_reads=10000, chunk_bytes=64 << 20, **kwargs):
    """``atropos detect --detector known`` of one FASTQ file, read in chunks, stopping after ``max_reads`` records
    (None: the whole file, which must fit one batch -- see the module doc).  ``n_reads`` defaults to ``max_reads``.
    Returns the reference's ``summary['detect']`` dict; ``matches`` is a 1-tuple of lists.  ``device_gunzip=True``
    (here and in ``detect_files``): BGZF ``.gz`` input is inflated on the GPU."""
    return _detect_paths([path], KnownContaminantDetector, known_contaminants, max_reads, chunk_bytes, kwargs)


def detect_files(path1, path2, known_contaminants, max_reads=10000, chunk_bytes=64 << 20, **kwargs):
    """The same for paired files: ``matches`` is a 2-tuple of lists, one per read.  ``path2=None``: ``path1`` is an
    interleaved file (the reference's ``-l``), as in ``trim_files``; ``max_reads`` counts pairs either way."""
    paths = [path1] if path2 is None else [path1, path2]
    return _detect_paths(paths, PairedDetector, known_contaminants, max_reads, chunk_bytes, kwargs, interleaved=path2 is None)


def detect_from_args(argv, paired=False):
    """Build the detector from the subset of ``atropos detect`` options the device path covers (same spellings and
    defaults as commands/detect/cli.py): ``-d/--detector known``, ``-k/--kmer-size``, ``--max-reads``,
    ``-e/--past-end-bases``, ``-i/--include-contaminants``, ``-x/--known-contaminant name=SEQ``,
    ``-F/--known-contaminants-file``, ``--min-kmer-match-frac``.  Returns a ``KnownContaminantDetector`` (``paired``:
    a ``PairedDetector``) whose ``n_reads`` is ``--max-reads``.  Anything else raises."""
    import argparse
    ap = argparse.ArgumentParser(prog="detect", add_help=False)
    for flags, spec in (
            (("-d", "--detector"), dict(default=None, choices=("known", "heuristic", "khmer"))),
            (("-k", "--kmer-size"), dict(default=12, type=int)),
            (("--max-reads",), dict(default=10000, type=int)),
            (("-e", "--past-end-bases"), dict(default=("A",), nargs="*")),
            (("-i", "--include-contaminants"), dict(default="all", choices=("all", "known", "unknown"))),
            (("-x", "--known-contaminant"), dict(default=None, dest="known_adapter", action="append")),
            (("-F", "--known-contaminants-file"), dict(default=None, dest="known_adapters_file", action="append")),
            (("--min-kmer-match-frac",), dict(default=0.5, type=float)),
            (("--no-default-contaminants",), dict(default=True, dest="default_adapters", action="store_false"))):
        ap.add_argument(*flags, **spec)
    try:
        opts, rest = ap.parse_known_args(list(argv))
    except SystemExit:
        raise ValueError("detect: cannot parse %r" % (list(argv),))
    if rest:
        raise NotImplementedError("detect: option(s) outside the device path: %s" % " ".join(rest))
    detector = opts.detector
    if detector is None and opts.include_contaminants == "known":
        detector = "known"
    if detector == "heuristic" or detector is None:
        raise NotImplementedError("the heuristic detector (k grows until nothing is over-represented: keys outgrow a "
                                  "machine word, and its merge walks candidates in set order); pass --detector known")
    if detector == "khmer":
        raise NotImplementedError("the khmer detector (a third-party probabilistic counter)")
    if opts.kmer_size < 1:
        raise ValueError("--kmer-size must be positive")
    if not 0 <= opts.min_kmer_match_frac <= 1:
        raise ValueError("--min-kmer-match-frac must lie in 0 .. 1")
    known = KnownContaminants()
    for item in opts.known_adapter or ():
        name, seq = item.split("=")
        known.add(name, seq)
    for path in opts.known_adapters_file or ():
        if "://" in path and not path.startswith("file:"):
            raise NotImplementedError("fetching a contaminant list from a URL")
        known.load_from_fasta(path[5:] if path.startswith("file:") else path)
    if not len(known):
        raise NotImplementedError("the default contaminant list (it is fetched from a URL); pass --known-contaminant "
                                  "or --known-contaminants-file")
    kwargs = dict(kmer_size=opts.kmer_size, n_reads=opts.max_reads, include=opts.include_contaminants,
                  past_end_bases=tuple(opts.past_end_bases), min_kmer_match_frac=opts.min_kmer_match_frac)
    return PairedDetector(known, **kwargs) if paired else KnownContaminantDetector(known, **kwargs)

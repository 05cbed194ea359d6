"""Contaminant detection on the GPU: the device twins of the reference's ``atropos detect --detector known``
(``KnownContaminantDetector``, commands/detect/__init__.py:495-549) and ``--detector heuristic`` (``HeuristicDetector``,
:552-745) -- "which adapters are in these reads?", the step before ``trim``.

**Known contaminants.**  The reference keeps the *set* of filtered read sequences and intersects, per distinct read and
both strands, the read's k-mer set with the k-mer set of every known sequence, in Python sets; that is why it samples
10 000 reads.  Here the reads of a ``FastqBatch`` stay in device memory and three passes run over them
(detect_kernels.hip): the read filter (complexity <= 1.0, past-end cut, length tests), the exact distinct pass (hash,
``torch.sort``, byte compare of reads that share a hash) and the match pass over one representative of every distinct
sequence, which leaves four integers per known sequence in a device counter block: the sum of matching k-mers, the
number of distinct reads over ``min_kmer_match_frac``, the largest match among those, and the number of distinct reads
that hold the whole known sequence.  Everything else (thresholds, fractions, filters, the sort) is host arithmetic on
those integers; all floating point of the per-read decisions is hoisted into host tables built with the reference's own
expressions (``complexity_table``, ``hit_thresholds``).

**De-novo discovery** (``HeuristicDetector``; no known list is needed).  The reference counts every k-mer of the distinct
reads in a dict of Python sets of whole reads, keeps the k-mers seen more than ``min_count(k)`` times, and repeats with
k + 1 over the reads that held one, until nothing is over-represented.  Here that loop is integer counting over the
resident representatives (detect_kmer_kernels.hip): a k-mer is known by its *class*, the dense rank of its text among
the k-mers of that length, and the class of a (k + 1)-mer is the rank of the pair (class of its k-mer, next byte) -- a
40-bit key that ``torch.sort`` orders, so no key outgrows a machine word and nothing is hashed.  The classes at
``kmer_size`` come from ranks of pairs by doubling (1, 2, 4, 8, then 8 + 4 for 12).  One level is a handful of launches
and one read-back of the state block; the over-represented classes land in a candidate table on the device.  The host
takes the candidates' texts and counts and runs the reference's greedy merge, its 50 % cut, the matching against known
sequences (with ``align.Aligner``) and ``Detector._filter_and_sort`` in Python; abundance and ``longest_match`` of the
few final sequences come from one more pass over the representatives.  ``min_count(k)`` is the reference's own
expression, evaluated on the host.

Distinctness is over the whole run: ``add_batch`` keeps the chunks resident and the passes run once over all of them
put together, so the reads looked at must fit one batch (< 4 GiB of FASTQ text; ``ValueError`` beyond).

Differences from the reference, all where its result depends on the iteration order of a set of strings (which changes
with the interpreter's hash seed):

* Known detector: matches with an equal sort key (``len(seq) * log(count)``) come in the order of the known sequences
  in the input list; ``known_names`` is sorted.
* Heuristic detector, the tie rules:

  - the candidates enter the stable sort of the merge ordered by k ascending and, inside one k, by their first
    occurrence: the distinct reads in the order of their first records, start offsets ascending.  That is the
    reference's own insertion order (lower k first; inside one k the k-mers as a scan of the reads of that level meets
    them) with its set of reads walked in input order.  Ordering one k by text instead changes results the reference
    gives under every hash seed: two overlapping k-mers of one adapter with equal sort keys come in offset order
    there, whichever read is walked first;
  - ``longest_match``: the reference keeps the first read of a set in which the sequence starts at the smallest
    index.  Here: among the reads of ``result_seqs[x]`` (the reads still in play at level ``len(x)`` that hold ``x``)
    where ``x`` starts at the smallest index, the one whose first record comes first in the input; the value is that
    read's kept text from that index on, with the reference's ``seqlen = len(x) - idx``;
  - the names and sequences of a match with several equally good known sequences (``set_known``) come sorted (the
    sequences by ``repr``: the reference's 1-tuple ``(contam.seq,)`` inside ``known_seqs`` is kept, it is data);
  - final sort ties stay in the order of the list being sorted: known matches in the reference's dict order (which
    is insertion order and does not depend on a hash), then unknown ones.

A read that holds a byte without a complement makes the reference raise ``KeyError`` (known detector: any kept read;
heuristic detector: a final sequence or its longest match that reaches the known matching); here it is a
``ValueError``.  Reads are at most 320 bases (``AtroposUnsupported`` beyond, nothing is counted), ``kmer_size`` is
4 .. 32, the heuristic detector holds at most 2^31 - 1 kept bases of distinct reads and 2^20 candidates (the host merge
is quadratic in them).

Out of scope (``NotImplementedError`` at the interface): the khmer detector (a third-party probabilistic counter),
``--past-end-bases`` given as a regular expression, fetching the default contaminant list from a URL, the adapter cache
file.  No contaminant list ships with the package: the caller passes a FASTA file or ``name=SEQ`` pairs, or runs the
heuristic detector without one.
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


# ---------------------------------------------------------------------------------------------- de-novo discovery
class HeuristicMatch(object):
    """A match of the heuristic detector: the reference's ``Match`` made from a sequence (:130-228).  It is unknown
    (``known_seqs`` None, ``is_known`` False) until ``set_known`` names the known sequences it fits; ``longest_match``
    is ``(text, seqlen)`` or None."""

    def __init__(self, seq, count=0, abundance=None, longest_match=None):
        self.seq, self.count, self.abundance, self.longest_match = seq, count, abundance, longest_match
        self.names = self.known_seqs = self.match_frac = self.match_frac2 = None

    def __len__(self):
        return len(self.seq)

    def __repr__(self):
        return "%s => %s (%s))" % (self.seq, self.names, self.known_seqs) if self.is_known else self.seq

    @property
    def is_known(self):
        return self.known_seqs is not None

    @property
    def seq_complexity(self):
        return sequence_complexity(self.seq)

    @property
    def count_is_frequency(self):
        return isinstance(self.count, float)

    def set_known(self, names, seqs, match_frac, match_frac2=None):
        self.names = tuple(names) if names else None
        self.known_seqs, self.match_frac, self.match_frac2 = seqs, match_frac, match_frac2

    def summarize(self):
        out = dict(longest_kmer=self.seq, kmer_freq=self.count,
                   kmer_freq_type="frequency" if self.count_is_frequency else "count", abundance=self.abundance,
                   is_known=self.is_known, known_to_contaminant_match_frac=None, contaminant_to_known_match_frac=None,
                   longest_match=None, known_names=None, known_seqs=None)
        if self.longest_match:
            out.update(longest_match=self.longest_match[0])
        if self.is_known:
            out.update(known_to_contaminant_match_frac=self.match_frac, contaminant_to_known_match_frac=self.match_frac2,
                       known_names=self.names, known_seqs=self.known_seqs)
        return out


class _KnownMatcher(object):
    """``ContaminantMatcher`` (:231-286) without its running total, which the heuristic detector never reads."""

    def __init__(self, seq, names, kmer_size):
        self.seq, self.names, self.kmer_size = seq, names, kmer_size
        self.kmers = {seq[i:i + kmer_size] for i in range(len(seq) - kmer_size + 1)}
        self.n_kmers = len(self.kmers)

    def match(self, seq, seqrc):
        """(share of this sequence's k-mers found, share of the text's k-mers that are found, the text): of ``seq`` and
        its reverse complement the one that holds more of them, ``seq`` on a tie."""
        k = self.kmer_size
        sides = []
        for text in (seq, seqrc):
            kmers = {text[i:i + k] for i in range(len(text) - k + 1)}
            sides.append((float(len(self.kmers & kmers)), kmers, text))
        n, kmers, text = sides[0] if sides[0][0] >= sides[1][0] else sides[1]
        return (n / self.n_kmers if self.n_kmers > 0 else 0), (n / len(kmers) if len(kmers) > 0 else 0), text


def _align(seq1, seq2, min_overlap_frac=0.9):
    """The reference's module-level ``align`` (:835-858): ``seq2`` inside ``seq1`` without an error or an indel,
    overlapping at least ``min_overlap_frac`` of the shorter of the two."""
    from .align import Aligner, SEMIGLOBAL
    aligner = Aligner(seq1, 0.0, SEMIGLOBAL, False, False)
    aligner.min_overlap = math.ceil(min(len(seq1), len(seq2)) * min_overlap_frac)
    aligner.indel_cost = 100000
    match = aligner.locate(seq2)
    return seq1[match[0]:match[1]] if match else None


def merge_candidates(results):
    """The reference's greedy merge of overlapping candidates (:621-644) and what follows up to the ``Match`` objects
    (:646-658): ``results`` is a list of (sequence, count) in the order they enter the stable sort; returns the
    [sequence, count] pairs within 50 % of the top count, most frequent first."""
    todo = sorted(results, key=lambda r: len(r[0]) * math.log(r[1]), reverse=True)        # (stable: ties keep their order)
    done = []
    while len(todo) > 1:
        top, total = todo[0]
        apart = []
        for other, count in todo[1:]:
            if len(top) >= len(other) and other in top:          # a piece of the current sequence: its count joins
                total += count
            elif top in other:                                   # a longer one around it: take it over while the counts are close
                if total < 2 * count:
                    top = other
                total += count
            else:
                apart.append((other, count))
        done.append([top, total])
        todo = apart
    done += [list(r) for r in todo]
    if not done:
        return []
    done.sort(key=lambda r: r[1], reverse=True)
    floor = int(done[0][1] * 0.5)
    return [r for r in done if r[1] >= floor]


class HeuristicDetector(object):
    """``HeuristicDetector`` (:552-745) over device-resident reads: the over-represented k-mers for growing k are
    counted on the device (see the module doc), the merge and the known matching are the reference's, on the host.

    ``add_batch`` takes FastqBatches; ``candidates`` is the host view of the device's candidate table, ``matches`` /
    ``summarize`` the reference's result.  ``known_contaminants`` is optional.  ``n_reads`` as in the known detector."""

    CAPACITY = _lib.KMER_MAX_CANDIDATES

    def __init__(self, known_contaminants=None, kmer_size=12, n_reads=10000, overrep_cutoff=100, include="all",
                 past_end_bases=("A",), min_frequency=0.001, min_contaminant_match_frac=0.9, backend=None):
        if include not in ("all", "known", "unknown"):
            raise ValueError("include must be 'all', 'known' or 'unknown'")
        self.known_contaminants = known_contaminants
        self.kmer_size, self.n_reads, self.overrep_cutoff = int(kmer_size), n_reads, overrep_cutoff
        self.include = include
        self.past_end_bases = _check_past_end(past_end_bases)
        self.min_frequency, self.min_contaminant_match_frac = min_frequency, min_contaminant_match_frac
        self._be = backend
        self._handle = None
        self._batches = []
        self._resident = 0
        self._read_length = None
        self._found = None
        self.reads = 0
        self.timings = {}

    backend = KnownContaminantDetector.backend
    add_batch = KnownContaminantDetector.add_batch
    close = KnownContaminantDetector.close
    __del__ = KnownContaminantDetector.__del__

    @property
    def _counts(self):
        return self._found

    @_counts.setter
    def _counts(self, value):                  # (add_batch drops the kept result through this name)
        self._found = value

    def _create(self):
        if self._handle is None:
            self._handle = self.backend.detect_create(
                [], self.kmer_size, "".join(self.past_end_bases).encode("ascii"), [], _complexity_table(MAX_READ), MAX_READ)
        return self._handle

    def min_count(self, kmer_size):
        """The reference's ``_min_count`` (:569-573), its own expression."""
        n_reads = self.reads if self.n_reads is None else self.n_reads
        return math.ceil(n_reads * max(
            self.min_frequency,
            (self._read_length - kmer_size + 1) * self.overrep_cutoff /
            float(4 ** kmer_size)))

    @property
    def min_report_freq(self):
        return 0.1 * (self.reads if self.n_reads is None else self.n_reads)

    # -- the device passes ------------------------------------------------------------------------------------
    def _ranks_at_k0(self, be, tab, slot_rep, data, total, clock):
        """The classes of the ``kmer_size``-mers by ranks of pairs: 1 -> 2 -> 4 -> ..., then the set bits of
        ``kmer_size`` from the top.  Returns (cls, (begin, end, head))."""
        ids = {1: None}

        def combine(a, b):
            keys = be.detect_kmer_pair_keys(tab, slot_rep, data, ids[a], a, ids[b], b)
            sk, si = torch.sort(keys)
            cls = be.empty((max(total, 1),), torch.int32)
            begin, end, head, _ = be.detect_kmer_rank(sk, si, None, cls)
            ids[a + b] = cls
            return begin, end, head

        k0, top = self.kmer_size, 1
        classes = None
        while 2 * top <= k0:
            classes = combine(top, top)
            top *= 2
        have, bit = top, top // 2
        while bit:
            if k0 & bit:
                classes = combine(have, bit)
                have += bit
            bit //= 2
        clock.stop("rank")
        return ids[k0], classes

    def discover(self, recompute=False, timed=False):
        """The device passes over everything added so far.  Returns a dict: ``kept``, ``distinct``, ``levels`` (the
        first level without an over-represented k-mer), ``over`` (over-represented classes per level), ``rows`` (the
        candidate table, int32 [n, 5]: level, count, representative, offset, quirk) and ``texts`` (bytes per row),
        and the device state the support pass reads.  Kept until reads are added."""
        if self._found is not None and not (timed or recompute):
            return self._found
        be = self.backend
        h = self._create()
        k0 = self.kmer_size
        empty = dict(kept=0, distinct=0, levels=k0, over={k0: 0}, rows=np.zeros((0, _lib.KMER_C_WORDS), np.int32), texts=[],
                     nrep=0, tab=None, slot_rep=None, level=None, batch=None, kept_t=None)
        if not self._batches:
            self._found = empty
            return empty
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
        # a stable sort: inside a run of equal hashes the records ascend, so the representative of a sequence is its
        # first record (the longest-match tie rule names it)
        hs, o = torch.sort(hashes.index_select(0, idx), stable=True)
        order = idx.index_select(0, o).contiguous()
        m = int(order.shape[0])
        if m == 0:
            host = be.detect_read(h, block)
            self._found = dict(empty, kept=int(host[0]))
            self.timings = clock.seconds
            return self._found
        pos = torch.arange(m, device=hs.device, dtype=torch.int64)
        start = torch.ones((m,), dtype=torch.bool, device=hs.device)
        start[1:] = hs[1:] != hs[:-1]
        head = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 0).values.contiguous()
        rep = be.detect_mark(h, batch.data, batch.records, kept, order, head, block)
        host = be.detect_read(h, block)
        if int(host[3]):
            raise _lib.AtroposUnsupported("detect: %d read(s) longer than %d bases" % (int(host[3]), MAX_READ))
        reps = torch.sort(order[rep > 0]).values.contiguous()
        nrep = int(reps.shape[0])
        lens = kept.index_select(0, reps).to(torch.int64)
        ends = torch.cumsum(lens, 0)
        total = int(ends[-1].item())
        if total > _lib.KMER_MAX_SLOTS:
            raise _lib.AtroposUnsupported("detect: %d kept bases of distinct reads (at most 2^31 - 1)" % total)
        tab, slot_rep, level = be.detect_kmer_slots(batch.records, kept, reps, (ends - lens).contiguous(), total, k0)
        clock.stop("distinct")
        cls, classes = self._ranks_at_k0(be, tab, slot_rep, batch.data, total, clock)
        # the level loop: one read-back of the state block per level
        cap = self.CAPACITY
        state, cand = be.detect_kmer_state(cap)
        slot_list, n, k = None, total, k0
        cls_prev = cand_of_prev = spare = None
        over = {}
        while True:
            cand_of = be.detect_kmer_level(tab, slot_rep, slot_list, n, cls, cls_prev, classes, cand_of_prev, k,
                                           self.min_count(k), level, cand, cap, state)
            list_next, keys_next = be.detect_kmer_next(tab, slot_rep, slot_list, n, cls, batch.data, level, k, state)
            words = state.cpu()
            if int(words[_lib.KMER_S_CANDIDATES]) > cap:
                raise _lib.AtroposUnsupported("detect: more than %d over-represented k-mers (the merge is quadratic in "
                                              "them); raise kmer_size or min_frequency" % cap)
            over[k] = int(words[_lib.KMER_S_OVER + k])
            n_next = int(words[_lib.KMER_S_SURVIVORS])
            if over[k] == 0:
                levels = k
                break
            if n_next == 0:                                   # no read is long enough for a (k + 1)-mer
                levels = k + 1
                over[k + 1] = 0
                break
            sk, si = torch.sort(keys_next[:n_next])
            cls_new = spare if spare is not None else be.empty((max(total, 1),), torch.int32)
            slot_list = list_next[:n_next]
            classes = be.detect_kmer_rank(sk, si, slot_list, cls_new)[:3]
            spare, cls_prev, cls, cand_of_prev = cls_prev, cls, cls_new, cand_of
            n, k = n_next, k + 1
        clock.stop("levels")
        ncand = int(words[_lib.KMER_S_CANDIDATES])
        rows = cand[:ncand].cpu().numpy()
        texts = []
        if ncand:
            text_off = np.zeros((ncand + 1,), np.int64)
            np.cumsum(rows[:, _lib.KMER_C_LEVEL], out=text_off[1:])
            packed = be.detect_kmer_gather(tab, nrep, batch.data, cand, torch.from_numpy(text_off).to(cand.device))
            raw = packed.cpu().numpy().tobytes()
            texts = [raw[text_off[i]:text_off[i + 1]] for i in range(ncand)]
        clock.stop("gather")
        self.timings = clock.seconds
        self._found = dict(kept=int(host[0]), distinct=int(host[1]), levels=levels, over=over, rows=rows, texts=texts,
                           nrep=nrep, tab=tab, slot_rep=slot_rep, level=level, batch=batch, kept_t=kept)
        return self._found

    def counters(self, **kwargs):
        """``kept`` and ``distinct`` as the known detector's ``counters`` names them."""
        found = self.discover(**kwargs)
        return dict(kept=found["kept"], distinct=found["distinct"])

    def candidates(self):
        """{text: count} of the candidates the reference would hold in ``results`` before the merge, in the order of
        the tie rule: the over-represented k-mers of every level but the last non-empty one, without those the
        reference's ``seq in cur`` test drops and those of complexity <= 1.0."""
        found = self.discover()
        last = found["levels"] - 1
        picked = []
        for row, text in zip(found["rows"], found["texts"]):
            if int(row[_lib.KMER_C_LEVEL]) >= last or int(row[_lib.KMER_C_QUIRK]):
                continue
            seq = text.decode("latin-1")
            if sequence_complexity(seq) > 1.0:
                picked.append((int(row[_lib.KMER_C_LEVEL]), int(row[_lib.KMER_C_REP]), int(row[_lib.KMER_C_OFFSET]), seq,
                               int(row[_lib.KMER_C_COUNT])))
        picked.sort(key=lambda c: c[:3])
        return {seq: count for _, _, _, seq, count in picked}

    def support(self, sequences):
        """(abundance, longest_match) per sequence: the distinct reads that hold it, and ``(text, seqlen)`` by the tie
        rule of the module doc (None when no read of its level holds it)."""
        found = self.discover()
        be = self.backend
        out = []
        for at in range(0, len(sequences), _lib.KMER_MAX_PATTERNS):
            part = sequences[at:at + _lib.KMER_MAX_PATTERNS]
            abundance, words = be.detect_kmer_support(found["tab"], found["nrep"], found["batch"].data, found["level"],
                                                      [s.encode("latin-1") for s in part])
            for seq, ab, word in zip(part, abundance.tolist(), words.tolist()):
                longest = None
                if word != -1:
                    first, rec = (word >> 32) & 0xFFFFFFFF, word & 0xFFFFFFFF
                    row = found["batch"].records[rec].cpu().tolist()
                    off, kl = row[2] & 0xFFFFFFFF, int(found["kept_t"][rec].item())
                    text = bytes(found["batch"].data[off + first:off + kl].cpu().tolist()).decode("latin-1")
                    longest = (text, len(seq) - first)
                out.append((int(ab), longest))
        return out

    # -- the host side ----------------------------------------------------------------------------------------
    def _get_contaminants(self):
        results = merge_candidates(list(self.candidates().items()))
        if not results:
            return []
        support = self.support([x[0] for x in results])
        matches = [HeuristicMatch(x[0], count=x[1], abundance=ab, longest_match=lm) for x, (ab, lm) in zip(results, support)]
        if not self.known_contaminants:
            return matches
        with _lib.thread_backend(self.backend):               # (the aligners of the known matching live on this backend)
            return self._match_known(matches)

    def _match_known(self, matches):
        """Matching against the known sequences (:664-743)."""
        from .util import reverse_complement
        contaminants = [_KnownMatcher(seq, names, self.kmer_size) for seq, names in self.known_contaminants.iter_sequences()]
        known = {}
        unknown = []

        def find_best_match(match, seq, best_matches, best_match_frac):
            try:
                seqrc = reverse_complement(seq)
            except KeyError as err:
                raise ValueError("candidate %r holds %s, a base without a complement (the reference raises KeyError)"
                                 % (seq, err))
            for contam in contaminants:
                match_frac1, match_frac2, compare_seq = contam.match(seq, seqrc)
                if match_frac1 < best_match_frac[0]:
                    continue
                if contam.seq in compare_seq or _align(compare_seq, contam.seq, self.min_contaminant_match_frac):
                    if match_frac1 > best_match_frac[0] or (
                            match_frac1 == best_match_frac[0] and match_frac2 > best_match_frac[1]):
                        best_matches = {}
                        best_match_frac = (match_frac1, match_frac2)
                    best_matches[contam] = (match, (match_frac1, match_frac2))
            return best_matches, best_match_frac

        for match in matches:
            best_matches, best_match_frac = find_best_match(match, match.seq, {}, (self.min_contaminant_match_frac, 0))
            if match.longest_match:
                best_matches, best_match_frac = find_best_match(match, match.longest_match[0], best_matches, best_match_frac)
            if best_matches:
                for contam, found in best_matches.items():
                    if contam not in known or found[1] > known[contam][1]:
                        known[contam] = found
            else:
                unknown.append(match)
        # resolve many-many relationships
        new_matches = {}
        for contam, (match, match_frac) in known.items():
            new_matches.setdefault(match, []).append((contam, match_frac))
        known = []
        for match, contams in new_matches.items():
            contams.sort(key=lambda x: x[1], reverse=True)
            contam, match_frac = contams[0]
            equiv = [other for other in contams[1:] if other[1] == match_frac]
            if len(equiv) == 0:
                match.set_known(sorted(contam.names), [contam.seq], *match_frac)
            else:
                names = set(contam.names)
                seqs = {(contam.seq,)}
                for other in equiv:
                    names.update(other[0].names)
                    seqs.add(other[0].seq)
                match.set_known(sorted(names), sorted(seqs, key=repr), *match_frac)
            known.append(match)
        return known + unknown

    def matches(self, min_len=None, min_complexity=1.1, min_match_frac=0.1, limit=20):
        """``Detector.matches`` / ``_filter_and_sort`` (:382-443) with ``min_report_freq = 0.1 * n_reads``."""
        min_len = self.kmer_size if min_len is None else min_len
        if self._read_length is None:
            return []
        found = self._get_contaminants()

        def keep(m):
            if m.count < self.min_report_freq:
                return False
            if min_len and len(m) < min_len:
                return False
            if min_complexity and m.seq_complexity < min_complexity:
                return False
            if self.include == "known" and not m.is_known:
                return False
            if self.include == "unknown" and m.is_known:
                return False
            if min_match_frac and m.is_known and m.match_frac < min_match_frac:
                return False
            return True

        found = [m for m in found if keep(m)]
        found.sort(key=_sort_key, reverse=True)
        return found if limit is None else found[:limit]

    def _args_summary(self):
        out = dict(kmer_size=self.kmer_size, n_reads=self.reads if self.n_reads is None else self.n_reads,
                   overrep_cutoff=self.overrep_cutoff, include=self.include, past_end_bases=self.past_end_bases)
        if self.known_contaminants:
            out["known_contaminants"] = self.known_contaminants.summarize()
        return out

    def summarize(self, **kwargs):
        """The reference's ``summary['detect']``."""
        out = self._args_summary()
        out["matches"] = ([m.summarize() for m in self.matches(**kwargs)],)
        return out


DETECTORS = {"known": KnownContaminantDetector, "heuristic": HeuristicDetector}


class PairedDetector(object):
    """Two independent detectors, one per read of the pair (``PairedDetector``, :461-492)."""

    def __init__(self, known_contaminants, detector_class=KnownContaminantDetector, **kwargs):
        self.read1_detector = detector_class(known_contaminants, **kwargs)
        self.read2_detector = detector_class(known_contaminants, **kwargs)

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


def _detector_class(kwargs):
    name = kwargs.pop("detector", "known")
    if name not in DETECTORS:
        raise ValueError("detector must be one of %s" % ", ".join(sorted(DETECTORS)))
    return DETECTORS[name]


def detect_file(path, known_contaminants=None, max_reads=10000, chunk_bytes=64 << 20, **kwargs):
    """``atropos detect`` of one FASTQ file, read in chunks, stopping after ``max_reads`` records (None: the whole
    file, which must fit one batch -- see the module doc).  ``detector="known"`` (the default; it needs
    ``known_contaminants``) or ``"heuristic"`` (the list is optional); the other keywords are the detector's.
    ``n_reads`` defaults to ``max_reads``.  Returns the reference's ``summary['detect']`` dict; ``matches`` is a
    1-tuple of lists.  ``device_gunzip=True`` (here and in ``detect_files``): BGZF ``.gz`` input is inflated on the GPU."""
    return _detect_paths([path], _detector_class(kwargs), known_contaminants, max_reads, chunk_bytes, kwargs)


def detect_files(path1, path2, known_contaminants=None, max_reads=10000, chunk_bytes=64 << 20, **kwargs):
    """The same for paired files: ``matches`` is a 2-tuple of lists, one per read.  ``path2=None``: ``path1`` is an
    interleaved file (the reference's ``-l``), as in ``trim_files``; ``max_reads`` counts pairs either way."""
    paths = [path1] if path2 is None else [path1, path2]
    kwargs["detector_class"] = _detector_class(kwargs)
    return _detect_paths(paths, PairedDetector, known_contaminants, max_reads, chunk_bytes, kwargs, interleaved=path2 is None)


def _parse_detect_args(argv, heuristic):
    """The options of ``atropos detect`` the device path covers, with the spellings and defaults of
    commands/detect/cli.py; ``heuristic``: with the two options of the heuristic detector."""
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
    if heuristic:
        ap.add_argument("--min-frequency", default=0.001, type=float)
        ap.add_argument("--min-contaminant-match-frac", default=0.9, type=float)
    try:
        opts, rest = ap.parse_known_args(list(argv))
    except SystemExit:
        raise ValueError("detect: cannot parse %r" % (list(argv),))
    if rest:
        raise NotImplementedError("detect: option(s) outside the device path: %s" % " ".join(rest))
    if opts.kmer_size < 1:
        raise ValueError("--kmer-size must be positive")
    if not 0 <= opts.min_kmer_match_frac <= 1:
        raise ValueError("--min-kmer-match-frac must lie in 0 .. 1")
    return opts


def _known_from_opts(opts):
    known = KnownContaminants()
    for item in opts.known_adapter or ():
        name, seq = item.split("=")
        known.add(name, seq)
    for path in opts.known_adapters_file or ():
        if "://" in path and not path.startswith("file:"):
            raise NotImplementedError("fetching a contaminant list from a URL")
        known.load_from_fasta(path[5:] if path.startswith("file:") else path)
    return known


def detect_from_args(argv, paired=False):
    """Build the known-contaminant detector from the subset of ``atropos detect`` options its device path covers (same
    spellings and defaults as commands/detect/cli.py): ``-d/--detector known``, ``-k/--kmer-size``, ``--max-reads``,
    ``-e/--past-end-bases``, ``-i/--include-contaminants``, ``-x/--known-contaminant name=SEQ``,
    ``-F/--known-contaminants-file``, ``--min-kmer-match-frac``.  Returns a ``KnownContaminantDetector`` (``paired``:
    a ``PairedDetector``) whose ``n_reads`` is ``--max-reads``.  Anything else raises; the heuristic detector and the
    reference's choice between the detectors are ``detector_from_args``'."""
    opts = _parse_detect_args(argv, heuristic=False)
    detector = opts.detector
    if detector is None and opts.include_contaminants == "known":
        detector = "known"
    if detector == "heuristic" or detector is None:
        raise NotImplementedError("detect_from_args builds the known-contaminant detector only; detector_from_args "
                                  "builds the heuristic one as well (or pass --detector known)")
    if detector == "khmer":
        raise NotImplementedError("the khmer detector (a third-party probabilistic counter)")
    known = _known_from_opts(opts)
    if not len(known):
        raise NotImplementedError("the default contaminant list (it is fetched from a URL); pass --known-contaminant "
                                  "or --known-contaminants-file")
    kwargs = dict(kmer_size=opts.kmer_size, n_reads=opts.max_reads, include=opts.include_contaminants,
                  past_end_bases=tuple(opts.past_end_bases), min_kmer_match_frac=opts.min_kmer_match_frac)
    return PairedDetector(known, **kwargs) if paired else KnownContaminantDetector(known, **kwargs)


def detector_from_args(argv, paired=False):
    """Every option of ``detect_from_args`` plus ``--min-frequency`` and ``--min-contaminant-match-frac``, and the
    reference's choice of the detector (``CommandRunner.__call__``, :64-71): the one ``-d`` names; else ``known`` with
    ``-i known`` and a list, ``heuristic`` for ``--max-reads <= 50000``, and where the reference would take ``khmer``
    a ``NotImplementedError`` that names ``-d heuristic``.  The heuristic detector needs no known list (with
    ``-i unknown`` a list given is not used, as in the reference)."""
    opts = _parse_detect_args(argv, heuristic=True)
    include = opts.include_contaminants
    known = _known_from_opts(opts) if include != "unknown" else KnownContaminants()
    detector = opts.detector
    if not detector:
        if len(known) and include == "known":
            detector = "known"
        elif opts.max_reads <= 50000:
            detector = "heuristic"
        else:
            detector = "khmer"
    common = dict(kmer_size=opts.kmer_size, n_reads=opts.max_reads, include=include, past_end_bases=tuple(opts.past_end_bases))
    if detector == "khmer":
        raise NotImplementedError("the khmer detector (a third-party probabilistic counter), which the reference takes "
                                  "above 50000 reads; pass -d heuristic (or -d known with a list)")
    if detector == "known":
        if not len(known):
            raise NotImplementedError("the default contaminant list (it is fetched from a URL); pass --known-contaminant "
                                      "or --known-contaminants-file")
        kwargs = dict(common, min_kmer_match_frac=opts.min_kmer_match_frac)
    else:
        if not 0 <= opts.min_contaminant_match_frac <= 1:
            raise ValueError("--min-contaminant-match-frac must lie in 0 .. 1")
        kwargs = dict(common, min_frequency=opts.min_frequency, min_contaminant_match_frac=opts.min_contaminant_match_frac)
    cls = DETECTORS[detector]
    known = known if len(known) else None
    return PairedDetector(known, detector_class=cls, **kwargs) if paired else cls(known, **kwargs)

"""The trim report: ``summary['trim']`` of the reference (RecordHandler.summarize, commands/trim/__init__.py:129-137)
and the input totals ``Pipeline.finish`` writes (commands/base.py:98-110), counted on the device while a trim pipeline
built with ``report=True`` runs.

Every read of the layout has one resident block of int64 counters (atr_report_*, csrc/report_core.hpp).  The stages of
``atropos_amd.trim`` add to it as they go -- a trimmer stage the bases it counts as trimmed, an adapter round the
(side, length, errors) bin of every match and the base before a 3' match, the end of a run the destinations, the
written bases and the input totals -- and ``summary()`` copies the blocks to the host, once.  ``TrimReport`` is what
``trim_file`` / ``trim_files`` use and what a caller of ``pipe.run(batch)`` uses:

    rep = TrimReport(pipe)
    for batch in batches:
        rep.add(pipe.run(batch))
    summary = rep.summary()
    rep.close()

Modifier names and descriptions are restated here as data.  Not covered (refused when the pipeline is built, see
``check_envelope``): linked adapters, the insert aligner, --merge-overlapping, --bisulfite; report writers, the
multiprocess merge of summaries, timing and the echo of the options are no part of it.
"""
from . import _lib
from .adapters import ANYWHERE, BACK, FRONT, PREFIX, SUFFIX, where_int_to_dict

# the slot of a trimmer stage in the counter block; (class name, description) of the reference's modifiers
SLOT_CUT, SLOT_NEXTSEQ, SLOT_QUALITY, SLOT_NEND, SLOT_MINCUT = range(5)
TRIMMERS = {SLOT_CUT: ("UnconditionalCutter", "Cut unconditionally"),
            SLOT_NEXTSEQ: ("NextseqQualityTrimmer", "Quality trimmed (NextSeq)"),
            SLOT_QUALITY: ("QualityTrimmer", "Quality-trimmed"),
            SLOT_NEND: ("NEndTrimmer", "End Ns trimmed"),
            SLOT_MINCUT: ("MinCutter", "Cut conditionally")}
# destination -> the name of the filter that sends reads there (filters.py: FilterWrapper.name)
FILTER_NAMES = {_lib.DEST_TOO_SHORT: "too_short", _lib.DEST_TOO_LONG: "too_long", _lib.DEST_TOO_MANY_N: "too_many_n",
                _lib.DEST_TRIMMED: "TrimmedFilter", _lib.DEST_UNTRIMMED: "UntrimmedFilter"}
OUTPUT_DESTS = {"too_short": _lib.DEST_TOO_SHORT, "too_long": _lib.DEST_TOO_LONG, "untrimmed": _lib.DEST_UNTRIMMED}


def check_envelope(linked=False, aligner="adapter", merge_overlapping=False, bisulfite=False):
    """What a pipeline with ``report=True`` refuses, when it is built."""
    for flag, what in ((linked, "linked adapters (a LinkedMatch counts into its two parts)"),
                       (aligner != "adapter", "--aligner insert (InsertAdapterCutter's summary)"),
                       (merge_overlapping, "--merge-overlapping (MergeOverlapping's summary, the merged-read filter)"),
                       (bisulfite, "--bisulfite (the bisulfite trimmers' own counters)")):
        if flag:
            raise NotImplementedError("report: " + what + " is outside the device trim report")


class _MateReport(object):
    """The counter block of one read of the layout and the launches that add to it.  ``pipe``: the TrimPipeline that
    modifies the read, or None for the second read of the legacy mode (written as it came)."""

    def __init__(self, pipe, backend, max_read_len, variant):
        self.pipe, self.be = pipe, backend
        self.adapters = list(pipe.adapters) if pipe is not None else []
        self.variant = _lib.REPORT_VARIANTS[variant]
        # Adapter.match_to accepts errors up to max_error_rate * (aligned adapter bases) <= rate * len(adapter)
        max_errors = max([int(len(a.sequence) * a.max_error_rate) + 1 for a in self.adapters] or [0])
        if max_read_len is None:
            # every read the pipeline takes (split_long: 32 736 bases), or as many bases as the bound of the block
            # (REPORT_MAX_WORDS) leaves each of the adapters' tables
            fit = (_lib.REPORT_MAX_WORDS - _lib.REPORT_HDR) // max(len(self.adapters), 1) - _lib.REPORT_ADJ
            max_read_len = max(0, min(_lib.MAX_LONG_READ_LEN, fit // (2 * (max_errors + 1)) - 1))
        try:
            self.handle = backend.report_create(len(self.adapters), int(max_read_len), max_errors)
        except _lib.AtroposUnsupported:
            raise _lib.AtroposUnsupported("report: the table of %d adapter(s) x %d bases x %d errors is beyond the bound of the "
                                          "counter block" % (len(self.adapters), max_read_len, max_errors))
        self.max_read_len, self.max_errors = int(max_read_len), max_errors
        self.counters = backend.report_counters(self.handle)

    def intervals(self, batch, before, begin, end, mode, front, back, slot):
        self.be.report_intervals(self.handle, batch.records, before[0], before[1], begin, end, mode, front, back, slot,
                                 self.counters)

    def adapter_round(self, batch, took, best, which, front, default_front, begin, end, longest):
        if longest > self.max_read_len:
            raise _lib.AtroposUnsupported("report: a read of %d bases is beyond the %d bases the tables of %d adapter(s) hold "
                                          "within the bound of the counter block" % (longest, self.max_read_len, len(self.adapters)))
        self.be.report_adapters(self.handle, batch.data, batch.records, took, best, which, front, default_front, begin, end,
                                longest, 2 if self.pipe.action == "mask" else 1, self.variant, self.counters)

    def outputs(self, res):
        self.be.report_outputs(self.handle, res.batch.records, res.begin, res.end, res.matched, res.dest, self.counters)

    def close(self):
        if self.handle is not None:
            self.be.report_destroy(self.handle)
            self.handle = None

    # ---------------------------------------------------------------------------------------------- host side
    def adapter_summaries(self, words):
        """{adapter name: what Adapter.summarize returns} from the block (adapters/__init__.py:474-505)."""
        L, E = self.max_read_len, self.max_errors
        per = _lib.REPORT_ADJ + 2 * (L + 1) * (E + 1)
        out = {}
        for k, adapter in enumerate(self.adapters):
            base = _lib.REPORT_HDR + k * per
            hist = words[base + _lib.REPORT_ADJ:base + per].reshape(2, L + 1, E + 1)
            lengths, errors = [{}, {}], [{}, {}]
            for side, length, err in zip(*hist.nonzero()):
                count = int(hist[side, length, err])
                lengths[side][int(length)] = lengths[side].get(int(length), 0) + count
                errors[side].setdefault(int(length), {})[int(err)] = count
            adjacent = dict(zip(("A", "C", "G", "T", ""), (int(v) for v in words[base:base + 5])))
            n_front, n_back = sum(lengths[0].values()), sum(lengths[1].values())
            where = adapter.where
            stats = {"adapter_class": type(adapter).__name__, "total_front": n_front, "total_back": n_back,
                     "total": n_front + n_back, "match_probabilities": adapter.random_match_probabilities(),
                     "where": where_int_to_dict(where), "sequence": adapter.sequence, "max_error_rate": adapter.max_error_rate}
            if where in (ANYWHERE, FRONT, PREFIX):                           # adapters/__init__.py:496-503
                stats["lengths_front"], stats["errors_front"] = lengths[0], errors[0]
            if where in (ANYWHERE, BACK, SUFFIX):
                stats["lengths_back"], stats["errors_back"] = lengths[1], errors[1]
            if where in (BACK, SUFFIX):
                stats["adjacent_bases"] = adjacent
            out[adapter.name] = stats
        return out

    def modifier_summaries(self, words, present):
        """{modifier name: (description, what its summarize() returns)} of this read; ``present``: the trimmer slots
        the reference gives this read a modifier for."""
        out = {}
        if self.adapters:
            out["AdapterCutter"] = ("AdapterCutter", {"records_with_adapters": int(words[_lib.REPORT_WITH_ADAPTERS]),
                                                      "adapters": self.adapter_summaries(words)})
        for slot in present:
            name, desc = TRIMMERS[slot]
            out[name] = (desc, {"bp_trimmed": int(words[_lib.REPORT_TRIM + slot])})
        return out


class TrimReport(object):
    """The report of the runs of ``pipe`` (a TrimPipeline, PairedTrimPipeline or LegacyPairedPipeline built with
    ``report=True``) between its construction and ``close()``.  ``source``: what keys the input totals (trim_file:
    the input path; trim_files: the tuple of the two).  ``max_read_len``: the longest read the adapter tables hold (default:
    every read the pipeline takes, 32 736 bases, or what the bound of the counter block leaves a large adapter set);
    ``variant``: 'auto' | 'lds' | 'global', how an adapter round counts (atr_report_adapters)."""

    def __init__(self, pipe, source=0, max_read_len=None, variant="auto"):
        if not getattr(pipe, "report", False):
            raise ValueError("TrimReport needs a pipeline built with report=True")
        self.pipe, self.source = pipe, source
        self.legacy = hasattr(pipe, "first")
        self.paired = hasattr(pipe, "p1")
        pipes = [pipe.first, None] if self.legacy else ([pipe.p1, pipe.p2] if self.paired else [pipe])
        be = _lib.get_backend()
        self.mates, self.batches = [], 0
        try:
            for p in pipes:
                self.mates.append(_MateReport(p, be, max_read_len, variant))
        except Exception:
            self.close()
            raise
        for p, mate in zip(pipes, self.mates):
            if p is not None:
                if p._reporter is not None:
                    self.close()
                    raise ValueError("the pipeline already has a TrimReport; close() it first")
                p._reporter = mate

    def add(self, result):
        """Count what ``pipe.run`` returned: destinations, written bases, input totals."""
        reads = (result.read1, result.read2) if self.paired else (result,)
        self.batches += len(result.dest) > 0
        for mate, res in zip(self.mates, reads):
            mate.outputs(res)

    def close(self):
        for mate in self.mates:
            if mate.pipe is not None and mate.pipe._reporter is mate:
                mate.pipe._reporter = None
            mate.close()

    def summary(self):
        """The blocks, copied to the host once each, as the reference's dicts."""
        words = [m.be.report_read(m.handle, m.counters) for m in self.mates]
        if any(int(w[_lib.REPORT_OVERFLOW]) for w in words):
            raise _lib.AtroposUnsupported("report: %d adapter match(es) fell outside the table (length or errors); the "
                                          "counts would be wrong" % sum(int(w[_lib.REPORT_OVERFLOW]) for w in words))
        first = self.mates[0].pipe
        pipes = [m.pipe for m in self.mates]
        both = [p for p in pipes if p is not None]
        # which read gets which trimmer (trim/__init__.py:477-524): a pair of cutters when either read has lengths,
        # the quality / N trimmers on every read that is modified
        present = []
        if "C" in first.op_order and any(p.cut_front or p.cut_back for p in both):
            present.append(SLOT_CUT)
        if "G" in first.op_order and first.nextseq_trim is not None:
            present.append(SLOT_NEXTSEQ)
        if "Q" in first.op_order and first.quality_cutoff:
            present.append(SLOT_QUALITY)
        if first.trim_n:
            present.append(SLOT_NEND)
        if any(p.min_front or p.min_back for p in both):
            present.append(SLOT_MINCUT)
        per_mate = [m.modifier_summaries(w, present) if m.pipe is not None else None for m, w in zip(self.mates, words)]
        modifiers = {}
        if not self.paired:                                              # SingleEndModifiers.summarize, modifiers.py:1053-1061
            for name, (desc, summ) in per_mate[0].items():
                modifiers[name] = dict({key: (value,) for key, value in summ.items()}, desc=desc)
            for flag, name in ((first.length_tag, "LengthTagModifier"), (first.strip_suffix, "SuffixRemover"),
                               (first.prefix or first.suffix, "PrefixSuffixAdder"), (first.zero_cap, "ZeroCapper")):
                if flag:
                    modifiers[name] = {"desc": name}                     # (no summary of their own, no display_str)
        else:                                                            # PairedEndModifiers.summarize, :1107-1138
            names = list(per_mate[0]) + [n for n in (per_mate[1] or {}) if n not in per_mate[0]]
            for name in names:
                summs = [(pm or {}).get(name) for pm in per_mate]
                desc, keys = next((s[0], list(s[1])) for s in summs if s is not None)
                modifiers[name] = dict({key: tuple(None if s is None else s[1][key] for s in summs) for key in keys}, desc=desc)
        w1 = words[0]
        filters = {}
        for code, flag in ((_lib.DEST_TOO_SHORT, first.minimum_length is not None and first.minimum_length > 0),
                           (_lib.DEST_TOO_LONG, first.maximum_length is not None), (_lib.DEST_TOO_MANY_N, first.max_n is not None),
                           (_lib.DEST_TRIMMED, first.discard_trimmed), (_lib.DEST_UNTRIMMED, first.discard_untrimmed)):
            if flag:
                filters[FILTER_NAMES[code]] = {"records_filtered": int(w1[_lib.REPORT_DEST + code])}
        # every sequence formatter that wrote a record (writers.py:130-170): the main output and the side outputs
        written = [_lib.DEST_KEEP] + [OUTPUT_DESTS[kind] for kind in self.pipe.outputs]
        formatters = {"records_written": sum(int(w1[_lib.REPORT_DEST + d]) for d in written),
                      "bp_written": [sum(int(w[_lib.REPORT_DEST_BP + d]) for d in written) for w in words] + [0] * (2 - len(words))}
        records = int(w1[_lib.REPORT_IN_RECORDS])
        bp = [int(w[_lib.REPORT_IN_BASES]) for w in words] + [0] * (2 - len(words))
        out = {"trim": {"modifiers": modifiers, "filters": filters, "formatters": formatters},
               "record_counts": {self.source: records}, "total_record_count": records,
               "bp_counts": {self.source: bp}, "total_bp_counts": tuple(bp), "sum_total_bp_count": sum(bp)}
        if not self.batches:                                             # (Pipeline.process_batch never saw a source)
            out.update(record_counts={}, bp_counts={}, total_bp_counts=())
        return out

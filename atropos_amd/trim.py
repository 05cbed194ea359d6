"""Device-resident trimming pipeline, single-end and paired-end: FASTQ bytes in, trimmed FASTQ bytes out.

This is the batched, stage-wise replacement for the reference's per-read loop
``RecordHandler.handle_record`` -> ``Modifiers.modify`` -> ``Filters.filter`` ->
``Formatters.format`` (atropos/commands/trim/__init__.py:122-127, :422-601;
commands/base.py:65-78): every stage is ONE kernel launch over the whole batch.

Stages, in the order the reference's ``op_order`` (default "CGQAW") and the fixed tail of
``trim/__init__.py`` apply them:

  C  UnconditionalCutter            -> atr_clip_batch
  G  NextseqQualityTrimmer          -> atr_quality_trim_batch(nextseq=1)
  Q  QualityTrimmer                 -> atr_quality_trim_batch
  A  AdapterCutter(times, action)   -> atr_pack_records + atr_locate_batch + atr_adapter_postfilter
                                       + atr_match_trim_batch per round (plain or linked adapters)
     InsertAdapterCutter (paired)   -> the insert aligner + atr_insert_plan_batch (with error correction)
  -  bisulfite trimmers (--bisulfite), then NEndTrimmer (--trim-n), then MinCutter (--cut-min)
                                    -> interval arithmetic; atr_nend_trim_batch
  -  filters (-m, -M, --max-n, --discard-trimmed/-untrimmed) -> atr_read_filter_batch (+ atr_pair_filter_batch)
  -  MergeOverlapping (-R, paired)  -> atr_locate_pairs_batch + atr_merge_plan_batch + atr_merge_emit_batch
  -  ZeroCapper (-z) and the read-name modifiers (length tag, suffix removal, prefix / suffix)
  -  FastqFormat                    -> atr_fastq_emit
  W  OverwriteRead (-w, paired)     -> atr_overwrite_plan_batch + atr_overwrite_apply_batch
  -  InterleavedFormatter (-L)      -> atr_fastq_emit_pairs (interleaved input, -l, is fastq.read_chunks' business)
  -  Formatters (``{name}`` in the output path: one file per adapter name)
                                    -> atr_demux_groups + atr_fastq_emit_grouped

Paired-end input runs in "both" mode (``PairedTrimPipeline``) or in the reference's legacy mode
(``LegacyPairedPipeline``).  ``trim_file`` / ``trim_files`` also write the info / rest / wildcard files and the
too-short / too-long / untrimmed outputs, and make the --stats pre / post summaries.  What the pipeline does not
cover (options ``pipeline_from_args`` does not know, and the combinations the constructors refuse) raises instead
of silently differing; those stay on the per-read object path (``atropos_amd.modifiers``).
"""
import time

import torch

from . import _lib
from .adapters import LinkedAdapter
from .report import SLOT_CUT, SLOT_MINCUT, SLOT_NEND, SLOT_NEXTSEQ, SLOT_QUALITY, TrimReport, check_envelope
from .fastq import (FastaBatch, FastqBatch, RecordSource, StageClock, guess_format, input_format, make_sink, open_by_extension,
                    read_chunks, sniff_format)

DEST_MERGED = 6              # MergedReadFilter (filters.py:109-113): installed first, so a merged pair goes nowhere else
DEST_NAMES = {_lib.DEST_KEEP: "keep", _lib.DEST_TOO_SHORT: "too_short", _lib.DEST_TOO_LONG: "too_long",
              _lib.DEST_TOO_MANY_N: "too_many_n", _lib.DEST_TRIMMED: "trimmed", _lib.DEST_UNTRIMMED: "untrimmed"}


# the names the reference's --stats post keys its destinations by (dest.name, commands/trim/filters.py); the
# trimmed / untrimmed filters have none
POST_STATS_NAMES = {_lib.DEST_KEEP: "NoFilter", _lib.DEST_TOO_SHORT: "too_short", _lib.DEST_TOO_LONG: "too_long",
                    _lib.DEST_TOO_MANY_N: "too_many_n"}


def _stats_modes(stats):
    modes = (stats,) if isinstance(stats, str) else tuple(stats or ())
    if any(m not in ("pre", "post") for m in modes):
        raise ValueError("stats must be a sequence of 'pre' and 'post'")
    return modes


class TrimStats(object):
    """``atropos trim --stats pre|post|both`` (StatsRecordHandlerWrapper, commands/trim/__init__.py:140-205) over
    the device state of a run: pre-trim statistics of every chunk before the first stage, post-trim statistics of
    what each destination receives, per destination name."""

    def __init__(self, modes, paired, quality_base):
        from . import stats as S
        cls = S.PairedEndReadStatistics if paired else S.SingleEndReadStatistics
        self.make = lambda: cls(qualities=True, quality_base=quality_base)
        self.pre = self.make() if "pre" in modes else None
        self.post = {} if "post" in modes else None

    def add_post(self, counts, collect):
        """``counts``: {destination name: reads} of a chunk; ``collect(stats, code)`` adds destination ``code``."""
        if self.post is None:
            return
        codes = {name: code for code, name in DEST_NAMES.items()}
        for name, v in counts.items():
            if not v:
                continue
            if name == "merged":
                raise NotImplementedError("post-trim statistics of merged pairs (the reference collects them with "
                                          "read2 = None and fails)")
            code = codes[name]
            if code not in POST_STATS_NAMES:
                raise NotImplementedError("post-trim statistics of the reads the %s filter takes (the reference's "
                                          "filter has no name)" % name)
            key = POST_STATS_NAMES[code]
            if key not in self.post:
                self.post[key] = self.make()
            collect(self.post[key], code)

    @staticmethod
    def check(modes, discard_trimmed, discard_untrimmed, merging):
        """Refuse post-trim statistics the reference cannot make, before any output is opened."""
        if "post" not in modes:
            return
        if merging:
            raise NotImplementedError("post-trim statistics of merged pairs (the reference collects them with "
                                      "read2 = None and fails)")
        if discard_trimmed or discard_untrimmed:
            raise NotImplementedError("post-trim statistics with --discard-trimmed / --discard-untrimmed / "
                                      "--untrimmed-output (the reference's trimmed / untrimmed filters have no name)")

    def summary(self):
        out = {}
        if self.pre is not None:
            out["pre"] = {0: self.pre.summarize()}
        if self.post is not None:
            out["post"] = {name: {0: st.summarize()} for name, st in self.post.items()}
        return out


def write_mask(batch, begin, end, ubegin, uend):
    """'N' over the masked parts [begin, ubegin) and [uend, end) of every sequence line of the chunk: after it the
    read IS what AdapterCutter's 'mask' action returns (modifiers.py:155-172), for the stages that look at bases."""
    off = batch.records[:, 2].to(torch.int64) & 0xFFFFFFFF
    for lo, hi in ((begin, torch.minimum(ubegin, end)), (torch.maximum(uend, begin), end)):
        lens = (hi - lo).clamp(min=0).to(torch.int64)
        total = int(lens.sum().item())
        if total == 0:
            continue
        first = torch.cumsum(lens, 0) - lens
        idx = torch.repeat_interleave(off + lo.to(torch.int64) - first, lens) + torch.arange(total, device=off.device)
        batch.data[idx] = ord("N")


def mask_before_later_stages(op_order, action):
    """A 'mask' adapter stage followed by a stage that reads bases (NextSeq trimming looks for G's): the N's must be in
    the chunk before that stage runs."""
    return action == "mask" and "A" in op_order and any(op in "GQ" for op in op_order[op_order.index("A") + 1:])


def _raise_device_error(err):
    """The exception the reference raises for the error word of the insert or merge kernels (pair * 8 + kind)."""
    if err == _lib.INT64_MAX:
        return
    if err % 8 == 4:
        raise ValueError("Invalid alignment while trying to merge pair %d" % (err // 8))
    exc = {1: KeyError, 2: IndexError, 3: ValueError}[err % 8]
    raise exc("error correction of pair %d: %s" % (err // 8, {
        1: "base without a complement", 2: "overlap outside a read",
        3: "Cannot determine the mode of an empty sequence"}[err % 8]))


class TrimResult(object):
    """State of a batch after the pipeline: kept interval per read, the destination filter
    and the adapter flag; all device tensors."""

    def __init__(self, batch, begin, end, ubegin, uend, matched, dest, rounds=None, adapters=None, read_batch=None):
        self.batch, self.begin, self.end, self.ubegin, self.uend = batch, begin, end, ubegin, uend
        self.matched, self.dest = matched, dest
        self.rounds, self.adapters = rounds, adapters           # adapter rounds kept for the info / rest / wildcard files
        self.read_batch = read_batch or batch                   # the records as read (batch: after the read-name modifiers)
        # a demultiplexed run (TrimPipeline(demultiplex=True)): the output code of every read (int32, -1: not written
        # here) and the outputs' names -- the adapters' names, then "unknown" for the untrimmed output if there is one
        self.group, self.group_names = None, None
        self.fmt = getattr(batch, "fmt", "fastq")               # what ``text`` writes by default: "fasta" over a FastaBatch

    def aux_text(self, kinds=("info", "rest", "wildcard")):
        """The lines the reference's InfoFormatter / RestFormatter / WildcardFormatter write for this batch
        (commands/trim/writers.py:193-222; Match.get_info_record / rest / wildcards, align/__init__.py:117-170),
        every read in input order whatever its destination: {kind: bytes}.  Assembled on the host from the result
        arrays of the adapter rounds (the pipeline must have been built with ``aux``)."""
        lines = self.aux_lines(kinds)
        return {k: "".join(line + "\n" for per_read in v for line in per_read).encode("ascii", "replace")
                for k, v in lines.items()}

    def aux_lines(self, kinds=("info", "rest", "wildcard")):
        """{kind: one list of lines per read} (see aux_text; the paired-end result interleaves the two reads' lists)."""
        if self.rounds is None:
            raise ValueError("the pipeline was built without aux=(...): the adapter rounds were not kept")
        n = len(self.batch)
        raw = bytes(self.read_batch.data[:self.read_batch.nbytes].cpu().numpy().tobytes())
        recs = self.read_batch.records.cpu().numpy().astype("int64")
        recs[:, [0, 2, 4]] &= 0xFFFFFFFF                       # (offsets are unsigned 32-bit)
        final = self.batch.records.cpu().numpy().astype("int64")           # (an unmatched read's line carries its final name)
        final[:, [0, 4]] &= 0xFFFFFFFF
        raw_final = raw if self.batch is self.read_batch else bytes(self.batch.data.cpu().numpy().tobytes())
        fb, fe = self.begin.cpu().numpy(), self.end.cpu().numpy()
        rounds = [tuple(t.cpu().numpy() for t in r) for r in self.rounds]
        out = {k: [[] for _ in range(n)] for k in kinds}
        for i in range(n):
            name = raw[recs[i, 0]:recs[i, 0] + recs[i, 1]].decode("ascii", "replace")
            so, qo, has_q = int(recs[i, 2]), int(recs[i, 4]), recs[i, 5] > 0 or recs[i, 3] == 0
            last = None
            lines = []
            for took, rec, which, b0, e0 in rounds:
                if not took[i]:
                    continue
                ad = self.adapters[int(which[i])]
                astart, astop, rstart, rstop, _matches, errors = (int(v) for v in rec[i, :6])
                seq = raw[so + b0[i]:so + e0[i]].decode("ascii", "replace")
                qual = raw[qo + b0[i]:qo + e0[i]].decode("ascii", "replace") if has_q else ""
                last = (ad, astart, astop, rstart, rstop, seq)
                lines.append("\t".join(str(f) for f in (name, errors, rstart, rstop, seq[:rstart], seq[rstart:rstop], seq[rstop:],
                                                        ad.name, qual[:rstart], qual[rstart:rstop], qual[rstop:])))
            # (the name the read has when the files are written, i.e. after the read-name modifiers: the rest and wildcard
            # lines and an unmatched read's info line carry it; a match's info record was made before them)
            fname = raw_final[final[i, 0]:final[i, 0] + final[i, 1]].decode("ascii", "replace")
            if "info" in out:
                if last is None:
                    seq = raw[so + fb[i]:so + max(fb[i], fe[i])].decode("ascii", "replace")
                    # (an unmatched read's line is written from the read as it leaves the pipeline: zero-capped qualities)
                    fqo = int(final[i, 4])
                    qual = raw_final[fqo + fb[i]:fqo + max(fb[i], fe[i])].decode("ascii", "replace") if has_q else ""
                    lines = ["\t".join((fname, "-1", seq, qual))]
                out["info"][i] = lines
            if last is None:
                continue
            ad, astart, astop, rstart, rstop, seq = last
            front = ad._front_flag if ad._front_flag is not None else rstart == 0        # Match._guess_is_front
            if "rest" in out:
                rest = seq[:rstart] if front else seq[rstop:]
                if rest:
                    out["rest"][i].append(rest + " " + fname)
            if "wildcard" in out:
                chars = [seq[rstart + k] for k in range(astop - astart)
                         if ad.sequence[astart + k] == "N" and rstart + k < len(seq)]
                out["wildcard"][i].append("".join(chars) + " " + fname)
        return out

    def counts(self):
        c = torch.bincount(self.dest.to(torch.int64), minlength=6).cpu().tolist()
        return {DEST_NAMES[i]: int(c[i]) for i in range(6)}

    def demux_text(self):
        """What a demultiplexed run writes for this batch: {adapter name or "unknown": FASTQ text (bytes)}, the names
        that receive a read only.  One grouped emit (atr_fastq_emit_grouped), sliced by its segment boundaries."""
        if self.group is None:
            raise ValueError("the pipeline was built without demultiplex=True")
        text, edges = self.batch.backend.fastq_emit_grouped(self.batch.data, self.batch.records, self.begin, self.end,
                                                            self.ubegin, self.uend, self.group, len(self.group_names))
        host = text.cpu().numpy()
        out = {}
        for g, name in enumerate(self.group_names):
            if edges[g + 1] > edges[g]:
                out[name] = out.get(name, b"") + host[edges[g]:edges[g + 1]].tobytes()
        return out

    def text(self, which=_lib.DEST_KEEP, fmt=None):
        """Formatted text (bytes) of the reads sent to destination ``which``: ``fmt`` = "fastq" | "fasta", by default
        the format the batch was read from.  FASTQ of a FASTA batch is the reference's ValueError."""
        be = self.batch.backend
        fmt = fmt or self.fmt
        if fmt == "fastq" and self.fmt == "fasta":
            raise ValueError(NO_QUALITIES)
        emit = be.fasta_emit if fmt == "fasta" else be.fastq_emit
        out = emit(self.batch.data, self.batch.records, self.begin, self.end, self.ubegin, self.uend, self.dest, which)
        return bytes(out.cpu().numpy().tobytes())


NO_QUALITIES = "Output format cannot be FASTQ since no quality values are available."     # io/seqio.py:1053-1056


def output_format(path, fasta_input):
    """"fasta" | "fastq" for one output path, as the reference's ``get_format`` (io/seqio.py:1008-1067): by the path's
    own name; a name that says nothing gets FASTA when the input has no qualities and FASTQ otherwise; FASTQ by name
    for reads without qualities is its ValueError."""
    fmt = guess_format(path) or ("fasta" if fasta_input else "fastq")
    if fmt == "fastq" and fasta_input:
        raise ValueError(NO_QUALITIES)
    return fmt


def refuse_for_fasta(pipe):
    """What a pipeline cannot do with reads that have no qualities: the options the reference crashes on or needs
    qualities for are a ValueError naming the option, what is out of scope a NotImplementedError."""
    paired = _is_paired(pipe)
    first = pipe.p1 if paired else pipe
    second = getattr(pipe, "p2", None)
    pipes = [first] + ([second] if second is not None else [])
    for given, option in ((any(p.quality_cutoff for p in pipes), "-q / --quality-cutoff"),
                          (any(p.nextseq_trim is not None for p in pipes), "--nextseq-trim"),
                          (getattr(pipe, "overwrite_low_quality", None), "-w / --overwrite-low-quality"),
                          (pipe.stats, "--stats"),
                          (getattr(pipe, "correct_mismatches", None), "--correct-mismatches"),
                          (getattr(pipe, "merge_overlapping", False), "-R / --merge-overlapping")):
        if given:
            raise ValueError("%s needs quality values: the input is FASTA" % option)
    if pipe.report:
        raise NotImplementedError("report=True with FASTA input")
    if getattr(pipe, "demultiplex", False):
        raise NotImplementedError("demultiplexing ({name} in the output path) with FASTA input")


class TrimFormats(object):
    """The formats of one file run, settled before any output is opened: ``inputs`` (one per input path, all the
    same), ``outputs`` (one per main output path) and ``dests`` ({destination code: one per path} of the too-short /
    too-long / untrimmed files)."""

    def __init__(self, pipe, paths_in, paths_out, merged_out=None, byte_ranges=None, explicit=None):
        self.inputs = [input_format(p, explicit) for p in paths_in]
        if len(set(self.inputs)) > 1:
            raise ValueError("the two input files are of different formats (%s)" % " and ".join(self.inputs))
        self.fasta = fasta = self.inputs[0] == "fasta"
        paired = _is_paired(pipe)
        if self.inputs[0] == "bam":
            if len(paths_in) > 1:
                raise NotImplementedError("two BAM files as the reads of a pair are not provided: one name-sorted BAM "
                                          "file holds both (trim_files(path, None, ...), -l)")
            if byte_ranges is not None and any(r is not None for r in byte_ranges):
                raise NotImplementedError("a byte range of BAM input is not provided")
        demux = pipe_demultiplexes(pipe, paths_out, merged_out)
        if fasta:
            refuse_for_fasta(pipe)
            if demux:
                raise NotImplementedError("demultiplexing ({name} in the output path) with FASTA input")
            if paired and (len(paths_in) == 1 or len(paths_out) == 1):
                raise NotImplementedError("interleaved FASTA input / output (-l / -L) is not provided")
            if byte_ranges is not None and any(r is not None for r in byte_ranges):
                raise NotImplementedError("a byte range of FASTA input is not provided")
        self.outputs = [output_format(p, fasta) for p in paths_out]
        if merged_out is not None:
            self.outputs_merged = output_format(merged_out, fasta)
        codes = {name: code for code, name in DEST_NAMES.items()}
        self.dests = {codes[kind]: [output_format(p, fasta) for p in (paths if paired else (paths,))]
                      for kind, paths in pipe.outputs.items()}
        if "fasta" in self.outputs or (merged_out is not None and self.outputs_merged == "fasta"):
            # FASTQ reads into a FASTA-named file: the plain formatter does it, the grouped / pair / merge ones do not
            if demux or (paired and len(paths_out) == 1) or (merged_out is not None and self.outputs_merged == "fasta"):
                raise NotImplementedError("FASTA output of demultiplexed, interleaved or merged reads is not provided")


class _Mate(object):
    """The state of one read (of the pairs) during one ``run`` of ``pipe``: its chunk, the kept interval, the adapter
    flag and the unmasked interval, and what the later stages and the result need of the adapter stage."""

    def __init__(self, pipe, batch):
        n = len(batch)
        self.batch = batch
        self.begin = torch.zeros((n,), dtype=torch.int32, device=batch.records.device)
        self.end = batch.seq_lens.clone()
        self.matched = torch.zeros((n,), dtype=torch.uint8, device=self.begin.device)
        self.ubegin = self.uend = None
        self.rounds = [] if pipe.aux else None                # the adapter rounds kept for the info / rest / wildcard files
        self.sides = None                                     # per read: [any 5' match, any 3' match] (bisulfite)
        self.after = None                                     # the interval right after the adapter stage (bisulfite)
        self.last_which = (torch.zeros((n,), dtype=torch.int64, device=self.begin.device)
                           if ("{name}" in pipe.prefix or "{name}" in pipe.suffix or pipe.demultiplex) else None)
        self.unmasked = None                                  # a copy of the chunk before the mask / the zero cap
        # OverwriteRead: (the reads that are clones of their mates, the mate's adapters) -- a clone carries the mate's
        # match, so `last_which` of those reads indexes the OTHER read's adapter list ({name} in --prefix / --suffix)
        self.foreign = None


def _run_stages(pipes, mates, insert_stage=None, overwrite_stage=None):
    """The op-order stages, ``pipes[k]`` over ``mates[k]`` (one read, or the two reads of the pairs).  The A stage is
    ``insert_stage()`` if given (the paired insert aligner), else the adapter stage of every pipe that has adapters;
    the W stage is ``overwrite_stage()`` if given (OverwriteRead, pairs only); returns what the last
    ``insert_stage()`` returned."""
    op_order, action = pipes[0].op_order, pipes[0].action
    found = None
    for op in op_order:
        if op == "W":
            if overwrite_stage is not None:
                overwrite_stage()
            continue
        if op != "A":
            for pipe, m in zip(pipes, mates):
                pipe._simple_stage(op, m)
            continue
        if insert_stage is not None:
            found = insert_stage()
        else:
            for pipe, m in zip(pipes, mates):
                if pipe.adapters:
                    pipe._adapter_stage(m)
        for m in mates:
            if m.ubegin is not None and mask_before_later_stages(op_order, action):
                if m.rounds is not None:                      # (the info / rest / wildcard lines show the read a match saw)
                    m.unmasked = m.batch.data.clone()
                write_mask(m.batch, m.begin, m.end, m.ubegin, m.uend)
                m.ubegin = m.uend = None
    return found


def _batch_from_bytes(pipe, data, explicit=None):
    """The one batch of ``trim_bytes``: a FastaBatch if the text is FASTA (and the pipeline takes FASTA)."""
    if explicit not in (None, "fasta", "fastq"):
        raise ValueError("input_format must be 'fasta' or 'fastq'")
    if (explicit or sniff_format(bytes(data[:1 << 16]))) == "fasta":
        refuse_for_fasta(pipe)
        return FastaBatch.from_bytes(data, final=True)[0]
    return FastqBatch.from_bytes(data, final=True)[0]


def _trim_stream(pipe, paths_in, paths_out, chunk_bytes, keep_output, output_parts, merged_out=None, byte_ranges=None,
                 device_gzip=False, device_gunzip=False, input_format=None):
    """What ``TrimPipeline.trim_file`` (one input), ``PairedTrimPipeline.trim_files`` (two inputs in lock step, or one
    interleaved input) and ``shard.sharded_trim_file`` (``byte_ranges``: a rank's part of the input) do with every
    chunk of ``fastq.read_chunks``; returns the destination counts.  A paired pipeline with ONE input path reads it as
    an interleaved file, with ONE output path it writes the pairs interleaved (``atr_fastq_emit_pairs``)."""
    if _is_paired(pipe) and len(paths_out) == 1 and pipe.outputs:
        raise NotImplementedError("interleaved output with --too-short-output / --too-long-output / --untrimmed-output "
                                  "(the reference interleaves those files as well)")
    if device_gzip:
        # the main outputs compressed on the device (fastq.DeviceGzipSink); refused before anything is opened
        if output_parts and int(output_parts) > 1:
            raise NotImplementedError("device_gzip with part files (output_parts > 1)")
        if pipe_demultiplexes(pipe, paths_out, merged_out):
            raise NotImplementedError("device_gzip with demultiplexed outputs ({name} in the output path)")
        for p in list(paths_out) + ([merged_out] if merged_out is not None else []):
            if not str(p).endswith(".gz"):
                raise ValueError("device_gzip: the output path must end in .gz (%r)" % str(p))
    # FASTA or FASTQ, per input and per output (by explicit format, name, first byte): refusals come before any file
    formats = TrimFormats(pipe, paths_in, paths_out, merged_out, byte_ranges, input_format)
    if not pipe.report:
        return _trim_chunks(pipe, paths_in, paths_out, chunk_bytes, keep_output, output_parts, merged_out, byte_ranges, None,
                            device_gzip, device_gunzip, formats)
    # the report's counters: made before any output is opened (the table bound refuses here), on the device until the
    # file is done
    report = TrimReport(pipe, source=tuple(paths_in) if len(paths_in) == 2 else paths_in[0])
    try:
        return _trim_chunks(pipe, paths_in, paths_out, chunk_bytes, keep_output, output_parts, merged_out, byte_ranges, report,
                            device_gzip, device_gunzip, formats)
    finally:
        report.close()


def _is_paired(pipe):
    """The pipeline takes pairs (``run(batch1, batch2)``): the paired pipeline or the legacy one."""
    return isinstance(pipe, PairedTrimPipeline)


def pipe_demultiplexes(pipe, paths_out, merged_out=None):
    return bool(getattr(pipe, "demultiplex", False)) or any(
        p is not None and "{name}" in str(p) for p in list(paths_out) + [merged_out])


def _trim_chunks(pipe, paths_in, paths_out, chunk_bytes, keep_output, output_parts, merged_out, byte_ranges, report,
                 device_gzip=False, device_gunzip=False, formats=None):
    """The chunk loop of ``_trim_stream``; ``report``: the run's TrimReport or None; ``device_gzip``: the main
    outputs and the merged output through ``fastq.DeviceGzipSink`` (side files stay on the host path);
    ``device_gunzip``: BGZF ``.gz`` input inflated on the GPU (``fastq.ChunkedFastqReader``); ``formats``: the run's
    ``TrimFormats``."""
    formats = formats or TrimFormats(pipe, paths_in, paths_out, merged_out, byte_ranges)
    paired = _is_paired(pipe)
    interleaved_in = paired and len(paths_in) == 1
    interleaved_out = paired and len(paths_out) == 1
    first = pipe.p1 if paired else pipe
    merging = paired and pipe.merge_overlapping
    TrimStats.check(pipe.stats, first.discard_trimmed, first.discard_untrimmed, merging)
    be = _lib.get_backend()
    emitters = [be.fasta_emit if fmt == "fasta" else be.fastq_emit for fmt in formats.outputs]    # (one per main output)
    totals = {name: 0 for name in DEST_NAMES.values()}
    clock = StageClock()
    demux = not paired and pipe.demultiplex
    if demux:
        # one file per output name, opened when its first read arrives (the reference leaves no file for a name
        # without reads); the chunk's grouped text crosses to the host once and every segment goes to its file
        sinks, demux_files = [], {}
        demux_paths = pipe._demux_paths(paths_out[0])
        pipe.demux_counts = {}
    else:
        # (an interleaved output takes both reads' text of a chunk: twice the room, as the merged output below)
        room = chunk_bytes + (64 << 20)
        sinks = [make_sink(p, output_parts, (2 * room if interleaved_out else room) + 32, be, clock, keep=keep_output,
                           device_gzip=device_gzip) for p in paths_out]
    aux_files = {kind: open_by_extension(path) for kind, path in (pipe.aux or {}).items()}
    dest_codes = {name: code for code, name in DEST_NAMES.items()}
    dest_files = {dest_codes[kind]: [open_by_extension(p) for p in (paths if paired else (paths,))]
                  for kind, paths in pipe.outputs.items()                # (paired: a path per read)
                  if not (demux and kind == "untrimmed")}                # (demultiplexing: that path is the last group's)
    merged_sink = None
    if merging:
        totals["merged"] = 0
        if merged_out is not None:
            # a merged record is at most its two input records, and each input chunk may carry up to 64 MB over
            merged_sink = make_sink(merged_out, output_parts, 2 * (chunk_bytes + (64 << 20)) + 32, be, clock, keep=keep_output,
                                    device_gzip=device_gzip)
    stats = TrimStats(pipe.stats, paired, first.quality_base) if pipe.stats else None
    try:
        for batches in read_chunks(paths_in, chunk_bytes, be, clock, byte_ranges, device_gunzip, interleaved=interleaved_in,
                                   input_formats=formats.inputs):
            t0 = time.perf_counter()
            if stats is not None and stats.pre is not None:
                stats.pre.collect_batch(*batches)             # before any stage writes into the chunks
            res = pipe.run(*batches)
            reads = (res.read1, res.read2) if paired else (res,)
            if demux:
                texts = []
                grouped, edges = be.fastq_emit_grouped(res.batch.data, res.batch.records, res.begin, res.end, res.ubegin,
                                                       res.uend, res.group, len(res.group_names))
                per_group = torch.bincount(res.group[res.group >= 0].to(torch.int64), minlength=len(res.group_names)).cpu().tolist()
            elif interleaved_out:
                texts = [res.device_text_interleaved(_lib.DEST_KEEP)]
            else:
                texts = [emit(r.batch.data, r.batch.records, r.begin, r.end, r.ubegin, r.uend, r.dest, _lib.DEST_KEEP)
                         for emit, r in zip(emitters, reads)]
            counts = res.counts()
            if report is not None:
                report.add(res)
            if stats is not None:                             # (collect_batch's order: batches, intervals, masks)
                post =([r.batch for r in reads] + [t for r in reads for t in (r.begin, r.end)] +
                        [t for r in reads for t in (r.ubegin, r.uend)] + [res.dest])
                stats.add_post(counts, lambda st, code: st.collect_batch(*post, code))
            clock.add("trim_and_format", t0)
            for sink, text in zip(sinks, texts):
                sink.write(text)
            if demux and edges[-1]:
                host = grouped.cpu().numpy()
                for g, name in enumerate(res.group_names):
                    if edges[g + 1] > edges[g]:
                        if g not in demux_files:
                            demux_files[g] = open_by_extension(demux_paths[g])
                        demux_files[g].write(memoryview(host[edges[g]:edges[g + 1]]))
                        pipe.demux_counts[name] = pipe.demux_counts.get(name, 0) + per_group[g]
            if merged_sink is not None:
                merged_sink.write(res.merged if res.merged is not None else texts[0][:0])
            if aux_files:                                     # host-assembled lines (debugging outputs, not a throughput path)
                for kind, blob in res.aux_text(tuple(aux_files)).items():
                    aux_files[kind].write(blob)
            for code, fhs in dest_files.items():              # the filtered reads that have a file of their own
                for fh, r, fmt in zip(fhs, reads, formats.dests[code]):
                    fh.write(r.text(code, fmt))
            for name, v in counts.items():
                totals[name] += v
        if stats is not None:
            pipe.stats_summary = stats.summary()
        if report is not None:
            pipe.report_summary = report.summary()
    finally:
        for obj in sinks + ([merged_sink] if merged_sink is not None else []) + list(aux_files.values()) + [
                fh for fhs in dest_files.values() for fh in fhs]:
            obj.close()
        if demux:
            for fh in demux_files.values():
                fh.close()
        pipe.stage_seconds = dict(clock.seconds)
    return totals


class TrimPipeline(object):
    """The single-end trimming steps of ``atropos trim`` as whole-batch device stages.

    Args mirror the command line (trim/cli.py): ``adapters`` -- list of
    ``atropos_amd.adapters.Adapter`` / ``LinkedAdapter`` (from ``AdapterParser``);
    ``times`` (-n), ``action`` ('trim' | 'mask' | None); ``cut`` (-u, list of ints);
    ``nextseq_trim``; ``quality_cutoff`` ((front, back), -q); ``quality_base``; ``trim_n``;
    ``minimum_length`` (-m), ``maximum_length`` (-M), ``max_n``; ``discard_trimmed``,
    ``discard_untrimmed``; ``op_order``.
    """

    def __init__(self, adapters=(), times=1, action="trim", cut=(), nextseq_trim=None, quality_cutoff=None,
                 quality_base=33, trim_n=False, minimum_length=None, maximum_length=None, max_n=None,
                 discard_trimmed=False, discard_untrimmed=False, op_order="CGQAW", aux=None, length_tag=None,
                 strip_suffix=(), prefix="", suffix="", zero_cap=False, outputs=None, cut_min=(), bisulfite=None,
                 stats=None, report=False, demultiplex=False):
        self.adapters = list(adapters)
        # demultiplex=True: every result carries the output code of its reads (TrimResult.group / demux_text);
        # trim_file switches it on for a call whose output path holds "{name}" (one file per adapter name)
        self.demultiplex = bool(demultiplex)
        # report=True: trim_file leaves the reference's summary['trim'] and input totals in self.report_summary; a
        # caller of run() collects them with atropos_amd.report.TrimReport, which hangs its counters in here
        self.report, self._reporter = bool(report), None
        # stats=("pre",) / ("post",) / ("pre", "post"): trim_file leaves the reference's --stats summary in
        # self.stats_summary (TrimStats)
        self.stats = _stats_modes(stats)
        # --bisulfite: a list of cutters applied after the op-order stages and before --trim-n (trim/__init__.py:497-516):
        # ("min", front, back, count_trimmed, only_trimmed) = MinCutter, ("nondir", rrbs) = NonDirectionalBisulfiteTrimmer
        self.bisulfite = list(bisulfite or ())
        # --cut-min: MinCutter with its defaults (modifiers.py:587-650; after --trim-n, trim/__init__.py:520-524)
        cut_min = list(cut_min or ())
        self.min_front = sum(c for c in cut_min if c > 0)
        self.min_back = -sum(c for c in cut_min if c < 0)
        if (self.min_front or self.min_back) and action != "trim":
            raise NotImplementedError("--cut-min with --mask-adapter / --no-trim (a match counts as trimmed bases that "
                                      "are still there)")
        # --too-short-output / --too-long-output / --untrimmed-output: {"too_short" | "too_long" | "untrimmed": path};
        # the untrimmed file switches the UntrimmedFilter on like --discard-untrimmed (trim/__init__.py:617-630)
        self.outputs = dict(outputs) if outputs else {}
        if "untrimmed" in self.outputs:
            discard_untrimmed = True
        # read-name modifiers and the quality cap, applied after every trimming step (trim/__init__.py:526-541)
        self.length_tag, self.strip_suffix = length_tag or None, list(strip_suffix or ())
        self.prefix, self.suffix, self.zero_cap = prefix or "", suffix or "", bool(zero_cap)
        self._name_mods = bool(self.length_tag or self.strip_suffix or self.prefix or self.suffix)
        self.aux = dict(aux) if aux else None            # {"info" | "rest" | "wildcard": path}: --info-file, --rest-file, --wildcard-file
        self.times, self.action = int(times), action
        if action not in ("trim", "mask", None):
            raise ValueError("action must be 'trim', 'mask' or None")
        cut = list(cut or ())
        self.cut_front = sum(c for c in cut if c > 0)                    # modifiers.py:577-582
        self.cut_back = sum(c for c in cut if c < 0)
        self.nextseq_trim = nextseq_trim
        if quality_cutoff is not None and not isinstance(quality_cutoff, (tuple, list)):
            quality_cutoff = (0, quality_cutoff)                          # "-q 10" = 3' cutoff only (trim/cli.py)
        self.quality_cutoff = quality_cutoff
        self.quality_base = quality_base
        self.trim_n = trim_n
        self.minimum_length = minimum_length
        self.maximum_length = maximum_length
        self.max_n = max_n
        self.discard_trimmed, self.discard_untrimmed = discard_trimmed, discard_untrimmed
        self.op_order = op_order
        linked = [a for a in self.adapters if isinstance(a, LinkedAdapter)]
        if linked and len(linked) != len(self.adapters):
            raise NotImplementedError("mixing linked and plain adapters (the reference's AdapterCutter raises "
                                      "AttributeError as soon as two of them match a read)")
        self._linked = bool(linked)
        if self.aux and self._linked:
            raise NotImplementedError("--info-file / --rest-file / --wildcard-file with linked adapters")
        if self.bisulfite:
            if self._linked:
                raise NotImplementedError("--bisulfite with linked adapters")
            for spec in self.bisulfite:
                if action != "trim" and (spec[0] == "nondir" or spec[3]):
                    raise NotImplementedError("--bisulfite cutters that count the adapters' bases or look at the read's "
                                              "first bases, with --mask-adapter / --no-trim")
        if self._linked and (self.min_front or self.min_back):
            raise NotImplementedError("--cut-min with linked adapters (what a LinkedMatch counts as trimmed is not the interval)")
        if self._linked and ("{name}" in self.prefix or "{name}" in self.suffix):
            raise NotImplementedError("{name} in --prefix / --suffix with linked adapters")
        if self.report:
            check_envelope(linked=self._linked, bisulfite=bool(self.bisulfite))
        if self.demultiplex:
            self._check_demux()

    # ------------------------------------------------------------------ demultiplexing
    def _check_demux(self):
        """What a demultiplexed run refuses (trim/cli.py:765-768 and the limits of this pipeline)."""
        if self.discard_trimmed:
            raise ValueError("Do not use --discard-trimmed when demultiplexing.")
        if self._linked:
            raise NotImplementedError("demultiplexing ({name} in the output path) with linked adapters")
        if self.report:
            raise NotImplementedError("the trim report of a demultiplexed run ({name} in the output path)")
        names, _, _ = self._demux_groups()
        if len(names) > _lib.EMIT_MAX_GROUPS:
            raise _lib.AtroposUnsupported("demultiplexing: %d outputs (at most %d, the group bound of atr_fastq_emit_grouped)"
                                          % (len(names), _lib.EMIT_MAX_GROUPS))

    def _demux_groups(self):
        """(the outputs' names, the output of every adapter, the untrimmed output or -1): adapters that share a name
        share an output; unless --discard-untrimmed is given the untrimmed output is --untrimmed-output or the file of
        the name "unknown" (trim/__init__.py:620-624)."""
        names, adapter_group = [], []
        for ad in self.adapters:
            if ad.name not in names:
                names.append(ad.name)
            adapter_group.append(names.index(ad.name))
        untrimmed = -1
        if "untrimmed" in self.outputs or not self.discard_untrimmed:
            if "untrimmed" not in self.outputs and "unknown" in names:
                untrimmed = names.index("unknown")
            else:
                untrimmed = len(names)
                names.append("unknown")
        return names, adapter_group, untrimmed

    def _demux_paths(self, path_out):
        """The file of every output of ``_demux_groups``."""
        names, _, untrimmed = self._demux_groups()
        paths = [path_out.format(name=name) for name in names]
        if "untrimmed" in self.outputs:
            paths[untrimmed] = self.outputs["untrimmed"]
        return paths

    # ------------------------------------------------------------------ adapter rounds
    @staticmethod
    def _front_code(adapter):
        flag = adapter._front_flag
        return 2 if flag is None else (1 if flag else 0)

    def _round_plain(self, m, active):
        """One ``_best_match`` + ``trimmed`` round (modifiers.py:107-122, :133-139)."""
        batch, begin, end = m.batch, m.begin, m.end
        be = batch.backend
        source = RecordSource(batch, begin, end)
        best = which = None
        for idx, adapter in enumerate(self.adapters):
            rec = adapter.match_source(source)
            if best is None:
                best = rec
                which = torch.zeros((len(batch),), dtype=torch.int64, device=rec.device)
                continue
            better = (rec[:, 1] >= 0) & ((best[:, 1] < 0) | (rec[:, 4] > best[:, 4]))     # strict >: first wins
            best = torch.where(better[:, None], rec, best)
            which = torch.where(better, torch.full_like(which, idx), which)
        codes = torch.tensor([self._front_code(a) for a in self.adapters], dtype=torch.uint8, device=best.device)
        front = codes[which].contiguous() if len(self.adapters) > 1 else None
        took = (active != 0) & (best[:, 1] >= 0)                          # reads this round's match applies to
        if m.rounds is not None:                                          # (... and the read the match saw)
            m.rounds.append((took, best.clone(), which.clone(), begin.clone(), end.clone()))
        if m.last_which is not None:
            m.last_which = torch.where(took, which, m.last_which)
            if m.foreign is not None:                                     # (a match of its own replaces the copied one)
                m.foreign = (m.foreign[0] & ~took, m.foreign[1])
        if m.sides is not None:                                           # Match.front / _guess_is_front of this round's match
            code = codes[which]
            is_front = torch.where(code == 2, best[:, 2] == 0, code == 1)
            m.sides[0] |= took & is_front
            m.sides[1] |= took & ~is_front
        best = best.contiguous()
        if self._reporter is not None:                                    # Adapter.trimmed counts, once per match and round
            self._reporter.adapter_round(batch, took, best, which, front, self._front_code(self.adapters[0]), begin, end,
                                         source.max_len())
        be.match_trim_batch(best, front, int(codes[0].item()), begin, end, active, m.matched)

    def _round_linked(self, m, active):
        """LinkedAdapter.match_to + trimmed (adapters/__init__.py:648-706) for linked adapters
        whose 5' parts are mutually exclusive: the first one whose 5' part matches is used."""
        from .adapters import linked_records_from_source
        batch, begin, end = m.batch, m.begin, m.end
        be = batch.backend
        which, _count, front, back = linked_records_from_source(self.adapters, batch, begin, end, active)
        claimed = (which >= 0).to(torch.uint8)
        be.match_trim_batch(front.contiguous(), None, 1, begin, end, claimed.clone(), None)    # read[front.rstop:]
        be.match_trim_batch(back.contiguous(), None, 0, begin, end, claimed.clone(), None)     # then read[:back.rstart]
        m.matched |= claimed
        active &= claimed                                                 # no 5' match: the loop over `times` stops

    def _adapter_stage(self, m):
        """Sets the mate's adapter flag and, with the 'mask' action, its unmasked interval."""
        begin, end = m.begin, m.end
        n = len(m.batch)
        dev = begin.device
        m.matched = torch.zeros((n,), dtype=torch.uint8, device=dev)
        m.ubegin = m.uend = None
        if not self.adapters or n == 0:
            return
        before_b, before_e = begin.clone(), end.clone()
        if self.bisulfite:
            m.sides = [torch.zeros((n,), dtype=torch.bool, device=dev), torch.zeros((n,), dtype=torch.bool, device=dev)]
        active = (end > begin).to(torch.uint8)                            # if len(read) == 0: return read
        for _ in range(self.times):
            if self._linked:
                self._round_linked(m, active)
            else:
                self._round_plain(m, active)
        if self.action == "mask":                                         # modifiers.py:155-172
            m.ubegin, m.uend = begin.clone(), end.clone()
            begin.copy_(before_b)
            end.copy_(before_e)
        elif self.action is None:                                         # :173-174
            begin.copy_(before_b)
            end.copy_(before_e)
        if self.bisulfite:
            m.after = (begin.clone(), end.clone())

    def _bisulfite_stage(self, m):
        """MinCutter / RRBSTrimmer / NonDirectionalBisulfiteTrimmer (modifiers.py:587-650, :786-831) as interval
        arithmetic.  What a cutter counts as already trimmed: with count_trimmed everything that is gone from that end
        (Sequence.clipped + the matches' rsize_total = the interval); without, what the trimmers removed AFTER the
        adapter stage for a read with a match (clipped[2], clipped[3]) and everything for a read without one."""
        batch, begin, end = m.batch, m.begin, m.end
        has = m.matched != 0
        total = batch.seq_lens
        ab, ae = m.after if m.after is not None else (begin, end)
        sides = m.sides if m.sides is not None else [torch.zeros_like(has), torch.zeros_like(has)]
        for spec in self.bisulfite:
            if spec[0] == "nondir":
                # ^C[AG]A on the read as it is now -> two bases off the 5' end (counting only what was cut after a
                # match); else, with rrbs, the RRBS cutter
                off = (batch.records[:, 2].to(torch.int64) & 0xFFFFFFFF) + begin.to(torch.int64)
                last = batch.data.numel() - 1
                c0, c1, c2 = (batch.data[(off + k).clamp(max=last)] for k in range(3))
                hit = (end - begin >= 3) & (c0 == 67) & ((c1 == 65) | (c1 == 71)) & (c2 == 65)
                self._min_cut(begin, end, total, has, sides, ab, ae, 2, 0, False, False, hit)
                if spec[1]:
                    # (NonDirectionalBisulfiteTrimmer builds its RRBSTrimmer as RRBSTrimmer(trim_3p): the 2 lands in
                    # trim_5p and trim_3p keeps its default -- two bases from EITHER trimmed end, modifiers.py:808-813)
                    self._min_cut(begin, end, total, has, sides, ab, ae, 2, 2, False, True, ~hit & (end > begin))
            else:
                _kind, front, back, count_trimmed, only_trimmed = spec
                self._min_cut(begin, end, total, has, sides, ab, ae, front, back, count_trimmed, only_trimmed, None)

    @staticmethod
    def _min_cut(begin, end, total, has, sides, ab, ae, front, back, count_trimmed, only_trimmed, where):
        live = end > begin                                                # Trimmer.clip leaves an empty read alone
        if where is not None:
            live = live & where
        trim_front = trim_back = live
        if only_trimmed:                                                  # :612-621
            trim_front = live & has & sides[0]
            trim_back = live & has & sides[1]
        if count_trimmed:
            gone_f, gone_b = begin, total - end
        else:
            gone_f = torch.where(has, begin - ab, begin)
            gone_b = torch.where(has, ae - end, total - end)
        tf = torch.where(trim_front, (front - gone_f).clamp(min=0), torch.zeros_like(begin))
        tb = torch.where(trim_back, (back - gone_b).clamp(min=0), torch.zeros_like(begin))
        nb = torch.minimum(begin + tf, end)
        ne = torch.maximum(end - tb, nb)
        begin.copy_(nb)
        end.copy_(ne)

    # ------------------------------------------------------------------ whole pipeline
    def _simple_stage(self, op, m):
        """The C, G, Q stages (interval updates without alignment)."""
        batch, begin, end = m.batch, m.begin, m.end
        be = batch.backend
        rep = self._reporter                                              # Trimmer.trimmed_bases of the stage
        if op == "C" and (self.cut_front or self.cut_back):
            before = (begin.clone(), end.clone()) if rep else None
            be.clip_batch(batch.records, begin, end, self.cut_front, self.cut_back)
            if rep:
                rep.intervals(batch, before, begin, end, _lib.REPORT_CLIP, self.cut_front, -self.cut_back, SLOT_CUT)
        elif op == "G" and self.nextseq_trim is not None:
            before = (begin.clone(), end.clone()) if rep else None
            be.quality_trim_batch(batch.data, batch.records, begin, end, 0, int(self.nextseq_trim),
                                  self.quality_base, True)
            if rep:
                rep.intervals(batch, before, begin, end, _lib.REPORT_SUBSEQ, 0, 0, SLOT_NEXTSEQ)
        elif op == "Q" and self.quality_cutoff:
            before = (begin.clone(), end.clone()) if rep else None
            be.quality_trim_batch(batch.data, batch.records, begin, end, int(self.quality_cutoff[0]),
                                  int(self.quality_cutoff[1]), self.quality_base, False)
            if rep:
                rep.intervals(batch, before, begin, end, _lib.REPORT_SUBSEQ, 0, 0, SLOT_QUALITY)

    def _filter_stage(self, m, masks=False):
        """The bisulfite cutters, --trim-n, --cut-min, then the read filters: destination byte per read (or the fail
        masks)."""
        batch, begin, end, ubegin, uend = m.batch, m.begin, m.end, m.ubegin, m.uend
        be = batch.backend
        if self.bisulfite:
            self._bisulfite_stage(m)
        rep = self._reporter
        if self.trim_n:
            before = (begin.clone(), end.clone()) if rep else None
            be.nend_trim_batch(batch.data, batch.records, begin, end, ubegin, uend)
            if rep:
                rep.intervals(batch, before, begin, end, _lib.REPORT_NEND, 0, 0, SLOT_NEND)
        if (self.min_front or self.min_back) and rep:                     # (MinCutter counts what it asks clip() for)
            rep.intervals(batch, (begin, end), begin, end, _lib.REPORT_MINCUT, self.min_front, self.min_back, SLOT_MINCUT)
        if self.min_front or self.min_back:
            # at least min_front / min_back bases gone from the two ends, whatever removed them so far: everything that
            # was cut, quality-trimmed or adapter-trimmed is in the interval (clipped[] + the matches' rsize_total)
            live = end > begin                                            # Trimmer.clip leaves an empty read alone
            total = batch.seq_lens
            nb = torch.minimum(torch.maximum(begin, torch.full_like(begin, self.min_front)), end)
            ne = torch.maximum(torch.minimum(end, total - self.min_back), nb)
            begin.copy_(torch.where(live, nb, begin))
            end.copy_(torch.where(live, ne, end))
        min_len = self.minimum_length if self.minimum_length is not None and self.minimum_length > 0 else 0
        max_len = self.maximum_length if self.maximum_length is not None else -1
        max_n = float(self.max_n) if self.max_n is not None else -1.0
        return be.read_filter_batch(batch.data, batch.records, begin, end, ubegin, uend, m.matched, min_len, max_len,
                                    max_n, self.discard_trimmed, self.discard_untrimmed, masks=masks)

    def run(self, batch):
        """All stages over one FastqBatch; returns a TrimResult."""
        m = _Mate(self, batch)
        _run_stages([self], [m])
        return self._result(m, self._filter_stage(m))

    def _result(self, m, dest):
        """The tail of a run: the zero cap and the read-name modifiers, then the TrimResult of the mate."""
        b, n = m.batch, len(m.batch)
        fmt = getattr(b, "fmt", "fastq")
        if self.zero_cap and n and fmt != "fasta":              # (no qualities: the reference does not install ZeroCapper)
            if m.rounds is not None and m.unmasked is None:        # a match's info record shows the read as the match saw it:
                m.unmasked = b.data.clone()                        # before ZeroCapper (align/__init__.py:145-170)
            self._zero_cap(m)
        read_batch = b if m.unmasked is None else FastqBatch(m.unmasked, b.nbytes, b.records, b.backend, b.line_ends)
        batch = self._rewrite_names(m) if self._name_mods and n else b
        res = TrimResult(batch, m.begin, m.end, m.ubegin, m.uend, m.matched, dest, m.rounds, self.adapters, read_batch)
        res.fmt = fmt
        if self.demultiplex:
            names, adapter_group, untrimmed = self._demux_groups()
            table = torch.tensor(adapter_group or [0], dtype=torch.int32, device=dest.device)
            res.group = b.backend.demux_groups(dest, m.matched, m.last_which, table, len(adapter_group), untrimmed)
            res.group_names = names
        return res

    def _zero_cap(self, m):
        """ZeroCapper (modifiers.py:709-720): quality characters below the base become the base, in the chunk."""
        batch = m.batch
        rec = batch.records
        lens = rec[:, 5].to(torch.int64)
        start = rec[:, 4].to(torch.int64) & 0xFFFFFFFF
        first = torch.cumsum(lens, 0) - lens
        idx = torch.repeat_interleave(start - first, lens) + torch.arange(int(lens.sum().item()), device=rec.device)
        batch.data[idx] = batch.data[idx].clamp(min=self.quality_base)

    def _rewrite_names(self, m):
        """LengthTagModifier, SuffixRemover, PrefixSuffixAdder (modifiers.py:652-695) in the reference's order: the
        new names are made on the host (string work per read, as in the reference), appended to the chunk in device
        memory, and the records point at them -- the formatter copies whatever name a record names."""
        import re
        import numpy as np
        batch = m.batch
        raw = bytes(batch.data[:batch.nbytes].cpu().numpy().tobytes())
        recs = batch.records.cpu().numpy().astype("int64")
        lens = (m.end - m.begin).clamp(min=0).cpu().tolist()
        took = m.matched.cpu().tolist()
        which = m.last_which.cpu().tolist() if m.last_which is not None else None
        foreign = m.foreign[0].cpu().tolist() if m.foreign is not None else None
        tag = self.length_tag
        regex = re.compile(r"\b" + tag + r"[0-9]*\b") if tag else None
        names, offs, cur = [], [], 0
        for i in range(recs.shape[0]):
            off = recs[i, 0] & 0xFFFFFFFF
            name = raw[off:off + recs[i, 1]].decode("latin-1")
            if tag and name.find(tag) >= 0:
                name = regex.sub(tag + str(lens[i]), name)
            for sfx in self.strip_suffix:
                if name.endswith(sfx):
                    name = name[:-len(sfx)]
            if self.prefix or self.suffix:
                ads = m.foreign[1] if (foreign is not None and foreign[i]) else self.adapters
                ad = ads[which[i]].name if (which is not None and took[i]) else "no_adapter"
                name = self.prefix.replace("{name}", ad) + name + self.suffix.replace("{name}", ad)
            blob = name.encode("latin-1")
            names.append(blob)
            offs.append(cur)
            cur += len(blob)
        base = (batch.data.numel() + 15) // 16 * 16
        if base + cur >= (1 << 32) - 16:
            raise ValueError("the chunk and its rewritten names must stay below 4 GiB")
        extra = torch.from_numpy(np.frombuffer(b"".join(names) + b"\0" * 16, dtype=np.uint8).copy()).to(batch.data.device)
        data = torch.cat([batch.data, torch.zeros((base - batch.data.numel(),), dtype=torch.uint8, device=extra.device), extra])
        noff = np.asarray(offs, dtype=np.int64) + base
        # the '+' line keeps the text the file had (FastqFormat prints name2, io/seqio.py:690-699): flag bit 1,
        # the old name's offset in `reserved`, its length above the flag bits (atr_fastq_record)
        rep = (recs[:, 6] & 1) != 0
        recs[:, 7] = np.where(rep, recs[:, 0], recs[:, 7])
        flags = np.where(rep, (recs[:, 6] & 1) | 2 | (recs[:, 1] << 8), recs[:, 6])
        recs[:, 6] = np.where(flags >= (1 << 31), flags - (1 << 32), flags)
        recs[:, 0] = np.where(noff >= (1 << 31), noff - (1 << 32), noff)
        recs[:, 1] = [len(b) for b in names]
        records = torch.from_numpy(recs.astype(np.int32)).to(batch.records.device)
        return FastqBatch(data, batch.nbytes, records, batch.backend, batch.line_ends)

    def trim_bytes(self, data, which=_lib.DEST_KEEP, input_format=None, fmt=None):
        """FASTQ (FASTA) text in, trimmed text out (one batch).  ``input_format``: "fastq" | "fasta", by default what
        the first byte says (``fastq.sniff_format``); ``fmt``: the output's, by default the input's."""
        return self.run(_batch_from_bytes(self, data, input_format)).text(which, fmt)

    def trim_file(self, path_in, path_out, chunk_bytes=256 << 20, keep_output=False, output_parts=1, device_gzip=False,
                  device_gunzip=False, input_format=None):
        """Stream a FASTQ file through the GPU in chunks of whole records; returns the
        destination counts.  (Plain files; compressed input is the caller's business.)
        Host side: ``fastq.read_chunks`` (the one chunk loop, over ``ChunkedFastqReader``) / ``FastqSink`` (page-locked staging buffers, threaded
        reads, read-ahead; device -> host copies on their own stream and write-behind, so the GPU
        works on chunk i + 1 while chunk i travels back and into the file).  ``keep_output``: overwrite
        an existing output file in place instead of truncating it first.  ``output_parts`` > 1: the output
        as that many part files ``<path_out>.part<i>`` with a writer each (``fastq.PartSink``: chunk k goes to
        part k mod N; what the reference's ``--no-writer-process`` does with its worker processes) -- for hosts
        that serialise the writers of one file.  The seconds the loop spent waiting per stage are left in
        ``self.stage_seconds``.

        ``{name}`` in ``path_out`` demultiplexes, as the reference's ``-o`` does (commands/trim/writers.py:119-154):
        every read that is kept goes to the file named after the adapter of its last match, a read without a match
        to the file of the name ``unknown`` or to --untrimmed-output (nowhere with --discard-untrimmed); a name
        without reads leaves no file.  The records per name are left in ``self.demux_counts``.  Single-end only, as
        in the reference; linked adapters, ``report=True`` and part files are refused with it.

        ``device_gzip``: ``path_out`` ends in ``.gz`` and is compressed on the GPU (``fastq.DeviceGzipSink``: BGZF
        members, any gzip reader takes them) instead of by one host thread; the decompressed bytes are the same.
        Side files stay on the host path; with ``{name}`` or ``output_parts`` > 1 it is a NotImplementedError.

        ``device_gunzip``: a ``path_in`` that ends in ``.gz`` and holds BGZF members (``bgzip``, htslib,
        ``device_gzip=True``) is inflated on the GPU, a wave per member, instead of by one host thread; any other
        input is read as without the flag (``fastq.ChunkedFastqReader``).  ``device_gunzip="any"``: every other
        ``.gz`` member -- an ordinary gzip file -- is inflated on the GPU as well (a speculative two-pass gunzip).
        The flag only changes where the text comes from, and combines with every other option.

        FASTA: the input is read as FASTA when ``input_format`` = "fasta", else when its name ends in .fasta / .fa /
        .fna (a compression suffix aside), else when its first byte is '>' (``fastq.input_format``).  The output is
        FASTA when its name says so, FASTQ when its name says so, and what the input is otherwise (``output_format``);
        the same goes for the too-short / too-long / untrimmed files.  FASTA input into a FASTQ-named file, and the
        options that need qualities (``refuse_for_fasta``), are refused before any file is opened.

        Unaligned BAM: a name that ends in .bam (or ``input_format`` = "bam") is inflated, walked and decoded to FASTQ
        text on the GPU (``fastq.ChunkedFastqReader``), whatever ``device_gunzip`` says; everything else works as on
        FASTQ.  BAM / SAM output and SAM text input are a NotImplementedError before any file is opened."""
        if device_gzip and ("{name}" in path_out or self.demultiplex):
            raise NotImplementedError("device_gzip with demultiplexed outputs ({name} in the output path)")
        if "{name}" not in path_out and not self.demultiplex:
            return _trim_stream(self, [path_in], [path_out], chunk_bytes, keep_output, output_parts, device_gzip=device_gzip,
                                device_gunzip=device_gunzip, input_format=input_format)
        if "{name}" not in path_out:
            raise ValueError("a demultiplexing pipeline needs {name} in the output path")
        if output_parts and int(output_parts) > 1:
            raise ValueError("part files of a demultiplexed output ({name} in the output path) are not provided")
        was = self.demultiplex
        self.demultiplex = True
        try:
            self._check_demux()                               # before any output is opened
            return _trim_stream(self, [path_in], [path_out], chunk_bytes, keep_output, output_parts, device_gunzip=device_gunzip,
                                input_format=input_format)
        finally:
            self.demultiplex = was


class PairedTrimResult(object):
    """Result of the paired-end pipeline: one TrimResult per read, sharing the destination."""

    def __init__(self, res1, res2, merged=None):
        self.read1, self.read2, self.dest = res1, res2, res1.dest
        self.merged = merged                     # uint8 device tensor: the FASTQ text of the merged reads, or None

    def counts(self):
        c = torch.bincount(self.dest.to(torch.int64), minlength=7).cpu().tolist()
        out = {DEST_NAMES[i]: int(c[i]) for i in range(6)}
        if self.merged is not None:
            out["merged"] = int(c[DEST_MERGED])
        return out

    def aux_text(self, kinds=("info", "rest", "wildcard")):
        """The info / rest / wildcard lines of the pairs: read 1's, then read 2's, pair after pair
        (Formatters.format calls every info formatter on read 1 and on read 2, writers.py:156-159)."""
        l1, l2 = self.read1.aux_lines(kinds), self.read2.aux_lines(kinds)
        # (`if read2:` in Formatters.format: a read 2 that was trimmed to nothing is false and gets no lines)
        has2 = (self.read2.end > self.read2.begin).cpu().tolist()
        return {k: "".join(line + "\n" for a, b, two in zip(l1[k], l2[k], has2) for line in (a + b if two else a)).encode("ascii", "replace")
                for k in kinds}

    def merged_text(self):
        """FASTQ text of the merged reads (the --merged-output file), in input order."""
        return b"" if self.merged is None else bytes(self.merged.cpu().numpy().tobytes())

    def text(self, which=_lib.DEST_KEEP, fmt=None):
        return self.read1.text(which, fmt), self.read2.text(which, fmt)

    def device_text_interleaved(self, which=_lib.DEST_KEEP):
        """``text_interleaved`` as a uint8 device tensor (one ``atr_fastq_emit_pairs``)."""
        r1, r2 = self.read1, self.read2
        return r1.batch.backend.fastq_emit_pairs(r1.batch, r1.begin, r1.end, r1.ubegin, r1.uend,
                                                 r2.batch, r2.begin, r2.end, r2.ubegin, r2.uend, self.dest, which)

    def text_interleaved(self, which=_lib.DEST_KEEP):
        """Formatted FASTQ text (bytes) of the pairs sent to destination ``which``, read 1 then read 2 of every pair:
        what the reference's ``-L`` file holds (InterleavedFormatter, io/seqio.py:740-749)."""
        return bytes(self.device_text_interleaved(which).cpu().numpy().tobytes())


class PairedTrimPipeline(object):
    """Paired-end trimming in "both" mode (both reads are modified; trim/cli.py:633-648) as
    whole-batch device stages.  ``aligner``: 'adapter' -- one AdapterCutter per read
    (``adapters1`` / ``adapters2``), or 'insert' -- InsertAdapterCutter with exactly one 3'
    adapter per read (trim/__init__.py:406-456).  ``pair_filter``: 'any' or 'both'.
    ``correct_mismatches`` ('liberal' | 'conservative' | 'N', insert aligner only): error
    correction of the overlaps, written IN PLACE into the two FASTQ chunks in device memory
    (a batch is consumed by ``run``).  ``merge_overlapping``: MergeOverlapping as the last modifier
    (commands/trim/modifiers.py:864-931, trim/__init__.py:546-552): pairs whose reads overlap by
    ``merge_min_overlap`` (a fraction of the shorter read up to 1, else bases) at ``merge_error_rate``
    become ONE read -- destination ``DEST_MERGED``, text in ``PairedTrimResult.merged`` -- corrected
    first with ``correct_mismatches`` unless the insert aligner already saw the pair.
    ``overwrite_low_quality`` = (lowq, highq, window): OverwriteRead (``-w``, modifiers.py:511-563) at ``W``'s place in
    ``op_order``: a read whose first ``window`` kept qualities average below ``lowq`` while its mate's average at
    least ``highq`` is replaced by the mate's reverse complement (``_overwrite_stage``); ``self.overwritten`` counts
    them per read.  ``lowq > highq`` and ``window < 1`` are a ValueError.  Refused with it (NotImplementedError; the
    reference runs them): ``aux`` files (the clone's match_info lines), ``report=True``, ``stats`` post,
    ``cut_min`` / ``cut_min2`` and ``bisulfite`` (both read ``clipped[]``, which the clone copies unmirrored),
    ``merge_overlapping`` (the ``corrected`` flag), linked adapters."""

    def __init__(self, adapters1=(), adapters2=(), aligner="adapter", times=1, action="trim", cut=(), cut2=(),
                 nextseq_trim=None, quality_cutoff=None, quality_base=33, trim_n=False, minimum_length=None,
                 maximum_length=None, max_n=None, discard_trimmed=False, discard_untrimmed=False, pair_filter="any",
                 op_order="CGQAW", insert_args=None, correct_mismatches=None, merge_overlapping=False,
                 merge_min_overlap=0.9, merge_error_rate=0.2, aux=None, length_tag=None, strip_suffix=(), prefix="",
                 suffix="", zero_cap=False, outputs=None, cut_min=(), cut_min2=(), bisulfite=None, bisulfite2=None,
                 stats=None, report=False, overwrite_low_quality=None):
        self.stats = _stats_modes(stats)                                  # as TrimPipeline's: trim_files' summary
        # -w LOWQ,HIGHQ,WINDOW (OverwriteRead, modifiers.py:511-563): the stage at W's place in op_order; the reads it
        # overwrote, per read of the pair, add up in self.overwritten
        self.overwrite_low_quality, self.overwritten = None, [0, 0]
        if overwrite_low_quality is not None:
            lowq, highq, window = (int(v) for v in overwrite_low_quality)
            if lowq > highq:
                raise ValueError("For --overwrite-low-quality, LOWQ must be <= HIGHQ")           # cli.py:745-748
            if window < 1:
                raise ValueError("--overwrite-low-quality: WINDOW must be at least 1")
            self.overwrite_low_quality = (lowq, highq, window)
            for given, what in ((aux, "--info-file / --rest-file / --wildcard-file (the clone's match_info lines)"),
                                (report, "report=True"), ("post" in self.stats, "--stats post / both"),
                                (cut_min or cut_min2, "--cut-min / --cut-min2 (the clone copies clipped[] unmirrored)"),
                                (bisulfite or bisulfite2, "--bisulfite (the clone copies clipped[] unmirrored)"),
                                (merge_overlapping, "--merge-overlapping (the clone's corrected flag)"),
                                (any(isinstance(a, LinkedAdapter) for a in list(adapters1) + list(adapters2)), "linked adapters")):
                if given:
                    raise NotImplementedError("--overwrite-low-quality with " + what)
        self.report = bool(report)                                        # as TrimPipeline's: trim_files' report_summary
        if self.report:
            check_envelope(aligner=aligner, merge_overlapping=bool(merge_overlapping), bisulfite=bool(bisulfite or bisulfite2))
        # {"too_short" | "too_long" | "untrimmed": (path for read 1, path for read 2)}: the filtered pairs' own files
        self.outputs = dict(outputs) if outputs else {}
        if "untrimmed" in self.outputs:
            discard_untrimmed = True                                      # (the UntrimmedFilter is on, trim/__init__.py:617)
        common = dict(times=times, action=action, nextseq_trim=nextseq_trim, quality_cutoff=quality_cutoff,
                      quality_base=quality_base, trim_n=trim_n, minimum_length=minimum_length,
                      maximum_length=maximum_length, max_n=max_n, discard_trimmed=discard_trimmed,
                      discard_untrimmed=discard_untrimmed, op_order=op_order, aux=aux, length_tag=length_tag,
                      strip_suffix=strip_suffix, prefix=prefix, suffix=suffix, zero_cap=zero_cap, report=report)
        self.aux = dict(aux) if aux else None
        if (aux or length_tag or strip_suffix or prefix or suffix or zero_cap) and (aligner != "adapter" or merge_overlapping):
            raise NotImplementedError("--info-file / --rest-file / --wildcard-file, read-name modifiers and --zero-cap with "
                                      "the insert aligner or with merging")
        self.p1 = TrimPipeline(adapters=adapters1, cut=cut, cut_min=cut_min, bisulfite=bisulfite, **common)
        self.p2 = TrimPipeline(adapters=adapters2, cut=cut2, cut_min=cut_min2, bisulfite=bisulfite2, **common)
        if (bisulfite or bisulfite2) and aligner != "adapter":
            raise NotImplementedError("--bisulfite with the insert aligner")
        self.aligner, self.action, self.op_order = aligner, action, op_order
        if pair_filter not in ("any", "both"):
            raise ValueError("pair_filter must be 'any' or 'both'")
        self.min_affected = 2 if pair_filter == "both" else 1            # trim/__init__.py:549
        if correct_mismatches not in (None, "liberal", "conservative", "N"):
            raise ValueError("correct_mismatches must be 'liberal', 'conservative' or 'N'")
        if correct_mismatches and aligner != "insert" and not merge_overlapping:
            raise ValueError("error correction needs the insert aligner or --merge-overlapping")
        self.merge_overlapping = bool(merge_overlapping)
        # above 1: a number of bases; up to 1: a fraction of the shorter read (modifiers.py:867)
        self.merge_min_overlap = merge_min_overlap if merge_min_overlap <= 1 else int(merge_min_overlap)
        self.merge_error_rate = float(merge_error_rate)
        self.merged_pairs = 0
        self.correct_mismatches = correct_mismatches
        self.corrected_pairs, self.corrected_bp = 0, [0, 0]               # ErrorCorrectorMixin counters
        self.insert = None
        if aligner == "insert":
            from .adapters import BACK
            from .align import InsertAligner
            if len(self.p1.adapters) != 1 or len(self.p2.adapters) != 1 or any(
                    isinstance(a, LinkedAdapter) or a.where != BACK for a in self.p1.adapters + self.p2.adapters):
                raise ValueError("Insert aligner requires a single 3' adapter for each read")   # trim/__init__.py:406-411
            self.insert = InsertAligner(self.p1.adapters[0].sequence, self.p2.adapters[0].sequence, **(insert_args or {}))
        elif aligner != "adapter":
            raise ValueError("aligner must be 'adapter' or 'insert'")

    @staticmethod
    def _fallback(adapter, batch, st, miss, n):
        """Adapter.match_to records for the reads listed in ``miss`` (-1 records elsewhere)."""
        none = torch.zeros((n, 8), dtype=torch.int16, device=st[0].device)
        none[:, 1] = -1
        if miss.numel() == 0:
            return none
        if miss.numel() == n:
            return adapter.match_source(RecordSource(batch, st[0], st[1]))
        sub = FastqBatch(batch.data, batch.nbytes, batch.records.index_select(0, miss).contiguous(), batch.backend)
        rec = adapter.match_source(RecordSource(sub, st[0].index_select(0, miss).contiguous(),
                                                st[1].index_select(0, miss).contiguous()))
        none[miss] = rec
        return none

    def _insert_stage(self, mate1, mate2):
        """InsertAdapterCutter over the batch (commands/trim/modifiers.py:391-496): sets the mates' adapter flags (and
        unmasked intervals); returns (the pairs with an insert match, the pairs it corrected or None)."""
        b1, b2, st1, st2 = mate1.batch, mate2.batch, (mate1.begin, mate1.end), (mate2.begin, mate2.end)
        be = b1.backend
        n = len(b1)
        src1, src2 = RecordSource(b1, st1[0], st1[1]), RecordSource(b2, st2[0], st2[1])
        max_len = 0
        if n:
            max_len = int(torch.maximum((st1[1] - st1[0]).max(), (st2[1] - st2[0]).max()).clamp_(min=0).item())
        if max_len > _lib.INSERT_MAX_READ:
            raise _lib.AtroposHipError("InsertAligner: reads longer than %d bases are outside the device envelope"
                                       % _lib.INSERT_MAX_READ)
        table = be.translate_table(_lib.TABLE_DNA15)
        pb1 = src1.planes(max_len, _lib.TABLE_DNA15, table, count=True)
        pb2 = src2.planes(max_len, _lib.TABLE_DNA15, table, count=True)
        if pb1.uncoded_reads or pb2.uncoded_reads:
            # soft-masked reads: match_insert tells the cases apart in the insert compare and folds them in the adapter
            # compares (atr_insert_match_batch_coded) -- both reads again, with the case-sensitive codes
            table = be.case_sensitive_table()
            pb1 = src1.planes(max_len, _lib.TABLE_CUSTOM, table)
            pb2 = src2.planes(max_len, _lib.TABLE_CUSTOM, table)
        # match_insert complements read 2 only as far as read 1 reaches (align/__init__.py:259-267)
        bad = be.planes_count_uncoded(pb2.packed, pb2.lens, pb1.lens, n, max_len)
        if bad:
            raise ValueError("%d second read(s) contain bases without an upper-case IUPAC code where they face the first "
                             "read; the device insert aligner cannot reverse-complement them" % bad)
        ins = self.insert.match_insert_batch(pb1, pb2).records
        insert_matched = (ins[:, 0, 1] >= 0).to(torch.uint8)                # read.insert_overlap, modifiers.py:397
        # semi-global fallback (modifiers.py:405-407): only the pairs without an insert match need it
        miss = torch.nonzero(ins[:, 0, 1] < 0).squeeze(1)
        fb1 = self._fallback(self.p1.adapters[0], b1, st1, miss, n)
        fb2 = self._fallback(self.p2.adapters[0], b2, st2, miss, n)
        action = {None: 0, "trim": 1, "mask": 2}[self.action]
        uend1 = uend2 = None
        if action == 2:
            uend1, uend2 = st1[1].clone(), st2[1].clone()
        from .modifiers import COMP_TABLE, _ACTIONS
        correct = _ACTIONS[self.correct_mismatches] if self.correct_mismatches else -1
        # NB: with error correction the bases / qualities of both FASTQ chunks are rewritten in place
        matched1, matched2, corrected, err = be.insert_plan_batch(
            ins.contiguous(), fb1.contiguous(), fb2.contiguous(), b1, b2, st1[0], st1[1], st2[0], st2[1], uend1, uend2,
            self.insert.min_insert_overlap, True, action, correct, 1, COMP_TABLE)
        _raise_device_error(err)
        for m, matched, uend in ((mate1, matched1, uend1), (mate2, matched2, uend2)):
            m.matched, m.ubegin, m.uend = matched, (m.begin.clone() if action == 2 else None), uend
        # read.corrected of both reads: a later correct_errors call (MergeOverlapping) returns at once for these pairs
        # (modifiers.py:232-233) -- also for the ones corrected from complementary fallback matches, which have no
        # insert match
        return insert_matched, (self._count_corrected(corrected) if correct >= 0 else None)

    def _overwrite_stage(self, mate1, mate2):
        """OverwriteRead over the batch (commands/trim/modifiers.py:538-563) on the reads as they are now: where one
        read's first WINDOW kept qualities average below LOWQ and the other's at least HIGHQ, the worse read becomes
        the reverse complement of the better one -- real text appended to the worse read's chunk
        (atr_overwrite_plan_batch + atr_overwrite_apply_batch), its record re-pointed, its interval the whole clone,
        its adapter flag (and last adapter) the better read's."""
        from .modifiers import COMP_TABLE
        lowq, highq, window = self.overwrite_low_quality
        mates = (mate1, mate2)
        n = len(mate1.batch)
        if n == 0:
            return
        for m in mates:                                                   # the reference's clone carries the N's
            if m.ubegin is not None:
                write_mask(m.batch, m.begin, m.end, m.ubegin, m.uend)
                m.ubegin = m.uend = None
        b1, b2 = mate1.batch, mate2.batch
        be = b1.backend
        which, grow1, grow2 = be.overwrite_plan(b1, mate1.begin, mate1.end, b2, mate2.begin, mate2.end, lowq, highq, window,
                                                self.p1.quality_base)
        need = (int(grow1[n].item()), int(grow2[n].item()))
        if not any(need):
            return
        shared = b1.data.data_ptr() == b2.data.data_ptr()                 # (an interleaved chunk: one tail behind the other)

        def grown(data, extra):
            base = (data.numel() + 15) // 16 * 16
            if base + extra >= (1 << 32) - 16:
                raise ValueError("the chunk and its rewritten names must stay below 4 GiB")
            pad = torch.zeros((base - data.numel() + extra + 16,), dtype=torch.uint8, device=data.device)
            return torch.cat([data, pad]), base

        if shared:
            data1, tail1 = grown(b1.data, need[0] + need[1])
            data2, tail2 = data1, tail1 + need[0]
            ends = (tail1 + need[0] + need[1],) * 2
        else:
            (data1, tail1), (data2, tail2) = grown(b1.data, need[0]), grown(b2.data, need[1])
            ends = (tail1 + need[0], tail2 + need[1])
        rec1, rec2 = b1.records.clone(), b2.records.clone()
        err = be.overwrite_apply(data1, rec1, mate1.begin, mate1.end, data2, rec2, mate2.begin, mate2.end, which, grow1, grow2,
                                 tail1, tail2, COMP_TABLE)
        if err != _lib.INT64_MAX:
            raise KeyError("--overwrite-low-quality: pair %d: base without a complement" % (err // 8))
        # (nbytes covers the clones: the read-name modifiers read the names from the chunk's first nbytes)
        mate1.batch = FastqBatch(data1, max(b1.nbytes, ends[0]), rec1, be, b1.line_ends, b1.stride)
        mate2.batch = FastqBatch(data2, max(b2.nbytes, ends[1]), rec2, be, b2.line_ends, b2.stride)
        first, second = which == 1, which == 2
        m1, m2 = mate1.matched, mate2.matched
        mate1.matched, mate2.matched = torch.where(first, m2, m1), torch.where(second, m1, m2)
        if mate1.last_which is not None:
            w1, w2 = mate1.last_which, mate2.last_which
            mate1.last_which, mate2.last_which = torch.where(first, w2, w1), torch.where(second, w1, w2)
            mate1.foreign, mate2.foreign = (first, self.p2.adapters), (second, self.p1.adapters)
        self.overwritten[0] += int(first.sum().item())
        self.overwritten[1] += int(second.sum().item())

    def _count_corrected(self, corrected):
        """ErrorCorrectorMixin's counters over the changed-base counts of a batch; returns the pairs with a change."""
        pairs = (corrected.sum(dim=1) > 0).to(torch.uint8)
        self.corrected_pairs += int(pairs.sum().item())
        tot = corrected.sum(dim=0).cpu().tolist()
        self.corrected_bp[0] += int(tot[0])
        self.corrected_bp[1] += int(tot[1])
        return pairs

    def _merge_stage(self, b1, b2, st1, st2, insert_matched, already_corrected=None):
        """MergeOverlapping over the batch: the alignments ``Aligner(reverse_complement(read2), error_rate,
        flags).locate(read1)`` of the pairs long enough to be tried (atr_locate_pairs_batch, one call per
        flag set), then the merge itself.  Returns (merged flags uint8 [n], merged FASTQ text)."""
        from .align import SEMIGLOBAL, START_WITHIN_SEQ1, STOP_WITHIN_SEQ2
        from .modifiers import COMP_TABLE, _ACTIONS
        be = b1.backend
        n = len(b1)
        dev = st1[0].device
        len1, len2 = (st1[1] - st1[0]).clamp(min=0), (st2[1] - st2[0]).clamp(min=0)
        shorter = torch.minimum(len1, len2)
        if self.merge_min_overlap > 1:
            need = torch.full_like(shorter, int(self.merge_min_overlap))
        else:                                                              # max(2, round(frac * shorter)), :870-874
            need = torch.round(shorter.to(torch.float64) * float(self.merge_min_overlap)).to(torch.int32).clamp(min=2)
        tried = shorter >= need                                            # :876-877
        if insert_matched is None:
            insert_matched = torch.zeros((n,), dtype=torch.uint8, device=dev)
        align = torch.zeros((n, 8), dtype=torch.int16, device=dev)
        align[:, 1] = -1
        from .align import case_sensitive_pair_table
        tables = [be.translate_table(_lib.TABLE_DNA15)]
        tables.append(case_sensitive_pair_table(tables[0]))     # soft-masked reads: second try, both reads with it
        for flags, group in ((START_WITHIN_SEQ1 | STOP_WITHIN_SEQ2, tried & (insert_matched != 0)),
                             (SEMIGLOBAL, tried & (insert_matched == 0))):      # :879-886
            idx = torch.nonzero(group).squeeze(1)
            if idx.numel() == 0:
                continue
            sides = []
            for b, st in ((b2, st2), (b1, st1)):                            # reference = read 2, query = read 1
                sub = b if idx.numel() == n else FastqBatch(b.data, b.nbytes, b.records.index_select(0, idx).contiguous(),
                                                            b.backend)
                begin, end = (st[0], st[1]) if idx.numel() == n else (st[0].index_select(0, idx).contiguous(),
                                                                      st[1].index_select(0, idx).contiguous())
                max_len = int((end - begin).max().clamp_(min=0).item())
                if max_len > _lib.MAX_READ_LEN:
                    raise _lib.AtroposHipError("MergeOverlapping: reads longer than %d bases are outside the device "
                                               "envelope" % _lib.MAX_READ_LEN)
                sides.append((sub, begin, end, max_len))
            for table in tables:
                # the aligner compares characters (_align.pyx:390-391): upper-case IUPAC codes first; if a read is
                # soft-masked, both reads again with the table that tells the cases apart
                packs, bad = [], 0
                for sub, begin, end, max_len in sides:
                    packed, lens, nbad = be.pack_records(sub.data, sub.records, begin, end, max_len, table, count_invalid=True)
                    packs.append((packed, lens, max_len))
                    bad += nbad
                if not bad:
                    break
            if bad:
                raise ValueError("%d read(s) contain characters the device pair aligner has no 4-bit code for (upper-case "
                                 "IUPAC letters, or A C G T N W B D H V in either case)" % bad)
            (rp, rl, rmax), (qp, ql, qmax) = packs
            # the merge below only looks at alignments with matches >= need (modifiers.py:896-897)
            need_g = need.to(torch.int32) if idx.numel() == n else need.to(torch.int32).index_select(0, idx)
            if max(rmax, qmax) > _lib.PAIRS_MAX_LEN:        # reads of 321 .. 736 bases: the per-pair aligner's long path
                from .align import long_pairs_records
                rec = long_pairs_records(be, rp, rl, rmax, True, qp, ql, qmax, int(idx.numel()), self.merge_error_rate, flags,
                                         False, False, 1, 1)
            else:
                rec = be.locate_pairs_batch(rp, rl, rmax, True, qp, ql, qmax, int(idx.numel()), self.merge_error_rate, flags,
                                            False, False, 1, 1, need=need_g.contiguous())
            if idx.numel() == n:
                align = rec
            else:
                align[idx] = rec
        correct = _ACTIONS[self.correct_mismatches] if self.correct_mismatches else -1
        # pairs the merge must not correct: bit 0 the insert aligner saw them (modifiers.py:900), bit 1 a read of
        # the pair was corrected before (correct_errors' own guard, :232-233)
        no_correct = insert_matched if already_corrected is None else insert_matched | (already_corrected << 1)
        kind, text, corrected, err = be.merge_batch(align.contiguous(), need.to(torch.int32).contiguous(),
                                                    no_correct.contiguous(), b1, b2, st1[0], st1[1], st2[0], st2[1],
                                                    correct, 1, COMP_TABLE)
        _raise_device_error(err)
        merged = kind != 0
        if correct >= 0:
            self._count_corrected(corrected)
        self.merged_pairs += int(merged.sum().item())
        return merged, text

    def run(self, batch1, batch2):
        if len(batch1) != len(batch2):
            raise ValueError("the two FASTQ batches hold different numbers of records")
        pipes, mates = (self.p1, self.p2), (_Mate(self.p1, batch1), _Mate(self.p2, batch2))
        insert = (lambda: self._insert_stage(*mates)) if self.aligner == "insert" else None
        overwrite = (lambda: self._overwrite_stage(*mates)) if self.overwrite_low_quality else None
        insert_matched, already_corrected = _run_stages(pipes, mates, insert, overwrite) or (None, None)
        masks = [pipe._filter_stage(m, masks=True) for pipe, m in zip(pipes, mates)]
        dest = batch1.backend.pair_filter_batch(masks[0], masks[1], self.min_affected)
        merged_text = None
        if self.merge_overlapping:                                  # the last modifier, the first filter
            if self.action == "mask":
                # masked adapters: MergeOverlapping sees the reads with their N's (modifiers.py:155-172 made them part of
                # the sequence): written into the chunk here, the intervals then need no mask any more
                for m in mates:
                    if m.ubegin is not None:
                        write_mask(m.batch, m.begin, m.end, m.ubegin, m.uend)
                        m.ubegin = m.uend = None
            m1, m2 = mates
            merged, merged_text = self._merge_stage(batch1, batch2, (m1.begin, m1.end), (m2.begin, m2.end), insert_matched,
                                                    already_corrected)
            dest = torch.where(merged, torch.full_like(dest, DEST_MERGED), dest)
        return PairedTrimResult(self.p1._result(mates[0], dest), self.p2._result(mates[1], dest), merged_text)

    def trim_files(self, in1, in2, out1, out2=None, chunk_bytes=128 << 20, merged_out=None, keep_output=False, output_parts=1,
                   device_gzip=False, device_gunzip=False, input_format=None):
        """Stream two FASTQ files through the GPU in lock step (chunks of whole records, the
        same number from each file); returns the destination counts.

        ``in2=None``: ``in1`` is an INTERLEAVED file, read 1 and read 2 of every pair in turn (the reference's
        ``-l``; ``fastq.read_chunks(interleaved=True)``): an odd number of records is a ``FormatError``, the names of
        the two reads are not compared.  ``out2=None``: ``out1`` is written interleaved (the reference's ``-L``):
        one formatter call (``atr_fastq_emit_pairs``) and one sink per chunk; ``device_gzip`` and ``output_parts``
        act on that sink as on any other.  A merged output stays a file of its own.  Interleaved output together
        with the filtered pairs' own files (``outputs=``) is a NotImplementedError: the reference interleaves those
        files too (trim/__init__.py:568-573), which is not provided.

        ``merged_out``: the
        --merged-output file (without it merged reads are dropped, as by the reference).
        ``output_parts`` > 1: every output as that many part files (``TrimPipeline.trim_file``); part i of
        ``out1`` and part i of ``out2`` hold the same pairs in the same order.  ``device_gzip``: the outputs
        (all ending in ``.gz``) are compressed on the GPU, as in ``TrimPipeline.trim_file``.  ``device_gunzip``: BGZF
        ``.gz`` inputs are inflated on the GPU, as in ``TrimPipeline.trim_file``.  FASTA input and output, and
        ``input_format``, as in ``TrimPipeline.trim_file``; both inputs are of one format, interleaved FASTA is a
        NotImplementedError."""
        if device_gzip and any(p is not None and "{name}" in str(p) for p in (out1, out2, merged_out)):
            raise NotImplementedError("device_gzip with demultiplexed outputs ({name} in the output path)")
        if any(p is not None and "{name}" in str(p) for p in (out1, out2, merged_out)):
            raise ValueError("Demultiplexing not supported for paired-end files, yet.")        # trim/cli.py:769-771
        return _trim_stream(self, [in1] if in2 is None else [in1, in2], [out1] if out2 is None else [out1, out2], chunk_bytes,
                            keep_output, output_parts, merged_out, device_gzip=device_gzip, device_gunzip=device_gunzip,
                            input_format=input_format)

    def trim_bytes(self, data1, data2, which=_lib.DEST_KEEP, input_format=None, fmt=None):
        """Two FASTQ (FASTA) texts in (same number of records, one format), the two trimmed texts out; ``input_format``
        and ``fmt`` as in ``TrimPipeline.trim_bytes``."""
        b1, b2 = _batch_from_bytes(self, data1, input_format), _batch_from_bytes(self, data2, input_format)
        if getattr(b1, "fmt", "fastq") != getattr(b2, "fmt", "fastq"):
            raise ValueError("the two inputs are of different formats")
        return self.run(b1, b2).text(which, fmt)


class LegacyPairedPipeline(PairedTrimPipeline):
    """Paired-end input without any option that switches full paired-end trimming on (-A / -G / -B / -U, -q,
    --trim-n, --pair-filter ...): the reference's backwards-compatible 'legacy mode' (trim/cli.py:630-648) -- the
    single-end pipeline on read 1, its filters on read 1 alone (FilterFactory wraps them in SingleWrapper,
    filters.py:100-107), read 2 written as it came for every pair that is kept."""

    def __init__(self, first):
        self.first = self.p1 = first                                      # (trim_files reads p1's filter settings)
        self.stats, self.aux, self.outputs, self.merge_overlapping = (), None, {}, False
        self.report = first.report

    def run(self, batch1, batch2):
        if len(batch1) != len(batch2):
            raise ValueError("the two FASTQ batches hold different numbers of records")
        res1 = self.first.run(batch1)
        n = len(batch2)
        dev = batch2.records.device
        res2 = TrimResult(batch2, torch.zeros((n,), dtype=torch.int32, device=dev), batch2.seq_lens.clone(), None, None,
                          torch.zeros((n,), dtype=torch.uint8, device=dev), res1.dest)
        return PairedTrimResult(res1, res2)


def pipeline_from_args(argv, paired_input=False, report=False):
    """Build a TrimPipeline (or, when paired-end options are present, a PairedTrimPipeline) from
    the subset of ``atropos trim`` command-line options the device pipeline covers (same
    spellings and defaults as trim/cli.py:57-335, :455-530, :655-803).  Anything else raises --
    the caller then uses the per-read object path.  ``paired_input``: the reads come as pairs (-pe1 / -pe2); without
    an option that asks for full paired-end trimming that is the reference's legacy mode (LegacyPairedPipeline).
    ``report``: the pipelines' ``report=`` (the trim report, atropos_amd.report)."""
    import argparse
    from .adapters import AdapterParser
    if isinstance(argv, str):
        argv = argv.split()
    ap = argparse.ArgumentParser(prog="atropos_amd.trim", add_help=False)
    ap.add_argument("-a", "--adapter", action="append", default=[], dest="adapters")
    ap.add_argument("-g", "--front", action="append", default=[])
    ap.add_argument("-b", "--anywhere", action="append", default=[])
    ap.add_argument("-A", action="append", default=[], dest="adapters2")
    ap.add_argument("-G", action="append", default=[], dest="front2")
    ap.add_argument("-B", action="append", default=[], dest="anywhere2")
    ap.add_argument("--aligner", choices=("adapter", "insert"), default="adapter")
    ap.add_argument("-e", "--error-rate", type=float, default=None)
    ap.add_argument("-O", "--overlap", type=int, default=None)
    ap.add_argument("-n", "--times", type=int, default=1)
    ap.add_argument("-N", "--no-match-adapter-wildcards", action="store_false", dest="match_adapter_wildcards",
                    default=True)
    ap.add_argument("--match-read-wildcards", action="store_true", default=False)
    ap.add_argument("--no-indels", action="store_false", dest="indels", default=True)
    ap.add_argument("--indel-cost", type=int, default=None)
    ap.add_argument("--adapter-max-rmp", type=float, default=None)
    ap.add_argument("--insert-max-rmp", type=float, default=1E-6)
    ap.add_argument("--insert-match-error-rate", type=float, default=None)
    ap.add_argument("--insert-match-adapter-error-rate", type=float, default=None)
    ap.add_argument("--no-trim", action="store_true", default=False)
    ap.add_argument("--mask-adapter", action="store_true", default=False)
    ap.add_argument("--op-order", default="CGQAW")
    ap.add_argument("-u", "--cut", type=int, action="append", default=[])
    ap.add_argument("-U", type=int, action="append", default=[], dest="cut2")
    ap.add_argument("--bisulfite", default=None)
    ap.add_argument("--cut-min", type=int, action="append", default=[])
    ap.add_argument("--cut-min2", type=int, action="append", default=[])
    ap.add_argument("-q", "--quality-cutoff", default=None)
    ap.add_argument("--quality-base", type=int, default=33)
    ap.add_argument("--nextseq-trim", type=int, default=None)
    ap.add_argument("--trim-n", action="store_true", default=False)
    ap.add_argument("-m", "--minimum-length", type=int, default=None)
    ap.add_argument("-M", "--maximum-length", type=int, default=None)
    ap.add_argument("--max-n", type=float, default=None)
    ap.add_argument("--discard-trimmed", "--discard", action="store_true", default=False)
    ap.add_argument("--discard-untrimmed", "--trimmed-only", action="store_true", default=False)
    ap.add_argument("--pair-filter", choices=("any", "both"), default=None)
    ap.add_argument("--correct-mismatches", choices=("liberal", "conservative", "N"), default=None)
    ap.add_argument("-R", "--merge-overlapping", action="store_true", default=False)
    ap.add_argument("--merge-min-overlap", type=float, default=0.9)
    ap.add_argument("--merge-error-rate", type=float, default=None)
    ap.add_argument("-x", "--prefix", default="")
    ap.add_argument("-y", "--suffix", default="")
    ap.add_argument("--strip-suffix", action="append", default=[])
    ap.add_argument("--length-tag", default=None)
    ap.add_argument("-z", "--zero-cap", action="store_true", default=False)
    ap.add_argument("--too-short-output", default=None)
    ap.add_argument("--too-long-output", default=None)
    ap.add_argument("--untrimmed-output", default=None)
    ap.add_argument("--too-short-paired-output", default=None)
    ap.add_argument("--too-long-paired-output", default=None)
    ap.add_argument("--untrimmed-paired-output", default=None)
    ap.add_argument("--info-file", default=None)
    ap.add_argument("--rest-file", "-r", default=None)
    ap.add_argument("--wildcard-file", default=None)
    ap.add_argument("-w", "--overwrite-low-quality", default=None)
    ap.add_argument("-l", "--interleaved-input", default=None)
    ap.add_argument("-L", "--interleaved-output", default=None)
    ap.add_argument("--input-read", type=int, choices=(0, 1, 2), default=0)
    o = ap.parse_args(argv)
    if o.input_read:
        raise NotImplementedError("--input-read 1 | 2 (one read of the pairs of a SAM / BAM file) is not provided")
    paired_input = bool(paired_input or o.interleaved_input)              # (-l is paired input, cli.py:614-618)
    overwrite = None
    if o.overwrite_low_quality:                                           # three comma-separated ints (cli.py:284-291)
        overwrite = tuple(int(v) for v in str(o.overwrite_low_quality).split(","))
        if len(overwrite) != 3:
            raise ValueError("--overwrite-low-quality takes LOWQ,HIGHQ,WINDOW")
    paired = bool(o.adapters2 or o.front2 or o.anywhere2 or o.cut2 or o.cut_min2 or o.pair_filter or o.aligner == "insert" or
                  o.merge_overlapping or (overwrite and paired_input))
    if overwrite and not paired_input:
        raise ValueError("--overwrite-low-quality is not valid for single-end reads")     # cli.py:741-744
    if overwrite and overwrite[0] > overwrite[1]:
        raise ValueError("For --overwrite-low-quality, LOWQ must be <= HIGHQ")              # cli.py:745-748
    for cm in (o.cut_min, o.cut_min2):                                     # cli.py:810-830
        if len(cm) > 2:
            raise ValueError("You cannot remove bases from more than two ends.")
        if len(cm) == 2 and cm[0] * cm[1] > 0:
            raise ValueError("You cannot remove bases from the same end twice.")
    if paired_input:
        # cli.py:630-641, the reference's own list: any of these asks for full paired-end trimming, none of them is its
        # legacy mode.  (--aligner insert and -R are NOT on it: the reference then modifies read 1 alone, which the insert
        # aligner and the merge stage have no meaning for -- refused here rather than run as something else)
        full = bool(o.adapters2 or o.front2 or o.anywhere2 or o.cut2 or o.cut_min2 or o.quality_cutoff or o.trim_n or
                    o.pair_filter or o.too_short_paired_output or o.too_long_paired_output or o.interleaved_input or overwrite)
        if not full and (o.aligner == "insert" or o.merge_overlapping):
            raise NotImplementedError("--aligner insert / --merge-overlapping with paired-end input and none of the options "
                                      "that switch the reference's legacy mode off (trim/cli.py:630-641)")
        legacy = not full
        paired = full
    else:
        legacy = False
    if o.merge_min_overlap <= 0:
        raise ValueError("--merge-min-overlap must be positive")          # positive(float, True), cli.py:206-207
    if o.merge_overlapping and o.merge_error_rate is None:
        o.merge_error_rate = o.error_rate or 0.2                          # cli.py:690-691 (before -e gets its default)
    insert_args = None
    if o.aligner == "adapter":                                            # cli.py:659-666
        if o.indels and o.indel_cost is None:
            o.indel_cost = 1
        if o.overlap is None:
            o.overlap = 3 if o.adapter_max_rmp is None else 1
    else:                                                                 # cli.py:667-684
        if o.indels and o.indel_cost is None:
            o.indel_cost = 3
        if o.overlap is None:
            o.overlap = 1
            if o.adapter_max_rmp is None:
                o.adapter_max_rmp = 1E-6
        if o.insert_match_error_rate is None:
            o.insert_match_error_rate = o.error_rate or 0.2
        if o.insert_match_adapter_error_rate is None:
            o.insert_match_adapter_error_rate = o.insert_match_error_rate
        insert_args = dict(insert_max_rmp=o.insert_max_rmp, max_insert_mismatch_frac=o.insert_match_error_rate,
                           max_adapter_mismatch_frac=o.insert_match_adapter_error_rate,
                           read_wildcards=o.match_read_wildcards, adapter_wildcards=o.match_adapter_wildcards)
    if o.error_rate is None:
        o.error_rate = 0.1                                                # cli.py:801-802
    for cut in (o.cut, o.cut2):
        if len(cut) > 2 or (len(cut) == 2 and cut[0] * cut[1] > 0):
            raise ValueError("You cannot remove bases from the same end twice.")
    qc = None
    if o.quality_cutoff is not None:
        qc = [int(x) for x in str(o.quality_cutoff).split(",")]
        if all(c <= 0 for c in qc):
            qc = None                                                     # :750-754
        elif len(qc) == 1:
            qc = [0] + qc
    from .util import RandomMatchProbability
    kwargs = dict(max_error_rate=o.error_rate, min_overlap=o.overlap, read_wildcards=o.match_read_wildcards,
                  adapter_wildcards=o.match_adapter_wildcards, indels=o.indels,
                  match_probability=RandomMatchProbability())             # trim/__init__.py:345, :364
    if o.indel_cost is not None:
        kwargs["indel_cost"] = o.indel_cost
    if o.adapter_max_rmp:
        kwargs["max_rmp"] = o.adapter_max_rmp                             # trim/__init__.py:367-368
    parser = AdapterParser(**kwargs)
    adapters = parser.parse_multi(o.adapters, o.anywhere, o.front)
    action = None if o.no_trim else ("mask" if o.mask_adapter else "trim")    # trim/cli.py:103-111
    adapters2 = parser.parse_multi(o.adapters2, o.anywhere2, o.front2) if paired else []
    if (not adapters and not adapters2 and not qc and o.nextseq_trim is None and not o.cut and not o.cut2 and
            (o.minimum_length is None or o.minimum_length <= 0) and o.maximum_length is None and not o.trim_n and
            o.max_n is None and not overwrite):
        raise ValueError("You need to provide at least one adapter sequence.")        # trim/__init__.py:386-404
    if action == "mask" and any(isinstance(a, LinkedAdapter) for a in adapters + adapters2):
        raise NotImplementedError("--mask-adapter with a linked adapter: the reference's AdapterCutter fails on it "
                                  "(LinkedMatch has no astart, modifiers.py:158)")
    common = dict(times=o.times, action=action, nextseq_trim=o.nextseq_trim, quality_cutoff=qc,
                  quality_base=o.quality_base, trim_n=o.trim_n, minimum_length=o.minimum_length,
                  maximum_length=o.maximum_length, max_n=o.max_n, discard_trimmed=o.discard_trimmed,
                  discard_untrimmed=o.discard_untrimmed, op_order=o.op_order, report=report)
    bis1 = bis2 = None
    if o.bisulfite:                                                       # cli.py:702-739, trim/__init__.py:497-516
        kind = o.bisulfite
        if kind == "swift":
            if not paired:
                raise ValueError("Swift trimming is only compatible with paired-end reads")
            bis1, bis2 = [("min", 0, 10, False, False)], [("min", 10, 0, False, False)]
        elif kind == "non-directional":
            # (the reference's run fails at the end: NonDirectionalBisulfiteTrimmer.summarize reads the RRBS cutter it
            # only has with rrbs, modifiers.py:824-831)
            raise NotImplementedError("--bisulfite non-directional: the reference command fails on it")
        elif kind == "non-directional-rrbs":
            bis1 = bis2 = [("nondir", True)]
        elif kind == "rrbs":
            bis1 = bis2 = [("min", 0, 2, False, True)]
        elif kind in ("truseq", "epignome"):
            bis1 = bis2 = None                                            # (the reference adds no modifier for these)
        else:
            specs = []
            for arg in kind.split(";"):
                parts = [int(x) for x in arg.split(",")]
                if len(parts) != 4:
                    raise ValueError("Invalidate format for bisulfite parameters")
                # (cli.py:714-729: the flags index the tuple (False, True) -- 0 / 1, and -2 / -1 by Python's indexing; anything
                #  else is the parser's format error.  One negative length is accepted there and handed to MinCutter as
                #  it is: refused here rather than guessed at.)
                if any(f not in (0, 1, -1, -2) for f in parts[2:]):
                    raise ValueError("Invalidate format for bisulfite parameters")
                if parts[0] <= 0 and parts[1] <= 0:
                    specs.append(None)
                    continue
                if parts[0] < 0 or parts[1] < 0:
                    raise NotImplementedError("--bisulfite with a negative length next to a positive one")
                specs.append([("min", parts[0], parts[1], (False, True)[parts[2]], (False, True)[parts[3]])])
            if paired and len(specs) == 1:
                specs = [specs[0], specs[0]]
            elif not paired and len(specs) > 1:
                raise ValueError("Too many bisulfite parameters for single-end reads")
            bis1, bis2 = specs[0], (specs[1] if len(specs) > 1 else None)
    if legacy and (bis1 or bis2):
        raise NotImplementedError("--bisulfite with paired-end input in legacy mode")
    aux = {kind: path for kind, path in (("info", o.info_file), ("rest", o.rest_file), ("wildcard", o.wildcard_file)) if path}
    outputs = {kind: path for kind, path in (("too_short", o.too_short_output), ("too_long", o.too_long_output),
                                             ("untrimmed", o.untrimmed_output)) if path}
    if paired and outputs:
        second = dict(too_short=o.too_short_paired_output, too_long=o.too_long_paired_output, untrimmed=o.untrimmed_paired_output)
        if any(second[kind] is None for kind in outputs):
            raise NotImplementedError("paired-end input: --too-short-output / --too-long-output / --untrimmed-output need "
                                      "their --*-paired-output as well")
        outputs = {kind: (path, second[kind]) for kind, path in outputs.items()}
    if legacy and (aux or outputs or o.length_tag or o.strip_suffix or o.prefix or o.suffix or o.zero_cap):
        raise NotImplementedError("side files and read-name modifiers with paired-end input in legacy mode")
    if o.interleaved_output and outputs:
        raise NotImplementedError("interleaved output with --too-short-output / --too-long-output / --untrimmed-output "
                                  "(the reference interleaves those files as well)")
    if o.interleaved_output and not (paired or legacy):                   # (-l alone made the input paired above)
        raise ValueError("interleaved output needs paired-end input")
    pipe = _pipeline_from_options(o, paired, legacy, adapters, adapters2, common, bis1, bis2, aux, outputs, insert_args,
                                  overwrite)
    # the two paths are the caller's to hand to trim_files (in2=None / out2=None)
    pipe.interleaved_input, pipe.interleaved_output = o.interleaved_input, o.interleaved_output
    return pipe


def _pipeline_from_options(o, paired, legacy, adapters, adapters2, common, bis1, bis2, aux, outputs, insert_args,
                           overwrite=None):
    """The pipeline object of ``pipeline_from_args`` once its options are checked."""
    if not paired:
        first = TrimPipeline(adapters=adapters, cut=o.cut, cut_min=o.cut_min, bisulfite=bis1, aux=aux or None, outputs=outputs or None, length_tag=o.length_tag,
                             strip_suffix=o.strip_suffix, prefix=o.prefix, suffix=o.suffix, zero_cap=o.zero_cap, **common)
        return LegacyPairedPipeline(first) if legacy else first
    return PairedTrimPipeline(outputs=outputs or None, aux=aux or None, length_tag=o.length_tag, strip_suffix=o.strip_suffix, prefix=o.prefix,
                              suffix=o.suffix, zero_cap=o.zero_cap, adapters1=adapters, adapters2=adapters2, aligner=o.aligner, cut=o.cut, cut2=o.cut2,
                              cut_min=o.cut_min, cut_min2=o.cut_min2, bisulfite=bis1, bisulfite2=bis2,
                              pair_filter=o.pair_filter or "any", insert_args=insert_args, overwrite_low_quality=overwrite,
                              correct_mismatches=o.correct_mismatches, merge_overlapping=o.merge_overlapping,
                              merge_min_overlap=o.merge_min_overlap,
                              merge_error_rate=0.2 if o.merge_error_rate is None else o.merge_error_rate, **common)

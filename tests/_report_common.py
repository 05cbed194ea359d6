"""Shared by test_report_host.py and test_gpu_report.py: the golden cases of tests/golden/trim_report.json.gz, the
comparison rule, and the per-object host path the small shapes are compared with."""
import base64

import numpy as np

from atropos_amd.fastq import FastqBatch
from atropos_amd.report import TrimReport
from atropos_amd.trim import pipeline_from_args

from .conftest import load_golden

KINDS = ("info", "rest", "wildcard", "too_short", "too_short2", "too_long", "too_long2", "untrimmed", "untrimmed2")


# ---------------------------------------------------------------------------------------------- golden cases
_GOLDEN = None
_INPUTS = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden("trim_report.json.gz")
    return _GOLDEN


def input_text(name):
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = load_golden("trim_cases.json.gz")["inputs"]
    return base64.b64decode(_INPUTS[name])


def case_ids(kind):
    return ["%d:%s" % (i, c["args"][:60]) for i, c in enumerate(golden()[kind])]


def plain(obj, key=None):
    """A report summary as the fixture stores the reference's (make_trim_report_golden.py): tuples as lists, keys as
    strings, an adapter without a name of its own (a running number) as "#<position in its cutter>"."""
    if isinstance(obj, dict):
        if key == "adapters":
            return {("#%d" % pos if str(k).isdigit() else str(k)): plain(v) for pos, (k, v) in enumerate(obj.items(), 1)}
        return {str(k): plain(v, k) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [plain(v, key) for v in obj]
    assert obj is None or type(obj) in (bool, int, float, str), type(obj)
    return obj


def same(a, b, path=""):
    """``a == b`` with the types of the leaves: 1 is not 1.0 and not True."""
    assert type(a) is type(b), "%s: %r is not %r" % (path, type(a), type(b))
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), "%s: keys %r != %r" % (path, sorted(a), sorted(b))
        for k in a:
            same(a[k], b[k], path + "/" + k)
    elif isinstance(a, list):
        assert len(a) == len(b), "%s: %r != %r" % (path, a, b)
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (path, i))
    else:
        assert a == b, "%s: %r != %r" % (path, a, b)


def expected(case, source):
    """The golden of a case with the reference's source index 0 replaced by ``source`` (ours keys the input totals by
    the input path(s) as given)."""
    keys = ("trim", "record_counts", "total_record_count", "bp_counts", "total_bp_counts", "sum_total_bp_count")
    out = {k: case[k] for k in keys}
    for k in ("record_counts", "bp_counts"):
        assert list(out[k]) in ([], ["0"])                      # (a file without a record: the reference saw no batch)
        out[k] = {str(source): v for v in out[k].values()}
    return out


def fill_args(case, tmp_path):
    args = case["args"]
    for kind in KINDS:
        args = args.replace("{%s}" % kind, str(tmp_path / (kind + ".txt")))
    return args


def run_case(case, tmp_path, chunk_bytes=1 << 16):
    """A golden case through ``trim_file`` / ``trim_files`` of the installed backend; asserts the summary."""
    paired = "input1" in case
    names = [case["input1"], case["input2"]] if paired else [case["input"]]
    ins = [str(tmp_path / ("in%d.fastq" % k)) for k in range(len(names))]
    for path, name in zip(ins, names):
        with open(path, "wb") as fh:
            fh.write(input_text(name))
    outs = [str(tmp_path / ("out%d.fastq" % k)) for k in range(len(names))]
    pipe = pipeline_from_args(fill_args(case, tmp_path), paired_input=paired, report=True)
    if paired:
        pipe.trim_files(ins[0], ins[1], outs[0], outs[1], chunk_bytes=chunk_bytes)
    else:
        pipe.trim_file(ins[0], outs[0], chunk_bytes=chunk_bytes)
    source = tuple(ins) if paired else ins[0]
    assert list(pipe.report_summary["record_counts"]) == ([source] if case["total_record_count"] else [])
    same(plain(pipe.report_summary), expected(case, source))
    return pipe


# ---------------------------------------------------------------------------------------------- the host path
def host_summary(argstr, text):
    """What the per-object host path counts for single-end FASTQ ``text``: ``modifiers.AdapterCutter`` over
    ``adapters.Adapter`` (Adapter.trimmed per match, twice with the mask action) for the adapter block, plain Python
    sums for the rest.  Independent of the report kernels; covers adapters, -u, -m and the written totals."""
    from atropos_amd.modifiers import AdapterCutter
    from atropos_amd.reads import Read
    pipe = pipeline_from_args(argstr)
    cutter = AdapterCutter(pipe.adapters, times=pipe.times, action=pipe.action)
    lines = text.decode("latin-1").split("\n")
    records = bases = cut = written = written_bp = too_short = 0
    for i in range(0, len(lines) - 1, 4):
        read = Read(lines[i][1:], lines[i + 1], lines[i + 3])
        records += 1
        bases += len(read)
        if (pipe.cut_front or pipe.cut_back) and len(read) > 0:
            cut += pipe.cut_front - pipe.cut_back
            read = read[pipe.cut_front:len(read) + pipe.cut_back if pipe.cut_back else None]
        read = cutter(read)
        if pipe.minimum_length and len(read) < pipe.minimum_length:
            too_short += 1
            continue
        written += 1
        written_bp += len(read)
    mods = {"AdapterCutter": {"records_with_adapters": (cutter.with_adapters,), "desc": "AdapterCutter",
                              "adapters": ({a.name: a.summarize() for a in pipe.adapters},)}}
    if pipe.cut_front or pipe.cut_back:
        mods["UnconditionalCutter"] = {"bp_trimmed": (cut,), "desc": "Cut unconditionally"}
    filters = {"too_short": {"records_filtered": too_short}} if pipe.minimum_length else {}
    return {"trim": {"modifiers": mods, "filters": filters,
                     "formatters": {"records_written": written, "bp_written": [written_bp, 0]}},
            "record_counts": {0: records}, "total_record_count": records, "bp_counts": {0: [bases, 0]},
            "total_bp_counts": (bases, 0), "sum_total_bp_count": bases}


def device_summary(argstr, text, max_read_len=None, variant="auto", pieces=1):
    """The report of ``pipe.run`` over ``text`` (in ``pieces`` batches of whole records) on the installed backend."""
    pipe = pipeline_from_args(argstr, report=True)
    rep = TrimReport(pipe, max_read_len=max_read_len, variant=variant)
    try:
        lines = text.split(b"\n")
        nrec = (len(lines) - 1) // 4
        step = max(1, -(-nrec // pieces))
        for lo in range(0, max(nrec, 1), step):
            part = b"\n".join(lines[4 * lo:4 * min(nrec, lo + step)])
            batch, _ = FastqBatch.from_bytes(part + b"\n" if part else b"", final=True)
            rep.add(pipe.run(batch))
        return rep.summary()
    finally:
        rep.close()


def fastq_of(seqs):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)).encode()


def synthetic_reads(n, seed, adapter, read_len=60, lower=0.03):
    """Reads of up to ``read_len`` bases that run into ``adapter`` at a random place (whole, cut by the read end, absent,
    right at the start), some with a substitution in it, some lower-case or with N before it."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        k = int(rng.randint(0, read_len + 10))
        body = "".join("ACGT"[v] for v in rng.randint(0, 4, size=k))
        if k and rng.rand() < 0.1:
            body = body[:-1] + "N"
        ad = list(adapter)
        if rng.rand() < 0.3:
            ad[int(rng.randint(0, len(ad)))] = "ACGT"[int(rng.randint(0, 4))]
        seq = (body + "".join(ad) + "".join("ACGT"[v] for v in rng.randint(0, 4, size=read_len)))[:int(rng.randint(1, read_len + 1))]
        if rng.rand() < lower:
            seq = seq.lower()
        out.append(seq)
    return out

"""CPU tier of the trim report (atropos_amd.report): every golden case of tests/golden/trim_report.json.gz -- the
reference's summary['trim'] and input totals -- through the CPU twin of the report kernels (tests/emu/emu_report.cpp,
a harness, not parity evidence for the kernels), the envelope refusals, and the TrimReport interface."""
import pytest

from atropos_amd import _lib
from atropos_amd.trim import pipeline_from_args

from . import _report_common as R
from .emu.backend import EmuBackend

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


@pytest.fixture()
def report_backend():
    prev = _lib.set_backend(EmuBackend(), _test_double=True)
    yield _lib.get_backend()
    _lib.set_backend(prev, _test_double=True)


def test_fixture_conditions():
    g = R.golden()
    assert len(g["cases"]) >= 40 and len(g["paired"]) >= 15


@pytest.mark.parametrize("index", range(len(R.golden()["cases"])), ids=R.case_ids("cases"))
def test_single_end_golden(report_backend, tmp_path, index):
    R.run_case(R.golden()["cases"][index], tmp_path)


@pytest.mark.parametrize("index", range(len(R.golden()["paired"])), ids=R.case_ids("paired"))
def test_paired_golden(report_backend, tmp_path, index):
    R.run_case(R.golden()["paired"][index], tmp_path)


@pytest.mark.parametrize("args,paired", [
    ("-a ^ACGTACGT..." + TRUSEQ, False),                                     # a linked adapter
    ("-a " + TRUSEQ + " --bisulfite rrbs", False),
    ("--aligner insert -a " + TRUSEQ + " -A " + TRUSEQ, True),
    ("-a " + TRUSEQ + " -A " + TRUSEQ + " -R", True),
    ("-a " + TRUSEQ + " -A " + TRUSEQ + " --bisulfite swift", True),
])
def test_envelope_refusals(report_backend, tmp_path, args, paired):
    """Refused when the pipeline is built: no output path exists afterwards."""
    out = tmp_path / "out.fastq"
    with pytest.raises(NotImplementedError, match="^report: "):
        pipe = pipeline_from_args(args, paired_input=paired, report=True)
        pipe.trim_file(str(tmp_path / "in.fastq"), str(out))                # (never reached)
    assert not out.exists()
    pipeline_from_args(args, paired_input=paired)                            # without the report the pipeline stands


def test_reads_beyond_the_table_raise(report_backend):
    """A read longer than the adapter tables hold: the run raises instead of miscounting."""
    text = R.fastq_of(["ACGT" * 20 + TRUSEQ])
    with pytest.raises(_lib.AtroposUnsupported, match="^report: "):
        R.device_summary("-a " + TRUSEQ, text, max_read_len=100)
    with pytest.raises(_lib.AtroposUnsupported, match="^report: "):           # the table bound itself
        R.device_summary("-a " + TRUSEQ, text, max_read_len=1 << 20)


def test_table_bound_refuses_before_any_output(report_backend, tmp_path):
    """More adapters than a counter block holds: refused when the run starts, before an output path exists."""
    src, out = tmp_path / "in.fastq", tmp_path / "out.fastq"
    src.write_bytes(R.input_text("small.fastq"))
    args = " ".join("-a ACGTTGCA%s" % "".join("ACGT"[(k >> s) & 3] for s in (0, 2, 4, 6)) for k in range(65))
    pipe = pipeline_from_args(args + " --too-short-output %s -m 5" % (tmp_path / "short.fastq"), report=True)
    with pytest.raises(_lib.AtroposUnsupported, match="^report: "):
        pipe.trim_file(str(src), str(out))
    assert not out.exists() and not (tmp_path / "short.fastq").exists()
    assert pipe.p1._reporter is None if hasattr(pipe, "p1") else pipe._reporter is None


def test_default_tables_take_every_read_of_the_pipeline(report_backend):
    """The default table length is the pipeline's own read limit while the block's bound allows it, and shrinks with
    the adapter set instead of refusing it."""
    one = R.TrimReport(pipeline_from_args("-a " + TRUSEQ, report=True))
    assert one.mates[0].max_read_len == _lib.MAX_LONG_READ_LEN
    one.close()
    args = " ".join("-a ACGTTGCA%s" % "".join("ACGT"[(k >> s) & 3] for s in (0, 2, 4)) for k in range(64))
    many = R.TrimReport(pipeline_from_args(args, report=True))
    assert 736 < many.mates[0].max_read_len < _lib.MAX_LONG_READ_LEN
    assert many.mates[0].counters.numel() <= _lib.REPORT_MAX_WORDS
    many.close()


def test_value_types(report_backend, tmp_path):
    """The tuples of SingleEndModifiers / PairedEndModifiers.summarize, as tuples (the golden comparison reads them as
    JSON lists)."""
    g = R.golden()
    single = next(c for c in g["cases"] if c["args"] == "-q 10 --trim-n -m 5 -a TTAGACATATCTCCGTCG")
    mods = R.run_case(single, tmp_path).report_summary["trim"]["modifiers"]
    assert type(mods["QualityTrimmer"]["bp_trimmed"]) is tuple and len(mods["QualityTrimmer"]["bp_trimmed"]) == 1
    cutter = mods["AdapterCutter"]
    assert type(cutter["records_with_adapters"]) is tuple and type(cutter["records_with_adapters"][0]) is int
    assert type(cutter["adapters"]) is tuple and len(cutter["adapters"]) == 1 and type(cutter["adapters"][0]) is dict
    (stats,) = cutter["adapters"][0].values()
    assert all(type(k) is int and type(v) is int for k, v in stats["lengths_back"].items())
    assert all(type(k) is int and type(e) is int for k, v in stats["errors_back"].items() for e in v)
    paired = next(c for c in g["paired"] if c["args"] == "-a TTAGACATAT -A CAGTGGAGTA -q 10 --pair-filter both -m 20 --trim-n")
    summary = R.run_case(paired, tmp_path).report_summary
    mods = summary["trim"]["modifiers"]
    for name, key in (("QualityTrimmer", "bp_trimmed"), ("NEndTrimmer", "bp_trimmed"), ("AdapterCutter", "records_with_adapters"),
                      ("AdapterCutter", "adapters")):
        assert type(mods[name][key]) is tuple and len(mods[name][key]) == 2, (name, key)
    assert type(summary["total_bp_counts"]) is tuple and type(summary["trim"]["formatters"]["bp_written"]) is list
    legacy = next(c for c in g["paired"] if c["args"] == "-a TTAGACATAT -m 14")
    mods = R.run_case(legacy, tmp_path).report_summary["trim"]["modifiers"]
    assert type(mods["AdapterCutter"]["adapters"]) is tuple and mods["AdapterCutter"]["adapters"][1] is None
    assert mods["AdapterCutter"]["records_with_adapters"] == (3, None)


def test_report_off_leaves_no_summary(report_backend, tmp_path):
    path = tmp_path / "in.fastq"
    path.write_bytes(R.input_text("small.fastq"))
    pipe = pipeline_from_args("-a TTAGACATATCTCCGTCG -q 10")
    assert pipe.report is False
    pipe.trim_file(str(path), str(tmp_path / "out.fastq"))
    assert not hasattr(pipe, "report_summary") and pipe._reporter is None
    with pytest.raises(ValueError):
        R.TrimReport(pipe)


@pytest.mark.parametrize("args", ["-a " + TRUSEQ + " -q 20 -u 3 --trim-n -m 30",
                                  "-b " + TRUSEQ + " -n 2 --mask-adapter --max-n 2"])
def test_two_half_batches_equal_one(report_backend, args):
    text = R.input_text("synth.fastq")
    whole = R.device_summary(args, text)
    assert whole["total_record_count"] == 1200
    R.same(R.plain(R.device_summary(args, text, pieces=2)), R.plain(whole))
    R.same(R.plain(R.device_summary(args, text, pieces=2, variant="global")), R.plain(whole))


def test_matches_the_host_path(report_backend):
    """The per-object host path (the oracle of the GPU tier's small shapes) agrees with the twin on the fixture's
    synthetic reads -- and through them with the reference."""
    text = R.input_text("synth.fastq")
    for args in ("-a " + TRUSEQ + " -u 3 -u -2 -m 20", "-b " + TRUSEQ + " -n 2 --mask-adapter"):
        R.same(R.plain(R.device_summary(args, text)), R.plain(R.host_summary(args, text)))


def test_close_detaches(report_backend):
    pipe = pipeline_from_args("-a " + TRUSEQ, report=True)
    rep = R.TrimReport(pipe)
    with pytest.raises(ValueError):
        R.TrimReport(pipe)                                                     # one report at a time
    assert pipe._reporter is not None
    rep.close()
    assert pipe._reporter is None
    R.TrimReport(pipe).close()

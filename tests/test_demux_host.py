"""CPU tier of demultiplexing (``{name}`` in the output path of ``TrimPipeline.trim_file``): every golden case of
tests/golden/trim_demux.json.gz -- the files the reference leaves -- through the CPU twin of the grouped formatter
(tests/emu/emu_demux.cpp, a harness, not parity evidence for the kernels), the refusals, and chunking."""
import pytest

from atropos_amd import _lib
from atropos_amd.fastq import FastqBatch
from atropos_amd.trim import TrimPipeline, pipeline_from_args

from . import _demux_common as D
from .emu.backend import EmuBackend

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
SHORT = "ACGTTGCAAC"


@pytest.fixture()
def demux_backend():
    prev = _lib.set_backend(EmuBackend(), _test_double=True)
    yield _lib.get_backend()
    _lib.set_backend(prev, _test_double=True)


def test_fixture_conditions():
    cases = D.golden()
    assert len(cases) >= 15
    assert {c["input"] for c in cases} == {"synth.fastq", "small.fastq"}
    assert any(len(c["files"]) >= 12 for c in cases)


@pytest.mark.parametrize("index", range(len(D.golden())), ids=D.case_ids())
def test_golden(demux_backend, tmp_path, index):
    case = D.golden()[index]
    got, pipe = D.check_case(case, tmp_path)
    # the records per name, and the counts trim_file returns keep their keys
    for name, count in pipe.demux_counts.items():
        assert count > 0
    mux = sum(text.count(b"\n") // 4 for name, text in got.items() if name.startswith("out.") or name == "untrimmed.txt")
    assert sum(pipe.demux_counts.values()) == mux
    assert pipe.demultiplex is False                                       # (switched on for that call only)


@pytest.mark.parametrize("index", [0, 2, 9, 14])
def test_chunked_equals_unchunked(demux_backend, tmp_path, index):
    """64 KiB chunks: every file is appended to chunk after chunk, in input order."""
    D.check_case(D.golden()[index], tmp_path, chunk_bytes=1 << 16)


def _no_output(tmp_path):
    return sorted(p.name for p in tmp_path.iterdir()) == ["in.fastq"]


def _input(tmp_path):
    src = tmp_path / "in.fastq"
    src.write_bytes(D.input_text(D.golden()[5]))
    return str(src)


def test_discard_trimmed_is_refused(demux_backend, tmp_path):
    src = _input(tmp_path)
    pipe = pipeline_from_args("-a first=%s --discard-trimmed" % SHORT)
    with pytest.raises(ValueError, match="Do not use --discard-trimmed when demultiplexing."):
        pipe.trim_file(src, str(tmp_path / "out.{name}.fastq"))
    assert _no_output(tmp_path)


def test_paired_is_refused(demux_backend, tmp_path):
    src = _input(tmp_path)
    for args in ("-a %s -A %s" % (SHORT, TRUSEQ), "-a %s" % SHORT):         # both mode, legacy mode
        pipe = pipeline_from_args(args, paired_input=True)
        for outs in ((str(tmp_path / "o.{name}.1.fastq"), str(tmp_path / "o.2.fastq")),
                     (str(tmp_path / "o.1.fastq"), str(tmp_path / "o.{name}.2.fastq"))):
            with pytest.raises(ValueError, match="Demultiplexing not supported for paired-end files"):
                pipe.trim_files(src, src, outs[0], outs[1])
    assert _no_output(tmp_path)


def test_part_files_are_refused(demux_backend, tmp_path):
    src = _input(tmp_path)
    with pytest.raises(ValueError, match="part files"):
        pipeline_from_args("-a first=%s" % SHORT).trim_file(src, str(tmp_path / "out.{name}.fastq"), output_parts=2)
    assert _no_output(tmp_path)


def test_linked_adapters_are_refused(demux_backend, tmp_path):
    src = _input(tmp_path)
    with pytest.raises(NotImplementedError, match="linked"):
        pipeline_from_args("-a ^ACGTACGT..." + TRUSEQ).trim_file(src, str(tmp_path / "out.{name}.fastq"))
    assert _no_output(tmp_path)


def test_report_is_refused(demux_backend, tmp_path):
    src = _input(tmp_path)
    with pytest.raises(NotImplementedError, match="report"):
        pipeline_from_args("-a first=%s" % SHORT, report=True).trim_file(src, str(tmp_path / "out.{name}.fastq"))
    assert _no_output(tmp_path)


def test_group_bound_is_refused(demux_backend, tmp_path):
    """More outputs than the grouped formatter takes: 1024 adapter names and "unknown"."""
    src = _input(tmp_path)
    base = pipeline_from_args("-a first=%s" % SHORT)
    import copy
    ads = []
    for k in range(_lib.EMIT_MAX_GROUPS):
        ad = copy.copy(base.adapters[0])
        ad.name = "n%d" % k
        ads.append(ad)
    pipe = TrimPipeline(adapters=ads)
    with pytest.raises(_lib.AtroposUnsupported, match="demultiplexing"):
        pipe.trim_file(src, str(tmp_path / "out.{name}.fastq"))
    assert _no_output(tmp_path)
    TrimPipeline(adapters=ads, discard_untrimmed=True)._check_demux()       # 1024 outputs: inside the bound
    with pytest.raises(_lib.AtroposUnsupported):
        TrimPipeline(adapters=ads, demultiplex=True)


def test_result_group_and_demux_text(demux_backend):
    """``TrimPipeline(demultiplex=True).run``: the group codes and the text per name of one batch."""
    case = D.golden()[1]                                                   # three named adapters
    pipe = pipeline_from_args(case["args"])
    pipe.demultiplex = True
    batch, _ = FastqBatch.from_bytes(D.input_text(case), final=True)
    res = pipe.run(batch)
    assert res.group_names == ["first", "second", "third", "unknown"]
    assert res.group.dtype.is_floating_point is False and res.group.shape[0] == len(batch)
    assert int(res.group.min()) >= 0 and int(res.group.max()) == 3          # nothing filtered: every read has an output
    texts = res.demux_text()
    assert {"out.%s.fastq" % k: v for k, v in texts.items()} == D.expected_files(case)
    plain = pipeline_from_args(case["args"]).run(batch)
    assert plain.group is None
    with pytest.raises(ValueError):
        plain.demux_text()


def test_same_name_shares_a_file(demux_backend, tmp_path):
    """Two adapters with one name (the reference keys its formatters by name): one output, input order kept."""
    case = D.golden()[0]
    src = tmp_path / "in.fastq"
    src.write_bytes(D.input_text(case))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    pipeline_from_args("-a x=%s -a x=%s" % (SHORT, TRUSEQ)).trim_file(str(src), str(tmp_path / "a" / "o.{name}.fastq"))
    exp = D.expected_files(case)
    merged = (tmp_path / "a" / "o.x.fastq").read_bytes()
    assert merged.count(b"\n") == exp["out.first.fastq"].count(b"\n") + exp["out.second.fastq"].count(b"\n")
    assert (tmp_path / "a" / "o.unknown.fastq").read_bytes() == exp["out.unknown.fastq"]
    # in input order: the same bytes as the kept and matched reads of an ordinary run with --discard-untrimmed
    pipeline_from_args("-a x=%s -a x=%s --discard-untrimmed" % (SHORT, TRUSEQ)).trim_file(str(src), str(tmp_path / "b" / "o.fastq"))
    assert merged == (tmp_path / "b" / "o.fastq").read_bytes()


def test_path_without_name_is_unchanged(demux_backend, tmp_path):
    """No ``{name}``: one output file, and nothing of the demultiplexing state appears."""
    case = D.golden()[0]
    src = tmp_path / "in.fastq"
    src.write_bytes(D.input_text(case))
    pipe = pipeline_from_args(case["args"])
    pipe.trim_file(str(src), str(tmp_path / "out.fastq"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.fastq", "out.fastq"]
    assert not hasattr(pipe, "demux_counts")
    exp = D.expected_files(case)
    assert (tmp_path / "out.fastq").read_bytes().count(b"\n") == sum(v.count(b"\n") for v in exp.values())

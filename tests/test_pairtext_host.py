"""Interleaved FASTQ in and out on the CPU twins: the pair formatter ``atr_fastq_emit_pairs`` against the plain model,
the interleaved chunk loop, and ``pipeline_from_args`` + ``trim_files`` / ``text_interleaved`` against the files the
reference writes (tests/golden/pairtext.json.gz)."""
import os

import pytest

from atropos_amd import _lib
from tests import _pairtext_common as P
from tests.conftest import load_golden


@pytest.fixture()
def pair_backend():
    """The CPU emulation with the paired-text entry points served by their own twin library."""
    prev = _lib.set_backend(P.PairTextEmuBackend(), _test_double=True)
    yield _lib.get_backend()
    _lib.set_backend(prev, _test_double=True)


@pytest.fixture(scope="module")
def doc():
    return load_golden("pairtext.json.gz")


# ---------------------------------------------------------------------------------------------- the formatter
def test_pair_formatter_layouts(pair_backend):
    rep, calls = P.check_pairs_layouts(pair_backend)
    assert calls >= 9 + 18 + 6 + 3
    assert rep["interleaved"]["one"] and rep["halves"]["two"] and rep["two"]["two"]      # (what the GPU kernel would do)
    assert all(r["overflow"] for k, r in rep.items())                                    # the 2 900-base reads


def test_pair_formatter_tiles(pair_backend):
    for hint, rep in P.check_pairs_tiles(pair_backend).items():
        assert rep["edge_calls"] == 6 and rep["empty_tile"] >= 1
        assert rep["permuted_unordered"] > 10 and rep["renamed_unordered"] > 5 and rep["renamed_staged"] > 5


def test_pair_formatter_stage_limit(pair_backend):
    for hint, rep in P.check_pairs_stage_limit(pair_backend).items():
        assert (rep["one"], rep["overflow"]) == (1, 1), (hint, rep)


def test_pair_formatter_refuses_half_a_mask(pair_backend):
    import torch
    t = torch.zeros((16,), dtype=torch.int32)
    ptr = _lib._ptr
    with pytest.raises(ValueError):
        pair_backend._call("atr_fastq_emit_pairs", ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), None, ptr(t), ptr(t), ptr(t), ptr(t),
                           None, None, None, 0, 1, 0, ptr(t), ptr(t), None)


# ---------------------------------------------------------------------------------------------- the chunk loop
def test_interleaved_chunks_carry_the_odd_record(pair_backend, doc, tmp_path):
    from atropos_amd.fastq import read_chunks
    paths = P.write_inputs(doc, tmp_path)
    text = P.fixture_files(doc)["il"]
    size = P.odd_first_chunk(text)
    chunks = list(read_chunks([paths["il"]], size, interleaved=True))
    assert len(chunks) >= 3 and all(len(c) == 2 and len(c[0]) == len(c[1]) for c in chunks)
    assert all(c[0].data is c[1].data and c[0].stride == 2 for c in chunks)
    got = []
    for b1, b2 in chunks:
        for r1, r2 in zip(b1.to_records(), b2.to_records()):
            got += [r1, r2]
    from atropos_amd.fastq import FastqBatch
    assert got == FastqBatch.from_bytes(text)[0].to_records() and len(got) == 440
    assert all(r[0].split()[0].endswith("/1") for r in got[0::2]) and all(r[0].split()[0].endswith("/2") for r in got[1::2])


def test_interleaved_head_counts_pairs(pair_backend, doc):
    from atropos_amd.fastq import FastqBatch
    text = P.fixture_files(doc)["il"]
    b1, b2 = FastqBatch.from_bytes(text)[0].mates()
    lines = text.splitlines(True)
    for mate in (b1, b2):
        for pairs in (0, 1, 7, 220):
            head, consumed = mate.head(pairs)
            assert len(head) == pairs and consumed == len(b"".join(lines[:8 * pairs]))


def test_interleaved_refusals(pair_backend, doc, tmp_path):
    from atropos_amd.fastq import FormatError, read_chunks
    paths = P.write_inputs(doc, tmp_path)
    with pytest.raises(ValueError):
        next(read_chunks([paths["il"]], 1 << 20, byte_ranges=[(0, 100)], interleaved=True))
    with pytest.raises(ValueError):
        next(read_chunks([paths["r1"], paths["r2"]], 1 << 20, interleaved=True))
    with pytest.raises(FormatError, match="Interleaved input file incomplete: Last record has no partner."):
        list(read_chunks([paths["odd"]], 1 << 20, interleaved=True))


# ---------------------------------------------------------------------------------------------- the drivers
def test_detect_of_an_interleaved_file(pair_backend, doc, tmp_path):
    assert P.check_detect_interleaved(doc, tmp_path) == 2


def test_qc_and_error_rate_of_an_interleaved_file(pair_backend, doc, tmp_path):
    """On the statistics twin (tests/emu/emu_stats.cpp); the GPU test compares what this twin counts with the kernels."""
    qc, err = P.check_stats_interleaved(doc, tmp_path)
    assert qc["pre"][0]["read1"] != qc["pre"][0]["read2"]


def test_statistics_twin_argument_checks(pair_backend):
    """The twin refuses what atr_read_stats_* refuse (tests/test_stats_host.py calls the library's own checks)."""
    import torch
    from atropos_amd import _lib
    assert pair_backend._symbol_of("atr_read_stats_bytes")(0) == -1
    assert pair_backend._symbol_of("atr_read_stats_bytes")(_lib.MAX_LONG_READ_LEN + 1) == -2
    assert pair_backend.read_stats_words(150) * 8 == pair_backend._symbol_of("atr_read_stats_bytes")(150)
    block = torch.zeros((pair_backend.read_stats_words(150),), dtype=torch.int64)
    with pytest.raises(ValueError):
        pair_backend.read_stats_merge(block, 100, block, 150)


# ---------------------------------------------------------------------------------------------- the overwrite stage
def test_overwrite_plan_and_apply(pair_backend):
    total = P.check_overwrite_matrix(pair_backend)
    assert total[0] > 30 and total[1] > 30


def test_overwrite_refusals(pair_backend, tmp_path):
    from atropos_amd.trim import PairedTrimPipeline, pipeline_from_args
    both = ["-a", P.AD1, "-A", P.AD2]
    pipe = pipeline_from_args(both + ["-w", "10,20,20"], paired_input=True)
    assert isinstance(pipe, PairedTrimPipeline) and pipe.overwrite_low_quality == (10, 20, 20) and pipe.overwritten == [0, 0]
    pipe = pipeline_from_args(["-a", P.AD1, "-w", "10,20,20"], paired_input=True)        # -w: never the legacy mode
    assert type(pipe) is PairedTrimPipeline
    assert type(pipeline_from_args(["-w", "10,20,20"], paired_input=True)) is PairedTrimPipeline    # ... and enough to run
    with pytest.raises(ValueError, match="--overwrite-low-quality is not valid for single-end reads"):
        pipeline_from_args(["-a", P.AD1, "-w", "10,20,20"])
    with pytest.raises(ValueError, match="For --overwrite-low-quality, LOWQ must be <= HIGHQ"):
        pipeline_from_args(both + ["-w", "21,20,20"], paired_input=True)
    with pytest.raises(ValueError, match="LOWQ must be <= HIGHQ"):
        PairedTrimPipeline(overwrite_low_quality=(21, 20, 20))
    with pytest.raises(ValueError):
        PairedTrimPipeline(overwrite_low_quality=(10, 20, 0))
    for extra in (["--info-file", str(tmp_path / "i")], ["--cut-min", "5"], ["--cut-min2", "5"], ["--bisulfite", "rrbs"],
                  ["-R"], ["-a", "AAAA...CCCC"]):
        with pytest.raises(NotImplementedError):
            pipeline_from_args(both + ["-w", "10,20,20"] + extra, paired_input=True)
    with pytest.raises(NotImplementedError):
        pipeline_from_args(both + ["-w", "10,20,20"], paired_input=True, report=True)
    with pytest.raises(NotImplementedError):
        PairedTrimPipeline(overwrite_low_quality=(10, 20, 20), stats=("post",))
    assert os.listdir(str(tmp_path)) == []


def test_overwritten_counts(pair_backend, doc):
    from atropos_amd.fastq import FastqBatch
    from atropos_amd.trim import pipeline_from_args
    blobs = P.fixture_files(doc)
    pipe = pipeline_from_args(["-a", P.AD1, "-A", P.AD2, "-w", "10,20,20"], paired_input=True)
    pipe.run(FastqBatch.from_bytes(blobs["r1"])[0], FastqBatch.from_bytes(blobs["r2"])[0])
    assert pipe.overwritten[0] >= 5 and pipe.overwritten[1] >= 5
    again = pipeline_from_args(["-a", P.AD1, "-A", P.AD2, "-w", "10,20,20", "-l", "x"])
    again.run(*FastqBatch.from_bytes(blobs["il"])[0].mates())                          # (one chunk for both reads)
    assert again.overwritten == pipe.overwritten


def test_overwrite_read_object_path(doc):
    """``modifiers.OverwriteRead`` and ``Read.reverse_complement`` (host classes, no backend) against the reference's
    modifier called on the same pairs: names, bases, qualities, name2 and ``corrected`` of both reads."""
    from atropos_amd.modifiers import OverwriteRead
    from atropos_amd.reads import Read
    show = lambda r: [r.name, r.sequence, r.qualities, r.name2, int(r.corrected)]
    seen = dict(none=0, first=0, second=0, error=0)
    for case in doc["overwrite_read"]:
        lowq, highq, window, base = case["args"]
        reads = [Read(name, seq, qual, name2) for name, seq, qual, name2, _ in case["before"]]
        assert [show(r) for r in reads] == case["before"]
        if case["error"]:
            with pytest.raises(KeyError):
                OverwriteRead(lowq, highq, window, base=base)(*reads)
            seen["error"] += 1
            continue
        got = OverwriteRead(lowq, highq, window, base=base)(*reads)
        assert [show(r) for r in got] == case["after"], case["args"]
        changed = [a[0] != b[0] for a, b in zip(case["after"], case["before"])]
        seen["first" if changed[0] else ("second" if changed[1] else "none")] += 1
    assert seen["first"] >= 5 and seen["second"] >= 5 and seen["none"] >= 20 and seen["error"] >= 1
    read = Read("r", "ACGTNacgtRY", "ABCDEFGHIJK", "r", clipped=[1, 2, 3, 4], corrected=1, insert_overlap=True)
    back = read.reverse_complement()
    assert (back.sequence, back.qualities, back.name2, back.clipped, back.corrected, back.insert_overlap) == (
        "RYacgtNACGT", "KJIHGFEDCBA", "r", [1, 2, 3, 4], 1, True) and back.clipped is not read.clipped
    assert back.reverse_complement() == read


def test_fixture_cases_file_to_file(pair_backend, doc, tmp_path):
    """Every case of the fixture, cut into at least three chunks (an odd first chunk) and as one chunk."""
    from atropos_amd.fastq import FormatError
    paths = P.write_inputs(doc, tmp_path)
    size = P.odd_first_chunk(P.fixture_files(doc)["il"])
    ran = 0
    for k, case in enumerate(doc["cases"]):
        for chunk_bytes in (size, 1 << 22):
            if case["error"] is not None:
                with pytest.raises(FormatError) as err:
                    P.run_case_files(case, paths, tmp_path, "%d.%d" % (k, chunk_bytes), chunk_bytes)
                assert str(err.value) == case["error"]
                continue
            got = P.run_case_files(case, paths, tmp_path, "%d.%d" % (k, chunk_bytes), chunk_bytes)
            assert got == P.want_files(case), (case["args"], case["input"], case["output"], chunk_bytes)
            ran += 1
    assert ran >= 2 * 19


def test_fixture_cases_one_batch(pair_backend, doc):
    for case in doc["cases"]:
        if case["error"] is None:
            assert P.run_case_bytes(case, doc) == P.want_files(case), (case["args"], case["input"], case["output"])


def test_interleaved_output_options(pair_backend, doc, tmp_path):
    """-L through the device gzip sink and into part files: they act on the one sink."""
    import gzip
    from atropos_amd.trim import pipeline_from_args
    paths = P.write_inputs(doc, tmp_path)
    case = next(c for c in doc["cases"] if c["input"] == "il" and c["output"] == "il" and "--trim-n" in c["args"])
    want = P.want_files(case)["out.il.fastq"]
    size = P.odd_first_chunk(P.fixture_files(doc)["il"])
    pipe = pipeline_from_args(case["args"].split() + ["-l", paths["il"]])
    out = os.path.join(str(tmp_path), "out.fastq.gz")
    pipe.trim_files(paths["il"], None, out, chunk_bytes=size, device_gzip=True)
    assert gzip.open(out, "rb").read() == want
    out = os.path.join(str(tmp_path), "parts.fastq")
    pipe.trim_files(paths["il"], None, out, chunk_bytes=size, output_parts=2)
    parts = [open("%s.part%d" % (out, i), "rb").read() for i in range(2)]
    assert sorted(b"".join(parts).split(b"@pair")) == sorted(want.split(b"@pair")) and all(parts)


def test_pipeline_from_args_interleaved(pair_backend, tmp_path):
    from atropos_amd.trim import LegacyPairedPipeline, PairedTrimPipeline, pipeline_from_args
    P_AD1, P_AD2 = P.AD1, P.AD2
    pipe = pipeline_from_args(["-a", P_AD1, "-l", "in.fastq"])                  # -l: paired input, never the legacy mode
    assert isinstance(pipe, PairedTrimPipeline) and not isinstance(pipe, LegacyPairedPipeline)
    assert (pipe.interleaved_input, pipe.interleaved_output) == ("in.fastq", None)
    pipe = pipeline_from_args(["-a", P_AD1, "-L", "out.fastq"], paired_input=True)
    assert isinstance(pipe, LegacyPairedPipeline) and pipe.interleaved_output == "out.fastq"
    with pytest.raises(ValueError):
        pipeline_from_args(["-a", P_AD1, "-L", "out.fastq"])                     # single-end input
    # side outputs with an interleaved output: refused before any file is opened
    side = ["--too-short-output", str(tmp_path / "s1"), "--too-short-paired-output", str(tmp_path / "s2"), "-m", "30"]
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", P_AD1, "-A", P_AD2, "-L", str(tmp_path / "o")] + side)
    pipe = pipeline_from_args(["-a", P_AD1, "-A", P_AD2] + side)
    with pytest.raises(NotImplementedError):
        pipe.trim_files(str(tmp_path / "missing.1"), str(tmp_path / "missing.2"), str(tmp_path / "o"))
    assert os.listdir(str(tmp_path)) == []

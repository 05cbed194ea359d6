"""FASTA in and out on the CPU twin (tests/emu/emu_fasta.cpp over fasta_core.hpp): the index and the formatter at the
C ABI against the plain model of ``_fasta_common``, the chunk loop, and ``pipeline_from_args`` + ``trim_file`` /
``trim_files`` against the files the reference writes (tests/golden/fasta.json.gz)."""
import os
import subprocess

import pytest

from atropos_amd import _lib, fastq
from atropos_amd.trim import pipeline_from_args
from tests import _fasta_common as F

AD = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"
DOC = F.load_doc()


@pytest.fixture()
def fasta_backend():
    """The CPU emulation with the FASTA entry points served by their own twin library."""
    prev = _lib.set_backend(F.FastaEmuBackend(), _test_double=True)
    yield _lib.get_backend()
    _lib.set_backend(prev, _test_double=True)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return F.write_inputs(DOC, tmp_path_factory.mktemp("fasta_inputs"))


# ---------------------------------------------------------------------------------------------- index and formatter
@pytest.mark.parametrize("label", sorted(F.index_texts(DOC)))
def test_index_against_the_model(fasta_backend, label):
    text = F.index_texts(DOC)[label]
    n, tail = F.check_index(fasta_backend, text)
    assert (n > 0) == (b">" in text)
    if label in ("wrap", "messy", "long", "n4097", "w1"):
        assert tail > 0                                                  # the gather path
    if label == "two":
        assert tail == 0                                                 # every record in place
    if label == "long":
        assert tail > 70000


def test_index_is_the_same_twice(fasta_backend):
    text = F.index_texts(DOC)["messy"]
    a, b = F.run_index(fasta_backend, text), F.run_index(fasta_backend, text)
    assert a[1:] == b[1:]


def test_cut_at_every_byte(fasta_backend):
    text = F.fixture_inputs(DOC)["wrap"]
    at = text.index(b">read002")                                          # read002, read003, read004: wrapped at 70, 1000, 7
    window = text[at:text.index(b">read006")]
    assert F.check_cut_everywhere(fasta_backend, window, 0, len(window)) == len(window) + 1
    messy = F.fixture_inputs(DOC)["messy"]
    F.check_cut_everywhere(fasta_backend, messy, 0, 300)                 # CR, CRLF, blank and '#' lines at the cut


def test_head(fasta_backend):
    assert F.check_head(fasta_backend, F.fixture_inputs(DOC)["messy"]) == 200
    batch, _ = fastq.FastaBatch.from_bytes(b">a\nAC\n>b\nGT\n", backend=fasta_backend)
    with pytest.raises(NotImplementedError):
        batch.mates()


def test_error_word(fasta_backend):
    bad = F.fixture_inputs(DOC)["bad"]
    with pytest.raises(fastq.FormatError) as info:
        fastq.FastaBatch.from_bytes(bad, backend=fasta_backend)
    assert str(info.value) == "At line 3: Expected '>' at beginning of FASTA record, but got 'ACGTACGT'."
    data = F.K.upload_text(fasta_backend, bad)
    assert fasta_backend.fasta_index(data, len(bad))[-1] == 3 * 8 + _lib.FASTA_ERR_HEADER
    long_line = b"  " + b"ACGT" * 40 + b"\r\n>r\nAC\n"
    with pytest.raises(fastq.FormatError) as info:
        fastq.FastaBatch.from_bytes(long_line, final=False, backend=fasta_backend)
    shown = ("ACGT" * 40)[:97] + "..."                                    # (util.truncate_string: at most 100 characters)
    assert str(info.value) == "At line 1: Expected '>' at beginning of FASTA record, but got %r." % shown
    assert F.model_index(bad)["error"] == (3, b"ACGTACGT")


def test_emit_against_the_model(fasta_backend):
    assert F.check_emit(fasta_backend, F.fixture_inputs(DOC)["messy"]) == 36
    assert F.check_emit(fasta_backend, F.generated(257, 16, 9)) == 36
    assert F.check_emit(fasta_backend, b"") == 36


def test_emit_from_a_fastq_batch(fasta_backend):
    assert F.check_emit(fasta_backend, None, fastq_text=F.fixture_inputs(DOC)["fq"]) == 36


# ---------------------------------------------------------------------------------------------- the file drivers
@pytest.mark.parametrize("k", range(len(DOC["cases"])))
def test_golden_case(fasta_backend, paths, tmp_path, k):
    case = DOC["cases"][k]
    F.check_case(case, paths, tmp_path / "whole")
    F.check_case(case, paths, tmp_path / "chunked", chunk_bytes=4096)     # records straddle the chunks' ends


def test_small_chunks_are_many(fasta_backend, paths):
    for key in ("two", "wrap", "messy", "r2w"):
        assert F.count_chunks(paths[key], 4096, fasta_backend) >= 5
    total = sum(len(b) for (b,) in fastq.read_chunks([paths["messy"]], 4096, fasta_backend))
    assert total == 200


def test_fixture_is_not_hollow():
    cases = DOC["cases"]
    assert len(cases) >= 30 + 4 and sum(1 for c in cases if c["error"]) == 2
    assert sum(1 for c in cases if len(c["input"]) == 2) >= 8 and sum(1 for c in cases if "out.info" in c["files"]) >= 6
    assert any(c["input"] == ["fq"] for c in cases)


# (options, the option the message names)
REFUSED = [("-q 20", "-q"), ("--nextseq-trim 20", "--nextseq-trim"), ("-A %s -w 10,20,20" % AD, "-w"),
           ("-A %s --aligner insert --correct-mismatches liberal" % AD, "--correct-mismatches"), ("-A %s -R" % AD, "-R")]


@pytest.mark.parametrize("extra,named", REFUSED)
def test_refused_for_fasta_before_any_output(fasta_backend, paths, tmp_path, extra, named):
    pipe = pipeline_from_args(("-a %s " % AD + extra).split(), paired_input="-A" in extra)
    out = [str(tmp_path / "out.1.fasta"), str(tmp_path / "out.2.fasta")]
    with pytest.raises(ValueError) as info:
        if "-A" in extra:
            pipe.trim_files(paths["r1"], paths["r2"], out[0], out[1])
        else:
            pipe.trim_file(paths["two"], out[0])
    assert str(info.value).startswith(named + " ") and "FASTA" in str(info.value) and os.listdir(str(tmp_path)) == []
    with pytest.raises(ValueError):
        if "-A" in extra:
            pipe.trim_bytes(F.fixture_inputs(DOC)["r1"], F.fixture_inputs(DOC)["r2"])
        else:
            pipe.trim_bytes(F.fixture_inputs(DOC)["two"])


def test_stats_and_statistics_drivers_refuse_fasta(fasta_backend, paths, tmp_path):
    from atropos_amd import stats
    from atropos_amd.trim import TrimPipeline
    from atropos_amd.adapters import AdapterParser
    pipe = TrimPipeline(adapters=AdapterParser().parse_multi([AD], [], []), stats=("pre",))
    with pytest.raises(ValueError, match="--stats"):
        pipe.trim_file(paths["two"], str(tmp_path / "out.fasta"))
    for call in (lambda: stats.qc_file(paths["two"]), lambda: stats.qc_files(paths["r1"], paths["r2"]),
                 lambda: stats.error_rate_file(paths["two"])):
        with pytest.raises(ValueError, match="FASTA"):
            call()
    assert os.listdir(str(tmp_path)) == []


def test_out_of_scope_for_fasta(fasta_backend, paths, tmp_path):
    out = str(tmp_path / "out.fasta")
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", AD], report=True).trim_file(paths["two"], out)
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", "one=" + AD]).trim_file(paths["two"], str(tmp_path / "out.{name}.fasta"))
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", AD, "-A", AD]).trim_files(paths["r1"], None, out, str(tmp_path / "out.2.fasta"))   # -l
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", AD, "-A", AD]).trim_files(paths["r1"], paths["r2"], out)                          # -L
    with pytest.raises(NotImplementedError):
        next(fastq.read_chunks([paths["two"]], 1 << 20, fasta_backend, byte_ranges=[(0, 100)]))
    with pytest.raises(NotImplementedError):
        next(fastq.read_chunks([paths["two"]], 1 << 20, fasta_backend, interleaved=True))
    # FASTQ reads into FASTA-named files of the formatters that only write FASTQ
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", "one=" + AD]).trim_file(paths["fq"], str(tmp_path / "out.{name}.fasta"))
    with pytest.raises(NotImplementedError):
        pipeline_from_args(["-a", AD, "-A", AD]).trim_files(paths["fq"], paths["fq"], out)
    assert os.listdir(str(tmp_path)) == []


def test_fastq_named_output_of_fasta_input(fasta_backend, paths, tmp_path):
    for name, kwargs in (("out.fastq", {}), ("out.fq.gz", {}), ("reads_sequence.txt", {})):
        with pytest.raises(ValueError, match="Output format cannot be FASTQ since no quality values are available."):
            pipeline_from_args(["-a", AD]).trim_file(paths["two"], str(tmp_path / name), **kwargs)
    with pytest.raises(ValueError, match="Output format cannot be FASTQ"):
        pipeline_from_args(["-a", AD, "-m", "30", "--too-short-output", str(tmp_path / "short.fastq")]).trim_file(
            paths["two"], str(tmp_path / "out.fasta"))
    assert os.listdir(str(tmp_path)) == []


def test_guess_format():
    table = {"a.fasta": "fasta", "a.fa": "fasta", "a.fna": "fasta", "a.FA": "fasta", "a.fa.gz": "fasta", "a.fasta.bz2": "fasta",
             "a.fna.xz": "fasta", "a.fastq": "fastq", "a.fq": "fastq", "a.fq.gz": "fastq", "s_1_sequence.txt": "fastq",
             "s_1_sequence.txt.gz": "fastq", "a.txt": None, "a": None, "a.gz": None, "a.fasta.part0": None, "dir.fa/reads": None}
    assert {name: fastq.guess_format(name) for name in table} == table
    for name in ("a.csfasta", "a.csfa", "a.sam", "a.bam", "a.bam.gz"):
        with pytest.raises(NotImplementedError):
            fastq.guess_format(name)


def test_input_format_by_keyword_name_and_first_byte(fasta_backend, tmp_path):
    two = F.fixture_inputs(DOC)["two"]
    want = next(c for c in DOC["cases"] if c["args"] == "-a " + AD and c["input"] == ["two"])
    want = F.base64.b64decode(want["files"]["out.fasta"])
    plain = tmp_path / "reads.txt"
    plain.write_bytes(b"\n# comment\n" + two)
    assert fastq.input_format(str(plain)) == "fasta" and fastq.input_format(str(plain), "fastq") == "fastq"
    out = tmp_path / "trimmed"                                            # a name that says nothing: what the input is
    pipeline_from_args(["-a", AD]).trim_file(str(plain), str(out))
    assert out.read_bytes() == want
    # the reader alone decides by the first chunk
    assert sum(len(b) for (b,) in fastq.read_chunks([str(plain)], 4096, fasta_backend)) == 200
    named = tmp_path / "reads.fastq"                                      # the keyword wins over the name
    named.write_bytes(two)
    pipeline_from_args(["-a", AD]).trim_file(str(named), str(out), input_format="fasta")
    assert out.read_bytes() == want
    with pytest.raises(fastq.FormatError, match="expected to start with '@'"):
        pipeline_from_args(["-a", AD]).trim_file(str(named), str(tmp_path / "o.fastq"))
    fq = tmp_path / "reads"
    fq.write_bytes(F.fixture_inputs(DOC)["fq"])
    assert fastq.input_format(str(fq)) == "fastq"
    with pytest.raises(ValueError):
        fastq.input_format(str(fq), "sam")


def test_mixed_formats_raise(fasta_backend, paths, tmp_path):
    pipe = pipeline_from_args(["-a", AD, "-A", AD])
    with pytest.raises(ValueError, match="different formats"):
        pipe.trim_files(paths["r1"], paths["fq"], str(tmp_path / "o1.fasta"), str(tmp_path / "o2.fasta"))
    with pytest.raises(ValueError, match="different formats"):
        next(fastq.read_chunks([paths["r1"], paths["fq"]], 1 << 20, fasta_backend))
    assert os.listdir(str(tmp_path)) == []


def test_trim_bytes_and_text_formats(fasta_backend):
    inputs = F.fixture_inputs(DOC)
    want = next(c for c in DOC["cases"] if c["args"] == "-a " + AD and c["input"] == ["two"])
    pipe = pipeline_from_args(["-a", AD])
    assert pipe.trim_bytes(inputs["messy"]) == F.base64.b64decode(want["files"]["out.fasta"])
    assert pipe.trim_bytes(inputs["fq"], fmt="fasta") == F.base64.b64decode(want["files"]["out.fasta"])
    assert pipe.trim_bytes(inputs["fq"]).startswith(b"@read000\n")
    with pytest.raises(ValueError, match="Output format cannot be FASTQ"):
        pipe.trim_bytes(inputs["two"], fmt="fastq")
    batch, _ = fastq.FastaBatch.from_bytes(inputs["two"], backend=fasta_backend)
    assert pipe.run(batch).fmt == "fasta"


def test_part_files_and_compressed_files(fasta_backend, paths, tmp_path):
    import gzip
    want = next(c for c in DOC["cases"] if c["args"] == "-a " + AD and c["input"] == ["two"])
    want = F.base64.b64decode(want["files"]["out.fasta"])
    pipe = pipeline_from_args(["-a", AD])
    pipe.trim_file(paths["wrap"], str(tmp_path / "out.fa"), chunk_bytes=4096, output_parts=2)
    parts = [(tmp_path / ("out.fa.part%d" % k)).read_bytes() for k in (0, 1)]
    assert all(parts) and sorted(b"".join(parts).split(b">")) == sorted(want.split(b">"))
    gz_in = tmp_path / "in.fasta.gz"
    gz_in.write_bytes(gzip.compress(F.fixture_inputs(DOC)["messy"]))
    pipe.trim_file(str(gz_in), str(tmp_path / "out.fasta.gz"), chunk_bytes=4096)
    assert gzip.decompress((tmp_path / "out.fasta.gz").read_bytes()) == want


# ---------------------------------------------------------------------------------------------- the stand-alone driver
def test_fuzz_driver_under_the_sanitizers(tmp_path):
    """tests/emu/fasta_fuzz_main.cpp: the twin over random line soups, as a program of its own with
    -fsanitize=address,undefined (nothing of it is loaded into Python)."""
    from tests.emu import backend as emu
    exe = str(tmp_path / "fasta_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DATR_HOST_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + emu._INC + [os.path.join(emu._HERE, "fasta_fuzz_main.cpp"),
                                                                      os.path.join(emu._HERE, "emu_fasta.cpp"), "-o", exe])
    out = subprocess.run([exe, "300", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    assert b"ok: 300 soups" in out.stdout

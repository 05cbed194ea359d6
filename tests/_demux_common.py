"""Shared by test_demux_host.py and test_gpu_demux.py: the golden cases of tests/golden/trim_demux.json.gz (every file
the reference leaves for ``-o out.{name}.fastq``), and the runner that compares a ``trim_file`` run with them."""
import base64

from atropos_amd.trim import pipeline_from_args

from .conftest import load_golden

KINDS = ("too_short", "too_long", "untrimmed")

# ---------------------------------------------------------------------------------------------- golden cases
_GOLDEN = None
_INPUTS = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden("trim_demux.json.gz")["cases"]
    return _GOLDEN


def case_ids():
    return ["%d:%s" % (i, c["args"][:60]) for i, c in enumerate(golden())]


def input_text(case):
    """The text a case's run read: the named input of trim_cases.json.gz, or its first ``head`` records."""
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = load_golden("trim_cases.json.gz")["inputs"]
    text = base64.b64decode(_INPUTS[case["input"]])
    return text if case["head"] is None else b"".join(text.splitlines(True)[:4 * case["head"]])


def expected_files(case):
    return {name: base64.b64decode(blob) for name, blob in case["files"].items()}


def run_case(case, tmp_path, chunk_bytes=256 << 20):
    """A golden case through ``trim_file`` of the installed backend, writing to ``out.{name}.fastq`` in a directory
    of its own; returns ({file name: bytes} of everything the run left there, the pipeline).  An adapter without
    a name of its own is named by a running number: its file is looked at as ``out.#<position>.fastq``, as the
    fixture stores it."""
    src = tmp_path / "in.fastq"
    src.write_bytes(input_text(case))
    work = tmp_path / "run"
    work.mkdir()
    args = case["args"]
    for kind in KINDS:
        args = args.replace("{%s}" % kind, str(work / (kind + ".txt")))
    pipe = pipeline_from_args(args)
    pipe.trim_file(str(src), str(work / "out.{name}.fastq"), chunk_bytes=chunk_bytes)
    numbered = {"out.%s.fastq" % ad.name: "out.#%d.fastq" % pos for pos, ad in enumerate(pipe.adapters, 1)
                if ad.name.isdigit()}
    return {numbered.get(p.name, p.name): p.read_bytes() for p in work.iterdir()}, pipe


def check_case(case, tmp_path, chunk_bytes=256 << 20):
    got, pipe = run_case(case, tmp_path, chunk_bytes)
    exp = expected_files(case)
    assert sorted(got) == sorted(exp)
    for name in exp:
        assert got[name] == exp[name], name
    return got, pipe

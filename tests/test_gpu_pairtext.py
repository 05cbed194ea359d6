"""Interleaved FASTQ in and out on the MI355X: the kernels of ``atr_fastq_emit_pairs`` under every staged
instantiation against the plain model, the interleaved file drivers, and the fixture's cases end to end against the
files the reference writes (tests/golden/pairtext.json.gz)."""
import pytest

from tests import _pairtext_common as P
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def doc():
    return load_golden("pairtext.json.gz")


def test_pair_formatter_layouts(hip_backend):
    rep, calls = P.check_pairs_layouts(hip_backend)
    assert calls >= 27 + 18 + 6 + 3
    # interleaved chunks are staged as one span, two chunks (and two far spans of one chunk) side by side; every
    # layout also has tiles beyond the stage (the 2 900-base reads), which take the byte-per-lane path
    assert rep["interleaved"]["one"] > 50 and rep["halves"]["two"] > 50 and rep["two"]["two"] > 50
    assert all(r["overflow"] for r in rep.values())
    assert rep["shifted"]["one"] > 50 and rep["shifted"]["two"] > 50


def test_pair_formatter_tiles(hip_backend):
    reps = P.check_pairs_tiles(hip_backend)
    assert sorted(reps) == [0, 700, 780]
    for hint, rep in reps.items():
        assert rep["edge_calls"] == 6 and rep["empty_tile"] >= 1
        assert rep["permuted_unordered"] > 10 and rep["renamed_unordered"] > 5 and rep["renamed_staged"] > 5


def test_pair_formatter_stage_limit(hip_backend):
    reps = P.check_pairs_stage_limit(hip_backend)
    assert len(reps) == 3
    for hint, rep in reps.items():
        assert (rep["one"], rep["overflow"]) == (1, 1), (hint, rep)


def test_pair_formatter_is_deterministic(hip_backend):
    m1, m2, dest, which = P.pair_cases()["two"]
    run = P.PairRun(hip_backend, m1, m2, dest, which)
    dev = []
    for side in run.sides:
        dev += [side["data"], side["recs"], side["begin"], side["end"], side["ubegin"], side["uend"]]
    first = P.emit_pairs_call(hip_backend, dev, len(dest), run.d_dest, which, 700)
    assert first == P.emit_pairs_call(hip_backend, dev, len(dest), run.d_dest, which, 700)


def test_overwrite_plan_and_apply(hip_backend):
    total = P.check_overwrite_matrix(hip_backend)
    assert total[0] > 30 and total[1] > 30


def test_overwritten_counts(hip_backend, doc):
    from atropos_amd.fastq import FastqBatch
    from atropos_amd.trim import pipeline_from_args
    blobs = P.fixture_files(doc)
    pipe = pipeline_from_args(["-a", P.AD1, "-A", P.AD2, "-w", "10,20,20"], paired_input=True)
    pipe.run(FastqBatch.from_bytes(blobs["r1"])[0], FastqBatch.from_bytes(blobs["r2"])[0])
    assert pipe.overwritten[0] >= 5 and pipe.overwritten[1] >= 5
    again = pipeline_from_args(["-a", P.AD1, "-A", P.AD2, "-w", "10,20,20", "-l", "x"])
    again.run(*FastqBatch.from_bytes(blobs["il"])[0].mates())
    assert again.overwritten == pipe.overwritten


def test_drivers_of_an_interleaved_file(hip_backend, doc, tmp_path):
    from atropos_amd import _lib
    on_gpu = P.check_stats_interleaved(doc, tmp_path)
    assert P.check_detect_interleaved(doc, tmp_path) == 2
    # the statistics twin of the CPU tests counts what the kernels count
    prev = _lib.set_backend(P.PairTextEmuBackend(), _test_double=True)
    try:
        assert P.check_stats_interleaved(doc, tmp_path) == on_gpu
    finally:
        _lib.set_backend(prev, _test_double=True)


def test_fixture_cases_file_to_file(hip_backend, doc, tmp_path):
    from atropos_amd.fastq import FormatError
    paths = P.write_inputs(doc, tmp_path)
    size = P.odd_first_chunk(P.fixture_files(doc)["il"])
    for k, case in enumerate(doc["cases"]):
        if case["error"] is not None:
            with pytest.raises(FormatError) as err:
                P.run_case_files(case, paths, tmp_path, str(k), size)
            assert str(err.value) == case["error"]
            continue
        got = P.run_case_files(case, paths, tmp_path, str(k), size)
        assert got == P.want_files(case), (case["args"], case["input"], case["output"])


def test_fixture_cases_one_batch(hip_backend, doc):
    for case in doc["cases"]:
        if case["error"] is None:
            assert P.run_case_bytes(case, doc) == P.want_files(case), (case["args"], case["input"], case["output"])

"""GPU tier of known-contaminant detection: the reference's golden cases on the device, the device against the CPU
twin on 1 M synthetic reads and against a plain-Python restatement on a slice of them, the file drivers."""
import numpy as np
import pytest
import torch

from atropos_amd import _lib, detect, synth
from atropos_amd.fastq import FastqBatch

from . import _detect_common as DC
from ._detect_kernels_common import COMP, python_counters  # noqa: F401  (the model lives with the per-kernel checks)

pytestmark = pytest.mark.gpu

SLICE = 20000            # reads the plain-Python restatement looks at (about 15 s on one core)


@pytest.mark.parametrize("name", DC.case_names())
def test_golden_case_on_the_device(name, hip_backend):
    case = next(c for c in DC.golden()["cases"] if c["name"] == name)
    n = DC.run_case(case, hip_backend)
    assert n > 0 or name == "no_contaminants"


def synth_text(n, seed, known, length=150):
    return synth.contaminated_fastq(n, seed, known, length)


def _counters(det):
    c = det.counters()
    return c["kept"], c["distinct"], np.stack([c["matches"], c["hits"], c["max_n"], c["abundance"]])


def test_device_equals_twin_and_plain_python_on_synthetic_reads(hip_backend):
    case = DC.golden()["cases"][0]
    known = DC.known_of(case)
    n = 1 << 20
    rec = synth_text(n, 7, [s for s in known.sequences if len(s) >= 30])
    text = rec.tobytes()
    twin = DC.DetectEmuBackend()
    got = []
    for be in (hip_backend, twin):
        det = detect.KnownContaminantDetector(known, backend=be)
        det.add_batch(FastqBatch.from_bytes(text, backend=be)[0])
        got.append(_counters(det))
        det.close()
    print("1 M synthetic reads: kept %d, distinct %d, hits %d" % (got[0][0], got[0][1], int(got[0][2][1].sum())))
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1]
    assert np.array_equal(got[0][2], got[1][2])
    assert got[0][1] < got[0][0] and got[0][2][1].sum() > 100000 and got[0][2][3].sum() > 1000
    # a slice against the restatement of the contract
    part = rec[:SLICE]
    det = detect.KnownContaminantDetector(known, backend=hip_backend)
    det.add_batch(FastqBatch.from_bytes(part.tobytes(), backend=hip_backend)[0])
    reads = [bytes(r[3:153]).decode() for r in part]
    distinct, exp = python_counters(reads, list(known.iter_sequences()), 12, ("A",), 0.5)
    kept, dist, body = _counters(det)
    assert dist == distinct
    assert np.array_equal(body, exp)


def test_chunked_detect_file_equals_one_batch(hip_backend, tmp_path):
    case = DC.golden()["cases"][0]
    known = DC.known_of(case)
    rec = synth_text(40000, 11, [s for s in known.sequences if len(s) >= 30], length=120)
    path = tmp_path / "reads.fastq"
    path.write_bytes(rec.tobytes())
    det = detect.KnownContaminantDetector(known, n_reads=40000, backend=hip_backend)
    det.add_batch(FastqBatch.from_bytes(rec.tobytes(), backend=hip_backend)[0])
    one = det.summarize()
    assert one["matches"][0]
    chunked = detect.detect_file(str(path), known, max_reads=None, n_reads=40000, chunk_bytes=1 << 20)
    assert chunked == one
    # max_reads stops the file: equal to the head of the reads as one batch
    head = detect.KnownContaminantDetector(known, n_reads=5000, backend=hip_backend)
    head.add_batch(FastqBatch.from_bytes(rec[:5000].tobytes(), backend=hip_backend)[0])
    assert detect.detect_file(str(path), known, max_reads=5000, chunk_bytes=1 << 19) == head.summarize()


def test_paired_equals_two_single_runs(hip_backend, tmp_path):
    case = DC.golden()["cases"][0]
    known = DC.known_of(case)
    long_enough = [s for s in known.sequences if len(s) >= 30]
    recs = [synth_text(20000, 21, long_enough, length=100), synth_text(20000, 22, long_enough[3:], length=100)]
    paths = []
    for k, r in enumerate(recs):
        paths.append(str(tmp_path / ("r%d.fastq" % k)))
        open(paths[-1], "wb").write(r.tobytes())
    both = detect.detect_files(paths[0], paths[1], known, max_reads=None, n_reads=20000, chunk_bytes=1 << 20)
    singles = [detect.detect_file(p, known, max_reads=None, n_reads=20000, chunk_bytes=1 << 20) for p in paths]
    assert len(both["matches"]) == 2 and both["matches"][0] and both["matches"][1]
    assert both["matches"] == (singles[0]["matches"][0], singles[1]["matches"][0])
    assert {k: v for k, v in both.items() if k != "matches"} == {k: v for k, v in singles[0].items() if k != "matches"}


def test_unsupported_envelope_leaves_no_partial_counters(hip_backend):
    kc = detect.KnownContaminants()
    kc.add("x", "ACGTACGTACGTACGTACGTAC")
    good = "@a\n%s\n+\n%s\n" % ("ACGTTGCATGCATGACTGACTAGCTAGCTACGATCGAC", "I" * 38)
    text = (good + "@r\n%s\n+\n%s\n" % ("ACGT" * 81, "I" * 324)).encode()
    batch = FastqBatch.from_bytes(text, backend=hip_backend)[0]
    det = detect.KnownContaminantDetector(kc, backend=hip_backend)
    det.add_batch(batch)
    with pytest.raises(_lib.AtroposUnsupported):
        det.counters()
    h = det._create()
    block = hip_backend.detect_counters(h)
    with pytest.raises(_lib.AtroposUnsupported):
        hip_backend.detect_filter(h, batch.data, batch.records, 324, block)
    assert not hip_backend.detect_read(h, block).any()
    det.close()
    for k in (3, 33):
        with pytest.raises(_lib.AtroposUnsupported):
            detect.KnownContaminantDetector(kc, kmer_size=k, backend=hip_backend).counters()
    seq = "ACGTTGCAGGATCCATXGACTGACCATGGTACA"
    det = detect.KnownContaminantDetector(kc, backend=hip_backend)
    det.add_batch(FastqBatch.from_bytes(("@r\n%s\n+\n%s\n" % (seq, "I" * len(seq))).encode(), backend=hip_backend)[0])
    with pytest.raises(ValueError, match="1 read"):
        det.matches()

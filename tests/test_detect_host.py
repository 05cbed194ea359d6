"""CPU tier of known-contaminant detection (atropos_amd.detect): the golden cases of the reference through the
CPU twin of the kernels (tests/emu/emu_detect.cpp -- a harness, not parity evidence for the kernels), and the host
pieces on their own."""
import math
import random

import numpy as np
import pytest

from atropos_amd import _lib, detect
from atropos_amd.fastq import FastqBatch

from . import _detect_common as DC


@pytest.fixture(scope="module")
def twin():
    return DC.DetectEmuBackend()


@pytest.mark.parametrize("name", DC.case_names())
def test_golden_case_on_the_twin(name, twin):
    case = next(c for c in DC.golden()["cases"] if c["name"] == name)
    n = DC.run_case(case, twin)
    assert n > 0 or name == "no_contaminants"


def test_golden_file_is_not_hollow():
    cases = DC.golden()["cases"]
    assert len(cases) >= 18
    exact = sum(all(r["top_exact"] for r in c["results"]) for c in cases)
    assert 2 * exact >= len(cases)
    assert any(len(c["fastq"]) == 2 for c in cases)
    assert sum(bool(r["full"]) for c in cases for r in c["results"]) >= len(cases) - 1
    # the default limit of 20 cuts something: once with a defined top-20 list, once with a tie group at the cut
    first = [c["results"][0] for c in cases]
    assert any(len(r["full"]) > 20 and r["top_exact"] and r["top"] == r["full"][:20] for r in first)
    assert any(len(r["full"]) > 20 and not r["top_exact"] for r in first)
    # bit sets of one, two, three and four words
    words = set()
    for c in cases:
        known = c["known"] or DC.golden()["default_known"]
        most = max(detect.distinct_kmers(seq, c["options"]["kmer_size"]) for _, seq in known)
        words.add((most + 31) // 32)
    assert {1, 2, 3, 4} <= words


def test_limit_is_applied_after_the_sort(twin):
    case = next(c for c in DC.golden()["cases"] if c["name"] == "limit_cuts")
    det = DC.detector_of(case, twin)
    det.add_batch(FastqBatch.from_bytes(case["fastq"][0].encode(), backend=twin)[0])
    full = DC.rows(det.matches(limit=None))
    assert len(full) > 20
    assert DC.rows(det.matches()) == full[:20] and DC.rows(det.matches(limit=3)) == full[:3]


def test_forced_hash_collisions_keep_the_distinct_count_exact():
    """Every read gets the same hash: the distinct pass must fall back to byte compares and count exactly."""
    case = next(c for c in DC.golden()["cases"] if c["name"] == "duplicates")
    be = DC.DetectEmuBackend(force_hash=True)
    assert DC.run_case(case, be) > 0
    rng = random.Random(3)
    seqs = ["".join(rng.choice("ACGT") for _ in range(40)) for _ in range(50)]
    reads = [rng.choice(seqs) for _ in range(400)] + [s[:30] for s in seqs[:10]]
    text = "".join("@r\n%s\n+\n%s\n" % (s, "I" * len(s)) for s in reads)
    kc = detect.KnownContaminants()
    kc.add("x", "ACGTACGTACGTACGTACGTAC")
    for backend in (be, DC.DetectEmuBackend()):
        det = detect.KnownContaminantDetector(kc, backend=backend)
        det.add_batch(FastqBatch.from_bytes(text.encode(), backend=backend)[0])
        c = det.counters()
        assert c["distinct"] == len(set(reads)) and c["kept"] == len(reads)


def test_several_batches_are_one_set(twin):
    """Distinctness is over the whole run, not per add_batch."""
    case = next(c for c in DC.golden()["cases"] if c["name"] == "duplicates")
    text = case["fastq"][0].encode()
    lines = text.split(b"\n")
    cutoff = (len(lines) // 8) * 4
    parts = [b"\n".join(lines[:cutoff]) + b"\n", b"\n".join(lines[cutoff:])]
    det = DC.detector_of(case, twin)
    for p in parts:
        det.add_batch(FastqBatch.from_bytes(p, backend=twin)[0])
    DC.check_result(case, 0, det)


def test_known_contaminants_parsing(tmp_path):
    lines = ["# comment", ">a first description", "ACGT", "TTGG", "", ">b", "ACGTTTGG", ">c x", "GGGG", "#skip", "CC"]
    kc = detect.KnownContaminants.from_fasta(lines)
    assert kc.sequences == ["ACGTTTGG", "GGGGCC"]
    assert dict(kc.iter_sequences()) == {"ACGTTTGG": {"a", "b"}, "GGGGCC": {"c"}}
    assert kc.summarize() == dict(path=None, auto_reverse_complement=False, num_adapter_names=3, num_adapter_seqs=2)
    path = tmp_path / "k.fa"
    path.write_text("\n".join(lines) + "\n")
    assert detect.KnownContaminants.from_fasta(str(path)).sequences == kc.sequences
    with pytest.raises(ValueError):
        detect.KnownContaminants.from_fasta(["ACGT"])
    kc.add("d", "GGGGCC")
    assert dict(kc.iter_sequences())["GGGGCC"] == {"c", "d"} and len(kc) == 2 and kc.names == ["a", "b", "c", "d"]


def test_thresholds_against_brute_force():
    for frac in (0.0, 0.1, 0.25, 0.3, 1 / 3, 0.5, 0.75, 0.9, 1.0):
        nks = list(range(0, 130))
        got = detect.hit_thresholds(nks, frac)
        for nk, thr in zip(nks, got):
            hits = [n for n in range(nk + 1) if nk and n / nk > frac]
            assert thr == (hits[0] if hits else -1), (frac, nk)
            if thr > 0:
                assert not (thr - 1) / nk > frac


def test_complexity_table_against_the_direct_expression():
    f = detect.complexity_table(_lib.DETECT_MAX_READ)
    assert f.shape == (321, 321) and f.dtype == np.float64
    log2 = math.log(2)
    for n in range(1, 321):
        for count in range(1, n + 1):
            frac = count / float(n)
            assert f[n, count] == frac * math.log(frac) / log2
    # the exact-1.0 cases: two bases at 50 / 50; 25 / 25 of a longer length
    for n in (2, 20, 100, 320):
        assert -(0 + f[n, n // 2] + f[n, n // 2]) == 1.0
    assert -(0 + f[80, 20] + f[80, 20]) == 1.0
    assert detect.sequence_complexity("ACACACAC") == 1.0 and detect.sequence_complexity("acgtACGT") == 2.0
    assert detect.sequence_complexity("NNNN") == 0


def test_detect_from_args_accepts_and_rejects(tmp_path):
    fa = tmp_path / "k.fa"
    fa.write_text(">x\nACGTACGTACGTACGTTTGA\n")
    d = detect.detect_from_args(["-d", "known", "-k", "10", "--max-reads", "500", "-x", "a=ACGTTGCAACGTAC", "-F", str(fa),
                                 "-e", "A", "G", "--min-kmer-match-frac", "0.3", "-i", "known"])
    assert isinstance(d, detect.KnownContaminantDetector)
    assert (d.kmer_size, d.n_reads, d.past_end_bases, d.min_kmer_match_frac, d.include) == (10, 500, ("A", "G"), 0.3, "known")
    assert d.known_contaminants.sequences == ["ACGTTGCAACGTAC", "ACGTACGTACGTACGTTTGA"]
    assert isinstance(detect.detect_from_args(["-i", "known", "-x", "a=ACGTTGCAACGTAC"], paired=True), detect.PairedDetector)
    for bad in (["-d", "heuristic", "-x", "a=ACGT"], ["-d", "khmer", "-x", "a=ACGT"], ["-x", "a=ACGT"],
                ["-d", "known", "-x", "a=ACGT", "-e", "A{8,}.*"], ["-d", "known"],
                ["-d", "known", "-F", "https://example.org/list.fa"], ["-d", "known", "-x", "a=ACGT", "--adapter-cache-file", "f"],
                ["-d", "known", "-x", "a=ACGT", "--min-frequency", "0.1"]):
        with pytest.raises(NotImplementedError):
            detect.detect_from_args(bad)
    with pytest.raises(ValueError):
        detect.detect_from_args(["-d", "known", "-x", "a=ACGT", "--min-kmer-match-frac", "2"])


def test_unsupported_envelope_and_invalid_bases(twin):
    kc = detect.KnownContaminants()
    kc.add("x", "ACGTACGTACGTACGTACGTAC")
    text = ("@r\n%s\n+\n%s\n" % ("ACGT" * 81, "I" * 324)).encode()
    det = detect.KnownContaminantDetector(kc, backend=twin)
    det.add_batch(FastqBatch.from_bytes(text, backend=twin)[0])
    with pytest.raises(_lib.AtroposUnsupported):
        det.counters()
    for k in (3, 33):
        with pytest.raises(_lib.AtroposUnsupported):
            detect.KnownContaminantDetector(kc, kmer_size=k, backend=twin).counters()
    long_kc = detect.KnownContaminants()
    rng = random.Random(1)
    long_kc.add("long", "".join(rng.choice("ACGT") for _ in range(200)))       # 189 distinct 12-mers
    with pytest.raises(_lib.AtroposUnsupported):
        detect.KnownContaminantDetector(long_kc, backend=twin).counters()
    # more known sequences than the match kernel's LDS holds: 556 with up to 64 distinct k-mers each
    for count, ok in ((556, True), (557, False)):
        many = detect.KnownContaminants()
        for i in range(count):
            many.add("s%d" % i, "".join(rng.choice("ACGT") for _ in range(60)))
        d = detect.KnownContaminantDetector(many, backend=twin)
        if ok:
            assert d.counters()["kept"] == 0
        else:
            with pytest.raises(_lib.AtroposUnsupported):
                d.counters()
    for frac in (-0.1, 1.5):
        with pytest.raises(ValueError):
            detect.KnownContaminantDetector(kc, min_kmer_match_frac=frac)
    # a byte without a complement in a kept read: the reference raises KeyError
    seq = "ACGTTGCAGGATCCATXGACTGACCATGGTACA"
    det = detect.KnownContaminantDetector(kc, backend=twin)
    det.add_batch(FastqBatch.from_bytes(("@r\n%s\n+\n%s\n" % (seq, "I" * len(seq))).encode(), backend=twin)[0])
    with pytest.raises(ValueError, match="1 read"):
        det.matches()


def test_heuristic_pieces_raise():
    kc = detect.KnownContaminants()
    kc.add("x", "ACGTACGTACGTACGTACGTAC")
    with pytest.raises(NotImplementedError):
        detect.KnownContaminantDetector(kc, past_end_bases=("A{8,}.*|A{2,}$",))

"""CPU tier of the heuristic detector (atropos_amd.detect.HeuristicDetector): the plain model of _heuristic_common.py
against the reference's golden results, the CPU twin of the kernels (tests/emu/emu_kmer.cpp -- a harness, not parity
evidence for the kernels) against the model at the C ABI, and the whole detector on the twin."""
import ctypes as C
import os
import random
import subprocess

import pytest

from atropos_amd import _lib, detect

from . import _heuristic_common as H
from .emu import backend as emu


@pytest.fixture(scope="module")
def twin():
    return H.KmerEmuBackend()


def case_names():
    return [c["name"] for c in H.golden()["cases"]]


def case_of(name):
    return next(c for c in H.golden()["cases"] if c["name"] == name)


# ---------------------------------------------------------------------------------------------- model vs golden
def check_rows(ours, per_seed, key, model_sets=None):
    """``ours`` against the reference's rows of every seed: equal but for ``longest_match``, which must be one of the
    suffixes at the smallest index (``model_sets[seq]``, where given)."""
    for res in per_seed:
        ref = res[key]
        assert [r[:3] + r[4:] for r in ours] == [r[:3] + r[4:] for r in ref]
        for mine, theirs in zip(ours, ref):
            assert (mine[3] is None) == (theirs[3] is None)
            if model_sets is not None and theirs[3] is not None:
                assert theirs[3] in model_sets[mine[0]], mine[0]


@pytest.mark.parametrize("name", case_names())
def test_model_against_the_reference(name):
    case = case_of(name)
    o = case["options"]
    for k, reads in enumerate(case["reads"]):
        full, nd = H.model_rows(reads, o, case["known"], limit=None)
        if not case["defined"]:                                          # the rows differ between hash seeds: what does not
            for res in case["results"][k]:
                assert [r[:3] for r in full] == [r[:3] for r in res["full"]] and res["n_distinct"] == nd
            continue
        top = full[:20]                                                 # (the default limit cuts the sorted list)
        per_seed = case["results"][k]
        assert all(r["n_distinct"] == nd for r in per_seed)
        mo = H.Model(reads, o["kmer_size"], H.min_count_fn(o["n_reads"], len(reads[0]), o["overrep_cutoff"], o["min_frequency"]),
                     tuple(o["past_end_bases"]))
        sets = {r[0]: mo.support(r[0])[2] for r in full}
        check_rows(full, per_seed, "full", sets)
        check_rows(top, per_seed, "top", sets)
        for r in full:                                                  # the model's own value: the lowest record
            assert r[3] == mo.longest_match(r[0])[0]


def test_golden_file_is_not_hollow():
    cases = H.golden()["cases"]
    assert len(cases) >= 20 and 4 * sum(c["defined"] for c in cases) >= 3 * len(cases)
    assert all(len(per_file) == 8 for c in cases for per_file in c["results"])
    assert any(len(c["reads"]) == 2 for c in cases)
    assert sum(bool(c["results"][0][0]["full"]) for c in cases) >= len(cases) - 2      # (two cases are empty on purpose)
    rows = [r for c in cases for r in c["results"][0][0]["full"]]
    assert any(r[4] for r in rows) and any(not r[4] for r in rows)
    # the quirk case: the model flags candidates there, and only there among the two
    for name, flagged in (("poly_a_quirk", True), ("poly_a_quirk_control", False)):
        c = case_of(name)
        o = c["options"]
        mo = H.Model(c["reads"][0], 12, H.min_count_fn(o["n_reads"], len(c["reads"][0][0])))
        assert any(q for _, q in mo.entries.values()) == flagged
    c = case_of("reads_run_out")
    o = c["options"]
    mo = H.Model(c["reads"][0], 12, H.min_count_fn(o["n_reads"], len(c["reads"][0][0]), 100, 0.0))
    assert mo.levels == max(len(t) for t, _ in mo.D) + 1


# ---------------------------------------------------------------------------------------------- twin vs model
def planted(rng, n, length, motif, every=3):
    return [(H.rseq(rng, rng.randint(0, length - len(motif))) + motif + H.rseq(rng, length))[:length] if i % every == 0
            else H.rseq(rng, length) for i in range(n)]


@pytest.mark.parametrize("k0", [4, 12, 32])
def test_kmer_sizes_and_read_lengths(k0, twin):
    rng = random.Random(k0)
    motif = H.rseq(rng, 48)
    seqs = planted(rng, 120, 90, motif)
    seqs += [H.rseq(rng, n) for n in (0, 1, k0 - 1, k0, k0 + 1, 64, 65, 319, 320)] + [motif[:k0], motif[:k0 + 1]]
    seqs += [(H.rseq(rng, 200) + motif + H.rseq(rng, 320))[:320] for _ in range(6)]
    seqs[0] = seqs[0][:90].ljust(90, "C")
    # k0 = 4: thresholds that fall from level to level (14, 4, 1, 1 ...)
    n_reads, cutoff = (40, 1) if k0 == 4 else (len(seqs), 100)
    mo = H.check_against_model(seqs, twin, kmer_size=k0, n_reads=n_reads, overrep_cutoff=cutoff,
                               patterns=[motif[:20], motif, "ACGT" * 3, seqs[3][:30]])
    assert mo.levels > k0 + 2
    if k0 == 4:
        mins = [H.min_count_fn(n_reads, 90, 1)(k) for k in range(4, 12)]
        assert mins[0] > mins[1] > mins[2] >= mins[-1]


@pytest.mark.parametrize("nrep", [1, 63, 64, 65, 257, 16385])
def test_numbers_of_representatives(nrep, twin):
    rng = random.Random(nrep)
    motif = H.rseq(rng, 30)
    length = 24 if nrep > 1000 else 60
    seqs = set()
    while len(seqs) < nrep:
        one = (H.rseq(rng, rng.randint(0, 8)) + motif + H.rseq(rng, length))[:length] if len(seqs) % 4 == 0 else H.rseq(rng, length)
        if H.filter_seq(one, 12, ("A",)) == one:                        # (the filter keeps it whole: nrep distinct reads)
            seqs.add(one)
    seqs = sorted(seqs)
    rng.shuffle(seqs)
    seqs += seqs[:nrep // 3]                                            # duplicates: representatives are first records
    mo = H.check_against_model(seqs, twin, kmer_size=12, n_reads=min(nrep, 2000), ranks=nrep <= 257)
    assert len(mo.D) == nrep


def test_runs_of_every_length_and_many_classes(twin):
    """A k-mer occurring 1 .. 1025 times (runs that cross every block boundary of the rank kernel) and more than
    2^16 distinct classes, through the pair keys and the rank call themselves."""
    rng = random.Random(7)
    kmers = set()
    while len(kmers) < 46:
        kmers.add(H.rseq(rng, 12))
    kmers = sorted(kmers)
    times = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025] + list(range(3, 38))
    pool = [x for x, t in zip(kmers, times) for _ in range(t)]
    rng.shuffle(pool)
    seqs, at = [], 0
    while at < len(pool):                                               # reads of 12-mers joined by a 13th base that varies
        seqs.append("".join(x + "ACGT"[(at + i) % 4] for i, x in enumerate(pool[at:at + 5])) + H.rseq(rng, 6))
        at += 5
    seqs += [H.rseq(rng, 150) for _ in range(520)]                      # 72 000 more 12-mers, nearly all distinct
    mo = H.check_against_model(seqs, twin, kmer_size=12, n_reads=100000)
    counts = {}
    for text, _ in mo.D:
        for i in range(len(text) - 11):
            counts[text[i:i + 12]] = counts.get(text[i:i + 12], 0) + 1
    assert len(counts) > (1 << 16) and {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} <= set(counts.values())


def test_count_at_the_threshold(twin):
    """count == min_count is not over-represented, min_count + 1 is; a single over-represented level yields no
    candidate (the last non-empty level is never added)."""
    rng = random.Random(11)
    a, b = H.rseq(rng, 12), H.rseq(rng, 12)
    n_reads = 5000                                                      # min_count(12) = ceil(5000 * 0.001) = 5
    seqs = [H.rseq(rng, 20) + a + H.rseq(rng, 20) for _ in range(5)] + [H.rseq(rng, 20) + b + H.rseq(rng, 20) for _ in range(6)]
    seqs += [H.rseq(rng, 52) for _ in range(40)]
    mo = H.check_against_model(seqs, twin, kmer_size=12, n_reads=n_reads)
    assert H.min_count_fn(n_reads, 52)(12) == 5
    assert mo.table() == {(12, b, 6, 0)} and mo.over == {12: 1, 13: 0} and mo.candidates() == {}
    det = H.detector_for(seqs, twin, kmer_size=12, n_reads=n_reads)
    assert det.matches(limit=None) == [] and det.summarize()["matches"] == ([],)


def test_quirk_read(twin):
    rng = random.Random(13)
    ad = H.ADAPTERS[0]
    seqs = H.read_through(rng, [ad], 200, 80, frac=0.6, inserts=[10, 20, 30, 40])
    seqs.append(ad[:20] + "A" * 9 + H.rseq(rng, 51))                     # kept: exactly the 20-mer
    mo = H.check_against_model(seqs, twin, kmer_size=12, n_reads=len(seqs))
    assert {x for (k, x), (c, q) in mo.entries.items() if q} == {ad[:19], ad[1:20]}


def test_refusals_by_argument(twin):
    """2^31 slots, a capacity above 2^20, kmer_size outside 4 .. 32, 65 patterns: refused before any pointer is read."""
    fns = H.load_twin()
    big = 1 << 31
    assert fns["atr_detect_kmer_slots"][0](None, None, None, None, 1, big, 12, None, None, None, None) == -2
    assert fns["atr_detect_kmer_slots"][0](None, None, None, None, 1, big - 1, 12, None, None, None, None) == -1
    for k in (3, 33):
        assert fns["atr_detect_kmer_slots"][0](None, None, None, None, 1, 10, k, None, None, None, None) == -2
    assert fns["atr_detect_kmer_pair_keys"][0](None, None, big, None, None, 1, None, 1, None, None) == -2
    assert fns["atr_detect_kmer_pair_keys"][0](None, None, 10, None, None, 200, None, 121, None, None) == -2
    assert fns["atr_detect_kmer_rank"][0](None, None, None, big, None, None, None, None, C.byref(C.c_int64()), None, 0, None) == -2
    assert fns["atr_detect_kmer_rank_work_bytes"][0](big) == 0
    level = fns["atr_detect_kmer_level"][0]
    assert level(None, None, None, 10, None, None, None, None, None, None, None, 12, 0, None, None, (1 << 20) + 1, None, None) == -2
    assert level(None, None, None, 10, None, None, None, None, None, None, None, 12, 0, None, None, 1 << 20, None, None) == -1
    assert level(None, None, None, big, None, None, None, None, None, None, None, 12, 0, None, None, 0, None, None) == -2
    assert level(None, None, None, 10, None, None, None, None, None, None, None, 321, 0, None, None, 0, None, None) == -2
    assert fns["atr_detect_kmer_gather"][0](None, 1, None, None, None, (1 << 20) + 1, None, None) == -2
    assert fns["atr_detect_kmer_support"][0](None, 1, None, None, None, None, 65, None, None, None) == -2
    for k in (3, 33):
        det = H.detector_for(["ACGTTGCAGGATCCATGACTGACCATGGTACA"], twin, kmer_size=k)
        with pytest.raises(_lib.AtroposUnsupported):
            det.discover()
    det = H.detector_for(["ACGT" * 81], twin)
    with pytest.raises(_lib.AtroposUnsupported):
        det.discover()


def test_candidate_capacity(twin, monkeypatch):
    """More over-represented k-mers than the table holds: refused, whatever part was written."""
    rng = random.Random(17)
    seqs = H.read_through(rng, H.ADAPTERS, 120, 80, inserts=[10, 20, 30])
    monkeypatch.setattr(detect.HeuristicDetector, "CAPACITY", 50)
    det = H.detector_for(seqs, twin, n_reads=len(seqs))
    with pytest.raises(_lib.AtroposUnsupported, match="over-represented"):
        det.discover()


def test_zero_known_sequences_handle(twin):
    """A detector without known sequences filters without the shortest-known-sequence test."""
    h = twin.detect_create([], 12, b"A", [], detect._complexity_table(detect.MAX_READ), detect.MAX_READ)
    assert twin.detect_counters(h).shape[0] == _lib.DETECT_HDR
    twin.detect_destroy(h)


# ---------------------------------------------------------------------------------------------- the whole detector
@pytest.mark.parametrize("name", case_names())
def test_golden_case_on_the_twin(name, twin):
    case = case_of(name)
    o = case["options"]
    for k, reads in enumerate(case["reads"]):
        det = H.case_detector(case, k, twin)
        full = det.matches(limit=None)
        ours = H.match_rows(full)
        model, nd = H.model_rows(reads, o, case["known"], limit=None)
        assert ours == model and [[type(v) for v in r] for r in ours] == [[type(v) for v in r] for r in model]
        assert det.counters()["distinct"] == nd
        assert H.match_rows(det.matches()) == model[:20]
        if case["defined"]:
            check_rows(ours, case["results"][k], "full")
            check_rows(H.match_rows(det.matches()), case["results"][k], "top")
        summary = det.summarize(limit=None)
        assert summary["matches"] == ([m.summarize() for m in full],)
        for m, s in zip(full, summary["matches"][0]):
            assert set(s) == {"longest_kmer", "kmer_freq", "kmer_freq_type", "abundance", "is_known", "known_to_contaminant_match_frac",
                              "contaminant_to_known_match_frac", "longest_match", "known_names", "known_seqs"}
            assert (s["longest_kmer"], s["kmer_freq"], s["kmer_freq_type"], s["abundance"], s["is_known"]) == (
                m.seq, m.count, "count", m.abundance, m.is_known)
            assert s["longest_match"] == m.longest_match[0] and s["known_names"] == m.names
            assert (s["known_seqs"] is None) == (not m.is_known)
        assert ("known_contaminants" in summary) == bool(case["known"])
        det.close()
    if len(case["reads"]) == 2:
        pd = detect.PairedDetector(H.known_of(case), detector_class=detect.HeuristicDetector, kmer_size=o["kmer_size"],
                                   n_reads=o["n_reads"], backend=twin)
        from atropos_amd.fastq import FastqBatch
        pd.add_batch(*[FastqBatch.from_bytes(H.fastq(r), final=True, backend=twin)[0] for r in case["reads"]])
        both = pd.summarize(limit=None)["matches"]
        assert [[s["longest_kmer"] for s in side] for side in both] == [
            [r[0] for r in H.model_rows(reads, o, case["known"], limit=None)[0]] for reads in case["reads"]]
        pd.close()


def test_candidate_without_complement_is_a_value_error(twin):
    rng = random.Random(19)
    odd = "ACGTXCAGGATCCATGGACTGACCATGGTACAGTC"
    seqs = [H.rseq(rng, 20) + odd + H.rseq(rng, 25) for _ in range(60)] + [H.rseq(rng, 80) for _ in range(60)]
    kc = detect.KnownContaminants()
    kc.add("x", H.ADAPTERS[0])
    det = H.detector_for(seqs, twin, known=kc, n_reads=len(seqs))
    with pytest.raises(ValueError, match="complement"):
        det.matches()
    assert H.detector_for(seqs, twin, n_reads=len(seqs)).matches()[0].seq == odd


def test_detector_from_args(tmp_path):
    fa = tmp_path / "k.fa"
    fa.write_text(">x\nACGTACGTACGTACGTTTGA\n")
    d = detect.detector_from_args([])
    assert isinstance(d, detect.HeuristicDetector) and d.known_contaminants is None
    assert (d.kmer_size, d.n_reads, d.min_frequency, d.min_contaminant_match_frac, d.include) == (12, 10000, 0.001, 0.9, "all")
    d = detect.detector_from_args(["-k", "10", "--max-reads", "50000", "-F", str(fa), "--min-frequency", "0.01",
                                   "--min-contaminant-match-frac", "0.8", "-e", "A", "G"])
    assert isinstance(d, detect.HeuristicDetector) and d.known_contaminants.sequences == ["ACGTACGTACGTACGTTTGA"]
    assert (d.kmer_size, d.n_reads, d.min_frequency, d.min_contaminant_match_frac, d.past_end_bases) == (10, 50000, 0.01, 0.8, ("A", "G"))
    assert isinstance(detect.detector_from_args(["-i", "known", "-x", "a=ACGTTGCAACGTAC"]), detect.KnownContaminantDetector)
    assert isinstance(detect.detector_from_args(["-d", "known", "-x", "a=ACGTTGCAACGTAC"]), detect.KnownContaminantDetector)
    assert isinstance(detect.detector_from_args(["-i", "known"]), detect.HeuristicDetector)          # no list: as the reference
    d = detect.detector_from_args(["-i", "unknown", "-x", "a=ACGTTGCAACGTAC"])
    assert isinstance(d, detect.HeuristicDetector) and d.known_contaminants is None
    assert isinstance(detect.detector_from_args(["-d", "heuristic", "--max-reads", "100000"]), detect.HeuristicDetector)
    p = detect.detector_from_args(["-x", "a=ACGTTGCAACGTAC"], paired=True)
    assert isinstance(p, detect.PairedDetector) and isinstance(p.read2_detector, detect.HeuristicDetector)
    with pytest.raises(NotImplementedError, match="-d heuristic"):
        detect.detector_from_args(["--max-reads", "50001"])
    for bad in (["-d", "khmer"], ["-d", "known"], ["-e", "A{8,}.*"], ["--adapter-cache-file", "f"],
                ["-F", "https://example.org/list.fa"]):
        with pytest.raises(NotImplementedError):
            detect.detector_from_args(bad)
    with pytest.raises(ValueError):
        detect.detector_from_args(["--min-contaminant-match-frac", "2"])
    # detect_from_args is unchanged: it keeps raising for the heuristic detector and its options
    for bad in (["-d", "heuristic", "-x", "a=ACGT"], ["-x", "a=ACGT"], ["-d", "known", "-x", "a=ACGT", "--min-frequency", "0.1"]):
        with pytest.raises(NotImplementedError):
            detect.detect_from_args(bad)


def test_detect_file_two_chunks_equal_one(tmp_path, twin):
    rng = random.Random(23)
    seqs = H.read_through(rng, H.ADAPTERS, 240, 90, inserts=[15, 30, 45, 60])
    path = tmp_path / "r.fastq"
    path.write_bytes(H.fastq(seqs))
    _lib.set_backend(twin, _test_double=True)
    try:
        one = detect.detect_file(str(path), None, detector="heuristic", max_reads=200)
        two = detect.detect_file(str(path), None, detector="heuristic", max_reads=200, chunk_bytes=len(H.fastq(seqs)) // 2)
    finally:
        _lib.set_backend(None)
    assert one == two and one["matches"][0] and one["n_reads"] == 200
    assert [m["longest_kmer"] for m in one["matches"][0]] == [
        r[0] for r in H.model_rows(seqs[:200], dict(kmer_size=12, n_reads=200, overrep_cutoff=100, min_frequency=0.001,
                                                    past_end_bases=["A"], include="all", min_contaminant_match_frac=0.9))[0]]
    with pytest.raises(ValueError):
        detect.detect_file(str(path), None, detector="khmer")


# ---------------------------------------------------------------------------------------------- sanitizer program
def test_sanitized_fuzz_program(tmp_path):
    """tests/emu/kmer_fuzz_main.cpp: a stand-alone program over detect_kmer_core.hpp and the twin, against a model of
    its own in C++ (std::map), compiled with AddressSanitizer and UBSan and run as a child process."""
    exe = str(tmp_path / "kmer_fuzz")
    cpp = [os.path.join(emu._HERE, f) for f in ("kmer_fuzz_main.cpp", "emu_kmer.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DATR_HOST_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + emu._INC + cpp + ["-o", exe])
    done = subprocess.run([exe, "40"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0, done.stdout.decode("utf-8", "replace")[-3000:]
    assert b"ok" in done.stdout

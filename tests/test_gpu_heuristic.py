"""The kernels of atropos_amd/csrc/detect_kmer_kernels.hip and the heuristic detector on the device: the C-ABI checks of
tests/_heuristic_common.py against the plain Python model (candidate table, classes per level, level[], the classes at
kmer_size, support words), every golden case of the reference through ``HeuristicDetector`` and ``PairedDetector``,
and one case at size against numpy and ``bytes.find``.  Every comparison is exact."""
import random

import numpy as np
import pytest
import torch

from atropos_amd import detect
from atropos_amd.fastq import FastqBatch

from . import _heuristic_common as H

pytestmark = pytest.mark.gpu


def planted(rng, n, length, motif):
    return [(H.rseq(rng, rng.randint(0, length - len(motif))) + motif + H.rseq(rng, length))[:length] if i % 3 == 0
            else H.rseq(rng, length) for i in range(n)]


@pytest.mark.parametrize("k0", [4, 12, 32])
def test_kmer_sizes_and_read_lengths(k0, hip_backend):
    rng = random.Random(k0)
    motif = H.rseq(rng, 48)
    seqs = planted(rng, 120, 90, motif)
    seqs += [H.rseq(rng, n) for n in (0, 1, k0 - 1, k0, k0 + 1, 64, 65, 319, 320)] + [motif[:k0], motif[:k0 + 1]]
    seqs += [(H.rseq(rng, 200) + motif + H.rseq(rng, 320))[:320] for _ in range(6)]
    n_reads, cutoff = (40, 1) if k0 == 4 else (len(seqs), 100)
    pats = [motif[:20], motif, "ACGT" * 3, seqs[3][:30]]
    mo = H.check_against_model(seqs, hip_backend, kmer_size=k0, n_reads=n_reads, overrep_cutoff=cutoff, patterns=pats)
    assert mo.levels > k0 + 2
    # a worker stream, twice into the same tables
    side = torch.cuda.Stream(device=hip_backend.device)
    side.wait_stream(torch.cuda.current_stream(hip_backend.device))
    with torch.cuda.stream(side):
        det = H.detector_for(seqs, hip_backend, kmer_size=k0, n_reads=n_reads, overrep_cutoff=cutoff)
        first = det.discover()
        rows = {(tuple(r), t) for r, t in zip(first["rows"].tolist(), first["texts"])}
        level = first["level"].cpu().tolist()
        again = det.discover(recompute=True)
        assert {(tuple(r), t) for r, t in zip(again["rows"].tolist(), again["texts"])} == rows
        assert again["level"].cpu().tolist() == level == mo.level and again["over"] == mo.over
        assert {(r[0], t.decode("latin-1"), r[1], r[4]) for r, t in rows} == mo.table()
        assert det.support(pats) == [(mo.support(p)[0], mo.longest_match(p)) for p in pats]
        det.close()
    torch.cuda.current_stream(hip_backend.device).wait_stream(side)


@pytest.mark.parametrize("nrep", [1, 63, 64, 65, 257, 16385])
def test_numbers_of_representatives(nrep, hip_backend):
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
    seqs += seqs[:nrep // 3]
    mo = H.check_against_model(seqs, hip_backend, kmer_size=12, n_reads=min(nrep, 2000), ranks=nrep <= 257)
    assert len(mo.D) == nrep


def test_runs_of_every_length_and_many_classes(hip_backend):
    rng = random.Random(7)
    kmers = set()
    while len(kmers) < 46:
        kmers.add(H.rseq(rng, 12))
    kmers = sorted(kmers)
    times = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025] + list(range(3, 38))
    pool = [x for x, t in zip(kmers, times) for _ in range(t)]
    rng.shuffle(pool)
    seqs, at = [], 0
    while at < len(pool):
        seqs.append("".join(x + "ACGT"[(at + i) % 4] for i, x in enumerate(pool[at:at + 5])) + H.rseq(rng, 6))
        at += 5
    seqs += [H.rseq(rng, 150) for _ in range(520)]
    H.check_against_model(seqs, hip_backend, kmer_size=12, n_reads=100000)


def test_threshold_quirk_and_capacity(hip_backend, monkeypatch):
    rng = random.Random(11)
    a, b = H.rseq(rng, 12), H.rseq(rng, 12)
    seqs = [H.rseq(rng, 20) + a + H.rseq(rng, 20) for _ in range(5)] + [H.rseq(rng, 20) + b + H.rseq(rng, 20) for _ in range(6)]
    seqs += [H.rseq(rng, 52) for _ in range(40)]
    mo = H.check_against_model(seqs, hip_backend, kmer_size=12, n_reads=5000)
    assert mo.table() == {(12, b, 6, 0)} and mo.candidates() == {}
    rng = random.Random(13)
    ad = H.ADAPTERS[0]
    seqs = H.read_through(rng, [ad], 200, 80, frac=0.6, inserts=[10, 20, 30, 40])
    seqs.append(ad[:20] + "A" * 9 + H.rseq(rng, 51))
    mo = H.check_against_model(seqs, hip_backend, kmer_size=12, n_reads=len(seqs))
    assert {x for (k, x), (c, q) in mo.entries.items() if q} == {ad[:19], ad[1:20]}
    monkeypatch.setattr(detect.HeuristicDetector, "CAPACITY", 50)
    det = H.detector_for(seqs, hip_backend, n_reads=len(seqs))
    from atropos_amd import _lib
    with pytest.raises(_lib.AtroposUnsupported, match="over-represented"):
        det.discover()
    h = hip_backend.detect_create([], 12, b"A", [], detect._complexity_table(detect.MAX_READ), detect.MAX_READ)
    with pytest.raises(_lib.AtroposUnsupported):                         # no known sequences: the match pass is refused
        hip_backend.detect_match(h, None, None, None, torch.zeros((1,), dtype=torch.int64), None, None)
    hip_backend.detect_destroy(h)


@pytest.mark.parametrize("name", [c["name"] for c in H.golden()["cases"]])
def test_golden_case_on_the_device(name, hip_backend):
    case = next(c for c in H.golden()["cases"] if c["name"] == name)
    o = case["options"]
    sides = []
    for k, reads in enumerate(case["reads"]):
        det = H.case_detector(case, k, hip_backend)
        ours = H.match_rows(det.matches(limit=None))
        model, nd = H.model_rows(reads, o, case["known"], limit=None)
        assert ours == model and det.counters()["distinct"] == nd
        assert H.match_rows(det.matches()) == model[:20]
        if case["defined"]:
            for res in case["results"][k]:
                assert [r[:3] + r[4:] for r in ours] == [r[:3] + r[4:] for r in res["full"]]
        sides.append(det.summarize(limit=None)["matches"][0])
        det.close()
    if len(case["reads"]) == 2:
        pd = detect.PairedDetector(H.known_of(case), detector_class=detect.HeuristicDetector, kmer_size=o["kmer_size"],
                                   n_reads=o["n_reads"], backend=hip_backend)
        pd.add_batch(*[FastqBatch.from_bytes(H.fastq(r), final=True, backend=hip_backend)[0] for r in case["reads"]])
        assert pd.summarize(limit=None)["matches"] == tuple(sides)
        pd.close()


def check_at_size(backend):
    """(test_at_size) 2^18 reads x 100 bases, 40 % read-through of two planted adapters, 5 % duplicates.  Neither the reference nor the
    twin runs at this size: every level-k0 count against a numpy count over the distinct reads, abundance and the
    longest-match index of the final matches against ``bytes.find``, the final sequences against the model on a
    2 000-read sample of the same generator."""
    n, length, k0 = 1 << 18, 100, 12
    rng = np.random.default_rng(20261021)
    reads = rng.integers(0, 4, size=(n, length), dtype=np.uint8)
    ads = [np.frombuffer(a.encode(), dtype=np.uint8) for a in H.ADAPTERS]
    code = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = code[reads]
    through = np.nonzero(rng.random(n) < 0.4)[0]
    # inserts that leave room for the whole adapter: then every k-mer of an adapter has the same count, the longest
    # candidate has the largest sort key (len * log(count)) at any number of reads, and the final sequences of a sample
    # and of the whole set can be compared.  (With inserts that cut the adapter the key is not invariant under scale:
    # counts fall towards the adapter's end, and a 63-mer can outrank the 66-mer at 2 000 reads and not at 2^18.)
    inserts = rng.integers(10, length - max(len(a) for a in H.ADAPTERS) + 1, size=through.shape[0])
    which = rng.integers(0, 2, size=through.shape[0])
    for r, ins, w in zip(through.tolist(), inserts.tolist(), which.tolist()):
        ad = ads[w][:length - ins]
        reads[r, ins:ins + ad.shape[0]] = ad
    dup = np.nonzero(rng.random(n) < 0.05)[0]
    reads[dup] = reads[rng.integers(0, n, size=dup.shape[0])]
    texts = [row.tobytes() for row in reads]
    body = b"".join(b"@r\n" + t + b"\n+\n" + b"I" * length + b"\n" for t in texts)
    sample = [t.decode() for t in texts[:2000]]
    det = detect.HeuristicDetector(None, kmer_size=k0, n_reads=n, backend=backend)
    det.add_batch(FastqBatch.from_bytes(body, final=True, backend=backend)[0])
    found = det.discover()
    # the distinct reads as the filter keeps them, with the model's filter
    keep = {}
    for rec, t in enumerate(texts):
        kept = H.filter_seq(t.decode(), k0, ("A",))
        if kept is not None and kept not in keep:
            keep[kept] = rec
    D = list(keep)
    assert found["distinct"] == len(D)
    # level k0: packed 12-mers of the kept part of every distinct read, np.unique
    lut = np.zeros(256, np.int64)
    lut[code] = np.arange(4)
    codes = lut[reads[np.fromiter(keep.values(), dtype=np.int64)]]
    lens = np.fromiter((len(t) for t in D), dtype=np.int64)
    width = length - k0 + 1
    v = np.zeros((codes.shape[0], width), np.int64)
    for j in range(k0):
        v = v * 4 + codes[:, j:j + width]
    values, counts = np.unique(v[np.arange(width)[None, :] <= (lens[:, None] - k0)], return_counts=True)
    min_count = det.min_count(k0)
    expect = {int(v): int(c) for v, c in zip(values[counts > min_count], counts[counts > min_count])}
    got = {}
    for row, text in zip(found["rows"], found["texts"]):
        if int(row[0]) == k0:
            v = 0
            for ch in text:
                v = v * 4 + int(lut[ch])
            got[v] = int(row[1])
    assert got == expect and len(got) == found["over"][k0] and len(got) > 50
    matches = det.matches(limit=None)
    assert matches
    for m in matches:
        seq = m.seq
        hits = [(t.find(seq), keep[t]) for t in D if seq in t]
        assert m.abundance == len(hits)
        # the longest-match index: the smallest first index over the reads that hold the sequence (every such read holds
        # all its k-mers, so it is still in play at that level)
        assert len(seq) - m.longest_match[1] == min(h[0] for h in hits)
        first_rec = min(h for h in hits if h[0] == min(x[0] for x in hits))[1]
        assert m.longest_match[0] == H.filter_seq(texts[first_rec].decode(), k0, ("A",))[len(seq) - m.longest_match[1]:]
    small = H.model_rows(sample, dict(kmer_size=k0, n_reads=2000, overrep_cutoff=100, min_frequency=0.001, past_end_bases=["A"],
                                      include="all", min_contaminant_match_frac=0.9), limit=None)[0]
    print("at size:", [(m.seq, m.count, m.abundance) for m in matches], "sample:", [r[:3] for r in small])
    # (as sets: which of two adapters planted at the same rate has the larger count is chance)
    assert sorted(m.seq for m in matches) == sorted(r[0] for r in small) == sorted(H.ADAPTERS)
    det.close()


def test_at_size(hip_backend):
    check_at_size(hip_backend)

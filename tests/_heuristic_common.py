"""Shared by test_heuristic_host.py (the CPU twin, tests/emu/emu_kmer.cpp) and test_gpu_heuristic.py (the kernels of
atropos_amd/csrc/detect_kmer_kernels.hip): a plain Python model of the heuristic detector -- dicts and sets, written
from the description of the reference's algorithm and the tie rules in atropos_amd/detect.py's module doc, taken from
nowhere -- the twin's loader and backend, the golden cases of tests/golden/heuristic_cases.json.gz and the comparisons
at the C ABI.  Neither the twin nor the device has a hash hook: there is no hash in these passes."""
import ctypes as C
import math
import os
import random
import re
import subprocess

import numpy as np
import torch

from atropos_amd import _lib, detect
from atropos_amd.fastq import FastqBatch

from .conftest import load_golden
from .emu import backend as emu

KMER_ENTRY_POINTS = tuple(n for n in _lib.PROTOTYPES if n.startswith("atr_detect_kmer_"))
_twin = []


def twin_sources():
    cpp = os.path.join(emu._HERE, "emu_kmer.cpp")
    return cpp, [cpp, os.path.join(emu._HERE, "emu_abi.hpp"), os.path.join(emu._ROOT, "include", "atropos_hip.h")] + [
        os.path.join(emu._CSRC, f) for f in ("detect_kmer_core.hpp", "fastq_core.hpp")]


def build_twin():
    so = os.path.join(emu._HERE, "libemu_kmer.so")
    cpp, deps = twin_sources()
    if emu.stale(so, deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU"] + emu._INC + [cpp, "-o", so])
    return so


def load_twin():
    if not _twin:
        _twin.append(_lib.attach_prototypes(C.CDLL(build_twin()), "emu_", KMER_ENTRY_POINTS))
    return _twin[0]


class KmerEmuBackend(emu.EmuBackend, _lib.KmerCalls):
    """The CPU stand-in with the atr_detect_kmer_* entry points, which go to a twin library of their own."""

    def _call(self, name, *args):
        if name not in KMER_ENTRY_POINTS:
            return super()._call(name, *args)
        fn, at = load_twin()[name]
        return _lib._check(None, fn(*args) if at is None else fn(*args[:at], None, *args[at:]), name)

    _host = _call


# ---------------------------------------------------------------------------------------------- the model
def complexity(seq):
    up = seq.upper()
    total = 0.0
    for b in "ACGT":
        n = up.count(b)
        if n:
            p = n / float(len(up))
            total += p * math.log(p) / math.log(2)
    return -total


def filter_seq(seq, kmer_size, past_end_bases):
    """What a read keeps (None: dropped): complexity, the past-end cut, the length against kmer_size only."""
    if complexity(seq) <= 1.0:
        return None
    if past_end_bases:
        m = re.search("|".join(b + "{8,}.*|" + b + "{2,}$" for b in past_end_bases), seq)
        if m:
            seq = seq[:m.start()]
    return seq if len(seq) >= kmer_size and seq else None


def min_count_fn(n_reads, read_length, overrep_cutoff=100, min_frequency=0.001):
    return lambda k: math.ceil(n_reads * max(min_frequency, (read_length - k + 1) * overrep_cutoff / float(4 ** k)))


class Model(object):
    """The level loop over the distinct filtered reads.  ``D``: (text, first record) per distinct read, ``level``:
    the largest k with the read in S_k, ``entries``: {(k, text): [count, quirk]} of every over-represented k-mer,
    ``over``: their number per level, ``levels``: the first level without one."""

    def __init__(self, seqs, kmer_size, min_count, past_end_bases=("A",)):
        self.k0 = kmer_size
        self.kept = [filter_seq(s, kmer_size, past_end_bases) for s in seqs]
        seen = {}
        self.D = []
        for rec, text in enumerate(self.kept):
            if text is not None and text not in seen:
                seen[text] = len(self.D)
                self.D.append((text, rec))
        self.level = [kmer_size] * len(self.D)
        self.entries, self.over, self.first = {}, {}, {}
        members, prev, k = list(range(len(self.D))), None, kmer_size
        while True:
            kmers = {}
            for d in members:
                text = self.D[d][0]
                for i in range(len(text) - k + 1):
                    e = kmers.setdefault(text[i:i + k], [0, set(), (d, i)])       # (members ascend: the first occurrence)
                    e[0] += 1
                    e[1].add(d)
            cur = {x: e for x, e in kmers.items() if e[0] > min_count(k)}
            self.over[k] = len(cur)
            if not cur:
                self.levels = k
                break
            nxt = set()
            for x, (count, reads, first) in cur.items():
                self.entries[(k, x)] = [count, 0]
                self.first[(k, x)] = first
                nxt |= reads
            for d in nxt:
                self.level[d] = k + 1
            if prev:
                for x, (count, reads, _) in prev.items():
                    if any(self.D[d][0] in cur for d in reads):        # the whole read is an over-represented k-mer
                        self.entries[(k - 1, x)][1] = 1
            members, prev, k = sorted(nxt), cur, k + 1

    def table(self):
        return {(k, x, c, q) for (k, x), (c, q) in self.entries.items()}

    def candidates(self):
        out = {}
        for (k, x) in sorted(self.entries, key=lambda e: (e[0], self.first[e])):
            count, quirk = self.entries[(k, x)]
            if k <= self.levels - 2 and not quirk and complexity(x) > 1.0:
                out[x] = count
        return out

    def support(self, seq):
        """(abundance, the support word or None, the set of suffixes at the smallest index)."""
        abundance = sum(seq in text for text, _ in self.D)
        hits = [(text.index(seq), rec, text) for d, (text, rec) in enumerate(self.D) if self.level[d] >= len(seq) and seq in text]
        if not hits:
            return abundance, None, set()
        first = min(h[0] for h in hits)
        return abundance, min(hits)[:2], {text[first:] for idx, _, text in hits if idx == first}

    def longest_match(self, seq):
        _, word, _ = self.support(seq)
        if word is None:
            return None
        text = self.kept[word[1]]
        return (text[word[0]:], len(seq) - word[0])


def merge(results):
    """The greedy merge, the re-sort and the 50 % cut, from the description of the reference's loop."""
    results = sorted(results, key=lambda r: len(r[0]) * math.log(r[1]), reverse=True)
    merged = []
    while len(results) > 1:
        seq1, count1 = results[0]
        rest = []
        for seq2, count2 in results[1:]:
            if len(seq1) >= len(seq2) and seq2 in seq1:
                count1 += count2
            elif seq1 in seq2:
                if count1 < 2 * count2:
                    seq1 = seq2
                count1 += count2
            else:
                rest.append((seq2, count2))
        merged.append((seq1, count1))
        results = rest
    results = merged + results
    if not results:
        return []
    results.sort(key=lambda r: r[1], reverse=True)
    floor = int(results[0][1] * 0.5)
    return [r for r in results if r[1] >= floor]


COMP = dict(zip("ACGTRYSWKMBDHVNacgtryswkmbdhvn", "TGCAYRSWMKVHDBNtgcayrswmkvhdbn"))


def exact_overlap(seq1, seq2, min_overlap_frac):
    """An error-free, gap-free semiglobal alignment of at least ceil(frac * shorter) bases exists."""
    need = max(1, math.ceil(min(len(seq1), len(seq2)) * min_overlap_frac))
    for shift in range(-len(seq2) + 1, len(seq1)):
        lo, hi = max(0, shift), min(len(seq1), shift + len(seq2))
        if hi - lo >= need and seq1[lo:hi] == seq2[lo - shift:hi - shift]:
            return True
    return False


def model_rows(seqs, options, known=None, limit=20):
    """The rows [seq, count, abundance, longest_match, is_known, names, known_seqs (by repr), match_frac, match_frac2]
    the model reports for the reads ``seqs`` (in record order)."""
    o = options
    k0, n_reads = o["kmer_size"], o["n_reads"]
    if not seqs:
        return [], 0
    mc = min_count_fn(n_reads, len(seqs[0]), o["overrep_cutoff"], o["min_frequency"])
    mo = Model(seqs, k0, mc, tuple(o["past_end_bases"]))
    found = []
    for seq, count in merge(list(mo.candidates().items())):
        found.append(dict(seq=seq, count=count, abundance=mo.support(seq)[0], longest=mo.longest_match(seq), names=None,
                          known_seqs=None, frac=None, frac2=None))
    if known and found:
        frac_min = o["min_contaminant_match_frac"]
        kn = {}                                                        # sequence -> names, first-seen order
        for name, s in known:
            kn.setdefault(s, set()).add(name)
        kmers_of = lambda s: {s[i:i + k0] for i in range(len(s) - k0 + 1)}
        best_of = {}                                                   # known sequence -> (match index, fracs)
        unknown = []
        for at, m in enumerate(found):
            best, bar = {}, (frac_min, 0)
            for text in [m["seq"]] + ([m["longest"][0]] if m["longest"] else []):
                rc = "".join(COMP[c] for c in reversed(text))
                for s in kn:
                    fw, rv = kmers_of(text), kmers_of(rc)
                    nf, nr = float(len(kmers_of(s) & fw)), float(len(kmers_of(s) & rv))
                    n, mine, cmp_seq = (nf, fw, text) if nf >= nr else (nr, rv, rc)
                    f1 = n / len(kmers_of(s)) if kmers_of(s) else 0
                    f2 = n / len(mine) if mine else 0
                    if f1 < bar[0]:
                        continue
                    if s in cmp_seq or exact_overlap(cmp_seq, s, frac_min):
                        if f1 > bar[0] or (f1 == bar[0] and f2 > bar[1]):
                            best, bar = {}, (f1, f2)
                        best[s] = (at, (f1, f2))
            if best:
                for s, hit in best.items():
                    if s not in best_of or hit[1] > best_of[s][1]:
                        best_of[s] = hit
            else:
                unknown.append(at)
        by_match = {}
        for s, (at, fracs) in best_of.items():
            by_match.setdefault(at, []).append((s, fracs))
        order = []
        for at, hits in by_match.items():
            hits.sort(key=lambda h: h[1], reverse=True)
            s, fracs = hits[0]
            same = [h for h in hits[1:] if h[1] == fracs]
            m = found[at]
            if not same:
                m.update(names=sorted(kn[s]), known_seqs=[s])
            else:
                names, ks = set(kn[s]), {(s,)}
                for other, _ in same:
                    names |= kn[other]
                    ks.add(other)
                m.update(names=sorted(names), known_seqs=sorted(ks, key=repr))
            m.update(frac=fracs[0], frac2=fracs[1])
            order.append(at)
        found = [found[at] for at in order + unknown]

    def keep(m):
        known_ = m["known_seqs"] is not None
        return not (m["count"] < 0.1 * n_reads or len(m["seq"]) < k0 or complexity(m["seq"]) < 1.1
                    or (o["include"] == "known" and not known_) or (o["include"] == "unknown" and known_)
                    or (known_ and m["frac"] < 0.1))

    found = [m for m in found if keep(m)]
    found.sort(key=lambda m: len(m["seq"]) * math.log(m["count"]), reverse=True)
    found = found if limit is None else found[:limit]
    rows = [[m["seq"], m["count"], m["abundance"], m["longest"][0] if m["longest"] else None, m["known_seqs"] is not None,
             m["names"], jsonable(m["known_seqs"]), m["frac"], m["frac2"]] for m in found]
    return rows, len(mo.D)


def jsonable(known_seqs):
    """known_seqs as the golden file stores it: the 1-tuple becomes a list."""
    return None if known_seqs is None else [list(s) if isinstance(s, tuple) else s for s in known_seqs]


def match_rows(matches):
    return [[m.seq, m.count, m.abundance, m.longest_match[0] if m.longest_match else None, m.is_known,
             list(m.names) if m.names else None, jsonable(m.known_seqs), m.match_frac, m.match_frac2] for m in matches]


# ---------------------------------------------------------------------------------------------- at the C ABI
def fastq(seqs):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)).encode("latin-1")


def detector_for(seqs, backend, known=None, **kwargs):
    det = detect.HeuristicDetector(known, backend=backend, **kwargs)
    if seqs:
        det.add_batch(FastqBatch.from_bytes(fastq(seqs), final=True, backend=backend)[0])
    return det


def check_against_model(seqs, backend, kmer_size=12, n_reads=None, patterns=(), ranks=True, **kwargs):
    """The device state after ``HeuristicDetector.discover`` (every atr_detect_kmer_* call goes through it) against the
    model: the candidate table as a set, the classes per level, level[], the classes at kmer_size, the support words
    of the final sequences and of ``patterns``.  Returns the model."""
    n_reads = len(seqs) if n_reads is None else n_reads
    det = detector_for(seqs, backend, kmer_size=kmer_size, n_reads=n_reads, **kwargs)
    mc = min_count_fn(n_reads, len(seqs[0]), det.overrep_cutoff, det.min_frequency)
    mo = Model(seqs, kmer_size, mc, det.past_end_bases)
    for k in range(kmer_size, kmer_size + 40):
        assert det.min_count(k) == mc(k)
    found = det.discover()
    assert found["distinct"] == len(mo.D) and found["kept"] == sum(t is not None for t in mo.kept)
    rows = found["rows"]
    got = {(int(r[0]), t.decode("latin-1"), int(r[1]), int(r[4])) for r, t in zip(rows, found["texts"])}
    assert len(got) == len(rows)
    assert got == mo.table()
    firsts = {(int(r[0]), t.decode("latin-1")): (int(r[2]), int(r[3])) for r, t in zip(rows, found["texts"])}
    assert firsts == mo.first
    assert found["levels"] == mo.levels
    assert found["over"] == mo.over
    if mo.D:
        assert found["level"].cpu().tolist() == mo.level
        tab = found["tab"].cpu().numpy()
        assert tab[:, 2].tolist() == [rec for _, rec in mo.D]
        if ranks:
            check_ranks(det, found, mo)
    assert det.candidates() == mo.candidates() and list(det.candidates()) == list(mo.candidates())
    final = [s for s, _ in merge(list(mo.candidates().items()))]
    pats = final + [p for p in patterns if p not in final]
    if pats and mo.D:
        for seq, (ab, lm) in zip(pats, det.support(pats)):
            assert (ab, lm) == (mo.support(seq)[0], mo.longest_match(seq)), seq
    det.close()
    return mo


def check_ranks(det, found, mo):
    """Two slots have the same class at kmer_size exactly when their k-mers are the same text; no room, no class."""
    be, k0 = det.backend, det.kmer_size
    total = sum(len(t) for t, _ in mo.D)
    slot_rep = found["slot_rep"]
    assert slot_rep.shape[0] == total
    cls, (begin, end, head) = det._ranks_at_k0(be, found["tab"], slot_rep, found["batch"].data, total, detect._Clock(be, False))
    cls = cls.cpu().numpy()[:total]
    texts = []
    for text, _ in mo.D:
        texts += [text[o:o + k0] if o + k0 <= len(text) else None for o in range(len(text))]
    assert slot_rep.cpu().tolist() == [d for d, (t, _) in enumerate(mo.D) for _ in t]
    by_class = {}
    for c, x in zip(cls.tolist(), texts):
        if x is None:
            assert c == -1
        else:
            assert c >= 0 and by_class.setdefault(c, x) == x
    assert len(set(by_class.values())) == len(by_class) == len({x for x in texts if x is not None})
    # the classes' runs: count = end - begin
    counts = {}
    for x in texts:
        if x is not None:
            counts[x] = counts.get(x, 0) + 1
    b, e = begin.cpu().numpy(), end.cpu().numpy()
    assert {x: int(e[c] - b[c]) for c, x in by_class.items()} == counts


# ---------------------------------------------------------------------------------------------- read sets
def rseq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def read_through(rng, adapters, n, length, frac=0.4, inserts=None):
    out = []
    for _ in range(n):
        if rng.random() < frac:
            ins = rng.choice(inserts) if inserts else rng.randint(length // 4, length - 5)
            out.append((rseq(rng, ins) + rng.choice(adapters) + rseq(rng, length))[:length])
        else:
            out.append(rseq(rng, length))
    return out


ADAPTERS = ("AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCACGATCTCGTATGCCGTCTTCTGCTTG", "CTGTCTCTTATACACATCTCCGAGCCCACGAGACTAAGGCGAATCTCGTATGCCGTCTTCTGCTTG")

_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden("heuristic_cases.json.gz")
    return _GOLDEN


def known_of(case):
    if not case["known"]:
        return None
    kc = detect.KnownContaminants()
    for name, seq in case["known"]:
        kc.add(name, seq)
    return kc


def case_detector(case, k, backend, cls=None):
    o = case["options"]
    det = detect.HeuristicDetector(known_of(case), kmer_size=o["kmer_size"], n_reads=o["n_reads"], overrep_cutoff=o["overrep_cutoff"],
                                   include=o["include"], past_end_bases=tuple(o["past_end_bases"]), min_frequency=o["min_frequency"],
                                   min_contaminant_match_frac=o["min_contaminant_match_frac"], backend=backend)
    if case["reads"][k]:
        det.add_batch(FastqBatch.from_bytes(fastq(case["reads"][k]), final=True, backend=backend)[0])
    return det

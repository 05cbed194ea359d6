"""Shared by test_detect_host.py and test_gpu_detect.py: the golden cases of tests/golden/detect_cases.json.gz,
the comparison rule, and the loader of the CPU twin (tests/emu/emu_detect.cpp)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import torch

from atropos_amd import detect
from atropos_amd.fastq import FastqBatch

from .conftest import ROOT, load_golden
from .emu.backend import EmuBackend, _check, _ptr

_HERE = os.path.join(ROOT, "tests", "emu")
_SO = os.path.join(_HERE, "libemu_detect.so")
_SRCS = [os.path.join(_HERE, "emu_detect.cpp"), os.path.join(ROOT, "atropos_amd", "csrc", "detect_core.hpp"),
         os.path.join(ROOT, "atropos_amd", "csrc", "fastq_core.hpp"), os.path.join(ROOT, "include", "atropos_hip.h")]


def build_twin():
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "atropos_amd", "csrc"),
                               _SRCS[0], "-o", _SO])
    return _SO


class DetectEmuBackend(EmuBackend):
    """The CPU test backend plus the detect twin.  ``force_hash``: every read hashes alike (test hook)."""

    def __init__(self, force_hash=False):
        super().__init__()
        self.det = C.CDLL(build_twin())
        self.det.emu_detect_counter_words.restype = C.c_int64
        self.det.emu_detect_counter_words.argtypes = [C.c_void_p]
        self.det.emu_detect_destroy.restype = None
        self.det.emu_detect_destroy.argtypes = [C.c_void_p]
        self.det.emu_detect_create.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.det.emu_detect_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int]
        self.det.emu_detect_mark.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p]
        self.det.emu_detect_match.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_void_p]
        self.force_hash = bool(force_hash)

    def detect_create(self, seqs, kmer_size, past_end_bases, thresholds, complexity, max_len):
        lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
        thr = np.asarray(thresholds, dtype=np.int32)
        cx = np.ascontiguousarray(complexity, dtype=np.float64)
        h = C.c_void_p()
        _check(self.det.emu_detect_create(b"".join(seqs), lens.ctypes.data, len(seqs), int(kmer_size), bytes(past_end_bases),
                                          len(past_end_bases), thr.ctypes.data, cx.ctypes.data, int(max_len), C.byref(h)),
               "atr_detect_create")
        return h

    def detect_destroy(self, h):
        self.det.emu_detect_destroy(h)

    def detect_counters(self, h):
        return torch.zeros((self.det.emu_detect_counter_words(h),), dtype=torch.int64)

    def detect_filter(self, h, data, records, longest, counters):
        n = records.shape[0]
        kept = torch.zeros((n,), dtype=torch.int32)
        hashes = torch.zeros((n,), dtype=torch.int64)
        _check(self.det.emu_detect_filter(h, _ptr(data), _ptr(records), n, int(longest), _ptr(kept), _ptr(hashes),
                                          _ptr(counters), int(self.force_hash)), "atr_detect_filter_batch")
        return kept, hashes

    def detect_mark(self, h, data, records, kept, order, head, counters):
        rep = torch.zeros((order.shape[0],), dtype=torch.uint8)
        _check(self.det.emu_detect_mark(h, _ptr(data), _ptr(records), _ptr(kept), _ptr(order), _ptr(head), order.shape[0],
                                        _ptr(rep), _ptr(counters)), "atr_detect_mark_batch")
        return rep

    def detect_match(self, h, data, records, kept, order, rep, counters):
        _check(self.det.emu_detect_match(h, _ptr(data), _ptr(records), _ptr(kept), _ptr(order), _ptr(rep), order.shape[0],
                                         _ptr(counters)), "atr_detect_batch")

    def detect_read(self, h, counters):
        return counters.numpy().copy()


# ---------------------------------------------------------------------------------------------- golden cases
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden("detect_cases.json.gz")
    return _GOLDEN


def case_names():
    return [c["name"] for c in golden()["cases"]]


def known_of(case):
    kc = detect.KnownContaminants()
    for name, seq in case["known"] or golden()["default_known"]:
        kc.add(name, seq)
    return kc


def detector_of(case, backend, known=None):
    o = case["options"]
    return detect.KnownContaminantDetector(known or known_of(case), kmer_size=o["kmer_size"], n_reads=o["n_reads"],
                                           overrep_cutoff=o["overrep_cutoff"], include=o["include"],
                                           past_end_bases=tuple(o["past_end_bases"]),
                                           min_kmer_match_frac=o["min_kmer_match_frac"], backend=backend)


def rows(matches):
    return [[m.seq, m.count, m.abundance, m.match_frac, sorted(m.names)] for m in matches]


def grouped(rows_):
    """[(sort key, set of sequences)] of a sorted match list: the order up to ties."""
    out = []
    for seq, count, _, _, _ in rows_:
        key = len(seq) * math.log(count)
        if out and out[-1][0] == key:
            out[-1][1].add(seq)
        else:
            out.append((key, {seq}))
    return out


def check_result(case, k, det):
    """The comparison rule of the golden cases for read file ``k`` of ``case`` (see make_detect_golden.py)."""
    ref = case["results"][k]
    name = "%s[%d]" % (case["name"], k)
    assert det.counters()["distinct"] == ref["n_distinct"], name
    ours = rows(det.matches(limit=None))
    assert {r[0]: r[1:] for r in ours} == {r[0]: r[1:] for r in ref["full"]}, name      # exact, floats included
    assert len(ours) == len(ref["full"]), name
    assert grouped(ours) == grouped(ref["full"]), name
    # inside a group of equal keys ours come in the order of the known list
    index = {seq: i for i, seq in enumerate(det.known_contaminants.sequences)}
    for a, b in zip(ours, ours[1:]):
        if len(a[0]) * math.log(a[1]) == len(b[0]) * math.log(b[1]):
            assert index[a[0]] < index[b[0]], name
    if ref["top_exact"]:
        top = rows(det.matches())
        assert {r[0]: r[1:] for r in top} == {r[0]: r[1:] for r in ref["top"]}, name
        assert grouped(top) == grouped(ref["top"]), name
    return len(ours)


def run_case(case, backend):
    known = known_of(case)
    total = 0
    for k, text in enumerate(case["fastq"]):
        det = detector_of(case, backend, known)
        batch, _ = FastqBatch.from_bytes(text.encode("latin-1"), final=True, backend=backend)
        det.add_batch(batch)
        total += check_result(case, k, det)
        det.close()
    return total

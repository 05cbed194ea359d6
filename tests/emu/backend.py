"""TEST INFRASTRUCTURE: the backend the CPU test-suite installs through ``atropos_amd._lib.set_backend``.  It serves the
product's own wrappers (``_lib.AbiCalls``) and prototypes (``_lib.PROTOTYPES``) with the lock-step CPU emulation of
the gfx950 kernels: the twins under tests/emu/, compiled from the product's per-lane source with -DATR_HOST_EMU, export
``emu_x`` with the signature of ``atr_x`` (emu_abi.hpp checks that when they compile).  Never importable from the
product package."""
import ctypes as C
import os
import subprocess

import torch

from atropos_amd import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "atropos_amd", "csrc")
_INC = ["-I" + os.path.join(_ROOT, "include"), "-I" + _CSRC]

# twin library -> (its sources, the product headers a rebuild depends on, the optimisation level, the entry points it
# stands in for as prefixes of their names without "atr_").  "locate" serves every entry point no other row claims.
TWINS = {
    "locate": (("emu_locate.cpp", "emu_insert.cpp", "emu_misc.cpp", "emu_fastq.cpp"),
               ("locate_core.hpp", "aligner_host.hpp", "insert_core.hpp", "insert_host.hpp", "misc_core.hpp", "filter_core.hpp",
                "piece_core.hpp", "fastq_core.hpp", "pairs_core.hpp", "pairs_fast_core.hpp", "linked_core.hpp", "linked_host.hpp"),
               "-O1", ()),
    "demux": (("emu_demux.cpp",), ("demux_core.hpp", "fastq_core.hpp"), "-O1", ("fastq_emit_grouped", "demux_")),
    "report": (("emu_report.cpp",), ("report_core.hpp", "fastq_core.hpp"), "-O1", ("report_",)),
    "detect": (("emu_detect.cpp",), ("detect_core.hpp", "fastq_core.hpp"), "-O1", ("detect_",)),
    "gzip": (("emu_gzip.cpp",), ("deflate_core.hpp",), "-O2", ("gzip_",)),
    "gunzip": (("emu_gunzip.cpp",), ("inflate_core.hpp", "deflate_core.hpp"), "-O2", ("gunzip_", "bgzf_")),
}
_loaded = {}


def twin_sources(name):
    """(the .cpp files of twin ``name``, everything a rebuild of it depends on)."""
    cpps = [os.path.join(_HERE, f) for f in TWINS[name][0]]
    return cpps, cpps + [os.path.join(_CSRC, f) for f in TWINS[name][1]] + [
        os.path.join(_HERE, "emu_abi.hpp"), os.path.join(_ROOT, "include", "atropos_hip.h")]


def stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def build_twin(name):
    so = os.path.join(_HERE, "libemu_%s.so" % name)
    cpps, deps = twin_sources(name)
    if stale(so, deps):
        subprocess.check_call(["g++", TWINS[name][2], "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU"] + _INC + cpps + ["-o", so])
    return so


def twin_of(name):
    """The twin library that stands in for entry point ``name`` (an ``atr_`` name)."""
    for twin, row in TWINS.items():
        if name[4:].startswith(row[3] or ("\0",)):
            return twin
    return "locate"


def load_twin(name):
    """Twin library ``name``, compiled if stale and loaded once per process: (the CDLL, {atr_ name: (function, stream
    position)} of the entry points it exports a stand-in for, with ``_lib.PROTOTYPES``' own prototypes)."""
    if name not in _loaded:
        lib = C.CDLL(build_twin(name))
        mine = [n for n in _lib.PROTOTYPES if twin_of(n) == name and hasattr(lib, "emu_" + n[4:])]
        _loaded[name] = (lib, _lib.attach_prototypes(lib, "emu_", mine))
    return _loaded[name]


class EmuBackend(_lib.AbiCalls):
    name = "emu"
    device = torch.device("cpu")

    def __init__(self):
        self.lib = load_twin("locate")[0]       # (the tests reach the emulation's own hooks and globals through it)
        self.inflate_calls = 0

    # -- what AbiCalls asks of a backend -------------------------------------------
    def empty(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)   # (the twins rely on zeroed outputs)

    def _symbol(self, name):
        return load_twin(twin_of(name))[1][name][0]

    def _call(self, name, *args):
        """No device, no stream: the twin gets NULL where the entry point takes one."""
        fn, at = load_twin(twin_of(name))[1][name]
        return _lib._check(None, fn(*args) if at is None else fn(*args[:at], None, *args[at:]), name)

    _host = _call

    def _workspace(self, need, first=0):
        return self.empty((max(need, first, 16),), torch.uint8)

    # -- the differences ------------------------------------------------------------
    def translate_table(self, kind):
        # no atr_translate_table twin: the fixed tables come from the same aligner_host.hpp code via throw-away aligners
        h = self.aligner_create(b"A", 0.1, 15, kind == _lib.TABLE_ACGT, kind == _lib.TABLE_IUPAC, 1, 1)
        got, table = self.aligner_query_table(h)
        self.aligner_destroy(h)
        assert got == kind
        return table

    def locate_planes_applies(self, h, max_len, ragged=False):
        # the emulation takes every width of the pre-pass's envelope, not only the ones the library instantiates
        fn = self.lib.emu_locate_planes_all_widths
        fn.argtypes = _lib.PROTOTYPES["atr_locate_planes_applies"][1]
        return bool(fn(h, int(max_len), int(bool(ragged))))

    def insert_match_correct_batch(self, h, planes1, planes2, seq1, qual1, seq2, qual2, action, min_qual_diff, comp,
                                   changed=None, newlen=None):
        # no fused kernel to emulate: the two steps of its contract one after the other
        out = self.insert_match_batch(h, planes1.packed, planes1.lens, planes2.packed, planes2.lens, planes1.nreads, planes1.max_len)
        changed, newlen = self.insert_correct_batch(out, seq1, qual1, planes1.lens, seq2, qual2, planes2.lens, action, min_qual_diff,
                                                    comp, changed, newlen, planes1=planes1, planes2=planes2)
        return out, changed, newlen

    def gunzip_members(self, *args):
        # test hook: the drivers' tests count the inflate calls
        self.inflate_calls += 1
        return super().gunzip_members(*args)

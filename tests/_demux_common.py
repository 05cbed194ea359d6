"""Shared by test_demux_host.py and test_gpu_demux.py: the golden cases of tests/golden/trim_demux.json.gz (every file
the reference leaves for ``-o out.{name}.fastq``), the runner that compares a ``trim_file`` run with them, and the
loader of the CPU twin (tests/emu/emu_demux.cpp)."""
import base64
import ctypes as C
import os
import subprocess

import torch

from atropos_amd.trim import pipeline_from_args

from .conftest import ROOT, load_golden
from .emu.backend import EmuBackend, _check, _ptr

_HERE = os.path.join(ROOT, "tests", "emu")
_SO = os.path.join(_HERE, "libemu_demux.so")
_SRCS = [os.path.join(_HERE, "emu_demux.cpp"), os.path.join(ROOT, "atropos_amd", "csrc", "demux_core.hpp"),
         os.path.join(ROOT, "atropos_amd", "csrc", "fastq_core.hpp"), os.path.join(ROOT, "include", "atropos_hip.h")]
KINDS = ("too_short", "too_long", "untrimmed")


def build_twin():
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in _SRCS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DATR_HOST_EMU",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "atropos_amd", "csrc"),
                               _SRCS[0], "-o", _SO])
    return _SO


class DemuxEmuBackend(EmuBackend):
    """The CPU test backend plus the twin of the grouped formatter and the group codes."""

    def __init__(self):
        super().__init__()
        self.dmx = C.CDLL(build_twin())
        self.dmx.emu_fastq_emit_grouped.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int64] + [C.c_void_p] * 3
        self.dmx.emu_demux_groups.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int64, C.c_void_p]

    def fastq_emit_grouped(self, data, records, begin, end, ubegin, uend, group, n_groups):
        n = records.shape[0]
        offsets = torch.zeros((max(n, 1),), dtype=torch.int64)
        bounds = torch.zeros((max(int(n_groups), 0) + 1,), dtype=torch.int64)
        args = (_ptr(data), _ptr(records), _ptr(begin), _ptr(end), _ptr(ubegin), _ptr(uend), _ptr(group), int(n_groups),
                C.c_int64(n), _ptr(offsets), _ptr(bounds))
        _check(self.dmx.emu_fastq_emit_grouped(*args, None), "emu_fastq_emit_grouped")
        edges = bounds.tolist()
        out = torch.zeros((max(edges[-1], 1),), dtype=torch.uint8)
        if edges[-1]:
            _check(self.dmx.emu_fastq_emit_grouped(*args, _ptr(out)), "emu_fastq_emit_grouped")
        return out[:edges[-1]], edges

    def demux_groups(self, dest, matched, last_which, adapter_group, n_adapters, untrimmed_group):
        n = dest.shape[0]
        group = torch.zeros((n,), dtype=torch.int32)
        _check(self.dmx.emu_demux_groups(_ptr(dest), _ptr(matched), _ptr(last_which), _ptr(adapter_group), int(n_adapters),
                                         int(untrimmed_group), C.c_int64(n), _ptr(group)), "emu_demux_groups")
        return group


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

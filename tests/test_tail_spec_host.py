"""The band sweeps of the run-time compiled DP tail (csrc/tail_filter.hpp) against the generic band_locate /
band_locate_last they replace, on the CPU (tests/emu/emu_tail_spec.cpp, the product's per-lane source under
ATR_HOST_EMU): random aligners, reads and window words, the records compared word for word -- and the same twin as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

from .conftest import ROOT

_SRC = os.path.join(ROOT, "tests", "emu", "emu_tail_spec.cpp")
_FLAGS = ["-std=c++17", "-DATR_HOST_EMU", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "atropos_amd", "csrc")]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_tail") / "libemu_tail_spec.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + _FLAGS + [_SRC, "-o", so])
    lib = C.CDLL(so)
    lib.emu_tail_spec_run.restype = C.c_longlong
    lib.emu_tail_spec_run.argtypes = [C.c_uint64, C.c_int, C.c_longlong, C.POINTER(C.c_longlong)]
    return lib


@pytest.mark.parametrize("seed", [1, 2])
def test_band_sweeps_equal_the_generic_ones(twin, seed):
    """2 x 30 aligners x 2 500 cases = 150 000 (aligner, read, window word) cases; the first aligner is C2's."""
    acc = C.c_longlong(0)
    bad = twin.emu_tail_spec_run(seed, 30, 2500, C.byref(acc))
    assert bad == 0, "%d cases differ" % bad
    assert acc.value > 10000, "too few cases with a match: %d" % acc.value


def test_standalone_under_sanitizers(tmp_path):
    prog = str(tmp_path / "emu_tail_spec")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DEMU_TAIL_MAIN"] + _FLAGS +
                          [_SRC, "-o", prog])
    run = subprocess.run([prog, "12", "1000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = run.stderr.decode("utf-8", "replace")
    assert run.returncode == 0, (run.stdout.decode()[-500:], err[-2000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-2000:]

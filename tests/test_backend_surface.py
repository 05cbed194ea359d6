"""The two backends' surfaces: what the product feature-detects on a backend, what the CPU test backend adds to the
shared wrappers (``_lib.AbiCalls``), the twins' prototypes, and the one mapping of error codes to exceptions."""
import inspect
import re

import pytest

from atropos_amd import _lib

from .emu import backend as emu
from .emu.backend import EmuBackend

# Every name the product (align/__init__.py, adapters.py, batch.py, shard.py) or bench.py looks for on a backend with
# hasattr / getattr, and whether the CPU test backend had it before the wrappers were shared: a name it grew would
# switch the code under test onto a device-only path.
PROBED = {
    "locate_one": False, "compare_one": False, "locate_pair_one": False, "multi_locate_one": False,
    "insert_match_one": False, "side_streams": False, "aligner_prepare": False, "locate_planes_applies": True,
    "locate_ascii_batch": False, "locate_ascii_planes_batch": False, "linked_group_applies": False,
    "stage_host_bytes": False, "worker_context": False, "last_unresolved": False,
}

# What EmuBackend defines itself, and why the shared wrapper does not serve.
OVERRIDES = {
    "empty": "plumbing AbiCalls asks of a backend: host tensors, zeroed (the twins rely on it)",
    "translate_table": "no atr_translate_table twin: the tables are read back from throw-away aligners",
    "locate_planes_applies": "the emulation takes every width of the envelope (emu_locate_planes_all_widths)",
    "insert_match_correct_batch": "no fused kernel to emulate: match, then correct",
    "gunzip_members": "test hook: counts the inflate calls, then the shared wrapper",
}


def test_probed_names():
    be = EmuBackend()
    assert {name: hasattr(be, name) for name in PROBED} == PROBED
    assert [name for name in PROBED if not hasattr(_lib.HipBackend, name)] == []
    assert not issubclass(EmuBackend, _lib.HipBackend)


def test_overrides_are_listed():
    own = {name for name, v in vars(EmuBackend).items() if callable(v) and not name.startswith("_")}
    assert own == set(OVERRIDES)
    shared = [name for name, v in vars(_lib.AbiCalls).items() if callable(v) and not name.startswith("_")]
    assert len(shared) >= 50
    for name in shared:
        if name not in OVERRIDES:
            assert getattr(EmuBackend, name) is getattr(_lib.AbiCalls, name), name


def test_twin_prototypes_are_the_abis():
    seen = set()
    for twin in emu.TWINS:
        lib, fns = emu.load_twin(twin)
        for name, (fn, at) in fns.items():
            res, args = _lib.PROTOTYPES[name]
            assert fn is getattr(lib, "emu_" + name[4:]) and fn.restype is res and fn.argtypes is args, name
            assert at == (args.index(_lib.STREAM) if _lib.STREAM in args else None), name
            assert name not in seen, name
            seen.add(name)
    # every entry point a shared wrapper calls has a twin somewhere, but for the one table the double reads back
    called = set(re.findall(r'"(atr_[a-z0-9_]+)"', inspect.getsource(_lib.AbiCalls)))
    assert len(called) > 70 and called <= set(_lib.PROTOTYPES)
    assert called - seen == {"atr_translate_table"}


def test_error_codes_through_the_shared_check(emu_backend):
    assert emu_backend._call.__func__ is EmuBackend._call and _lib._check(None, 3, "x") == 3
    with pytest.raises(_lib.AtroposUnsupported):                                           # -2
        emu_backend.aligner_create(b"A" * 129, 0.1, 14, False, False, 1, 1)
    with pytest.raises(ValueError):                                                        # -1
        emu_backend.aligner_create(b"ACGT", 0.1, 14, False, False, 0, 1)
    for rc, exc in ((-1, ValueError), (-2, _lib.AtroposUnsupported), (-4, MemoryError), (-3, _lib.AtroposHipError),
                    (-5, _lib.AtroposHipError), (-77, _lib.AtroposHipError)):
        with pytest.raises(exc) as info:
            _lib._check(None, rc, "atr_x")
        assert "atr_x" in str(info.value)
        assert (type(info.value) is _lib.AtroposHipError) == (rc in (-3, -5, -77))
    assert issubclass(_lib.AtroposUnsupported, _lib.AtroposHipError)


def test_stream_argument_forms():
    """What a direct caller of the library may pass where a prototype has STREAM: None, an integer, or what
    ``HipBackend._stream()`` returns (a STREAM).  The refusal asked for comes before any device work."""
    lib = _lib.load_library()
    assert isinstance(_lib.STREAM(0), _lib.C.c_void_p)
    assert inspect.getsource(_lib.HipBackend._stream).count("return STREAM(") == 1
    for stream in (None, 0, _lib.STREAM(0), _lib.STREAM(None)):
        assert lib.atr_clip_batch(None, None, None, 1, -1, 0, stream) == -1
        assert lib.atr_fastq_emit(None, None, None, None, None, None, None, 0, 1, 0, None, None, None, stream) == -1

"""CPU tier of the device gzip compressor (``gzip_blocks``, ``fastq.DeviceGzipSink``, ``device_gzip=True``): the cases
of tests/_gzip_common.py through the CPU twin of the kernels (tests/emu/emu_gzip.cpp, built from the product's
deflate_core.hpp), checked by independent decoders -- ``gzip.decompress``, ``zlib.decompress(member, 31)`` and, for
one written file, ``/usr/bin/gzip -t``."""
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch

from atropos_amd import _lib, fastq
from atropos_amd.trim import pipeline_from_args

from . import _gzip_common as G
from .emu.backend import EmuBackend


@pytest.fixture(scope="module")
def twin():
    return EmuBackend()


@pytest.fixture()
def gz_backend(twin):
    prev = _lib.set_backend(twin, _test_double=True)
    yield twin
    _lib.set_backend(prev, _test_double=True)


def test_fixture_conditions(twin):
    """What a fixture is named after is read from the parsed stream, not from how it was built.

    ``dist_limit`` (a distance code that the 15-bit limit binds) is not among them.  It needs about 4 200 matches
    whose distance symbols count like Fibonacci numbers, to within one match.  A generator that plants them one by
    one where the one-entry hash table still holds the source, and feeds the model's counts back into its targets,
    stayed at an unconstrained depth of 10 or 11 over 75 rounds: short runs and copies from near by match each other
    by chance a hundred times a block.  That path of ``gz_build_lengths`` is covered by ``test_build_lengths_fuzz``."""
    assert G.huffman_depth(G.CONTENTS["fibonacci"](G.BLOCK)) > 15          # an unconstrained code would be too deep
    block = G.CONTENTS["no_match"](G.BLOCK)
    assert len({block[i:i + 3] for i in range(len(block) - 2)}) == len(block) - 2 and len(set(block)) == 256
    quiet = G._quiet()
    assert len({quiet[i:i + 3] for i in range(len(quiet) - 2)}) == len(quiet) - 2
    G.fixture_conditions(twin)
    for kind in ("binned", "uniform"):
        assert (1 << 20) <= len(G.ratio_fixture(kind)) <= (5 << 18)


@pytest.mark.parametrize("content", sorted(G.CONTENTS))
def test_round_trip_and_structure(twin, content):
    for n in G.case_lengths(content):
        data = G.CONTENTS[content](n)
        assert len(data) == n
        stream, starts = G.compress(twin, data, offsets=True)
        members = G.check_stream(stream, data, starts, twin.gzip_bound(n))
        if content == "random":
            for (at, size, isize) in members:
                assert size <= isize + 31


@pytest.mark.parametrize("content", sorted(G.CONTENTS))
def test_tokens_and_codes(twin, content):
    """Every member of every case, read by the independent inflater: its tokens are those of the plain model of match
    and parse, its three codes are complete, monotone and -- where no limit binds -- optimal, its size is its bits."""
    worst = 0.0
    for n in G.case_lengths(content):
        for info in G.check_case(twin, content, n):
            worst = max([worst] + info["ratios"])
    if worst:
        print("%s: a limited code costs at most %.4f of the package-merge optimum" % (content, worst))


def _fuzz_histograms(rng, nmax, count):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for i in range(count):
        n = int(rng.integers(2, nmax + 1))
        kind = i % 6
        if kind == 0:
            f = fib[:min(n, 40)] + [fib[39]] * max(0, n - 40)
        elif kind == 1:
            f = [min(1 << min(k, 31), 0x7fffffff // nmax) for k in range(n)]
        elif kind == 2:
            f = [int(rng.integers(1, 100))] * n
        elif kind == 3:
            f = [1] * (n - 1) + [int(rng.integers(n, 1 << 20))]
        elif kind == 4:
            f = rng.integers(1, 1 << int(rng.integers(1, 20)), n).tolist()
        else:
            f = (rng.pareto(0.7, n) * 3 + 1).clip(1, 1 << 22).astype(int).tolist()
        yield sorted(int(v) for v in f)


@pytest.mark.parametrize("nmax,maxbits,count", [(19, 7, 3000), (286, 15, 1500)])
def test_build_lengths_fuzz(twin, nmax, maxbits, count):
    """``gz_build_lengths`` driven directly: the code properties over Fibonacci, geometric, all-equal, single-heavy,
    uniform and heavy-tailed histograms; the limit binds in many of them."""
    bound = worst = 0
    for freqs in _fuzz_histograms(np.random.default_rng(nmax), nmax, count):
        if sum(freqs) >= 1 << 32:
            continue
        lengths = G.twin_build_lengths(freqs, maxbits)
        ratio = G.check_code(freqs, lengths, maxbits, "fuzz %r" % (freqs[:8],))
        if ratio is not None:
            bound += 1
            worst = max(worst, ratio)
    print("limit %d bound in %d histograms; worst cost / package-merge optimum %.4f" % (maxbits, bound, worst))
    assert bound >= count // 20


def test_deterministic_and_concatenation(twin):
    a = G.CONTENTS["synth_fastq"](2 * G.BLOCK)
    b = G.ratio_fixture("binned")[:G.BLOCK + 4321]
    za, zb = G.compress(twin, a), G.compress(twin, b)
    assert za == G.compress(twin, a)
    assert za + zb == G.compress(twin, a + b)


def test_abi_errors(twin):
    """The refusals come before any pointer is looked at."""
    bound, work_bytes = twin._symbol("atr_gzip_bound"), twin._symbol("atr_gzip_work_bytes")
    blocks = lambda *a: twin._symbol("atr_gzip_blocks")(*(a + (None,)))         # (the stream)
    assert bound(-1) == -1 and work_bytes(-1) == 0
    assert bound(0) == 0 and bound(G.BLOCK + 1) == G.BLOCK + 1 + 2 * 31
    assert blocks(None, -1, None, 0, None, None, None) == -1
    assert blocks(None, 100, None, bound(100) - 1, None, None, None) == -1
    assert blocks(None, 100, None, -5, None, None, None) == -1
    assert blocks(None, 1 << 32, None, bound(1 << 32), None, None, None) == -2
    assert blocks(None, 100, None, bound(100), None, None, None) == -1
    buf = (16 * b"\xaa" + 12 * b"\xaa")
    raw = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    assert twin._symbol("atr_gzip_eof")(raw.data_ptr()) == 28
    assert bytes(raw.numpy().tobytes()) == G.EOF == _lib.GZIP_EOF
    assert gzip.decompress(G.EOF) == b""


@pytest.mark.parametrize("kind", ["binned", "uniform"])
def test_ratio(twin, kind):
    """LZ77 and the per-block code pay for themselves: no larger than Huffman-only coding of the same blocks."""
    data = G.ratio_fixture(kind)
    stream = G.compress(twin, data)
    G.check_stream(stream, data)
    cap = G.huffman_only_cap(data)
    print("%s: %d bytes -> %d (Z_HUFFMAN_ONLY + framing: %d)" % (kind, len(data), len(stream), cap))
    assert len(stream) <= cap


# ---------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("args,every", [("-a %s -m 30" % G.TRUSEQ, 3), ("-a %s -m 30 -y _longer_names_make_two_members_a_chunk" % G.TRUSEQ, 25)])
def test_trim_file(gz_backend, tmp_path, args, every):
    src = tmp_path / "in.fastq"
    src.write_bytes(G.fastq_input(every=every))
    plain = pipeline_from_args(args).trim_file(str(src), str(tmp_path / "out.fastq"), chunk_bytes=1 << 16)
    pipe = pipeline_from_args(args)
    got = pipe.trim_file(str(src), str(tmp_path / "out.fastq.gz"), chunk_bytes=1 << 16, device_gzip=True)
    assert got == plain and plain["keep"] > 300
    raw = (tmp_path / "out.fastq.gz").read_bytes()
    assert gzip.decompress(raw) == (tmp_path / "out.fastq").read_bytes()
    members = G.parse_members(raw)
    assert raw.endswith(G.EOF) and len(members) >= 5
    if every == 25:                                                        # chunks of more than one member
        assert sum(1 for m in members if m[2] == G.BLOCK) >= 2
    if os.path.exists("/usr/bin/gzip"):
        subprocess.check_call(["/usr/bin/gzip", "-t", str(tmp_path / "out.fastq.gz")])
    # the default path is untouched: a host-compressed file, no BGZF framing
    pipeline_from_args(args).trim_file(str(src), str(tmp_path / "host.fastq.gz"), chunk_bytes=1 << 16)
    host = (tmp_path / "host.fastq.gz").read_bytes()
    assert gzip.decompress(host) == (tmp_path / "out.fastq").read_bytes() and host[3] != 4


def test_trim_files_paired(gz_backend, tmp_path):
    G.check_paired(tmp_path)


def test_empty_outputs(gz_backend, tmp_path):
    """No record in, or no read kept: the file is the 28-byte end-of-file member."""
    (tmp_path / "empty.fastq").write_bytes(b"")
    pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(str(tmp_path / "empty.fastq"), str(tmp_path / "a.fastq.gz"), device_gzip=True)
    assert (tmp_path / "a.fastq.gz").read_bytes() == G.EOF
    (tmp_path / "in.fastq").write_bytes(G.fastq_input(nrec=40))
    counts = pipeline_from_args("-a %s -m 500" % G.TRUSEQ).trim_file(str(tmp_path / "in.fastq"), str(tmp_path / "b.fastq.gz"),
                                                                     device_gzip=True)
    assert counts["keep"] == 0
    raw = (tmp_path / "b.fastq.gz").read_bytes()
    assert raw == G.EOF and gzip.decompress(raw) == b""


def test_refusals(gz_backend, tmp_path):
    (tmp_path / "in.fastq").write_bytes(G.fastq_input(nrec=40))
    src = str(tmp_path / "in.fastq")
    for bad in ("out.fastq", "out.fastq.bz2", "out.fastq.xz"):
        with pytest.raises(ValueError):
            fastq.make_sink(str(tmp_path / bad), 1, 1 << 20, gz_backend, device_gzip=True)
        with pytest.raises(ValueError):
            pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(src, str(tmp_path / bad), device_gzip=True)
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a x=%s" % G.TRUSEQ).trim_file(src, str(tmp_path / "o.{name}.fastq.gz"), device_gzip=True)
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(src, str(tmp_path / "p.fastq.gz"), output_parts=2, device_gzip=True)
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a %s -A %s" % (G.TRUSEQ, G.TRUSEQ), paired_input=True).trim_files(
            src, src, str(tmp_path / "q1.fastq.gz"), str(tmp_path / "q2.fastq.gz"), output_parts=2, device_gzip=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.fastq"]
    # without the flag every call is as before
    assert isinstance(fastq.make_sink(str(tmp_path / "h.fastq.gz"), 1, 1 << 20, gz_backend), fastq.CompressedSink)
    sink = fastq.make_sink(str(tmp_path / "d.fastq.gz"), 1, 1 << 20, gz_backend, device_gzip=True)
    assert isinstance(sink, fastq.DeviceGzipSink)
    sink.close()
    assert (tmp_path / "d.fastq.gz").read_bytes() == G.EOF


def test_sink_chunks(gz_backend, tmp_path):
    """``DeviceGzipSink`` driven directly: chunks of any size, an empty one in between, staging buffers smaller than
    a chunk's compressed text."""
    data = G.CONTENTS["random"](3 * G.BLOCK + 5) + G.ratio_fixture("uniform")[:200000]
    sink = fastq.DeviceGzipSink(str(tmp_path / "s.gz"), 1 << 16, gz_backend)
    cuts = [0, 70000, 70000, 70001, 3 * G.BLOCK + 5, len(data)]
    for lo, hi in zip(cuts, cuts[1:]):
        sink.write(torch.frombuffer(bytearray(data[lo:hi]), dtype=torch.uint8) if hi > lo else torch.zeros((0,), dtype=torch.uint8))
    sink.close()
    raw = (tmp_path / "s.gz").read_bytes()
    assert gzip.decompress(raw) == data and raw.endswith(G.EOF)

"""GPU tier of the device gzip compressor: the cases of tests/_gzip_common.py (the ones test_gzip_host.py runs on the
CPU twin) through the gfx950 kernels -- ``HipBackend.gzip_blocks``, ``fastq.DeviceGzipSink`` and ``device_gzip=True``
of the file drivers -- checked by ``gzip.decompress``, ``zlib.decompress(member, 31)`` and, token by token, by the
independent inflater and the plain model of tests/_deflate_ref.py; then the launch: more members than workgroups and
than threads of the scan, members of unlike size, text at odd addresses."""
import gzip

import numpy as np
import pytest
import torch

from atropos_amd import _lib, fastq
from atropos_amd.trim import pipeline_from_args

from . import _gzip_common as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("content", sorted(G.CONTENTS))
def test_round_trip_and_structure(hip_backend, content):
    for n in G.case_lengths(content):
        data = G.CONTENTS[content](n)
        stream, starts = G.compress(hip_backend, data, offsets=True)
        members = G.check_stream(stream, data, starts, hip_backend.gzip_bound(n))
        if content == "random":
            for (at, size, isize) in members:
                assert size <= isize + 31


@pytest.mark.parametrize("content", sorted(G.CONTENTS))
def test_tokens_and_codes(hip_backend, content):
    """Every member of every case, read by the independent inflater: its tokens are those of the plain model of match
    and parse -- a lost integer max, a table read before the tile before it was entered, a wrong cut at a segment's end
    show here --, its codes are complete, monotone and optimal where no limit binds, its size is its bits."""
    for n in G.case_lengths(content):
        G.check_case(hip_backend, content, n)


def test_fixture_conditions(hip_backend):
    G.fixture_conditions(hip_backend)


def _alone(backend, cache, block):
    if block not in cache:
        cache[block] = G.compress(backend, block)
    return cache[block]


@pytest.mark.parametrize("nblocks,tail", [(513, 5), (1025, 129)])
def test_members_are_independent(hip_backend, nblocks, tail):
    """A workgroup encodes blocks b, b + 512, ... with one LDS and one match array: after a full block rich in matches
    come a stored block, a block without a match and a short one, and every member is, byte for byte, what its block
    gives alone."""
    rich = [G.CONTENTS[c](G.BLOCK) for c in ("one_byte", "every_symbol", "fibonacci")]
    poor = [G.CONTENTS["random"](G.BLOCK), G.CONTENTS["no_match"](G.BLOCK), G._quiet()[:G.BLOCK]]
    blocks = [rich[k % 3] if k < 512 else poor[k % 3] for k in range(nblocks - 1)] + [G._quiet()[:tail]]
    stream, starts = G.compress(hip_backend, b"".join(blocks), offsets=True)
    assert len(starts) == nblocks + 1 and starts[-1] == len(stream)
    cache = {}
    for k, block in enumerate(blocks):
        assert stream[starts[k]:starts[k + 1]] == _alone(hip_backend, cache, block), "member %d" % k
    for block, member in cache.items():
        G.check_member(member, block, model=False)
    assert sum(1 for b in blocks[512:] if len(_alone(hip_backend, cache, b)) == len(b) + 31) >= (nblocks - 513) // 3


@pytest.mark.parametrize("nblocks", [1024, 1025, 2049])
def test_scan_beyond_1024_members(hip_backend, nblocks):
    """The scan gives a thread several members once there are more than 1024; the members differ in size."""
    rnd = np.frombuffer(G.CONTENTS["random"](6000), dtype=np.uint8)
    text = np.full((nblocks, G.BLOCK), ord("F"), dtype=np.uint8)
    for k in range(7):
        text[k::7, :k * 1000] = rnd[:k * 1000]
    text[:, -1] = np.arange(nblocks) % 251                                 # (no two blocks alike)
    data = text.tobytes()[:(nblocks - 1) * G.BLOCK + 777]
    stream, starts = G.compress(hip_backend, data, offsets=True)
    members = G.check_stream(stream, data, starts, hip_backend.gzip_bound(len(data)))
    assert len(members) == nblocks and starts[-1] == len(stream)
    assert len({size for _, size, _ in members}) >= 7


def test_text_alignment(hip_backend):
    """Text at 1, 2 and 3 bytes past an allocation, of lengths 4k + r for every r around one and two blocks (the last,
    partial word of the byte-wise load), on two streams in turn: the bytes are those of the aligned text."""
    base = G.CONTENTS["synth_fastq"](2 * G.BLOCK + 8)
    lengths = [G.BLOCK + d for d in range(-3, 4)] + [2 * G.BLOCK + d for d in range(-3, 4)]
    assert {n % 4 for n in lengths} == {0, 1, 2, 3}
    dev = torch.frombuffer(bytearray(b"xyz" + base), dtype=torch.uint8).to(hip_backend.device)
    streams = [torch.cuda.Stream(device=hip_backend.device) for _ in range(2)]
    expect = {}
    for i, (off, n) in enumerate((off, n) for off in (1, 2, 3) for n in lengths):
        data = (b"xyz" + base)[off:off + n]
        if data not in expect:
            expect[data] = G.compress(hip_backend, data)                   # (from an allocation of its own: aligned)
            G.check_stream(expect[data], data)
        streams[i % 2].wait_stream(torch.cuda.current_stream(hip_backend.device))
        with torch.cuda.stream(streams[i % 2]):
            view = dev[off:off + n]
            assert view.data_ptr() % 4 == (dev.data_ptr() + off) % 4 != 0
            out, total = hip_backend.gzip_blocks(view)
            got = bytes(out[:total].cpu().numpy().tobytes())
        assert got == expect[data], (off, n)


def test_deterministic_and_concatenation(hip_backend):
    a = G.CONTENTS["synth_fastq"](2 * G.BLOCK)
    b = G.ratio_fixture("binned")[:G.BLOCK + 4321]
    za, zb = G.compress(hip_backend, a), G.compress(hip_backend, b)
    assert za == G.compress(hip_backend, a)
    with torch.cuda.stream(torch.cuda.Stream(device=hip_backend.device)):
        assert za == G.compress(hip_backend, a)                            # a second stream
    assert za + zb == G.compress(hip_backend, a + b)


def test_many_blocks_and_unaligned_text(hip_backend):
    """More blocks than workgroups of a launch (every workgroup takes several), and text that starts at an odd
    address."""
    data = G.ratio_fixture("uniform")
    data = (data * (600 * G.BLOCK // len(data) + 1))[:600 * G.BLOCK + 3]
    G.check_stream(G.compress(hip_backend, data), data)
    dev = torch.frombuffer(bytearray(b"x" + data[:3 * G.BLOCK]), dtype=torch.uint8).to(hip_backend.device)
    out, total = hip_backend.gzip_blocks(dev[1:])
    assert gzip.decompress(bytes(out[:total].cpu().numpy().tobytes())) == data[:3 * G.BLOCK]


def test_abi_errors(hip_backend):
    """The refusals come before any pointer is looked at."""
    lib = hip_backend.lib
    assert lib.atr_gzip_bound(-1) == -1 and lib.atr_gzip_work_bytes(-1) == 0
    assert lib.atr_gzip_bound(0) == 0 and lib.atr_gzip_bound(G.BLOCK + 1) == G.BLOCK + 1 + 2 * 31
    assert lib.atr_gzip_blocks(None, -1, None, 0, None, None, None, None) == -1
    assert lib.atr_gzip_blocks(None, 100, None, lib.atr_gzip_bound(100) - 1, None, None, None, None) == -1
    assert lib.atr_gzip_blocks(None, 100, None, -5, None, None, None, None) == -1
    assert lib.atr_gzip_blocks(None, 1 << 32, None, lib.atr_gzip_bound(1 << 32), None, None, None, None) == -2
    assert lib.atr_gzip_blocks(None, 100, None, lib.atr_gzip_bound(100), None, None, None, None) == -1
    raw = torch.zeros((28,), dtype=torch.uint8)
    assert lib.atr_gzip_eof(raw.data_ptr()) == 28
    assert bytes(raw.numpy().tobytes()) == G.EOF == _lib.GZIP_EOF


@pytest.mark.parametrize("kind", ["binned", "uniform"])
def test_ratio(hip_backend, kind):
    """LZ77 and the per-block code pay for themselves: no larger than Huffman-only coding of the same blocks."""
    data = G.ratio_fixture(kind)
    stream = G.compress(hip_backend, data)
    G.check_stream(stream, data)
    cap = G.huffman_only_cap(data)
    print("%s: %d bytes -> %d (Z_HUFFMAN_ONLY + framing: %d)" % (kind, len(data), len(stream), cap))
    assert len(stream) <= cap


def test_same_bytes_as_the_twin(hip_backend):
    """The kernels and their CPU twin run one source (deflate_core.hpp): the streams are identical."""
    from .emu.backend import EmuBackend
    twin = EmuBackend()
    inputs = [G.ratio_fixture("binned")[:3 * G.BLOCK + 99], G.CONTENTS["fibonacci"](G.BLOCK + 5), G.CONTENTS["random"](700)]
    for content, edge in (("cl_limit", 511), ("every_symbol", 16385), ("segment_cut", 4097), ("tail_match", 513),
                          ("tail_match_far", 20480), ("window_edge", 32769 + 600)):
        inputs += [G.CONTENTS[content](G.BLOCK), G.CONTENTS[content](edge)]
    for data in inputs:
        assert G.compress(hip_backend, data) == G.compress(twin, data)


# ---------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("args,every", [("-a %s -m 30" % G.TRUSEQ, 3), ("-a %s -m 30 -y _longer_names_make_two_members_a_chunk" % G.TRUSEQ, 25)])
def test_trim_file(hip_backend, tmp_path, args, every):
    src = tmp_path / "in.fastq"
    src.write_bytes(G.fastq_input(every=every))
    plain = pipeline_from_args(args).trim_file(str(src), str(tmp_path / "out.fastq"), chunk_bytes=1 << 16)
    got = pipeline_from_args(args).trim_file(str(src), str(tmp_path / "out.fastq.gz"), chunk_bytes=1 << 16, device_gzip=True)
    assert got == plain and plain["keep"] > 300
    raw = (tmp_path / "out.fastq.gz").read_bytes()
    assert gzip.decompress(raw) == (tmp_path / "out.fastq").read_bytes()
    members = G.parse_members(raw)
    assert raw.endswith(G.EOF) and len(members) >= 5
    if every == 25:                                                        # chunks of more than one member
        assert sum(1 for m in members if m[2] == G.BLOCK) >= 2


def test_trim_files_paired(hip_backend, tmp_path):
    G.check_paired(tmp_path)


def test_empty_outputs(hip_backend, tmp_path):
    (tmp_path / "empty.fastq").write_bytes(b"")
    pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(str(tmp_path / "empty.fastq"), str(tmp_path / "a.fastq.gz"), device_gzip=True)
    assert (tmp_path / "a.fastq.gz").read_bytes() == G.EOF
    (tmp_path / "in.fastq").write_bytes(G.fastq_input(nrec=40))
    counts = pipeline_from_args("-a %s -m 500" % G.TRUSEQ).trim_file(str(tmp_path / "in.fastq"), str(tmp_path / "b.fastq.gz"),
                                                                     device_gzip=True)
    raw = (tmp_path / "b.fastq.gz").read_bytes()
    assert counts["keep"] == 0 and raw == G.EOF and gzip.decompress(raw) == b""


def test_refusals(hip_backend, tmp_path):
    (tmp_path / "in.fastq").write_bytes(G.fastq_input(nrec=40))
    src = str(tmp_path / "in.fastq")
    for bad in ("out.fastq", "out.fastq.bz2", "out.fastq.xz"):
        with pytest.raises(ValueError):
            fastq.make_sink(str(tmp_path / bad), 1, 1 << 20, hip_backend, device_gzip=True)
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a x=%s" % G.TRUSEQ).trim_file(src, str(tmp_path / "o.{name}.fastq.gz"), device_gzip=True)
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a %s" % G.TRUSEQ).trim_file(src, str(tmp_path / "p.fastq.gz"), output_parts=2, device_gzip=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.fastq"]

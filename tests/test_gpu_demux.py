"""GPU tier of demultiplexing: the golden cases of tests/golden/trim_demux.json.gz on the device, and the grouped
formatter (atr_fastq_emit_grouped) against a path that exists without it and has tests of its own: for every
group g, ``fastq_emit`` with a uint8 destination array that marks the records of g.  Every segment equals that
text byte for byte and the segment boundaries equal the lengths."""
import numpy as np
import pytest
import torch

from atropos_amd import _lib
from atropos_amd.fastq import FastqBatch

from . import _demux_common as D

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
GROUPS = (1, 2, 3, 63, 64, 65, 1024)


@pytest.mark.parametrize("index", range(len(D.golden())), ids=D.case_ids())
def test_golden(hip_backend, tmp_path, index):
    D.check_case(D.golden()[index], tmp_path)


def test_golden_chunked(hip_backend, tmp_path):
    D.check_case(D.golden()[0], tmp_path, chunk_bytes=1 << 16)


# ---------------------------------------------------------------------------------------------- the grouped formatter
_BATCHES = {}


def records(n, zero=False):
    """n records of 0 to 80 bases (``zero``: none at all), every eighth with the name repeated on the '+' line; with a
    kept interval and an unmasked interval inside it per record.  Made once per size, never written to."""
    key = (n, zero)
    if key not in _BATCHES:
        rng = np.random.RandomState(1000 + n + (7 if zero else 0))
        lens = np.zeros(n, dtype=np.int64) if zero else rng.randint(0, 81, size=n)
        if not zero and n > 2:
            lens[1] = 0
        text = []
        for i, k in enumerate(lens):
            name = "r%d len=%d" % (i, k)
            seq = "".join("ACGT"[v] for v in rng.randint(0, 4, size=k))
            qual = "".join(chr(33 + v) for v in rng.randint(2, 41, size=k))
            text.append("@%s\n%s\n+%s\n%s\n" % (name, seq, name if i % 8 == 3 else "", qual))
        batch, _ = FastqBatch.from_bytes("".join(text).encode(), final=True)
        begin = np.array([rng.randint(0, k + 1) for k in lens], dtype=np.int32)
        end = np.array([rng.randint(b, k + 1) for b, k in zip(begin, lens)], dtype=np.int32)
        ub = np.array([rng.randint(b, e + 1) for b, e in zip(begin, end)], dtype=np.int32)
        ue = np.array([rng.randint(u, e + 1) for u, e in zip(ub, end)], dtype=np.int32)
        dev = batch.records.device
        _BATCHES[key] = (batch,) + tuple(torch.from_numpy(a).to(dev) for a in (begin, end, ub, ue))
    return _BATCHES[key]


def pattern(kind, n, G):
    r = np.arange(n)
    rng = np.random.RandomState(n * 2000 + G)
    if kind == "one":                                          # all records in one group
        return np.full(n, G - 1)
    if kind == "alternating":                                  # neighbours in a wave never share a group (G > 1)
        return r % G
    if kind == "runs64":                                       # group boundaries on wave boundaries
        return (r // 64) % G
    if kind == "runs256":                                      # ... and on block boundaries
        return (r // 256) % G
    if kind == "gaps":                                         # no record in the first, the middle and the last group
        allowed = [g for g in range(G) if g not in (0, G // 2, G - 1)] or [min(1, G - 1)]
        return np.asarray(allowed)[rng.randint(0, len(allowed), size=n)]
    if kind == "minus":                                        # records that are not written, mixed in
        g = rng.randint(0, G, size=n)
        g[rng.rand(n) < 0.3] = -1
        return g
    if kind == "none":                                         # nothing is written
        return np.full(n, -1)
    return rng.randint(0, G, size=n)                           # "random", "zero", "masked"


def check(be, n, G, kind):
    batch, begin, end, ub, ue = records(n, zero=(kind == "zero"))
    if kind != "masked":
        ub = ue = None
    codes = pattern(kind, n, G)
    group = torch.from_numpy(codes.astype(np.int32)).to(begin.device)
    text, edges = be.fastq_emit_grouped(batch.data, batch.records, begin, end, ub, ue, group, G)
    assert len(edges) == G + 1 and edges[0] == 0 and edges[-1] == text.numel()
    host = text.cpu().numpy().tobytes()
    present = set(int(g) for g in np.unique(codes) if g >= 0)
    for g in range(G):
        if g not in present:
            assert edges[g + 1] == edges[g], (n, G, kind, g)
            continue
        dest = (group == g).to(torch.uint8)
        one = be.fastq_emit(batch.data, batch.records, begin, end, ub, ue, dest, 1).cpu().numpy().tobytes()
        assert edges[g + 1] - edges[g] == len(one), (n, G, kind, g)
        assert host[edges[g]:edges[g + 1]] == one, (n, G, kind, g)


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("kind", ["one", "alternating", "runs64", "runs256", "gaps", "minus", "none", "zero", "masked"])
def test_grouped_equals_one_emit_per_group(hip_backend, kind, G):
    for n in SIZES:
        check(hip_backend, n, G, kind)


def test_out_of_range_codes_are_not_written(hip_backend):
    batch, begin, end, _, _ = records(257)
    codes = np.arange(257) % 5 - 1                             # -1 .. 3 with G = 3: -1 and 3 are outside
    group = torch.from_numpy(codes.astype(np.int32)).to(begin.device)
    text, edges = hip_backend.fastq_emit_grouped(batch.data, batch.records, begin, end, None, None, group, 3)
    inside = torch.from_numpy(np.where(codes >= 3, -1, codes).astype(np.int32)).to(begin.device)
    text2, edges2 = hip_backend.fastq_emit_grouped(batch.data, batch.records, begin, end, None, None, inside, 3)
    assert edges == edges2 and torch.equal(text, text2)


def test_no_records(hip_backend):
    batch, _ = FastqBatch.from_bytes(b"", final=True)
    empty = torch.zeros((0,), dtype=torch.int32, device=batch.records.device)
    text, edges = hip_backend.fastq_emit_grouped(batch.data, batch.records, empty, empty, None, None, empty, 4)
    assert text.numel() == 0 and edges == [0] * 5


def test_group_bound(hip_backend):
    batch, begin, end, _, _ = records(64)
    group = torch.zeros((64,), dtype=torch.int32, device=begin.device)
    with pytest.raises(_lib.AtroposUnsupported):
        hip_backend.fastq_emit_grouped(batch.data, batch.records, begin, end, None, None, group, 1025)
    lib = hip_backend.lib
    assert lib.atr_fastq_emit_grouped_work_bytes(64, 1025) == 0 and lib.atr_fastq_emit_grouped_work_bytes(64, 1024) > 0
    assert lib.atr_fastq_emit_grouped(None, None, None, None, None, None, None, 1025, 64, 0, None, None, None, None,
                                      None) == -2               # ATR_ERR_UNSUPPORTED, before any pointer is looked at
    assert lib.atr_fastq_emit_grouped(None, None, None, None, None, None, None, 0, 64, 0, None, None, None, None,
                                      None) == -1


def test_group_codes(hip_backend):
    """atr_demux_groups against the rule, every destination x matched x adapter."""
    dest = np.repeat(np.arange(6), 8).astype(np.uint8)
    matched = np.tile(np.repeat([0, 1], 4), 6).astype(np.uint8)
    which = np.tile(np.arange(4), 12).astype(np.int64)
    table = np.array([2, 0, 0, 1], dtype=np.int32)
    dev = hip_backend.device
    for untrimmed in (3, -1):
        exp = np.full(48, -1, dtype=np.int32)
        keep = dest == _lib.DEST_KEEP
        exp[keep & (matched == 1)] = table[which[keep & (matched == 1)]]
        exp[(keep & (matched == 0)) | (dest == _lib.DEST_UNTRIMMED)] = untrimmed
        got = hip_backend.demux_groups(torch.from_numpy(dest).to(dev), torch.from_numpy(matched).to(dev),
                                       torch.from_numpy(which).to(dev), torch.from_numpy(table).to(dev), 4, untrimmed)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), exp)

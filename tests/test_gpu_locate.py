"""GPU parity tests proper: the HIP kernels, called through the C ABI, against the
oracle and the committed golden vectors.  Bit-exact (integer work)."""
import numpy as np
import pytest
import torch

from . import _cases
from .conftest import load_golden, tup

pytestmark = pytest.mark.gpu


def test_native_library_is_loaded(hip_backend):
    import ctypes  # noqa: F401
    from atropos_amd import _lib
    assert hip_backend.name == "hip" and hip_backend.device.type == "cuda"
    with open("/proc/self/maps") as fh:
        assert "libatropos_hip.so" in fh.read()
    assert "MI355" in torch.cuda.get_device_name(0) or "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    assert _lib.get_backend() is hip_backend


def test_calls_on_a_worker_stream_equal_the_default_stream(hip_backend):
    """pack_reads + locate_batch inside ``worker_context()`` (a stream of its own) give the records of the same calls
    on the default stream: 130 reads of 40 bases, three tiles with a ragged last one, every path that takes them."""
    from atropos_amd import synth
    be = hip_backend
    reads = synth.single_end(0, 130, 40, synth.TRUSEQ_34, synth.SEEDS["C2"], device=be.device)
    h = be.aligner_create(synth.TRUSEQ_34.encode(), 0.1, 14, False, False, 3, 1)
    table = be.aligner_query_table(h)[1]

    def records(path):
        packed = be.pack_reads(reads, None, 40, table)
        return be.locate_batch(h, packed, None, 130, 40, path=path)
    try:
        for path in ("auto", "full", "filtered", "wave"):
            want = records(path).cpu()
            with be.worker_context() as stream:
                assert torch.cuda.current_stream(be.device) == stream != torch.cuda.default_stream(be.device)
                got = records(path)
            assert torch.equal(got.cpu(), want), path
            assert int((want[:, 1] >= 0).sum()) > 10
    finally:
        be.aligner_destroy(h)


def test_golden_locate(hip_backend):
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    checked, unsupported = _cases.check_golden_locate(Aligner, _lib.AtroposHipError)
    assert checked > 6000 and unsupported < 200


def test_batches_all_flags(hip_backend, oracle):
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    assert _cases.check_batches_against_oracle(Aligner, oracle, _lib.AtroposHipError, 23, 300) > 20000


def test_filtered_pipeline(hip_backend, oracle):
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    assert _cases.check_filtered_pipeline(Aligner, oracle, _lib.AtroposHipError, 41, 600) > 50000


def test_filtered_pipeline_narrow(hip_backend, oracle):
    """33..40-base adapters without START_WITHIN_SEQ1: the pre-pass sweeps 32 rows only
    (filter_core.hpp, NARROW mode)."""
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    assert _cases.check_filtered_pipeline(Aligner, oracle, _lib.AtroposHipError, 43, 300, (33, 40), (14, 10, 6, 14)) > 30000


def test_piece_pipeline(hip_backend, oracle):
    """atr_locate_planes_batch (two-pass pre-pass on plane64 reads) == full sweep == filtered pipeline == oracle."""
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    total, refused = _cases.check_piece_pipeline(Aligner, oracle, _lib.AtroposHipError, 23, 150, 300,
                                                 lengths=(70, 100, 128, 150, 150, 160, 180, 200, 224, 250, 260, 288, 300))
    assert total > 20000 and refused < 80


def test_piece_pipeline_long_adapters(hip_backend, oracle):
    """Round 6: adapters of 41 .. 64 bases through the two-pass pre-pass (generic kernels: 64- and 96-column windows) ==
    full sweep == one-pass pipeline == oracle; and the reference README's 64-mer on a 1 M-read batch."""
    from atropos_amd import _lib, synth
    from atropos_amd.align import Aligner
    total, refused = _cases.check_piece_pipeline(Aligner, oracle, _lib.AtroposHipError, 29, 120, 300,
                                                 lengths=(70, 100, 128, 150, 150, 160, 180, 200, 224, 250, 260, 288, 300),
                                                 mrange=(41, 64))
    assert total > 15000 and refused < 60
    n = 1_000_000
    reads = synth.single_end(0, n, 150, synth.PE_ADAPTER1, 0xA72050007, "cuda")
    for e in (0.1, 0.08):
        al = Aligner(synth.PE_ADAPTER1, e, 14, False, False, 3, 1)
        planes = al.pack(reads, layout="auto")
        assert planes.layout == "plane64"                     # (the envelope takes the 64-mer)
        rec = al.locate_batch(planes).records
        tiles = al.pack(reads, layout="tile64")
        assert torch.equal(rec, al.locate_batch(tiles, path="filtered").records)
        assert torch.equal(rec, al.locate_batch(tiles, filtered=False).records)
        sl = reads[:100_000].cpu().numpy()
        exp = oracle.locate_many(synth.PE_ADAPTER1, sl, np.full(len(sl), 150, np.int32), e, 14, False, False, 3, 1, _cases.oracle_threads())
        assert np.array_equal(rec[:100_000, :6].cpu().numpy().astype(np.int32), exp)
        assert 0.4 < float((rec[:, 1] >= 0).float().mean().item()) < 0.7


def test_piece_pipeline_start_within_seq1(hip_backend, oracle):
    """Round 6: flags 11 / 15 (-g / -b adapters) through the two-pass pre-pass == full sweep == one-pass pipeline == oracle,
    and a 1 M-read batch with the adapter at the read START (5' adapter, partial at the start, with errors, absent)."""
    from atropos_amd import _lib, synth
    from atropos_amd.align import Aligner
    total, refused = _cases.check_piece_pipeline(Aligner, oracle, _lib.AtroposHipError, 31, 120, 300,
                                                 lengths=(70, 100, 128, 150, 150, 160, 180, 200, 224, 250, 260, 288, 300),
                                                 mrange=(20, 64), flag_choices=(11, 15, 11, 15))
    assert total > 12000 and refused < 70
    n = 1_000_000
    adapter = synth.TRUSEQ_34[:28]
    back = synth.single_end(0, n, 150, adapter, 0xA72050008, "cuda")
    reads = torch.flip(back, dims=[1])                                  # the adapter (reversed) now sits at the read START
    radapter = adapter[::-1]
    for flags in (11, 15):
        al = Aligner(radapter, 0.1, flags, False, False, 3, 1)
        planes = al.pack(reads, layout="auto")
        assert planes.layout == "plane64"
        rec = al.locate_batch(planes).records
        tiles = al.pack(reads, layout="tile64")
        assert torch.equal(rec, al.locate_batch(tiles, filtered=False).records)
        sl = reads[:60_000].cpu().numpy()
        exp = oracle.locate_many(radapter, sl, np.full(len(sl), 150, np.int32), 0.1, flags, False, False, 3, 1, _cases.oracle_threads())
        assert np.array_equal(rec[:60_000, :6].cpu().numpy().astype(np.int32), exp)
        assert 0.3 < float((rec[:, 1] >= 0).float().mean().item()) < 0.8


def test_long_reads(hip_backend, oracle):
    """Reads of 737 .. 32 736 bases (the reference has no length limit): locate_long_kernel's rolling origin base
    against the reference's own answers (long_reads.json.gz) and the oracle; long and short reads in one list."""
    import random
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    assert _cases.check_golden_long_reads(Aligner, _lib.AtroposHipError) > 600
    assert _cases.check_golden_long_reads(Aligner, _lib.AtroposHipError, batch=False) > 600
    assert _cases.check_long_reads(Aligner, oracle, _lib.AtroposHipError, 31, 60) > 1200
    rng = random.Random(3)
    ref = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"
    for flags in (14, 10, 15):
        al = Aligner(ref, 0.1, flags, False, False, 3, 1)
        reads = [_cases.rseq(rng, _lib.MAX_LONG_READ_LEN - 34) + ref, _cases.rseq(rng, 32000) + ref + _cases.rseq(rng, 702),
                 _cases.rseq(rng, 20000), ref + _cases.rseq(rng, 9000)]
        reads += [(_cases.rseq(rng, rng.randint(0, 9000)) + _cases.mutate(rng, ref, 0.05) + _cases.rseq(rng, 9000))[:rng.randint(737, 9000)]
                  for _ in range(70)]
        got = al.locate_batch(reads).tuples()
        for q, g in zip(reads, got):
            assert g == oracle.locate(ref, q, 0.1, flags, False, False, 3, 1), (flags, len(q), g)
    with pytest.raises(Exception):
        Aligner(ref, 0.1, 14, False, False, 3, 1).locate_batch(["A" * (_lib.MAX_LONG_READ_LEN + 1)])


def test_long_pairs(hip_backend, oracle):
    """atr_locate_pairs_long_batch (sides of 321 .. 1 500 bases, 64-bit cells) and Aligner with a long reference: the
    reference's own answers (long_pairs.json.gz) and the oracle."""
    from atropos_amd import _lib
    from atropos_amd.align import Aligner, PairAligner
    assert _cases.check_golden_long_pairs(Aligner, PairAligner, _lib.AtroposHipError) == 400
    assert _cases.check_long_pairs(Aligner, PairAligner, oracle, 41, 60) > 600


def test_uniform_partial_overlaps(hip_backend, oracle):
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    assert _cases.check_uniform_partial_overlaps(Aligner, oracle, _lib.AtroposHipError, 17, 120) > 40000


def test_every_column_size(hip_backend, oracle):
    """One batch per register-column size (m = 1..128), indel and no-indel kernels,
    equality and wildcard compare modes."""
    import random
    from atropos_amd.align import Aligner
    rng = random.Random(99)
    for m in range(1, 129):
        ref = _cases.rseq(rng, m)
        for ic, wr in ((1, False), (100000, False), (1, True), (100000, True)):
            e = 0.1 if m >= 10 else 0.34
            al = Aligner(ref, e, 14, wr, False, 3, ic)
            reads = _cases.planted_reads(rng, ref, 96, 220)
            got = al.locate_batch(reads, path="filtered").tuples()
            assert got == al.locate_batch(reads, path="full").tuples() and got == al.locate_batch(reads).tuples()
            assert got == al.locate_batch(reads, path="wave").tuples()
            for q, g in zip(reads, got):
                assert g == oracle.locate(ref, q, e, 14, wr, False, 3, ic), (m, ic, wr, q)


def test_synthetic_heads(hip_backend):
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    heads = load_golden("synth_heads.json.gz")
    for name in ("C1", "C2"):
        w = synth.workload(name, 0, heads[name]["count"], device="cuda")
        al = Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
        for path in ("auto", "filtered", "full", "wave"):
            assert al.locate_batch(w["reads"], path=path).tuples() == [tup(x) for x in heads[name]["out"]], path


def test_c1_full_against_oracle(hip_backend, oracle):
    """BASELINE config C1 in full: 10 k x 100 bp, 33-bp adapter, e=0.1."""
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    w = synth.workload("C1", 0, 10000, device="cuda")
    al = Aligner(w["adapter"], 0.1, 14, False, False, 3, 1)
    got = al.locate_batch(w["reads"]).numpy()[:, :6].astype(np.int32)
    reads = w["reads"].cpu().numpy()
    exp = oracle.locate_many(w["adapter"], reads, np.full(len(reads), 100, np.int32), 0.1, 14, False, False, 3, 1, 4)
    assert np.array_equal(got, exp)
    assert (exp[:, 1] >= 0).sum() > 3000


def test_c2_sample_and_full_size_properties(hip_backend, oracle):
    """BASELINE config C2 at full size (10 M x 150 bp on the device): all records
    bit-exact against the oracle (locate_many, in chunks), plus size-independent
    properties over all 10 M records."""
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    n_total = 10_000_000
    w = synth.workload("C2", 0, n_total, device="cuda")
    reads = w["reads"]
    al = Aligner(w["adapter"], 0.1, 14, False, False, 3, 1)
    batch = al.pack(reads, layout="auto")
    assert batch.layout == "plane64"                         # what bench.py times: the two-pass pre-pass on bit planes
    rec = al.locate_batch(batch).records
    torch.cuda.synchronize()
    # (0) the two-pass pipeline, the one-pass filtered pipeline and the full sweep agree on all 10 M records
    tiles = al.pack(reads, layout="tile64")
    assert torch.equal(rec, al.locate_batch(tiles, path="filtered").records)
    assert torch.equal(rec, al.locate_batch(tiles, filtered=False).records)
    del tiles
    # (1) parity of all 10 M records
    nfound = _cases.check_locate_all(oracle, rec, w["adapter"], reads, None, 0.1, 14, False, False, 3, 1, "C2 10 M")
    # (2) invariants of every record
    r = rec.to(torch.int32)
    found = r[:, 1] >= 0
    f = r[found]
    m = len(w["adapter"])
    assert 0.45 < found.float().mean().item() < 0.60 and nfound == int(found.sum().item())
    assert bool((f[:, 0] == 0).all())                        # BACK adapter: refstart is always 0
    assert bool(((f[:, 1] > 0) & (f[:, 1] <= m)).all())
    assert bool(((f[:, 2] >= 0) & (f[:, 2] <= f[:, 3]) & (f[:, 3] <= 150)).all())
    assert bool(((f[:, 1] < m) <= (f[:, 3] == 150)).all())   # partial adapter only at the read's end
    assert bool((f[:, 5] <= (f[:, 1] * 0.1).floor().to(torch.int32)).all())   # errors <= floor(length*e)
    assert bool((f[:, 4] + f[:, 5] >= f[:, 1]).all()) and bool((f[:, 4] <= f[:, 1]).all())
    assert bool((r[~found][:, [0, 2, 3, 4, 5]] == 0).all())
    # (3) determinism / idempotence: same batch, same records; independent of batch split
    rec2 = al.locate_batch(batch).records
    assert torch.equal(rec, rec2)
    lo = 4_321_000
    part = al.locate_batch(reads[lo:lo + 100_037]).records
    assert torch.equal(part, rec[lo:lo + 100_037])
    # (4) exact-occurrence property: reads containing the whole adapter verbatim match it with 0 errors
    ad = torch.tensor(list(w["adapter"].encode()), dtype=torch.uint8, device="cuda")
    sub = reads[:1_000_000]
    win = sub.unfold(1, m, 1)                                # [N, 117, 34]
    hit = (win == ad).all(dim=2)
    has = hit.any(dim=1)
    first = hit.float().argmax(dim=1).to(torch.int32)
    rs = r[:1_000_000][has]
    assert bool((rs[:, 5] == 0).all()) and bool((rs[:, 4] == m).all()) and bool((rs[:, 2] == first[has]).all())


@pytest.mark.parametrize("kind", ["edits", "partial", "lowcomplex"])
def test_hard_batches_against_oracle(hip_backend, oracle, kind):
    """The batches C2's friendly generator does not produce (synth.hard_batch; round-5 verdict item 6): 2 M reads where
    every read keeps the exact DP busy -- the two-pass pipeline, the one-pass pipeline and the full sweep agree on every
    record, and all records are bit-exact against the oracle."""
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    n = 2_000_000
    reads = synth.hard_batch(kind, 0, n, device="cuda")
    al = Aligner(synth.TRUSEQ_34, 0.1, 14, False, False, 3, 1)
    batch = al.pack(reads, layout="auto")
    assert batch.layout == "plane64"
    rec = al.locate_batch(batch).records
    left = hip_backend.last_unresolved(n)
    tiles = al.pack(reads, layout="tile64")
    assert torch.equal(rec, al.locate_batch(tiles, path="filtered").records)
    assert torch.equal(rec, al.locate_batch(tiles, filtered=False).records)
    nfound = _cases.check_locate_all(oracle, rec, synth.TRUSEQ_34, reads, None, 0.1, 14, False, False, 3, 1, "hard " + kind)
    found = float((rec[:, 1] >= 0).float().mean().item())
    assert nfound == int((rec[:, 1] >= 0).sum().item())
    assert found > (0.4 if kind == "lowcomplex" else 0.99)
    assert left is not None and 0 <= left <= n


def test_pair_aligner_against_oracle(hip_backend, oracle):
    from atropos_amd.align import PairAligner
    from atropos_amd._lib import AtroposHipError
    assert _cases.check_pairs_against_oracle(PairAligner, oracle, AtroposHipError, seed=78, rounds=120) > 3000


def test_pairs_fast_pipeline_vs_oracle(hip_backend, oracle):
    """The fast pair pipeline (bit-vector costs, threat analysis, banded payload; pairs_fast_core.hpp) on the
    settings it takes: overlapping pairs in both directions, unrelated pairs, tandem repeats; 150- and 320-base
    envelopes (three mask-word counts, all band classes)."""
    from atropos_amd.align import PairAligner
    assert _cases.check_pairs_fast(PairAligner, oracle, seed=5, rounds=60, top=150) == 60 * 96
    assert _cases.check_pairs_fast(PairAligner, oracle, seed=6, rounds=30, top=250, npairs=130) == 30 * 130
    assert _cases.check_pairs_fast(PairAligner, oracle, seed=7, rounds=20, top=320, npairs=70) == 20 * 70
    assert _cases.check_pairs_fast(PairAligner, oracle, seed=8, rounds=40, top=40, npairs=200) == 40 * 200


def test_pairs_fast_at_size(hip_backend, oracle):
    """2 M C3 pairs and 500 k C5 pairs through atr_locate_pairs_batch (MergeOverlapping's two flag sets): all records
    against the oracle (locate_pairs_many: the reverse complement of read 2 as the reference of its pair), and every pair
    against the full sweep of pairs_core.hpp (atr_locate_pairs_full_batch).  (The oracle takes 5.5 s + 4.4 s for the C5
    pairs of the two flag sets on 16 threads: no pair is left out.)"""
    import numpy as np
    import torch
    from atropos_amd import _lib, synth
    from atropos_amd.align import PairAligner
    for config, n in (("C3", 2_000_000), ("C5", 500_000)):
        w = synth.workload(config, 11, n, device="cuda")
        for flags in (15, 9):
            pa = PairAligner(0.2, flags, revcomp_ref=True)
            be = _lib.get_backend()
            rb = pa._pack(w["reads2"], _lib.TABLE_DNA15, be, True)
            qb = pa._pack(w["reads1"], _lib.TABLE_DNA15, be, True)
            # need = 1 everywhere: every alignment matters, and the long reads take the fast pipeline too
            got = pa.locate_batch(rb, qb, need=torch.ones((n,), dtype=torch.int32, device="cuda")).records
            assert _cases.check_pairs_all(oracle, got, w["reads2"], w["reads1"], 0.2, flags, "pairs %s flags=%d" % (config, flags)) == n
            full = be.locate_pairs_full_batch(rb.packed, rb.lens, rb.max_len, True, qb.packed, qb.lens, qb.max_len, n, 0.2, flags, 1, 1)
            assert torch.equal(got, full), (config, flags)
            # with a bound on the matches: the pairs that reach it keep their record, the others may turn into None
            need = torch.full((n,), 100 if config == "C3" else 180, dtype=torch.int32, device="cuda")
            part = pa.locate_batch(rb, qb, need=need).records
            reach = (full[:, 1] >= 0) & (full[:, 4] >= need.to(torch.int16))
            assert torch.equal(part[reach], full[reach]) and int(reach.sum()) > n // 10
            rest = part[~reach]
            assert bool(((rest[:, 1] < 0) | (rest[:, 4] < need[~reach].to(torch.int16))).all())


def test_single_process_multi_stream(hip_backend):
    """The single-process multi-device driver on the one GPU there is: three backends on device 0 -- one
    host thread, stream, scratch and set of aligner handles each -- must reproduce the single-stream
    records (the per-thread side streams and event pairs of the filtered pipeline included)."""
    from atropos_amd import _lib, shard, synth
    from atropos_amd.align import Aligner
    w = synth.workload("C2", 0, 3_000_001, device="cuda")
    reads = w["reads"]
    make = lambda: Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
    want = make().locate_batch(reads).records.cpu()
    backends = [_lib.HipBackend(0) for _ in range(3)]
    for _ in range(3):
        got, seconds = shard.sharded_locate_threads(make, reads, backends)
        assert len(seconds) == 3 and torch.equal(got, want)


@pytest.mark.parametrize("planes", [False, True])
def test_pack_staged_window_edges(hip_backend, planes):
    """The LDS-staged pack (row stride <= 256) against the plain one (wide rows) on matrices allocated
    to the byte: odd strides leave the 16-byte staging window hanging over both ends of the matrix
    (those pieces are copied byte by byte), strides 250..256 need more than the default 64 KB of LDS."""
    from atropos_amd import _lib
    be = hip_backend
    gen = torch.Generator().manual_seed(77)
    mixed = torch.tensor(list(b"ACGTNRYacgtn.-"), dtype=torch.uint8)
    # mostly A C G T (the four-bases-per-step path of the staged plane pack, api.hip) with the odd other byte
    mostly = torch.tensor(list(b"ACGT" * 40 + b"NRYacgtn.-"), dtype=torch.uint8)
    custom = bytearray(be.translate_table(_lib.TABLE_DNA15))
    custom[ord("G")] = 0                                   # a table without a code for one of the four letters: no fast path
    tables = (be.translate_table(_lib.TABLE_DNA15), be.translate_table(_lib.TABLE_IUPAC), be.translate_table(_lib.TABLE_ACGT),
              bytes(custom))
    case = 0
    for width in (1, 15, 16, 17, 63, 100, 101, 150, 249, 250, 251, 255, 256):
        for nreads in (1, 63, 64, 65, 300):
            case += 1
            letters = mostly if case % 2 else mixed
            table = tables[case % len(tables)]
            host = letters[torch.randint(0, len(letters), (nreads, width), generator=gen)]
            lens = torch.randint(0, width + 1, (nreads,), generator=gen, dtype=torch.int32)
            tight = host.clone().to(be.device)                                 # exactly nreads * width bytes
            wide = torch.zeros((nreads, 512), dtype=torch.uint8)
            wide[:, :width] = host
            wide = wide.to(be.device)
            dl = lens.to(be.device)
            a, bad_a = be.pack_reads(tight, dl, width, table, count_invalid=True, planes=planes)
            b, bad_b = be.pack_reads(wide, dl, width, table, count_invalid=True, planes=planes)
            torch.cuda.synchronize()
            assert bad_a == bad_b, (width, nreads)
            assert torch.equal(a.cpu(), b.cpu()), (width, nreads)
            # a sub-matrix in the middle of a bigger allocation: the window may touch the neighbours, never use them
            pool = torch.full((nreads * width + 64,), 0x41, dtype=torch.uint8, device=be.device)
            inner = pool[29:29 + nreads * width].view(nreads, width)
            inner.copy_(tight)
            c = be.pack_reads(inner, dl, width, table, planes=planes)
            torch.cuda.synchronize()
            assert torch.equal(a.cpu(), c.cpu()), (width, nreads)


def test_dpmatrix_debug(hip_backend):
    from atropos_amd.align import Aligner
    assert _cases.check_dpmatrix_golden(Aligner) == 90


def test_ragged_tail_mode(hip_backend, oracle):
    from atropos_amd.align import Aligner
    assert _cases.check_ragged_tail_mode(Aligner, oracle, 4, nreads=200_000) == 1_000_000


def test_long_reference(hip_backend):
    """References of 129 .. 320 bases: Aligner.locate through the per-pair aligner (register strips)."""
    from atropos_amd.align import Aligner
    from atropos_amd._lib import AtroposHipError
    from oracle import oracle
    assert _cases.check_long_reference(Aligner, oracle, AtroposHipError, batch_rounds=12) > 400


def test_long_reference_envelope(hip_backend, oracle):
    from atropos_amd.align import Aligner, PairAligner
    assert _cases.check_long_reference_envelope(Aligner, PairAligner, oracle) > 250


def test_per_read_api(hip_backend, oracle):
    """Aligner.locate(str) (HipBackend.locate_one: cached buffers) == the oracle, for aligners used in turn, empty and
    maximum-length queries, references beyond an aligner handle (those keep the batch path)."""
    import random
    from atropos_amd import _lib
    from atropos_amd.align import Aligner
    rng = random.Random(11)
    aligners = []
    for m, flags, e, wr, wq, ic in ((33, 14, 0.1, False, False, 1), (20, 11, 0.2, True, False, 2), (64, 15, 0.1, False, True, 1),
                                    (100, 10, 0.12, False, False, 100000), (5, 8, 0.3, False, False, 1), (150, 14, 0.1, False, False, 1)):
        ref = _cases.rseq(rng, m, "ACGTN" if wr else "ACGT")
        aligners.append((Aligner(ref, e, flags, wr, wq, 3, ic), ref, (e, flags, wr, wq, 3, ic)))
    total = 0
    for rnd in range(300):
        al, ref, args = aligners[rnd % len(aligners)]
        n = rng.choice([0, 1, 30, 150, 151, 300, _lib.MAX_READ_LEN if len(ref) <= 128 else 320])
        q = (_cases.rseq(rng, rng.randint(0, n)) + _cases.mutate(rng, ref, 0.05))[:n] if rng.random() < 0.7 else _cases.rseq(rng, n, "ACGTN")
        assert al.locate(q) == oracle.locate(ref, q, *args), (ref, q, args)
        total += 1
    assert total == 300
    # the per-pair form (what MergeOverlapping calls through the module swap): atr_locate_pair_one
    from atropos_amd.align import PairAligner
    from atropos_amd.util import reverse_complement
    for rnd in range(200):
        flags = rng.choice([15, 9, 14, 11, 0, 3])
        e, ic, rc = rng.choice([0.1, 0.2]), rng.choice([1, 2, 100000]), rng.random() < 0.5
        wr, wq = (rng.random() < 0.2, rng.random() < 0.2) if not rc else (False, False)
        top = rng.choice([30, 150, 255, 319 if flags & 8 else 255])
        m, n = rng.randint(0, top), rng.randint(0, top)
        frag = _cases.rseq(rng, m + n + 1)
        ref, q = frag[:m], _cases.mutate(rng, frag[rng.randint(0, m):][:n], 0.05)[:n]
        pa = PairAligner(e, flags, wr, wq, 3, ic, revcomp_ref=rc)
        assert pa.locate(reverse_complement(ref) if rc else ref, q) == oracle.locate(ref, q, e, flags, wr, wq, 3, ic), (ref, q, flags, e, ic, rc)


def test_locate_stream_equals_one_call(hip_backend, oracle):
    """Aligner.locate_stream (consecutive batches on two streams, a workspace each) yields, batch by batch, the records
    of locate_batch -- plane64 and tile64 batches, equal-length and ragged, in input order; all records of the whole set
    against the oracle."""
    import numpy as np
    import torch
    from atropos_amd import synth
    from atropos_amd.align import Aligner
    from atropos_amd.shard import sharded_locate_stream
    w = synth.workload("C2", 3 << 20, 1_500_000, device="cuda:0")
    al = Aligner(w["adapter"], w["max_error_rate"], 14, False, False, w["min_overlap"], w["indel_cost"])
    reads = w["reads"]
    parts = [reads[lo:lo + 250_000] for lo in range(0, reads.shape[0], 250_000)]
    for layout in ("plane64", "tile64"):
        batches = [al.pack(p, layout=layout) for p in parts]
        one = [al.locate_batch(b).records.clone() for b in batches]
        torch.cuda.synchronize()
        for depth in (1, 2, 3):
            got = [r.records for r in al.locate_stream(batches, depth=depth)]
            torch.cuda.synchronize()
            assert len(got) == len(one)
            for g, o in zip(got, one):
                assert torch.equal(g, o)
    # raw ASCII sub-batches through the shard helper (packs as it goes), against one call over the whole set
    rec, gathered = sharded_locate_stream(al, reads, sub_batch=400_000)
    torch.cuda.synchronize()
    whole = al.locate_batch(reads).records
    assert torch.equal(rec, whole) and torch.equal(gathered, whole.cpu())
    nfound = _cases.check_locate_all(oracle, rec, w["adapter"], reads, None, w["max_error_rate"], 14, False, False,
                                     w["min_overlap"], w["indel_cost"], "locate_stream 1.5 M")
    assert nfound == int((rec[:, 1] >= 0).sum().item()) and nfound > 0.4 * reads.shape[0]


def test_pack_planes_against_numpy(hip_backend):
    """atr_pack_planes (pack_fast.hpp: round 6's branch-free core -- index bits gathered with v_dot4, invalid bytes walked
    per lane) against a numpy restatement of the layout (include/atropos_hip.h): random rows of A C G T with IUPAC letters,
    lower case, N runs and arbitrary bytes mixed in; ragged lengths, per-read starts, rows of 40 .. 256 bytes, batches
    that end inside a tile, both translate tables."""
    from atropos_amd import _lib
    rng = np.random.default_rng(41)
    be = hip_backend
    alphabet = np.frombuffer(b"ACGT" * 60 + b"NNNRYSWKMBDHVacgtn.-*X\x00\xff", np.uint8)
    total = 0
    for kind in (_lib.TABLE_DNA15, _lib.TABLE_ACGT, _lib.TABLE_IUPAC):
        table = be.translate_table(kind)
        tab = np.frombuffer(table, np.uint8).astype(np.uint32) & 15
        for n, width, max_len in ((1, 40, 33), (63, 150, 150), (65, 151, 150), (1000, 256, 250), (4099, 100, 100), (70001, 150, 150)):
            mat = alphabet[rng.integers(0, len(alphabet), (n, width))]
            if n > 500:                                              # clean rows too: the fast path alone
                mat[::3] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (len(mat[::3]), width))]
            lens = rng.integers(0, max_len + 1, n).astype(np.int32)
            starts = np.where(rng.random(n) < 0.3, rng.integers(0, 8, n), 0).astype(np.int32)
            lens = np.maximum(lens, starts)                          # (len counts from the row's start: len - start bases are packed)
            for use_lens, use_starts in ((False, False), (True, False), (True, True)):
                d_mat = torch.from_numpy(mat).cuda()
                d_lens = torch.from_numpy(lens).cuda() if use_lens else None
                d_starts = torch.from_numpy(starts).cuda() if use_starts else None
                got = be.pack_reads(d_mat, d_lens, max_len, table, starts=d_starts, planes=True).cpu().numpy().view(np.uint32)
                nch = (max_len + 31) // 32
                st = starts if use_starts else np.zeros(n, np.int32)
                ln = (lens if use_lens else np.full(n, max_len, np.int32)) - st
                ln = np.clip(ln, 0, max_len)
                pos = np.arange(32 * nch)[None, :]
                src = np.minimum(pos + st[:, None], width - 1)
                codes = np.where(pos < ln[:, None], tab[np.take_along_axis(mat, src, 1)], 0).astype(np.uint64)   # [n, 32 nch]
                ntiles = (n + 63) // 64
                want = np.zeros((ntiles, nch, 64, 4), np.uint32)
                bits = codes.reshape(n, nch, 32)
                wts = (np.uint64(1) << np.arange(32, dtype=np.uint64))
                for p in range(4):
                    words = (((bits >> np.uint64(p)) & np.uint64(1)) * wts).sum(axis=2).astype(np.uint32)       # [n, nch]
                    buf = np.zeros((ntiles * 64, nch), np.uint32)
                    buf[:n] = words
                    want[:, :, :, p] = buf.reshape(ntiles, 64, nch).transpose(0, 2, 1)
                assert np.array_equal(got[:want.size].reshape(want.shape), want), (kind, n, width, max_len, use_lens, use_starts)
                total += n
    assert total > 400_000

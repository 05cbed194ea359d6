"""The kernels of atropos_amd/csrc/fastq_kernels.hip and fastq_emit_kernels.hip at the C ABI, with inputs of their own, against the plain Python
model of tests/_fastq_kernels_common.py: the launch shapes, alignments and edges that the pipelines never choose.
Every comparison is exact.  tests/test_fastq_kernels_host.py runs the same checks on the CPU twin."""
import pytest

from . import _fastq_kernels_common as K

pytestmark = pytest.mark.gpu

# bytes per LDS stage of the four emit_staged_kernel instantiations, by record_bytes_hint: EMIT_STAGE = 13 * 1024 in
# fastq_device.hpp -- <32> EMIT_STAGE, <8> EMIT_STAGE / 4, <16> EMIT_STAGE / 2, <16> EMIT_STAGE
EMIT_STAGES = {0: 13312, 300: 3328, 390: 6656, 500: 13312}
EMIT_TILES = {0: 32, 300: 8, 390: 16, 500: 16}


def _brief(by_hint):
    return {h: {k: (sorted(v) if isinstance(v, set) else v) for k, v in r.items() if k != "need_in"} for h, r in by_hint.items()}


def test_emit_table_matches_the_launcher():
    assert {h: (t, s) for h, t, s in K.EMIT_VARIANTS} == {h: (EMIT_TILES[h], EMIT_STAGES[h]) for h in EMIT_STAGES}


def test_formatter_every_instantiation_and_the_byte_per_lane_kernel(hip_backend):
    """Hints 0, 300, 390, 500 -> emit_staged_kernel<32>, <8, STAGE/4>, <16, STAGE/2>, <16>; unaligned d_bytes, unaligned
    d_out and both -> emit_kernel.  Whole output against the model, 64 guard bytes of 0xEE on either side."""
    rep = K.check_emit_variants(hip_backend)
    print(_brief(rep["staged"]), rep["lanes"], rep["calls"])
    assert sorted(rep["staged"]) == [0, 300, 390, 500]                      # all four staged instantiations ran
    for hint, tiles in rep["staged"].items():
        assert tiles["staged"] > 0 and tiles["overflow"] > 0, hint          # a tile that fit, a tile that overflowed
        assert len(tiles["mis_in"]) >= 8 and len(tiles["mis_out"]) >= 8, hint
    assert rep["lanes"] == dict(input=3, output=3, both=3)                  # offsets 1, 7, 15 each
    assert rep["calls"] == 4 * 3 + 9                                        # every call checked its guard bytes


def test_formatter_tile_edges_offsets_order_and_names(hip_backend):
    """Per staged instantiation: n around the tile size, arrays passed from record k on, an empty tile, records out of
    file order, renamed records."""
    rep = K.check_emit_tiles(hip_backend)
    print(_brief(rep))
    assert sorted(rep) == [0, 300, 390, 500]
    for hint, r in rep.items():
        assert r["edge_calls"] == 5 and r["offset_calls"] == 8, hint
        assert r["staged"] > 0 and r["overflow"] > 0, hint
        assert len(r["mis_in"]) >= 8 and len(r["mis_out"]) >= 8, hint
        assert r["empty_tile"] >= 1, hint
        assert r["permuted_unordered"] > 0 and r["renamed_unordered"] > 0 and r["renamed_staged"] > 0, hint


def test_formatter_stage_limit(hip_backend):
    """(in_hi - in_lo) + mis_in + 16 == STAGE exactly (staged) and STAGE + 1 (the in-kernel fallback), per variant."""
    rep = K.check_emit_stage_limit(hip_backend)
    print(rep)
    assert sorted(rep) == [0, 300, 390, 500]
    for hint, (fit, overflow, need_in) in rep.items():
        assert fit > 0 and overflow > 0, hint
        assert need_in == [EMIT_STAGES[hint], EMIT_STAGES[hint] + 1], hint


def test_formatter_offsets_at_the_scan_edges(hip_backend):
    """n = 0, 1, around one and two scan blocks, and 1 048 576 + 1025 (a run of two block totals per thread of
    scan_sums_kernel): text, every offset and the total against the host model."""
    rep = K.check_emit_offsets(hip_backend)
    print(rep)
    assert tuple(rep) == K.OFFSET_COUNTS and rep[0] == 0 and all(rep[n] > 0 for n in K.OFFSET_COUNTS[2:])


def test_index_newlines_on_block_boundaries(hip_backend):
    rep = K.check_index(hip_backend)
    print(rep)
    assert rep["texts"] == 6 and rep["records"] > 6 * 120 and rep["errors"] == [1, 2, 3, 4]


def test_pack_records_against_pack_reads(hip_backend):
    rep = K.check_pack_records(hip_backend)
    print({k: v for k, v in rep.items() if k != "tables"})
    assert rep["cases"] == sum(2 * len(K.pack_nreads(m)) + 2 for m in K.PACK_MAX_LENS)
    assert rep["shifts"] == {0, 1, 2, 3}
    assert rep["long_lines"] > 0 and rep["truncated"] > 0 and rep["invalid"] > 0
    assert len(rep["tables"]) == 6                                          # three tables x both layouts


def test_quality_and_nextseq_trim_alignments(hip_backend, oracle):
    rep = K.check_quality_trim(hip_backend, oracle)
    print(rep)
    assert rep["records"] == 2 * 5 * (640 + 16)
    assert rep["stop_first"] > 0 and rep["stop_later"] > 0 and rep["stop_never"] > 0 and rep["changed"] > 0


def test_nend_trim(hip_backend, oracle):
    rep = K.check_nend_trim(hip_backend, oracle)
    print(rep)
    assert rep["records"] == 2 * 312 and rep["emptied"] > 0 and rep["inner_only"] > 0 and rep["by_mask"] > 0


def test_clip_and_match_trim(hip_backend):
    rep = K.check_clip(hip_backend)
    assert rep["run"] == 9 and rep["refused"] == 16 and rep["shorter_than_cut"] > 0
    rep = K.check_match_trim(hip_backend)
    assert rep["run"] == 5 and rep["guessed_front"] > 0 and rep["trimmed"] > 0


def test_read_and_pair_filters(hip_backend):
    rep = K.check_read_filter(hip_backend)
    print({k: v for k, v in rep.items() if k != "sides"})
    assert rep["configs"] == 54 + 8 and rep["records"] == 62 * 1025
    assert all(rep["dests"][d] > 0 for d in range(6))
    assert rep["n_fired_by_mask"] > 0
    assert all(rep["sides"][m] == {False, True} for m in (0, 0.2, 0.999, 1, 3)) and rep["sides"][-1] == {False}
    pairs = K.check_pair_filter(hip_backend)
    assert pairs["pairs"] == 2 * 4096 and pairs["differ"] > 0

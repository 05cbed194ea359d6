"""The checks of tests/test_gpu_fastq_kernels.py on the CPU twin (tests/emu/emu_fastq.cpp): the Python model and the case
builders of tests/_fastq_kernels_common.py stay verified without a GPU.  The twin has one formatter, so the formatter
checks run once, without the loop over the launch variants.  Two more tests tie the model to the reference itself:
its quality / nextseq / N-end functions over tests/golden/qualtrim_fuzz.json.gz and its indexer over
tests/golden/fastq_fuzz.json.gz (both hold the reference's own outputs)."""
import base64

from . import _fastq_kernels_common as K
from .conftest import load_golden


def test_formatter_alignments(emu_backend):
    rep = K.check_emit_variants(emu_backend)
    assert list(rep["staged"]) == [0] and rep["lanes"] == dict(input=3, output=3, both=3) and rep["calls"] == 3 + 9
    tiles = rep["staged"][0]                                    # (the case itself: what the staged kernels would do with it)
    assert tiles["staged"] > 0 and tiles["overflow"] > 0 and len(tiles["mis_in"]) >= 8 and len(tiles["mis_out"]) >= 8


def test_formatter_tile_edges_offsets_order_and_names(emu_backend):
    rep = K.check_emit_tiles(emu_backend)
    assert list(rep) == [0]
    r = rep[0]
    assert r["edge_calls"] == 5 and r["offset_calls"] == 8 and r["empty_tile"] >= 1
    assert r["permuted_unordered"] > 0 and r["renamed_unordered"] > 0 and r["renamed_staged"] > 0


def test_formatter_case_covers_every_variant():
    """The generated text has, for each of the four tile / stage sizes, tiles that fit and tiles that overflow and at
    least 8 span misalignments on either side -- from the model alone, so it holds wherever the GPU test runs."""
    case = K.shared_formatter_case()
    _, offsets = K.model_format(case["data"], case["recs"], case["begin"], case["end"], case["ubegin"], case["uend"], case["dest"],
                                case["which"])
    for hint, tile, stage in K.EMIT_VARIANTS:
        rep = K.tile_report(case["recs"], offsets, tile, stage)
        assert rep["staged"] > 0 and rep["overflow"] > 0 and rep["unordered"] == 0, hint
        assert len(rep["mis_in"]) >= 8 and len(rep["mis_out"]) >= 8, hint


def test_formatter_stage_limit(emu_backend):
    rep = K.check_emit_stage_limit(emu_backend)
    assert rep[0][0] == 1 and rep[0][1] == 1 and rep[0][2] == [13312, 13313]
    for hint, tile, stage in K.EMIT_VARIANTS:                   # the cases of the other variants, from the model
        case = K.stage_limit_case(tile, stage)
        _, offsets = K.model_format(case["data"], case["recs"], case["begin"], case["end"], None, None, None, 0)
        tiles = K.tile_report(case["recs"], offsets, tile, stage)
        assert (tiles["staged"], tiles["overflow"], tiles["need_in"]) == (1, 1, [stage, stage + 1])


def test_formatter_offsets_at_the_scan_edges(emu_backend):
    """(The twin's offsets are a serial sum: this run proves the model and the case builder.)"""
    rep = K.check_emit_offsets(emu_backend)
    assert tuple(rep) == K.OFFSET_COUNTS and rep[0] == 0 and all(rep[n] > 0 for n in K.OFFSET_COUNTS[2:])


def test_index_newlines_on_block_boundaries(emu_backend):
    rep = K.check_index(emu_backend)
    assert rep["texts"] == 6 and rep["records"] > 6 * 120 and rep["errors"] == [1, 2, 3, 4]


def test_pack_records_against_pack_reads(emu_backend):
    rep = K.check_pack_records(emu_backend)
    assert rep["cases"] == sum(2 * len(K.pack_nreads(m)) + 2 for m in K.PACK_MAX_LENS)
    assert rep["shifts"] == {0, 1, 2, 3}
    assert rep["long_lines"] > 0 and rep["truncated"] > 0 and rep["invalid"] > 0 and len(rep["tables"]) == 6


def test_quality_and_nextseq_trim_alignments(emu_backend, oracle):
    rep = K.check_quality_trim(emu_backend, oracle)
    assert rep["records"] == 2 * 5 * (640 + 16)
    assert rep["stop_first"] > 0 and rep["stop_later"] > 0 and rep["stop_never"] > 0 and rep["changed"] > 0


def test_nend_trim(emu_backend, oracle):
    rep = K.check_nend_trim(emu_backend, oracle)
    assert rep["records"] == 2 * 312 and rep["emptied"] > 0 and rep["inner_only"] > 0 and rep["by_mask"] > 0


def test_clip_and_match_trim(emu_backend):
    rep = K.check_clip(emu_backend)
    assert rep["run"] == 9 and rep["refused"] == 16 and rep["shorter_than_cut"] > 0
    rep = K.check_match_trim(emu_backend)
    assert rep["run"] == 5 and rep["guessed_front"] > 0 and rep["trimmed"] > 0


def test_read_and_pair_filters(emu_backend):
    rep = K.check_read_filter(emu_backend)
    assert rep["configs"] == 54 + 8 and rep["records"] == 62 * 1025
    assert all(rep["dests"][d] > 0 for d in range(6)) and rep["n_fired_by_mask"] > 0
    assert all(rep["sides"][m] == {False, True} for m in (0, 0.2, 0.999, 1, 3)) and rep["sides"][-1] == {False}
    pairs = K.check_pair_filter(emu_backend)
    assert pairs["pairs"] == 2 * 4096 and pairs["differ"] > 0


def test_model_trimmers_against_the_reference_fixture(oracle):
    """quality_trim_index, nextseq_trim_index and NEndTrimmer as the model states them, over every case of
    qualtrim_fuzz.json.gz (outputs of the reference's own functions)."""
    cases = load_golden("qualtrim_fuzz.json.gz")["cases"]
    for c in cases:
        seq, qual = c["seq"].encode("latin-1"), c["qual"].encode("latin-1")
        assert list(K.model_quality_trim(oracle, qual, c["cf"], c["cb"], c["base"])) == list(c["qtrim"]), c
        assert K.model_nextseq_trim(oracle, seq, qual, c["cg"], c["base"]) == c["nextseq"], c
        start, stop = K.model_n_end_trim(oracle, seq)
        assert [seq[start:stop].decode("latin-1"), qual[start:stop].decode("latin-1")] == c["nend"], c
    assert len(cases) > 2000


def test_model_index_against_the_reference_reader_fixture():
    """The model's indexer over fastq_fuzz.json.gz: the reference reader's record tuples, or -- where it raises -- the
    error of the same kind on the first record that fails (an error in a trailing, incomplete record is the
    reader's business, not the index's: there the model only has to see the leftover lines)."""
    kinds = {"expected to start with '@'": K.ERR_AT, "expected to start with '+'": K.ERR_PLUS, "don't match": K.ERR_NAME2,
             "Error creating sequence record": K.ERR_LENGTH}
    cases = load_golden("fastq_fuzz.json.gz")
    good = coded = leftover = 0
    for k, case in enumerate(cases):
        text = base64.b64decode(case["text"])
        if text and not text.endswith((b"\n", b"\r")):
            text += b"\n"                                       # as FastqBatch.from_bytes(final=True) terminates the last line
        records, err = K.model_records(text)
        nlines = len(K.model_lines(text))
        if "error" not in case:
            assert err == K.INT64_MAX and nlines % 4 == 0, k
            got = [[n.decode("latin-1"), s.decode("latin-1"), q.decode("latin-1"), n.decode("latin-1") if rep else ""]
                   for n, s, rep, q in records]
            assert got == case["records"], k
            good += 1
        elif err != K.INT64_MAX:
            code = [c for text_, c in kinds.items() if text_ in case["error"][1]]
            assert code == [err % 8], (k, case["error"], err)
            coded += 1
        else:
            assert nlines % 4 != 0, (k, case["error"])
            leftover += 1
    assert good + coded + leftover == 300 and good > 150 and coded > 20 and leftover > 5

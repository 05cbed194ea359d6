"""GPU tier of the trim report: the golden cases on the device, the smallest shapes at which the report kernels can go
wrong against the per-object host path (``modifiers.AdapterCutter`` over ``adapters.Adapter``, plain Python sums:
independent of the report kernels), accumulation across chunks, and the 64-bit counters."""
import numpy as np
import pytest
import torch

from atropos_amd import _lib
from atropos_amd.fastq import FastqBatch
from atropos_amd.trim import pipeline_from_args

from . import _report_common as R

pytestmark = pytest.mark.gpu

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
AD = "GATTACAGATTACA"
FRONT = "CCTTGGAACCTTGG"


def agree(args, text, **kw):
    """Device report == host path (source key 0 on both sides)."""
    ours = R.device_summary(args, text, **kw)
    R.same(R.plain(ours), R.plain(R.host_summary(args, text)))
    return ours


@pytest.mark.parametrize("index", range(len(R.golden()["cases"])), ids=R.case_ids("cases"))
def test_single_end_golden(hip_backend, tmp_path, index):
    R.run_case(R.golden()["cases"][index], tmp_path)


@pytest.mark.parametrize("index", range(len(R.golden()["paired"])), ids=R.case_ids("paired"))
def test_paired_golden(hip_backend, tmp_path, index):
    R.run_case(R.golden()["paired"][index], tmp_path)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_wave_and_block_edges(hip_backend, n):
    text = R.fastq_of(R.synthetic_reads(n, 100 + n, AD))
    ours = agree("-a %s -u 2 -m 10" % AD, text)
    assert ours["total_record_count"] == n


def test_only_empty_reads(hip_backend):
    ours = agree("-a %s -u 2 -m 1" % AD, R.fastq_of([""] * 130))
    assert ours["total_record_count"] == 130 and ours["sum_total_bp_count"] == 0
    assert ours["trim"]["modifiers"]["UnconditionalCutter"]["bp_trimmed"] == (0,)       # clip counts nothing for them


def test_shortest_and_longest_reads(hip_backend):
    """Reads of 1 base, and of the table's maximum length with the 3' adapter at the very start (everything goes) and a
    5' adapter that ends at the last base: the last bin of both histograms."""
    L = 80
    body = "".join("ACGT"[v] for v in np.random.RandomState(5).randint(0, 4, size=L))
    reads = ["A", "G", AD[:1], AD + body[:L - len(AD)], body[:L - len(FRONT)] + FRONT]
    args = "-a back=%s -g front=%s" % (AD, FRONT)
    ours = agree(args, R.fastq_of(reads * 3), max_read_len=L)
    ads = ours["trim"]["modifiers"]["AdapterCutter"]["adapters"][0]
    assert ads["back"]["lengths_back"] == {L: 3} and ads["front"]["lengths_front"] == {L: 3}
    with pytest.raises(_lib.AtroposUnsupported, match="^report: "):
        R.device_summary(args, R.fastq_of(reads), max_read_len=L - 1)


def test_three_adapters_last_one_matches(hip_backend):
    """Bodies of A and G alone, eight bases of overlap asked for: adapters one (T's) and two (C's) cannot match, so
    every count belongs to the third table."""
    rng = np.random.RandomState(7)
    reads = []
    for _ in range(300):
        body = "".join("AG"[v] for v in rng.randint(0, 2, size=rng.randint(0, 50)))
        reads.append(body + AD[:int(rng.randint(8, len(AD) + 1))] if rng.rand() < 0.7 else body)
    ours = agree("-a one=TTTTTTTTTTTTCC -a two=CCCCCCCCCCCCTT -a three=%s -O 8" % AD, R.fastq_of(reads))
    ads = ours["trim"]["modifiers"]["AdapterCutter"]["adapters"][0]
    assert ads["one"]["total"] == 0 and ads["two"]["total"] == 0 and ads["three"]["total"] > 150
    assert ads["one"]["lengths_back"] == {} and sum(ads["three"]["adjacent_bases"].values()) == ads["three"]["total"]
    assert type(ours["trim"]["modifiers"]["AdapterCutter"]["records_with_adapters"]) is tuple


def test_times_three_with_masks(hip_backend):
    rng = np.random.RandomState(9)
    reads = ["".join("ACGT"[v] for v in rng.randint(0, 4, size=rng.randint(0, 12))).join([AD] * int(rng.randint(0, 5)))
             for _ in range(200)]
    ours = agree("-b %s -n 3 --mask-adapter" % AD, R.fastq_of(reads))
    cutter = ours["trim"]["modifiers"]["AdapterCutter"]
    (stats,) = cutter["adapters"][0].values()
    assert stats["total"] > 2 * cutter["records_with_adapters"][0]                    # every match counted twice


def test_adjacent_base_edge_cases(hip_backend):
    """A 3' match at rstart == 0, one before a lower-case base and one before N: all three count under ''."""
    reads = [AD + "ACGT", "acgta" + AD, "ACGTN" + AD, "ACGTC" + AD, "ACGTT" + AD + "AA"]
    ours = agree("-a %s" % AD, R.fastq_of(reads))
    (stats,) = ours["trim"]["modifiers"]["AdapterCutter"]["adapters"][0].values()
    assert stats["adjacent_bases"] == {"A": 0, "C": 1, "G": 0, "T": 1, "": 3}


def test_lds_and_global_variants(hip_backend):
    text = R.fastq_of(R.synthetic_reads(20000, 11, AD))
    args = "-b %s -a other=ACCGGTTAACCGGTT -n 2" % AD
    host = R.plain(R.host_summary(args, text))
    for variant in ("lds", "global"):
        R.same(R.plain(R.device_summary(args, text, variant=variant)), host)
    # no LDS table for a 614-base read with errors 0 .. 5: 2 x (8 + 2 x 615 x 6) = 14 776 words > 12 288
    with pytest.raises(_lib.AtroposUnsupported):
        R.device_summary(args + " -e 0.3", R.fastq_of(["ACGT" * 150 + AD]), variant="lds")
    agree(args + " -e 0.3", R.fastq_of(["ACGT" * 150 + AD, "ACGT" * 100]))             # 'auto' then counts in global memory


def test_accumulation_across_chunks(hip_backend, tmp_path):
    text = R.fastq_of(R.synthetic_reads(70000, 13, TRUSEQ, read_len=100))
    args = "-a %s -q 20 -u 3 --trim-n -m 25" % TRUSEQ
    path = tmp_path / "in.fastq"
    path.write_bytes(text)
    outs = []
    for report in (True, False):
        pipe = pipeline_from_args(args, report=report)
        out = tmp_path / ("out%d.fastq" % report)
        pipe.trim_file(str(path), str(out), chunk_bytes=len(text) // 5)
        outs.append(out.read_bytes())
        if report:
            chunked = pipe.report_summary
    assert outs[0] == outs[1] and len(outs[0]) > 0
    whole = R.device_summary(args, text)
    assert chunked["total_record_count"] == 70000
    R.same(R.plain(chunked["trim"]), R.plain(whole["trim"]))
    assert chunked["bp_counts"] == {str(path): whole["bp_counts"][0]}


def test_counters_are_64_bit(hip_backend):
    """A block pre-loaded just below 2^32 still adds correctly, in every kind of word."""
    text = R.fastq_of(R.synthetic_reads(500, 17, AD))
    args = "-a %s -u 2" % AD
    base = R.device_summary(args, text)
    pipe = pipeline_from_args(args, report=True)
    rep = R.TrimReport(pipe)
    try:
        start = (1 << 32) - 3
        rep.mates[0].counters.fill_(start)
        batch, _ = FastqBatch.from_bytes(text, final=True)
        rep.add(pipe.run(batch))
        torch.cuda.synchronize()
        words = hip_backend.report_read(rep.mates[0].handle, rep.mates[0].counters) - start
        rep.mates[0].counters.copy_(torch.from_numpy(words).to(rep.mates[0].counters.device))
        R.same(R.plain(rep.summary()), R.plain(base))
        assert base["sum_total_bp_count"] + start > (1 << 32)
    finally:
        rep.close()

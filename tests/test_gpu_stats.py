"""Read statistics on the GPU (atr_read_stats_batch through atropos_amd.stats and the trim pipelines' stats=):
exact against the reference's summaries (tests/golden/stats_fuzz.json.gz) and against the numpy model of
test_stats_host at size; chunking and merging do not change a count; post-trim statistics are those of the
files written."""
import base64

import numpy as np
import pytest
import torch

from .conftest import load_golden
from .test_stats_host import check_errors, check_summary, empty_counts, finish, model_counts

pytestmark = pytest.mark.gpu

TRUSEQ = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
PE1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACACAGTGATCTCGTATGCCGTCTTCTGCTTG"
PE2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGTAGATCTCGGTGGTCGCCGTATCATT"


@pytest.fixture(scope="module")
def be():
    from atropos_amd import _lib
    _lib.set_backend(None)
    return _lib.get_backend()


def _batch(text):
    from atropos_amd.fastq import FastqBatch
    return FastqBatch.from_bytes(text.encode("latin-1") if isinstance(text, str) else text, final=True)[0]


def _same_counts(a, b):
    for k in ("count", "longest", "withq", "skipped"):
        assert a[k] == b[k], k
    for k in ("lengths", "gc", "meanq", "seq", "qual", "first_len", "first_gc", "first_mq"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def test_golden_cases(be):
    from atropos_amd.reads import Read
    from atropos_amd.stats import PairedEndReadStatistics, SingleEndReadStatistics
    doc = load_golden("stats_fuzz.json.gz")
    for case in doc["cases"]:
        qb = case["quality_base"]
        if len(case["fastq"]) == 1:
            st = SingleEndReadStatistics(qualities=True, quality_base=qb)
            st.collect_batch(_batch(case["fastq"][0]))
            per_read = [st]
        else:
            st = PairedEndReadStatistics(qualities=True, quality_base=qb)
            st.collect_batch(_batch(case["fastq"][0]), _batch(case["fastq"][1]))
            per_read = [st.read1, st.read2]
        got = st.summarize()
        for k in range(len(case["fastq"])):
            check_summary(got["read%d" % (k + 1)], case["summary"]["read%d" % (k + 1)], case["name"])
        check_errors([s.counts() for s in per_read], case, case["name"])
        # the per-record API goes through the same device path
        one = SingleEndReadStatistics(qualities=True, quality_base=qb)
        for rec in _batch(case["fastq"][0]).to_records():
            one.collect(Read(rec[0], rec[1], rec[2]))
        check_summary(one.summarize()["read1"], case["summary"]["read1"], case["name"] + " (collect)")


def _device_batch(be, seqs, quals, lens):
    """A FastqBatch over records laid out as [sequence][qualities] back to back (no names) in device memory."""
    from atropos_amd.fastq import FastqBatch
    n = lens.numel()
    off = torch.cumsum(2 * lens.to(torch.int64), 0) - 2 * lens.to(torch.int64)
    total = int((2 * lens.to(torch.int64)).sum().item())
    assert total < (1 << 32) - 16                      # (offsets are unsigned 32-bit, stored in int32)
    data = torch.zeros(((total + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=be.device)
    width = seqs.shape[1]
    pos = torch.arange(width, device=be.device)
    valid = pos[None, :] < lens[:, None]
    idx = (off[:, None] + pos[None, :])[valid]
    data[idx] = seqs[valid]
    data[idx + lens.to(torch.int64)[:, None].expand(-1, width)[valid]] = quals[valid]
    records = torch.zeros((n, 8), dtype=torch.int32, device=be.device)
    u32 = lambda x: torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32)
    records[:, 2] = u32(off)
    records[:, 3] = lens.to(torch.int32)
    records[:, 4] = u32(off + lens.to(torch.int64))
    records[:, 5] = lens.to(torch.int32)
    return FastqBatch(data, total, records, be)


def test_at_size(be):
    """10 M synthetic 150 bp reads and 1 M ragged reads of up to 5 000 arbitrary bytes: every counter exact."""
    from atropos_amd import synth
    from atropos_amd.stats import ReadStatistics
    gen = torch.Generator(device=be.device)
    gen.manual_seed(7)
    n = 10_000_000
    w = synth.workload("C2", 0, n, device=str(be.device))
    seqs = w["reads"]
    quals = torch.randint(35, 75, seqs.shape, dtype=torch.uint8, device=be.device, generator=gen)
    lens = torch.full((n,), seqs.shape[1], dtype=torch.int32, device=be.device)
    st = ReadStatistics(qualities=True)
    st.collect_batch(_device_batch(be, seqs, quals, lens))
    del w
    want = finish(model_counts(seqs.cpu().numpy(), quals.cpu().numpy(), lens.cpu().numpy().astype(np.int64)))
    _same_counts(st.counts(), want)
    del seqs, quals

    m = 1_000_000
    rng = np.random.RandomState(11)
    L = np.where(rng.rand(m) < 0.1, rng.randint(0, 5001, m), rng.randint(0, 301, m)).astype(np.int64)
    order = np.argsort(L, kind="stable")
    st = ReadStatistics(qualities=True, quality_base=64)
    acc = empty_counts(5000)
    # the reads in slices of similar length (little padding for the model); all bytes 0 .. 255
    for lo in range(0, m, 50_000):
        sel = order[lo:lo + 50_000]
        wdt = max(1, int(L[sel].max()))
        S = rng.randint(0, 256, (len(sel), wdt), dtype=np.uint8)
        Q = rng.randint(0, 256, (len(sel), wdt), dtype=np.uint8)
        model_counts(S, Q, L[sel], quality_base=64, acc=acc, chunk=20_000)
        st.collect_batch(_device_batch(be, torch.from_numpy(S).to(be.device), torch.from_numpy(Q).to(be.device),
                                       torch.from_numpy(L[sel]).to(be.device)))
    _same_counts(st.counts(), finish(acc))


def _synth_text(name):
    doc = load_golden("trim_cases.json.gz")
    return base64.b64decode(doc["inputs"][name])


def test_chunking_and_merge(be, tmp_path):
    from atropos_amd.fastq import FastqBatch
    from atropos_amd.stats import SingleEndReadStatistics, qc_file, qc_files
    text = _synth_text("synth.fastq") * 3
    path = tmp_path / "in.fastq"
    path.write_bytes(text)
    whole = SingleEndReadStatistics(qualities=True)
    batch, _ = FastqBatch.from_bytes(text)
    whole.collect_batch(batch)
    small = qc_file(str(path), chunk_bytes=max(4096, len(text) // 40))
    assert small == {"pre": {0: whole.summarize()}}
    # two halves merged == the whole
    half = len(batch) // 2
    a, b = SingleEndReadStatistics(qualities=True), SingleEndReadStatistics(qualities=True)
    a.collect_batch(batch.head(half)[0])
    rest = FastqBatch(batch.data, batch.nbytes, batch.records[half:], be)
    b.collect_batch(rest)
    _same_counts(a.merge(b).counts(), whole.counts())
    # paired files in lock step
    p1, p2 = tmp_path / "1.fastq", tmp_path / "2.fastq"
    p1.write_bytes(_synth_text("synth_pe.1.fastq"))
    p2.write_bytes(_synth_text("synth_pe.2.fastq"))
    got = qc_files(str(p1), str(p2), chunk_bytes=8192)
    assert got["pre"][0]["read1"] == qc_file(str(p1))["pre"][0]["read1"]
    assert got["pre"][0]["read2"] == qc_file(str(p2))["pre"][0]["read1"]


@pytest.mark.parametrize("args", [
    "-a %s -q 20 -m 20 -M 90 --max-n 3" % TRUSEQ,
    "-a %s --mask-adapter --trim-n -m 25" % TRUSEQ,
    "-a %s --quality-base 64 --zero-cap -m 40" % TRUSEQ,
])
def test_post_equals_written_single(be, tmp_path, args):
    from atropos_amd.stats import qc_file
    from atropos_amd.trim import pipeline_from_args
    src = tmp_path / "in.fastq"
    src.write_bytes(_synth_text("synth.fastq") * 4)
    pipe = pipeline_from_args(args)
    pipe.stats = ("pre", "post")
    qb = pipe.quality_base
    outs = {k: str(tmp_path / (k + ".fastq")) for k in ("too_short", "too_long", "too_many_n")}
    pipe.outputs = dict(outs)
    counts = pipe.trim_file(str(src), str(tmp_path / "out.fastq"), chunk_bytes=20000)
    summ = pipe.stats_summary
    assert summ["pre"] == qc_file(str(src), quality_base=qb)["pre"]
    names = {"keep": "NoFilter", "too_short": "too_short", "too_long": "too_long", "too_many_n": "too_many_n"}
    files = dict(outs, keep=str(tmp_path / "out.fastq"))
    assert set(summ["post"]) == {names[k] for k, v in counts.items() if v}
    for kind, v in counts.items():
        if v:
            assert summ["post"][names[kind]] == qc_file(files[kind], quality_base=qb)["pre"], kind


@pytest.mark.parametrize("args", [
    "--aligner insert -a %s -A %s -q 20 -m 30" % (PE1, PE2),
    "--aligner insert -a %s -A %s --correct-mismatches liberal -m 30 --mask-adapter" % (PE1, PE2),
])
def test_post_equals_written_paired(be, tmp_path, args):
    from atropos_amd.stats import qc_files
    from atropos_amd.trim import pipeline_from_args
    p1, p2 = tmp_path / "1.fastq", tmp_path / "2.fastq"
    p1.write_bytes(_synth_text("synth_pe.1.fastq") * 3)
    p2.write_bytes(_synth_text("synth_pe.2.fastq") * 3)
    pipe = pipeline_from_args(args, paired_input=True)
    pipe.stats = ("pre", "post")
    short = (str(tmp_path / "s1.fastq"), str(tmp_path / "s2.fastq"))
    pipe.outputs = {"too_short": short}
    o1, o2 = str(tmp_path / "o1.fastq"), str(tmp_path / "o2.fastq")
    counts = pipe.trim_files(str(p1), str(p2), o1, o2, chunk_bytes=30000)
    summ = pipe.stats_summary
    assert summ["pre"] == qc_files(str(p1), str(p2))["pre"]
    assert summ["post"]["NoFilter"] == qc_files(o1, o2)["pre"]
    if counts["too_short"]:
        assert summ["post"]["too_short"] == qc_files(*short)["pre"]


def test_trim_stats_golden(be, tmp_path):
    from atropos_amd.trim import pipeline_from_args
    doc = load_golden("stats_fuzz.json.gz")
    assert len(doc["trim"]) >= 5
    for idx, case in enumerate(doc["trim"]):
        paths = []
        for k, name in enumerate(case["inputs"]):
            paths.append(tmp_path / ("in%d_%d.fastq" % (idx, k)))
            paths[-1].write_bytes(_synth_text(name))
        paired = len(paths) == 2
        pipe = pipeline_from_args(case["args"], paired_input=paired)
        pipe.stats = ("pre", "post")
        if paired:
            pipe.trim_files(str(paths[0]), str(paths[1]), str(tmp_path / "o1"), str(tmp_path / "o2"), chunk_bytes=16384)
        else:
            pipe.trim_file(str(paths[0]), str(tmp_path / "o1"), chunk_bytes=16384)
        got = pipe.stats_summary
        label = case["args"]
        for k, want in case["pre"].items():
            check_summary(got["pre"][0][k], want, label + " pre " + k)
        assert set(got["post"]) == set(case["post"]), label
        for dest, per in case["post"].items():
            for k, want in per.items():
                check_summary(got["post"][dest][0][k], want, "%s post %s %s" % (label, dest, k))


def test_unsupported_destinations(be, tmp_path):
    from atropos_amd.trim import pipeline_from_args
    src = tmp_path / "in.fastq"
    src.write_bytes(_synth_text("synth.fastq"))
    pipe = pipeline_from_args("-a %s --discard-untrimmed" % TRUSEQ)
    pipe.stats = ("post",)
    with pytest.raises(NotImplementedError):
        pipe.trim_file(str(src), str(tmp_path / "out.fastq"))
    assert not (tmp_path / "out.fastq").exists()          # refused before any output is opened

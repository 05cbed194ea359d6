"""Read statistics, CPU tier: a numpy model of what atr_read_stats_batch counts feeds atropos_amd.stats' summariser,
which must give the reference's summaries (tests/golden/stats_fuzz.json.gz, make_stats_golden.py); the integer
rounding on ties; argument checks of the atr_read_stats_* entry points, which touch no device."""
import ctypes
import math

import numpy as np
import pytest

from .conftest import load_golden

ACGTN = b"ACGTN"


# ---------------------------------------------------------------------------------------------- the model
def parse_fastq(text):
    """[(sequence bytes, quality bytes)] of a FASTQ text with "\\n" or "\\r\\n" line ends."""
    lines = text.encode("latin-1").replace(b"\r\n", b"\n").split(b"\n")
    return [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def matrices(records):
    """Padded uint8 matrices of sequences and qualities, and the lengths."""
    lens = np.array([len(s) for s, _ in records], dtype=np.int64)
    width = max(1, int(lens.max()) if len(lens) else 1)
    seq = np.zeros((len(records), width), dtype=np.uint8)
    qual = np.zeros((len(records), width), dtype=np.uint8)
    for i, (s, q) in enumerate(records):
        seq[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        qual[i, :len(q)] = np.frombuffer(q, dtype=np.uint8)
    return seq, qual, lens


def _round_even(num, den):
    q, r = np.divmod(num, den)
    return q + ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))


def empty_counts(width):
    return dict(count=0, longest=0, withq=0, skipped=0, lengths=np.zeros(width + 1, np.int64),
                gc=np.zeros(101, np.int64), meanq=np.zeros(256, np.int64),
                seq=np.zeros((width, 256), np.int64), qual=np.zeros((width, 256), np.int64),
                first_len=np.full(width + 1, -1, np.int64), first_gc=np.full(101, -1, np.int64),
                first_mq=np.full(256, -1, np.int64), next=0)


def _first_seen(first, values, idx):
    """first[v] = the smallest index among idx[values == v] (or what it was, if smaller)."""
    u, pos = np.unique(values, return_index=True)
    cur, new = first[u], idx[pos]
    first[u] = np.where(cur < 0, new, np.minimum(cur, new))


def model_counts(seq, qual, lens, quality_base=33, chunk=1 << 20, acc=None):
    """What the kernels add for reads seq[i, :lens[i]] with qualities (numpy, integer only).  ``acc``: counts to
    add into (same layout as ReadStatistics.counts(); tables as wide as the reads)."""
    if acc is None:
        acc = empty_counts(seq.shape[1])
    width = acc["seq"].shape[0]
    assert seq.shape[1] <= width
    pos = np.arange(seq.shape[1])
    for lo in range(0, seq.shape[0], chunk):
        S, Q, L = seq[lo:lo + chunk], qual[lo:lo + chunk], lens[lo:lo + chunk].astype(np.int64)
        idx = acc["next"] + lo + np.arange(len(L), dtype=np.int64)
        acc["count"] += len(L)
        acc["lengths"] += np.bincount(L, minlength=width + 1)[:width + 1]
        _first_seen(acc["first_len"], L, idx)
        ne = L > 0
        if not ne.any():
            continue
        S, Q, L, idx = S[ne], Q[ne], L[ne], idx[ne]
        valid = pos[None, :] < L[:, None]
        acc["longest"] = max(acc["longest"], int(L.max()))
        acc["withq"] += len(L)
        gc = (((S == ord("C")) | (S == ord("G"))) & valid).sum(axis=1)
        gcb = _round_even(100 * gc, L)
        acc["gc"] += np.bincount(gcb, minlength=101)
        _first_seen(acc["first_gc"], gcb, idx)
        qs = (Q.astype(np.int64) * valid).sum(axis=1) - quality_base * L
        mqb = _round_even(qs, L) + quality_base
        acc["meanq"] += np.bincount(mqb, minlength=256)
        _first_seen(acc["first_mq"], mqb, idx)
        idx = (pos[None, :] * 256 + S.astype(np.int64))[valid]
        acc["seq"] += np.bincount(idx, minlength=width * 256).reshape(width, 256)
        idx = (pos[None, :] * 256 + Q.astype(np.int64))[valid]
        acc["qual"] += np.bincount(idx, minlength=width * 256).reshape(width, 256)
    acc["next"] += seq.shape[0]
    return acc


def finish(acc):
    """Trim the tables to the longest non-empty read and the length histogram to the longest read."""
    out = dict(acc)
    del out["next"]
    out["seq"], out["qual"] = acc["seq"][:acc["longest"]], acc["qual"][:acc["longest"]]
    nz = np.nonzero(acc["lengths"])[0]
    nlen = int(nz.max()) + 1 if len(nz) else 1
    out["lengths"], out["first_len"] = acc["lengths"][:nlen], acc["first_len"][:nlen]
    return out


# ---------------------------------------------------------------------------------------------- comparisons
def check_hist(got, want, label):
    assert got["hist"] == {int(k): v for k, v in want["hist"]}, label
    s = got["summary"]
    assert s["mean"] == want["mean"], (label, s["mean"], want["mean"])
    assert math.isclose(s["stdev"], want["stdev"], rel_tol=1e-12, abs_tol=1e-300), (label, s["stdev"], want["stdev"])
    assert s["median"] == want["median"], (label, s["median"], want["median"])
    assert list(s["modes"]) == want["modes"], (label, s["modes"], want["modes"])


def _columns(table):
    cols = list(table["columns"])
    rows = [list(r) for r in (table["rows"].values() if isinstance(table["rows"], dict) else table["rows"])]
    return len(rows), {c: [r[j] for r in rows] for j, c in enumerate(cols)}


def check_summary(got, want, label):
    assert got["counts"] == want["counts"], label
    for key in ("lengths", "gc", "qualities"):
        assert (key in got) == (key in want), (label, key)
        if key in want:
            check_hist(got[key], want[key], "%s %s" % (label, key))
    for key in ("bases", "base_qualities"):
        assert (key in got) == (key in want), (label, key)
        if key in want:
            assert _columns(got[key]) == _columns(want[key]), (label, key)
    if "bases" in got:
        assert list(got["bases"]["columns"][:4]) == list("ACGT") and got["bases"]["columns"][-1] == "N"


def check_errors(counts_per_read, case, label):
    from atropos_amd.stats import error_rate_from_counts
    for e in case["errors"]:
        for k, c in enumerate(counts_per_read):
            if e["total_len"][k] == 0:
                continue
            est, total = error_rate_from_counts(c, e["max_bases"])
            assert total == e["total_len"][k], (label, e["max_bases"])
            assert math.isclose(est, e["estimate"][k], rel_tol=1e-12), (label, e["max_bases"], est, e["estimate"][k])


# ---------------------------------------------------------------------------------------------- tests
def test_golden_summaries_from_model_counts():
    from atropos_amd.stats import summarize_counts
    doc = load_golden("stats_fuzz.json.gz")
    assert len(doc["cases"]) >= 8
    for case in doc["cases"]:
        counts = []
        for k, text in enumerate(case["fastq"]):
            c = finish(model_counts(*matrices(parse_fastq(text)), quality_base=case["quality_base"]))
            counts.append(c)
            got = summarize_counts(c, case["quality_base"], True)
            check_summary(got, case["summary"]["read%d" % (k + 1)], "%s read%d" % (case["name"], k + 1))
        check_errors(counts, case, case["name"])


def test_round_half_even():
    from atropos_amd.stats import div_round_even
    assert div_round_even(100, 8) == 12 and round(100 / 8) == 12           # 12.5 -> 12
    assert div_round_even(300, 8) == 38 and round(300 / 8) == 38           # 37.5 -> 38
    assert div_round_even(-1, 2) == 0 and round(-1 / 2) == 0               # -0.5 -> 0
    assert div_round_even(-3, 2) == -2 and round(-3 / 2) == -2             # -1.5 -> -2
    assert div_round_even(-5, 2) == -2 and round(-5 / 2) == -2             # -2.5 -> -2
    assert div_round_even(-7, 3) == -2 and round(-7 / 3) == -2
    rng = np.random.RandomState(3)
    for den in list(range(1, 300)) + [32735, 32736]:
        nums = np.concatenate([rng.randint(-255 * den, 255 * den + 1, size=60), np.arange(-3 * den, 3 * den + 1, max(1, den // 2))])
        for num in nums.tolist():
            assert div_round_even(num, den) == round(num / den), (num, den)
        assert (_round_even(np.array(nums), den) == np.array([round(n / den) for n in nums.tolist()])).all()


def test_summary_edge_rules():
    from atropos_amd.stats import hist_summary, summarize_counts
    one = hist_summary({7: 3})
    assert one["summary"] == dict(mean=7.0, stdev=0, median=7.0, modes=[7])
    with pytest.raises(ValueError):
        hist_summary({})
    # zero-length reads only: count and lengths, no GC (the reference cannot summarise the empty GC histogram)
    c = finish(model_counts(*matrices([(b"", b""), (b"", b"")])))
    assert c["count"] == 2 and c["lengths"].tolist() == [2] and c["longest"] == 0
    with pytest.raises(ValueError):
        summarize_counts(c)
    # qualities=None: quality statistics appear with the first non-empty read
    c = finish(model_counts(*matrices([(b"", b""), (b"AC", b"II")])))
    s = summarize_counts(c, 33, None)
    assert s["qualities"]["hist"] == {40: 1} and s["base_qualities"]["columns"] == (40,)
    c2 = dict(c, withq=0)
    assert "qualities" not in summarize_counts(c2, 33, None)
    with pytest.raises(RuntimeError):
        summarize_counts(dict(c, skipped=1))


def test_layout_matches_library():
    from atropos_amd import _lib
    from atropos_amd.stats import layout
    lib = _lib.load_library()
    for cap in (1, 150, 256, _lib.MAX_LONG_READ_LEN):
        assert lib.atr_read_stats_bytes(cap) == layout(cap)["words"] * 8


def test_abi_argument_checks_without_device():
    from atropos_amd import _lib
    lib = _lib.load_library()
    fake = ctypes.c_void_p(1 << 20)                      # never dereferenced: every call below fails its checks
    assert lib.atr_read_stats_bytes(0) == -1
    assert lib.atr_read_stats_bytes(_lib.MAX_LONG_READ_LEN + 1) == -2
    assert lib.atr_read_stats_clear(None, 150, None) == -1
    assert lib.atr_read_stats_clear(fake, 0, None) == -1
    assert lib.atr_read_stats_clear(fake, _lib.MAX_LONG_READ_LEN + 1, None) == -2

    def batch(stats=fake, max_len=150, longest=150, qb=33, data=fake, recs=fake, b=fake, e=fake, ub=None, ue=None,
              n=10, base=0):
        return lib.atr_read_stats_batch(stats, max_len, longest, qb, data, recs, b, e, ub, ue, None, 0, n, base, None)

    assert batch(stats=None) == -1
    assert batch(max_len=0) == -1
    assert batch(max_len=_lib.MAX_LONG_READ_LEN + 1, longest=10) == -2
    assert batch(longest=151) == -1 and batch(longest=-1) == -1
    assert batch(qb=-1) == -1 and batch(qb=256) == -1
    assert batch(n=-1) == -1
    assert batch(base=-1) == -1
    assert batch(b=None) == -1                            # begin without end
    assert batch(ub=fake) == -1                           # unmasked_begin without unmasked_end
    assert batch(b=None, e=None, ub=fake, ue=fake) == -1  # a mask needs the interval
    assert batch(data=None) == -1 and batch(recs=None) == -1
    assert batch(data=None, recs=None, n=0) == 0          # nothing to do, nothing launched
    assert lib.atr_read_stats_merge(fake, 100, fake, 150, 0, None) == -1
    assert lib.atr_read_stats_merge(None, 150, fake, 150, 0, None) == -1
    assert lib.atr_read_stats_merge(fake, 150, fake, 0, 0, None) == -1
    assert lib.atr_read_stats_merge(fake, 150, fake, 150, -1, None) == -1


def test_tiles_and_missing_qualities_refused():
    from atropos_amd.reads import Read
    from atropos_amd.stats import ReadStatistics, SingleEndReadStatistics
    with pytest.raises(NotImplementedError):
        ReadStatistics(qualities=True, tiles=True)
    st = SingleEndReadStatistics(backend=object())       # queued reads do not touch the backend
    with pytest.raises(NotImplementedError):
        st.collect(Read("r", "ACGT", None))
    with pytest.raises(NotImplementedError):
        ReadStatistics().collect(Read("r", "ACGT", "IIII"))


def test_post_stats_refused_before_any_output(tmp_path):
    from atropos_amd.trim import PairedTrimPipeline, TrimPipeline
    src, dst = tmp_path / "in.fastq", tmp_path / "out.fastq"
    src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(NotImplementedError):
        TrimPipeline(discard_untrimmed=True, stats=("post",)).trim_file(str(src), str(dst))
    with pytest.raises(NotImplementedError):
        PairedTrimPipeline(merge_overlapping=True, stats=("pre", "post")).trim_files(
            str(src), str(src), str(dst), str(tmp_path / "out2.fastq"))
    assert not dst.exists()


def test_trim_stats_keyword():
    from atropos_amd.trim import PairedTrimPipeline, TrimPipeline
    assert TrimPipeline(stats=("pre", "post")).stats == ("pre", "post")
    assert TrimPipeline().stats == ()
    assert PairedTrimPipeline(stats=("post",)).stats == ("post",)
    with pytest.raises(ValueError):
        TrimPipeline(stats=("during",))

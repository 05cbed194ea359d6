"""The CPU oracle (oracle/align_oracle.c) against the golden vectors generated from
the reference itself (tests/golden/make_golden.py).  This is what pins the oracle on
a machine where /root/reference does not exist."""
from .conftest import load_golden, tup


def test_kats_locate(oracle):
    kats = load_golden("kats.json")
    assert len(kats["locate"]) > 200
    for c in kats["locate"]:
        got = oracle.locate(c["ref"], c["query"], c["e"], c["flags"], c["wr"], c["wq"], c["mo"], c["ic"])
        assert got == tup(c["out"]), c


def test_kats_compare(oracle):
    kats = load_golden("kats.json")
    for c in kats["compare_prefixes"]:
        assert oracle.compare_prefixes(c["ref"], c["query"], c["wr"], c["wq"]) == tup(c["out"]), c
    for c in kats["compare_suffixes"]:
        assert oracle.compare_suffixes(c["ref"], c["query"], c["wr"], c["wq"]) == tup(c["out"]), c


def test_kats_multi(oracle):
    for c in load_golden("kats.json")["multi_locate"]:
        got = oracle.multi_locate(c["ref"], c["query"], c["e"], c["flags"], c["mo"], c["mx"])
        assert got == [tup(x) for x in c["out"]], c


def _insert_norm(res):
    if res is None:
        return None
    return [list(res[0]), None if res[1] is None else list(res[1]), None if res[2] is None else list(res[2])]


def test_kats_insert(oracle):
    for c in load_golden("kats.json")["match_insert"]:
        orc = oracle.InsertOracle(c["a1"], c["a2"], **c["kw"])
        assert _insert_norm(orc.match_insert(c["r1"], c["r2"])) == c["out"], c


def test_locate_fuzz(oracle):
    cases = load_golden("locate_fuzz.json.gz")
    assert len(cases) == 6000
    for c in cases:
        got = oracle.locate(c["ref"], c["query"], c["e"], c["flags"], c["wr"], c["wq"], c["mo"], c["ic"])
        assert got == tup(c["out"]), c


def test_long_reads(oracle):
    from tests._cases import long_read_case
    cases = load_golden("long_reads.json.gz")
    assert len(cases) == 700
    for c in cases:
        got = oracle.locate(c["ref"], long_read_case(c), c["e"], c["flags"], c["wr"], c["wq"], c["mo"], c["ic"])
        assert got == tup(c["out"]), c


def test_long_pairs(oracle):
    from tests._cases import long_pair_case
    cases = load_golden("long_pairs.json.gz")
    assert len(cases) == 400
    for c in cases:
        ref, q = long_pair_case(c)
        assert oracle.locate(ref, q, c["e"], c["flags"], c["wr"], c["wq"], c["mo"], c["ic"]) == tup(c["out"]), c


def test_multi_fuzz(oracle):
    for c in load_golden("multi_fuzz.json.gz"):
        got = oracle.multi_locate(c["ref"], c["query"], c["e"], c["flags"], c["mo"], c["mx"])
        exp = None if c["out"] is None else [tup(x) for x in c["out"]]
        assert got == exp, c


def test_prefix_fuzz(oracle):
    for c in load_golden("prefix_fuzz.json.gz"):
        assert oracle.compare_prefixes(c["ref"], c["query"], c["wr"], c["wq"]) == tup(c["prefix"]), c
        assert oracle.compare_suffixes(c["ref"], c["query"], c["wr"], c["wq"]) == tup(c["suffix"]), c


def test_insert_fuzz(oracle):
    cache = {}
    for c in load_golden("insert_fuzz.json.gz") + load_golden("insert_long.json.gz"):
        key = (c["a1"], c["a2"], repr(sorted(c["kw"].items())))
        if key not in cache:
            cache[key] = oracle.InsertOracle(c["a1"], c["a2"], **c["kw"])
        assert _insert_norm(cache[key].match_insert(c["r1"], c["r2"])) == c["out"], c
    # pairs of 2 x 321 .. 600 bases (round 5): the C restatement takes them up to its own table width
    pinned = 0
    for c in load_golden("insert_longer.json.gz"):
        key = (c["a1"], c["a2"], repr(sorted(c["kw"].items())))
        if key not in cache:
            cache[key] = oracle.InsertOracle(c["a1"], c["a2"], **c["kw"])
        try:
            got = cache[key].match_insert(c["r1"], c["r2"])
        except (ValueError, OverflowError):
            continue
        assert _insert_norm(got) == c["out"], c
        pinned += 1
    assert pinned >= 40


def test_rmp_values(oracle):
    for k, size, p, q, rep in load_golden("rmp.json"):
        assert repr(oracle.rmp(k, size, p, q)) == rep, (k, size, p, q)


def test_synth_heads(oracle):
    """The synthetic workload generator reproduces the reads the golden outputs were
    computed on, and the oracle reproduces the reference's outputs on them."""
    from atropos_amd import synth
    heads = load_golden("synth_heads.json.gz")

    def rows(t):
        return [bytes(x.tolist()).decode("ascii") for x in t]

    for name in ("C1", "C2"):
        w = synth.workload(name, 0, heads[name]["count"])
        outs = [oracle.locate(w["adapter"], q, w["max_error_rate"], 14, False, False, w["min_overlap"],
                              w["indel_cost"]) for q in rows(w["reads"])]
        assert outs == [tup(x) for x in heads[name]["out"]]
        assert sum(o is not None for o in outs) > heads[name]["count"] // 3
    for name in ("C3", "C5"):
        w = synth.workload(name, 0, heads[name]["count"])
        orc = oracle.InsertOracle(w["adapter1"], w["adapter2"], **heads[name]["kw"])
        outs = [_insert_norm(orc.match_insert(a, b)) for a, b in zip(rows(w["reads1"]), rows(w["reads2"]))]
        assert outs == heads[name]["out"]


def test_oracle_linked_c4_head(oracle):
    """oracle.linked_many (Adapter.match_to + LinkedAdapter.match_to restated in C) on the head of
    the C4 read set against what the reference returned for it (synth_heads.json.gz)."""
    import numpy as np
    from atropos_amd import synth
    heads = load_golden("synth_heads.json.gz")["C4"]
    w = synth.workload("C4", 0, heads["count"])
    r = w["reads"].numpy()
    wh, f, b = oracle.linked_many(w["fronts"], w["backs"], r, np.full(len(r), 150, np.int32), w["max_error_rate"],
                                  w["min_overlap"], w["indel_cost"], True, False, 2)
    for i in range(len(r)):
        exp = heads["out"][i]
        hits = [a for a in range(4) if exp[a] is not None]
        assert int(wh[i, 0]) == (hits[0] if hits else -1) and int(wh[i, 1]) == len(hits)
        if hits:
            ef, eb = exp[hits[0]]
            assert list(f[i]) == ef
            assert (None if b[i, 1] < 0 else list(b[i])) == eb


def test_oracle_match_to_golden(oracle):
    """oracle.match_to against the reference's Adapter.match_to outputs (match_to_fuzz.json.gz), for
    the cases it restates: adapters with indels, no RMP filter."""
    cases = load_golden("match_to_fuzz.json.gz") + load_golden("kats.json")["match_to"]
    n = 0
    for c in cases:
        kw = c["kw"]
        if c.get("use_rmp") or not kw.get("indels", True):
            continue
        got = oracle.match_to(c["seq"].upper().replace("U", "T"), c["where"], c["read"], kw.get("max_error_rate", 0.1),
                              kw.get("min_overlap", 3), kw.get("indel_cost", 1), kw.get("adapter_wildcards", True),
                              kw.get("read_wildcards", False))
        assert (None if got is None else list(got)) == c["out"], c
        n += 1
    assert n > 1000


def test_oracle_linked_fuzz(oracle):
    """oracle.linked_many against the reference's LinkedAdapter.match_to results (linked_fuzz.json.gz)."""
    import numpy as np
    n = 0
    for c in load_golden("linked_fuzz.json.gz"):
        kw = c["kw"]
        width = max(len(q) for q in c["reads"])
        mat = np.zeros((len(c["reads"]), width), np.uint8)
        for i, q in enumerate(c["reads"]):
            mat[i, :len(q)] = np.frombuffer(q.encode(), np.uint8)
        lens = np.array([len(q) for q in c["reads"]], np.int32)
        wh, f, b = oracle.linked_many(c["fronts"], c["backs"], mat, lens, kw["max_error_rate"], kw["min_overlap"],
                                      kw["indel_cost"], True, kw["read_wildcards"], 2)
        for i, exp in enumerate(c["out"]):
            got = [int(wh[i, 0]), int(wh[i, 1]), None if f[i, 1] < 0 else [int(v) for v in f[i]],
                   None if b[i, 1] < 0 else [int(v) for v in b[i]]]
            assert got == exp, (c["fronts"], c["backs"], kw, c["reads"][i])
            n += 1
    assert n == 3840


def test_correct_errors_fuzz(oracle):
    """oracle.correct_errors (orc_correct_errors) against 4 000 reference runs of
    ErrorCorrectorMixin.correct_errors (tests/golden/make_round3_golden.py)."""
    cases = load_golden("correct_errors_fuzz.json.gz")
    assert len(cases) == 4000
    seen = set()
    for c in cases:
        try:
            s1, q1, s2, q2, ch = oracle.correct_errors(c["seq1"], c["qual1"], c["seq2"], c["qual2"], c["im"], c["action"],
                                                       c["mqd"], c["truncate"])
            got = dict(seq1=s1, qual1=q1, seq2=s2, qual2=q2, corrected=list(ch), pairs=int(ch[0] > 0 or ch[1] > 0), bp=list(ch))
        except (KeyError, IndexError, ValueError) as exc:
            got = dict(error=type(exc).__name__)
        assert got == c["out"], c
        seen.add(got.get("error", "ok"))
    assert seen == {"ok", "KeyError", "IndexError", "ValueError"}


def test_long_multi_and_compare(oracle):
    """the C restatement on the 737 .. 3 000-character cases of round 5 (reference outputs)"""
    g = load_golden("long_multi_compare.json.gz")
    for c in g["compare"]:
        k = 0
        for wr in (False, True):
            for wq in (False, True):
                exp_p, exp_s = c["out"][k]
                k += 1
                assert list(oracle.compare_prefixes(c["ref"], c["query"], wr, wq)) == exp_p
                assert list(oracle.compare_suffixes(c["ref"], c["query"], wr, wq)) == exp_s
    for c in g["multi"]:
        for r in c["runs"]:
            got = oracle.multi_locate(c["ref"], c["query"], r["e"], r["flags"], r["min_overlap"])
            assert (None if got is None else [list(t) for t in got]) == r["out"]


def test_qualtrim_fuzz(oracle):
    """quality_trim_index / nextseq_trim_index (_qualtrim.pyx:7-84) and NEndTrimmer (modifiers.py:766-784): the
    checker of SURVEY 8 row f4 against what the reference returned (make_round6_golden.py)."""
    cases = load_golden("qualtrim_fuzz.json.gz")["cases"]
    assert len(cases) == 3000
    trimmed = 0
    for c in cases:
        s, q = c["seq"], c["qual"]
        assert list(oracle.quality_trim_index(q, c["cf"], c["cb"], c["base"])) == c["qtrim"], c
        if s:
            assert oracle.nextseq_trim_index(s, q, c["cg"], c["base"]) == c["nextseq"], c
        a, b = oracle.n_end_trim(s)
        assert ([s[a:b], q[a:b]] if a < b else ["", ""]) == c["nend"], c
        trimmed += c["qtrim"] != [0, len(q)]
    assert trimmed > 1500


def test_locate_pairs_many_equals_locate(oracle):
    """locate_pairs_many (the threaded driver with a reference per pair, harness only) == locate pair by pair, on random
    overlapping and unrelated pairs of ragged lengths: every flag set of the callers, wildcards, indel costs, the
    reverse-complemented reference included, for 1, 3 and 16 threads; a base without complement raises as
    reverse_complement does."""
    import random
    import numpy as np
    import pytest
    from tests._cases import mutate, rseq
    rng = random.Random(2024)
    total = found = 0
    for rnd in range(48):
        npairs = rng.choice([1, 2, 97, 250])
        flags = rng.choice([15, 9, 14, 11, 0, 3])
        e, ic, mo = rng.choice([0.1, 0.2]), rng.choice([1, 2, 100000]), rng.choice([1, 3])
        rc = rnd % 2 == 0
        wr, wq = (rng.random() < 0.3, rng.random() < 0.3) if not rc else (False, False)
        alpha = "ACGTN" if (wr or wq or rc) else "ACGT"
        width = rng.choice([40, 150, 250])
        refs, queries = [], []
        for _ in range(npairs):
            m, n = rng.randint(0, width), rng.randint(0, width)
            frag = rseq(rng, m + n + 1, alpha)
            refs.append(frag[:m])
            queries.append(mutate(rng, frag[rng.randint(0, m):][:n], 0.05)[:n] if rng.random() < 0.8 else rseq(rng, n))
        stored = [oracle.reverse_complement(r) if rc else r for r in refs]      # what the caller holds: read 2 as sequenced
        rmat = np.full((npairs, width + 3), ord("#"), np.uint8)                 # bytes past a row's length are never read
        qmat = np.full((npairs, width), ord("#"), np.uint8)
        for i, (r, q) in enumerate(zip(stored, queries)):
            rmat[i, :len(r)] = np.frombuffer(r.encode(), np.uint8)
            qmat[i, :len(q)] = np.frombuffer(q.encode(), np.uint8)
        rl = np.array([len(r) for r in refs], np.int32)
        ql = np.array([len(q) for q in queries], np.int32)
        exp = np.zeros((npairs, 6), np.int32)
        exp[:, 1] = -1
        for i, (r, q) in enumerate(zip(refs, queries)):
            t = oracle.locate(r, q, e, flags, wr, wq, mo, ic)
            if t is not None:
                exp[i] = t
        for nthreads in (1, 3, 16):
            got = oracle.locate_pairs_many(rmat, rl, qmat, ql, e, flags, wr, wq, mo, ic, rc, nthreads)
            assert got.dtype == np.int32 and got.shape == (npairs, 6)
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert len(bad) == 0, (rnd, nthreads, int(bad[0]), refs[bad[0]], queries[bad[0]], got[bad[0]], exp[bad[0]])
        total += npairs
        found += int((exp[:, 1] >= 0).sum())
    assert total > 2000 and found > total // 3
    with pytest.raises(KeyError):
        oracle.locate_pairs_many(np.frombuffer(b"ACXT", np.uint8)[None, :], [4], np.frombuffer(b"ACGT", np.uint8)[None, :], [4],
                                 0.1, 15, revcomp_ref=True)

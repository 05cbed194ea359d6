"""Device-resident FASTQ pipeline on the real HIP kernels (through the C ABI): against the
output text of the reference's `atropos trim` command (committed golden cases), and -- at a
size where every kernel runs many blocks -- against the CPU twins of the kernels."""
import numpy as np
import pytest

from . import _cases

pytestmark = pytest.mark.gpu


def test_trim_pipeline_reference_cli_cases(hip_backend):
    assert _cases.check_trim_golden() >= 86


def test_trim_file_chunking(hip_backend, tmp_path):
    counts = _cases.check_fastq_chunking(tmp_path)
    assert counts["keep"] > 0 and counts["too_short"] > 0


def _big_fastq(nreads, seed):
    """nreads x 150 bp C2 reads with decaying qualities, ragged tails and N ends."""
    from atropos_amd import synth
    reads = synth.workload("C2", 0, nreads, device="cpu")["reads"].numpy()
    rng = np.random.RandomState(seed)
    n = reads.shape[1]
    qual = np.clip(38 - (np.arange(n)[None, :] * rng.uniform(0, 0.25, size=(nreads, 1))).astype(np.int64)
                   + rng.randint(-3, 4, size=(nreads, n)), 2, 40).astype(np.uint8) + 33
    lens = np.where(rng.rand(nreads) < 0.1, rng.randint(0, n + 1, size=nreads), n)
    nend = rng.rand(nreads) < 0.1
    parts = []
    for i in range(nreads):
        L = int(lens[i])
        seq = bytes(reads[i, :L])
        if nend[i] and L > 6:
            seq = b"NN" + seq[2:L - 3] + b"NNN"
        parts.append(b"@r%d len=%d\n%s\n+\n%s\n" % (i, L, seq, bytes(qual[i, :L])))
    return b"".join(parts)


@pytest.mark.parametrize("args", [
    "-a AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC -q 15,20 --trim-n -m 20",
    "-b AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC -n 2 --mask-adapter --max-n 0.2",
    "-a ^ACGT...AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC -e 0.15 -u 2 --discard-untrimmed",
    "-a AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC$ --no-indels -e 0.2 -g ^ACGTAC -n 2",     # packed compare_prefixes/suffixes
])
def test_large_batch_equals_cpu_twin(hip_backend, args):
    from atropos_amd import _lib
    from atropos_amd.trim import pipeline_from_args
    from tests.emu.backend import EmuBackend
    data = _big_fastq(70000, 5)          # (>= PLANES_MIN_READS: the 3' adapters go through the two-pass pre-pass, ragged)
    got = pipeline_from_args(args).trim_bytes(data)
    prev = _lib.set_backend(EmuBackend(), _test_double=True)
    planes_from, _lib.PLANES_MIN_READS = _lib.PLANES_MIN_READS, 1 << 60       # the twin: the one-pass pipeline on tile64
    try:
        want = pipeline_from_args(args).trim_bytes(data)
    finally:
        _lib.PLANES_MIN_READS = planes_from
        _lib.set_backend(prev, _test_double=True)
    assert len(got) == len(want) and got == want, _cases._first_diff(got, want)
    assert len(got) > 20000


def check_quality_trim_fixture():
    """Row f4 on the backend in place: every case of qualtrim_fuzz.json.gz (reference outputs) through the text pipeline --
    `-q cf,cb`, `--nextseq-trim cg`, `--trim-n`, grouped by their cutoffs and quality base.  Returns the cases run."""
    from atropos_amd.trim import pipeline_from_args
    from .conftest import load_golden
    cases = [c for c in load_golden("qualtrim_fuzz.json.gz")["cases"] if c["seq"] and min(map(ord, c["qual"])) >= 33]
    groups = {}
    for c in cases:
        if c["cf"] or c["cb"]:                                     # (`-q 0,0` alone is "no modifier at all": the command refuses it)
            groups.setdefault(("-q %d,%d --quality-base %d" % (c["cf"], c["cb"], c["base"]), "q"), []).append(c)
        groups.setdefault(("--nextseq-trim %d --quality-base %d" % (c["cg"], c["base"]), "g"), []).append(c)
        groups.setdefault(("--trim-n", "n"), []).append(c)
    ran = 0
    for (args, kind), cs in sorted(groups.items()):
        data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, c["seq"].encode(), c["qual"].encode()) for i, c in enumerate(cs))
        out = pipeline_from_args(args).trim_bytes(data).split(b"\n")
        assert len(out) == 4 * len(cs) + 1, args
        for i, c in enumerate(cs):
            s, q = c["seq"], c["qual"]
            if kind == "q":
                want = [s[c["qtrim"][0]:c["qtrim"][1]], q[c["qtrim"][0]:c["qtrim"][1]]]
            elif kind == "g":
                want = [s[:c["nextseq"]], q[:c["nextseq"]]]
            else:
                want = c["nend"]
            assert [out[4 * i + 1].decode(), out[4 * i + 3].decode()] == want, (args, c)
            ran += 1
    return ran


def test_quality_trim_fixture(hip_backend):
    assert check_quality_trim_fixture() > 7000


def check_slice_against_oracle(oracle, nrecords, step, args=""):
    """The at-size single-end text pipeline against a restatement that shares NO code with the kernels (round-4 verdict:
    the twin above is compiled from the same *_core.hpp), every `step`-th record: the modifiers in the reference's order
    (CGQA, then NEndTrimmer: commands/trim/__init__.py:422-519) -- nextseq_trim_index and quality_trim_index on the
    checker (_qualtrim.pyx:7-84; round-5 verdict item 7), Adapter.match_to restated on the oracle (literal shortcut,
    locate, acceptance test: adapters/__init__.py:338-400), AdapterCutter's trim (read[:rstart], modifiers.py:107-187),
    ^N+ / N+$ -- on the record's own text."""
    from atropos_amd import synth
    from atropos_amd.trim import pipeline_from_args
    adapter = synth.TRUSEQ_34
    data = _big_fastq(nrecords, 5)
    got = pipeline_from_args(("%s -a %s" % (args, adapter)).strip()).trim_bytes(data)
    src, out = data.split(b"\n"), got.split(b"\n")
    assert len(out) == len(src) and len(src) == 4 * nrecords + 1
    qt = "-q 15,20" in args
    trimmed = qtrimmed = 0
    for i in range(0, nrecords, step):
        name, seq, plus, qual = src[4 * i:4 * i + 4]
        seq, qual = seq.decode(), qual.decode()
        before = len(seq)
        if "--nextseq-trim 20" in args and seq:
            stop = oracle.nextseq_trim_index(seq, qual, 20)
            seq, qual = seq[:stop], qual[:stop]
        if qt and seq:
            a, b = oracle.quality_trim_index(qual, 15, 20)
            seq, qual = seq[a:b], qual[a:b]
        qtrimmed += len(seq) != before
        m = _cases.oracle_match_to(oracle, adapter, 14, seq, 0.1, 3, 1, False, False)
        if m is not None:
            seq, qual = seq[:m[2]], qual[:m[2]]
        trimmed += int(m is not None)
        if "--trim-n" in args and seq:
            a, b = oracle.n_end_trim(seq)
            seq, qual = (seq[a:b], qual[a:b]) if a < b else ("", "")
        assert out[4 * i:4 * i + 4] == [name, seq.encode(), plus, qual.encode()], (i, src[4 * i + 1], m, out[4 * i + 1])
    return trimmed, qtrimmed


@pytest.mark.parametrize("args", ["", "-q 15,20 --nextseq-trim 20 --trim-n"])
def test_large_batch_slice_against_oracle(hip_backend, oracle, args):
    """All 70 000 records of the at-size single-end text pipeline against the restatement (step 1).  The restatement
    trims the adapter from 31 349 records without the quality modifiers, from 23 495 with them, and the quality
    modifiers shorten 41 247: the bounds sit just below, so the input keeps exercising every stage."""
    trimmed, qtrimmed = check_slice_against_oracle(oracle, 70000, 1, args)
    assert trimmed > (23_000 if args else 31_000) and (not args or qtrimmed > 41_000)


def test_paired_pipeline_reference_cli_cases(hip_backend):
    assert _cases.check_trim_golden_paired() >= 47


def test_paired_file_chunking(hip_backend, tmp_path):
    counts = _cases.check_paired_file_chunking(tmp_path)
    assert counts["keep"] > 0 and counts["too_short"] > 0


def _big_pairs(npairs, seed):
    """npairs x (2 x 150 bp) C3 pairs with qualities, ragged lengths and N tails."""
    from atropos_amd import synth
    w = synth.workload("C3", 3, npairs, device="cpu")
    rng = np.random.RandomState(seed)
    texts = []
    # both reads of a pair cut to the same length: the reference's own correction raises on some
    # unequal-length pairs ("mode of an empty sequence"), and so does the device path
    lens = np.where(rng.rand(npairs) < 0.08, rng.randint(25, 151, size=npairs), 150)
    for reads in (w["reads1"].numpy(), w["reads2"].numpy()):
        n = reads.shape[1]
        qual = np.clip(38 - (np.arange(n)[None, :] * rng.uniform(0, 0.3, size=(npairs, 1))).astype(np.int64)
                       + rng.randint(-3, 4, size=(npairs, n)), 2, 40).astype(np.uint8) + 33
        parts = []
        for i in range(npairs):
            L = int(lens[i])
            seq = bytes(reads[i, :L])
            if rng.rand() < 0.1 and L > 8:
                seq = seq[:L - 4] + b"NNNN"
            parts.append(b"@p%d/x\n%s\n+\n%s\n" % (i, seq, bytes(qual[i, :L])))
        texts.append(b"".join(parts))
    return texts


@pytest.mark.parametrize("args", [
    "--aligner insert -a {a1} -A {a2} -R --merge-min-overlap 0.5 --correct-mismatches liberal",
    "-a {a1} -A {a2} -R --merge-min-overlap 20 --merge-error-rate 0.15 --correct-mismatches conservative -q 15 -m 20",
    "-R --merge-min-overlap 12 -u 2 -U 3 --trim-n",
])
def test_large_paired_merge_equals_cpu_twin(hip_backend, args):
    """MergeOverlapping as a device stage at a size where every kernel runs many blocks (the golden cases
    above pin the same code to the reference's output files)."""
    from atropos_amd import _lib, synth
    from atropos_amd.fastq import FastqBatch
    from atropos_amd.trim import pipeline_from_args
    from tests.emu.backend import EmuBackend
    args = args.format(a1=synth.PE_ADAPTER1, a2=synth.PE_ADAPTER2)
    d1, d2 = _big_pairs(30000, 9)

    def run():
        pipe = pipeline_from_args(args)
        b1, _ = FastqBatch.from_bytes(d1, final=True)
        b2, _ = FastqBatch.from_bytes(d2, final=True)
        res = pipe.run(b1, b2)
        return res.text() + (res.merged_text(),), res.counts()

    got, counts = run()
    prev = _lib.set_backend(EmuBackend(), _test_double=True)
    try:
        want, wcounts = run()
    finally:
        _lib.set_backend(prev, _test_double=True)
    assert counts == wcounts and counts["merged"] > 10000
    for g, w in zip(got, want):
        assert len(g) == len(w) and g == w, _cases._first_diff(g, w)


def _records(text):
    lines = text.split(b"\n")
    return {lines[k]: (lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)}


def check_merge_slice_against_oracle(oracle, npairs, every):
    """The paired text pipeline with the MergeOverlapping stage against a restatement that shares NO code with the
    kernels: `-u 2 -U 3` (UnconditionalCutter) then MergeOverlapping(12, 0.15) -- commands/trim/modifiers.py:864-931 --
    restated on the checker's Aligner.locate for every `every`-th pair: which file the pair lands in, the merged
    sequence and qualities."""
    from atropos_amd.fastq import FastqBatch
    from atropos_amd.trim import pipeline_from_args
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    d1, d2 = _big_pairs(npairs, 9)
    pipe = pipeline_from_args("-R --merge-min-overlap 12 --merge-error-rate 0.15 -u 2 -U 3")
    b1, _ = FastqBatch.from_bytes(d1, final=True)
    b2, _ = FastqBatch.from_bytes(d2, final=True)
    res = pipe.run(b1, b2)
    out1, out2 = (_records(t) for t in res.text())
    merged = _records(res.merged_text())
    src1, src2 = d1.split(b"\n"), d2.split(b"\n")
    nmerged = 0
    for i in range(0, npairs, every):
        name = src1[4 * i]
        s1, q1 = src1[4 * i + 1].decode()[2:], src1[4 * i + 3].decode()[2:]
        s2, q2 = src2[4 * i + 1].decode()[3:], src2[4 * i + 3].decode()[3:]
        exp = None
        if len(s1) >= 12 and len(s2) >= 12:
            rc2 = "".join(comp[c] for c in reversed(s2))
            rq2 = q2[::-1]
            al = oracle.locate(rc2, s1, 0.15, 15)
            if al is not None and al[4] >= 12:
                r2_start, r2_stop, r1_start, r1_stop = al[:4]
                if r2_start == 0 and r2_stop == len(s2):
                    exp = (s1, q1)
                elif r1_start == 0 and r1_stop == len(s1):
                    exp = (rc2, rq2)
                elif r1_start > 0:
                    exp = (s1 + rc2[r2_stop:], q1 + rq2[r2_stop:])
                else:
                    assert r2_start > 0
                    exp = (rc2 + s1[r1_stop:], rq2 + q1[r1_stop:])
        if exp is None:
            assert name not in merged and out1[name] == (s1.encode(), q1.encode()) and out2[name] == (s2.encode(), q2.encode()), i
        else:
            nmerged += 1
            assert name not in out1 and name not in out2 and merged[name] == (exp[0].encode(), exp[1].encode()), (i, al, merged.get(name), exp)
    return nmerged


def test_large_paired_merge_slice_against_oracle(hip_backend, oracle):
    """All 30 000 pairs of the paired text pipeline with the MergeOverlapping stage against the restatement (every = 1),
    which merges 28 881 of them."""
    assert check_merge_slice_against_oracle(oracle, 30000, 1) > 28_500


def test_fastq_reader_fuzz_vs_reference(hip_backend):
    total, errors = _cases.check_fastq_reader_golden()
    assert total == 300 and errors > 40

"""Device-resident FASTQ pipeline (index -> trim stages -> filters -> formatter) against the
output text of the reference's `atropos trim` command, with the device work done by the CPU
twins of the kernels (tests/emu/emu_fastq.cpp + the alignment emulation)."""
from . import _cases


def test_trim_pipeline_reference_cli_cases(emu_backend):
    assert _cases.check_trim_golden() >= 86


def test_trim_pipeline_through_the_two_pass_prepass(emu_backend, monkeypatch):
    """The same reference outputs with every batch, however short, packed as bit planes where the two-pass pre-pass
    takes the adapter (ragged batches: the reads come out of quality trimming / earlier adapters)."""
    from atropos_amd import _lib
    calls = []
    real = emu_backend.locate_planes_batch
    monkeypatch.setattr(_lib, "PLANES_MIN_READS", 1)
    monkeypatch.setattr(emu_backend, "locate_planes_batch", lambda *a: (calls.append(a[3]), real(*a))[1])
    assert _cases.check_trim_golden() >= 86
    assert len(calls) >= 10


def test_trim_file_chunking(emu_backend, tmp_path):
    counts = _cases.check_fastq_chunking(tmp_path)
    assert counts["keep"] > 0 and counts["too_short"] > 0


def test_pipeline_rejects_what_it_does_not_cover(emu_backend):
    import pytest
    from atropos_amd.trim import pipeline_from_args
    pipe = pipeline_from_args("-g ^ACGTACGT --no-indels")                # anchored without indels: compare_prefixes path
    assert pipe.trim_bytes(b"@r\nACGTACGTAA\n+\nIIIIIIIIII\n") == b"@r\nAA\n+\nII\n"
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a AAAA...TTTT -a GGGG")                     # linked + plain adapters mixed
    with pytest.raises(SystemExit):
        pipeline_from_args("-a ACGT --trim-primer")                      # modifier outside the pipeline
    with pytest.raises(NotImplementedError):
        pipeline_from_args("--aligner insert -a ACGTACGTAC -A ACGTACGTAC --length-tag length=")   # not with the insert aligner
    with pytest.raises(NotImplementedError):
        pipeline_from_args("-a ^ACGT...TTTT --info-file x")             # info file with a linked adapter


def test_paired_pipeline_reference_cli_cases(emu_backend):
    assert _cases.check_trim_golden_paired() >= 47


def test_paired_file_chunking(emu_backend, tmp_path):
    counts = _cases.check_paired_file_chunking(tmp_path)
    assert counts["keep"] > 0 and counts["too_short"] > 0


def test_fastq_reader_fuzz_vs_reference(emu_backend):
    total, errors = _cases.check_fastq_reader_golden()
    assert total == 300 and errors > 40


def test_paired_merge_slice_against_oracle(emu_backend, oracle):
    """MergeOverlapping restated on the checker (no code shared with the kernels) -- the CPU-tier size of
    tests/test_gpu_fastq.py::test_large_paired_merge_slice_against_oracle"""
    from .test_gpu_fastq import check_merge_slice_against_oracle
    assert check_merge_slice_against_oracle(oracle, 400, 2) > 150


def test_quality_trim_fixture(emu_backend):
    """Row f4 against the reference's outputs (qualtrim_fuzz.json.gz) -- CPU-tier twin of the GPU test of the same name"""
    from .test_gpu_fastq import check_quality_trim_fixture
    assert check_quality_trim_fixture() > 7000


def test_batch_slice_against_oracle_with_quality_trimming(emu_backend, oracle):
    from .test_gpu_fastq import check_slice_against_oracle
    trimmed, qtrimmed = check_slice_against_oracle(oracle, 3000, 1, "-q 15,20 --nextseq-trim 20 --trim-n")
    assert trimmed > 800 and qtrimmed > 1000


def test_chunked_reader_read_ahead_and_carry(emu_backend, tmp_path):
    """ChunkedFastqReader (round 6: file reads run READ_AHEAD chunks ahead of the carry): every record comes out once and
    in order -- over more chunks than staging buffers, with a caller that takes fewer records than a chunk holds (the
    surplus is carried over, as in a paired run), with records left over when the file is exhausted, and with a last line
    that has no line end."""
    import numpy as np
    from atropos_amd.fastq import ChunkedFastqReader
    rng = np.random.default_rng(11)
    recs = []
    for i in range(700):
        n = int(rng.integers(20, 90))
        seq = "".join("ACGT"[k] for k in rng.integers(0, 4, n))
        recs.append("@read%d some text\n%s\n+\n%s\n" % (i, seq, "I" * n))
    text = "".join(recs)[:-1]                                  # (no line end behind the last quality line)
    path = tmp_path / "in.fastq"
    path.write_bytes(text.encode())
    for take_all in (True, False):
        reader = ChunkedFastqReader(str(path), 4096, emu_backend)
        assert len(reader.buf) == ChunkedFastqReader.READ_AHEAD + 1
        got, chunks = [], 0
        try:
            while True:
                batch = reader.next_batch()
                chunks += 1
                if take_all:
                    head, consumed = batch, None
                else:                                           # two records fewer than the chunk holds, when it has them
                    head, consumed = batch.head(max(len(batch) - 2, min(len(batch), 1)))
                data = bytes(head.data[:head.nbytes].cpu().numpy().tobytes())
                nrec = len(head)
                end = reader.consumed if consumed is None else consumed
                got.append(data[:end])
                assert data[:end].count(b"\n") == 4 * nrec
                if reader.advance(consumed):
                    break
                assert chunks < 400
        finally:
            reader.close()
        assert chunks > 2 * (ChunkedFastqReader.READ_AHEAD + 1)
        assert b"".join(got) == (text + "\n").encode()


def _fastq_text(n, min_len, max_len, seed, eol="\n", tag=""):
    import numpy as np
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        m = int(rng.integers(min_len, max_len + 1))
        seq = "".join("ACGT"[k] for k in rng.integers(0, 4, m))
        recs.append("@read%d%s\n%s\n+\n%s\n" % (i, tag, seq, "I" * m))
    return "".join(recs).replace("\n", eol).encode()


def _chunk_records(batch):
    return [(name, seq, qual) for name, seq, qual, _ in batch.to_records()]


def _text_records(text):
    lines = text.replace(b"\r\n", b"\n").decode().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def test_read_chunks_one_file(emu_backend, tmp_path):
    """fastq.read_chunks over one file in many small chunks: every record once and in order, with "\\n" and
    "\\r\\n" line ends and with a last record that has no line end."""
    from atropos_amd.fastq import read_chunks
    for k, (eol, cut) in enumerate((("\n", 0), ("\r\n", 0), ("\n", 1), ("\r\n", 2))):
        text = _fastq_text(500, 20, 90, 3 + k, eol)
        text = text[:len(text) - cut]                          # (cut: the last line end is missing)
        path = tmp_path / ("in%d.fastq" % k)
        path.write_bytes(text)
        got, chunks = [], 0
        for batches in read_chunks([str(path)], 4096, emu_backend):
            assert len(batches) == 1
            got += _chunk_records(batches[0])
            chunks += 1
        assert chunks > 8
        assert got == _text_records(text)
        assert len(got) == 500


def test_read_chunks_two_files_in_lock_step(emu_backend, tmp_path):
    """Short R1 records next to R2 records of more than twice their size: every pair of batches holds the same
    number of records and nothing is lost."""
    from atropos_amd.fastq import read_chunks
    text1, text2 = _fastq_text(600, 20, 40, 5, tag="/1"), _fastq_text(600, 150, 250, 6, tag="/2")
    assert len(text2) > 2 * len(text1)
    paths = [str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq")]
    for p, t in zip(paths, (text1, text2)):
        open(p, "wb").write(t)
    got1, got2, chunks = [], [], 0
    for b1, b2 in read_chunks(paths, 8192, emu_backend):
        assert len(b1) == len(b2)
        got1 += _chunk_records(b1)
        got2 += _chunk_records(b2)
        chunks += 1
    assert chunks > 8
    assert got1 == _text_records(text1) and got2 == _text_records(text2)
    assert len(got1) == len(got2) == 600


def test_read_chunks_unequal_record_counts(emu_backend, tmp_path):
    """Two files with different numbers of records are a ValueError: when the shorter file ends many chunks before
    the other, and when both end in the same chunk."""
    import pytest
    from atropos_amd.fastq import read_chunks
    full = _fastq_text(400, 50, 60, 7)
    ends = [i + 1 for i, c in enumerate(full) if c == 10][3::4]             # the byte behind every record
    paths = [str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq")]
    open(paths[0], "wb").write(full)
    for nrec, chunk_bytes, chunks_before in ((150, 4096, 4), (399, 4096, 4), (399, 1 << 20, 0)):
        open(paths[1], "wb").write(full[:ends[nrec - 1]])
        seen = 0
        with pytest.raises(ValueError, match="^the two input files hold different numbers of records$"):
            for b1, b2 in read_chunks(paths, chunk_bytes, emu_backend):
                assert len(b1) == len(b2)
                seen += 1
        assert seen >= chunks_before
    for order in (paths, paths[::-1]):                         # (both files whole in one chunk, either one short)
        with pytest.raises(ValueError, match="different numbers of records"):
            for _ in read_chunks(order, 1 << 20, emu_backend):
                raise AssertionError("a chunk of files that do not match was handed out")


def test_read_chunks_closes_the_readers_when_the_consumer_leaves(emu_backend, tmp_path, monkeypatch):
    """A consumer that breaks out of the loop (or raises in it) leaves no reader open: staging buffers handed back,
    file closed."""
    import pytest
    from atropos_amd import fastq
    made = []

    class Recorded(fastq.ChunkedFastqReader):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(fastq, "ChunkedFastqReader", Recorded)
    paths = [str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq")]
    for k, p in enumerate(paths):
        open(p, "wb").write(_fastq_text(500, 30, 80, 8 + k))
    for batches in fastq.read_chunks(paths, 4096, emu_backend):
        assert len(made) == 2 and all(r.buf and not r.file.closed for r in made)
        break
    assert len(made) == 2 and all(r.buf == [] and r.file.closed for r in made)
    del made[:]
    with pytest.raises(KeyError):
        for batches in fastq.read_chunks(paths[:1], 4096, emu_backend):
            raise KeyError("the consumer fails")
    assert len(made) == 1 and made[0].buf == [] and made[0].file.closed


def test_read_chunks_byte_ranges(emu_backend, tmp_path):
    """A byte range of shard.fastq_shard_ranges yields the records of that range and no other, for every shard of a
    3-way split and for an empty shard; compressed input has no byte ranges."""
    import gzip
    import pytest
    from atropos_amd.fastq import read_chunks
    from atropos_amd.shard import fastq_shard_ranges
    text = _fastq_text(700, 20, 90, 10)
    path = str(tmp_path / "in.fastq")
    open(path, "wb").write(text)
    ranges = fastq_shard_ranges(path, 3)
    assert all(hi > lo for lo, hi in ranges)
    whole = []
    for lo, hi in ranges + [(ranges[1][0], ranges[1][0]), (len(text), len(text))]:
        got, chunks = [], 0
        for (batch,) in read_chunks([path], 4096, emu_backend, byte_ranges=[(lo, hi)]):
            got += _chunk_records(batch)
            chunks += 1
        assert got == _text_records(text[lo:hi])
        assert chunks > 3 if hi > lo else (chunks == 1 and got == [])
        whole += got
    assert whole == _text_records(text)
    # a file of one long record split four ways: the shards behind the first are empty
    long_path = str(tmp_path / "long.fastq")
    open(long_path, "wb").write(b"@r\n" + b"A" * 3000 + b"\n+\n" + b"I" * 3000 + b"\n")
    counts = [sum(len(b) for (b,) in read_chunks([long_path], 4096, emu_backend, byte_ranges=[r]))
              for r in fastq_shard_ranges(long_path, 4)]
    assert sorted(counts) == [0, 0, 0, 1]
    gz = str(tmp_path / "in.fastq.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(text)
    with pytest.raises(ValueError):
        next(read_chunks([gz], 4096, emu_backend, byte_ranges=[(0, 100)]))

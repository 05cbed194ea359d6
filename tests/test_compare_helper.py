"""_cases.assert_records_equal -- the comparison every whole-set GPU test goes through -- on arrays of the sizes and
shapes those tests hand it: one altered field in one row must be found and named, whichever row it is.  No GPU."""
import numpy as np
import pytest

from . import _cases

N = 1_000_003                      # (not a multiple of anything a strided or blocked comparison would step by)

SHAPES = [
    ("locate records [n, 6]", (N, 6), np.int32),
    ("insert records [n, 3, 6]", (N, 3, 6), np.int32),
    ("which / count [n]", (N,), np.int32),
    ("changed / newlen [n, 2]", (N, 2), np.int32),
    ("bases / qualities [n, 250]", (N, 250), np.uint8),
]


def _array(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, shape)]
    return rng.integers(-1, 151, shape).astype(dtype)


@pytest.mark.parametrize("label,shape,dtype", SHAPES, ids=[s[0] for s in SHAPES])
def test_one_altered_field_is_found_and_named(label, shape, dtype):
    exp = _array(shape, dtype, 7)
    got = exp.copy()
    assert _cases.assert_records_equal(got, exp, label) == N
    inner = shape[1:]
    fields = [tuple(0 for _ in inner), tuple(d - 1 for d in inner), tuple(d // 2 for d in inner)]
    for base in (0, 5_000_000):
        for row, field in zip((0, N - 1, N // 2 + 1), fields):
            at = (row,) + field
            keep = got[at]
            got[at] = keep + 1
            with pytest.raises(AssertionError) as err:
                _cases.assert_records_equal(got, exp, label, base=base)
            text = str(err.value)
            assert text.startswith("%s: 1 of %d rows differ, the first at %d\n" % (label, N, base + row)), text[:200]
            rows = [ln for ln in text.split("\n")[1:] if ln.startswith("  row ")]
            assert len(rows) == 1 and rows[0].startswith("  row %d: got " % (base + row)), rows
            assert str(got[row].tolist()) in rows[0] and str(exp[row].tolist()) in rows[0]
            got[at] = keep
            assert _cases.assert_records_equal(got, exp, label, base=base) == N


def test_several_rows_and_the_read_text():
    exp = _array((N, 6), np.int32, 3)
    got = exp.copy()
    reads = _array((N, 150), np.uint8, 4)
    lens = np.full(N, 150, np.int32)
    bad = [17, 4_096, 65_536, 500_000, 777_777, 999_999, N - 1]
    for k, row in enumerate(bad):
        got[row, k % 6] ^= 1
    lens[17] = 31
    with pytest.raises(AssertionError) as err:
        _cases.assert_records_equal(got, exp, "many", reads, lens, base=2_500_000)
    lines = str(err.value).split("\n")
    assert lines[0] == "many: 7 of %d rows differ, the first at %d" % (N, 2_500_017)
    assert [ln.split(":")[0] for ln in lines[1:6]] == ["  row %d" % (2_500_000 + r) for r in bad[:5]]
    assert lines[6] == "  read 2500017: " + bytes(reads[17, :31]).decode() and len(lines) == 7
    # without lens the whole row is the read
    with pytest.raises(AssertionError) as err:
        _cases.assert_records_equal(got, exp, "many", reads)
    assert str(err.value).split("\n")[6] == "  read 17: " + bytes(reads[17]).decode()


def test_dtype_and_shape_mismatches_are_rejected():
    a = _array((1000, 6), np.int32, 1)
    _cases.assert_records_equal(a, a.copy(), "same")
    for other in (a.astype(np.int16), a.astype(np.int64), a[:, :5], a[:999], a[:1], a[0], a[:, :1], a.reshape(1000, 6, 1),
                  np.concatenate([a, a[:, :2]], axis=1), a.tolist(), None):
        with pytest.raises(AssertionError):
            _cases.assert_records_equal(other, a, "mismatch")
        with pytest.raises(AssertionError):
            _cases.assert_records_equal(a, other, "mismatch")
    one = np.zeros(1000, np.int32)
    with pytest.raises(AssertionError):
        _cases.assert_records_equal(one, np.zeros((1000, 1), np.int32), "1-D against a column")
    with pytest.raises(AssertionError):
        _cases.assert_records_equal(np.int32(0), np.int32(0), "no row axis")
    with pytest.raises(AssertionError):
        _cases.assert_records_equal(a, a.copy(), "reads of another batch", reads=np.zeros((999, 150), np.uint8))
    assert _cases.assert_records_equal(a[:0], a[:0].copy(), "empty") == 0

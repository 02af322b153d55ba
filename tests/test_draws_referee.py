"""CPU: the numpy restatement of the device draws' contract (tests/draws_ref.py) against what does not depend on it -- the
published known answers of Philox4x32-10, the set properties of a draw without replacement, and the distributions the contract
promises, deterministic at a fixed seed.  The chi-square bars are 99.9 % quantiles: a correct restatement exceeds one of them at
a given seed once in a thousand."""
import numpy as np
import pytest

import draws_ref as R

SEED = 0x5EEDFACE12345678


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = R.philox4x32(np.array(ctr), np.array(key))
        assert " ".join("%08x" % int(v) for v in got) == want
    # vectorised = one at a time
    ctr = np.array([k[0] for k in kat]); key = np.array([k[1] for k in kat])
    got = R.philox4x32(ctr, key)
    assert [" ".join("%08x" % int(v) for v in row) for row in got] == [k[2] for k in kat]


@pytest.mark.parametrize("n,N", [(1, 1), (16, 8), (17, 17), (1000, 64), (4097, 1024), (70001, 2048)])
def test_rows_without_replacement_are_distinct_and_in_range(n, N):
    row = R.choice_row(SEED, 3, 5, n, N)
    assert row.dtype == np.int32 and row.shape == (N,)
    assert row.min() >= 0 and row.max() < n and len(set(row.tolist())) == N


def test_rows_with_replacement_are_in_range_and_bad_rows_are_zero():
    row = R.choice_row(SEED, 3, 5, 5, 64)
    assert row.min() >= 0 and row.max() < 5 and len(set(row.tolist())) == 5
    assert (R.choice_row(SEED, 3, 5, 1, 4) == 0).all()
    for n in (0, -3, 2 ** 31):
        assert (R.choice_row(SEED, 0, 0, n, 8) == 0).all()
    assert R.draw(SEED, 0, [4, 0, 9], 8)[4] == 1 and R.draw(SEED, 0, [4, 9], 8)[4] == 0


def test_same_counter_same_row_other_counter_other_row():
    a = R.choice_row(SEED, 7, 2, 500, 64)
    assert (a == R.choice_row(SEED, 7, 2, 500, 64)).all()
    for other in (R.choice_row(SEED, 8, 2, 500, 64), R.choice_row(SEED, 7, 3, 500, 64), R.choice_row(SEED + 1, 7, 2, 500, 64),
                  R.choice_row(SEED, 7 + 2 ** 32, 2, 500, 64), R.choice_row(SEED + 2 ** 32, 7, 2, 500, 64)):
        assert (a != other).any()
    s = R.scalars_row(SEED, 7, 2)
    assert s == R.scalars_row(SEED, 7, 2) and s != R.scalars_row(SEED, 8, 2) and s != R.scalars_row(SEED, 7, 3)
    assert R.scalars_row(SEED, 7, 2, False, False) == (0.0, 0.0, 0.5)
    assert R.scalars_row(SEED, 7, 2, True, False) == (s[0], 0.0, 0.5)
    assert 0.0 <= s[0] < 1.0 and 0.0 <= s[2] < 1.0 and abs(s[1]) <= 8.6


def test_composition_goes_through_sub():
    sub = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108, 7, 8, 9], dtype=np.int32)
    off = np.array([0, 9, 9, 12])
    ch = R.draw(SEED, 1, [50, 50, 50], 4, sub=sub, sub_off=off)[0]
    assert set(ch[0].tolist()) <= set(range(100, 109)) and (ch[0] == sub[R.choice_row(SEED, 1, 0, 9, 4)]).all()
    assert (ch[1] == R.choice_row(SEED, 1, 1, 50, 4)).all()
    assert (ch[2] == sub[9 + R.choice_row(SEED, 1, 2, 3, 4)]).all() and set(ch[2].tolist()) <= {7, 8, 9}


# ---- distribution: M = 8192 (step, b) draws, 256 steps x 32 rows
M_STEPS, M_ROWS = 256, 32
M = M_STEPS * M_ROWS


def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def _wilson_hilferty_999(df):
    return df * (1.0 - 2.0 / (9.0 * df) + 3.0902 * np.sqrt(2.0 / (9.0 * df))) ** 3


@pytest.fixture(scope="module")
def draws_16_8():
    return np.stack([R.choice_row(SEED, s, b, 16, 8) for s in range(M_STEPS) for b in range(M_ROWS)])


def test_first_position_is_uniform(draws_16_8):
    c = np.bincount(draws_16_8[:, 0], minlength=16)
    x = _chi2(c, M / 16.0)
    print("chi2 first position (df 15):", x)
    assert x < 37.70


def test_first_two_positions_are_uniform_over_ordered_pairs(draws_16_8):
    a, b = draws_16_8[:, 0].astype(np.int64), draws_16_8[:, 1].astype(np.int64)
    assert (a != b).all()
    c = np.bincount(a * 16 + b, minlength=256).reshape(16, 16)
    assert (np.diag(c) == 0).all()
    x = _chi2(c[~np.eye(16, dtype=bool)], M / 240.0)
    bar = _wilson_hilferty_999(239.0)
    print("chi2 ordered pairs (df 239):", x, "bar", bar)
    assert x < bar


def test_first_position_with_replacement_is_uniform():
    d = np.stack([R.choice_row(SEED, s, b, 5, 8) for s in range(M_STEPS) for b in range(M_ROWS)])
    x = _chi2(np.bincount(d[:, 0], minlength=5), M / 5.0)
    print("chi2 with replacement (df 4):", x)
    assert x < 18.47                              # the 99.9 % quantile at 4 degrees of freedom


def test_coin_is_uniform_and_normal_is_standard():
    s = np.array([R.scalars_row(SEED, st, b) for st in range(M_STEPS) for b in range(M_ROWS)])
    x = _chi2(np.bincount((s[:, 0] * 16).astype(np.int64), minlength=16), M / 16.0)
    print("chi2 coin (df 15):", x, "normal mean", s[:, 1].mean(), "var", s[:, 1].var())
    assert x < 37.70
    assert abs(s[:, 1].mean()) < 4.0 / np.sqrt(M)
    assert abs(s[:, 1].var() - 1.0) < 4.0 * np.sqrt(2.0 / M)
    xh = _chi2(np.bincount((s[:, 2] * 16).astype(np.int64), minlength=16), M / 16.0)
    assert xh < 37.70

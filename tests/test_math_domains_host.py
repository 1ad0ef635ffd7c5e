"""The device-math sweeps, host side (no GPU): (a) the comparison harness finds a planted one-bit
difference and nothing else; (b) the grids of tests/math_domains.py are what they say -- sizes,
domains, NaNs, exact hard cases; (c) the oracle's accuracy on these grids against numpy.longdouble
(64-bit mantissa), under the project's own bounds (tests/test_oracle_c.py).  The device's
side of the same grids is tests/test_gpu_math_domains.py."""
import numpy as np
import pytest

from oracle import cbind as O
from tests import math_domains as D

LD = np.longdouble
PI_LD = LD(3) + LD("0.1415926535897932384626433832795028841971")
LN2_LD = LD("0.6931471805599453094172321214581765680755")


# --------------------------------------------------------------------------- (a) the harness
def test_the_harness_reports_exactly_the_planted_difference():
    g = D.log_sums()
    want = g.oracle()
    assert D.differences(g.args(), want, want) is None
    got = want.copy()
    at = 123457
    got[at] ^= np.uint64(1)
    count, first, message = D.differences(g.args(), got, want)
    assert (count, first) == (1, at)
    assert f"0x{int(g.args()[at, 0]):016x}" in message and f"0x{int(got[at]):016x}" in message
    assert f"0x{int(want[at]):016x}" in message and "1 of" in message
    with pytest.raises(AssertionError, match=f"first at index {at}"):
        D.assert_same_words(g, got, want)


def test_the_harness_counts_every_difference_and_names_the_first():
    g = D.sincos_grid()
    want = g.oracle()
    got = want.copy()
    got[[77, 5000, 5001], [1, 0, 1]] ^= np.uint64(1)      # (two-word results: sin or cos alone)
    count, first, message = D.differences(g.args(), got, want)
    assert (count, first) == (3, 77) and f"0x{int(g.args()[77, 0]):016x}" in message


def test_generated_arguments_are_the_written_out_ones():
    g = D.neg_log_short_29(15)
    a = g.args()[:, 0]
    assert a[0] == 15 * (1 << 25) + 1 and a[-1] == (1 << 29) - 1 and np.all(a & np.uint64(1))
    small = D.Grid("neg_log_short_29", first=g.first, stride=2, n=1000)
    assert np.array_equal(small.oracle(), O.math_bulk("neg_log_short_29", small.args()))
    assert D.dbl(small.oracle()[:1])[0] == O.neg_log_short(int(a[0]), 29)


def test_bulk_forms_equal_the_scalar_functions_and_are_thread_invariant():
    x = D.dbl(D.log_sums().words[:500, 0])
    assert np.array_equal(D.dbl(O.math_bulk("dlog", D.bits(x))), [O.dlog(v) for v in x])
    assert np.array_equal(D.dbl(O.math_bulk("dlog_tab", D.bits(x))), [O.dlog_tab(v) for v in x])
    assert np.array_equal(D.dbl(O.math_bulk("dexp", D.bits(-x))), [O.dexp(-v) for v in x])
    assert np.array_equal(D.dbl(O.math_bulk("dexp_tab", D.bits(-x))), [O.dexp_tab(-v) for v in x])
    k = D.sincos_grid().words[:200]
    assert np.array_equal(D.dbl(O.math_bulk("sincos2pi", k)), [O.sincos2pi(int(v)) for v in k[:, 0]])
    g = D.philox_grid()
    out = g.oracle()
    for i, (key, answer) in enumerate(D.PHILOX_KNOWN):
        assert tuple(int(v) for v in g.words[i]) == key and tuple(int(v) for v in out[i]) == answer
    assert np.array_equal(out, g.oracle(n_threads=3))
    with pytest.raises(ValueError):
        O.math_bulk("div", None, n=4)                      # two words cannot be generated


# --------------------------------------------------------------------------- (b) the grids
def test_grid_sizes_are_as_stated():
    assert D.neg_log_short_25().n == 1 << 24
    assert sum(D.neg_log_short_29(c).n for c in range(16)) == 1 << 28
    assert D.sqrt_call_site().n == 1 << 24 and D.sqrt_tail().n == 1 << 20
    assert D.sqrt_contract().n == 200 * 67 + 1
    assert D.sqrt_hard_boundary().n == 1 << 20 and D.sqrt_hard_representable().n == 1 << 20
    assert D.log_exponents().n == 2046 * (3 + 3 + 3 * 128 + 16)
    assert D.log_uniforms().n == 4 + (1 << 21) and D.log_sums().n == 1 << 20
    assert D.exp_specials().n == len(D.EXP_SPECIALS) == 9
    assert D.exp_ties_ln2().n == 5 * (2 * 1021 + 1) and D.exp_ties_ln2_64().n == 5 * (2 * 65344 + 1)
    assert D.exp_uniform().n == 1 << 21 and D.exp_log_uniform().n == 1 << 20
    assert D.sincos_grid().n == 24 + (1 << 21)
    assert len(D.div_widths()) == 7 + 32 and D.div_grid().n == 39 * D.DIV_PER_WIDTH
    assert D.philox_grid().n == 3 + 64 + (1 << 20) and D.u52_grid().n == 6 + (1 << 20)


def test_short_logarithm_chunks_tile_every_odd_argument_once():
    firsts = [D.neg_log_short_29(c).first for c in range(16)]
    assert firsts == [1 + c * (1 << 25) for c in range(16)]
    assert all(D.neg_log_short_29(c).stride == 2 for c in range(16))
    assert D.neg_log_short_29(15).first + 2 * ((1 << 24) - 1) == (1 << 29) - 1
    g = D.neg_log_short_25()
    assert (g.first, g.stride, g.first + 2 * (g.n - 1)) == (1, 2, (1 << 25) - 1)


def test_every_value_is_inside_its_stated_domain():
    for g in D.sqrt_grids():
        x = D.dbl(g.words[:, 0])
        assert np.all((x >= 2.0 ** D.SQRT_LO_EXP) & (x <= 2.0 ** D.SQRT_HI_EXP)), g.label
    x = D.dbl(D.sqrt_call_site().words[:, 0])
    assert x.min() == 2.0 * O.neg_log_short((1 << 25) - 1, 25) > 2.0 ** -25 and x.max() == 2.0 * O.neg_log_short(1, 25) < 35.0
    x = D.dbl(D.sqrt_tail().words[:, 0])
    assert x.min() > 2 * 24 * 0.693 and x.max() < 2 * (24 + 53) * 0.6932
    e = np.frexp(D.dbl(D.sqrt_contract().words[:, 0]))[1] - 1
    assert set(e.tolist()) == set(range(-100, 101))
    for g in (D.log_exponents(), D.log_uniforms(), D.log_sums()):
        x = D.dbl(g.words[:, 0])
        assert np.all(np.isfinite(x) & (x >= 2.0 ** -1022)), g.label      # positive normal
    w = D.log_exponents().words[:, 0]
    assert set((w >> np.uint64(52)).tolist()) == set(range(1, 2047))
    frac = set((w[:406] & np.uint64(D.FRAC)).tolist())
    assert {0, 1, D.FRAC, D.LOG_THRESHOLD_FRAC - 1, D.LOG_THRESHOLD_FRAC} <= frac
    assert all(((j << 45) + s) & D.FRAC in frac for j in range(128) for s in (-1, 0, 1))
    # fdlibm's threshold: the reduction halves the mantissa from this fraction on
    assert ((D.LOG_THRESHOLD_FRAC >> 32) + 0x95F64) & 0x100000 and not (((D.LOG_THRESHOLD_FRAC - 1) >> 32) + 0x95F64) & 0x100000
    x = D.dbl(D.log_uniforms().words[:, 0])
    assert x.min() == 2.0 ** -53 and x.max() == 1 - 2.0 ** -53
    x = D.dbl(D.log_sums().words[:, 0])
    assert x.min() == 2.0 ** -10 and x.max() == 16.0
    x = D.dbl(D.log_subnormals().words[:, 0])
    assert np.all((x >= 0) & (x < 2.0 ** -1022))
    for g in (D.exp_ties_ln2(), D.exp_ties_ln2_64(), D.exp_uniform(), D.exp_log_uniform()):
        x = D.dbl(g.words[:, 0])
        assert np.all((x >= -708.0) & (x <= 0.0)), g.label
    x = D.dbl(D.exp_log_uniform().words[:, 0])
    assert x.max() <= -1e-12 and x.min() < -700 and x.max() > -1e-11
    x = D.dbl(D.exp_positive().words[:, 0])
    assert np.all((x > 0) & (x <= D.EXP_CLAMP)) and x.max() == D.EXP_CLAMP
    k = D.sincos_grid().words[:, 0]
    assert k.max() < (1 << 52) and set((k >> np.uint64(49)).tolist()) == set(range(8))
    assert D.u52_grid().words.max() < (1 << 52) and D.philox_grid().words.max() < (1 << 32)
    a, w, r = (D.dbl(D.div_grid().words[:, i]) for i in range(3))
    assert np.all(np.abs(a) <= 8 * w * (1 + 2.0 ** -52)) and np.array_equal(r, 1.0 / w)
    assert np.all((a == 0) | (np.abs(a) >= 2.0 ** -100 * w))
    rand = D.div_widths()[7:]
    assert np.all((rand >= 2.0 ** -20) & (rand < 2.0 ** 20)) and D.div_widths()[6] == 2450000.1 - 2450000.0


def test_the_rint_ties_meet_both_signs_of_the_table_index_and_of_the_shift():
    x = D.dbl(D.exp_ties_ln2_64().words[:, 0])
    k = np.rint(x * (64.0 / D.LN2)).astype(np.int64)
    assert set((k & 63).tolist()) == set(range(64))
    assert (k >> 6).min() == -1021 and (k >> 6).max() == 0 and k.min() == -65344
    # each integer and each half-integer is met from both sides
    q = D.dbl(D.exp_ties_ln2().words[:, 0]) / D.LN2
    for target in (-3.0, -3.5, -1020.5):
        assert (q < target).any() and (q > target).any() and np.abs(q - target).min() < 1e-12


def test_no_nan_except_the_listed_one():
    for g in D.sqrt_grids() + D.dlog_grids() + D.dexp_grids()[1:] + [D.div_grid()]:
        assert not np.isnan(D.dbl(g.words)).any(), g.label
    assert np.flatnonzero(np.isnan(D.dbl(D.exp_specials().words[:, 0]))).tolist() == [D.EXP_SPECIALS.index("NaN")]
    x = D.dbl(D.exp_specials().words[:, 0])
    assert x[3] == -708.0 and x[4] < -708.0 < x[5] and x[6] == -709.0 and x[7] == -np.inf
    assert np.signbit(x[0]) and x[0] == 0 and x[1] == -(2.0 ** -1074) and x[2] == -1e-300


def test_the_hard_cases_of_the_square_root_are_exact():
    """In Python integers, with X = x 2^(104 - 2 t): |X - (y + 1/2)^2| <= ulp(X) / 2 (X is the rounding
    of the square of the midpoint), and ulp(X) / 2 <= |X - y^2| <= 3 ulp(X) / 2 on the drawn side (X is
    one ulp from the rounding of y^2).  Both exponent parities occur."""
    y, t, sign = D.sqrt_hard_y()
    assert all((1 << 52) <= int(v) < (1 << 53) for v in y[:1000]) and len(y) == 1 << 20
    sub = np.r_[0:20000, (1 << 20) - 20000:(1 << 20)]

    def integers(grid):
        w = grid.words[sub, 0]
        m = ((w & np.uint64(D.FRAC)) | np.uint64(1 << 52)).astype(object)
        e = (w >> np.uint64(52)).astype(np.int64).astype(object) - 1075
        return m, e - (2 * t[sub] - 104)          # X = m 2^e', an integer for e' >= 0

    m, e = integers(D.sqrt_hard_boundary())
    assert all(52 <= int(v) <= 53 for v in e)
    for mi, ei, yi in zip(m, e, y[sub]):
        X, ulp = int(mi) << int(ei), 1 << int(ei)
        assert 2 * abs(4 * X - (2 * int(yi) + 1) ** 2) <= 4 * ulp          # |X - (y + 1/2)^2| <= ulp / 2
    parities = set((D.sqrt_hard_boundary().words[:, 0] >> np.uint64(52)).astype(np.int64) & 1)
    assert parities == {0, 1}
    m, e = integers(D.sqrt_hard_representable())
    for mi, ei, yi, si in zip(m, e, y[sub], sign[sub]):
        X, ulp, y2 = int(mi) << int(ei), 1 << int(ei), int(yi) ** 2
        assert ulp <= 2 * abs(X - y2) <= 3 * ulp and (X > y2) == (si > 0)
    parities = set((D.sqrt_hard_representable().words[:, 0] >> np.uint64(52)).astype(np.int64) & 1)
    assert parities == {0, 1}


def test_numpy_and_the_oracle_agree_on_the_ieee_operations():
    """sqrt and / are IEEE operations: the oracle's (C) and numpy's are the same words, so the GPU test
    may compare the device with either."""
    for g in D.sqrt_grids():
        want = D.bits(np.sqrt(D.dbl(g.words[:, 0])))
        D.assert_same_words(g, g.oracle(n_threads=4), want)
    g = D.div_grid()
    a, w = D.dbl(g.words[:, 0]), D.dbl(g.words[:, 1])
    D.assert_same_words(g, g.oracle(), D.bits(a / w))
    D.assert_same_words(D.div_plain_grid(), D.div_plain_grid().oracle(), D.bits(a / w))


# --------------------------------------------------------------------------- (c) the oracle's accuracy
def _ulps(got, ref):
    """|got - ref| in ulps of the double nearest ref (ref: longdouble)."""
    return np.abs(got.astype(LD) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(LD)


def _worst(err, x):
    i = int(np.argmax(err))
    return float(err[i]), x[i]


@pytest.mark.parametrize("grid", ["exponents", "uniforms", "sums"])
def test_dlog_is_within_one_ulp(grid):
    g = {"exponents": D.log_exponents, "uniforms": D.log_uniforms, "sums": D.log_sums}[grid]()
    x = D.dbl(g.words[:, 0])
    worst, at = _worst(_ulps(D.dbl(g.oracle()), np.log(x.astype(LD))), x)
    print(f"dlog [{g.label}]: worst {worst:.4f} ulp at {at.hex()}")
    assert worst <= 1.0


@pytest.mark.parametrize("grid,limit", [("exponents", 1.408), ("uniforms", 1.0), ("sums", 1.0)])
def test_dlog_tab_is_within_its_absolute_bound(grid, limit):
    """3e-16 + 1 ulp where the kernels use it (S in [w_max, K], and the uniforms).  A FINDING of the
    grid over every exponent: the documented bound does not hold over the whole normal range -- from
    |log x| ~ 11 on (17 748 of the 830 676 arguments) the two roundings of fma(-e, ln 2, LRC_j) and of
    the final difference, each half an ulp of the RESULT, add to the table's error; worst case 1.408 of
    the bound (1.41 ulp) at x = 0x1.97fffffffffffp-370.  The measured worst case is asserted there (the
    function is deterministic on the fixed grid); the oracle's comment and DESIGN.md state 1.5 ulp."""
    g = {"exponents": D.log_exponents, "uniforms": D.log_uniforms, "sums": D.log_sums}[grid]().of("dlog_tab")
    x = D.dbl(g.words[:, 0])
    ref = np.log(x.astype(LD))
    err = np.abs(D.dbl(g.oracle()).astype(LD) - ref)
    bound = LD(3e-16) + np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
    worst, at = _worst(err / bound, x)
    print(f"dlog_tab [{g.label}]: worst {worst:.4f} of (3e-16 + 1 ulp) at {at.hex()}")
    assert worst <= limit


def _exp_case(fn, index):
    g = D.dexp_grids()[index].of(fn)
    x = D.dbl(g.words[:, 0])
    x_in = x[x >= -708.0]
    got = D.dbl(O.math_bulk(fn, D.bits(x_in)))
    worst, at = _worst(_ulps(got, np.exp(x_in.astype(LD))), x_in)
    print(f"{fn} [{g.label}]: worst {worst:.4f} ulp at {at.hex()}")
    return worst


@pytest.mark.parametrize("index", [1, 2, 3, 4, 5], ids=["ties-ln2", "ties-ln2-64", "uniform", "log-uniform", "positive"])
def test_dexp_is_within_one_ulp(index):
    assert _exp_case("dexp", index) <= 1.0


@pytest.mark.parametrize("index", [1, 2, 3, 4], ids=["ties-ln2", "ties-ln2-64", "uniform", "log-uniform"])
def test_dexp_tab_is_within_two_ulp(index):
    assert _exp_case("dexp_tab", index) <= 2.0


@pytest.mark.parametrize("fn", ["dexp", "dexp_tab"])
def test_exp_special_values(fn):
    got = D.dbl(D.exp_specials().of(fn).oracle())
    named = dict(zip(D.EXP_SPECIALS, got))
    assert named["-0.0"] == 1.0 and named["-2^-1074"] == 1.0 and named["-1e-300"] == 1.0
    assert named["-709"] == 0.0 and named["-inf"] == 0.0 and named["NaN"] == 0.0 and named["-708 - ulp"] == 0.0
    assert 0.0 < named["-708"] < named["-708 + ulp"] < 3.31e-308 and named["-708"] > 3.30e-308
    assert not np.signbit(got).any()


def test_sincos2pi_is_within_its_bound():
    g = D.sincos_grid()
    k = g.words[:, 0]
    out = D.dbl(g.oracle())
    o = (k >> np.uint64(49)).astype(np.int64)
    rem = k & np.uint64((1 << 49) - 1)
    phi = (2 * rem + np.uint64(1)).astype(LD) * LD(2.0 ** -50)          # exact: 50 bits
    phi = np.where(o & 1, LD(1) - phi, phi)                             # exact
    a = phi * (PI_LD / 4)
    s, c = np.sin(a), np.cos(a)
    swap = ((o + 1) & 2) != 0
    ss, cc = np.where(swap, c, s), np.where(swap, s, c)
    ss = np.where(o & 4, -ss, ss)
    cc = np.where((o + 2) & 4, -cc, cc)
    u = (2 * k + np.uint64(1)).astype(LD) * LD(2.0 ** -53)
    bound = LD(5e-16) + LD(4e-16) * 2 * PI_LD * u
    worst_s, at_s = _worst(np.abs(out[:, 0].astype(LD) - ss) / bound, k)
    worst_c, at_c = _worst(np.abs(out[:, 1].astype(LD) - cc) / bound, k)
    print(f"sincos2pi: worst sin {worst_s:.4f} of the bound at k = {int(at_s)}, cos {worst_c:.4f} at k = {int(at_c)}")
    assert worst_s <= 1.0 and worst_c <= 1.0
    assert np.abs(out[:, 0] ** 2 + out[:, 1] ** 2 - 1).max() < 5e-16


def _short_log_worst(b, first, stride, n):
    """max |orc_neg_log_short(n, b) - t| / (4e-16 max(1, t)), t = b ln 2 - log n in longdouble."""
    worst, at, worst_abs = 0.0, 0, 0.0
    step = 1 << 21
    for lo in range(0, n, step):
        m = min(step, n - lo)
        args = np.uint64(first) + np.arange(lo, lo + m, dtype=np.uint64) * np.uint64(stride)
        got = D.dbl(O.math_bulk(f"neg_log_short_{b}", args, n_threads=4))
        t = LD(b) * LN2_LD - np.log(args.astype(LD))
        err = np.abs(got.astype(LD) - t)
        rel = err / (LD(4e-16) * np.maximum(LD(1), t))
        i = int(np.argmax(rel))
        if rel[i] > worst:
            worst, at = float(rel[i]), int(args[i])
        worst_abs = max(worst_abs, float(err.max()))
    return worst, at, worst_abs


@pytest.mark.parametrize("b,stride", [(25, 2), (29, 32)], ids=["b25-every-argument", "b29-every-16th"])
def test_neg_log_short_is_within_its_relative_bound(b, stride):
    """4e-16 max(1, t): all of b = 25, every 16th odd argument of b = 29.  (The absolute error reaches
    3e-15 near t = 17: the bound is relative, as the oracle's comment now says.)"""
    worst, at, worst_abs = _short_log_worst(b, 1, stride, 1 << 24)
    print(f"neg_log_short b = {b}: worst {worst:.4f} of 4e-16 max(1, t) at n = {at}; largest absolute error {worst_abs:.3e}")
    assert worst <= 1.0

"""The argument grids of the device-math sweeps, shared by tests/test_gpu_math_domains.py (device
against oracle, bit for bit) and tests/test_math_domains_host.py (the grids' own properties and the
oracle's accuracy on them).  docs/KERNELS.md, "Device math: contracts, call sites and what is swept",
says why each grid is what it is.

Every seed is fixed.  Every value is built from integers or exact bit patterns with IEEE + - * only
(no libm call); where a grid is *defined* through the oracle (the call-site arguments of the square
root) it is computed by the oracle.  A grid is a `Grid`: the function's name (a key of
oracle.cbind.MATH_FUNCTIONS), and either an array of uint64 words [n, words in] or generated arguments
first + i * stride."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cbind as O

U64 = np.uint64
LN2 = 6.93147180559945286227e-01        # RN(ln 2): det_math.h
ONE = 0x3FF0000000000000
FRAC = (1 << 52) - 1
CHUNK = 1 << 24                          # the probe's largest call (MCMC_HIP_PROBE_MAX_ELEMENTS)


class Grid:
    def __init__(self, fn, words=None, first=0, stride=1, n=None, label=""):
        self.fn, self.label = fn, label
        self.words_in, self.words_out = O.MATH_FUNCTIONS[fn][1:]
        if words is not None:
            words = np.ascontiguousarray(words, dtype=U64).reshape(-1, self.words_in)
            words.setflags(write=False)
            n = len(words)
        self.words, self.first, self.stride, self.n = words, int(first), int(stride), int(n)
        assert 0 < self.n <= CHUNK

    def args(self):
        """The arguments as words [n, words in], generated ones written out."""
        if self.words is not None:
            return self.words
        return (U64(self.first) + np.arange(self.n, dtype=U64) * U64(self.stride)).reshape(-1, 1)

    def of(self, fn):
        """The same arguments for another function of the same shape."""
        return Grid(fn, self.words, self.first, self.stride, self.n, self.label)

    def oracle(self, fn=None, n_threads=1):
        return O.math_bulk(fn or self.fn, self.words, self.first, self.stride, self.n, n_threads)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(U64)


def dbl(w):
    return np.ascontiguousarray(w, dtype=U64).view(np.float64)


def differences(args, got, want):
    """None if the words agree; else (count, index of the first, message): the message names the
    first differing argument in hex, both results and the count."""
    got = np.asarray(got, dtype=U64).reshape(len(args), -1)
    want = np.asarray(want, dtype=U64).reshape(len(args), -1)
    bad = np.flatnonzero((got != want).any(axis=1))
    if not len(bad):
        return None
    i = int(bad[0])
    hexes = lambda row: "(" + ", ".join(f"0x{int(v):016x}" for v in row) + ")"   # noqa: E731
    return (len(bad), i,
            f"{len(bad)} of {len(args)} differ; first at index {i}: argument {hexes(args[i])} "
            f"gives {hexes(got[i])}, expected {hexes(want[i])}")


def assert_same_words(grid, got, want):
    diff = differences(grid.args(), got, want)
    assert diff is None, f"{grid.fn} [{grid.label}]: {diff[2]}"


def _rng(seed):
    return np.random.default_rng(seed)


def _rand_frac(rng, n):
    return rng.integers(0, 1 << 52, n, dtype=U64)


def _compose(exp, frac, sign=0):
    """Doubles (as words) from biased exponents and 52-bit fractions."""
    return (U64(sign) << U64(63)) | (np.asarray(exp, dtype=U64) << U64(52)) | np.asarray(frac, dtype=U64)


def _neighbours(x, reach=1):
    """x and the doubles up to `reach` ulps on either side of it (x finite, not 0), as words."""
    w = bits(x).astype(np.int64)
    return np.concatenate([w + k for k in range(-reach, reach + 1)]).view(U64)


# ----------------------------------------------------------------------------- neg_log_short
def neg_log_short_25():
    """Every odd n < 2^25."""
    return Grid("neg_log_short_25", first=1, stride=2, n=1 << 24, label="every odd n < 2^25")


def neg_log_short_29(chunk):
    """Odd n in [chunk 2^25, (chunk + 1) 2^25), chunk < 16: together every odd n < 2^29."""
    assert 0 <= chunk < 16
    return Grid("neg_log_short_29", first=1 + chunk * (1 << 25), stride=2, n=1 << 24,
                label=f"odd n < 2^29, chunk {chunk} of 16")


# ----------------------------------------------------------------------------- square roots
@functools.lru_cache(None)
def sqrt_call_site():
    """All 2^24 arguments of PairRng: 2 neg_log_short(2 kr + 1, 25) (the doubling is exact)."""
    e = dbl(neg_log_short_25().oracle(n_threads=4))
    return Grid("sqrt_midrange", bits(2.0 * e), label="2 E_r of every kr")


@functools.lru_cache(None)
def sqrt_tail():
    """2^20 arguments of the redrawn lowest bin: 2 fma(24, ln 2, -dlog(u52(k)))."""
    k = _rand_frac(_rng(101), 1 << 20)
    k[:4] = [0, 1, FRAC - 1, FRAC]
    t = dbl(O.math_bulk("tail_of_k", np.stack([k, np.full_like(k, 24)], axis=1)))
    return Grid("sqrt_midrange", bits(2.0 * t), label="2 E_r of the redrawn tail")


SQRT_LO_EXP, SQRT_HI_EXP = -100, 100     # the contract of sqrt_midrange: [2^-100, 2^100]


@functools.lru_cache(None)
def sqrt_contract():
    """Every binade of [2^-100, 2^100]: mantissas 1, 1 + ulp, 2 - ulp and 64 random; and 2^100."""
    rng = _rng(102)
    exps = np.arange(SQRT_LO_EXP, SQRT_HI_EXP, dtype=np.int64) + 1023
    frac = np.concatenate([np.broadcast_to(np.array([0, 1, FRAC], dtype=U64)[None], (len(exps), 3)),
                           _rand_frac(rng, len(exps) * 64).reshape(len(exps), 64)], axis=1)
    w = _compose(exps[:, None], frac).ravel()
    w = np.concatenate([w, _compose([SQRT_HI_EXP + 1023], [0])])
    return Grid("sqrt_midrange", w, label="every binade of the contract")


def _round53(N):
    """Round the positive Python integers N (object array) to 53 significant bits, to nearest, ties to
    even: (m, e) with RN(N) = m 2^e, 2^52 <= m < 2^53."""
    m, e = [], []
    for v in N:
        s = v.bit_length() - 53
        if s <= 0:
            m.append(v << -s); e.append(s)
            continue
        q, r = v >> s, v & ((1 << s) - 1)
        half = 1 << (s - 1)
        q += 1 if (r > half or (r == half and (q & 1))) else 0
        if q == 1 << 53:
            q, s = 1 << 52, s + 1
        m.append(q); e.append(s)
    return np.array(m, dtype=object), np.array(e, dtype=object)


def _words_of(m, e):
    """The doubles m 2^e (normal; 2^52 <= m < 2^53) as words."""
    m = np.array([int(v) for v in m], dtype=U64)
    be = np.array([int(v) + 52 + 1023 for v in e], dtype=np.int64)
    assert be.min() > 0 and be.max() < 2047
    return _compose(be, m & U64(FRAC))


@functools.lru_cache(None)
def sqrt_hard_y():
    """The random 53-bit mantissas y (Python integers) and even shifts 2 t of the hard cases."""
    rng = _rng(103)
    y = (rng.integers(0, 1 << 52, 1 << 20, dtype=U64) | U64(1 << 52)).astype(object)
    t = rng.integers(-45, 46, 1 << 20).astype(object)    # x = X 2^(2 t - 104), X in [2^104, 2^106)
    sign = rng.integers(0, 2, 1 << 20) * 2 - 1
    return y, t, sign


@functools.lru_cache(None)
def sqrt_hard_boundary():
    """x = RN(((2 y + 1) / 2)^2) 4^t: the root lies next to the midpoint y + 1/2 of two doubles."""
    y, t, _ = sqrt_hard_y()
    m, e = _round53((2 * y + 1) ** 2)            # 4 X
    return Grid("sqrt_midrange", _words_of(m, e - 2 + 2 * t - 104), label="roots next to a rounding boundary")


@functools.lru_cache(None)
def sqrt_hard_representable():
    """x = (RN(y^2) +- 1 ulp) 4^t: the root lies next to the double y."""
    y, t, sign = sqrt_hard_y()
    m, e = _round53(y * y)
    m = m + sign.astype(object)
    low = m < (1 << 52)                          # (2^52 - 1: one binade down, ulp halves -- keep 1 ulp of x)
    m = np.where(low, (1 << 53) - 1, m)
    e = np.where(low, e - 1, e)
    high = m >= (1 << 53)
    m = np.where(high, 1 << 52, m)
    e = np.where(high, e + 1, e)
    return Grid("sqrt_midrange", _words_of(m, e + 2 * t - 104), label="roots next to a representable number")


def sqrt_grids():
    return [sqrt_call_site(), sqrt_tail(), sqrt_contract(), sqrt_hard_boundary(), sqrt_hard_representable()]


# ----------------------------------------------------------------------------- logarithms
LOG_THRESHOLD_FRAC = 0x6A09C << 32      # first fraction that fdlibm's reduction halves (hx + 0x95f64 carries)


@functools.lru_cache(None)
def log_exponents():
    """Every exponent of the normal range x mantissas 1, 1 + ulp, 2 - ulp, the neighbours of fdlibm's
    reduction threshold, the 128 table-interval ends +- 1 ulp and 16 random."""
    rng = _rng(201)
    exps = np.arange(1, 2047, dtype=np.int64)
    ends = (np.arange(128, dtype=np.int64) << 45)[:, None] + np.array([-1, 0, 1])[None]
    fixed = np.concatenate([[0, 1, FRAC], LOG_THRESHOLD_FRAC + np.array([-1, 0, 1]), ends.ravel() & FRAC])
    frac = np.concatenate([np.broadcast_to(fixed.astype(U64)[None], (len(exps), len(fixed))),
                           _rand_frac(rng, len(exps) * 16).reshape(len(exps), 16)], axis=1)
    return Grid("dlog", _compose(exps[:, None], frac).ravel(), label="every normal exponent")


def _u52(k):
    return (2 * np.asarray(k, dtype=U64) + U64(1)).astype(np.float64) * 2.0 ** -53   # exact


@functools.lru_cache(None)
def log_uniforms():
    """u52(k): k = 0, 1, 2^52 - 2, 2^52 - 1 and 2^21 random k -- what every -log u is taken of."""
    k = np.concatenate([np.array([0, 1, FRAC - 1, FRAC], dtype=U64), _rand_frac(_rng(202), 1 << 21)])
    return Grid("dlog", bits(_u52(k)), label="u52(k)")


@functools.lru_cache(None)
def log_sums():
    """2^20 values in [2^-10, 16]: the log-sum-exp's S and the stretch factor."""
    rng = _rng(203)
    w = _compose(rng.integers(-10, 4, 1 << 20) + 1023, _rand_frac(rng, 1 << 20))
    w[:3] = bits([2.0 ** -10, 16.0, 1.0])
    return Grid("dlog", w, label="[2^-10, 16]")


@functools.lru_cache(None)
def log_subnormals():
    """OUTSIDE dlog's contract ("a positive normal double"), but passed: the snooker move takes
    dlog(n2) of a squared distance that may be subnormal.  Both sides define the result (integer
    reduction: the exponent field 0 is read as 2^-1023).  +0 is included: a caller tests n2 > 0 only
    after the call has been issued."""
    w = np.concatenate([np.array([0, 1, 2, FRAC - 1, FRAC, 1 << 51], dtype=U64), _rand_frac(_rng(204), 1 << 12)])
    return Grid("dlog", w, label="subnormal arguments (snooker's n2)")


def dlog_grids():
    return [log_exponents(), log_uniforms(), log_sums(), log_subnormals()]


def dlog_tab_grids():
    return [g.of("dlog_tab") for g in (log_exponents(), log_uniforms(), log_sums())]


# ----------------------------------------------------------------------------- exponentials
EXP_SPECIALS = ["-0.0", "-2^-1074", "-1e-300", "-708", "-708 - ulp", "-708 + ulp", "-709", "-inf", "NaN"]


@functools.lru_cache(None)
def exp_specials():
    m708 = bits([-708.0])[0]
    w = np.array([1 << 63, (1 << 63) | 1, bits([-1e-300])[0], m708, m708 + U64(1), m708 - U64(1),
                  bits([-709.0])[0], bits([-np.inf])[0], 0x7FF8000000000000], dtype=U64)
    return Grid("dexp", w, label="special values")


def _ties(scale, k_lo, reach=2):
    """The doubles next to k scale and (k + 1/2) scale, k in [k_lo, 0] (scale = RN(ln 2) or
    RN(ln 2) / 64, a power-of-two quotient: exact): where rint(x / scale) changes and where it ties."""
    k = np.arange(k_lo, 1, dtype=np.float64)
    x = np.concatenate([k[:-1] * scale, (k[:-1] + 0.5) * scale, [-0.5 * scale]])   # (0 itself: a special)
    return _neighbours(x, reach)


@functools.lru_cache(None)
def exp_ties_ln2():
    return Grid("dexp", _ties(LN2, -1021), label="k ln 2 and (k + 1/2) ln 2")


@functools.lru_cache(None)
def exp_ties_ln2_64():
    return Grid("dexp", _ties(LN2 / 64.0, -65344), label="k ln 2 / 64 and (k + 1/2) ln 2 / 64")


@functools.lru_cache(None)
def exp_uniform():
    """2^21 values uniform in [-40, 0]: the differences a_k - a_max that matter to a mixture."""
    return Grid("dexp", bits(-40.0 * _rng(301).random(1 << 21)), label="uniform in [-40, 0]")


@functools.lru_cache(None)
def exp_log_uniform():
    """2^20 values log-uniform in [-708, -1e-12]: a random binade and a random mantissa."""
    rng = _rng(302)
    n = 3 << 19
    x = -dbl(_compose(rng.integers(-40, 10, n) + 1023, _rand_frac(rng, n)))
    x = x[(x >= -708.0) & (x <= -1e-12)][:1 << 20]
    assert len(x) == 1 << 20
    return Grid("dexp", bits(x), label="log-uniform in [-708, -1e-12]")


EXP_CLAMP = 700.0     # evidence_args.h kEvClamp, importance_args.h kImClamp


@functools.lru_cache(None)
def exp_positive():
    """OUTSIDE dexp's contract ("x <= 0"), but passed: the evidence and the importance weights take
    dexp(min(arg, 700)).  Both sides define the result (the same reduction; y 2^k stays finite up to
    709).  (0, 700]: 2^18 uniform, the rint steps and ties k ln 2, (k + 1/2) ln 2, and the clamp."""
    k = np.arange(1, 1010, dtype=np.float64)
    x = dbl(_neighbours(np.concatenate([k * LN2, (k - 0.5) * LN2]), 2))
    x = np.concatenate([x[x <= EXP_CLAMP], [EXP_CLAMP, dbl(bits([EXP_CLAMP]) - U64(1))[0], 2.0 ** -1074, 1e-300],
                        EXP_CLAMP * (1.0 - _rng(303).random(1 << 18))])
    return Grid("dexp", bits(x), label="(0, 700]: the clamped evidence / importance argument")


def dexp_grids():
    return [exp_specials(), exp_ties_ln2(), exp_ties_ln2_64(), exp_uniform(), exp_log_uniform(), exp_positive()]


def dexp_tab_grids():
    return [g.of("dexp_tab") for g in dexp_grids()[:-1]]


# ----------------------------------------------------------------------------- sincos2pi
@functools.lru_cache(None)
def sincos_grid():
    """Per octant o: k = o 2^49 + {0, 1, 2^49 - 1}; and 2^21 random k < 2^52."""
    edges = (np.arange(8, dtype=U64)[:, None] << U64(49)) + np.array([0, 1, (1 << 49) - 1], dtype=U64)[None]
    return Grid("sincos2pi", np.concatenate([edges.ravel(), _rand_frac(_rng(401), 1 << 21)]),
                label="octant edges and random k")


# ----------------------------------------------------------------------------- quotients
DIV_FIXED_WIDTHS = [1.0, 6.283185307179586, 360.0, 0.1, 1e-3, 1e6, 2450000.1 - 2450000.0]
DIV_PER_WIDTH = 16 * 3 + 3 + (1 << 16)


@functools.lru_cache(None)
def div_widths():
    rng = _rng(501)
    rand = dbl(_compose(rng.integers(-20, 20, 32) + 1023, _rand_frac(rng, 32)))
    return np.concatenate([DIV_FIXED_WIDTHS, rand])


@functools.lru_cache(None)
def div_grid():
    """(a, w, RN(1 / w)) per width w: a = j w and its two neighbours for j in [-8, 8] (for j = 0 the
    0 alone: its neighbours are subnormal, which no caller forms), 0 and +-2^-100 w, and 2^16 random a
    in [-8 w, 8 w]."""
    rng = _rng(502)
    rows = []
    for w in div_widths():
        j = np.arange(-8, 9, dtype=np.float64)
        jw = j[j != 0] * w
        a = np.concatenate([dbl(_neighbours(jw, 1)), [0.0, 2.0 ** -100 * w, -(2.0 ** -100) * w],
                            w * (16.0 * rng.random(1 << 16) - 8.0)])
        assert len(a) == DIV_PER_WIDTH
        rows.append(np.stack([bits(a), np.full(len(a), bits([w])[0]), np.full(len(a), bits([1.0 / w])[0])], axis=1))
    return Grid("div_by", np.concatenate(rows), label="periodic-wrap quotients")


def div_plain_grid():
    return Grid("div", div_grid().words[:, :2], label="periodic-wrap quotients")


# ----------------------------------------------------------------------------- philox and u52
PHILOX_KNOWN = [   # Random123 kat_vectors, philox4x32-10: (k0, k1, c0, c1, c2, c3) -> four words
    ((0, 0, 0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 6, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0xA4093822, 0x299F31D0, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@functools.lru_cache(None)
def philox_grid():
    """The three known answers, 64 blocks whose step words (c2, c3) run across 2^32, and 2^20 random
    (key, counter) sets."""
    rng = _rng(601)
    rand = rng.integers(0, 1 << 32, ((1 << 20), 6), dtype=U64)
    steps = np.arange((1 << 32) - 32, (1 << 32) + 32, dtype=U64)
    across = rng.integers(0, 1 << 32, (64, 6), dtype=U64)
    across[:, 4], across[:, 5] = steps & U64(0xFFFFFFFF), steps >> U64(32)
    known = np.array([k for k, _ in PHILOX_KNOWN], dtype=U64)
    return Grid("philox", np.concatenate([known, across, rand]), label="known answers, steps across 2^32, random")


@functools.lru_cache(None)
def u52_grid():
    k = np.concatenate([np.array([0, 1, FRAC - 1, FRAC, 1 << 51, (1 << 51) - 1], dtype=U64),
                        _rand_frac(_rng(602), 1 << 20)])
    return Grid("u52", k, label="edges and random k")

"""The device math of det_math.h against the oracle, bit for bit, function by function, on whole
argument domains (tests/math_domains.py; docs/KERNELS.md "Device math: contracts, call sites and what
is swept").  The device's side is the probe mcmc_hip_math_probe (math_probe_kernels.hip), the oracle's
the bulk forms of oracle/mcmc_oracle.c; the words are compared as uint64, with no tolerance.  The
square roots and the quotients are compared with numpy's, the IEEE operations they claim to equal.
The grids' own properties and the oracle's accuracy on them: tests/test_math_domains_host.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from cobaya_amd import engine as E  # noqa: E402
from oracle import cbind as O  # noqa: E402
from tests import math_domains as D  # noqa: E402

u64p = C.POINTER(C.c_uint64)


def device(grid, fn=None):
    """The probe's words [n] or [n, words out] of `fn` (default: the grid's function) on the grid."""
    fn = fn or grid.fn
    code, wi, wo = O.MATH_FUNCTIONS[fn]
    assert wi == grid.words_in
    out = np.empty((grid.n, wo), dtype=np.uint64)
    args = None if grid.words is None else grid.words.ctypes.data_as(u64p)
    rc = E.load_library().mcmc_hip_math_probe(code, args, grid.first, grid.stride, grid.n,
                                              out.ctypes.data_as(u64p))
    assert rc == E.OK, f"mcmc_hip_math_probe({fn}) returned {rc}"
    return out[:, 0] if wo == 1 else out


def check(grid, want=None):
    D.assert_same_words(grid, device(grid), grid.oracle(n_threads=4) if want is None else want)


def test_the_probe_refuses_what_it_cannot_run():
    lib = E.load_library()
    out = np.zeros(8, dtype=np.uint64)
    a = np.ones(24, dtype=np.uint64)
    po, pa = out.ctypes.data_as(u64p), a.ctypes.data_as(u64p)
    assert lib.mcmc_hip_math_probe(13, pa, 0, 1, 4, po) == E.ERR_ARG        # unknown function
    assert lib.mcmc_hip_math_probe(-1, pa, 0, 1, 4, po) == E.ERR_ARG
    assert lib.mcmc_hip_math_probe(2, pa, 0, 1, 4, None) == E.ERR_ARG       # null result
    assert lib.mcmc_hip_math_probe(12, None, 0, 1, 4, po) == E.ERR_ARG      # two words cannot be generated
    assert lib.mcmc_hip_math_probe(2, pa, 0, 1, (1 << 24) + 1, po) == E.ERR_ARG
    assert lib.mcmc_hip_math_probe(2, pa, 0, 1, -1, po) == E.ERR_ARG
    assert lib.mcmc_hip_math_probe(2, pa, 0, 1, 0, po) == E.OK and not out.any()
    assert lib.mcmc_hip_math_probe(1, None, 5, 3, 8, po) == E.OK             # u52(5 + 3 i), generated
    assert np.array_equal(out.view(np.float64), (2.0 * (5 + 3 * np.arange(8)) + 1) * 2.0 ** -53)


def test_philox_and_u52():
    g = D.philox_grid()
    got = device(g)
    for i, (_, answer) in enumerate(D.PHILOX_KNOWN):
        assert tuple(int(v) for v in got[i]) == answer
    D.assert_same_words(g, got, g.oracle())
    check(D.u52_grid())
    k = D.u52_grid().words[:, 0]
    D.assert_same_words(D.u52_grid(), device(D.u52_grid()), D.bits((2 * k + np.uint64(1)).astype(np.float64) * 2.0 ** -53))


def test_neg_log_short_every_radial_argument():
    check(D.neg_log_short_25())


@pytest.mark.parametrize("quarter", range(4))
def test_neg_log_short_every_accept_argument(quarter):
    for chunk in range(4 * quarter, 4 * quarter + 4):
        check(D.neg_log_short_29(chunk))


SQRT_GRIDS = ["call_site", "tail", "contract", "hard_boundary", "hard_representable"]


@pytest.mark.parametrize("fn", ["sqrt_midrange", "sqrt"])
@pytest.mark.parametrize("grid", SQRT_GRIDS)
def test_square_roots_are_correctly_rounded(grid, fn):
    """numpy.sqrt is the reference (the IEEE square root); the oracle's sqrt() is the same words
    (test_math_domains_host.py).  No argument is excluded: sqrt_midrange is correctly rounded on every
    grid, the whole of [2^-100, 2^100] as its comment claims."""
    g = getattr(D, "sqrt_" + grid)().of(fn)
    check(g, D.bits(np.sqrt(D.dbl(g.words[:, 0]))))


@pytest.mark.parametrize("fn", ["div_by", "div"])
def test_quotients_are_the_ieee_quotients(fn):
    g = D.div_grid() if fn == "div_by" else D.div_plain_grid()
    check(g, D.bits(D.dbl(g.words[:, 0]) / D.dbl(g.words[:, 1])))


@pytest.mark.parametrize("grid", ["exponents", "uniforms", "sums", "subnormals"])
def test_dlog(grid):
    check(getattr(D, "log_" + grid)())


@pytest.mark.parametrize("grid", ["exponents", "uniforms", "sums"])
def test_dlog_tab(grid):
    check(getattr(D, "log_" + grid)().of("dlog_tab"))


EXP_GRIDS = ["specials", "ties_ln2", "ties_ln2_64", "uniform", "log_uniform"]


@pytest.mark.parametrize("grid", EXP_GRIDS + ["positive"])
def test_dexp(grid):
    check(getattr(D, "exp_" + grid)())


@pytest.mark.parametrize("grid", EXP_GRIDS)
def test_dexp_tab(grid):
    check(getattr(D, "exp_" + grid)().of("dexp_tab"))


@pytest.mark.parametrize("fn", ["dexp", "dexp_tab"])
def test_exp_gives_zero_below_the_cut_off_and_for_nan(fn):
    got = dict(zip(D.EXP_SPECIALS, device(D.exp_specials().of(fn))))
    for name in ("-709", "-inf", "NaN", "-708 - ulp"):
        assert got[name] == 0, name                      # +0.0, the word
    assert got["-0.0"] == D.ONE and got["-708"] != 0


def test_sincos2pi():
    check(D.sincos_grid())


def test_control_the_comparison_sees_a_different_function():
    """Not vacuous: the probe's dlog against the oracle's dlog_tab on the same grid reports
    differences (two algorithms, equal to an ulp or so); like with like reports none."""
    g = D.log_sums()
    got = device(g)
    assert D.differences(g.args(), got, g.oracle("dlog")) is None
    diff = D.differences(g.args(), got, g.oracle("dlog_tab"))
    assert diff is not None and diff[0] > g.n // 100, diff
    with pytest.raises(AssertionError, match="differ; first at index"):
        D.assert_same_words(g, got, g.oracle("dlog_tab"))

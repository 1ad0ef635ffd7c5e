"""The binned Gaussian (plik-lite) target at every kernel geometry: the cases and their helpers.

`mcmc_hip_set_target_binned_gaussian` serves 1 <= n_bins <= 640, 1 <= n_lin <= 31 and the
calibration parameter at any position.  What a shape selects (capi_targets.hip, restated in
`geometry` below; the library is not asked):

    NT    = ceil(n_bins / 16)        16-row tiles of L^-1
    shift = (8 - NT mod 8) mod 8     virtual tile = real + shift: the groups of eight end at the LAST tile
    NG    = (NT + shift) / 8         groups = LDS chunks of pl_fused_kernel<NG, np>
    ntw   = ceil(NT / 8)             row tiles per wave of pl_chi2_kernel<ntw>  (= NG)
    KT    = ceil(n_bins / 4) rounded up to even   k-steps of four bins ("padded" when it was odd)
    np    = ceil(n_lin / 8)          k-step pairs over the parameters: pl_residual_mfma_kernel<np>
    nlp   = n_lin rounded up to 4    pl_residual_kernel<nlp> (behind MCMC_HIP_PL_SCALAR_RESIDUAL)

`STEP_CASES` steps every (NG, np), shift, ntw, KT parity, the n_lin at which the producer's clamp
`min(4 j + c, n_lin - 1)` changes arm, and the calibration parameter first, in the middle and last
(the gather `i = p + (p >= calib)` of three kernels); tests/test_binned_cases_host.py asserts that
coverage on the list itself and pins the oracle at every shape against a longdouble reference,
tests/test_gpu_binned_geometries.py runs the device against the oracle.  No GPU import here."""
import functools

import numpy as np

from cobaya_amd import pliklite as P
from oracle import cbind as O
from tests.pliklite_common import sampling_problem, small_dataset

N_WIDE = 645


@functools.lru_cache(maxsize=None)
def wide_dataset():
    """215 TT + 215 TE + 215 EE = 645 bins: wide enough for the upper limit (640) and for 641."""
    ds = P.synthetic_dataset(0, nbin_pol=215)
    assert ds.nbins == N_WIDE
    return ds


def first_bins(ds, n):
    """A `BinnedGaussian` of the first `n` entries of the data vector of `ds` (what `from_dataset`
    leaves for that selection: `used_bins` per spectrum, `used_indices`, `X_data`, the covariance
    sub-matrix)."""
    full = P.BinnedGaussian.from_dataset(ds)
    if not 1 <= n <= full.n_bins:
        raise ValueError(f"n must be in 1..{full.n_bins}")
    used, left = [], n
    for keep in full.used_bins:
        used.append(np.asarray(keep[:max(left, 0)], dtype=int))
        left -= len(keep)
    places = full.used_indices[:n]
    return P.BinnedGaussian(blmin=full.blmin, blmax=full.blmax, weights=full.weights, used_bins=used,
                            used_indices=places, X_data=full.X_data[:n].copy(),
                            cov=np.ascontiguousarray(full.cov[:n, :n]), lmax=full.lmax,
                            calibration_param=full.calibration_param)


def order_of(n_lin, calib):
    """Sampled position -> index in the calibration-last order: the emulator parameters keep their
    order around position `calib` (as orc_binned_delta reads them)."""
    order = list(range(n_lin))
    order.insert(calib, n_lin)
    return np.array(order)


def permuted_problem(target, emu, calib):
    """`sampling_problem` with the calibration parameter at position `calib`."""
    kinds, a, b, C = sampling_problem(target, emu)
    o = order_of(emu.n, calib)
    return kinds[o], a[o], b[o], np.ascontiguousarray(C[np.ix_(o, o)])


def fiducial(emu, calib):
    return np.concatenate((emu.theta0, [1.0]))[order_of(emu.n, calib)]


def start_points(emu, C, calib, n, seed=77):
    """`n` points drawn around the fiducial point with the (permuted) Fisher covariance `C`."""
    rng = np.random.default_rng(seed)
    return fiducial(emu, calib) + rng.standard_normal((n, emu.n + 1)) @ np.linalg.cholesky(C).T


def geometry(n_bins, n_lin):
    """What capi_targets.hip derives from a shape (see the module docstring)."""
    NT = (n_bins + 15) // 16
    shift = (8 - NT % 8) % 8
    quads = (n_bins + 3) // 4
    return {"NT": NT, "shift": shift, "NG": (NT + shift) // 8, "ntw": (NT + 7) // 8,
            "KT": (quads + 1) & ~1, "padded": quads % 2 == 1, "np": (n_lin + 7) // 8,
            "nlp": (n_lin + 3) & ~3}


N_BINS = (1, 16, 17, 33, 49, 65, 128, 129, 250, 256, 257, 384, 400, 513, 625, 640)
N_LIN = (1, 7, 8, 9, 16, 17, 24, 25, 31)
# No count of N_BINS has NT = 7 (mod 8) or 6 (mod 8): shift 1 comes from 111 bins (NT = 7; a count
# tests/test_gpu_pliklite.py evaluates and never steps), shift 2 from the 88 bins of the first
# batch case.
EXTRA_BINS = (88, 111)
BATCH_W = 16448     # 257 sets of 64: batches = 2, a grid of 129, the last workgroup takes one set

# (n_bins, n_lin, calib, W, gs).  Up to 215 bins the data vector is TT alone, where the binned response
# to emulator parameter 4 (the polarisation amplitude) is exactly zero: a wrong gather at p = 4 would
# change no bit there, so the calibration positions 4 and 5 sit in cases with TE bins (the host test
# asserts that the response columns on both sides of every calibration position are non-zero).
STEP_CASES = [
    # NG = 1
    (1, 31, 0, 64, 64), (16, 1, 1, 64, 64), (17, 9, 8, 64, 64), (33, 17, 6, 128, 64),
    (49, 7, 0, 64, 64), (65, 8, 3, 64, 64), (128, 25, 12, 128, 128), (111, 16, 16, 64, 64),
    # NG = 2
    (129, 8, 8, 64, 64), (250, 16, 0, 64, 64), (256, 24, 24, 128, 64), (129, 31, 31, 64, 64),
    # NG = 3
    (257, 1, 0, 64, 64), (384, 9, 4, 64, 64), (257, 24, 8, 64, 64), (384, 25, 0, 128, 64),
    # NG = 4
    (400, 7, 7, 64, 64), (400, 16, 7, 64, 64), (400, 17, 5, 64, 64), (400, 31, 15, 64, 64),
    # NG = 5
    (513, 8, 0, 64, 64), (625, 9, 5, 64, 64), (640, 17, 0, 128, 64), (640, 31, 31, 64, 64),
    # batches = 2: the LDS buffer parity of pl_fused_kernel carries from one set to the next
    # (par += NG: it flips between the sets at NG = 1 and stays at NG = 2)
    (88, 5, 5, BATCH_W, 64), (129, 9, 0, BATCH_W, 64),
]
STEP_CALLS = (1, 3, 5)          # steps per call (a call ends on an accept-only launch)
BATCH_CALLS = (1, 2, 3)         # six steps for the two batch cases
STEP_SEED = 5                   # engine / oracle seed of every case

# Cases that faulted or hung on the device and whose cause is not known: {case: what was seen}.
# They are not run (tests/test_gpu_binned_geometries.py), docs/KERNELS.md lists them under "Open".
HELD_BACK = {}


def calls_of(case):
    return BATCH_CALLS if case[3] == BATCH_W else STEP_CALLS


def case_id(case):
    return "-".join(str(v) for v in case)


def shapes(cases=None):
    """The distinct (n_bins, n_lin, calib) of the cases, in order."""
    out = []
    for c in (STEP_CASES if cases is None else cases):
        if c[:3] not in out:
            out.append(c[:3])
    return out


# the reduced lists of the two developer switches (tests/_binned_variant_worker.py)
SCALAR_N_LIN = (1, 4, 5, 8, 12, 13, 20, 24, 28, 31)      # every pl_residual_kernel<NLP>, NLP = 4..32
SCALAR_CASES = [(88, n, c) for n in SCALAR_N_LIN for c in sorted({0, min(2, n), n})]
UNFUSED_CASES = [(88, 5, 5, 64, 64), (129, 9, 0, 64, 64), (640, 31, 31, 64, 64)]
UNFUSED_CALLS = (1, 3, 5)       # nine steps


SMALL_BINS = 88     # the 48 TT + 20 TE + 20 EE bins of `small_dataset` (l <= 400), as tests/test_gpu_pliklite.py


@functools.lru_cache(maxsize=None)
def target_of(n_bins):
    """The first `n_bins` entries of the wide data vector; 88 bins: the whole small data set, which
    has all three spectra (the first 88 wide bins are TT alone)."""
    if n_bins == SMALL_BINS:
        t = P.BinnedGaussian.from_dataset(small_dataset())
        assert t.n_bins == SMALL_BINS
        return t
    return first_bins(wide_dataset(), n_bins)


@functools.lru_cache(maxsize=None)
def emulator_of(n_lin, n_bins=0):
    """The linear emulator over the multipoles of `target_of(n_bins)`."""
    return P.synthetic_emulator(n_lin, target_of(n_bins).lmax if n_bins == SMALL_BINS else wide_dataset().lmax)


def oracle_problem(n_bins, n_lin, calib, gs=64, seed=STEP_SEED):
    """The case on the oracle alone (no engine): the oracle's own Linv from `cov`, the proposal
    transform of the permuted Fisher covariance at the engine's default scale 2.4."""
    target, emu = target_of(n_bins), emulator_of(n_lin, n_bins)
    kinds, a, b, C = permuted_problem(target, emu, calib)
    B = O.Binned(target.bin_table(), target.weights, target.X_data, cov=target.cov,
                 theta0=emu.theta0, D0=emu.D0, J=emu.J, calib=calib)
    prob = O.Problem(n_lin + 1, kinds, a, b, T=O.proposal_transform(C, 2.4), group_size=gs,
                     seed=seed, binned=B)
    return target, emu, prob, B, C

"""checkpoint_kernels.hip (ckpt_window_kernel, ckpt_payload_kernel, ckpt_solve_kernel) on crafted
statistics, against the plain reference of tests/checkpoint_ref.py.  Nothing is sampled: the
accumulators are set (`set_moments`), and the solve kernel runs on payloads written into the
buffer `checkpoint_begin` returns -- what an all-reduce over ranks would have left there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (before the first Engine: one HIP runtime in the process)

from cobaya_amd import engine as E  # noqa: E402
from tests import checkpoint_ref as CR  # noqa: E402

EPS = CR.EPS
LD = np.longdouble


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bit_equal(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    bad = np.argwhere(_bits(a) != _bits(b))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} differ, first at {bad[:4].tolist()}"


def make_engine(d, W, gs, blocks=None):
    eng = E.Engine(d, W, group_size=gs, device=0, seed=3)
    eng.set_prior([0] * d, [-50.0] * d, [50.0] * d)
    eng.set_target_one()
    if blocks:
        eng.set_blocking(blocks, [1, 2])
    eng.set_proposal_cov(np.eye(d))
    eng.set_state(np.zeros((W, d)))          # (request_moments needs a state)
    eng.checkpoint_set_ring()
    return eng


class _View:     # __cuda_array_interface__ of n float64 at a device pointer (as engine.py's)
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False),
                                         "version": 2, "strides": None}


def inject(eng, ptr, P):
    """Overwrite the payload of the checkpoint begun on `eng` -- the all-reduce's place."""
    eng.sync()
    view = torch.as_tensor(_View(ptr, len(P)), device=torch.device("cuda", 0))
    view.copy_(torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64)))
    torch.cuda.synchronize()


def begin(eng, n_snap, gsum, S, window, n_win, steps_since=0.0):
    eng.set_moments(n_snap, gsum, S)
    eng.request_moments()
    ptr, n = eng.checkpoint_begin(window, n_win, steps_since)
    assert n == 5 + 2 * eng.d * eng.d + eng.d and ptr != 0
    return ptr


def payload_of(eng, n_snap, gsum, S, window, n_win, steps_since=0.0):
    begin(eng, n_snap, gsum, S, window, n_win, steps_since)
    eng.checkpoint_request_payload()
    n, g, s, _ = eng.fetch_moments()
    assert n == n_snap
    assert_bit_equal(g, gsum, "interval read-out: group sums")
    assert_bit_equal(s, S, "interval read-out: pooled sums")
    return eng.checkpoint_fetch_payload()


def solve(eng, P, lo, hi):
    """One checkpoint whose payload is replaced by P before the solve kernel runs."""
    d, G = eng.d, eng.G
    ptr = begin(eng, 1, np.zeros((G, d)), np.zeros((d, d)), 1, 1)
    inject(eng, ptr, P)
    eng.checkpoint_solve(lo, hi)
    eng.fetch_moments()
    return eng.checkpoint_fetch()


# ------------------------------------------------------------------ a. window and payload kernels
def _accumulators(rng, G, d):
    """Group sums and pooled second moments at mixed scales and signs."""
    cs = 10.0 ** rng.uniform(-3, 3, d)
    g = rng.standard_normal((G, d)) * cs * 10.0 ** rng.uniform(-1, 1, (G, 1))
    g[rng.random((G, d)) < 0.02] = 0.0
    A = rng.standard_normal((d, d))
    S = np.tril((A + A.T) * cs[:, None] * cs[None, :] * 100.0)
    return g, S + np.tril(S, -1).T           # (symmetric to the bit)


@pytest.mark.parametrize("d,W,gs", [
    (48, 8192, 64),       # G d = 6144: exactly one tile
    (48, 8256, 64),       # a tile and one group
    (30, 16384, 64), (128, 4096, 64),
    (100, 3968, 64),      # 61 groups + 1
    (7, 56192, 64),       # 877 groups + 1
    (1, 128, 64), (2, 512, 128), (32, 1024, 256)])
def test_window_and_payload_kernels(d, W, gs):
    """P[0], P[1], P[3] and sum_mean (a sequential sum of bit-specified means: a wrong slot, order
    or divisor shows) bit-equal to the reference; sum_mm and sum_Ncov to a derived bound against
    the long-double payload: a chain of G fused multiply-adds from +0 is within G u sum|terms|
    (u = eps / 2) of the exact sum to first order -- taken as (G + 2) eps sum_g |m_gi m_gj| --,
    and S - Nc mm adds a product and a difference: 2 eps (|S_ij| + Nc |mm_ij|) + Nc (the mm bound)."""
    G = W // gs
    rng = np.random.default_rng(100 * d + G)
    eng = make_engine(d, W, gs)
    intervals = []
    for k, window in enumerate([1, 2, 3, 1, 5]):
        n_snap = int(rng.integers(1, 40))
        g, S = _accumulators(rng, G, d)
        intervals.append((n_snap, g, S))
        ivs = intervals[-window:]
        n_win = sum(iv[0] for iv in ivs)
        steps_since = float(rng.integers(1, 10 ** 6))
        P = payload_of(eng, n_snap, g, S, window, n_win, steps_since)
        Nc = float(n_win) * float(gs)
        g_sum, S_sum, means = CR.window_sums([(iv[1], iv[2]) for iv in ivs], Nc)
        assert P[0] == G and P[1] == Nc * G and P[3] == steps_since * W
        assert P[2] == 0 and P[4] == 0           # (nothing stepped, nothing accepted)
        n_, N_, sum_Ncov, sum_mean, sum_mm = CR.unpack(P, d)
        assert_bit_equal(sum_mean, CR.sequential_sum(means), f"sum_mean, checkpoint {k}")
        r_mean, r_mm, r_Ncov, abs_mm = CR.payload(means, S_sum, Nc)
        assert_bit_equal(sum_mm, sum_mm.T, "symmetry of sum_mm")
        assert_bit_equal(sum_Ncov, sum_Ncov.T, "symmetry of sum_Ncov")
        b_mm = (G + 2) * EPS * abs_mm
        err = np.abs(sum_mm.astype(LD) - r_mm)
        assert np.all(err <= b_mm), (k, float((err - b_mm).max()))
        b_cov = 2 * EPS * (np.abs(S_sum).astype(LD) + LD(Nc) * np.abs(r_mm)) + LD(Nc) * b_mm
        err = np.abs(sum_Ncov.astype(LD) - r_Ncov)
        assert np.all(err <= b_cov), (k, float((err - b_cov).max()))
    eng.close()


def test_ring_wraps_and_reloads():
    """40 checkpoints on one engine (d = 5, G = 4).  The window lengths run through 1 ... 16 in
    steps of 7 (mod 16), not in step with the slot index: on the 16-slot ring the windows of
    checkpoints 16 ... 19 span slots 15 -> 0, that of checkpoint 18 is the whole ring.  At
    checkpoint 20 the ring is reloaded from the host's intervals with a capacity of 64, at
    checkpoint 30 once more with 14 intervals into 16 slots, so that the run wraps again from
    checkpoint 32 on (the whole ring at 34).  Integer accumulators and a power-of-two sample
    count per chain make every sum, mean and product exact: the payloads EQUAL numpy's."""
    d, W, gs = 5, 256, 64
    G = W // gs
    rng = np.random.default_rng(40)
    eng = make_engine(d, W, gs)
    assert eng.ckpt_capacity == 16
    intervals, crossing, full, ring_done = [], 0, 0, 0     # (ring_done: the ring's own count)
    for k in range(40):
        if k == 20:
            eng.checkpoint_set_ring(intervals[-16:], min_capacity=64)
            assert eng.ckpt_capacity == 64
        if k == 30:
            eng.checkpoint_set_ring(intervals[-14:])
            assert eng.ckpt_capacity == 16
        g = rng.integers(-1000, 1001, (G, d)).astype(np.float64)
        A = rng.integers(-1000, 1001, (d, d))
        S = (A + A.T).astype(np.float64)
        intervals.append((1, g, S))
        window = min(k + 1, (7 * k + 1) % 16 + 1)
        crossing += (k < 20 or k >= 30) and ring_done % 16 < window - 1
        full += (k < 20 or k >= 30) and window == 16
        ring_done = 16 if k == 19 else 14 if k == 29 else ring_done + 1
        n_win = (1, 2, 4)[k % 3]             # (the caller's count: any, here a power of two)
        if k == 17:
            eng.set_moments(1, g, S)
            eng.request_moments()
            with pytest.raises(E.EngineError, match="ring capacity 16"):
                eng.checkpoint_begin(17, n_win, 1.0)
            ptr, n = eng.checkpoint_begin(window, n_win, 1.0)
            eng.checkpoint_request_payload()
            eng.fetch_moments()
            P = eng.checkpoint_fetch_payload()
        else:
            P = payload_of(eng, 1, g, S, window, n_win, 1.0)
        ivs = intervals[-window:]
        Nc = float(n_win * gs)
        means = np.sum([iv[1] for iv in ivs], axis=0) / Nc
        S_sum = np.sum([iv[2] for iv in ivs], axis=0)
        mm = means.T @ means
        n_, N_, sum_Ncov, sum_mean, sum_mm = CR.unpack(P, d)
        assert n_ == G and N_ == Nc * G, k
        assert np.array_equal(sum_mean, means.sum(0)), k
        assert np.array_equal(sum_mm, mm), k
        assert np.array_equal(sum_Ncov, S_sum - Nc * mm), k
    assert crossing >= 8 and full >= 2       # windows that spanned slots 15 -> 0; whole rings
    eng.close()


# ------------------------------------------------------------------ b. the solve kernel
BLOCKS_53 = [list(range(20, 53)), list(range(0, 20))]
_measured = {}


def _check_solved(eng, ref_eng, case_name, d, P, ref, i_of_j=None):
    R_ref, cond, _ = ref
    T_before, cov_before = eng.get_proposal_transform(), eng.get_proposal_cov()
    dev = solve(eng, P, 0.0, np.inf)
    n, N, sum_Ncov, sum_mean, sum_mm = CR.unpack(P, d)
    assert dev["status"] == 0, case_name
    rel = abs(dev["Rminus1_groups"] - R_ref) / R_ref
    q = rel / (EPS * (cond + d))
    print(f"{case_name}: R-1 {dev['Rminus1_groups']:.17g} ref {R_ref:.17g} cond {cond:.3g} "
          f"rel {rel:.3g} rel / (eps (cond + d)) {q:.4g}")
    _measured[d] = max(_measured.get(d, 0.0), q)
    assert rel <= CR.C_DEVICE * EPS * (cond + d), case_name
    assert_bit_equal(dev["mean_of_covs"], sum_Ncov / N, f"{case_name}: mean_of_covs")
    assert (dev["n_chains"], dev["sum_N"], dev["d_accepted"], dev["d_steps"], dev["accepted"]) \
        == tuple(P[:5]), case_name
    # the learn path: the host's transform of the same covariance, bit for bit
    try:
        ref_eng.set_proposal_cov(dev["mean_of_covs"])
        host_T = ref_eng.get_proposal_transform()
    except E.NotPositiveDefinite:
        host_T = None
    if host_T is None:
        assert not dev["refreshed"], case_name
        assert_bit_equal(eng.get_proposal_transform(), T_before, f"{case_name}: T untouched")
        assert_bit_equal(eng.get_proposal_cov(), cov_before, f"{case_name}: cov untouched")
        return
    assert dev["refreshed"], case_name
    T = eng.get_proposal_transform()
    assert_bit_equal(T, host_T, f"{case_name}: T")
    assert_bit_equal(eng.get_proposal_cov(), dev["mean_of_covs"], f"{case_name}: cov")
    T_ld, cond_corr = CR.proposal_transform(dev["mean_of_covs"], i_of_j, eng.cfg.proposal_scale)
    err = np.sqrt(((T.astype(LD) - T_ld) ** 2).sum())
    assert err <= 64 * d * EPS * cond_corr * np.sqrt((T_ld ** 2).sum()), (case_name, float(err))


@pytest.mark.parametrize("d,blocks", [(d, None) for d in CR.DIMS] + [(53, BLOCKS_53)])
def test_solve_kernel_on_crafted_payloads(d, blocks):
    """Every kept case of crafted_payloads() at this d, injected as the all-reduced payload
    (n_chains comes from it: the engine is one group of 64).  d = 1: no eigenproblem; 2: no
    Householder step; 26 / 27: the dynamic-LDS attribute; 52 / 53: the LDS and the global-memory
    workspace; `blocks`: the blocked parameter order (i_of_j) of the learn path.  The family's
    `-blocks` payloads (and `-diagB` at d <= 3) give an M with exact zeros below its subdiagonal:
    the "column already tridiagonal" branch of wg_lambda_max."""
    eng = make_engine(d, 64, 64, blocks)
    ref_eng = E.Engine(d, 64, group_size=64, device=0)
    i_of_j = None
    if blocks:
        ref_eng.set_blocking(blocks, [1, 2])
        i_of_j = [i for b in blocks for i in b]
    cases = [c for c in CR.crafted_payloads() if c["d"] == d and c["kept"]]
    assert len(cases) >= 8
    for c in cases:
        _check_solved(eng, ref_eng, c["name"], d, c["P"], c["ref"], i_of_j)
    print(f"d = {d}: worst rel / (eps (cond + d)) = {_measured[d]:.4g} (bound {CR.C_DEVICE:g})")
    eng.close(), ref_eng.close()


def test_solve_kernel_on_g7(golden):
    """Cobaya's own multi-chain checkpoint (six chains of unequal length)."""
    g = golden("g7_multichain")
    d = g["means"].shape[1]
    P = CR.g7_payload(g)
    ref = CR.rminus1(*CR.unpack(P, d))
    eng = make_engine(d, 64, 64)
    ref_eng = E.Engine(d, 64, group_size=64, device=0)
    _check_solved(eng, ref_eng, "g7", d, P, ref)
    eng.close(), ref_eng.close()


# ------------------------------------------------------------------ c. statuses, learning window
def _good(d):
    return CR.case(np.random.default_rng(7 + d), d, 1e4, 8)


def _refused_payloads(d):
    out = {}
    n, N, sum_Ncov, sum_mean, sum_mm = (np.array(a) for a in CR.unpack(_good(d), d))
    k = d // 2
    mm1, m1 = sum_mm.copy(), sum_mean.copy()
    mm1[k, :] = mm1[:, k] = 0.0
    m1[k] = 0.0
    out["B zero in one coordinate"] = (1, CR.pack(n, N, sum_Ncov, m1, mm1))
    # B = I exactly (no chain mean, sum_mm = (n - 1) I), so nW = W = integers / 4096 with an
    # exactly singular leading block [[4, 4], [4, 4]]: the second pivot is 4 - 2 * 2 = 0
    Wint = np.diag(np.full(d, 9.0))
    Wint[:2, :2] = 4.0
    for i in range(2, d - 1):
        Wint[i + 1, i] = Wint[i, i + 1] = 1.0
    out["W exactly singular"] = (2, CR.pack(8.0, 4096.0, 4096.0 * Wint, np.zeros(d), 7.0 * np.eye(d)))
    mm3 = sum_mm.copy()
    mm3[1, 0] = np.nan
    out["NaN in sum_mm"] = (3, CR.pack(n, N, sum_Ncov, sum_mean, mm3))
    out["one chain"] = (None, CR.pack(1.0, N / n, sum_Ncov / n, sum_mean / n, sum_mm / n))
    # (a zero on the diagonal of mean_of_covs: the learn path refuses a non-positive diagonal, but
    # the Cholesky factorisation of nW -- the same diagonal over a positive scale -- has refused
    # it before: status 2, and nothing learnt)
    cov0 = sum_Ncov.copy()
    cov0[k, :] = cov0[:, k] = 0.0
    out["zero on the diagonal of mean_of_covs"] = (2, CR.pack(n, N, cov0, sum_mean, sum_mm))
    return out


@pytest.mark.parametrize("d", [3, 60])
def test_solve_kernel_statuses(d):
    """Payloads the reference sampler skips (LinAlgError, mcmc.py:870-887) end in a status, learn
    nothing and leave the proposal as it was -- with the learning window wide open; the host
    routine refuses the same payloads.  d = 3: the LDS workspace, d = 60: global memory."""
    eng = make_engine(d, 64, 64)
    good = _good(d)
    dev = solve(eng, good, -np.inf, np.inf)
    assert dev["status"] == 0 and dev["refreshed"]
    T0, cov0 = eng.get_proposal_transform(), eng.get_proposal_cov()
    for name, (status, P) in _refused_payloads(d).items():
        dev = solve(eng, P, -np.inf, np.inf)
        if status is None:
            assert dev["status"] != 0, name
        else:
            assert dev["status"] == status, (name, dev["status"])
        assert not dev["refreshed"], name
        assert_bit_equal(eng.get_proposal_transform(), T0, f"{name}: T")
        assert_bit_equal(eng.get_proposal_cov(), cov0, f"{name}: cov")
        with pytest.raises(E.EngineError):
            E.gelman_rubin(*CR.unpack(P, d))
        assert CR.rminus1(*CR.unpack(P, d)) is None or status is None, name
    # ... and the engine still solves a good payload afterwards
    dev = solve(eng, good, np.inf, -np.inf)
    assert dev["status"] == 0 and not dev["refreshed"]
    eng.close()


@pytest.mark.parametrize("d,gs", [(3, 64), (60, 128)])
def test_learning_window_edges(d, gs):
    """The proposal is learnt iff learn_lo <= R-1 x group_size <= learn_hi, to the last bit."""
    eng = make_engine(d, gs, gs)
    P = _good(d)
    T0 = eng.get_proposal_transform()
    dev = solve(eng, P, np.inf, -np.inf)
    assert dev["status"] == 0 and not dev["refreshed"]
    assert_bit_equal(eng.get_proposal_transform(), T0, "T untouched")
    rq = dev["Rminus1_groups"] * gs
    for lo, hi in ((np.nextafter(rq, np.inf), np.inf), (-np.inf, np.nextafter(rq, -np.inf))):
        dev = solve(eng, P, lo, hi)
        assert dev["status"] == 0 and not dev["refreshed"], (lo, hi)
        assert dev["Rminus1_groups"] * gs == rq
        assert_bit_equal(eng.get_proposal_transform(), T0, "T untouched")
    dev = solve(eng, P, rq, rq)
    assert dev["status"] == 0 and dev["refreshed"]
    assert np.any(_bits(eng.get_proposal_transform()) != _bits(T0))
    assert_bit_equal(eng.get_proposal_cov(), dev["mean_of_covs"], "cov")
    eng.close()

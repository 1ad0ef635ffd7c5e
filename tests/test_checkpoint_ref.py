"""CPU tests that pin the plain reference of the checkpoint (tests/checkpoint_ref.py) -- against
Cobaya's own R-1 of golden G7 and against a 50-digit restatement -- and measure the host routine
`mcmc_hip_gelman_rubin` on the crafted family; the device's bound in
tests/test_gpu_checkpoint_kernels.py is 8 x that measurement."""
import numpy as np
import pytest

from cobaya_amd import engine as E
from tests import checkpoint_ref as CR

EPS = CR.EPS
EPS_LD = float(np.finfo(np.longdouble).eps)


def test_long_double_is_wider_than_double():
    """The reference's claim to be one rests on it (x87 extended: 64-bit significand)."""
    assert EPS_LD <= 2.0 ** -63


def test_reference_reproduces_cobayas_rminus1_of_g7(golden):
    g = golden("g7_multichain")
    d = g["means"].shape[1]
    R, cond, W = CR.rminus1(*CR.unpack(CR.g7_payload(g), d))
    assert R == pytest.approx(float(g["Rminus1"]), rel=1e-9)
    np.testing.assert_allclose(W.astype(np.float64), g["new_proposal_cov"], rtol=1e-13)


def _mp_rminus1(P, d):
    """mcmc.py:856-889 once more, at 50 digits with mpmath's own Cholesky, inverse and symmetric
    eigensolver."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    n, N, sum_Ncov, sum_mean, sum_mm = CR.unpack(P, d)
    n, N = mp.mpf(float(n)), mp.mpf(float(N))
    W = mp.matrix(d, d)
    B = mp.matrix(d, d)
    for i in range(d):
        for j in range(d):
            W[i, j] = mp.mpf(float(sum_Ncov[i, j])) / N
            B[i, j] = (mp.mpf(float(sum_mm[i, j]))
                       - mp.mpf(float(sum_mean[i])) * mp.mpf(float(sum_mean[j])) / n) / (n - 1)
    sd = [mp.sqrt(B[i, i]) for i in range(d)]
    cB, nW = mp.matrix(d, d), mp.matrix(d, d)
    for i in range(d):
        for j in range(d):
            cB[i, j] = B[i, j] / sd[i] / sd[j]
            nW[i, j] = W[i, j] / sd[i] / sd[j]
    Li = mp.inverse(mp.cholesky(nW))
    M = Li * cB * Li.T
    M = (M + M.T) / 2
    ev = mp.eigsy(M, eigvals_only=True)
    return max(abs(e) for e in ev)


def test_reference_agrees_with_50_digits(golden):
    """Error of the reference: the long-double Cholesky, inverse and products lose at most
    ~ d eps_ld cond2(nW) (taken 64-fold here), the eigenvalues of the float64 cast of M a few
    d eps of the largest one (taken as 8 d eps): rel <= 8 d eps + 64 d eps_ld cond2(nW)."""
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(12)
    cases = [(c["name"], c["d"], c["P"], c["ref"]) for c in CR.crafted_payloads()
             if c["d"] <= 12 and c["kept"]]
    for d in (7, 12):
        for c, n in ((1e4, 8), (1e8, 300)):
            P = CR.case(rng, d, c, n)
            cases.append((f"d{d}-c{c:g}-n{n}", d, P, CR.rminus1(*CR.unpack(P, d))))
    g = golden("g7_multichain")
    dg = g["means"].shape[1]
    Pg = CR.g7_payload(g)
    cases.append(("g7", dg, Pg, CR.rminus1(*CR.unpack(Pg, dg))))
    assert len(cases) >= 30
    for name, d, P, ref in cases:
        assert ref is not None, name
        R, cond, _ = ref
        Rmp = _mp_rminus1(P, d)
        rel = abs(float((R - Rmp) / Rmp))
        assert rel <= 8 * d * EPS + 64 * d * EPS_LD * cond, (name, rel, cond)


def test_reference_refuses_what_the_reference_sampler_refuses():
    d = 3
    W = np.array([[2.0, 1, 0], [1, 2, 0], [0, 0, 1]])
    sing = np.array([[1.0, 1, 0], [1, 1, 0], [0, 0, 1]])
    mm = np.diag([3.0, 3.0, 6.0])      # B = diag(1, 1, 2): the normalisation keeps the block exact
    assert CR.rminus1(4.0, 400.0, 400.0 * W, np.zeros(d), mm) is not None
    assert CR.rminus1(4.0, 400.0, 400.0 * sing, np.zeros(d), mm) is None          # W singular
    assert CR.rminus1(4.0, 400.0, 400.0 * W, np.zeros(d), np.diag([3.0, 0.0, 6.0])) is None
    assert CR.proposal_transform(sing) is None
    T, cond = CR.proposal_transform(W, scale=2.0)
    np.testing.assert_allclose((T @ T.T).astype(np.float64), 4.0 * W, rtol=1e-15)


def test_window_sums_are_the_hosts_python_sums():
    rng = np.random.default_rng(5)
    ivs = [(rng.standard_normal((4, 3)) * 10.0 ** k, rng.standard_normal((3, 3))) for k in range(5)]
    g_sum, S_sum, means = CR.window_sums(ivs, 192.0)
    assert np.array_equal(g_sum, sum(iv[0] for iv in ivs))
    assert np.array_equal(S_sum, sum(iv[1] for iv in ivs))
    assert np.array_equal(means, sum(iv[0] for iv in ivs) / 192.0)


def test_host_gelman_rubin_on_the_crafted_family():
    """Measures C_host = max over the kept cases of rel_err / (eps (cond2(nW) + d)) of the host
    routine against the long-double reference, prints it (docs/MEASUREMENTS.md, "checkpoint
    kernels") and ties the device's committed bound to it: C_host <= C_DEVICE / 8."""
    fam = CR.crafted_payloads()
    assert len(fam) == len(CR.DIMS) * 12
    dropped = [c["name"] for c in fam if not c["kept"]]
    print(f"\ncrafted_payloads: {len(fam)} cases, {len(dropped)} dropped: {dropped}")
    assert 8 * len(dropped) <= len(fam)
    assert {c["d"] for c in fam if c["kept"]} == set(CR.DIMS)
    worst, worst_cond_only, per_d = (0.0, None), (0.0, None), {}
    for c in fam:
        if not c["kept"]:
            continue
        d = c["d"]
        R_ref, cond, W_ref = c["ref"]
        n, N, sum_Ncov, sum_mean, sum_mm = CR.unpack(c["P"], d)
        R, W = E.gelman_rubin(n, N, sum_Ncov, sum_mean, sum_mm)
        assert np.array_equal(W, sum_Ncov / N), c["name"]          # one IEEE division
        rel = abs(R - R_ref) / R_ref
        q = rel / (EPS * (cond + d))
        per_d[d] = max(per_d.get(d, 0.0), q)
        if q > worst[0]:
            worst = (q, c["name"])
        if rel / (EPS * cond) > worst_cond_only[0]:
            worst_cond_only = (rel / (EPS * cond), c["name"])
    print(f"C_host = {worst[0]:.4f} at {worst[1]}; without the + d: {worst_cond_only[0]:.4f} at "
          f"{worst_cond_only[1]}")
    print("per d:", {d: round(v, 4) for d, v in per_d.items()})
    assert worst[0] <= CR.C_HOST_MEASURED * 1.0000001      # the committed measurement is current
    assert worst[0] <= CR.C_DEVICE / 8
    # ... and C_DEVICE is 8 x the measurement rounded up to a power of two, no more
    assert CR.C_DEVICE == 2.0 ** np.ceil(np.log2(8 * CR.C_HOST_MEASURED))

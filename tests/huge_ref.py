"""The d-agnostic restatement of the oracle's incremental step (tests/huge_step_ref.c), built on
first use with the system C compiler and -ffp-contract=off, as the oracle is, and bound beside the
oracle library whose exports (orc_pair_variates, orc_dexp_tab, orc_dlog_tab) it calls."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from oracle import cbind as O

HERE = os.path.dirname(os.path.abspath(__file__))
# built once per source version, beside the engine's objects (git-ignored)
BUILD = os.path.join(os.path.dirname(HERE), "cobaya_amd", "csrc", "_obj")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        O.lib()   # the oracle first, its symbols global
        C.CDLL(O.lib()._name, mode=C.RTLD_GLOBAL)
        src = os.path.join(HERE, "huge_step_ref.c")
        with open(src, "rb") as f:
            tag = hashlib.sha256(f.read()).hexdigest()[:12]
        out = os.path.join(BUILD, "libhuge_ref_%s.so" % tag)
        if not os.path.exists(out):
            os.makedirs(BUILD, exist_ok=True)
            tmp = "%s.%d.tmp" % (out, os.getpid())
            subprocess.run(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off",
                            "-fno-fast-math", src, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, out)   # (atomic: concurrent test processes see a whole library)
        _LIB = C.CDLL(out)
        _LIB.huge_ref_run.restype = C.c_int64
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(prob, state, n_steps, walker0=0, step0=0, anchor=True):
    """Advance `state` (dict: x [W][d], y [W][K][d], logpost, logprior, loglike, weight, prior_rej,
    burn_left, n_accept, stuck) by n_steps on the oracle Problem `prob` (one block, K = 1..4)."""
    d, K, gs = prob.d, prob.K, prob.group_size
    W = state["x"].shape[0]
    G = W // gs
    c0 = step0 // d
    c1 = (step0 + n_steps - 1) // d
    ncyc = c1 - c0 + 1
    V = np.empty((G, ncyc, d, d))
    for g in range(G):
        for c in range(ncyc):
            # (the cycle index is kept modulo 2^32: oracle, orc_run)
            V[g, c] = np.asarray(prob.basis(walker0 // gs + g, (c0 + c) & 0xFFFFFFFF)).reshape(d, d)
    inv = np.where(prob.kind == 1, 1.0 / prob.scale, 0.0)
    mls = np.where(prob.kind == 1, prob.mls, 0.0)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in
            (prob.lo, prob.hi, prob.loc, inv, mls, prob.scale, prob.Linv, prob.mean, prob.cnorm,
             prob.weight)]
    st = state
    tot = lib().huge_ref_run(
        C.c_int(d), C.c_int(K), C.c_int(W), C.c_int(gs), C.c_uint32(walker0), C.c_uint64(prob.seed),
        C.c_uint64(step0), C.c_int(n_steps), C.c_uint64(prob.refresh_every), C.c_int(int(anchor)),
        _p(V), C.c_uint64(c0), C.c_int(ncyc), *[_p(a) for a in arrs],
        C.c_double(prob.uniform_logp), C.c_double(prob.temperature), C.c_double(prob.max_tries),
        _p(st["x"]), _p(st["y"]), _p(st["logpost"]), _p(st["logprior"]), _p(st["loglike"]),
        _p(st["weight"]), _p(st["prior_rej"]), _p(st["burn_left"]), _p(st["n_accept"]), _p(st["stuck"]))
    return int(tot)


def fresh_state(prob, x0, burn_in=0):
    """The state the engine's set_state makes (y is formed at the first step: anchor)."""
    W, d, K = x0.shape[0], prob.d, prob.K
    lp, ll = prob.evaluate(x0)[:2]
    return {"x": np.ascontiguousarray(x0, dtype=np.float64).copy(), "y": np.zeros((W, max(K, 1), d)),
            "logpost": lp + ll, "logprior": lp.copy(), "loglike": ll.copy(),
            "weight": np.ones(W, np.int32), "prior_rej": np.zeros(W, np.int32),
            "burn_left": np.full(W, burn_in + 1, np.int32), "n_accept": np.zeros(W, np.int64),
            "stuck": np.zeros(1, np.int32)}


def gaussian_info(d, K=1, seed=0, normal_every=0, scale=0.05):
    """A cobaya input of a correlated Gaussian (K = 1) or mixture in d parameters with uniform
    priors [0, 1] (and a normal prior on every `normal_every`-th parameter); returns (info, mean, cov)."""
    rng = np.random.default_rng(seed)
    names = ["p%d" % i for i in range(d)]
    means, covs = [], []
    for _ in range(K):
        A = rng.standard_normal((d, d)) / np.sqrt(d)
        C_ = scale ** 2 * (0.5 * (A @ A.T) + 0.5 * np.eye(d))
        sd = np.sqrt(np.diag(C_))
        covs.append(C_)
        means.append(0.5 + 0.2 * sd * rng.standard_normal(d))
    params = {}
    for i, p in enumerate(names):
        if normal_every and i % normal_every == 1:
            params[p] = {"prior": {"dist": "norm", "loc": 0.5, "scale": 0.5}, "ref": float(means[0][i]),
                         "proposal": float(np.sqrt(covs[0][i, i]))}
        else:
            params[p] = {"prior": {"min": 0.0, "max": 1.0}, "ref": float(means[0][i]),
                         "proposal": float(np.sqrt(covs[0][i, i]))}
    like = {"gaussian_mixture": {"means": [m.tolist() for m in means],
                                 "covs": [c.tolist() for c in covs], "input_params_prefix": "p"}}
    return {"likelihood": like, "params": params}, means[0], covs[0]

"""The reference of a FUNCTION target's Metropolis step ("Function targets"),
built from the oracle's exports the way tests/huge_ref.py is: `Problem.basis` gives the Haar
columns V, tests/function_step_ref.c forms the un-paired variates (orc_philox, orc_dlog,
orc_sincos2pi) and the trial t = fma(r, v, x), `Problem(K = 0).evaluate` gives support and
log-prior (eval_point), and the accept half applies the Metropolis rule and the bookkeeping of
every other target.  The log-likelihoods come in from outside: `FunctionRef.accept` takes, per
step, the array the function returned for the trial (`run`: a host function of the points)."""
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
        src = os.path.join(HERE, "function_step_ref.c")
        with open(src, "rb") as f:
            tag = hashlib.sha256(f.read()).hexdigest()[:12]
        out = os.path.join(BUILD, "libfunction_ref_%s.so" % tag)
        if not os.path.exists(out):
            os.makedirs(BUILD, exist_ok=True)
            tmp = "%s.%d.tmp" % (out, os.getpid())
            subprocess.run(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off",
                            "-fno-fast-math", src, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, out)   # (atomic: concurrent test processes see a whole library)
        _LIB = C.CDLL(out)
        _LIB.fn_ref_accept.restype = C.c_int64
        _LIB.fn_ref_propose.restype = None
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def problem(d, kinds, a, b, T, group_size=64, seed=1, temperature=1.0, max_tries=None, derived=None):
    """The oracle Problem of a function target: the priors and the proposal, no mode (K = 0: its
    `evaluate` returns the log-prior, -inf outside the support, as under the `one` likelihood).
    `derived`: the prior constants the engine reports (Engine.derived_constants), so that both
    see one problem."""
    return O.Problem(d, kinds, a, b, T=T, group_size=group_size, seed=seed,
                     temperature=temperature, max_tries=max_tries, derived=derived)


def evaluate(prob, x, loglike):
    """Model.logposterior's two parts for points x[n][d]: log-prior of the K = 0 problem and the
    function's values `loglike` (an array, or a host function of the points) -- -inf outside the
    support, where the likelihood is skipped (model.py:650-653)."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    lp = prob.evaluate(x)[0]
    ll = np.asarray(loglike(x) if callable(loglike) else loglike, dtype=np.float64).copy()
    ll[np.isinf(lp)] = -np.inf
    return lp, ll


class FunctionRef:
    """Walker state (walker-major x) of a function target, stepped one trial at a time."""

    def __init__(self, prob, x0, loglike0, burn_in=0, walker0=0):
        self.p = prob
        self.walker0 = int(walker0)
        self.x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        self.W, self.d = self.x.shape
        lp, ll = evaluate(prob, self.x, loglike0)
        self.logprior, self.loglike, self.logpost = lp, ll, lp + ll
        self.weight = np.ones(self.W, np.int32)
        self.prior_rej = np.zeros(self.W, np.int32)
        self.burn_left = np.full(self.W, burn_in + 1, np.int32)
        self.n_accept = np.zeros(self.W, np.int64)
        self.stuck = np.zeros(1, np.int32)
        self.bad = np.zeros(1, np.int32)
        self.step = 0
        self.t = np.empty_like(self.x)
        self.Ea = np.empty(self.W)
        self.lp_t = np.empty(self.W)
        self._cycle, self._V = None, None

    def _columns(self):
        """The column of the current step of every group, [G][d]."""
        d, gs = self.d, self.p.group_size
        cyc, col = divmod(self.step, d)
        if cyc != self._cycle:
            g0 = self.walker0 // gs
            # (the cycle index is kept modulo 2^32: oracle, orc_run)
            self._V = np.array([self.p.basis(g0 + g, cyc & 0xFFFFFFFF) for g in range(self.W // gs)])
            self._cycle = cyc
        return np.ascontiguousarray(self._V[:, col, :])

    def propose(self):
        """Steps 1-4: the trial points [W][d] of the current step (log-prior kept for accept)."""
        v = self._columns()
        lib().fn_ref_propose(C.c_int(self.d), C.c_int(self.W), C.c_int(self.p.group_size),
                             C.c_uint32(self.walker0), C.c_uint64(self.p.seed), C.c_uint64(self.step),
                             _p(v), _p(self.x), _p(self.t), _p(self.Ea))
        self.lp_t = self.p.evaluate(self.t)[0]
        return self.t

    def accept(self, ll):
        """Steps 5-7 with the values `ll` the function returned for the trial."""
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        assert ll.shape == (self.W,)
        acc = lib().fn_ref_accept(
            C.c_int(self.d), C.c_int(self.W), C.c_uint32(self.walker0),
            C.c_double(self.p.temperature), C.c_double(self.p.max_tries), _p(self.t), _p(self.lp_t),
            _p(ll), _p(self.Ea), _p(self.x), _p(self.logpost), _p(self.logprior), _p(self.loglike),
            _p(self.weight), _p(self.prior_rej), _p(self.burn_left), _p(self.n_accept),
            _p(self.stuck), _p(self.bad))
        self.step += 1
        return int(acc)

    def run(self, n_steps, f):
        """n_steps with a host function f(points[n][d]) -> loglike[n]."""
        acc = 0
        for _ in range(n_steps):
            acc += self.accept(f(self.propose()))
        return acc

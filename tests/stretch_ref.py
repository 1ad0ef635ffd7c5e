"""The reference of the stretch move on a function target ("Stretch move"),
built as tests/function_ref.py is: tests/stretch_step_ref.c forms the variates (orc_philox, orc_dlog)
and the trial t = fma(z, x - p, p), `Problem(K = 0).evaluate` gives support and log-prior
(eval_point), and the accept half applies the rule and the bookkeeping of every other target.  The
log-likelihoods come in from outside: `StretchRef.accept` takes, per half-update, the array the
function returned for the W / 2 trial rows (`run`: a host function of the points)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from oracle import cbind as O
from tests import function_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = FR.BUILD
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        O.lib()   # the oracle first, its symbols global
        C.CDLL(O.lib()._name, mode=C.RTLD_GLOBAL)
        src = os.path.join(HERE, "stretch_step_ref.c")
        with open(src, "rb") as f:
            tag = hashlib.sha256(f.read()).hexdigest()[:12]
        out = os.path.join(BUILD, "libstretch_ref_%s.so" % tag)
        if not os.path.exists(out):
            os.makedirs(BUILD, exist_ok=True)
            tmp = "%s.%d.tmp" % (out, os.getpid())
            subprocess.run(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off",
                            "-fno-fast-math", src, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, out)   # (atomic: concurrent test processes see a whole library)
        _LIB = C.CDLL(out)
        _LIB.st_ref_accept.restype = C.c_int64
        _LIB.st_ref_propose.restype = None
        _LIB.st_ref_variates.restype = None
    return _LIB


_p = FR._p


def problem(d, kinds, a, b, group_size=64, seed=1, temperature=1.0, max_tries=None, derived=None):
    """The oracle Problem of a function target under the stretch move: the priors alone (K = 0; no
    proposal)."""
    return FR.problem(d, kinds, a, b, np.eye(d), group_size=group_size, seed=seed,
                      temperature=temperature, max_tries=max_tries, derived=derived)


def variates(seed, gid, step, group_size, a=2.0):
    """(member of the other half, z, E_a) of global walkers `gid` (an array) at `step`."""
    gid = np.atleast_1d(np.asarray(gid, dtype=np.int64))
    log2_half = int(np.log2(group_size // 2))
    m, z, Ea = C.c_int32(), C.c_double(), C.c_double()
    out = np.empty((len(gid), 3))
    for j, g in enumerate(gid):
        lib().st_ref_variates(C.c_uint64(seed), C.c_uint32(int(g)), C.c_uint64(step), C.c_int(log2_half),
                              C.c_double(a), C.byref(m), C.byref(z), C.byref(Ea))
        out[j] = m.value, z.value, Ea.value
    return out[:, 0].astype(np.int64), out[:, 1], out[:, 2]


class StretchRef:
    """Walker state (walker-major x) of a function target, moved one half-update at a time.
    `stale_partners`: half 1 reads its partners from the state BEFORE the step (the ordering the
    kernel must not have; the tests' power check)."""

    def __init__(self, prob, x0, loglike0, a=2.0, burn_in=0, walker0=0, stale_partners=False):
        self.p = prob
        self.a = float(a)
        self.walker0 = int(walker0)
        self.stale = bool(stale_partners)
        self.x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        self.W, self.d = self.x.shape
        self.gs = prob.group_size
        assert self.W % self.gs == 0
        lp, ll = FR.evaluate(prob, self.x, loglike0)
        self.logprior, self.loglike, self.logpost = lp, ll, lp + ll
        self.weight = np.ones(self.W, np.int32)
        self.prior_rej = np.zeros(self.W, np.int32)
        self.burn_left = np.full(self.W, burn_in + 1, np.int32)
        self.n_accept = np.zeros(self.W, np.int64)
        self.stuck = np.zeros(1, np.int32)
        self.bad = np.zeros(1, np.int32)
        self.step = 0
        self.half = 0
        n = self.W // 2
        self.t = np.empty((n, self.d))
        self.Ea, self.q, self.lp_t = np.empty(n), np.empty(n), np.empty(n)
        self.partner = np.empty(n, np.int32)
        self._x_before = self.x.copy()

    def active(self):
        """Local indices of the walkers of the current half, ascending."""
        hg = self.gs // 2
        k = np.arange(self.W // 2)
        return (k // hg) * self.gs + self.half * hg + k % hg

    def propose(self):
        """Steps 1-3 of the current half-update: the W / 2 trial rows (log-prior kept for accept)."""
        if self.half == 0:
            self._x_before = self.x.copy()
        xp = self._x_before if (self.stale and self.half == 1) else self.x
        lib().st_ref_propose(C.c_int(self.d), C.c_int(self.W), C.c_int(self.gs), C.c_int(self.half),
                             C.c_uint32(self.walker0), C.c_uint64(self.p.seed), C.c_uint64(self.step),
                             C.c_double(self.a), _p(self.x), _p(xp), _p(self.t), _p(self.Ea), _p(self.q),
                             _p(self.partner))
        self.lp_t = self.p.evaluate(self.t)[0]
        return self.t

    def accept(self, ll):
        """Steps 5-6 with the values `ll` the function returned for the trial rows."""
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        assert ll.shape == (self.W // 2,)
        acc = lib().st_ref_accept(
            C.c_int(self.d), C.c_int(self.W), C.c_int(self.gs), C.c_int(self.half), C.c_uint32(self.walker0),
            C.c_double(self.p.temperature), C.c_double(self.p.max_tries), _p(self.t), _p(self.lp_t),
            _p(ll), _p(self.Ea), _p(self.q), _p(self.x), _p(self.logpost), _p(self.logprior),
            _p(self.loglike), _p(self.weight), _p(self.prior_rej), _p(self.burn_left), _p(self.n_accept),
            _p(self.stuck), _p(self.bad))
        self.step += self.half
        self.half ^= 1
        return int(acc)

    def run(self, n_steps, f):
        """n_steps (2 n half-updates) with a host function f(points[n][d]) -> loglike[n]."""
        acc = 0
        for _ in range(2 * n_steps):
            acc += self.accept(f(self.propose()))
        return acc

"""The reference of the mixtures of ensemble moves on a function target (DESIGN.md section 2,
"Ensemble move mixtures"), built as tests/stretch_ref.py is: tests/moves_step_ref.c forms the
variates (orc_philox, orc_dlog, orc_sincos2pi) and the trials of the three kinds,
`Problem(K = 0).evaluate` gives support and log-prior (eval_point), and the accept half applies the
rule and the bookkeeping of every other target.  The kind of a step is chosen HERE, from the word
the C file forms, by inverse CDF over the normalised weights.  The log-likelihoods come in from
outside: `MovesRef.accept` takes, per half-update, the array the function returned for the W / 2
trial rows (`run`: a host function of the points)."""
import ctypes as C
import hashlib
import math
import os
import subprocess

import numpy as np

from oracle import cbind as O
from tests import function_ref as FR
from tests.stretch_ref import problem  # noqa: F401  (the K = 0 problem: the priors alone)

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = FR.BUILD
STRETCH, DE, SNOOKER = 0, 1, 2
KINDS = {"stretch": STRETCH, "de": DE, "snooker": SNOOKER}
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        O.lib()   # the oracle first, its symbols global
        C.CDLL(O.lib()._name, mode=C.RTLD_GLOBAL)
        src = os.path.join(HERE, "moves_step_ref.c")
        with open(src, "rb") as f:
            tag = hashlib.sha256(f.read()).hexdigest()[:12]
        out = os.path.join(BUILD, "libmoves_ref_%s.so" % tag)
        if not os.path.exists(out):
            os.makedirs(BUILD, exist_ok=True)
            tmp = "%s.%d.tmp" % (out, os.getpid())
            subprocess.run(["cc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off",
                            "-fno-fast-math", src, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, out)   # (atomic: concurrent test processes see a whole library)
        _LIB = C.CDLL(out)
        _LIB.mv_ref_accept.restype = C.c_int64
        _LIB.mv_ref_kind_word.restype = C.c_uint32
        _LIB.mv_ref_propose.restype = None
        _LIB.mv_ref_variates.restype = None
    return _LIB


_p = FR._p


def members(moves, d):
    """The option's list -> [(kind id, normalised weight, p0, p1)], defaults filled in (stretch a 2,
    de gamma 2.38 / sqrt(2 d) and sigma 1e-5, snooker gamma 1.7); weights divided by their ascending
    sum."""
    out = []
    for member in moves:
        kind, weight = member[0], float(member[1])
        par = dict(member[2]) if len(member) > 2 else {}
        if kind == "stretch":
            p0, p1 = float(par.get("a", 2.0)), 0.0
        elif kind == "de":
            g = par.get("gamma")
            p0, p1 = (2.38 / math.sqrt(2 * d) if g is None else float(g)), float(par.get("sigma", 1e-5))
        else:
            p0, p1 = float(par.get("gamma", 1.7)), 0.0
        out.append((KINDS[kind], weight, p0, p1))
    total = 0.0
    for m in out:
        total += m[1]
    return [(k, w / total, p0, p1) for k, w, p0, p1 in out]


def choose(mix, seed, step):
    """Index of the member step `step` makes: word 0 of the block (0, 0x2001, S_lo, S_hi) against
    the thresholds floor(cum_j 2^32) of the ascending cumulative weights; the last member takes the
    rest; a one-member mixture draws nothing."""
    if len(mix) == 1:
        return 0
    w0 = int(lib().mv_ref_kind_word(C.c_uint64(seed), C.c_uint64(step)))
    cum = 0.0
    for j, m in enumerate(mix[:-1]):
        cum += m[1]
        if w0 < min(int(cum * 4294967296.0), 1 << 32):
            return j
    return len(mix) - 1


def variates(seed, gid, step, group_size, kind, p0=1.0, p1=0.0, flaw=0):
    """(members[n][3] of the other half, f, E_a) of global walkers `gid` (an array) at `step`: f is z
    for a stretch trial and gamma for a DE one."""
    gid = np.atleast_1d(np.asarray(gid, dtype=np.int64))
    log2_half = int(np.log2(group_size // 2))
    m = (C.c_int32 * 3)()
    f, Ea = C.c_double(), C.c_double()
    ms, out = np.empty((len(gid), 3), np.int64), np.empty((len(gid), 2))
    for j, g in enumerate(gid):
        lib().mv_ref_variates(C.c_uint64(seed), C.c_uint32(int(g)), C.c_uint64(step), C.c_int(log2_half),
                              C.c_int(kind), C.c_double(p0), C.c_double(p1), C.c_int(flaw), m, C.byref(f),
                              C.byref(Ea))
        ms[j] = m[0], m[1], m[2]
        out[j] = f.value, Ea.value
    return ms, out[:, 0], out[:, 1]


class MovesRef:
    """Walker state (walker-major x) of a function target, moved one half-update at a time by the
    mixture `moves` (the option's list).  `flaw`: a deliberately wrong rule of moves_step_ref.c (the
    tests' power checks)."""

    def __init__(self, prob, x0, loglike0, moves, burn_in=0, walker0=0, flaw=0):
        self.p = prob
        self.walker0 = int(walker0)
        self.flaw = int(flaw)
        self.x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        self.W, self.d = self.x.shape
        self.mix = members(moves, self.d)
        self.gs = prob.group_size
        assert self.W % self.gs == 0 and self.gs // 2 >= 3
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
        self.whole = np.ones(n, np.int32)
        self.partner = np.empty((n, 3), np.int32)
        self._scratch = np.empty(2 * self.d)
        self.kind = None            # kind of the last proposal
        self.kinds_made = []        # kind of every half-update proposed

    def active(self):
        """Local indices of the walkers of the current half, ascending."""
        hg = self.gs // 2
        k = np.arange(self.W // 2)
        return (k // hg) * self.gs + self.half * hg + k % hg

    def propose(self):
        """The W / 2 trial rows of the current half-update (log-prior kept for accept)."""
        kind, _, p0, p1 = self.mix[choose(self.mix, self.p.seed, self.step)]
        self.kind = kind
        self.kinds_made.append(kind)
        lib().mv_ref_propose(C.c_int(self.d), C.c_int(self.W), C.c_int(self.gs), C.c_int(self.half),
                             C.c_uint32(self.walker0), C.c_uint64(self.p.seed), C.c_uint64(self.step),
                             C.c_int(kind), C.c_double(p0), C.c_double(p1), C.c_int(self.flaw), _p(self.x),
                             _p(self.t), _p(self.Ea), _p(self.q), _p(self.whole), _p(self.partner),
                             _p(self._scratch))
        self.lp_t = np.where(self.whole != 0, self.p.evaluate(self.t)[0], -np.inf)
        return self.t

    def accept(self, ll):
        """The accept half with the values `ll` the function returned for the trial rows."""
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        assert ll.shape == (self.W // 2,)
        acc = lib().mv_ref_accept(
            C.c_int(self.d), C.c_int(self.W), C.c_int(self.gs), C.c_int(self.half), C.c_uint32(self.walker0),
            C.c_double(self.p.temperature), C.c_double(self.p.max_tries), _p(self.t), _p(self.lp_t),
            _p(ll), _p(self.Ea), _p(self.q), _p(self.x), _p(self.logpost), _p(self.logprior),
            _p(self.loglike), _p(self.weight), _p(self.prior_rej), _p(self.burn_left), _p(self.n_accept),
            _p(self.stuck), _p(self.bad))
        self.step += self.half
        self.half ^= 1
        return int(acc)

    def run(self, n_steps, f, each=None):
        """n_steps (2 n half-updates) with a host function f(points[n][d]) -> loglike[n]; `each(self)`
        after every whole step."""
        acc = 0
        for i in range(2 * n_steps):
            acc += self.accept(f(self.propose()))
            if each is not None and i % 2 == 1:
                each(self)
        return acc

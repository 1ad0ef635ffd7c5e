"""THE REFERENCE of the evidence sums (tests/test_evidence_host.py, tests/test_gpu_evidence.py): the
rule of DESIGN.md section 2 ("Evidence") in numpy plus `oracle.cbind.dexp`.  Sums, counts and c
are compared bit for bit.

    per walker:  delta_i = x_i - m_i;  z_j = sum_{i <= j} Linv[j][i] * delta_i, ONE ascending chain
                 from +0.0, z = z + (a * b);  s = sum_j z_j * z_j likewise;
                 e = dexp(min(c - logpost, 700));  inside radius r iff s <= R2_r
    per group g (group_size walkers) and radius r:  S = sum_l (inside ? e : +0.0), one ascending
                 chain from +0.0;  acc[g][r] = acc[g][r] + S;  cnt[g][r] += inside
    clamped:     the walkers with c - logpost > 700, of all accumulations
    c:           the maximum of logpost (NaN skipped; none: 0.0) when the ellipsoid becomes active:
                 at once for the first, inside the next closing request for a staged one
"""
import numpy as np

from oracle import cbind
from tests.oracle_engine import OracleEngine

CLAMP = 700.0


def rule_linv(cov):
    """inverse of chol(C), lower triangular (numpy's; the engine's own differs in the last bits)."""
    return np.tril(np.linalg.inv(np.linalg.cholesky(np.asarray(cov, dtype=np.float64))))


def rule_c(logpost):
    lp = np.asarray(logpost, dtype=np.float64)
    lp = lp[~np.isnan(lp)]
    return float(lp.max()) if len(lp) else 0.0


def rule_s(x, m, Linv):
    """s[W] = |Linv (x - m)|^2 in the rule's order of operations; x: [W, d]."""
    x, m, Linv = (np.asarray(v, dtype=np.float64) for v in (x, m, Linv))
    W, d = x.shape
    delta = x - m
    s = np.zeros(W)
    for j in range(d):
        z = np.zeros(W)
        for i in range(j + 1):
            z = z + Linv[j, i] * delta[:, i]
        s = s + z * z
    return s


def rule_e(logpost, c):
    """(e[W], clamped[W])."""
    arg = np.float64(c) - np.asarray(logpost, dtype=np.float64)
    cl = arg > CLAMP
    t = np.where(cl, CLAMP, arg)
    return np.array([cbind.dexp(v) for v in t], dtype=np.float64), cl


def ell_flat(m, Linv, c=0.0):
    return np.concatenate((np.asarray(m, float).reshape(-1), np.asarray(Linv, float).reshape(-1), [float(c)]))


class Rule:
    """Sums, counts, the clamp counter and the two ellipsoids of one engine (or one shard)."""

    def __init__(self, d, W, group_size, r2):
        self.d, self.W, self.gs, self.G = int(d), int(W), int(group_size), int(W) // int(group_size)
        self.r2 = np.array(r2, dtype=np.float64)
        self.active = self.staged = None      # flat m | Linv | c
        self.empty()

    def empty(self):
        n_r = len(self.r2)
        self.acc, self.cnt = np.zeros((self.G, n_r)), np.zeros((self.G, n_r), np.uint64)
        self.clamped, self.n = 0, 0

    def set_ellipsoid(self, m, cov=None, logpost=None, Linv=None):
        """The first becomes active at once (c from `logpost`), a later one is staged."""
        ell = ell_flat(m, rule_linv(cov) if Linv is None else Linv)
        if self.active is None:
            ell[-1] = rule_c(logpost)
            self.active = ell
        else:
            self.staged = ell

    def accumulate(self, x, logpost):
        d = self.d
        m, Linv, c = self.active[:d], self.active[d:d + d * d].reshape(d, d), self.active[-1]
        s = rule_s(x, m, Linv)
        e, cl = rule_e(logpost, c)
        self.clamped += int(cl.sum())
        for g in range(self.G):
            sl = slice(g * self.gs, (g + 1) * self.gs)
            for r, r2 in enumerate(self.r2):
                inside = s[sl] <= r2
                S = np.float64(0.0)
                for v in np.where(inside, e[sl], 0.0):
                    S = S + v
                self.acc[g, r] = self.acc[g, r] + S
                self.cnt[g, r] += np.uint64(inside.sum())
        self.n += 1
        return s, e

    def request(self, close, logpost=None):
        out = {"sums": self.acc.copy(), "counts": self.cnt.copy(), "clamped": self.clamped, "n": self.n,
               "active": None if self.active is None else self.active.copy(),
               "staged": None if self.staged is None else self.staged.copy()}
        if close:
            self.empty()
            if self.staged is not None:
                self.active, self.staged = self.staged, None
                self.active[-1] = rule_c(logpost)
        return out

    def set(self, sums, counts, clamped, n, active=None, staged=None):
        self.acc[...] = np.asarray(sums, np.float64).reshape(self.acc.shape)
        self.cnt[...] = np.asarray(counts, np.uint64).reshape(self.cnt.shape)
        self.clamped, self.n = int(clamped), int(n)
        self.active = None if active is None else np.array(active, dtype=np.float64)
        self.staged = None if staged is None else np.array(staged, dtype=np.float64)
        if self.staged is not None:
            self.staged[-1] = 0.0


class EvOracleEngine(OracleEngine):
    """The oracle-backed engine double with the evidence methods served by `Rule`; `ev_log` keeps,
    for the tests, what happened in stream order: ("ellipsoid", staged?), ("acc", step),
    ("request", close)."""

    _evr = None

    def configure_evidence(self, r2=()):
        r2 = np.asarray(r2, dtype=np.float64).reshape(-1)
        self._evr = Rule(self.d, self.W, self.group_size, r2) if len(r2) else None
        self._ev_req, self.ev_log = None, []

    def evidence_layout(self):
        r = self._evr
        if r is None:
            return {"on": 0, "n_radii": 0, "n_groups": 0, "n_ell": 0, "active": 0, "staged": 0, "n_accumulations": 0}
        return {"on": 1, "n_radii": len(r.r2), "n_groups": r.G, "n_ell": self.d * (self.d + 1) + 1,
                "active": int(r.active is not None), "staged": int(r.staged is not None), "n_accumulations": r.n}

    def evidence_set_ellipsoid(self, centre, covmat):
        self.ev_log.append(("ellipsoid", self._evr.active is not None))
        self._evr.set_ellipsoid(centre, covmat, self._state.logpost)

    def accumulate_evidence(self):
        self.ev_log.append(("acc", int(self._state.step)))
        self._evr.accumulate(self._state.x, self._state.logpost)

    def request_evidence(self, close=True):
        assert self._ev_req is None, "an evidence request is already pending"
        self.ev_log.append(("request", bool(close)))
        self._ev_req = self._evr.request(close, self._state.logpost)

    def fetch_evidence(self):
        out, self._ev_req = self._ev_req, None
        assert out is not None, "no evidence request is pending"
        return out

    def evidence_set(self, sums, counts, clamped, n_accumulations, active=None, staged=None):
        assert self._ev_req is None, "an evidence request is pending"
        self._evr.set(sums, counts, clamped, n_accumulations, active, staged)

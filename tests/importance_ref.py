"""THE REFERENCE of the importance sums (tests/test_importance_host.py, tests/test_gpu_importance.py): the
rule of DESIGN.md section 2 ("Importance") in numpy plus `oracle.cbind.dexp`.  Sums, counts and c are
compared bit for bit.

    c[k]:        when an interval opens (its first accumulation), the maximum of the FINITE delta[k] (NaN
                 and both infinities skipped; none: 0.0); fixed for the interval and read out with it
    per walker:  delta NaN or +inf: left out, counted in `nonfinite`;  delta -inf: used with e = +0.0,
                 counted in `zero`;  otherwise arg = delta - c, e = dexp(min(arg, 700)), `clamped` counts
                 arg > 700;   b_i = x_i - s_i (s: the moment shift),   u_i = e * b_i   (one rounding each)
    per group g (group_size walkers), over its USED walkers in ascending order, ONE chain each from +0.0,
                 chain = chain + (p * q): the product and the addition are separate roundings, nothing is
                 fused:   n (an integer),   S1 = sum e,   S2 = sum e * e,   M_i = sum u_i,
                 V_i = sum u_i * b_i,   with `cov`:  Q_ij = sum u_i * b_j  (j < i; at i (i - 1) / 2 + j)
                 then  sums[k][g] = sums[k][g] + chain  (S1 | S2 | M | V | Q)
    (a walker that is left out is written here as adding +0.0 in every chain: a chain that began at +0.0
    never holds -0.0, so the bits are those of skipping it)
    on the host: C = the largest c of the window's intervals; every interval's sums are scaled by
                 exp(c - C) in float64 (S2, a sum of squares, by its square) and added in interval order;
                 log_ratio = C + ln(S1 / n), ess = S1^2 / S2, mean = s + M / S1,
                 cov = Q / S1 - (M / S1)(M / S1)^T; the errors are delete-one-group jackknives
"""
import numpy as np

from oracle import cbind
from tests.oracle_engine import OracleEngine

CLAMP = 700.0


def n_chains(d, cov):
    return 2 + 2 * d + (d * (d - 1) // 2 if cov else 0)


def rule_c(delta):
    v = np.asarray(delta, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(v.max()) if len(v) else 0.0


def rule_e(delta, c):
    """(e[W], used[W], zero[W], clamped[W]) of one alternative."""
    delta = np.asarray(delta, dtype=np.float64)
    fin = np.isfinite(delta)
    zero = np.isneginf(delta)
    with np.errstate(all="ignore"):
        arg = delta - np.float64(c)
    cl = fin & (arg > CLAMP)
    e = np.zeros(len(delta))
    for w in np.flatnonzero(fin):
        e[w] = cbind.dexp(CLAMP if cl[w] else arg[w])
    return e, fin | zero, zero, cl


def ordered_sum(p):
    """One chain from +0.0 over the rows of p, in ascending order (cumsum adds sequentially), per column."""
    out = np.empty(p.shape[1])
    with np.errstate(all="ignore"):
        for c0 in range(0, p.shape[1], 512):
            blk = np.vstack((np.zeros((1, min(512, p.shape[1] - c0))), p[:, c0:c0 + 512]))
            out[c0:c0 + 512] = np.cumsum(blk, axis=0)[-1]
    return out


def group_chain(e, b, used, cov):
    """The chains S1 | S2 | M | V | Q of ONE group: e [gs], b [gs, d], used [gs]."""
    d = b.shape[1]
    with np.errstate(all="ignore"):
        e = np.where(used, e, 0.0)
        b = np.where(used[:, None], b, 0.0)
        u = e[:, None] * b
        cols = [e[:, None], (e * e)[:, None], u, u * b]
        if cov:
            i, j = np.tril_indices(d, -1)       # (row-major: (i, j < i) at i (i - 1) / 2 + j)
            cols.append(u[:, i] * b[:, j])
    return ordered_sum(np.hstack(cols))


class Rule:
    """The open interval of one engine (or one shard)."""

    def __init__(self, d, W, group_size, cov):
        self.d, self.W, self.gs, self.G = int(d), int(W), int(group_size), int(W) // int(group_size)
        self.cov = [bool(c) for c in cov]
        self.c = np.zeros(len(self.cov))
        self.empty()

    def empty(self):
        self.sums = [np.zeros((self.G, n_chains(self.d, c))) for c in self.cov]
        self.n = np.zeros((len(self.cov), self.G), np.uint64)
        self.counters = np.zeros((len(self.cov), 3), np.uint64)      # zero, nonfinite, clamped
        self.n_acc = 0

    def accumulate(self, x, delta, shift):
        """x: [W, d] the state, delta: [n_alt, W] the log-weights, shift: [d] the moment shift."""
        x = np.asarray(x, dtype=np.float64).reshape(self.W, self.d)
        delta = np.asarray(delta, dtype=np.float64).reshape(len(self.cov), self.W)
        with np.errstate(all="ignore"):
            b = x - np.asarray(shift, dtype=np.float64)
        for k, cov in enumerate(self.cov):
            if self.n_acc == 0:
                self.c[k] = rule_c(delta[k])
            e, used, zero, cl = rule_e(delta[k], self.c[k])
            self.counters[k] += np.array([zero.sum(), (~used).sum(), cl.sum()], np.uint64)
            for g in range(self.G):
                sl = slice(g * self.gs, (g + 1) * self.gs)
                with np.errstate(all="ignore"):
                    self.sums[k][g] = self.sums[k][g] + group_chain(e[sl], b[sl], used[sl], cov)
                self.n[k, g] += np.uint64(used[sl].sum())
        self.n_acc += 1

    def request(self, close):
        out = {"sums": np.concatenate([s.reshape(-1) for s in self.sums]), "n": self.n.copy(),
               "counters": self.counters.copy(), "c": self.c.copy(), "n_acc": self.n_acc}
        if close:
            self.empty()
            self.c = np.zeros(len(self.cov))
        return out

    def set(self, part):
        flat, at = np.asarray(part["sums"], np.float64).reshape(-1), 0
        for k, s in enumerate(self.sums):
            self.sums[k] = flat[at:at + s.size].reshape(s.shape).copy()
            at += s.size
        self.n = np.array(part["n"], np.uint64).reshape(self.n.shape)
        self.counters = np.array(part["counters"], np.uint64).reshape(self.counters.shape)
        self.c = np.array(part["c"], np.float64).reshape(self.c.shape)
        self.n_acc = int(part["n_acc"])


def same(got, want, c=True):
    """A read-out of the engine against the rule's, bit for bit (the payload of a NaN is not part of the
    rule: NaN equals NaN).  `c`: also compare the centring constants (those of an interval without an
    accumulation are not part of the rule)."""
    assert got["n_acc"] == want["n_acc"], (got["n_acc"], want["n_acc"])
    keys = ("sums", "c") if c else ("sums",)
    for k in keys:
        g, w = np.asarray(got[k], np.float64).reshape(-1), np.asarray(want[k], np.float64).reshape(-1)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        ok = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
        assert ok.all(), (k, np.flatnonzero(~ok)[:8], g[~ok][:8], w[~ok][:8])
    for k in ("n", "counters"):
        assert np.array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)), (k, got[k], want[k])


class ImOracleEngine(OracleEngine):
    """The oracle-backed engine double with the importance methods served by `Rule`; the log-weight
    functions receive CPU tensors.  `im_log` keeps, for the tests, what happened in stream order:
    ("acc", step), ("request", close), ("set", n_acc)."""

    _imr = None

    def configure_importance(self, cov=()):
        cov = [bool(c) for c in cov]
        self._imr = Rule(self.d, self.W, self.group_size, cov) if cov else None
        self._im_req, self._im_delta, self.im_log = None, None, []

    def importance_layout(self):
        r = self._imr
        if r is None:
            return {"n_alt": 0, "n_groups": 0, "n_sums": 0, "offsets": [], "cov": [], "n_accumulations": 0, "x_ptr": 0}
        sizes = [r.G * n_chains(r.d, c) for c in r.cov]
        return {"n_alt": len(r.cov), "n_groups": r.G, "n_sums": int(sum(sizes)),
                "offsets": [int(v) for v in np.concatenate(([0], np.cumsum(sizes)[:-1]))],
                "cov": [int(c) for c in r.cov], "n_accumulations": r.n_acc, "x_ptr": 0}

    def importance_row_views(self):
        import torch
        if self._im_delta is None:
            self._im_delta = torch.zeros((len(self._imr.cov), self.W), dtype=torch.float64)
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(self._state.x, dtype=np.float64).T))
        return list(x.unbind(0)), self._im_delta, None

    def accumulate_importance(self, delta):
        self.im_log.append(("acc", int(self._state.step)))
        self._imr.accumulate(self._state.x, delta.numpy(), self._shift)

    def request_importance(self, close=True):
        assert self._im_req is None, "an importance request is already pending"
        self.im_log.append(("request", bool(close)))
        self._im_req = self._imr.request(close)

    def fetch_importance(self):
        out, self._im_req = self._im_req, None
        assert out is not None, "no importance request is pending"
        return out

    def importance_set(self, part):
        assert self._im_req is None, "an importance request is pending"
        self.im_log.append(("set", int(part["n_acc"])))
        self._imr.set(part)

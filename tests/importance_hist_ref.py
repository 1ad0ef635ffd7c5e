"""THE REFERENCE of the reweighted marginal histograms (tests/test_importance_marginals_host.py,
tests/test_gpu_importance_marginals.py): the rule of DESIGN.md section 2 ("Importance marginals") in numpy.
The weight e of a walker is `tests.importance_ref.rule_e`'s (the oracle's dexp), the in-range test and the
bin are `tests.test_marginals_host.rule_bins`'s; the 128-bit counters are Python ints, compared word for word.

    q = 0 for a walker that is not used, else (uint64) floor(min(e, 2^16) * 2^32); saturated counts used
    walkers with e > 2^16; a used walker adds q where the unweighted histogram adds 1 (1-D: under, over or
    its bin, a NaN nowhere; pair: outside or its bin); the words are lo = total mod 2^64, hi = total >> 64.
"""
import numpy as np

from tests.importance_ref import ImOracleEngine, rule_e
from tests.test_marginals_host import MargOracleEngine, rule_bins

CAP, FRAC = 65536.0, 32
MASK = (1 << 64) - 1


def rule_q(e, used):
    """(q [W] uint64, saturated [W] bool) of one alternative."""
    e = np.asarray(e, dtype=np.float64)
    q = np.floor(np.minimum(e, CAP) * 2.0 ** FRAC).astype(np.uint64)     # (exact: a product by a power of two)
    return np.where(used, q, np.uint64(0)), used & (e > CAP)


def rule_add(x, q, dims1, bins1, pairs, bins2, lo, hi):
    """What one accumulation adds, per counter of the marginals slab's layout: uint64 (a sum of at most
    2^13 weights of at most 2^48 each cannot wrap).  x [W, d + m]: the state with the derived rows."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for i in dims1:
        inside, k = rule_bins(x[:, i], lo[i], hi[i], bins1)
        e = np.zeros(bins1 + 2, np.uint64)
        e[0] = q[x[:, i] < lo[i]].sum(dtype=np.uint64)
        e[1] = q[x[:, i] > hi[i]].sum(dtype=np.uint64)
        np.add.at(e, 2 + k[inside], q[inside])
        out.append(e)
    for i, j in pairs:
        in_i, ki = rule_bins(x[:, i], lo[i], hi[i], bins2)
        in_j, kj = rule_bins(x[:, j], lo[j], hi[j], bins2)
        inside = in_i & in_j
        e = np.zeros(bins2 * bins2 + 1, np.uint64)
        e[0] = q[~inside].sum(dtype=np.uint64)
        np.add.at(e, 1 + ki[inside] * bins2 + kj[inside], q[inside])
        out.append(e)
    assert len(x) <= 1 << 13
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def words(tot):
    """Python ints -> (lo, hi) uint64."""
    return (np.array([t & MASK for t in tot], dtype=np.uint64), np.array([t >> 64 for t in tot], dtype=np.uint64))


class HistRule:
    """The open interval of the histograms of one engine (or shard).  `on` [n_alt]; `mg`: the marginals'
    dims1, bins1, pairs, bins2, lo, hi.  The interval, c and n_acc are the sums': the caller passes c."""

    def __init__(self, on, mg):
        self.on, self.mg = [bool(v) for v in on], mg
        self.alts = [k for k, v in enumerate(self.on) if v]
        e1 = len(mg["dims1"]) * (mg["bins1"] + 2) if mg["dims1"] else 0
        e2 = len(mg["pairs"]) * (mg["bins2"] ** 2 + 1) if mg["pairs"] else 0
        self.n_counters = e1 + e2
        self.empty()

    def empty(self):
        self.tot = [[0] * self.n_counters for _ in self.alts]
        self.sat = [0] * len(self.alts)

    def accumulate(self, x, delta, c):
        """x [W, d + m], delta [n_alt, W], c [n_alt]: the interval's centring constants."""
        for h, k in enumerate(self.alts):
            e, used, _, _ = rule_e(delta[k], c[k])
            q, sat = rule_q(e, used)
            add = rule_add(x, q, **self.mg)
            self.tot[h] = [t + int(a) for t, a in zip(self.tot[h], add)]
            self.sat[h] += int(sat.sum())

    def request(self, close, n_acc):
        lo, hi = zip(*(words(t) for t in self.tot)) if self.alts else ((), ())
        out = {"lo": np.array(lo, np.uint64).reshape(len(self.alts), self.n_counters),
               "hi": np.array(hi, np.uint64).reshape(len(self.alts), self.n_counters),
               "saturated": np.array(self.sat, np.uint64), "n_acc": int(n_acc)}
        if close:
            self.empty()
        return out

    def set(self, part):
        lo, hi = (np.asarray(part[k], np.uint64).reshape(len(self.alts), self.n_counters) for k in ("lo", "hi"))
        self.tot = [[(int(b) << 64) + int(a) for a, b in zip(lo[h], hi[h])] for h in range(len(self.alts))]
        self.sat = [int(v) for v in np.asarray(part["saturated"]).reshape(-1)]


def same_hist(got, want):
    """A histogram read-out of the engine against the rule's, word for word."""
    assert got["n_acc"] == want["n_acc"], (got["n_acc"], want["n_acc"])
    for k in ("lo", "hi", "saturated"):
        g, w = np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), (k, len(bad), bad[:6].tolist(), g[g != w][:6], w[g != w][:6])


class HistOracleEngine(ImOracleEngine, MargOracleEngine):
    """The oracle-backed double with the importance and the marginal methods plus the four of the
    reweighted histograms, served by `HistRule`.  `hist_log` keeps what happened: ("configure", on),
    ("set", n)."""

    _hr = None

    def configure_importance(self, cov=()):
        super().configure_importance(cov)
        self._hr, self._hr_req = None, None

    def configure_marginals(self, *a, **k):
        super().configure_marginals(*a, **k)
        self._hr, self._hr_req = None, None

    def configure_importance_hist(self, on):
        assert self._imr is not None and getattr(self, "_mg", None) is not None, "importance and marginals first"
        assert len(on) == len(self._imr.cov)
        self.hist_log = getattr(self, "hist_log", []) + [("configure", [bool(v) for v in on])]
        self._hr = HistRule(on, self._mg) if any(on) else None
        self._hr_req = None

    def importance_hist_layout(self):
        r = self._hr
        if r is None:
            return {"n_hist": 0, "on": [False] * len(self._imr.cov) if self._imr else [], "n_counters": 0, "n_words": 0}
        return {"n_hist": len(r.alts), "on": list(r.on), "n_counters": r.n_counters,
                "n_words": len(r.alts) * (2 * r.n_counters + 1)}

    def accumulate_importance(self, delta):
        super().accumulate_importance(delta)
        if self._hr is not None:       # (c is the interval's: the sums' rule has just taken or kept it)
            self._hr.accumulate(self._state.x, delta.numpy(), self._imr.c)

    def request_importance(self, close=True):
        n_acc = self._imr.n_acc
        super().request_importance(close)
        if self._hr is not None:
            assert self._hr_req is None, "an importance histogram read-out is pending"
            self._hr_req = self._hr.request(close, n_acc)

    def fetch_importance_hist(self):
        out, self._hr_req = self._hr_req, None
        assert out is not None, "no importance histogram read-out is pending"
        return out

    def importance_hist_set(self, part):
        self.hist_log.append(("set", int(np.asarray(part["lo"]).size)))
        self._hr.set(part)

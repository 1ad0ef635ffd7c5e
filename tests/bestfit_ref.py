"""THE REFERENCE of the best-fit records and profiles (tests/test_bestfit_host.py,
tests/test_gpu_bestfit.py): the rule of DESIGN.md section 2 ("Best fit and profiles") in numpy.
Everything is compared on keys and integers, bit for bit.

    key(v):  b = bits(v); b ^= (b >> 63) ? ~0 : 1 << 63   -- NaN skipped, 0 = empty
    records: 0 `map` = maximum of logpost, 1 `bestfit` = maximum of loglike; words [key, global
             walker id, step, bits(logpost), bits(logprior), bits(loglike), bits(x[d])]; within an
             accumulation ties go to the lowest walker id, a later accumulation needs a strictly
             greater key; a merge takes the greater key, then the lower step, then the lower id
    slab:    [n][B]; bin min(floor((x - lo) * s), B - 1), s = B / (hi - lo), of the walkers with
             lo <= x <= hi holds the largest key of the profiled quantity
"""
import numpy as np

from tests.oracle_engine import OracleEngine

HEAD = 6
QUANTITIES = ("loglike", "logpost")


def rule_key(v):
    """The ordering keys of float64 values, through Python integers (NaN -> 0)."""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    out = np.zeros(v.shape, np.uint64)
    for idx, b in np.ndenumerate(v.view(np.uint64)):
        b = int(b)
        if v[idx] != v[idx]:
            continue
        out[idx] = (b ^ 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b ^ (1 << 63))
    return out


def rule_bins(x, lo, hi, B):
    """(in-range mask, bin of every value; the bin of an out-of-range value is meaningless)."""
    x = np.asarray(x, dtype=np.float64)
    s = np.float64(B) / (np.float64(hi) - np.float64(lo))
    inside = (x >= lo) & (x <= hi)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.minimum(np.floor((x - np.float64(lo)) * s), B - 1)
    return inside, np.where(inside, k, 0).astype(np.int64)


def rule_merge_records(a, b):
    out = np.array(a, dtype=np.uint64)
    for r in range(2):
        ka, kb = int(a[r][0]), int(b[r][0])
        if kb == 0:
            continue
        if ka == 0 or kb > ka or (kb == ka and (int(b[r][2]), int(b[r][1])) < (int(a[r][2]), int(a[r][1]))):
            out[r] = b[r]
    return out


class Rule:
    """Slab, records and the number of accumulations of one engine (or one shard of walkers)."""

    def __init__(self, d, dims, bins, lo, hi, quantity="loglike", walker_offset=0):
        self.d, self.dims, self.bins = int(d), [int(i) for i in dims], int(bins)
        self.lo = None if lo is None else np.array(lo, dtype=np.float64)
        self.hi = None if hi is None else np.array(hi, dtype=np.float64)
        assert quantity in QUANTITIES
        self.quantity, self.walker_offset = quantity, int(walker_offset)
        self.empty()

    def empty(self):
        n = len(self.dims)
        self.slab = np.zeros((n, self.bins if n else 0), np.uint64)
        self.records = np.zeros((2, HEAD + self.d), np.uint64)
        self.n = 0

    def accumulate(self, st):
        """st: {"x": [W, d], "logpost", "logprior", "loglike": [W], "step"} as get_full_state gives."""
        x = np.asarray(st["x"], dtype=np.float64)
        f = {k: np.asarray(st[k], dtype=np.float64) for k in ("logpost", "logprior", "loglike")}
        val = f[self.quantity]
        vkey = rule_key(val)
        for e, i in enumerate(self.dims):
            inside, k = rule_bins(x[:, i], self.lo[i], self.hi[i], self.bins)
            m = inside & (vkey != 0)
            np.maximum.at(self.slab[e], k[m], vkey[m])
        for r, name in enumerate(("logpost", "loglike")):
            keys = rule_key(f[name])
            best = int(keys.max())
            if best == 0 or best <= int(self.records[r, 0]):
                continue
            w = int(np.flatnonzero(keys == np.uint64(best))[0])      # the lowest id
            words = np.concatenate(([f["logpost"][w], f["logprior"][w], f["loglike"][w]], x[w])).view(np.uint64)
            self.records[r, 0] = best
            self.records[r, 1] = self.walker_offset + w
            self.records[r, 2] = int(st["step"])
            self.records[r, 3:] = words
        self.n += 1

    def read_and_empty(self):
        out = (self.slab.copy(), self.records.copy(), self.n)
        self.empty()
        return out

    def set(self, slab, records, n):
        self.slab[...] = np.asarray(slab, np.uint64).reshape(self.slab.shape)
        self.records[...] = np.asarray(records, np.uint64).reshape(self.records.shape)
        self.n = int(n)


def rule_over(states, d, dims, bins, lo, hi, quantity="loglike", walker_offset=0):
    """(slab, records, n) of the rule over a list of states, in their order."""
    r = Rule(d, dims, bins, lo, hi, quantity, walker_offset)
    for st in states:
        r.accumulate(st)
    return r.slab, r.records, r.n


class BfOracleEngine(OracleEngine):
    """The oracle-backed engine double with the best-fit methods served by `Rule`; it keeps every
    accumulated state for the tests."""

    _bfr = None

    def configure_bestfit(self, dims=(), bins=64, lo=None, hi=None, quantity="loglike"):
        self._bf_cfg = dict(dims=[int(i) for i in dims], bins=int(bins),
                            lo=None if lo is None else np.array(lo, float),
                            hi=None if hi is None else np.array(hi, float), quantity=quantity)
        self._bfr = Rule(self.d, walker_offset=self.walker_offset, **self._bf_cfg)
        self._bf_req = None
        self.bf_states = []

    def bestfit_layout(self):
        r = self._bfr
        if r is None:
            return {"on": 0, "n": 0, "bins": 0, "quantity": "loglike", "n_slab": 0, "n_records": 0}
        return {"on": 1, "n": len(r.dims), "bins": r.bins if r.dims else 0, "quantity": r.quantity,
                "n_slab": r.slab.size, "n_records": r.records.size}

    def accumulate_bestfit(self):
        s = self._state
        st = {"x": s.x.copy(), "logpost": s.logpost.copy(), "logprior": s.logprior.copy(),
              "loglike": s.loglike.copy(), "step": int(s.step)}
        self.bf_states.append(st)
        self._bfr.accumulate(st)

    def request_bestfit(self):
        assert self._bf_req is None, "a bestfit request is already pending"
        self._bf_req = self._bfr.read_and_empty()

    def fetch_bestfit(self):
        out, self._bf_req = self._bf_req, None
        assert out is not None, "no bestfit request is pending"
        return out

    def bestfit_set(self, slab, records, n_accumulations):
        assert self._bf_req is None, "a bestfit request is pending"
        self._bfr.set(slab, records, n_accumulations)

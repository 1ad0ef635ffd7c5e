"""THE REFERENCE of the autocorrelation sums (tests/test_autocorr_host.py, tests/test_gpu_autocorr.py):
the rule of DESIGN.md section 2 ("Autocorrelation") in numpy.

A sequential loop over the `group_size` walkers of a group and over the groups, vectorised over the
lags and the dimensions, reproduces the kernel's chains exactly: every sum is ONE chain in ascending
order from +0.0, `S = S + a`, `P = P + (a * b)` with the product rounded on its own (numpy forms it
as a temporary), and the accumulators add the groups in ascending order from their current value.
"""
import numpy as np

from tests.oracle_engine import OracleEngine


class Rule:
    """The ring of the last `lags + 1` snapshots with their group sums, the open accumulators
    sums[3][lags + 1][n] (P, A, B) and n_pairs[lags + 1]."""

    def __init__(self, dims, lags, group_size, shift):
        self.dims = [int(i) for i in dims]
        self.lags, self.gs = int(lags), int(group_size)
        self.shift = np.array(shift, dtype=np.float64)
        self.ring = []        # (a[G, gs, n], S[G, n]), the newest last
        n = len(self.dims)
        self.sums = np.zeros((3, self.lags + 1, n))
        self.n_pairs = np.zeros(self.lags + 1, np.int64)
        self.abs_sums = np.zeros((3, self.lags + 1, n))   # sum of |P_g|, |S_g|: for error bounds

    @property
    def held(self):
        return len(self.ring)

    def set_shift(self, shift):
        shift = np.array(shift, dtype=np.float64)
        if not np.array_equal(shift, self.shift):     # a CHANGE clears the ring and the sums
            self.ring = []
            self.sums[...] = 0
            self.abs_sums[...] = 0
            self.n_pairs[...] = 0
        self.shift = shift

    def accumulate(self, x):
        """x[W, d]: the ensemble as `get_state()["x"]` returns it."""
        x = np.asarray(x, dtype=np.float64)
        W, n, gs = len(x), len(self.dims), self.gs
        G = W // gs
        a = (x[:, self.dims] - self.shift[self.dims]).reshape(G, gs, n)
        S = np.zeros((G, n))
        for l in range(gs):
            S = S + a[:, l, :]
        self.ring = (self.ring + [(a, S)])[-(self.lags + 1):]
        h = len(self.ring)
        b = np.stack([self.ring[-1 - k][0] for k in range(h)])      # [h, G, gs, n]
        Sk = np.stack([self.ring[-1 - k][1] for k in range(h)])     # [h, G, n]
        P = np.zeros((h, G, n))
        for l in range(gs):
            P = P + (a[None, :, l, :] * b[:, :, l, :])
        for g in range(G):
            self.sums[0, :h] += P[:, g]
            self.sums[1, :h] += S[g][None, :]
            self.sums[2, :h] += Sk[:, g]
            self.abs_sums[0, :h] += np.abs(P[:, g])
            self.abs_sums[1, :h] += np.abs(S[g])[None, :]
            self.abs_sums[2, :h] += np.abs(Sk[:, g])
        self.n_pairs[:h] += 1

    def read_and_zero(self):
        out = (self.sums.copy(), self.n_pairs.copy())
        self.sums[...] = 0
        self.abs_sums[...] = 0
        self.n_pairs[...] = 0
        return out

    def set(self, sums, n_pairs):
        self.sums[...] = np.asarray(sums, dtype=np.float64).reshape(self.sums.shape)
        self.n_pairs[...] = n_pairs

    def reset(self):
        self.ring = []


def rule_window(snapshots, dims, lags, group_size, shift, dropped, counts, n_first_ring=None):
    """What the sampler's product must hold: the rule over ALL accumulated `snapshots` with the
    accumulators read out and zeroed where the window's intervals begin and end (`dropped`
    snapshots precede the window, `counts` are the snapshots of its intervals; where the earlier,
    dropped intervals ended does not matter: zeroing does not touch the ring), summed over the window
    in its order plus the unfinished interval.  `n_first_ring`: the ring was emptied after that
    many snapshots (a resume)."""
    r = Rule(dims, lags, group_size, shift)
    bounds = np.cumsum([dropped] + list(counts)).tolist()
    parts = []
    for t, x in enumerate(snapshots):
        if t in bounds:
            parts.append(r.read_and_zero())
        if t == n_first_ring:
            r.reset()
        r.accumulate(x)
    if len(snapshots) in bounds:
        parts.append(r.read_and_zero())
    parts.append((r.sums, r.n_pairs))
    parts = parts[1:]              # (the first read-out holds what preceded the window)
    assert len(parts) == len(counts) + 1
    sums, n = np.zeros_like(parts[0][0]), np.zeros_like(parts[0][1])
    for s_, n_ in parts:
        sums = sums + s_
        n = n + n_
    return sums, n


class AcOracleEngine(OracleEngine):
    """The oracle-backed engine double with the seven autocorrelation methods served by `Rule`; it
    keeps every accumulated snapshot for the tests."""

    _acr = None

    def configure_autocorr(self, dims=(), lags=16):
        dims = [int(i) for i in dims]
        self.ac_snapshots = []
        self._ac_req = None
        self._acr = Rule(dims, lags, self.group_size, self._shift) if dims else None

    def set_moment_shift(self, shift):
        super().set_moment_shift(shift)
        if self._acr is not None:
            self._acr.set_shift(shift)

    def autocorr_layout(self):
        r = self._acr
        if r is None:
            return {"n_dims": 0, "lags": 0, "n_doubles": 0, "held": 0}
        return {"n_dims": len(r.dims), "lags": r.lags, "n_doubles": r.sums.size, "held": r.held}

    def accumulate_autocorr(self):
        x = self._state.x.copy()
        self.ac_snapshots.append(x)
        self._acr.accumulate(x)

    def request_autocorr(self):
        assert self._ac_req is None, "an autocorr request is already pending"
        self._ac_req = self._acr.read_and_zero()

    def fetch_autocorr(self):
        out, self._ac_req = self._ac_req, None
        assert out is not None, "no autocorr request is pending"
        return out

    def autocorr_set(self, sums, n_pairs):
        assert self._ac_req is None, "an autocorr request is pending"
        self._acr.set(sums, n_pairs)

    def autocorr_reset(self):
        self._acr.reset()

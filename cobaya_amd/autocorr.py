"""Integrated autocorrelation times of the ensemble: the product (`AutoCorr`) and the sampler option
behind it (`parse_option`).

The sums come from the engine (mcmc_hip_autocorr_*; autocorr_kernels.hip), which multiplies every
moment snapshot of the window with the previous `lags` snapshots, walker by walker.  The rule
("Autocorrelation"): per lag k the engine holds accP[k] = sum a b,
accA[k] = sum a, accB[k] = sum b over the N[k] accumulations that held the lag (a: the newer
snapshot minus the moment shift, b: the snapshot k back), and with n_k = N[k] W

    C_k = accP[k] / n_k - (accA[k] / n_k) (accB[k] / n_k),    rho_k = C_k / C_0,
    tau(M) = 1 + 2 sum_{k=1..M} rho_k,

tau taken at the smallest M >= 1 with M >= c tau(M) (Sokal's window, c = 5).  Where no M <= lags
qualifies the parameter is flagged as not converged and tau(lags) is a lower bound.  One lag is
`interval_steps` sampler steps.
"""
from __future__ import annotations

import math

import numpy as np

MAX_LAGS = 64               # autocorr_args.h: kAcMaxLags
DEFAULT_LAGS = 16
OPTION_KEYS = ("params", "lags")


class AutoCorrError(ValueError):
    """An `autocorr` option (or a pair of products) that cannot be served; the message begins with
    the option's name."""


class AutoCorr:
    """Lagged cross-products of the ensemble and what follows from them.

    `params`: names, in the engine's order; `sums`: float64 [3][lags + 1][n] (P, A, B);
    `n_pairs`: int64 [lags + 1], the accumulations that held each lag; `n_walkers`: walkers every
    accumulation summed over (all processes' when combined); `interval_steps`: sampler steps between
    two accumulated snapshots."""

    def __init__(self, params, lags, interval_steps, n_walkers, sums=None, n_pairs=None):
        self.params = [str(p) for p in params]
        self.lags, self.interval_steps, self.n_walkers = int(lags), int(interval_steps), int(n_walkers)
        if not 1 <= self.lags <= MAX_LAGS:
            raise AutoCorrError(f"autocorr: lags must be an integer in 1..{MAX_LAGS}, got {lags!r}")
        shape = (3, self.lags + 1, len(self.params))
        self.sums = (np.zeros(shape) if sums is None
                     else np.array(sums, dtype=np.float64).reshape(-1))
        if self.sums.size != int(np.prod(shape)):
            raise AutoCorrError(f"autocorr: this layout holds {int(np.prod(shape))} sums, got {self.sums.size}")
        self.sums = self.sums.reshape(shape)
        self.n_pairs = (np.zeros(self.lags + 1, np.int64) if n_pairs is None
                        else np.array(n_pairs, dtype=np.int64).reshape(-1))
        if len(self.n_pairs) != self.lags + 1:
            raise AutoCorrError(f"autocorr: n_pairs holds lags + 1 = {self.lags + 1} counts, got {len(self.n_pairs)}")

    # -- layout
    def _layout(self):
        return tuple(self.params), self.lags, self.interval_steps, self.n_walkers

    def _index(self, name):
        try:
            return self.params.index(name)
        except ValueError:
            raise KeyError(f"no autocorrelation of {name!r} (have {self.params})") from None

    def held(self):
        """The largest lag any accumulation held (0: nothing beyond the variance)."""
        k = np.flatnonzero(self.n_pairs > 0)
        return int(k[-1]) if len(k) else 0

    # -- the estimator
    def covariance(self, name):
        """C_k, k = 0 .. lags (NaN where the lag was never held)."""
        i = self._index(name)
        n = self.n_pairs.astype(np.float64) * np.float64(self.n_walkers)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sums[0, :, i] / n - (self.sums[1, :, i] / n) * (self.sums[2, :, i] / n)

    def rho(self, name):
        """rho_k, k = 0 .. lags; rho[0] == 1.0."""
        c = self.covariance(name)
        with np.errstate(invalid="ignore", divide="ignore"):
            return c / c[0]

    def _sokal(self, name, c):
        """(tau, M, converged): the first M >= 1 with M >= c tau(M); else tau at the last held lag."""
        rho, last = self.rho(name), self.held()
        if last < 1 or not np.all(np.isfinite(rho[:last + 1])):
            return float("nan"), 0, False
        taus = 1.0 + 2.0 * np.cumsum(rho[1:last + 1])
        for M in range(1, last + 1):
            if M >= c * taus[M - 1]:
                return float(taus[M - 1]), M, True
        return float(taus[-1]), last, False

    def tau(self, name, c=5.0):
        """The integrated autocorrelation time in snapshots; a LOWER BOUND where
        `converged(name)` is False."""
        return self._sokal(name, c)[0]

    def window(self, name, c=5.0):
        """The M at which tau was taken."""
        return self._sokal(name, c)[1]

    def converged(self, name, c=5.0):
        """Whether Sokal's window was reached within `lags`."""
        return self._sokal(name, c)[2]

    def tau_steps(self, name, c=5.0):
        return self.tau(name, c) * self.interval_steps

    def n_samples(self):
        """n_0: the walkers of every accumulation."""
        return int(self.n_pairs[0]) * self.n_walkers

    def ess(self, name, c=5.0):
        """n_0 / tau: the independent samples among the accumulated walkers."""
        return self.n_samples() / self.tau(name, c)

    def thin(self, name=None, c=5.0):
        """(snapshots, steps) between two decorrelated snapshots: ceil(tau), at least 1; the
        maximum over the parameters when `name` is None."""
        names = self.params if name is None else [name]
        taus = [self.tau(n, c) for n in names]
        if not taus or not all(math.isfinite(t) for t in taus):
            raise AutoCorrError("autocorr: no lag beyond 0 has been accumulated yet")
        k = max(1, int(math.ceil(max(taus))))
        return k, k * self.interval_steps

    def worst(self, c=5.0):
        """(name, tau, converged) of the parameter with the largest tau (None without a finite one)."""
        best = None
        for n in self.params:
            t, _, ok = self._sokal(n, c)
            if math.isfinite(t) and (best is None or t > best[1]):
                best = (n, t, ok)
        return best

    # -- arithmetic, files
    def __add__(self, other):
        if not isinstance(other, AutoCorr):
            return NotImplemented
        if self._layout() != other._layout():
            raise AutoCorrError("autocorr: only sums of the same layout (parameters, lags, interval and "
                                "walkers) add up")
        return AutoCorr(self.params, self.lags, self.interval_steps, self.n_walkers,
                        self.sums + other.sums, self.n_pairs + other.n_pairs)

    def __eq__(self, other):
        return (isinstance(other, AutoCorr) and self._layout() == other._layout()
                and np.array_equal(self.sums, other.sums) and np.array_equal(self.n_pairs, other.n_pairs))

    __hash__ = None

    def save(self, path):
        extra = {}
        for i, n in enumerate(self.params):   # (for a reader without this class)
            extra[f"rho_{i}"] = self.rho(n)
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, params=np.array(self.params, dtype=str),
                     geometry=np.array([self.lags, self.interval_steps, self.n_walkers], dtype=np.int64),
                     sums=self.sums, n_pairs=self.n_pairs,
                     tau=np.array([self.tau(n) for n in self.params], dtype=np.float64),
                     converged=np.array([self.converged(n) for n in self.params], dtype=bool), **extra)

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        lags, interval, W = (int(v) for v in z["geometry"])
        return cls([str(p) for p in z["params"]], lags, interval, W, z["sums"], z["n_pairs"])


# ---------------------------------------------------------------------------------- the option
def parse_option(opt, sampled):
    """The sampler option `autocorr` -> None (off) or {"params": [names], "lags": L}.  `True` = every
    sampled parameter, 16 lags.  Refuses, by the option's name, unknown keys and parameter names,
    a parameter listed twice and `lags` outside 1..64."""
    if opt is None or opt is False:
        return None
    sampled = list(sampled)
    if opt is True:
        opt = {}
    if not isinstance(opt, dict):
        raise AutoCorrError(f"autocorr: expected True, None or a dict, got {opt!r}")
    unknown = sorted(set(opt) - set(OPTION_KEYS))
    if unknown:
        raise AutoCorrError(f"autocorr: unknown key(s) {unknown}; valid keys: {list(OPTION_KEYS)}")
    params = opt.get("params", "all")
    if isinstance(params, str):
        if params != "all":
            raise AutoCorrError(f"autocorr: params must be a list of names or 'all', got {params!r}")
        params = list(sampled)
    params = [str(p) for p in (params or [])]
    if not params:
        raise AutoCorrError("autocorr: params lists nothing (use None to turn the option off)")
    bad = sorted({n for n in params if n not in sampled})
    if bad:
        raise AutoCorrError(f"autocorr: unknown parameter name(s) {bad}; the sampled parameters are {sampled}")
    if len(set(params)) != len(params):
        twice = sorted({n for n in params if params.count(n) > 1})
        raise AutoCorrError(f"autocorr: params lists {twice} twice")
    lags = opt.get("lags", DEFAULT_LAGS)
    if isinstance(lags, bool) or not isinstance(lags, (int, np.integer, float)) or int(lags) != lags \
            or not 1 <= int(lags) <= MAX_LAGS:
        raise AutoCorrError(f"autocorr: lags must be an integer in 1..{MAX_LAGS}, got {lags!r}")
    return {"params": params, "lags": int(lags)}

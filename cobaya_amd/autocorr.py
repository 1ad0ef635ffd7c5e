"""Integrated autocorrelation times of the ensemble: the product (`AutoCorr`), the sampler option
behind it (`parse_option`) and what the sampler holds of it while it runs (`AutoCorrAccumulator`).

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

from .engine import EngineError
from .product import DeviceProduct, option_dict, option_int

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

    def summary(self, c=5.0):
        """One line for the log at the end of a run."""
        worst = self.worst(c)
        if worst is None:
            return "Autocorrelation: no lag beyond 0 was accumulated."
        if worst[2]:
            return ("Autocorrelation: largest tau = %.4g steps (%s); a snapshot every %d "
                    "steps decorrelates the rows." % (worst[1] * self.interval_steps, worst[0],
                                                      self.thin(c=c)[1]))
        return ("Autocorrelation: the window was not reached within %d lags of %d steps "
                "(%s: tau > %.4g steps); raise lags or moments_every." % (
                    self.lags, self.interval_steps, worst[0], worst[1] * self.interval_steps))

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
    opt = option_dict(opt, "autocorr", OPTION_KEYS, AutoCorrError)
    if opt is None:
        return None
    sampled = list(sampled)
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
    lags = option_int(opt.get("lags", DEFAULT_LAGS), "autocorr: lags", 1, MAX_LAGS, AutoCorrError)
    return {"params": params, "lags": lags}


# ---------------------------------------------------------------------------------- the sampler's side
ENGINE_METHODS = ("configure_autocorr", "accumulate_autocorr", "request_autocorr", "fetch_autocorr",
                  "autocorr_set", "autocorr_reset", "autocorr_layout")


class AutoCorrAccumulator(DeviceProduct):
    """What the sampler holds of the sums while it runs: a device product whose unfinished interval
    is never split.  A part is (sums, pairs per lag); the peek reads out and sets back."""

    name, error, ENGINE_METHODS = "autocorr", AutoCorrError, ENGINE_METHODS
    predates = "autocorr: this engine has no lagged cross-products (its library predates mcmc_hip_autocorr_*)"

    @staticmethod
    def parse(opt, spec):
        return parse_option(opt, spec.sampled)

    @classmethod
    def from_option(cls, opt, spec, engine_factory, host):
        self = super().from_option(opt, spec, engine_factory, host)
        if self is not None:
            self.cfg["interval_steps"] = int(host.snapshot_steps)   # one lag, fixed for the run
        return self

    def attach(self, engine, resumed=False, centre=None, covmat=None):
        """Hand the configuration to the engine (which allocates the ring, or refuses it)."""
        cfg, self.engine = self.cfg, engine
        try:
            engine.configure_autocorr([self.spec.sampled.index(n) for n in cfg["params"]], cfg["lags"])
        except EngineError as e:
            self.host.fail("autocorr: %s", str(e), cause=e)
        lay = engine.autocorr_layout()
        if (lay["n_dims"], lay["lags"]) != (len(cfg["params"]), cfg["lags"]):
            self.host.fail("autocorr: the engine lays its sums out differently (%r) from the product", lay)
        self.open = self._zero()

    def _zero(self):
        L1 = self.cfg["lags"] + 1
        return np.zeros((3, L1, len(self.cfg["params"]))), np.zeros(L1, np.int64)

    def product(self, intervals, combined=False, pending=False):
        """The intervals of the window, in their order, plus the unfinished interval."""
        cfg, host = self.cfg, self.host
        sums, n_pairs = self._zero()
        for s_, n_ in self._parts(pending):
            sums = sums + s_
            n_pairs = n_pairs + n_
        n_walkers = int(host.n_walkers)
        if combined and host.size > 1:
            # ONE host all-reduce, here and not in the loop; every process has accumulated the same
            # snapshots, so the pair counts must agree
            buf = np.concatenate((sums.reshape(-1), n_pairs.astype(np.float64), [float(n_walkers)]))
            host.all_reduce_sum(buf)
            L1 = cfg["lags"] + 1
            if not np.array_equal(buf[-1 - L1:-1], n_pairs.astype(np.float64) * host.size):
                host.fail("autocorr: the processes hold different pair counts (this one %r, the sum "
                          "over %d processes %r)", n_pairs.tolist(), host.size, buf[-1 - L1:-1].tolist())
            sums, n_walkers = buf[:-1 - L1].reshape(sums.shape), int(buf[-1])
        return AutoCorr(cfg["params"], cfg["lags"], cfg["interval_steps"], n_walkers, sums, n_pairs)

    def save(self, pending):
        cfg, n = self.cfg, len(self.ivs)
        open_s, open_n = self._peek(pending)
        L1, n_par = cfg["lags"] + 1, len(cfg["params"])
        return {"ac_params": np.array(cfg["params"], dtype=str),
                "ac_geometry": np.array([cfg["lags"], cfg["interval_steps"]], dtype=np.int64),
                "ac_iv": np.array([s_ for s_, _ in self.ivs], dtype=np.float64).reshape(n, 3, L1, n_par),
                "ac_iv_pairs": np.array([n_ for _, n_ in self.ivs], dtype=np.int64).reshape(n, L1),
                "ac_open": open_s, "ac_open_pairs": open_n}

    def load(self, z, n_intervals):
        """Resume: the configuration must be the one the sums were formed with; the sums of the
        window's intervals and of the unfinished one come back, the ring does not (it refills: the
        pairs that bridge the resume point are missing)."""
        cfg, fail = self.cfg, self.host.fail
        if "ac_iv" not in z:
            fail("autocorr: cannot resume -- the run was written without autocorr (the window "
                 "of its sums cannot begin in mid-run)")
        saved = ([str(p) for p in z["ac_params"]], int(z["ac_geometry"][0]), int(z["ac_geometry"][1]))
        if saved != (cfg["params"], cfg["lags"], cfg["interval_steps"]):
            fail("autocorr: cannot resume -- the run was written with params %r, lags %d and %d "
                 "steps per lag, and now has %r, %d and %d (sums of different lags do not add "
                 "up)", *saved, cfg["params"], cfg["lags"], cfg["interval_steps"])
        self.ivs = [(np.array(s_, dtype=np.float64), np.array(n_, dtype=np.int64))
                    for s_, n_ in zip(z["ac_iv"], z["ac_iv_pairs"])]
        if len(self.ivs) != n_intervals:
            fail("autocorr: the state file holds %d interval sums for %d intervals",
                 len(self.ivs), n_intervals)
        # the unfinished interval goes back to the device, where the next accumulation adds to it
        self.engine.autocorr_set(z["ac_open"], z["ac_open_pairs"])
        self.open = (np.array(z["ac_open"], dtype=np.float64), np.array(z["ac_open_pairs"], dtype=np.int64))

"""Streaming marginal histograms of the ensemble: the product (`Marginals`), the sampler option
behind it (`parse_option`, `resolve_ranges`) and what the sampler holds of it while it runs
(`MarginalsAccumulator`, which also states the methods every device product has).

The counts come from the engine (mcmc_hip_marginals_*; marginal_kernels.hip), which adds every
walker of every moment snapshot of the window -- not only the rows `max_rows` retains.  The rule
("Marginals"): on an axis of B bins over [lo, hi] a value is in range iff
lo <= x <= hi and falls in bin min(floor((x - lo) * s), B - 1) with s = B / (hi - lo); x == hi
falls in the last bin, a value on an interior edge in the upper one.

Function-derived parameters (`cobaya_amd.derived`) are histogrammed like sampled ones, from the rows
the engine keeps of them; each needs an explicit `ranges` entry (it has no prior).  Only they can be
NaN: a NaN compares false with everything, so in a 1-D entry it is counted NOWHERE (neither in a bin
nor under nor over), and in a pair it is counted `outside`.

`WeightedMarginals` holds the same histograms under the weights of an importance alternative
(`cobaya_amd.importance`; DESIGN.md section 2, "Importance marginals").
"""
from __future__ import annotations

import numpy as np

from .engine import EngineError
from .product import DeviceProduct, option_dict, option_int, option_ranges

MAX_BINS_1D = 1024          # marginal_args.h: kMargMaxBins1
MAX_BINS_2D = 64            # marginal_args.h: kMargMaxBins2
MAX_SLAB_BYTES = 64 << 20   # the uint64 slab (and its pinned read-out) one process may take
OPTION_KEYS = ("params", "pairs", "bins", "bins2d", "ranges")


class MarginalsError(ValueError):
    """A `marginals` option (or a pair of products) that cannot be served; the message begins
    with the option's name."""


def slab_size(n1, bins, n2, bins2d):
    """Counters of the slab: per 1-D entry [under, over, bins], per pair [outside, bins2d^2]."""
    return (n1 * (bins + 2) if n1 else 0) + (n2 * (bins2d * bins2d + 1) if n2 else 0)


class Marginals:
    """1-D and 2-D histograms over fixed ranges.

    `params`: names of the 1-D entries; `pairs`: (row name, column name) of the 2-D entries;
    `ranges`: {name: (lo, hi)} of every name in use; `slab`: the uint64 counters in the engine's
    layout (1-D entry k at k (bins + 2): [under, over, c_0 ..]; pair p behind them at
    p (bins2d^2 + 1): [outside, c_00 ..] row-major, first name = row); `n_accumulations`: ensemble
    snapshots added; `n_samples`: walkers added (accumulations x walkers)."""

    def __init__(self, params, pairs, bins, bins2d, ranges, slab=None, n_accumulations=0,
                 n_samples=0):
        self.params = [str(p) for p in params]
        self.pairs = [(str(a), str(b)) for a, b in pairs]
        self.bins, self.bins2d = int(bins), int(bins2d)
        self.ranges = {str(k): (float(v[0]), float(v[1])) for k, v in ranges.items()}
        for name in self.names_in_use():
            if name not in self.ranges:
                raise MarginalsError(f"marginals: no range for parameter {name!r}")
        n = slab_size(len(self.params), self.bins, len(self.pairs), self.bins2d)
        self.slab = (np.zeros(n, np.uint64) if slab is None
                     else np.array(slab, dtype=np.uint64).reshape(-1))
        if len(self.slab) != n:
            raise MarginalsError(f"marginals: this layout holds {n} counters, got {len(self.slab)}")
        self.n_accumulations, self.n_samples = int(n_accumulations), int(n_samples)

    # -- layout
    def names_in_use(self):
        seen = list(self.params)
        for a, b in self.pairs:
            seen += [n for n in (a, b) if n not in seen]
        return seen

    def _layout(self):
        return (tuple(self.params), tuple(self.pairs), self.bins, self.bins2d,
                tuple((n,) + self.ranges[n] for n in self.names_in_use()))

    def _entry(self, name):
        try:
            k = self.params.index(name)
        except ValueError:
            raise KeyError(f"no 1-D marginal of {name!r} (have {self.params})") from None
        return self.slab[k * (self.bins + 2):(k + 1) * (self.bins + 2)]

    def _entry2d(self, a, b):
        try:
            p = self.pairs.index((a, b))
        except ValueError:
            raise KeyError(f"no 2-D marginal of ({a!r}, {b!r}) (have {self.pairs}; the order "
                           "matters: the first name is the row)") from None
        n2 = self.bins2d * self.bins2d + 1
        off = len(self.params) * (self.bins + 2) if self.params else 0
        return self.slab[off + p * n2:off + (p + 1) * n2]

    # -- counts
    def counts(self, name):
        """uint64 [bins]: the walkers per bin of `name`."""
        return self._entry(name)[2:].copy()

    def counts2d(self, a, b):
        """uint64 [bins2d, bins2d]: rows follow `a`, columns `b`."""
        return self._entry2d(a, b)[1:].reshape(self.bins2d, self.bins2d).copy()

    def outside(self, name, b=None):
        """1-D: (under, over) of `name`; with a second name the `outside` count of that pair
        (a walker either coordinate of which left its range)."""
        if b is not None:
            return int(self._entry2d(name, b)[0])
        e = self._entry(name)
        return int(e[0]), int(e[1])

    def edges(self, name, bins=None):
        """The bins + 1 edges of `name` (`bins`: default the 1-D bin count; pass `bins2d` for the
        axis of a pair)."""
        lo, hi = self.ranges[name]
        return np.linspace(lo, hi, (self.bins if bins is None else int(bins)) + 1)

    # -- derived
    def density(self, name):
        """Counts normalised to integrate to 1 over [lo, hi] (what fell outside is left out)."""
        c = self.counts(name).astype(np.float64)
        lo, hi = self.ranges[name]
        total = c.sum()
        if total == 0:
            raise MarginalsError(f"marginals: no sample of {name!r} inside its range")
        return c / (total * ((hi - lo) / self.bins))

    def density2d(self, a, b):
        c = self.counts2d(a, b).astype(np.float64)
        (alo, ahi), (blo, bhi) = self.ranges[a], self.ranges[b]
        total = c.sum()
        if total == 0:
            raise MarginalsError(f"marginals: no sample of ({a!r}, {b!r}) inside its ranges")
        return c / (total * ((ahi - alo) / self.bins2d) * ((bhi - blo) / self.bins2d))

    def mean(self, name):
        """Sum of bin centres weighted by the counts: within half a bin width of the mean of the
        samples when none fell outside."""
        c = self.counts(name).astype(np.float64)
        e = self.edges(name)
        return float((c * 0.5 * (e[:-1] + e[1:])).sum() / c.sum())

    def quantile(self, name, q):
        """The value below which a fraction q of the in-range samples lies, linear inside a bin."""
        q = np.asarray(q, dtype=np.float64)
        if np.any((q < 0) | (q > 1)):
            raise MarginalsError("marginals: a quantile lies in [0, 1]")
        c = self.counts(name).astype(np.float64)
        if c.sum() == 0:
            raise MarginalsError(f"marginals: no sample of {name!r} inside its range")
        cum = np.concatenate(([0.0], np.cumsum(c)))
        target = q * cum[-1]
        # the bin in which the cumulative count reaches the target (empty bins are skipped)
        k = np.clip(np.searchsorted(cum, target, side="left") - 1, 0, self.bins - 1)
        e = self.edges(name)
        frac = np.where(c[k] > 0, (target - cum[k]) / np.where(c[k] > 0, c[k], 1.0), 0.0)
        out = e[k] + frac * (e[k + 1] - e[k])
        return float(out) if out.ndim == 0 else out

    # -- arithmetic, files
    def __add__(self, other):
        if not isinstance(other, Marginals):
            return NotImplemented
        if self._layout() != other._layout():
            raise MarginalsError("marginals: only histograms of the same layout (parameters, pairs, "
                                 "bins and ranges) add up")
        return Marginals(self.params, self.pairs, self.bins, self.bins2d, self.ranges,
                         self.slab + other.slab, self.n_accumulations + other.n_accumulations,
                         self.n_samples + other.n_samples)

    def __eq__(self, other):
        return (isinstance(other, Marginals) and self._layout() == other._layout()
                and np.array_equal(self.slab, other.slab)
                and (self.n_accumulations, self.n_samples) == (other.n_accumulations, other.n_samples))

    __hash__ = None

    def save(self, path):
        names = self.names_in_use()
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, params=np.array(self.params, dtype=str),
                     pairs=np.array(self.pairs, dtype=str).reshape(-1, 2),
                     bins=np.array([self.bins, self.bins2d], dtype=np.int64),
                     range_names=np.array(names, dtype=str),
                     ranges=np.array([self.ranges[n] for n in names], dtype=np.float64).reshape(-1, 2),
                     slab=self.slab,
                     n=np.array([self.n_accumulations, self.n_samples], dtype=np.int64))

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        ranges = {str(n): (float(r[0]), float(r[1])) for n, r in zip(z["range_names"], z["ranges"])}
        return cls([str(p) for p in z["params"]], [(str(a), str(b)) for a, b in z["pairs"]],
                   int(z["bins"][0]), int(z["bins"][1]), ranges, z["slab"], int(z["n"][0]),
                   int(z["n"][1]))


class WeightedMarginals(Marginals):
    """The histograms of `Marginals` under the weights of an importance alternative
    (`Importance.marginals(name)`): float64 weights in the same layout -- names, pairs, bins and ranges
    are those of the run's `marginals`, so both overlay bin for bin -- and the arithmetic of `Marginals`
    (`edges`, `density`, `density2d`, `mean`, `quantile`).

    `slab`: float64, the sums of the weights in units of exp(`log_scale`) (the centring constant C of
    the alternative; no ratio -- density, mean, quantile -- depends on it); `saturated`: used walkers whose
    weight lay above 2^16 times the largest one their interval opened with, and entered as 2^16;
    `n_accumulations`, `n_samples`: snapshots and walkers looked at."""

    def __init__(self, params, pairs, bins, bins2d, ranges, slab=None, n_accumulations=0, n_samples=0,
                 saturated=0, log_scale=0.0):
        super().__init__(params, pairs, bins, bins2d, ranges, None, n_accumulations, n_samples)
        if slab is not None:
            slab = np.array(slab, dtype=np.float64).reshape(-1)
            if len(slab) != len(self.slab):
                raise MarginalsError(f"marginals: this layout holds {len(self.slab)} weights, got {len(slab)}")
        self.slab = np.zeros(len(self.slab)) if slab is None else slab
        self.saturated, self.log_scale = int(saturated), float(log_scale)

    def weights(self, name):
        """float64 [bins]: the sum of the weights per bin of `name`."""
        return self.counts(name)

    def weights2d(self, a, b):
        """float64 [bins2d, bins2d]: rows follow `a`, columns `b`."""
        return self.counts2d(a, b)

    def outside(self, name, b=None):
        """As `Marginals.outside`, as weights."""
        if b is not None:
            return float(self._entry2d(name, b)[0])
        e = self._entry(name)
        return float(e[0]), float(e[1])

    def merge(self, other):
        """The weights of two shards of one run, added at their common scale."""
        if not isinstance(other, WeightedMarginals) or self._layout() != other._layout() \
                or self.n_accumulations != other.n_accumulations:
            raise MarginalsError("marginals: only weighted histograms of one run (layout and accumulations) merge")
        C = max(self.log_scale, other.log_scale)
        slab = self.slab * np.exp(self.log_scale - C) + other.slab * np.exp(other.log_scale - C)
        return WeightedMarginals(self.params, self.pairs, self.bins, self.bins2d, self.ranges, slab,
                                 self.n_accumulations, self.n_samples + other.n_samples,
                                 self.saturated + other.saturated, C)

    def __add__(self, other):
        return self.merge(other) if isinstance(other, WeightedMarginals) else NotImplemented

    def __eq__(self, other):
        return (isinstance(other, WeightedMarginals) and self._layout() == other._layout()
                and np.array_equal(self.slab, other.slab, equal_nan=True)
                and (self.n_accumulations, self.n_samples, self.saturated, self.log_scale)
                == (other.n_accumulations, other.n_samples, other.saturated, other.log_scale))

    __hash__ = None

    def save(self, path):
        names = self.names_in_use()
        with open(path, "wb") as f:
            np.savez(f, params=np.array(self.params, dtype=str),
                     pairs=np.array(self.pairs, dtype=str).reshape(-1, 2),
                     bins=np.array([self.bins, self.bins2d], dtype=np.int64),
                     range_names=np.array(names, dtype=str),
                     ranges=np.array([self.ranges[n] for n in names], dtype=np.float64).reshape(-1, 2),
                     weights=self.slab, log_scale=np.float64(self.log_scale),
                     n=np.array([self.n_accumulations, self.n_samples, self.saturated], dtype=np.int64))

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        ranges = {str(n): (float(r[0]), float(r[1])) for n, r in zip(z["range_names"], z["ranges"])}
        return cls([str(p) for p in z["params"]], [(str(a), str(b)) for a, b in z["pairs"]],
                   int(z["bins"][0]), int(z["bins"][1]), ranges, z["weights"], int(z["n"][0]), int(z["n"][1]),
                   int(z["n"][2]), float(z["log_scale"]))


# ---------------------------------------------------------------------------------- the option
def parse_option(opt, sampled, derived=()):
    """The sampler option `marginals` -> None (off) or a dict
    {"params": [names], "pairs": [(a, b)], "bins", "bins2d", "ranges": dict | "prior" | "covmat"}.
    `True` = every sampled parameter in 1-D, no pairs.  Refuses, by the option's name, unknown
    keys and parameter names, pairs of one parameter, bin counts out of range and a slab above
    64 MiB.  `derived`: the names of function-derived parameters, which `params`, `pairs` and
    `ranges` may list beside the sampled ones ("all" stays the sampled ones); each needs an explicit
    `ranges` entry."""
    opt = option_dict(opt, "marginals", OPTION_KEYS, MarginalsError, {"params": "all"})
    if opt is None:
        return None
    sampled, derived = list(sampled), [str(n) for n in derived]
    known = sampled + derived
    params = opt.get("params", "all")
    if isinstance(params, str):
        if params != "all":
            raise MarginalsError(f"marginals: params must be a list of names or 'all', got {params!r}")
        params = list(sampled)
    params = [str(p) for p in (params or [])]
    pairs = opt.get("pairs", None)
    if isinstance(pairs, str):
        if pairs != "all":
            raise MarginalsError(f"marginals: pairs must be a list of [a, b], 'all' or None, got {pairs!r}")
        pairs = [(a, b) for k, a in enumerate(sampled) for b in sampled[k + 1:]]
    out_pairs = []
    for pr in pairs or []:
        if isinstance(pr, str) or len(pr) != 2:
            raise MarginalsError(f"marginals: pairs holds [a, b] entries, got {pr!r}")
        out_pairs.append((str(pr[0]), str(pr[1])))
    bad = sorted({n for n in params if n not in known}
                 | {n for pr in out_pairs for n in pr if n not in known})
    if bad:
        raise MarginalsError(f"marginals: unknown parameter name(s) {bad}; the sampled parameters "
                             f"are {sampled}")
    if len(set(params)) != len(params):
        raise MarginalsError("marginals: params lists a parameter twice")
    for a, b in out_pairs:
        if a == b:
            raise MarginalsError(f"marginals: the pair [{a!r}, {b!r}] needs two different parameters")
    if not params and not out_pairs:
        raise MarginalsError("marginals: neither params nor pairs lists anything (use None to turn "
                             "the option off)")
    bins = option_int(opt.get("bins", 128), "marginals: bins", 1, MAX_BINS_1D, MarginalsError)
    bins2d = option_int(opt.get("bins2d", 32), "marginals: bins2d", 1, MAX_BINS_2D, MarginalsError)
    nbytes = 8 * slab_size(len(params), bins, len(out_pairs), bins2d)
    if nbytes > MAX_SLAB_BYTES:
        raise MarginalsError(f"marginals: {len(params)} parameters x {bins} bins and {len(out_pairs)} "
                             f"pairs x {bins2d}^2 bins take {nbytes} bytes of counters, above the "
                             f"{MAX_SLAB_BYTES} allowed: list fewer pairs or lower bins2d")
    ranges = option_ranges(opt.get("ranges", "prior"), "marginals", known, MarginalsError)
    in_use = params + [n for pr in out_pairs for n in pr]
    unranged = sorted({n for n in in_use if n in derived and not (isinstance(ranges, dict) and n in ranges)})
    if unranged:
        raise MarginalsError(f"marginals: derived parameter(s) {unranged} need an explicit ranges entry "
                             "(ranges: {name: [lo, hi]}): a derived parameter has no prior")
    return {"params": params, "pairs": out_pairs, "bins": bins, "bins2d": bins2d, "ranges": ranges}


def resolve_ranges(cfg, spec, centre=None, covmat=None):
    """{name: (lo, hi)} of every parameter in use.  An explicit entry wins; the rest follow the
    mode: "prior" (also behind a dict) -- the bounds of a uniform prior, loc +- 5 scale of a normal
    one; "covmat" -- centre +- 5 sigma of `covmat` (the initial points' mean and the proposal
    covariance in force at initialize()), clipped to the prior support."""
    names = list(cfg["params"])
    for pr in cfg["pairs"]:
        names += [n for n in pr if n not in names]
    explicit = cfg["ranges"] if isinstance(cfg["ranges"], dict) else {}
    mode = cfg["ranges"] if isinstance(cfg["ranges"], str) else "prior"
    out = {}
    for n in names:
        if n in explicit:
            out[n] = explicit[n]
            continue
        if n not in spec.sampled:
            raise MarginalsError(f"marginals: derived parameter {n!r} needs an explicit ranges entry: it "
                                 "has no prior")
        i = spec.sampled.index(n)
        uniform = int(spec.kinds[i]) == 0
        a, b = float(spec.a[i]), float(spec.b[i])
        plo, phi = (a, b) if uniform else (a - 5.0 * b, a + 5.0 * b)
        if mode == "covmat":
            if centre is None or covmat is None:
                raise MarginalsError("marginals: ranges: 'covmat' needs the initial points and the "
                                     "proposal covariance")
            sig = float(np.sqrt(covmat[i, i]))
            lo, hi = float(centre[i]) - 5.0 * sig, float(centre[i]) + 5.0 * sig
            if uniform:
                lo, hi = max(lo, a), min(hi, b)
        else:
            lo, hi = plo, phi
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise MarginalsError(f"marginals: ranges: {mode!r} gives [{lo}, {hi}] for {n!r}; give it "
                                 "an explicit range")
        out[n] = (lo, hi)
    return out


# ---------------------------------------------------------------------------------- the sampler's side
ENGINE_METHODS = ("configure_marginals", "accumulate_marginals", "request_marginals",
                  "fetch_marginals", "marginals_set")


class MarginalsAccumulator(DeviceProduct):
    """What the sampler holds of the histograms while it runs: a device product whose unfinished
    interval is split.  A part is (counts, accumulations); `ivs` keeps the counts.  Where the
    counts are held changes no sum."""

    name, reports, split, error, ENGINE_METHODS = "marginals", False, True, MarginalsError, ENGINE_METHODS
    tempered = ("marginals: the histograms count the walkers as they are, which at temperature %g "
                "follow the tempered law, not the posterior; use temperature: 1 or turn marginals off")
    predates = "marginals: this engine has no marginal histograms (its library predates mcmc_hip_marginals_*)"

    @staticmethod
    def parse(opt, spec):
        return parse_option(opt, spec.sampled, [f.name for f in getattr(spec, "derived_functions", ())])

    @staticmethod
    def _merge(a, b):
        return a[0] + b[0], int(a[1]) + int(b[1])

    def _empty(self):
        return np.zeros(self.cfg["n_counters"], np.uint64), 0

    def _kept(self, part):
        return part[0]

    def attach(self, engine, resumed=False, centre=None, covmat=None):
        """Fix the ranges and hand the layout to the engine.  A resumed run repeats the ranges of
        the state file: `load` configures the engine."""
        self.engine = engine
        if resumed:
            return
        try:
            ranges = resolve_ranges(self.cfg, self.spec, centre, covmat)
        except MarginalsError as e:
            self.host.fail("%s", str(e), cause=e)
        self._configure(ranges)

    def _configure(self, ranges):
        cfg, fail = self.cfg, self.host.fail
        # (the rows of the function-derived parameters follow the sampled ones: index d + r)
        names = list(self.spec.sampled) + [f.name for f in getattr(self.spec, "derived_functions", ())]
        ix = names.index
        cfg["resolved"] = dict(ranges)
        lo, hi = np.full(len(names), np.nan), np.full(len(names), np.nan)
        for n, (a, b) in cfg["resolved"].items():
            lo[ix(n)], hi[ix(n)] = a, b
        try:
            self.engine.configure_marginals([ix(n) for n in cfg["params"]], cfg["bins"],
                                            [(ix(a), ix(b)) for a, b in cfg["pairs"]], cfg["bins2d"], lo, hi)
        except EngineError as e:
            fail("marginals: %s", str(e), cause=e)
        cfg["n_counters"] = slab_size(len(cfg["params"]), cfg["bins"], len(cfg["pairs"]), cfg["bins2d"])
        if hasattr(self.engine, "marginals_layout"):
            # the engine's slab is the authority: the product must read it the way it is written
            lay = self.engine.marginals_layout()
            if (lay["n_counters"], lay["offset_pairs"]) != (
                    cfg["n_counters"], slab_size(len(cfg["params"]), cfg["bins"], 0, 0)):
                fail("marginals: the engine lays its counters out differently (%r) from the "
                     "product (%d counters)", lay, cfg["n_counters"])
        self.open = self._empty()

    def product(self, intervals, combined=False, pending=False):
        cfg = self.cfg
        slab, n_acc = self._merged(intervals, pending)
        n_samples = n_acc * int(self.host.n_walkers)
        if combined and self.host.size > 1:
            # ONE host all-reduce of integers (exact in float64 below 2^53), here and not in the loop
            buf = np.concatenate((slab.astype(np.float64), [float(n_samples)]))
            if buf.max() >= 2.0 ** 53:
                self.host.fail("marginals: a count above 2^53 cannot be summed over processes exactly")
            self.host.all_reduce_sum(buf)
            slab, n_samples = buf[:-1].astype(np.uint64), int(buf[-1])
        return Marginals(cfg["params"], cfg["pairs"], cfg["bins"], cfg["bins2d"], cfg["resolved"],
                         slab, n_acc, n_samples)

    def save(self, pending):
        """What a resumed run must repeat (names, bins and ranges) and the counts it goes on from."""
        cfg = self.cfg
        self._drain(pending)
        names = list(cfg["resolved"])
        return {"marg_params": np.array(cfg["params"], dtype=str),
                "marg_pairs": np.array(cfg["pairs"], dtype=str).reshape(-1, 2),
                "marg_bins": np.array([cfg["bins"], cfg["bins2d"]], dtype=np.int64),
                "marg_range_names": np.array(names, dtype=str),
                "marg_ranges": np.array([cfg["resolved"][n] for n in names], dtype=np.float64).reshape(-1, 2),
                "marg_iv": np.array(self.ivs, dtype=np.uint64).reshape(len(self.ivs), cfg["n_counters"]),
                "marg_open": self.open[0], "marg_open_n": np.int64(self.open[1])}

    def load(self, z, n_intervals):
        """Resume: the ranges are part of the geometry -- the saved ones are taken where the option
        derives them from the run's start (`covmat`) and must be repeated where it states them."""
        cfg, fail = self.cfg, self.host.fail
        if "marg_iv" not in z:
            fail("marginals: cannot resume -- the run was written without marginals (the window "
                 "of a histogram cannot begin in mid-run)")
        saved = {str(n): (float(r[0]), float(r[1])) for n, r in zip(z["marg_range_names"], z["marg_ranges"])}
        same = ([str(p) for p in z["marg_params"]] == cfg["params"]
                and [(str(a), str(b)) for a, b in z["marg_pairs"]] == cfg["pairs"]
                and [int(v) for v in z["marg_bins"]] == [cfg["bins"], cfg["bins2d"]])
        if same and cfg["ranges"] != "covmat":
            try:
                same = resolve_ranges(cfg, self.spec) == saved
            except MarginalsError as e:
                fail("%s", str(e), cause=e)
        elif same:
            explicit = cfg["ranges"] if isinstance(cfg["ranges"], dict) else {}
            same = all(saved.get(n) == r for n, r in explicit.items() if n in saved)
        if not same:
            fail("marginals: cannot resume -- the run was written with other parameters, pairs, "
                 "bins or ranges (the counts of different bins do not add up); saved ranges: %r", saved)
        self._configure(saved)
        self.ivs = [np.array(c, dtype=np.uint64) for c in z["marg_iv"]]
        if len(self.ivs) != n_intervals:
            fail("marginals: the state file holds %d interval histograms for %d intervals",
                 len(self.ivs), n_intervals)
        # the unfinished interval goes back to the device, where the next accumulation adds to it
        self.engine.marginals_set(z["marg_open"], int(z["marg_open_n"]))

"""Best fit, MAP and profile likelihoods of the ensemble: the product (`BestFit`), the sampler option
behind it (`parse_option`) and what the sampler holds of it while it runs (`BestFitAccumulator`, a
device product with the methods `marginals.MarginalsAccumulator` states).

The keys come from the engine (mcmc_hip_bestfit_*; bestfit_kernels.hip), which looks at every
walker of every moment snapshot of the window -- not only at the rows `max_rows` retains.  The
statistic is over those SNAPSHOT POPULATIONS, not over every trial between two snapshots.  The rule
("Best fit and profiles"): the ordering key of a double v is
b ^ ((b >> 63) ? ~0 : 1 << 63) with b = bits(v) -- an unsigned 64-bit integer ordered like the
doubles, NaN skipped, 0 = empty.  A record (`map`: maximum of logpost, `bestfit`: maximum of
loglike) holds key, global walker id, step counter, logpost, logprior, loglike and x[d] of the
winner; a profile bin holds the largest key of the profiled quantity among the walkers in that bin
(the marginals' binning rule).  Everything is a maximum, hence exact: it depends neither on the
launch nor on how the walkers are sharded.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .engine import EngineError
from .marginals import MarginalsError, resolve_ranges
from .product import DeviceProduct, option_dict, option_int, option_ranges

MAX_BINS = 1024             # bestfit_args.h: kBfMaxBins
RECORD_HEAD = 6             # bestfit_args.h: kBfRecordHead -- key, walker, step, logpost, logprior, loglike
QUANTITIES = ("loglike", "logpost")
OPTION_KEYS = ("params", "bins", "ranges", "quantity")
_SIGN = np.uint64(1 << 63)


class BestFitError(ValueError):
    """A `bestfit` option (or a pair of products) that cannot be served; the message begins with
    the option's name."""


# ---------------------------------------------------------------------------------- keys, records
def key_of(v):
    """uint64 ordering keys of float64 values (NaN -> 0, "empty")."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.uint64)
    key = np.where((b >> np.uint64(63)) != 0, ~b, b ^ _SIGN)
    return np.where(np.isnan(v), np.uint64(0), key).astype(np.uint64)


def value_of(key):
    """float64 values of ordering keys (0 -> NaN)."""
    key = np.ascontiguousarray(key, dtype=np.uint64)
    b = np.where((key >> np.uint64(63)) != 0, key ^ _SIGN, ~key).astype(np.uint64)
    return np.where(key == 0, np.nan, b.view(np.float64))


def empty_records(d):
    return np.zeros((2, RECORD_HEAD + int(d)), np.uint64)


def merge_records(a, b):
    """Two [2, 6 + d] uint64 record arrays -> the winner of each row: the greater key; ties go to
    the lower step, then to the lower walker id."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    out = a.copy()
    for r in range(2):
        ka, kb = int(a[r, 0]), int(b[r, 0])
        if kb > ka or (kb == ka and kb != 0
                       and (int(b[r, 2]), int(b[r, 1])) < (int(a[r, 2]), int(a[r, 1]))):
            out[r] = b[r]
    return out


def _merge(p, q):
    """(slab, records, n) of two parts of one layout."""
    return np.maximum(p[0], q[0]), merge_records(p[1], q[1]), int(p[2]) + int(q[2])


class BestFit:
    """The two records and the profiles over fixed ranges.

    `names`: every sampled parameter, in the sampler's order (x of a record follows it); `params`:
    the profiled ones; `ranges`: {name: (lo, hi)} of those; `quantity`: what the profiles hold,
    "loglike" or "logpost"; `slab`: uint64 [len(params), bins] keys (0 = empty bin); `records`:
    uint64 [2, 6 + d] words (row 0 `map`, row 1 `bestfit`; key 0 = empty); `n_accumulations`:
    ensemble snapshots looked at; `n_samples`: walkers looked at."""

    reports = True

    def __init__(self, names, params, bins, ranges, quantity="loglike", slab=None, records=None,
                 n_accumulations=0, n_samples=0):
        self.names = [str(n) for n in names]
        self.params = [str(p) for p in params]
        self.bins = int(bins)
        self.ranges = {str(k): (float(v[0]), float(v[1])) for k, v in ranges.items()}
        if quantity not in QUANTITIES:
            raise BestFitError(f"bestfit: quantity must be one of {list(QUANTITIES)}, got {quantity!r}")
        self.quantity = str(quantity)
        for name in self.params:
            if name not in self.names:
                raise BestFitError(f"bestfit: {name!r} is not a sampled parameter")
            if name not in self.ranges:
                raise BestFitError(f"bestfit: no range for parameter {name!r}")
        shape = (len(self.params), self.bins if self.params else 0)
        self.slab = (np.zeros(shape, np.uint64) if slab is None
                     else np.array(slab, dtype=np.uint64).reshape(-1))
        if self.slab.size != shape[0] * shape[1]:
            raise BestFitError(f"bestfit: this layout holds {shape[0] * shape[1]} keys, got {self.slab.size}")
        self.slab = self.slab.reshape(shape)
        d = len(self.names)
        self.records = (empty_records(d) if records is None
                        else np.array(records, dtype=np.uint64).reshape(-1))
        if self.records.size != 2 * (RECORD_HEAD + d):
            raise BestFitError(f"bestfit: the records of {d} parameters hold {2 * (RECORD_HEAD + d)} "
                               f"words, got {self.records.size}")
        self.records = self.records.reshape(2, RECORD_HEAD + d)
        self.n_accumulations, self.n_samples = int(n_accumulations), int(n_samples)

    def _layout(self):
        return (tuple(self.names), tuple(self.params), self.bins, self.quantity,
                tuple((n,) + self.ranges[n] for n in self.params))

    # -- records
    def _record(self, r):
        w = self.records[r]
        if int(w[0]) == 0:
            return None
        f = w.view(np.float64)
        x = f[RECORD_HEAD:].copy()
        return SimpleNamespace(point={n: float(v) for n, v in zip(self.names, x)}, x=x,
                               logpost=float(f[3]), logprior=float(f[4]), loglike=float(f[5]),
                               chi2=-2.0 * float(f[5]), walker=int(w[1]), step=int(w[2]))

    @property
    def map(self):
        """The snapshot walker of the highest logpost (None: nothing was accumulated)."""
        return self._record(0)

    @property
    def bestfit(self):
        """The snapshot walker of the highest loglike (None: nothing was accumulated)."""
        return self._record(1)

    # -- profiles
    def _row(self, name):
        try:
            return self.slab[self.params.index(name)]
        except ValueError:
            raise KeyError(f"no profile of {name!r} (have {self.params})") from None

    def profile(self, name):
        """float64 [bins]: the largest `quantity` seen in every bin of `name`, NaN where empty."""
        return value_of(self._row(name))

    def edges(self, name):
        lo, hi = self.ranges[name]
        self._row(name)
        return np.linspace(lo, hi, self.bins + 1)

    def delta_chi2(self, name):
        """2 (max - profile) per bin, NaN where empty."""
        p = self.profile(name)
        if np.all(np.isnan(p)):
            raise BestFitError(f"bestfit: no sample of {name!r} inside its range")
        with np.errstate(invalid="ignore"):
            return 2.0 * (np.nanmax(p) - p)

    def interval(self, name, delta=1.0):
        """(lo, hi): the span of the bins whose delta_chi2 is within `delta` of the profile's
        maximum (from the lower edge of the first such bin to the upper edge of the last)."""
        with np.errstate(invalid="ignore"):
            k = np.flatnonzero(self.delta_chi2(name) <= float(delta))
        e = self.edges(name)
        return float(e[k[0]]), float(e[k[-1] + 1])

    def summary(self):
        """One line for the log at the end of a run."""
        m, b = self.map, self.bestfit
        if m is None and b is None:
            return "Best fit: nothing was accumulated."
        parts = []
        if b is not None:
            parts.append("best fit chi2 = %.6g (walker %d, step %d)" % (b.chi2, b.walker, b.step))
        if m is not None:
            parts.append("MAP -logpost = %.6g (walker %d, step %d)" % (-m.logpost, m.walker, m.step))
        return ("Best fit over %d snapshots of the ensemble: " % self.n_accumulations
                + "; ".join(parts) + ".")

    # -- arithmetic, files
    def merge(self, other):
        if not isinstance(other, BestFit) or self._layout() != other._layout():
            raise BestFitError("bestfit: only products of the same layout (parameters, bins, ranges "
                               "and quantity) merge")
        slab, rec, n = _merge((self.slab, self.records, self.n_accumulations),
                              (other.slab, other.records, other.n_accumulations))
        return BestFit(self.names, self.params, self.bins, self.ranges, self.quantity, slab, rec, n,
                       self.n_samples + other.n_samples)

    def __eq__(self, other):
        return (isinstance(other, BestFit) and self._layout() == other._layout()
                and np.array_equal(self.slab, other.slab) and np.array_equal(self.records, other.records)
                and (self.n_accumulations, self.n_samples) == (other.n_accumulations, other.n_samples))

    __hash__ = None

    def save(self, path):
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, names=np.array(self.names, dtype=str), params=np.array(self.params, dtype=str),
                     bins=np.array([self.bins], dtype=np.int64), quantity=np.array(self.quantity, dtype=str),
                     ranges=np.array([self.ranges[n] for n in self.params], dtype=np.float64).reshape(-1, 2),
                     slab=self.slab, records=self.records,
                     n=np.array([self.n_accumulations, self.n_samples], dtype=np.int64))

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        params = [str(p) for p in z["params"]]
        ranges = {n: (float(r[0]), float(r[1])) for n, r in zip(params, z["ranges"])}
        return cls([str(n) for n in z["names"]], params, int(z["bins"][0]), ranges, str(z["quantity"]),
                   z["slab"], z["records"], int(z["n"][0]), int(z["n"][1]))


# ---------------------------------------------------------------------------------- the option
def parse_option(opt, sampled):
    """The sampler option `bestfit` -> None (off) or a dict {"params": [names], "bins", "ranges":
    dict | "prior" | "covmat", "quantity"}.  `True` = both records and the profile of every
    sampled parameter; "params": None = the records only.  Refuses, by the option's name, unknown
    keys and parameter names, a bin count out of range, bad ranges and an unknown quantity."""
    opt = option_dict(opt, "bestfit", OPTION_KEYS, BestFitError, {"params": "all"})
    if opt is None:
        return None
    sampled = list(sampled)
    params = opt.get("params", "all")
    if isinstance(params, str):
        if params != "all":
            raise BestFitError(f"bestfit: params must be a list of names, 'all' or None, got {params!r}")
        params = list(sampled)
    params = [str(p) for p in (params or [])]
    bad = sorted({n for n in params if n not in sampled})
    if bad:
        raise BestFitError(f"bestfit: unknown parameter name(s) {bad}; the sampled parameters are {sampled}")
    if len(set(params)) != len(params):
        raise BestFitError("bestfit: params lists a parameter twice")
    bins = option_int(opt.get("bins", 64), "bestfit: bins", 1, MAX_BINS, BestFitError)
    quantity = opt.get("quantity", "loglike")
    if quantity not in QUANTITIES:
        raise BestFitError(f"bestfit: quantity must be one of {list(QUANTITIES)}, got {quantity!r}")
    ranges = option_ranges(opt.get("ranges", "prior"), "bestfit", sampled, BestFitError)
    return {"params": params, "bins": bins, "ranges": ranges, "quantity": str(quantity)}


def _resolve(cfg, spec, centre=None, covmat=None):
    """{name: (lo, hi)} of the profiled parameters: `marginals.resolve_ranges`, which knows the
    three modes, under this option's name."""
    try:
        return resolve_ranges({"params": cfg["params"], "pairs": [], "ranges": cfg["ranges"]}, spec,
                              centre, covmat)
    except MarginalsError as e:
        raise BestFitError(str(e).replace("marginals:", "bestfit:", 1)) from e


# ---------------------------------------------------------------------------------- the sampler's side
ENGINE_METHODS = ("configure_bestfit", "accumulate_bestfit", "request_bestfit", "fetch_bestfit",
                  "bestfit_set")


class BestFitAccumulator(DeviceProduct):
    """What the sampler holds of the records and profiles while it runs: a device product whose
    unfinished interval is split (a maximum is exact).  A part is (slab, records, accumulations);
    `ivs` keeps one (slab, records) per checkpoint interval of the window, dropped with it: the
    product is the maximum over the later half of the run plus the unfinished interval."""

    name, split, error, ENGINE_METHODS = "bestfit", True, BestFitError, ENGINE_METHODS
    predates = "bestfit: this engine keeps no best fit and profiles (its library predates mcmc_hip_bestfit_*)"
    _merge = staticmethod(_merge)

    @staticmethod
    def parse(opt, spec):
        return parse_option(opt, spec.sampled)

    def _kept(self, part):
        return part[:2]

    def attach(self, engine, resumed=False, centre=None, covmat=None):
        """Fix the ranges and hand the layout to the engine.  A resumed run repeats the ranges of
        the state file: `load` configures the engine."""
        self.engine = engine
        if resumed:
            return
        try:
            ranges = _resolve(self.cfg, self.spec, centre, covmat)
        except BestFitError as e:
            self.host.fail("%s", str(e), cause=e)
        self._configure(ranges)

    def _empty(self):
        cfg = self.cfg
        n = len(cfg["params"])
        return np.zeros((n, cfg["bins"] if n else 0), np.uint64), empty_records(self.spec.d), 0

    def _configure(self, ranges):
        cfg, fail, ix = self.cfg, self.host.fail, self.spec.sampled.index
        cfg["resolved"] = {n: ranges[n] for n in cfg["params"]}
        lo, hi = np.full(self.spec.d, np.nan), np.full(self.spec.d, np.nan)
        for n, (a, b) in cfg["resolved"].items():
            lo[ix(n)], hi[ix(n)] = a, b
        try:
            self.engine.configure_bestfit([ix(n) for n in cfg["params"]], cfg["bins"], lo, hi,
                                          cfg["quantity"])
        except EngineError as e:
            fail("bestfit: %s", str(e), cause=e)
        self.open = self._empty()
        if hasattr(self.engine, "bestfit_layout"):
            # the engine's layout is the authority: the product must read it the way it is written
            lay = self.engine.bestfit_layout()
            if (lay["n_slab"], lay["n_records"]) != (self.open[0].size, self.open[1].size):
                fail("bestfit: the engine lays its slab and records out differently (%r) from the "
                     "product (%d keys, %d words)", lay, self.open[0].size, self.open[1].size)

    def product(self, intervals, combined=False, pending=False):
        cfg, host = self.cfg, self.host
        slab, rec, n_acc = self._merged(intervals, pending)
        n_samples = n_acc * int(host.n_walkers)
        if combined and host.size > 1:
            # ONE host all-reduce of a zero matrix in which every process fills its own row: the
            # 64-bit words as two 32-bit halves (exact in float64), then the merge rule over the rows
            words = np.concatenate((slab.reshape(-1), rec.reshape(-1)))
            buf = np.zeros((int(host.size), 2 * len(words) + 1))
            buf[host.rank, 0:-1:2] = (words >> np.uint64(32)).astype(np.float64)
            buf[host.rank, 1:-1:2] = (words & np.uint64(0xFFFFFFFF)).astype(np.float64)
            buf[host.rank, -1] = float(n_samples)
            flat = buf.reshape(-1)
            out = host.all_reduce_sum(flat)
            buf = (flat if out is None else np.asarray(out)).reshape(buf.shape)
            n_samples = int(buf[:, -1].sum())
            rows = ((buf[:, 0:-1:2].astype(np.uint64) << np.uint64(32)) | buf[:, 1:-1:2].astype(np.uint64))
            slab = rows[:, :slab.size].max(axis=0).reshape(slab.shape)
            recs = rows[:, slab.size:].reshape((-1,) + rec.shape)
            rec = recs[0]
            for other in recs[1:]:
                rec = merge_records(rec, other)
        return BestFit(self.spec.sampled, cfg["params"], cfg["bins"], cfg["resolved"], cfg["quantity"],
                       slab, rec, n_acc, n_samples)

    def save(self, pending):
        """What a resumed run must repeat (names, bins, quantity and ranges) and the keys and
        records it goes on from."""
        cfg = self.cfg
        self._drain(pending)
        n_iv = len(self.ivs)
        return {"bf_params": np.array(cfg["params"], dtype=str),
                "bf_bins": np.array([cfg["bins"], QUANTITIES.index(cfg["quantity"])], dtype=np.int64),
                "bf_ranges": np.array([cfg["resolved"][n] for n in cfg["params"]], dtype=np.float64).reshape(-1, 2),
                "bf_iv_slab": np.array([iv[0] for iv in self.ivs], dtype=np.uint64).reshape(
                    (n_iv,) + self.open[0].shape),
                "bf_iv_rec": np.array([iv[1] for iv in self.ivs], dtype=np.uint64).reshape(
                    (n_iv,) + self.open[1].shape),
                "bf_open_slab": self.open[0], "bf_open_rec": self.open[1],
                "bf_open_n": np.int64(self.open[2])}

    def load(self, z, n_intervals):
        """Resume: the ranges are part of the geometry -- the saved ones are taken where the option
        derives them from the run's start (`covmat`) and must be repeated where it states them."""
        cfg, fail = self.cfg, self.host.fail
        if "bf_iv_slab" not in z:
            fail("bestfit: cannot resume -- the run was written without bestfit (the window of a "
                 "maximum cannot begin in mid-run)")
        params = [str(p) for p in z["bf_params"]]
        saved = {n: (float(r[0]), float(r[1])) for n, r in zip(params, z["bf_ranges"])}
        same = (params == cfg["params"]
                and [int(v) for v in z["bf_bins"]] == [cfg["bins"], QUANTITIES.index(cfg["quantity"])])
        if same and cfg["ranges"] != "covmat":
            try:
                same = _resolve(cfg, self.spec) == saved
            except BestFitError as e:
                fail("%s", str(e), cause=e)
        elif same:
            explicit = cfg["ranges"] if isinstance(cfg["ranges"], dict) else {}
            same = all(saved.get(n) == r for n, r in explicit.items() if n in saved)
        if not same:
            fail("bestfit: cannot resume -- the run was written with other parameters, bins, quantity "
                 "or ranges (the maxima of different bins do not merge); saved ranges: %r", saved)
        self._configure(saved)
        self.ivs = [(np.array(s, dtype=np.uint64), np.array(r, dtype=np.uint64))
                    for s, r in zip(z["bf_iv_slab"], z["bf_iv_rec"])]
        if len(self.ivs) != n_intervals:
            fail("bestfit: the state file holds %d interval records for %d intervals",
                 len(self.ivs), n_intervals)
        # the unfinished interval goes back to the device, where the next accumulation goes on from it
        self.engine.bestfit_set(z["bf_open_slab"], z["bf_open_rec"], int(z["bf_open_n"]))

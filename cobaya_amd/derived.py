"""Derived parameters given as batched device functions: the product (`Derived`), the sampler option
behind their statistics (`parse_option` of `derived_stats`) and what the sampler holds of them while
it runs (`DerivedAccumulator`, a device product with the methods `marginals.MarginalsAccumulator`
states; it is FIRST among the products, so that the rows of z are configured before the marginals
that may read them and filled before those bin them).

A function-derived parameter (`model.DerivedFunction`) is called with every argument bound to a 1-D
torch.float64 tensor of one entry per walker -- a zero-copy view of a row of the state x[d][W] as it
lies in HBM, or of an earlier derived row -- under the engine's stream, and returns the (n,) values.
It must be elementwise in the walker index.  The values go to the rows z[m][W] of the engine
(mcmc_hip_derived_*; derived_kernels.hip), which sums them.  The rule (DESIGN.md section 2,
"Derived"): with a_j = z_j - shift_j and b_c = x_c - (moment shift)_c, over the USED walkers -- those
all m derived values of which are finite --

    N,   A[j] = sum a_j,   B[j][k] = sum a_j a_k,   C[j][c] = sum a_j b_c,   X[c] = sum b_c,   V[c] = sum b_c^2

per group in ascending order, then over the groups in ascending order; bad[j] counts the non-finite
values and min[j] / max[j] are those of the finite ones.  `shift` is the mean of the finite derived
values of the initial ensemble, fixed for the run.

Out of scope: derived outputs returned by a `device_function` likelihood itself, fixed or
function-valued INPUT parameters, derived names in `autocorr`, `bestfit` and `evidence`,
`emit: chains`, and the hosted path (under cobaya.run.run Cobaya's Model owns derived parameters).
"""
from __future__ import annotations

import numpy as np

from .engine import ERR_CALLBACK, EngineError
from .product import DeviceProduct, option_dict

MAX_NAMES = 32              # derived_args.h: kDvMaxNames
OPTION_KEYS = ("cross",)
SUM_KEYS = ("A", "B", "C", "X", "V")


class DerivedError(ValueError):
    """A `derived_stats` option (or a pair of products) that cannot be served; the message begins
    with the option's name."""


def tri_to_full(B, m):
    """The packed lower triangle ((j, k <= j) at j (j + 1) / 2 + k) -> the symmetric [m, m] matrix."""
    full = np.zeros((m, m))
    j, k = np.tril_indices(m)
    full[j, k] = B
    full[k, j] = B
    return full


def zero_part(m, nc):
    return {"N": 0, "A": np.zeros(m), "B": np.zeros(m * (m + 1) // 2), "C": np.zeros((m, nc)), "X": np.zeros(nc),
            "V": np.zeros(nc), "bad": np.zeros(m, np.uint64), "min": np.full(m, np.nan), "max": np.full(m, np.nan),
            "n": 0}


def add_parts(a, b):
    """The sums of two intervals (float64 on the host, in the order given)."""
    out = {k: a[k] + b[k] for k in SUM_KEYS}
    out.update(N=int(a["N"]) + int(b["N"]), n=int(a["n"]) + int(b["n"]), bad=a["bad"] + b["bad"],
               min=np.fmin(a["min"], b["min"]), max=np.fmax(a["max"], b["max"]))
    return out


# ---------------------------------------------------------------------------------- the product
class Derived:
    """Moments of the function-derived parameters over the used walkers.

    `names`: the derived parameters; `cross`: the sampled parameters whose cross-moments are kept;
    `shift` [m], `xshift` [n_cross]: what the sums are taken about; `n_samples`: walkers looked at
    (accumulations x walkers), `n_used` of them with all derived values finite; `A` [m], `B` [m, m]
    (symmetric), `C` [m, n_cross], `X`, `V` [n_cross]: the sums of the rule; `bad`, `vmin`, `vmax` [m]."""

    reports = True

    def __init__(self, names, cross, shift, xshift, n_samples, n_used, A, B, C, X, V, bad, vmin, vmax):
        self.names, self.cross = [str(n) for n in names], [str(n) for n in cross]
        m, nc = len(self.names), len(self.cross)
        self.n_samples, self.n_used = int(n_samples), int(n_used)
        try:
            self.shift = np.array(shift, dtype=np.float64).reshape(m)
            self.xshift = np.array(xshift, dtype=np.float64).reshape(nc)
            self.A = np.array(A, dtype=np.float64).reshape(m)
            B = np.array(B, dtype=np.float64)
            self.B = tri_to_full(B, m) if B.shape == (m * (m + 1) // 2,) and m != 1 else B.reshape(m, m)
            self.C = np.array(C, dtype=np.float64).reshape(m, nc)
            self.X = np.array(X, dtype=np.float64).reshape(nc)
            self.V = np.array(V, dtype=np.float64).reshape(nc)
            self.bad = np.array(bad, dtype=np.uint64).reshape(m)
            self.vmin = np.array(vmin, dtype=np.float64).reshape(m)
            self.vmax = np.array(vmax, dtype=np.float64).reshape(m)
        except ValueError as e:
            raise DerivedError(f"derived_stats: the arrays of {m} names and {nc} cross parameters do not "
                               f"fit together ({e})") from None

    # -- look-ups
    def _j(self, name):
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"no derived parameter {name!r} (have {self.names})") from None

    def _c(self, name):
        try:
            return self.cross.index(name)
        except ValueError:
            raise KeyError(f"no cross-moments with {name!r} were kept (derived_stats: cross holds "
                           f"{self.cross})") from None

    def _need(self):
        if self.n_used <= 0:
            raise DerivedError("derived_stats: no walker with finite derived values was accumulated")
        return float(self.n_used)

    # -- counts and extrema
    def nonfinite(self, name):
        """How many values of `name` were NaN or infinite."""
        return int(self.bad[self._j(name)])

    def min(self, name):
        """The smallest finite value of `name` (NaN: none)."""
        return float(self.vmin[self._j(name)])

    def max(self, name):
        return float(self.vmax[self._j(name)])

    # -- moments (over the used walkers; covariances with ddof = 0, like SampleCollection.cov)
    def mean(self, name):
        j = self._j(name)
        return float(self.shift[j] + self.A[j] / self._need())

    def cov(self):
        """[m, m]: the covariance matrix of the derived parameters."""
        N = self._need()
        ma = self.A / N
        return self.B / N - np.outer(ma, ma)

    def var(self, name):
        j, N = self._j(name), self._need()
        return float(self.B[j, j] / N - (self.A[j] / N) ** 2)

    def std(self, name):
        return float(np.sqrt(max(self.var(name), 0.0)))

    def cross_cov(self, name, sampled):
        """The covariance of derived `name` with the sampled parameter `sampled`."""
        j, c, N = self._j(name), self._c(sampled), self._need()
        return float(self.C[j, c] / N - (self.A[j] / N) * (self.X[c] / N))

    def sampled_mean(self, sampled):
        """The mean of a sampled parameter over the same (used) walkers."""
        c = self._c(sampled)
        return float(self.xshift[c] + self.X[c] / self._need())

    def corr(self, name, other):
        """The correlation coefficient of derived `name` with `other`: another derived parameter, or
        a sampled one of `cross`."""
        j, N = self._j(name), self._need()
        if other in self.names:
            k = self._j(other)
            return float(self.cov()[j, k] / np.sqrt(self.var(name) * self.var(other)))
        c = self._c(other)
        var_b = self.V[c] / N - (self.X[c] / N) ** 2
        return float(self.cross_cov(name, other) / np.sqrt(self.var(name) * var_b))

    def summary(self):
        """One line for the log at the end of a run."""
        if self.n_used <= 0:
            return "Derived: no walker with finite derived values (%d looked at)." % self.n_samples
        parts = ", ".join("%s = %.5g +- %.2g" % (n, self.mean(n), self.std(n)) for n in self.names)
        n_bad = int(self.bad.sum())
        return ("Derived: %s (%d of %d walkers used%s)." % (
            parts, self.n_used, self.n_samples, "; %d non-finite values" % n_bad if n_bad else ""))

    # -- arithmetic, files
    def _layout(self):
        return (tuple(self.names), tuple(self.cross), self.shift.tobytes(), self.xshift.tobytes())

    def merge(self, other):
        """The walkers of two shards of one run (the shifts are equal by construction): float64 on
        the host."""
        if not isinstance(other, Derived) or self._layout() != other._layout():
            raise DerivedError("derived_stats: only shards of one run (names, cross parameters and shifts) merge")
        return Derived(self.names, self.cross, self.shift, self.xshift, self.n_samples + other.n_samples,
                       self.n_used + other.n_used, self.A + other.A, self.B + other.B, self.C + other.C,
                       self.X + other.X, self.V + other.V, self.bad + other.bad,
                       np.fmin(self.vmin, other.vmin), np.fmax(self.vmax, other.vmax))

    def __eq__(self, other):
        return (isinstance(other, Derived) and self._layout() == other._layout()
                and (self.n_samples, self.n_used) == (other.n_samples, other.n_used)
                and all(np.array_equal(getattr(self, k), getattr(other, k), equal_nan=True)
                        for k in ("A", "B", "C", "X", "V", "vmin", "vmax"))
                and np.array_equal(self.bad, other.bad))

    __hash__ = None

    def save(self, path):
        extra = {}
        if self.n_used > 0:   # (for a reader without this class)
            extra = {"mean": np.array([self.mean(n) for n in self.names]), "cov": self.cov()}
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, names=np.array(self.names, dtype=str), cross=np.array(self.cross, dtype=str),
                     shift=self.shift, xshift=self.xshift,
                     n=np.array([self.n_samples, self.n_used], dtype=np.int64), A=self.A, B=self.B, C=self.C,
                     X=self.X, V=self.V, bad=self.bad, min=self.vmin, max=self.vmax, **extra)

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        return cls([str(n) for n in z["names"]], [str(n) for n in z["cross"]], z["shift"], z["xshift"],
                   int(z["n"][0]), int(z["n"][1]), z["A"], z["B"], z["C"], z["X"], z["V"], z["bad"], z["min"],
                   z["max"])


# ---------------------------------------------------------------------------------- the option
def parse_option(opt, sampled):
    """The sampler option `derived_stats` -> False (no moment kernel; rows and marginals still get
    their values) or {"cross": [names of sampled parameters]}.  None = {"cross": "all"}.  Refuses, by
    the option's name, unknown keys and names."""
    if opt is False:
        return False
    sampled = list(sampled)
    opt = option_dict(True if opt is None else opt, "derived_stats", OPTION_KEYS, DerivedError, {"cross": "all"},
                      expected="None, False or a dict")
    cross = opt.get("cross", "all")
    if isinstance(cross, str):
        if cross != "all":
            raise DerivedError(f"derived_stats: cross must be a list of names, 'all' or None, got {cross!r}")
        cross = sampled
    cross = [str(n) for n in (cross or [])]
    bad = sorted({n for n in cross if n not in sampled})
    if bad:
        raise DerivedError(f"derived_stats: cross names unknown parameter(s) {bad}; the sampled "
                           f"parameters are {sampled}")
    if len(set(cross)) != len(cross):
        raise DerivedError("derived_stats: cross lists a parameter twice")
    return {"cross": cross}


def check_values(what, val, n, like):
    """What a batched device function returned: a torch.float64 tensor of shape (n,) on the device of
    `like`; else an EngineError (ERR_CALLBACK) that begins with `what`."""
    import torch
    if not isinstance(val, torch.Tensor):
        raise EngineError(ERR_CALLBACK, f"{what}: its function must return a "
                             f"torch.Tensor, got {type(val).__name__}")
    if tuple(val.shape) != (n,):
        raise EngineError(ERR_CALLBACK, f"{what}: its function must return shape "
                             f"({n},), got shape {tuple(val.shape)}")
    if val.dtype != torch.float64:
        raise EngineError(ERR_CALLBACK, f"{what}: its function must return dtype "
                             f"torch.float64, got dtype {val.dtype}")
    if val.device != like.device:
        raise EngineError(ERR_CALLBACK, f"{what}: its function must return a tensor "
                             f"on device {like.device}, got device {val.device}")


# ---------------------------------------------------------------------------------- the sampler's side
ENGINE_METHODS = ("configure_derived", "derived_row_views", "derived_get_values", "accumulate_derived",
                  "request_derived", "fetch_derived", "derived_set")


class DerivedAccumulator(DeviceProduct):
    """What the sampler holds of the derived parameters while it runs: a device product whose
    unfinished interval is never split (the peek reads out and sets back).  It exists whenever the
    model has function-derived parameters, whatever `derived_stats` says (False: the functions are
    still evaluated, for the stored rows and the marginals; nothing is summed: `live` is False).
    `current`: the rows of z hold the values of the state as it is; the sampler calls `stale()`
    whenever the walkers have moved."""

    name, option = "derived", "derived_stats"

    def __init__(self, cfg, spec, host):
        super().__init__(cfg, spec, host)
        self.funcs = list(spec.derived_functions)
        self.names = [f.name for f in self.funcs]
        self.stats = self.live = self.reports = cfg is not False
        self.cross = list(cfg["cross"]) if self.stats else []
        self.shift, self.current = None, False

    @classmethod
    def from_option(cls, opt, spec, engine_factory, host):
        if not getattr(spec, "derived_functions", None):
            return None
        try:
            cfg = parse_option(opt, spec.sampled)
        except DerivedError as e:
            host.fail("%s", str(e), cause=e)
        names = [f.name for f in spec.derived_functions]
        if getattr(host, "emit", "snapshots") != "snapshots":
            host.fail("derived functions %s: emit: %s is not served (use emit: snapshots)", names, host.emit)
        if host.temperature != 1:
            host.fail("derived_stats: the sums weigh the walkers as they are, which at temperature %g follow "
                      "the tempered law, not the posterior; use temperature: 1", host.temperature)
        if not all(hasattr(engine_factory, m) for m in ENGINE_METHODS):
            host.fail("derived functions %s: this engine keeps no derived rows (its library predates "
                      "mcmc_hip_derived_*)", names)
        return cls(cfg, spec, host)

    # -- evaluation
    def evaluate(self, force=False):
        """Fill the rows of z from the state as it lies on the device: the functions in `params`
        order, under the engine's stream.  Nothing synchronises with the host."""
        eng = self.engine
        if self.current and not force:
            return
        import torch
        xrows, zrows, stream = eng.derived_row_views()
        rows = dict(zip(self.spec.sampled, xrows))
        n = len(xrows[0])
        with torch.cuda.stream(stream):
            for f, out in zip(self.funcs, zrows):
                try:
                    val = f.function(*[rows[a] for a in f.args])
                except Exception as e:
                    raise EngineError(ERR_CALLBACK, f"derived parameter '{f.name}': its function raised "
                                         f"{type(e).__name__}: {e}") from e
                check_values(f"derived parameter '{f.name}'", val, n, out)
                if val.data_ptr() != out.data_ptr():
                    out.copy_(val)
                rows[f.name] = out
        self.current = True

    def stale(self):
        """The walkers have moved: z no longer holds the values of the state."""
        self.current = False

    def values(self):
        """The derived columns [W][m] of the state as it is now (evaluated first if z is stale)."""
        self.evaluate()
        return self.engine.derived_get_values()

    # -- the device product
    def attach(self, engine, resumed=False, centre=None, covmat=None):
        """Configure z and the accumulators.  A fresh run conditions the sums on the mean of the
        finite derived values of the initial ensemble (all-reduced over the processes); a resumed
        run takes the shift of the state file: `load` configures the engine."""
        self.engine = engine
        self.xshift = None if centre is None else np.array(centre, dtype=np.float64)
        if resumed:
            return
        m = len(self.names)
        self._configure(np.zeros(m))
        try:
            z = self.values()
        except EngineError as e:
            self.host.fail("%s", str(e), cause=e)
        fin = np.isfinite(z)
        tot = np.concatenate((np.where(fin, z, 0.0).sum(0), fin.sum(0).astype(np.float64)))
        self.host.all_reduce_sum(tot)
        shift = np.where(tot[m:] > 0, tot[:m] / np.maximum(tot[m:], 1.0), 0.0)
        self._configure(np.where(np.isfinite(shift), shift, 0.0))

    def _configure(self, shift):
        self.shift = np.array(shift, dtype=np.float64)
        ix = self.spec.sampled.index
        try:
            self.engine.configure_derived(len(self.names), [ix(n) for n in self.cross], self.shift)
        except EngineError as e:
            self.host.fail("derived functions %s: %s", self.names, str(e), cause=e)
        self.current = False

    def accumulate(self):
        self.evaluate()
        if self.stats:
            self.engine.accumulate_derived()

    def _xshift(self):
        ix = self.spec.sampled.index
        full = np.zeros(self.spec.d) if self.xshift is None else self.xshift
        return np.array([full[ix(n)] for n in self.cross], dtype=np.float64)

    def product(self, intervals, combined=False, pending=False):
        """The intervals of the window, in their order, plus the unfinished interval."""
        host, m, nc = self.host, len(self.names), len(self.cross)
        total = zero_part(m, nc)
        for p in self._parts(pending):
            total = add_parts(total, p)
        out = Derived(self.names, self.cross, self.shift, self._xshift(), total["n"] * int(host.n_walkers),
                      total["N"], total["A"], total["B"], total["C"], total["X"], total["V"], total["bad"],
                      total["min"], total["max"])
        if combined and host.size > 1:
            # ONE host all-reduce of the sums; the extrema travel as a row per process
            flat = np.concatenate(([float(out.n_samples), float(out.n_used)], out.A, out.B.ravel(), out.C.ravel(),
                                   out.X, out.V, out.bad.astype(np.float64)))
            ext = np.zeros((int(host.size), 2 * m))
            ext[host.rank] = np.concatenate((np.nan_to_num(out.vmin, nan=np.inf), np.nan_to_num(out.vmax, nan=-np.inf)))
            buf = np.concatenate((flat, ext.ravel()))
            res = host.all_reduce_sum(buf)
            buf = buf if res is None else np.asarray(res)
            flat, ext = buf[:len(flat)], buf[len(flat):].reshape(ext.shape)
            o = 2
            A, o = flat[o:o + m], o + m
            B, o = flat[o:o + m * m].reshape(m, m), o + m * m
            Cc, o = flat[o:o + m * nc].reshape(m, nc), o + m * nc
            X, o = flat[o:o + nc], o + nc
            V, o = flat[o:o + nc], o + nc
            bad = flat[o:o + m].astype(np.uint64)
            vmin, vmax = ext[:, :m].min(0), ext[:, m:].max(0)
            out = Derived(self.names, self.cross, self.shift, out.xshift, int(flat[0]), int(flat[1]), A, B, Cc, X,
                          V, bad, np.where(np.isfinite(vmin), vmin, np.nan), np.where(np.isfinite(vmax), vmax, np.nan))
        return out

    # -- the state file
    @staticmethod
    def _stack(parts, m, nc):
        n = len(parts)
        return {"N": np.array([[p["N"], p["n"]] for p in parts], dtype=np.int64).reshape(n, 2),
                "A": np.array([p["A"] for p in parts], dtype=np.float64).reshape(n, m),
                "B": np.array([p["B"] for p in parts], dtype=np.float64).reshape(n, m * (m + 1) // 2),
                "C": np.array([p["C"] for p in parts], dtype=np.float64).reshape(n, m, nc),
                "X": np.array([p["X"] for p in parts], dtype=np.float64).reshape(n, nc),
                "V": np.array([p["V"] for p in parts], dtype=np.float64).reshape(n, nc),
                "bad": np.array([p["bad"] for p in parts], dtype=np.uint64).reshape(n, m),
                "min": np.array([p["min"] for p in parts], dtype=np.float64).reshape(n, m),
                "max": np.array([p["max"] for p in parts], dtype=np.float64).reshape(n, m)}

    @staticmethod
    def _unstack(z, prefix):
        keys = ("A", "B", "C", "X", "V", "bad", "min", "max")
        return [dict({k: np.array(z[prefix + k][i]) for k in keys}, N=int(z[prefix + "N"][i][0]),
                     n=int(z[prefix + "N"][i][1])) for i in range(len(z[prefix + "N"]))]

    def save(self, pending):
        """What a resumed run must repeat (names, cross parameters) and what it goes on from: the
        shift, the intervals of the window and the open sums."""
        m, nc = len(self.names), len(self.cross)
        out = {"dv_names": np.array(self.names, dtype=str), "dv_cross": np.array(self.cross, dtype=str),
               "dv_stats": np.int64(self.stats), "dv_shift": self.shift, "dv_xshift": self._xshift()}
        if self.stats:
            o = self._peek(pending)
            out.update({"dv_iv_" + k: v for k, v in self._stack(self.ivs, m, nc).items()})
            out.update({"dv_open_" + k: v for k, v in self._stack([o], m, nc).items()})
        return out

    def load(self, z, n_intervals):
        """Resume: names and cross parameters must be the ones the sums were formed with; the
        shift, the window's intervals and the unfinished one come back."""
        fail = self.host.fail
        if "dv_names" not in z:
            fail("derived functions %s: cannot resume -- the run was written without them (their "
                 "columns and the window of their sums cannot begin in mid-run)", self.names)
        saved = ([str(n) for n in z["dv_names"]], [str(n) for n in z["dv_cross"]], bool(z["dv_stats"]))
        if saved != (self.names, self.cross, self.stats):
            fail("derived_stats: cannot resume -- the run was written with derived parameters %r, cross "
                 "%r and statistics %s, and now has %r, %r and %s", *saved, self.names, self.cross, self.stats)
        self._configure(z["dv_shift"])
        if self.xshift is None and len(self.cross):
            full = np.zeros(self.spec.d)
            full[[self.spec.sampled.index(n) for n in self.cross]] = z["dv_xshift"]
            self.xshift = full
        if not self.stats:
            return
        self.ivs = self._unstack(z, "dv_iv_")
        if len(self.ivs) != n_intervals:
            fail("derived_stats: the state file holds %d interval sums for %d intervals", len(self.ivs), n_intervals)
        self.open = self._unstack(z, "dv_open_")[0]
        try:
            self.engine.derived_set(self.open)
        except EngineError as e:
            fail("derived_stats: %s", str(e), cause=e)

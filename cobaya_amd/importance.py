"""Importance reweighting of the ensemble (Cobaya's `post`, for the moments): the product (`Importance`),
the sampler option behind it (`parse_option`) and what the sampler holds of it while it runs
(`ImportanceAccumulator`, a device product with the methods `marginals.MarginalsAccumulator` states).

An alternative posterior is given by its log-weight: a batched device function of the sampled parameters
(the forms and checks of `model.DerivedFunction`), bound BY NAME to 1-D torch.float64 views of the rows of
the state x[d][W] under the engine's stream, which returns delta[W] = ln(new posterior density / sampled
posterior density) up to a constant.  It must be elementwise in the walker.  The sums come from the
engine (mcmc_hip_importance_*; importance_kernels.hip), which looks at every walker of every moment
snapshot.  The rule ("Importance"): per alternative and checkpoint interval, with c
the exact maximum of the finite delta of the interval's first accumulation (0.0: none) and s the moment
shift, a walker with delta NaN or +inf is left out (`nonfinite`), one with -inf is used with e = 0
(`zero`), every other has e = dexp(min(delta - c, 700)) (`clamped` counts delta - c > 700), and each group
of group_size walkers adds, over its used walkers in ascending order, one chain each from +0.0 with the
product and the addition as separate roundings,

    n,   S1 = sum e,   S2 = sum e * e,   M_i = sum u_i,   V_i = sum u_i * b_i,   Q_ij = sum u_i * b_j (j < i)

with b_i = x_i - s_i and u_i = e * b_i; the chain of an accumulation is then added to the interval's
value.  On the host, C = the largest c of the window; every interval's sums are scaled by exp(c - C) in
float64 (S2, a sum of squares, by its square) and added in interval order, and

    log_ratio = C + ln(S1 / n),   ess = S1^2 / S2,   mean = s + M / S1,   cov = Q / S1 - (M / S1)(M / S1)^T;

the standard errors are delete-one-group jackknives (groups are independent chains, so they absorb the
correlation between snapshots).

An alternative with `"marginals": True` also keeps a weighted copy of the run's `marginals` histograms
("Importance marginals"; importance_hist_kernels.hip): a used walker adds the
fixed-point weight q = floor(min(e, 2^16) * 2^32) where the unweighted histogram adds 1, into 128-bit
counters kept as words (lo, hi), with the intervals and the c of the sums.  On the host a counter is worth
(hi 2^64 + lo) 2^-32; the intervals are scaled by exp(c - C) and added in interval order, like S1.
`Importance.marginals(name)` gives them as a `marginals.WeightedMarginals`.

Out of scope: derived or bestfit products under the new weights, function-derived names as arguments,
per-alternative bins or ranges, `temperature != 1`, and writing reweighted chains.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .derived import check_values
from .engine import ERR_CALLBACK, EngineError
from .marginals import MAX_SLAB_BYTES, WeightedMarginals, slab_size
from .model import UnsupportedModel, parse_derived_function
from .product import DeviceProduct, known_keys

MAX_ALT = 8                 # importance_args.h: kImMaxAlt
MAX_DIM = 256               # importance_args.h: kImMaxDim
MAX_COV_DIM = 128           # importance_args.h: kImMaxCovDim
CLAMP = 700.0               # importance_args.h: kImClamp
OPTION_KEYS = ("function", "cov", "marginals")
LOW_ESS = 0.05              # an ESS fraction below this is warned about
HIST_CAP = 65536.0          # importance_hist_args.h: kImHistCap, the largest e a histogram takes in
HIST_METHODS = ("configure_importance_hist", "importance_hist_layout", "fetch_importance_hist",
                "importance_hist_set")
MARG_KEYS = ("params", "pairs", "bins", "bins2d", "ranges")


class ImportanceError(ValueError):
    """An `importance` option (or a pair of products) that cannot be served; the message begins with
    the option's name."""


def n_chains(d, cov):
    """Chains of one (alternative, group): S1 | S2 | M[d] | V[d] | with `cov` Q[d (d - 1) / 2], (i, j < i)
    at i (i - 1) / 2 + j."""
    return 2 + 2 * d + (d * (d - 1) // 2 if cov else 0)


def scaled(S, f):
    """The chains [G, n_chains] of weights e -> those of weights f e: S2, the sum of squares, takes f * f."""
    with np.errstate(invalid="ignore", over="ignore"):
        out = f * S
        out[:, 1] = (f * f) * S[:, 1]
    return out


def hist_value(lo, hi):
    """The 128-bit fixed-point counters (words lo, hi) as float64 weights: (hi 2^64 + lo) 2^-32."""
    return (np.asarray(hi, np.uint64).astype(np.float64) * 2.0 ** 64
            + np.asarray(lo, np.uint64).astype(np.float64)) * 2.0 ** -32


def split_sums(flat, d, cov, G):
    """The flat sums of a read-out -> one [G, n_chains] array per alternative."""
    out, at = [], 0
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    for cv in cov:
        k = G * n_chains(d, cv)
        out.append(flat[at:at + k].reshape(G, n_chains(d, cv)))
        at += k
    if at != len(flat):
        raise ImportanceError(f"importance: {len(flat)} sums do not fit {len(cov)} alternatives of {G} groups "
                              f"at d = {d}")
    return out


# ---------------------------------------------------------------------------------- the product
class Importance:
    """Weighted moments of the sampled parameters, the effective sample size and the ratio of evidences,
    per alternative.

    `names`: the alternatives; `params`: the sampled parameters; `shift` [d]: what the sums are taken
    about; `cov` [n_alt]: whether Q is kept; `n_walkers`: the walkers of the G groups held; `n_acc`:
    accumulations of the window; `C` [n_alt]: the centring constant the sums are scaled to; `sums`: per
    alternative float64 [G, n_chains], the window's total per group; `n` uint64 [n_alt, G]: the used
    walkers; `n_zero`, `n_nonfinite`, `n_clamped` int64 [n_alt].  `hist` (None: no alternative keeps
    reweighted marginals): {"layout": the `params`, `pairs`, `bins`, `bins2d`, `ranges` of the run's
    marginals, "weights": per alternative None or float64 [n_counters] in units of exp(C), "saturated"
    [n_alt]}."""

    reports = True

    def __init__(self, names, params, shift, cov, n_walkers, n_acc, C, sums, n, n_zero, n_nonfinite, n_clamped,
                 hist=None):
        self.names, self.params = [str(v) for v in names], [str(v) for v in params]
        na, d = len(self.names), len(self.params)
        self.marg, self.hist, self.n_saturated = None, [None] * na, np.zeros(na, np.int64)
        if hist is not None and any(w is not None for w in hist["weights"]):
            lay = hist["layout"]
            self.marg = {"params": [str(v) for v in lay["params"]], "pairs": [(str(a), str(b)) for a, b in lay["pairs"]],
                         "bins": int(lay["bins"]), "bins2d": int(lay["bins2d"]),
                         "ranges": {str(k): (float(v[0]), float(v[1])) for k, v in lay["ranges"].items()}}
            nc = slab_size(len(self.marg["params"]), self.marg["bins"], len(self.marg["pairs"]), self.marg["bins2d"])
            if len(hist["weights"]) != na:
                raise ImportanceError(f"importance: {len(hist['weights'])} sets of histograms for {na} alternatives")
            try:
                self.hist = [None if w is None else np.array(w, dtype=np.float64).reshape(nc) for w in hist["weights"]]
                self.n_saturated = np.array(hist["saturated"], dtype=np.int64).reshape(na)
            except ValueError as e:
                raise ImportanceError(f"importance: the reweighted histograms do not fit their layout of {nc} "
                                      f"counters ({e})") from None
        self.d, self.n_walkers, self.n_acc = d, int(n_walkers), int(n_acc)
        try:
            self.shift = np.array(shift, dtype=np.float64).reshape(d)
            self.cov_kept = [bool(c) for c in np.asarray(cov).reshape(na)]
            self.C = np.array(C, dtype=np.float64).reshape(na)
            self.n = np.array(n, dtype=np.uint64).reshape(na, -1)
            G = self.n.shape[1]
            self.sums = [np.array(s, dtype=np.float64).reshape(G, n_chains(d, c)) for s, c in zip(sums, self.cov_kept)]
            if len(self.sums) != na:
                raise ValueError(f"{len(self.sums)} arrays of sums")
            self.n_zero = np.array(n_zero, dtype=np.int64).reshape(na)
            self.n_nonfinite = np.array(n_nonfinite, dtype=np.int64).reshape(na)
            self.n_clamped = np.array(n_clamped, dtype=np.int64).reshape(na)
        except ValueError as e:
            raise ImportanceError(f"importance: the arrays of {na} alternatives and {d} parameters do not fit "
                                  f"together ({e})") from None

    @classmethod
    def from_parts(cls, names, params, shift, cov, n_walkers, parts, n_groups=None, marg=None):
        """From the read-outs of the window's intervals, in their order: dicts {"sums" (flat), "n"
        [n_alt, G], "counters" [n_alt, 3], "c" [n_alt], "n_acc"}.  Intervals without an accumulation
        are skipped.  `marg` (with reweighted marginals): the layout of the run's marginals plus "on"
        [n_alt]; every part then has "hist": {"lo", "hi" [n_hist, n_counters], "saturated" [n_hist]}."""
        na, d = len(names), len(params)
        parts = [p for p in parts if int(p["n_acc"]) > 0]
        G = int(np.asarray(parts[0]["n"]).reshape(na, -1).shape[1]) if parts else int(n_groups or 0)
        c = np.array([np.asarray(p["c"], np.float64).reshape(na) for p in parts]).reshape(len(parts), na)
        C = c.max(axis=0) if len(parts) else np.zeros(na)
        sums = [np.zeros((G, n_chains(d, cv))) for cv in cov]
        n, cnt = np.zeros((na, G), np.uint64), np.zeros((na, 3), np.int64)
        on = [k for k in range(na) if marg is not None and marg["on"][k]]
        weights, sat = [None] * na, np.zeros(na, np.int64)
        if on:
            nc = slab_size(len(marg["params"]), marg["bins"], len(marg["pairs"]), marg["bins2d"])
            for k in on:
                weights[k] = np.zeros(nc)
        for p, ci in zip(parts, c):
            for h, k in enumerate(on):     # (the scaling of S1: to the common C, in interval order)
                v = hist_value(np.asarray(p["hist"]["lo"]).reshape(len(on), -1)[h],
                               np.asarray(p["hist"]["hi"]).reshape(len(on), -1)[h])
                weights[k] = weights[k] + math.exp(ci[k] - C[k]) * v
                sat[k] += int(np.asarray(p["hist"]["saturated"]).reshape(-1)[h])
            split = split_sums(p["sums"], d, cov, G)
            for k in range(na):
                with np.errstate(invalid="ignore", over="ignore"):
                    sums[k] = sums[k] + scaled(split[k], math.exp(ci[k] - C[k]))
            n = n + np.asarray(p["n"], np.uint64).reshape(na, G)
            cnt = cnt + np.asarray(p["counters"]).reshape(na, 3).astype(np.int64)
        return cls(names, params, shift, cov, n_walkers, sum(int(p["n_acc"]) for p in parts), C, sums, n,
                   cnt[:, 0], cnt[:, 1], cnt[:, 2],
                   {"layout": marg, "weights": weights, "saturated": sat} if on else None)

    # -- look-ups
    def _k(self, name):
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"no alternative {name!r} (have {self.names})") from None

    @property
    def n_groups(self):
        return self.n.shape[1]

    @property
    def n_samples(self):
        """Walkers looked at: accumulations x walkers."""
        return self.n_acc * self.n_walkers

    def n_used(self, name):
        """Walkers whose log-weight was finite or -inf."""
        return int(self.n[self._k(name)].sum())

    def zero(self, name):
        """Walkers used with weight 0 (log-weight -inf)."""
        return int(self.n_zero[self._k(name)])

    def nonfinite(self, name):
        """Walkers left out (log-weight NaN or +inf)."""
        return int(self.n_nonfinite[self._k(name)])

    def clamped(self, name):
        """Walkers whose log-weight lay more than 700 above its interval's c."""
        return int(self.n_clamped[self._k(name)])

    def saturated(self, name):
        """Used walkers whose weight lay above 2^16 times the largest their interval opened with: they
        entered the reweighted histograms as 2^16 (0 for an alternative without histograms)."""
        return int(self.n_saturated[self._k(name)])

    def marginals(self, name):
        """The run's marginal histograms under the weights of `name`: a `WeightedMarginals`."""
        k = self._k(name)
        if self.hist[k] is None:
            raise ImportanceError(f"importance: alternative {name!r} keeps no reweighted marginals (give it "
                                  "'marginals': True beside the sampler option `marginals`)")
        m = self.marg
        return WeightedMarginals(m["params"], m["pairs"], m["bins"], m["bins2d"], m["ranges"], self.hist[k],
                                 self.n_acc, self.n_samples, self.saturated(name), self.C[k])

    # -- the estimates
    def _tot(self, k):
        """(n [G], S [G, n_chains], their totals) of alternative k."""
        n, S = self.n[k].astype(np.float64), self.sums[k]
        return n, S, n.sum(), S.sum(axis=0)

    def log_ratio(self, name):
        """ln(Z_new / Z_sampled) = C + ln(S1 / n) (NaN: nothing used; -inf: every weight is zero)."""
        k = self._k(name)
        _, _, nt, St = self._tot(k)
        if nt <= 0:
            return float("nan")
        return float(self.C[k] + math.log(St[0] / nt)) if St[0] > 0 else (-math.inf if St[0] == 0 else float("nan"))

    def log_ratio_stderr(self, name):
        """The delete-one-group jackknife error of `log_ratio` (NaN: fewer than two groups, or a group
        that holds all the weight)."""
        k = self._k(name)
        n, S, nt, St = self._tot(k)
        G = len(n)
        if G < 2 or nt <= 0:
            return float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            loo = np.log((St[0] - S[:, 0]) / (nt - n))
        if not np.all(np.isfinite(loo)):
            return float("nan")
        return float(math.sqrt((G - 1.0) / G * float(np.sum((loo - loo.mean()) ** 2))))

    def ess(self, name):
        """The effective sample size (sum w)^2 / sum w^2 (0.0: every weight is zero)."""
        _, _, _, St = self._tot(self._k(name))
        with np.errstate(all="ignore"):
            return float(St[0] / St[1] * St[0]) if St[1] > 0 else 0.0

    def ess_fraction(self, name):
        n = self.n_used(name)
        return self.ess(name) / n if n else float("nan")

    def _moments(self, k):
        """(M / S1 [d], V / S1 [d]) of alternative k (NaN: every weight is zero)."""
        d = self.d
        _, _, _, St = self._tot(k)
        with np.errstate(all="ignore"):
            return St[2:2 + d] / St[0], St[2 + d:2 + 2 * d] / St[0]

    def mean(self, name):
        """float64 [d]: the weighted means of the sampled parameters."""
        return self.shift + self._moments(self._k(name))[0]

    def mean_stderr(self, name):
        """float64 [d]: the delete-one-group jackknife errors of the means."""
        k, d = self._k(name), self.d
        n, S, _, St = self._tot(k)
        G = len(n)
        if G < 2:
            return np.full(d, np.nan)
        with np.errstate(all="ignore"):
            loo = (St[2:2 + d] - S[:, 2:2 + d]) / (St[0] - S[:, 0])[:, None]
            return np.sqrt((G - 1.0) / G * np.sum((loo - loo.mean(axis=0)) ** 2, axis=0))

    def var(self, name):
        m, v = self._moments(self._k(name))
        return v - m * m

    def std(self, name):
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.maximum(self.var(name), 0.0))

    def cov(self, name):
        """float64 [d, d]: the weighted covariance (ddof = 0, like SampleCollection.cov)."""
        k, d = self._k(name), self.d
        if not self.cov_kept[k]:
            raise ImportanceError(f"importance: alternative {name!r} keeps no covariance (cov: False); var() and "
                                  "std() are kept")
        _, _, _, St = self._tot(k)
        full = np.zeros((d, d))
        i, j = np.tril_indices(d, -1)
        full[i, j] = full[j, i] = St[2 + 2 * d:]
        full[np.arange(d), np.arange(d)] = St[2 + d:2 + 2 * d]
        m = self._moments(k)[0]
        with np.errstate(all="ignore"):
            return full / St[0] - np.outer(m, m)

    def warnings(self, name):
        """What the run's last log lines warn about: a low ESS fraction, clamped weights, weights that
        saturated the reweighted histograms."""
        out, f = [], self.ess_fraction(name)
        if self.n_used(name) and f < LOW_ESS:
            out.append("ESS fraction %.3g is below %g: the sampled posterior barely covers this one" % (f, LOW_ESS))
        if self.clamped(name):
            out.append("%d weights were clamped at exp(%g) above their interval's largest" % (self.clamped(name), CLAMP))
        if self.saturated(name):
            out.append("%d weights entered the reweighted marginals saturated at %g times their interval's largest"
                       % (self.saturated(name), HIST_CAP))
        return out

    def lines(self):
        """One line per alternative for the log at the end of a run: (text, warns)."""
        out = []
        for name in self.names:
            if not self.n_used(name):
                out.append(("Importance %s: no walker with a usable log-weight (%d looked at)."
                            % (name, self.n_samples), True))
                continue
            w = self.warnings(name)
            out.append(("Importance %s: ESS fraction %.3g, ln(Z_new / Z) = %.5g +- %.2g (%d of %d walkers used%s)%s"
                        % (name, self.ess_fraction(name), self.log_ratio(name), self.log_ratio_stderr(name),
                           self.n_used(name), self.n_samples,
                           "; %d with weight zero" % self.zero(name) if self.zero(name) else "",
                           ". WARNING: " + "; ".join(w) + "." if w else "."), bool(w)))
        return out

    def summary(self):
        return "\n".join(t for t, _ in self.lines())

    def report(self, log):
        """One log line per alternative; a warning where the ESS fraction is low or weights were clamped."""
        for text, warns in self.lines():
            (log.warning if warns else log.info)("%s", text)

    # -- arithmetic, files
    def _layout(self):
        base = (tuple(self.names), tuple(self.params), self.shift.tobytes(), tuple(self.cov_kept), self.n_acc)
        if self.marg is None:
            return base
        m = self.marg
        return base + (tuple(w is not None for w in self.hist), tuple(m["params"]), tuple(m["pairs"]), m["bins"],
                       m["bins2d"], tuple(sorted(m["ranges"].items())))

    def _hist(self, weights=None, saturated=None):
        """The constructor's `hist` (None: no histograms)."""
        if self.marg is None:
            return None
        return {"layout": self.marg, "weights": self.hist if weights is None else weights,
                "saturated": self.n_saturated if saturated is None else saturated}

    def hist_scaled_to(self, C):
        """The reweighted histograms per alternative (None: none), scaled from self.C to C >= self.C."""
        return [None if w is None else math.exp(self.C[k] - C[k]) * w for k, w in enumerate(self.hist)]

    def scaled_to(self, C):
        """The sums per alternative, scaled from self.C to the centring constants C >= self.C."""
        return [scaled(s, math.exp(self.C[k] - C[k])) for k, s in enumerate(self.sums)]

    def merge(self, other):
        """The groups of two shards of one run, side by side, scaled to their common C."""
        if not isinstance(other, Importance) or self._layout() != other._layout():
            raise ImportanceError("importance: only shards of one run (alternatives, parameters, shift and "
                                  "accumulations) merge")
        C = np.maximum(self.C, other.C)
        sums = [np.concatenate((a, b), axis=0) for a, b in zip(self.scaled_to(C), other.scaled_to(C))]
        return Importance(self.names, self.params, self.shift, self.cov_kept, self.n_walkers + other.n_walkers,
                          self.n_acc, C, sums, np.concatenate((self.n, other.n), axis=1),
                          self.n_zero + other.n_zero, self.n_nonfinite + other.n_nonfinite,
                          self.n_clamped + other.n_clamped,
                          self._hist([None if a is None else a + b
                                      for a, b in zip(self.hist_scaled_to(C), other.hist_scaled_to(C))],
                                     self.n_saturated + other.n_saturated))

    def __eq__(self, other):
        return (isinstance(other, Importance) and self._layout() == other._layout()
                and self.n_walkers == other.n_walkers and np.array_equal(self.C, other.C)
                and np.array_equal(self.n, other.n)
                and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(self.sums, other.sums))
                and all(np.array_equal(getattr(self, k), getattr(other, k))
                        for k in ("n_zero", "n_nonfinite", "n_clamped", "n_saturated"))
                and all((a is None) == (b is None) and (a is None or np.array_equal(a, b, equal_nan=True))
                        for a, b in zip(self.hist, other.hist)))

    __hash__ = None

    def save(self, path):
        extra = {"sums_%d" % k: s for k, s in enumerate(self.sums)}
        with np.errstate(all="ignore"):   # (for a reader without this class)
            extra.update(log_ratio=np.array([self.log_ratio(v) for v in self.names]),
                         log_ratio_stderr=np.array([self.log_ratio_stderr(v) for v in self.names]),
                         ess=np.array([self.ess(v) for v in self.names]),
                         mean=np.array([self.mean(v) for v in self.names]),
                         std=np.array([self.std(v) for v in self.names]))
        if self.marg is not None:      # (only then: a file without histograms is what it always was)
            m, names = self.marg, list(self.marg["ranges"])
            extra.update(hist_on=np.array([w is not None for w in self.hist], dtype=np.int64),
                         hist_weights=np.array([w for w in self.hist if w is not None], dtype=np.float64),
                         hist_saturated=self.n_saturated, marg_params=np.array(m["params"], dtype=str),
                         marg_pairs=np.array(m["pairs"], dtype=str).reshape(-1, 2),
                         marg_bins=np.array([m["bins"], m["bins2d"]], dtype=np.int64),
                         marg_range_names=np.array(names, dtype=str),
                         marg_ranges=np.array([m["ranges"][v] for v in names], dtype=np.float64).reshape(-1, 2))
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, names=np.array(self.names, dtype=str), params=np.array(self.params, dtype=str),
                     shift=self.shift, cov_kept=np.array(self.cov_kept, dtype=np.int64),
                     geometry=np.array([self.n_walkers, self.n_acc], dtype=np.int64), C=self.C, n=self.n,
                     counters=np.stack((self.n_zero, self.n_nonfinite, self.n_clamped), axis=1), **extra)

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        names = [str(v) for v in z["names"]]
        cnt = z["counters"].reshape(len(names), 3)
        hist = None
        if "hist_on" in z.files:
            rows = iter(z["hist_weights"])
            hist = {"layout": {"params": z["marg_params"], "pairs": z["marg_pairs"], "bins": z["marg_bins"][0],
                               "bins2d": z["marg_bins"][1],
                               "ranges": {str(v): r for v, r in zip(z["marg_range_names"], z["marg_ranges"])}},
                    "weights": [next(rows) if v else None for v in z["hist_on"]], "saturated": z["hist_saturated"]}
        return cls(names, [str(v) for v in z["params"]], z["shift"], z["cov_kept"], int(z["geometry"][0]),
                   int(z["geometry"][1]), z["C"], [z["sums_%d" % k] for k in range(len(names))], z["n"],
                   cnt[:, 0], cnt[:, 1], cnt[:, 2], hist)


# ---------------------------------------------------------------------------------- the option
def parse_option(opt, sampled, derived=()):
    """The sampler option `importance` -> None (off) or a list of {"name", "function" (a
    `model.DerivedFunction`: callable and argument names), "cov", "marginals" (whether the alternative
    keeps a weighted copy of the run's marginal histograms)}.  `sampled`: the sampled parameters
    the arguments are bound to by name; `derived`: the function-derived names, which are refused as
    arguments.  Refuses, by the option's name, anything else that cannot be served."""
    if opt is None or opt is False:
        return None
    sampled, d = list(sampled), len(sampled)
    if not isinstance(opt, dict) or not opt:
        raise ImportanceError(f"importance: expected None or a dict of 1..{MAX_ALT} named alternatives, got {opt!r}")
    if len(opt) > MAX_ALT:
        raise ImportanceError(f"importance: at most {MAX_ALT} alternatives are served, not {len(opt)}")
    out = []
    for name, alt in opt.items():
        what = f"importance: alternative {str(name)!r}"
        if not isinstance(alt, dict):
            raise ImportanceError(f"{what}: expected a dict with the key 'function' (and 'cov', 'marginals'), got {alt!r}")
        known_keys(alt, what, OPTION_KEYS, ImportanceError)
        if alt.get("function") is None:
            raise ImportanceError(f"{what}: no 'function' (the log-weight: a callable, a 'lambda ...' string or a "
                                  "'package.module:name' string)")
        try:
            fn = parse_derived_function(str(name), alt["function"])
        except UnsupportedModel as e:    # (the forms and checks of a derived function, under this option's name)
            raise ImportanceError(f"importance: {e}") from e
        if not fn.args:
            raise ImportanceError(f"{what}: its function takes no arguments; they are bound by name to the sampled "
                                  f"parameters {sampled}")
        for a in fn.args:
            if a in derived:
                raise ImportanceError(f"{what}: argument {a!r} is a function-derived parameter, which is out of "
                                      f"scope here; the arguments are sampled parameters ({sampled})")
            if a not in sampled:
                raise ImportanceError(f"{what}: argument {a!r} is not a sampled parameter; the sampled parameters "
                                      f"are {sampled}")
        cov = alt.get("cov")
        if cov is not None and not isinstance(cov, (bool, np.bool_)):
            raise ImportanceError(f"{what}: cov must be True, False or None, got {cov!r}")
        if cov and d > MAX_COV_DIM:
            raise ImportanceError(f"{what}: cov: True needs d <= {MAX_COV_DIM}, not d = {d} (means and variances "
                                  "are kept at any d)")
        marg = alt.get("marginals")
        if marg is not None and not isinstance(marg, (bool, np.bool_)):
            raise ImportanceError(f"{what}: marginals must be True, False or None, got {marg!r}")
        out.append({"name": str(name), "function": fn, "cov": bool(d <= MAX_COV_DIM if cov is None else cov),
                    "marginals": bool(marg)})
    return out


# ---------------------------------------------------------------------------------- the sampler's side
ENGINE_METHODS = ("configure_importance", "importance_layout", "importance_row_views", "accumulate_importance",
                  "request_importance", "fetch_importance", "importance_set")


class ImportanceAccumulator(DeviceProduct):
    """What the sampler holds of the sums while it runs: a device product whose unfinished interval
    is never split.  A part is the closing request's read-out: sums, counts and the c it was taken
    under; the peek is a request that does not close.  `eval_seconds`: host time spent in the
    log-weight functions (queueing their torch operations)."""

    name, closes, error, ENGINE_METHODS, MAX_DIM = "importance", True, ImportanceError, ENGINE_METHODS, MAX_DIM
    tempered = ("importance: the sums weigh the walkers as they are, which at temperature %g follow "
                "the tempered law, not the posterior; use temperature: 1 or turn importance off")
    predates = "importance: this engine keeps no importance sums (its library predates mcmc_hip_importance_*)"

    def __init__(self, cfg, spec, host):
        super().__init__(cfg, spec, host)
        self.names = [a["name"] for a in cfg]
        self.cov = [bool(a["cov"]) for a in cfg]
        self.want = [bool(a.get("marginals")) for a in cfg]      # reweighted marginals, per alternative
        self.marg = None                                         # the MarginalsAccumulator they follow
        self.shift, self.G, self.eval_seconds = None, 0, 0.0

    def pair_with(self, marginals, engine_factory):
        """The sampler hands over its `MarginalsAccumulator` (None: the option is off) once both are
        made, BEFORE the engine is created: an alternative that asks for marginals is refused by name
        without the sampler option, on an engine without the entry points, or above the slab allowed."""
        if not any(self.want):
            return
        first = self.names[self.want.index(True)]
        if marginals is None:
            self.host.fail("importance: alternative %r: marginals: True needs the sampler option `marginals` "
                           "(its parameters, pairs, bins and ranges are the ones reweighted)", first)
        if not all(hasattr(engine_factory, m) for m in HIST_METHODS):
            self.host.fail("importance: alternative %r: marginals: True: this engine keeps no reweighted marginal "
                           "histograms (its library predates mcmc_hip_importance_hist_*)", first)
        c = marginals.cfg
        nbytes = 16 * sum(self.want) * slab_size(len(c["params"]), c["bins"], len(c["pairs"]), c["bins2d"])
        if nbytes > MAX_SLAB_BYTES:
            self.host.fail("importance: marginals: True for %d alternatives takes %d bytes of 128-bit counters, "
                           "above the %d allowed: ask fewer alternatives for them, or fewer pairs or bins of "
                           "`marginals`", sum(self.want), nbytes, MAX_SLAB_BYTES)
        self.marg = marginals

    def _configure_hist(self):
        """Once the layout of the marginals is known to the engine (`attach` on a fresh run, `load` on a
        resume: `MarginalsAccumulator` comes first in either)."""
        try:
            self.engine.configure_importance_hist(self.want)
            lay = self.engine.importance_hist_layout()
        except EngineError as e:
            self.host.fail("importance: %s", str(e), cause=e)
        nc = int(self.marg.cfg["n_counters"])
        if ([bool(v) for v in lay["on"]], int(lay["n_counters"])) != (self.want, nc):
            self.host.fail("importance: the engine lays its reweighted histograms out differently (%r) from the "
                           "marginals (%d counters)", lay, nc)

    def _fetch(self):
        part = self.engine.fetch_importance()
        if self.marg is not None:      # (the same request copied out both slabs)
            part["hist"] = self.engine.fetch_importance_hist()
        return part

    def _marg_layout(self):
        if self.marg is None:
            return None
        c = self.marg.cfg
        return {"params": c["params"], "pairs": c["pairs"], "bins": c["bins"], "bins2d": c["bins2d"],
                "ranges": c["resolved"], "on": self.want}

    @staticmethod
    def parse(opt, spec):
        return parse_option(opt, spec.sampled, [f.name for f in getattr(spec, "derived_functions", None) or []])

    def attach(self, engine, resumed=False, centre=None, covmat=None):
        """Hand the alternatives to the engine.  The sums are taken about the moment shift (`centre`);
        a resumed run takes it from the state file: `load`."""
        self.engine = engine
        if centre is not None:
            self.shift = np.array(centre, dtype=np.float64)
        try:
            engine.configure_importance(self.cov)
            lay = engine.importance_layout()
        except EngineError as e:
            self.host.fail("importance: %s", str(e), cause=e)
        self.G = int(lay["n_groups"])
        want = sum(self.G * n_chains(self.spec.d, c) for c in self.cov)
        if (lay["n_alt"], [bool(c) for c in lay["cov"]], lay["n_sums"]) != (len(self.cov), self.cov, want):
            self.host.fail("importance: the engine lays its sums out differently (%r) from the product", lay)
        if self.marg is not None and not resumed:
            self._configure_hist()

    # -- evaluation
    def evaluate(self):
        """Fill the log-weights from the state as it lies on the device: the functions in the option's
        order, under the engine's stream.  Nothing synchronises with the host."""
        import torch
        t0 = time.perf_counter()
        xrows, delta, stream = self.engine.importance_row_views()
        rows = dict(zip(self.spec.sampled, xrows))
        n = len(xrows[0])
        with torch.cuda.stream(stream):
            for k, alt in enumerate(self.cfg):
                f, what = alt["function"], f"importance: alternative '{alt['name']}'"
                try:
                    val = f.function(*[rows[a] for a in f.args])
                except Exception as e:
                    raise EngineError(ERR_CALLBACK, f"{what}: its function raised {type(e).__name__}: {e}") from e
                check_values(what, val, n, delta)
                delta[k].copy_(val)
        self.eval_seconds += time.perf_counter() - t0
        return delta

    # -- the device product
    def accumulate(self):
        self.engine.accumulate_importance(self.evaluate())

    def product(self, intervals, combined=False, pending=False):
        """The intervals of the window, in their order, plus the unfinished interval."""
        host, parts = self.host, self._parts(pending)
        shift = np.zeros(self.spec.d) if self.shift is None else self.shift
        out = Importance.from_parts(self.names, self.spec.sampled, shift, self.cov, int(host.n_walkers), parts, self.G,
                                    self._marg_layout())
        if combined and host.size > 1:
            out = self._combined(out)
        return out

    def _reduced(self, buf):
        res = self.host.all_reduce_sum(buf)
        return buf if res is None else np.asarray(res).reshape(buf.shape)

    def _combined(self, own):
        """The groups of all processes side by side (every process has closed the same intervals):
        one host all-reduce for the common C, one of a zero matrix in which every process fills its own
        row with its sums scaled to it."""
        host, na, G = self.host, len(self.names), own.n_groups
        size, rank = int(host.size), int(host.rank)
        if np.any(own.n >= np.uint64(2 ** 53)):
            host.fail("importance: a count above 2^53 cannot be carried over processes exactly")
        head = np.zeros((size, na + 2))
        head[rank] = np.concatenate((own.C, [float(own.n_acc), float(G)]))
        head = self._reduced(head.reshape(-1)).reshape(size, na + 2)
        if not np.all(head[:, na:] == head[rank, na:]):
            host.fail("importance: the processes hold different windows (accumulations, groups: %r)",
                      head[:, na:].tolist())
        C = head[:, :na].max(axis=0)
        held = [w for w in own.hist_scaled_to(C) if w is not None]
        row = np.concatenate([s.reshape(-1) for s in own.scaled_to(C)]
                             + [own.n.astype(np.float64).reshape(-1), own.n_zero.astype(np.float64),
                                own.n_nonfinite.astype(np.float64), own.n_clamped.astype(np.float64)]
                             + held + ([own.n_saturated.astype(np.float64)] if held else []))
        buf = np.zeros((size, len(row)))
        buf[rank] = row
        buf = self._reduced(buf.reshape(-1)).reshape(size, len(row))
        n_sums = sum(s.size for s in own.sums)
        sums = [np.concatenate(s, axis=0) for s in zip(*(split_sums(b[:n_sums], own.d, self.cov, G) for b in buf))]
        n = np.concatenate([b[n_sums:n_sums + na * G].astype(np.uint64).reshape(na, G) for b in buf], axis=1)
        at = n_sums + na * G
        cnt = buf[:, at:at + 3 * na].sum(axis=0).astype(np.int64).reshape(3, na)
        hist = None
        if held:    # (the rows are added in rank order)
            tot, at = buf[:, at + 3 * na:].sum(axis=0), 0
            weights = [None] * na
            for k, w in enumerate(own.hist):
                if w is not None:
                    weights[k], at = tot[at:at + len(w)], at + len(w)
            hist = own._hist(weights, tot[at:].astype(np.int64))
        return Importance(self.names, own.params, own.shift, self.cov, own.n_walkers * size, own.n_acc, C, sums, n,
                          cnt[0], cnt[1], cnt[2], hist)

    # -- the state file
    def _stack(self, parts):
        k, na, G = len(parts), len(self.names), self.G
        n_sums = sum(G * n_chains(self.spec.d, c) for c in self.cov)
        out = {"sums": np.array([p["sums"] for p in parts], dtype=np.float64).reshape(k, n_sums),
               "n": np.array([p["n"] for p in parts], dtype=np.uint64).reshape(k, na, G),
               "counters": np.array([p["counters"] for p in parts], dtype=np.uint64).reshape(k, na, 3),
               "c": np.array([p["c"] for p in parts], dtype=np.float64).reshape(k, na),
               "nacc": np.array([p["n_acc"] for p in parts], dtype=np.int64).reshape(k)}
        if self.marg is not None:      # (written only when on)
            nh, nc = sum(self.want), int(self.marg.cfg["n_counters"])
            out.update(hlo=np.array([p["hist"]["lo"] for p in parts], dtype=np.uint64).reshape(k, nh, nc),
                       hhi=np.array([p["hist"]["hi"] for p in parts], dtype=np.uint64).reshape(k, nh, nc),
                       hsat=np.array([p["hist"]["saturated"] for p in parts], dtype=np.uint64).reshape(k, nh))
        return out

    @staticmethod
    def _unstack(z, prefix):
        out = [{"sums": np.array(z[prefix + "sums"][i]), "n": np.array(z[prefix + "n"][i]),
                "counters": np.array(z[prefix + "counters"][i]), "c": np.array(z[prefix + "c"][i]),
                "n_acc": int(z[prefix + "nacc"][i])} for i in range(len(z[prefix + "nacc"]))]
        if prefix + "hlo" in z:
            for i, p in enumerate(out):
                p["hist"] = {"lo": np.array(z[prefix + "hlo"][i]), "hi": np.array(z[prefix + "hhi"][i]),
                             "saturated": np.array(z[prefix + "hsat"][i]), "n_acc": p["n_acc"]}
        return out

    def save(self, pending):
        """What a resumed run must repeat (the alternatives' names and `cov`) and what it goes on from:
        the shift, the intervals of the window and the open sums, c included."""
        o = self._peek(pending)
        out = {"iw_names": np.array(self.names, dtype=str), "iw_cov": np.array(self.cov, dtype=np.int64),
               "iw_shift": np.zeros(self.spec.d) if self.shift is None else self.shift}
        if self.marg is not None:
            out["iw_hist_on"] = np.array(self.want, dtype=np.int64)
        out.update({"iw_iv_" + k: v for k, v in self._stack(self.ivs).items()})
        out.update({"iw_open_" + k: v for k, v in self._stack([o]).items()})
        return out

    def load(self, z, n_intervals):
        """Resume: the alternatives must be the ones the sums were formed with (their names and `cov`;
        the functions themselves cannot be compared); the shift, the window's intervals and the open
        sums come back, c included: no new maximum is taken for an interval that is under way."""
        fail = self.host.fail
        if "iw_names" not in z:
            fail("importance: cannot resume -- the run was written without importance (the window of its "
                 "sums cannot begin in mid-run)")
        saved = ([str(n) for n in z["iw_names"]], [bool(c) for c in z["iw_cov"]])
        if saved != (self.names, self.cov):
            fail("importance: cannot resume -- the run was written with the alternatives %r (cov: %r), and now "
                 "has %r (cov: %r): sums of different weights do not add up", *saved, self.names, self.cov)
        had = [bool(v) for v in z["iw_hist_on"]] if "iw_hist_on" in z else [False] * len(self.want)
        if had != self.want:
            fail("importance: cannot resume -- the run was written with marginals: %r per alternative, and now has "
                 "%r: a reweighted histogram cannot begin or end in mid-run", had, self.want)
        if self.marg is not None:      # (the marginals have configured the engine in their `load`)
            self._configure_hist()
        self.shift = np.array(z["iw_shift"], dtype=np.float64)
        self.ivs = self._unstack(z, "iw_iv_")
        if len(self.ivs) != n_intervals:
            fail("importance: the state file holds %d interval sums for %d intervals", len(self.ivs), n_intervals)
        self.open = self._unstack(z, "iw_open_")[0]
        try:
            self.engine.importance_set(self.open)
            if self.marg is not None:
                self.engine.importance_hist_set(self.open["hist"])
        except EngineError as e:
            fail("importance: %s", str(e), cause=e)

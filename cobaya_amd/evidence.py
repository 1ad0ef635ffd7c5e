"""Evidence of the run, ln Z = ln of the integral of L pi: the product (`Evidence`), the sampler option
behind it (`parse_option`) and what the sampler holds of it while it runs (`EvidenceAccumulator`, a
device product with the methods `marginals.MarginalsAccumulator` states, plus `learned`).

The estimator is Gelfand and Dey's harmonic mean with a truncated importance function (Robert and
Wraith 2009): for a normalised density phi whose support lies inside the prior's,
E_post[phi / (L pi)] = 1 / Z.  phi is uniform on an ellipsoid {|Linv (x - m)|^2 <= R^2} fixed BEFORE
the samples it is used on were drawn, so the estimate is unbiased in 1 / Z -- NOT in ln Z -- for any
target.  The sums come from the engine (mcmc_hip_evidence_*; evidence_kernels.hip), which looks at
every walker of every `every`-th moment snapshot.  The rule ("Evidence"): per
checkpoint interval, group g of group_size walkers and radius r (R^2_r = f_r d)

    acc[g][r] = sum over the interval's accumulations of the ordered sum of exp(c - logpost) over the
                group's walkers inside radius r,      cnt[g][r] = those walkers,

with c the maximum of logpost when the interval's ellipsoid became active.  Then

    ln Y_r = ln sum_g acc - ln(n_acc W) - c - [ln V_d + (d / 2) ln R^2_r + sum_i ln chol(C)_ii],

the intervals of the window averaged with weights n_acc, ln Z_r = -ln Y_r, and the standard error is
a delete-one-group jackknife (groups are independent chains, so it absorbs the correlation between
snapshots).  A radius whose ellipsoid leaves the prior box is `clipped`: reported, never chosen.
ONE ellipsoid spans the empty space between well-separated modes: the variance grows there (two
modes 6 sigma apart: sd of ln Z about 0.09 at d = 30 with 65 536 draws, about 0.2 at d = 2 with
4 096, against 0.006 and 0.025 for one mode); the spread of `lnZ_by_radius()` is the diagnostic.
"""
from __future__ import annotations

import math

import numpy as np

from .engine import EngineError
from .product import DeviceProduct, option_dict, option_int

MAX_RADII = 8               # evidence_args.h: kEvMaxRadii
MAX_DIM = 256               # evidence_args.h: kEvMaxDim
DEFAULT_RADII = (0.5, 0.75, 1.0, 1.5, 2.0)
OPTION_KEYS = ("radii", "every")


class EvidenceError(ValueError):
    """An `evidence` option (or a pair of products) that cannot be served; the message begins with
    the option's name."""


# ---------------------------------------------------------------------------------- ellipsoids
def ell_parts(ell, d):
    """(m[d], Linv[d, d], c) of a flat ellipsoid m | Linv | c."""
    ell = np.asarray(ell, dtype=np.float64)
    return ell[:d], ell[d:d + d * d].reshape(d, d), float(ell[-1])


def log_ball(d):
    """ln V_d, the volume of the unit ball: pi^(d / 2) / Gamma(d / 2 + 1)."""
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def log_volume(ell, d, r2):
    """ln of the ellipsoid's volume per radius: ln V_d + (d / 2) ln R^2 + sum_i ln chol(C)_ii (the
    diagonal of chol(C) is one over that of its inverse)."""
    _, Linv, _ = ell_parts(ell, d)
    return log_ball(d) + 0.5 * d * np.log(np.asarray(r2, np.float64)) - float(np.sum(np.log(np.diag(Linv))))


def clipped_radii(ell, d, r2, lo, hi):
    """bool per radius: m_i +- R sqrt(C_ii) leaves [lo_i, hi_i] in some dimension (the ellipsoid's
    bounding box; on the wall is inside)."""
    m, Linv, _ = ell_parts(ell, d)
    L = np.linalg.inv(Linv)
    sig = np.sqrt(np.sum(np.tril(L) ** 2, axis=1))
    R = np.sqrt(np.asarray(r2, np.float64))[:, None]
    return np.any((m - R * sig < np.asarray(lo)) | (m + R * sig > np.asarray(hi)), axis=1)


def prior_box(spec):
    """(lo[d], hi[d]) of the prior support: the bounds of a uniform prior, unbounded otherwise."""
    uniform = np.asarray(spec.kinds).astype(int) == 0
    a, b = np.asarray(spec.a, np.float64), np.asarray(spec.b, np.float64)
    return np.where(uniform, a, -np.inf), np.where(uniform, b, np.inf)


# ---------------------------------------------------------------------------------- the product
class Evidence:
    """ln Z with its jackknife error, per radius and the headline.

    `d`; `radii`: the ladder f_r (R^2 = f d); `n_walkers`: the walkers of the `G` groups held;
    per interval of the window (first axis): `sums` float64 [n, G, n_r], `counts` uint64
    [n, G, n_r], `c` float64 [n, G] (a group's centring constant: that of its process), `n_acc`
    int64 [n], `lnvol` float64 [n, n_r], `clip` bool [n, n_r]; `clamped`: arguments above 700."""

    reports = True

    def __init__(self, d, radii, n_walkers, sums, counts, c, n_acc, lnvol, clip, clamped=0):
        self.d, self.n_walkers, self.clamped = int(d), int(n_walkers), int(clamped)
        self.radii = [float(f) for f in radii]
        n_r = len(self.radii)
        self.n_acc = np.array(n_acc, dtype=np.int64).reshape(-1)
        n = len(self.n_acc)
        self.sums = np.array(sums, dtype=np.float64).reshape(n, -1, n_r)
        G = self.sums.shape[1]
        try:
            self.counts = np.array(counts, dtype=np.uint64).reshape(n, G, n_r)
            self.c = np.array(c, dtype=np.float64).reshape(n, G)
            self.lnvol = np.array(lnvol, dtype=np.float64).reshape(n, n_r)
            self.clip = np.array(clip, dtype=bool).reshape(n, n_r)
        except ValueError as e:
            raise EvidenceError(f"evidence: the arrays of {n} intervals, {G} groups and {n_r} radii "
                                f"do not fit together ({e})") from None

    # -- the estimate
    @property
    def n_groups(self):
        return self.sums.shape[1]

    @property
    def n_samples(self):
        """Walkers looked at: accumulations x walkers."""
        return int(self.n_acc.sum()) * self.n_walkers

    def _group_logs(self, r):
        """ln of every group's total over the window, each term scaled by its interval's
        exp(-c) / volume (-inf: nothing inside)."""
        with np.errstate(divide="ignore"):
            lt = np.log(self.sums[:, :, r]) - self.c - self.lnvol[:, r][:, None]
        if lt.shape[0] == 0:
            return np.full(self.n_groups, -np.inf)
        M = lt.max(axis=0)
        safe = np.where(np.isfinite(M), M, 0.0)
        with np.errstate(divide="ignore"):
            return safe + np.log(np.exp(lt - safe).sum(axis=0))

    def _estimate(self, r):
        """(ln Z, standard error) of radius r."""
        N, W, G = float(self.n_acc.sum()), float(self.n_walkers), self.n_groups
        lT = self._group_logs(r)
        M = lT.max() if G else -np.inf
        if N <= 0 or not np.isfinite(M):
            return float("nan"), float("nan")
        t = np.exp(lT - M)
        tot = t.sum()
        lnZ = -(M + math.log(tot) - math.log(W * N))
        if G < 2:
            return lnZ, float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            loo = -(M + np.log(tot - t) - math.log((W - W / G) * N))
        err = math.sqrt((G - 1.0) / G * float(np.sum((loo - loo.mean()) ** 2))) if np.all(np.isfinite(loo)) \
            else float("nan")
        return lnZ, err

    def lnZ_by_radius(self):
        """float64 [n_r]; their spread is the diagnostic of a posterior one ellipsoid fits badly."""
        return np.array([self._estimate(r)[0] for r in range(len(self.radii))])

    def stderr_by_radius(self):
        return np.array([self._estimate(r)[1] for r in range(len(self.radii))])

    def clipped(self):
        """bool [n_r]: the ellipsoid of some interval left the prior box at that radius -- the
        value is biased (the integral of phi over the support is below 1) and never chosen."""
        used = self.n_acc > 0
        return np.any(self.clip[used], axis=0) if used.any() else np.zeros(len(self.radii), bool)

    def inside_fraction(self):
        """float64 [n_r]: the share of the walkers looked at that fell inside."""
        n = self.n_samples
        inside = self.counts.sum(axis=(0, 1)).astype(np.float64)
        return inside / n if n else np.full(len(self.radii), np.nan)

    def _choice(self):
        """Index of the headline radius: unclipped, the smallest standard error (None: none)."""
        lnZ, err, clip = self.lnZ_by_radius(), self.stderr_by_radius(), self.clipped()
        ok = [r for r in range(len(self.radii)) if not clip[r] and np.isfinite(lnZ[r])]
        if not ok:
            return None
        with_err = [r for r in ok if np.isfinite(err[r])]
        return min(with_err, key=lambda r: err[r]) if with_err else ok[0]

    @property
    def lnZ(self):
        r = self._choice()
        return float("nan") if r is None else float(self._estimate(r)[0])

    @property
    def stderr(self):
        r = self._choice()
        return float("nan") if r is None else float(self._estimate(r)[1])

    @property
    def radius(self):
        """The f_r of the headline (None: every radius is clipped or empty)."""
        r = self._choice()
        return None if r is None else self.radii[r]

    def summary(self):
        """One line for the log at the end of a run."""
        if self._choice() is None:
            return "Evidence: no unclipped radius holds a sample (%d snapshots of the ensemble)." % int(self.n_acc.sum())
        by = ", ".join("%.4g" % v for v in self.lnZ_by_radius())
        return ("Evidence: ln Z = %.5g +- %.2g (R^2 = %g d; by radius: %s; %d snapshots of the ensemble%s)."
                % (self.lnZ, self.stderr, self.radius, by, int(self.n_acc.sum()),
                   "; %d arguments clamped" % self.clamped if self.clamped else ""))

    # -- arithmetic, files
    def _layout(self):
        return (self.d, tuple(self.radii), tuple(self.n_acc.tolist()), self.lnvol.tobytes(), self.clip.tobytes())

    def merge(self, other):
        """The groups of two shards of one run, side by side."""
        if not isinstance(other, Evidence) or self._layout() != other._layout():
            raise EvidenceError("evidence: only shards of one run (dimension, radii, intervals and "
                                "ellipsoids) merge")
        return Evidence(self.d, self.radii, self.n_walkers + other.n_walkers,
                        np.concatenate((self.sums, other.sums), axis=1),
                        np.concatenate((self.counts, other.counts), axis=1),
                        np.concatenate((self.c, other.c), axis=1), self.n_acc, self.lnvol, self.clip,
                        self.clamped + other.clamped)

    def __eq__(self, other):
        return (isinstance(other, Evidence) and self._layout() == other._layout()
                and (self.n_walkers, self.clamped) == (other.n_walkers, other.clamped)
                and np.array_equal(self.sums, other.sums) and np.array_equal(self.counts, other.counts)
                and np.array_equal(self.c, other.c))

    __hash__ = None

    def save(self, path):
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, geometry=np.array([self.d, self.n_walkers, self.clamped], dtype=np.int64),
                     radii=np.array(self.radii, dtype=np.float64), sums=self.sums, counts=self.counts,
                     c=self.c, n_acc=self.n_acc, lnvol=self.lnvol, clip=self.clip,
                     # (for a reader without this class)
                     lnZ=np.float64(self.lnZ), stderr=np.float64(self.stderr),
                     lnZ_by_radius=self.lnZ_by_radius(), stderr_by_radius=self.stderr_by_radius(),
                     clipped=self.clipped())

    @classmethod
    def load(cls, path):
        z = np.load(path, allow_pickle=False)
        d, W, clamped = (int(v) for v in z["geometry"])
        return cls(d, z["radii"], W, z["sums"], z["counts"], z["c"], z["n_acc"], z["lnvol"], z["clip"], clamped)


# ---------------------------------------------------------------------------------- the option
def parse_option(opt):
    """The sampler option `evidence` -> None (off) or {"radii": [f_r], "every": k}.  `True` = the
    default ladder beside every moment snapshot.  Refuses, by the option's name, unknown keys,
    radii that are not 1..8 ascending positive numbers and an `every` below 1."""
    opt = option_dict(opt, "evidence", OPTION_KEYS, EvidenceError)
    if opt is None:
        return None
    radii = opt.get("radii", DEFAULT_RADII)
    try:
        ok = not isinstance(radii, (str, bytes)) and all(
            not isinstance(f, bool) and isinstance(f, (int, float, np.integer, np.floating)) for f in radii)
        radii = [float(f) for f in radii] if ok else None
    except TypeError:
        radii = None
    if radii is None or not 1 <= len(radii) <= MAX_RADII or not all(math.isfinite(f) and f > 0 for f in radii) \
            or any(b <= a for a, b in zip(radii, radii[1:])):
        raise EvidenceError(f"evidence: radii must be 1..{MAX_RADII} ascending positive numbers, got "
                            f"{opt.get('radii')!r}")
    every = option_int(opt.get("every", 1), "evidence: every", 1, None, EvidenceError)
    return {"radii": radii, "every": every}


# ---------------------------------------------------------------------------------- the sampler's side
ENGINE_METHODS = ("configure_evidence", "evidence_set_ellipsoid", "accumulate_evidence", "request_evidence",
                  "fetch_evidence", "evidence_set", "evidence_layout")


class EvidenceAccumulator(DeviceProduct):
    """What the sampler holds of the sums while it runs: a device product whose unfinished interval
    is never split, and the one with `learned(centre, covmat)`.  A part is the closing request's
    read-out: sums, counts, `n` and the ellipsoid it was taken under; the peek is a request that does
    not close.  The ellipsoid handed to `learned` is only staged; the engine activates it, with a
    fresh c, inside the next closing request, so no interval mixes two ellipsoids."""

    name, closes, error, ENGINE_METHODS, MAX_DIM = "evidence", True, EvidenceError, ENGINE_METHODS, MAX_DIM
    tempered = ("evidence: the sums weigh the walkers as they are, which at temperature %g follow "
                "the tempered law, not the posterior; use temperature: 1 or turn evidence off")
    predates = "evidence: this engine keeps no evidence sums (its library predates mcmc_hip_evidence_*)"

    def __init__(self, cfg, spec, host):
        super().__init__(cfg, spec, host)
        self.phase, self.centre = 0, None
        self.r2 = np.array([f * spec.d for f in cfg["radii"]], dtype=np.float64)

    @staticmethod
    def parse(opt, spec):
        return parse_option(opt)

    def attach(self, engine, resumed=False, centre=None, covmat=None):
        """Hand the radii to the engine and activate the first ellipsoid: the initial points' mean
        and the proposal covariance in force at initialize().  A resumed run takes the ellipsoids
        of the state file: `load`."""
        self.engine = engine
        try:
            engine.configure_evidence(self.r2)
            lay = engine.evidence_layout()
            if (lay["on"], lay["n_radii"], lay["n_ell"]) != (1, len(self.r2), self.spec.d * (self.spec.d + 1) + 1):
                self.host.fail("evidence: the engine lays its sums out differently (%r) from the product", lay)
            if not resumed:
                self.centre = np.array(centre, dtype=np.float64)
                engine.evidence_set_ellipsoid(self.centre, covmat)
        except EngineError as e:
            self.host.fail("evidence: %s", str(e), cause=e)

    def accumulate(self):
        self.phase += 1
        if self.phase % self.cfg["every"] == 0:
            self.engine.accumulate_evidence()

    def learned(self, centre, covmat):
        """Stage the ellipsoid of the window's pooled mean and covariance (no mean: the centre
        stays).  A covariance the library cannot factorise leaves the ellipsoids as they are."""
        if centre is not None:
            self.centre = np.array(centre, dtype=np.float64)
        try:
            self.engine.evidence_set_ellipsoid(self.centre, covmat)
        except EngineError:
            pass

    def _meta(self, part):
        """(ln volume, clipped) per radius of a part's ellipsoid, worked out once."""
        if "lnvol" not in part:
            d = self.spec.d
            part["lnvol"] = log_volume(part["active"], d, self.r2)
            part["clip"] = clipped_radii(part["active"], d, self.r2, *prior_box(self.spec))
        return part["lnvol"], part["clip"]

    def product(self, intervals, combined=False, pending=False):
        """The intervals of the window, in their order, plus the unfinished interval."""
        host, d, n_r = self.host, self.spec.d, len(self.r2)
        parts, last = self._parts(pending), self.open
        parts = [p for p in parts if p["n"] > 0 and p["active"] is not None]
        n, G = len(parts), (last["sums"].shape[0] if last is not None else 0)
        sums = np.array([p["sums"] for p in parts], dtype=np.float64).reshape(n, G, n_r)
        counts = np.array([p["counts"] for p in parts], dtype=np.uint64).reshape(n, G, n_r)
        c = np.repeat(np.array([p["active"][-1] for p in parts], dtype=np.float64).reshape(n, 1), G, axis=1)
        n_acc = np.array([p["n"] for p in parts], dtype=np.int64)
        meta = [self._meta(p) for p in parts]
        lnvol = np.array([m[0] for m in meta], dtype=np.float64).reshape(n, n_r)
        clip = np.array([m[1] for m in meta], dtype=bool).reshape(n, n_r)
        clamped, n_walkers = sum(int(p["clamped"]) for p in parts), int(host.n_walkers)
        if combined and host.size > 1:
            # ONE host all-reduce of a zero matrix in which every process fills its own row: the
            # groups of all processes side by side (every process has closed the same intervals)
            if np.any(counts >= np.uint64(2 ** 53)):
                host.fail("evidence: a count above 2^53 cannot be carried over processes exactly")
            row = np.concatenate((sums.reshape(-1), counts.astype(np.float64).reshape(-1), c.reshape(-1),
                                  [float(clamped), float(n)]))
            buf = np.zeros((int(host.size), len(row)))
            buf[host.rank] = row
            flat = buf.reshape(-1)
            out = host.all_reduce_sum(flat)
            buf = (flat if out is None else np.asarray(out)).reshape(buf.shape)
            if not np.all(buf[:, -1] == float(n)):
                host.fail("evidence: the processes hold different numbers of intervals (%r)", buf[:, -1].tolist())
            k = n * G * n_r
            sums = np.concatenate([b[:k].reshape(n, G, n_r) for b in buf], axis=1)
            counts = np.concatenate([b[k:2 * k].astype(np.uint64).reshape(n, G, n_r) for b in buf], axis=1)
            c = np.concatenate([b[2 * k:2 * k + n * G].reshape(n, G) for b in buf], axis=1)
            clamped, n_walkers = int(buf[:, -2].sum()), n_walkers * int(host.size)
        return Evidence(d, self.cfg["radii"], n_walkers, sums, counts, c, n_acc, lnvol, clip, clamped)

    def save(self, pending):
        """What a resumed run must repeat (radii, every) and what it goes on from: the intervals
        of the window, the open sums, the snapshot phase, and the active and staged ellipsoids."""
        o = self._peek(pending)
        n, G, n_r = len(self.ivs), o["sums"].shape[0], len(self.r2)
        n_ell = self.spec.d * (self.spec.d + 1) + 1
        none = np.zeros(0)
        return {"ev_radii": np.array(self.cfg["radii"], dtype=np.float64),
                "ev_book": np.array([self.cfg["every"], self.phase], dtype=np.int64),
                "ev_centre": self.centre,
                "ev_iv_sums": np.array([p["sums"] for p in self.ivs], dtype=np.float64).reshape(n, G, n_r),
                "ev_iv_counts": np.array([p["counts"] for p in self.ivs], dtype=np.uint64).reshape(n, G, n_r),
                "ev_iv_n": np.array([[p["n"], p["clamped"]] for p in self.ivs], dtype=np.int64).reshape(n, 2),
                "ev_iv_ell": np.array([p["active"] for p in self.ivs], dtype=np.float64).reshape(n, n_ell),
                "ev_open_sums": o["sums"], "ev_open_counts": o["counts"],
                "ev_open_n": np.array([o["n"], o["clamped"]], dtype=np.int64),
                "ev_active": none if o["active"] is None else o["active"],
                "ev_staged": none if o["staged"] is None else o["staged"]}

    def load(self, z, n_intervals):
        """Resume: radii and `every` must be the ones the sums were formed with; the window's
        intervals, the open sums and both ellipsoids come back, c included."""
        cfg, fail = self.cfg, self.host.fail
        if "ev_iv_sums" not in z:
            fail("evidence: cannot resume -- the run was written without evidence (the window of "
                 "its sums cannot begin in mid-run)")
        saved = ([float(f) for f in z["ev_radii"]], int(z["ev_book"][0]))
        if saved != (cfg["radii"], cfg["every"]):
            fail("evidence: cannot resume -- the run was written with radii %r and every %d, and now "
                 "has %r and %d (sums of different radii do not add up)", *saved, cfg["radii"], cfg["every"])
        self.phase, self.centre = int(z["ev_book"][1]), np.array(z["ev_centre"], dtype=np.float64)
        self.ivs = [{"sums": np.array(s, dtype=np.float64), "counts": np.array(c, dtype=np.uint64),
                     "n": int(n[0]), "clamped": int(n[1]), "active": np.array(e, dtype=np.float64), "staged": None}
                    for s, c, n, e in zip(z["ev_iv_sums"], z["ev_iv_counts"], z["ev_iv_n"], z["ev_iv_ell"])]
        if len(self.ivs) != n_intervals:
            fail("evidence: the state file holds %d interval sums for %d intervals", len(self.ivs), n_intervals)
        act = z["ev_active"] if len(z["ev_active"]) else None
        stg = z["ev_staged"] if len(z["ev_staged"]) else None
        # the unfinished interval and both ellipsoids go back to the device
        try:
            self.engine.evidence_set(z["ev_open_sums"], z["ev_open_counts"], int(z["ev_open_n"][1]),
                                     int(z["ev_open_n"][0]), act, stg)
        except EngineError as e:
            fail("evidence: %s", str(e), cause=e)

"""What the six device products of the sampler share: the protocol and its state machine
(`DeviceProduct`) and the preamble of their options (`option_dict`, `known_keys`, `option_int`).
A seventh product starts here, and with a `Readout` in the library (csrc/readout.h)."""
from __future__ import annotations

import numpy as np


def known_keys(d, what, keys, error):
    unknown = sorted(set(d) - set(keys))
    if unknown:
        raise error(f"{what}: unknown key(s) {unknown}; valid keys: {list(keys)}")


def option_dict(opt, name, keys, error, default=None, expected="True, None or a dict"):
    """A sampler option as a dict with known keys, or None where it is off (None, False).  `True`
    stands for `default`.  Refuses, by the option's name, with the module's `error`."""
    if opt is None or opt is False:
        return None
    if opt is True:
        opt = dict(default or {})
    if not isinstance(opt, dict):
        raise error(f"{name}: expected {expected}, got {opt!r}")
    known_keys(opt, name, keys, error)
    return opt


def option_int(v, what, lo, hi, error):
    """`v` as an int in lo..hi (hi None: no upper end); `what`: "<option>: <key>"."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v \
            or int(v) < lo or (hi is not None and int(v) > hi):
        span = f"in {lo}..{hi}" if hi is not None else f">= {lo}"
        raise error(f"{what} must be an integer {span}, got {v!r}")
    return int(v)


def option_ranges(ranges, name, known, error):
    """`ranges` of an option: "prior", "covmat", or {name: (lo, hi)} over `known` names, cleaned."""
    if isinstance(ranges, str) and ranges in ("prior", "covmat"):
        return ranges
    if not isinstance(ranges, dict):
        raise error(f"{name}: ranges must be a dict, 'prior' or 'covmat', got {ranges!r}")
    bad = sorted(str(n) for n in ranges if n not in known)
    if bad:
        raise error(f"{name}: ranges names unknown parameter(s) {bad}")
    clean = {}
    for n, r in ranges.items():
        try:
            lo, hi = float(r[0]), float(r[1])
            ok = len(r) == 2
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok or not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise error(f"{name}: ranges[{n!r}] must be a finite [lo, hi] with lo < hi, got {r!r}")
        clean[str(n)] = (lo, hi)
    return clean


class DeviceProduct:
    """What the sampler holds of a device product while it runs.  A DEVICE PRODUCT is a subclass,
    listed in `EnsembleMCMC.PRODUCT_CLASSES`: `DerivedAccumulator`, `MarginalsAccumulator`,
    `AutoCorrAccumulator`, `BestFitAccumulator`, `EvidenceAccumulator`, `ImportanceAccumulator`.
    The sampler calls

      from_option(opt, spec, engine_factory, host) -> the object, or None where the option is off;
          refuses by the option's name BEFORE the engine is created.  `host` is what the sampler hands
          in: fail(msg, *args, cause=None), n_walkers, size, rank, all_reduce_sum, temperature,
          snapshot_steps (the steps between two moment snapshots)
      attach(engine, resumed, centre, covmat): configure the engine, cross-check its layout
      accumulate(), request(): beside every moment snapshot; beside every checkpoint request
      fetch_requested(): the requested read-out, kept in `fetched` until file(n_snap) closes the
          interval (an entry of `ivs` if n_snap is non-zero: one per interval of the window)
      drop(k): the window moved forward by k intervals
      save(pending) -> arrays for the state file, load(z, n_intervals): from it
      product(intervals, combined, pending); detach(pending): the engine goes, product() still works
      name, reports: the option (`option` where it is spelt differently), the key in products() and
          the file `prefix.<name>.npz`; whether the product has a summary() for the log
      learned(centre, covmat) -- OPTIONAL: after every checkpoint that yields a positive-definite
          covariance, the window's pooled mean (None where the host does not know it) and
          `mean_of_covs`
    `pending`: a checkpoint is requested and not processed yet -- its read-out is then fetched before
    anything else is read, and a product counts it as the newest interval.

    A subclass states `name`, `error` (its module's error class), `parse(opt, spec)`,
    `ENGINE_METHODS`, `predates` (what an engine without them is told) and, where it refuses
    `temperature != 1`, `tempered` (with one %g); it writes attach, product, save and load.  The engine
    is reached through request_<name>, fetch_<name> and <name>_set.  The unfinished interval comes in
    two flavours:

      split = False (autocorr, evidence, derived, importance): the sums are floats and the interval
          is NEVER split (a host part would change the order of the additions, hence the bits).  It
          stays on the device, `_peek` reads it without disturbing it, and an interval is the
          requested read-out alone.  `open`: the open interval as last read, which is what a product
          is formed from once the engine is gone.  `closes`: request_<name> takes a flag, and a
          request that does not close is the peek; else the peek reads out and sets back.
      split = True (marginals, bestfit): counts and maxima are exact, so `open` is the host's part,
          the device holds the rest, and `_drain` moves that over (which empties it on the device).
          The subclass states `_merge(a, b)` of two parts, `_empty()` and what of a part `ivs` keeps.

    `live` False: the product sums nothing (derived_stats: False) and the engine is not asked."""

    reports, split, closes, live, tempered = True, False, False, True, None

    def __init__(self, cfg, spec, host):
        self.cfg, self.spec, self.host, self.engine = cfg, spec, host, None
        self.ivs, self.open, self.fetched = [], None, None

    @classmethod
    def from_option(cls, opt, spec, engine_factory, host):
        try:
            cfg = cls.parse(opt, spec)
        except cls.error as e:
            host.fail("%s", str(e), cause=e)
        if cfg is None:
            return None
        if cls.tempered and host.temperature != 1:
            host.fail(cls.tempered, host.temperature)
        if not all(hasattr(engine_factory, m) for m in cls.ENGINE_METHODS):
            host.fail(cls.predates)
        if spec.d > getattr(cls, "MAX_DIM", spec.d):
            host.fail("%s: the %s kernel serves at most %d parameters, not %d", cls.name, cls.name,
                      cls.MAX_DIM, spec.d)
        return cls(cfg, spec, host)

    # -- the engine's side
    def _request(self, close=True):
        f = getattr(self.engine, "request_" + self.name)
        f(close) if self.closes else f()

    def _fetch(self):
        return getattr(self.engine, "fetch_" + self.name)()

    def _set(self, part):
        f = getattr(self.engine, self.name + "_set")
        f(*part) if isinstance(part, tuple) else f(part)

    def accumulate(self):
        getattr(self.engine, "accumulate_" + self.name)()

    def request(self):
        if self.live:
            self._request()

    def fetch_requested(self):
        if self.live and self.fetched is None:
            self.fetched = self._fetch()

    # -- the unfinished interval
    def _peek(self, pending):
        """The open interval, read WITHOUT disturbing it: a request that does not close, or a read-out
        (which zeroes the sums in stream order) set back to the same values, so that the device goes
        on adding to exactly the numbers it held."""
        if self.engine is not None and self.live:
            if pending:
                self.fetch_requested()
            self._request(False)
            self.open = self._fetch()
            if not self.closes:
                self._set(self.open)
        return self.open

    def _drain(self, pending):
        """Move what the device holds of the unfinished interval into `open`."""
        if pending:
            self.fetch_requested()
        self._request()
        self.open = self._merge(self.open, self._fetch())

    def _kept(self, part):
        return part

    def file(self, n_snap):
        """The interval closes: the read-out of the request at this checkpoint (split: merged with
        what the host held of it)."""
        if not self.live:
            return
        part, self.fetched = self.fetched, None
        if self.split:
            part = self.open if part is None else self._merge(self.open, part)
            self.open = self._empty()
        elif part is None:    # (no read-out was queued: request and fetch now)
            self._request()
            part = self._fetch()
        if n_snap:
            self.ivs.append(self._kept(part))

    def drop(self, k):
        self.ivs = self.ivs[k:]

    def _parts(self, pending):
        """Never split: the intervals of the window, in their order, the requested read-out that is
        not filed yet (the newest interval) and the unfinished interval."""
        parts = list(self.ivs)
        if self.fetched is not None:
            parts.append(self.fetched)
        last = self._peek(pending)
        return parts if last is None else parts + [last]

    def _merged(self, intervals, pending):
        """Split: the unfinished interval, the requested read-out that is not filed yet and the
        intervals of the window (`ivs` entries with their accumulations), merged into one part."""
        if self.engine is not None:
            self._drain(pending)
        part = self.open
        if self.fetched is not None:
            part = self._merge(part, self.fetched)
        for (n_snap, _, _), iv in zip(intervals, self.ivs):
            part = self._merge(part, (*iv, int(n_snap)) if isinstance(iv, tuple) else (iv, int(n_snap)))
        return part

    def detach(self, pending=False):
        if self.engine is not None and self.live and not (self.split and self.open is None):
            # (split: the device's part of the unfinished interval; else: kept for product())
            self._drain(pending) if self.split else self._peek(pending)
        self.engine = None

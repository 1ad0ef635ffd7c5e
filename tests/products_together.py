"""What the tests of the six device products SWITCHED ON TOGETHER share (tests/test_products_together_host.py,
tests/test_gpu_products_together.py): one option set with everything on, the CPU doubles composed into one
engine, and the comparison of two products down to their bytes.  No test lives here.

`ALL` switches on the five sampler options (`marginals`, `autocorr`, `bestfit`, `evidence`, `importance`) at
small sizes, and `DERIVED` adds two function-derived parameters to `params`, the second taking the first as
an argument, which switches on the sixth product (`derived`).  Every function here -- derived and log-weight
alike -- uses `+`, `-` and `*` on float64 only, squares written as products: each operation is then exactly
rounded, torch on the device and numpy on the host give the same bits, and ONE source string serves both
(`fn(source)` evaluates it for numpy).

There is no CPU double of the derived rows: ON THE HOST `derived` STAYS OUT.  `on_host(options)` takes the
derived name out of `marginals`, and the host tests use a model without `DERIVED`; the derived rows, their
sums and their way into the histogram are tested on the device alone."""
import copy

import numpy as np

from tests.autocorr_ref import AcOracleEngine
from tests.bestfit_ref import BfOracleEngine
from tests.evidence_ref import EvOracleEngine
from tests.importance_ref import ImOracleEngine
from tests.test_marginals_host import MargOracleEngine

# the function-derived parameters, in `params` order (t reads s)
DERIVED_FUNCTIONS = {"s": "lambda a, b: a + b", "t": "lambda a, s: a * s - s"}
# the log-weights of the two importance alternatives
IMPORTANCE_FUNCTIONS = {"bao": "lambda a: -0.5 * (((a - 0.31) * 2.5) * ((a - 0.31) * 2.5))",
                        "tilt": "lambda a, b: 0.5 * a - 0.25 * (b * b)"}
IMPORTANCE_COV = {"bao": True, "tilt": False}
DERIVED_RANGE = {"s": [-4.0, 4.0]}
PRODUCTS = ("derived", "marginals", "autocorr", "bestfit", "evidence", "importance")
ON_HOST = PRODUCTS[1:]


def renamed(source, names):
    """A function of `a` and `b` as the same function of the first two of `names`."""
    to = {"a": str(names[0]), "b": str(names[1])}
    return "".join(to.get(tok, tok) for tok in _tokens(source))


def _tokens(text):
    out, word = [], ""
    for ch in text:
        if ch.isalnum() or ch == "_":
            word += ch
        else:
            if word:
                out.append(word)
                word = ""
            out.append(ch)
    return out + ([word] if word else [])


def fn(source):
    """The function of a source string, for numpy arrays (the same text torch evaluates on the device)."""
    return eval(source, {})  # noqa: S307


def all_options(names=("a", "b")):
    """Everything on, over a model whose first two sampled parameters are `names[:2]`."""
    a, b = names[0], names[1]
    return {
        "marginals": {"params": list(names) + ["s"], "pairs": [[b, a]], "bins": 16, "bins2d": 8,
                      "ranges": copy.deepcopy(DERIVED_RANGE)},
        "autocorr": {"params": [b, a], "lags": 3},
        "bestfit": {"params": "all", "bins": 16},
        "evidence": {"radii": [1.0, 2.0]},
        "importance": {k: {"function": renamed(src, names), "cov": IMPORTANCE_COV[k]}
                       for k, src in IMPORTANCE_FUNCTIONS.items()},
    }


def derived_params(names=("a", "b")):
    """The `params` entries of the two derived functions."""
    return {k: {"derived": renamed(src, names)} for k, src in DERIVED_FUNCTIONS.items()}


ALL = all_options()
DERIVED = derived_params()


def on_host(options):
    """`options` without what needs the derived rows (for which there is no double)."""
    out = copy.deepcopy(options)
    if out.get("marginals"):
        out["marginals"]["params"] = [n for n in out["marginals"]["params"] if n not in DERIVED_FUNCTIONS]
        out["marginals"]["ranges"] = {n: r for n, r in out["marginals"]["ranges"].items()
                                      if n not in DERIVED_FUNCTIONS} or "prior"
    return out


def only(options, name):
    """The option set with `name` alone switched on."""
    return {k: (copy.deepcopy(v) if k == name else None) for k, v in options.items()}


# ------------------------------------------------------------------------------- the composed double
class AllOracleEngine(ImOracleEngine, EvOracleEngine, BfOracleEngine, AcOracleEngine, MargOracleEngine):
    """The five CPU doubles as one engine, by plain inheritance (their method names are disjoint and none has
    an `__init__` of its own).  `log` keeps what the sampler asked of it, in stream order, as (verb, what,
    flag): ("step", None, n), ("accumulate" | "fetch" | "set", product, None), ("request", product, closes?),
    with "moments" among the products for the checkpoint's own request and fetch."""

    @property
    def log(self):
        return self.__dict__.setdefault("_together_log", [])

    def step(self, n_steps):
        self.log.append(("step", None, int(n_steps)))
        return super().step(n_steps)


def _logged(method, verb, what, closes):
    def call(self, *args, **kw):
        flag = None
        if verb == "request":
            flag = bool(args[0] if args else kw.get("close", True)) if closes else True
        self.log.append((verb, what, flag))
        return getattr(super(AllOracleEngine, self), method)(*args, **kw)
    call.__name__ = method
    return call


for _what in ON_HOST + ("moments",):
    for _verb, _method in (("accumulate", "accumulate_" + _what), ("request", "request_" + _what),
                           ("fetch", "fetch_" + _what), ("set", _what + "_set")):
        if _what == "moments" and _verb in ("accumulate", "set"):
            continue
        setattr(AllOracleEngine, _method, _logged(_method, _verb, _what, _what in ("evidence", "importance")))


# ------------------------------------------------------------------------------- two products, to the byte
# what of a product is compared byte by byte beside its own `==` (which, through np.array_equal, takes -0.0
# for +0.0): its sums, counts and records
BYTES = {
    "marginals": ("slab",),
    "autocorr": ("sums", "n_pairs"),
    "bestfit": ("slab", "records"),
    "evidence": ("sums", "counts", "c", "n_acc"),
    "derived": ("A", "B", "C", "X", "V", "bad"),
    "importance": ("sums", "n", "C", "n_zero", "n_nonfinite", "n_clamped"),
}


def same_product(name, a, b):
    """Two product objects of `name` are equal, and their sums, counts and records have the same bytes."""
    assert type(a) is type(b), (name, type(a), type(b))
    assert a == b, f"{name}: the products differ"
    for attr in BYTES[name]:
        va, vb = getattr(a, attr), getattr(b, attr)
        va, vb = (va, vb) if isinstance(va, (list, tuple)) else ([va], [vb])
        assert len(va) == len(vb), (name, attr)
        for k, (x, y) in enumerate(zip(va, vb)):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape, (name, attr, k, x.dtype, y.dtype, x.shape, y.shape)
            assert x.tobytes() == y.tobytes(), f"{name}: {attr}[{k}] differs in its bytes"
    if name == "derived":     # (min and max: NaN where nothing was finite; -0.0 and +0.0 differ)
        for attr in ("vmin", "vmax"):
            x, y = getattr(a, attr), getattr(b, attr)
            assert np.all((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))), (name, attr)
    return True


# ------------------------------------------------------------------------------- a run, replayed through the rules
def same_bits(got, want, where=()):
    """`got` holds what `want` holds, bit for bit: dicts by the keys of `want`, tuples entry by entry, float
    arrays by their bits (the payload of a NaN is not part of any rule: NaN equals NaN), the rest by value."""
    if isinstance(want, dict):
        for k in want:
            same_bits(got[k], want[k], where + (k,))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), (where, len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, where + (k,))
    elif want is None:
        assert got is None, where
    elif isinstance(want, np.ndarray) and want.dtype == np.float64:
        g, w = np.asarray(got, np.float64).reshape(-1), want.reshape(-1)
        assert g.shape == w.shape, (where, g.shape, w.shape)
        ok = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
        assert ok.all(), (where, np.flatnonzero(~ok)[:6], g[~ok][:6], w[~ok][:6])
    elif isinstance(want, np.ndarray):
        g = np.asarray(got).reshape(-1)
        assert g.shape == want.reshape(-1).shape and np.array_equal(g, want.reshape(-1)), (where, g[:8], want.reshape(-1)[:8])
    else:
        assert got == want, (where, got, want)
    return True


def snapshots_of(smp):
    """Every accumulated snapshot of a run that stores one per launch (`snapshot_every` = `steps_per_launch`,
    `moments_every` 1, nothing thinned out): the blocks of the stored rows, as the states the rules take."""
    d, spl = smp.spec.d, int(smp.steps_per_launch)
    assert int(smp.snapshot_every) == spl and int(smp.moments_every) == 1 and smp._snap_stride == 1
    assert len(smp._rows) == smp._launches and smp._carried is None
    out = []
    for k, blk in enumerate(smp._rows, start=1):
        blk = np.asarray(blk, dtype=np.float64)
        out.append({"x": np.ascontiguousarray(blk[:, 5:5 + d]), "logpost": blk[:, 2].copy(), "logprior": blk[:, 3].copy(),
                    "loglike": blk[:, 4].copy(), "z": np.ascontiguousarray(blk[:, 5 + d:]), "step": k * spl})
    return out


def held_parts(smp):
    """{product: [the window's intervals ..., the unfinished interval]} as the accumulators hold them (call
    `products()` first: it brings the unfinished interval to the host)."""
    return {p.name: list(p.ivs) + [p.open] for p in smp._products if p.live}


def replay(smp):
    """{product: [the window's intervals ..., the unfinished interval]} from the numpy RULES applied to the
    stored rows of `smp`, interval by interval, in the form `held_parts` gives.  The derived values and the
    log-weights are formed here with numpy from the stored x, by the functions the run was given; `evidence`
    takes the ellipsoid (c included) that each interval's read-out reports as active."""
    from tests import autocorr_ref, bestfit_ref, derived_ref, evidence_ref, importance_ref
    from tests.test_marginals_host import rule_slab
    spec, d, W, gs = smp.spec, smp.spec.d, int(smp.n_walkers), int(smp.group_size)
    funcs = list(getattr(spec, "derived_functions", None) or [])
    sampled, names = list(spec.sampled), list(spec.sampled) + [f.name for f in funcs]
    ix, shift = names.index, np.asarray(smp._shift, dtype=np.float64)
    snaps = snapshots_of(smp)
    counts = [int(iv[0]) for iv in smp._intervals] + [int(smp._snaps_in_interval)]
    start = len(snaps) - sum(counts)
    assert start == smp._dropped_snapshots >= 0
    at = np.cumsum([start] + counts)
    spans = [snaps[at[i]:at[i + 1]] for i in range(len(counts))]
    accs = {p.name: p for p in smp._products}
    out = {}
    # the derived columns of every stored row are the functions of its own x, formed again here
    for s in snaps:
        rows = {n: s["x"][:, i] for i, n in enumerate(sampled)}
        for j, f in enumerate(funcs):
            rows[f.name] = f.function(*[rows[a] for a in f.args])
            same_bits(s["z"][:, j], np.asarray(rows[f.name], dtype=np.float64), ("stored", f.name, s["step"]))
    if "derived" in accs and accs["derived"].live:
        a = accs["derived"]
        rule = derived_ref.Rule(W, gs, len(funcs), [sampled.index(n) for n in a.cross], a.shift, shift)
        out["derived"] = []
        for span in spans:
            for s in span:
                rule.accumulate(s["x"], s["z"])
            out["derived"].append(rule.request())
    if "marginals" in accs:
        cfg = accs["marginals"].cfg
        lo, hi = np.full(len(names), np.nan), np.full(len(names), np.nan)
        for n, (a_, b_) in cfg["resolved"].items():
            lo[ix(n)], hi[ix(n)] = a_, b_
        args = ([ix(n) for n in cfg["params"]], cfg["bins"], [(ix(a_), ix(b_)) for a_, b_ in cfg["pairs"]], cfg["bins2d"], lo, hi)
        slabs = []
        for span in spans:
            slab = np.zeros(cfg["n_counters"], np.uint64)
            for s in span:
                slab += rule_slab(np.column_stack((s["x"], s["z"])), *args)
            slabs.append(slab)
        out["marginals"] = slabs[:-1] + [(slabs[-1], counts[-1])]
    if "autocorr" in accs:
        cfg = accs["autocorr"].cfg
        rule = autocorr_ref.Rule([sampled.index(n) for n in cfg["params"]], cfg["lags"], gs, shift)
        for s in snaps[:start]:       # (what precedes the window fills the ring)
            rule.accumulate(s["x"])
        rule.read_and_zero()
        out["autocorr"] = []
        for span in spans:
            for s in span:
                rule.accumulate(s["x"])
            out["autocorr"].append(rule.read_and_zero())
    if "bestfit" in accs:
        cfg = accs["bestfit"].cfg
        lo, hi = np.full(d, np.nan), np.full(d, np.nan)
        for n, (a_, b_) in cfg["resolved"].items():
            lo[sampled.index(n)], hi[sampled.index(n)] = a_, b_
        rule = bestfit_ref.Rule(d, [sampled.index(n) for n in cfg["params"]], cfg["bins"], lo, hi, cfg["quantity"],
                                walker_offset=smp.rank * W)
        parts = []
        for span in spans:
            for s in span:
                rule.accumulate(s)
            parts.append(rule.read_and_empty())
        out["bestfit"] = [p[:2] for p in parts[:-1]] + [parts[-1]]
    if "evidence" in accs:
        a = accs["evidence"]
        assert a.cfg["every"] == 1
        out["evidence"] = []
        for i, (span, held) in enumerate(zip(spans, list(a.ivs) + [a.open])):
            rule = evidence_ref.Rule(d, W, gs, a.r2)
            rule.active = np.array(held["active"], dtype=np.float64)
            for s in span:
                rule.accumulate(s["x"], s["logpost"])
            want = rule.request(False)
            out["evidence"].append({k: want[k] for k in ("sums", "counts", "clamped", "n")})
            if i and at[i] > 0:
                # c: the one before, or -- an ellipsoid staged meanwhile -- the largest logpost of the state
                # the closing request saw, which is the last snapshot of the interval before
                prev = (list(a.ivs) + [a.open])[i - 1]["active"]
                assert held["active"][-1] in (prev[-1], evidence_ref.rule_c(snaps[at[i] - 1]["logpost"])), i
    if "importance" in accs:
        a = accs["importance"]
        rule = importance_ref.Rule(d, W, gs, a.cov)
        out["importance"] = []
        for span in spans:
            for s in span:
                rows = {n: s["x"][:, i] for i, n in enumerate(sampled)}
                delta = np.stack([np.asarray(alt["function"].function(*[rows[k] for k in alt["function"].args]),
                                             dtype=np.float64) for alt in a.cfg])
                rule.accumulate(s["x"], delta, shift)
            want = rule.request(True)
            if want["n_acc"] == 0:    # (the c of an interval without an accumulation is not part of the rule)
                want.pop("c")
            out["importance"].append(want)
    return out


def same_as_replayed(smp):
    """Every live product of `smp`, interval by interval, equals the rules over its stored rows."""
    smp.products()
    held, want = held_parts(smp), replay(smp)
    assert set(held) == set(want), (sorted(held), sorted(want))
    for name in want:
        assert len(held[name]) == len(want[name]) == len(smp._intervals) + 1, (name, len(held[name]), len(want[name]))
        same_bits(held[name], want[name], (name,))
    return {name: len(parts) for name, parts in want.items()}

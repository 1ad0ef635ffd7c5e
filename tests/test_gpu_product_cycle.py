"""The life cycle the six device products share (configure / accumulate / request / fetch / set), on
the MI355X through the C ABI: one request in flight at most, a closing request empties the interval, a
`set` of what was fetched comes back bit for bit, and a slab configured again is a new, zeroed slab of
the new size.  What each product sums is tested in its own test_gpu_<product>.py; here only what they
have in common, at the smallest shape with two groups (d = 2, 128 walkers in groups of 64, one
accumulation, the one-likelihood target).  Every case but one asserts what the library did before the
cycle was written once (csrc/readout.h); the one: importance configured off and on again read back the
previous slab's n and c while slabs were zeroed on the null stream, which the engine's stream does not
wait for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (before the first Engine: one HIP runtime for both)

from cobaya_amd.engine import ERR_STATE, Engine, EngineError  # noqa: E402
from cobaya_amd.importance import n_chains  # noqa: E402

D, W, GS = 2, 128, 64
LO, HI = [-50.0] * D, [50.0] * D


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


class _Product:
    """One product through the engine's wrappers.  `configure(eng, k)`: at size k (0 or 1: two
    different sizes); `off(eng)`; `ready(eng)`: what an accumulation needs beyond the state;
    `slab(part)`: the arrays of a read-out that lie in the slab, `beside(part)`: what travels with
    them, `n(part)`: its accumulations; `n_words(k)`: the words a slab of size k reads out as."""
    request_args = ()

    def request(self, eng):
        getattr(eng, "request_" + self.name)(*self.request_args)

    def fetch(self, eng):
        return getattr(eng, "fetch_" + self.name)()

    def accumulate(self, eng):
        getattr(eng, "accumulate_" + self.name)()

    def ready(self, eng):
        pass

    def set(self, eng, part):
        f = getattr(eng, self.name + "_set")
        f(*part) if isinstance(part, tuple) else f(part)

    def beside(self, part):
        return []

    def zeroed(self, part):
        return not any(np.any(w) for w in self.slab(part) + self.beside(part))

    def emptied(self, part, before):
        return self.zeroed(part)

    def same(self, a, b):
        return self.n(a) == self.n(b) and all(
            np.array_equal(_bits(x), _bits(y))
            for x, y in zip(self.slab(a) + self.beside(a), self.slab(b) + self.beside(b)))


class _Marginals(_Product):
    name, bins = "marginals", ((8, 4), (5, 3))

    def configure(self, eng, k):
        eng.configure_marginals([0, 1], self.bins[k][0], [(0, 1)], self.bins[k][1], LO, HI)

    def off(self, eng):
        eng.configure_marginals()

    def slab(self, part):
        return [part[0]]

    def n(self, part):
        return part[1]

    def n_words(self, k):
        b1, b2 = self.bins[k]
        return 2 * (b1 + 2) + b2 * b2 + 1


class _AutoCorr(_Product):
    name, lags = "autocorr", (3, 5)

    def configure(self, eng, k):
        eng.configure_autocorr([0, 1], self.lags[k])

    def off(self, eng):
        eng.configure_autocorr()

    def slab(self, part):
        return [part[0]]

    def beside(self, part):   # (the pairs per lag are counted on the host)
        return [part[1]]

    def n(self, part):        # (the one accumulation held lag 0 alone)
        return int(part[1][0])

    def n_words(self, k):
        return 3 * (self.lags[k] + 1) * D


class _BestFit(_Product):
    name, bins = "bestfit", (8, 5)

    def configure(self, eng, k):
        eng.configure_bestfit([0, 1], self.bins[k], LO, HI)

    def off(self, eng):       # (bestfit has no "off": without dims it keeps its two records)
        eng.configure_bestfit()

    def slab(self, part):
        return [part[0], part[1]]

    def n(self, part):
        return part[2]

    def n_words(self, k):
        return D * self.bins[k] + 2 * (6 + D)


class _Evidence(_Product):
    name, request_args, radii = "evidence", (True,), ([2.0, 4.0], [1.0, 2.0, 6.0])

    def configure(self, eng, k):
        eng.configure_evidence(self.radii[k])

    def off(self, eng):
        eng.configure_evidence()

    def ready(self, eng):
        eng.evidence_set_ellipsoid(np.zeros(D), np.eye(D))

    def set(self, eng, p):
        eng.evidence_set(p["sums"], p["counts"], p["clamped"], p["n"], p["active"], p["staged"])

    def slab(self, p):        # (c, the slab's last word, travels at the end of `active`)
        return [p["sums"], p["counts"], np.array([p["clamped"]], np.uint64)]

    def beside(self, p):
        return [np.zeros(0) if p[k] is None else p[k] for k in ("active", "staged")]

    def n(self, p):
        return p["n"]

    def n_words(self, k):
        return 2 * (W // GS) * len(self.radii[k]) + 1

    def emptied(self, p, before):   # (c stays: it belongs to the ellipsoid, not to the interval)
        return (not any(np.any(w) for w in self.slab(p)) and p["staged"] is None
                and np.array_equal(_bits(p["active"]), _bits(before["active"])) and p["active"][-1] != 0.0)


class _Derived(_Product):
    name, shape = "derived", ((2, [0, 1]), (3, [0]))

    def configure(self, eng, k):
        m, cross = self.shape[k]
        eng.configure_derived(m, cross, np.zeros(m))

    def off(self, eng):
        eng.configure_derived(0)

    def ready(self, eng):
        eng.derived_set_values(np.random.default_rng(5).standard_normal((W, eng.n_derived)))

    def slab(self, p):
        return [np.array([p["N"]], np.uint64)] + [p[k] for k in ("A", "B", "C", "X", "V", "bad", "min", "max")]

    def n(self, p):
        return p["n"]

    def n_words(self, k):     # (fetch hands out B as its lower triangle)
        m, nc = self.shape[k][0], len(self.shape[k][1])
        return 1 + m + m * (m + 1) // 2 + m * nc + 2 * nc + 3 * m

    def zeroed(self, p):      # (the minimum and the maximum of nothing are NaN)
        return (not any(np.any(w) for w in self.slab(p)[:-2]) and np.all(np.isnan(p["min"]))
                and np.all(np.isnan(p["max"])))


class _Importance(_Product):
    name, request_args, cov = "importance", (True,), ([True, False], [True, True, False])

    def configure(self, eng, k):
        eng.configure_importance(self.cov[k])
        if k:
            eng.importance_set_group_size(W)

    def off(self, eng):
        eng.configure_importance()

    def accumulate(self, eng):
        _, delta, stream = eng.importance_row_views()
        with torch.cuda.stream(stream):
            delta.copy_(torch.from_numpy(np.random.default_rng(6).uniform(-3.0, 0.0, tuple(delta.shape))))
        eng.accumulate_importance(delta)

    def slab(self, p):
        return [p["sums"], p["n"], p["counters"], p["c"]]

    def n(self, p):
        return p["n_acc"]

    def n_words(self, k):     # per alternative: the chains and n of every group, 3 counters, c
        G = 1 if k else W // GS
        return sum(G * (n_chains(D, c) + 1) + 4 for c in self.cov[k])


PRODUCTS = [_Marginals(), _AutoCorr(), _BestFit(), _Evidence(), _Derived(), _Importance()]
each_product = pytest.mark.parametrize("P", PRODUCTS, ids=[p.name for p in PRODUCTS])


def _accumulated(P, k=0):
    """An engine with product P configured at size k and one accumulation in its slab."""
    eng = Engine(D, W, group_size=GS, device=0, seed=3)
    eng.set_prior([0] * D, LO, HI)
    eng.set_target_one()
    eng.set_proposal_cov(0.01 * np.eye(D))
    eng.set_state(np.random.default_rng(4).standard_normal((W, D)))
    P.configure(eng, k)
    P.ready(eng)
    P.accumulate(eng)
    return eng


def _read(P, eng):
    P.request(eng)
    return P.fetch(eng)


def _refused(call, *args):
    with pytest.raises(EngineError) as e:
        call(*args)
    assert e.value.code == ERR_STATE and "pending" in str(e.value), str(e.value)


def _size(P, part):
    return sum(np.asarray(w).size for w in P.slab(part))


@each_product
def test_one_request_is_in_flight_at_most(P):
    eng = _accumulated(P)
    _refused(P.fetch, eng)                  # nothing requested
    P.request(eng)
    _refused(P.request, eng)                # a second request
    part = P.fetch(eng)
    assert P.n(part) == 1
    P.request(eng)
    _refused(P.set, eng, part)              # set while pending
    P.fetch(eng)
    _refused(P.fetch, eng)                  # fetched: nothing is pending any more
    eng.close()


@each_product
def test_a_request_empties_the_interval_and_set_restores_it_bit_for_bit(P):
    eng = _accumulated(P)
    part = _read(P, eng)
    assert P.n(part) == 1 and not P.zeroed(part)
    empty = _read(P, eng)
    assert P.n(empty) == 0 and P.emptied(empty, part)
    if P.name == "autocorr":                # the ring is kept: it still holds the one snapshot
        assert eng.autocorr_layout()["held"] == 1
    P.set(eng, part)
    assert P.same(_read(P, eng), part)
    eng.close()


@each_product
def test_configuring_again_gives_a_new_zeroed_slab_of_the_new_size(P):
    eng = _accumulated(P)
    P.off(eng)
    P.configure(eng, 0)
    fresh = _read(P, eng)
    assert P.n(fresh) == 0 and P.zeroed(fresh) and _size(P, fresh) == P.n_words(0)
    P.ready(eng)
    P.accumulate(eng)
    P.configure(eng, 1)                     # another size, straight over a slab in use
    other = _read(P, eng)
    assert P.n(other) == 0 and P.zeroed(other) and _size(P, other) == P.n_words(1)
    P.ready(eng)
    P.accumulate(eng)
    other = _read(P, eng)
    assert P.n(other) == 1 and not P.zeroed(other) and _size(P, other) == P.n_words(1)
    eng.close()


@each_product
def test_the_engine_closes_with_a_request_pending(P):
    eng = _accumulated(P)
    P.request(eng)
    eng.close()

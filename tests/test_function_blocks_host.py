"""Several `device_function` likelihoods over parameter blocks, the parts that need no device:
the model (parsing, refusals by name, blocks by footprint against golden G15, the due table) and
the reference of the step (tests/function_blocks_ref.py) tied to tests/function_ref.py."""
import json
import os

import numpy as np
import pytest

from cobaya_amd.model import ProblemSpec, UnsupportedModel
from tests import function_blocks_ref as FB
from tests import function_ref as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def quad(p):   # a batched device function of any number of inputs
    return -0.5 * (p ** 2).sum(1)


def _info(likes, sampled="abcef", **par):
    return {"likelihood": {n: {"class": "device_function", "function": quad, "input_params": list(i), **o}
                           for n, (i, o) in likes.items()},
            "params": {p: {"prior": {"min": -3, "max": 3}, "ref": 0, "proposal": 1, **par.get(p, {})}
                       for p in sampled}}


THREE = {"slow": ("ab", {}), "fast": ("bce", {}), "mid": ("af", {})}


# ------------------------------------------------------------------------------ 1. the model
def test_several_functions_parse_with_their_own_inputs():
    spec = ProblemSpec.from_info(_info({"slow": ("ba", {"speed": 1}), "fast": ("bce", {"speed": 50}),
                                        "mid": ("af", {"speed": 7})}))
    assert spec.like_kind == "device_function" and spec.n_modes == 0 and spec.function is None
    assert [(n, idx) for n, _, idx in spec.functions] == [("slow", [1, 0]), ("fast", [1, 2, 3]),
                                                          ("mid", [0, 4])]
    # a prefix routes as for every other class
    info = _info({"x": ("", {}), "y": ("", {})}, sampled=["x_1", "x_2", "y_1"])
    for n in "xy":
        del info["likelihood"][n]["input_params"]
        info["likelihood"][n]["input_params_prefix"] = n + "_"
    assert [idx for _, _, idx in ProblemSpec.from_info(info).functions] == [[0, 1], [2]]
    # ... and a single device_function is what it was: all parameters, one component, no list
    one = ProblemSpec.from_info(_info({"only": ("abcef", {})}))
    assert one.functions == [] and one.function is quad


def test_param_blocking_equals_g15():
    with open(os.path.join(GOLDEN, "g15_function_blocking.json")) as f:
        g = json.load(f)
    assert len(g["cases"]) == 9
    for case in g["cases"]:
        likes = {n: ("".join(g["inputs"][n]), {"speed": s})
                 for n, s in zip(g["likelihoods"], case["speeds"])}
        spec = ProblemSpec.from_info(_info(likes, sampled=g["sampled"]))
        blocks, factors = spec.param_blocking(oversample_power=case["oversample_power"])
        assert blocks == case["blocks"] and factors == case["factors"], case
    # the figures the issue quotes
    case = next(c for c in g["cases"] if c["speeds"] == [1, 50, 7] and c["oversample_power"] == 1.0)
    assert case["blocks"] == [["a"], ["b"], ["f"], ["c", "e"]] and case["factors"] == [1, 1, 7, 57]


def test_due_tables_of_a_crafted_three_block_layout():
    """Blocks (a) | (b, f) | (c, e), slow -> fast.  slow(a, b) ends in block 1, mid(a, f) in block 1,
    fast(b, c, e) in block 2, top(a) in block 0: a slot of block b calls what reaches b or beyond."""
    likes = {**THREE, "top": ("a", {})}
    spec = ProblemSpec.from_info(_info(likes))
    blocks = [["a"], ["b", "f"], ["c", "e"]]
    assert spec.function_due(blocks) == [["slow", "fast", "mid", "top"], ["slow", "fast", "mid"], ["fast"]]
    idx = [[spec.sampled.index(p) for p in b] for b in blocks]
    assert FB.due_table(idx, [i for _, _, i in spec.functions]) == [[0, 1, 2, 3], [0, 1, 2], [1]]
    # one block: every function at every slot
    assert spec.function_due([list("abcef")]) == [["slow", "fast", "mid", "top"]]
    # the slowest block alone holds an input of everything: the fastest block calls one function
    assert spec.function_due([["c", "e"], ["b"], ["f"], ["a"]])[-1] == ["slow", "mid", "top"]


def test_refusals_by_name():
    nine = {"f%d" % k: ("abcef", {}) for k in range(9)}
    with pytest.raises(UnsupportedModel, match="9 device_function likelihoods.*at most 8"):
        ProblemSpec.from_info(_info(nine))
    with pytest.raises(UnsupportedModel, match=r"\['f'\] feed no likelihood"):
        ProblemSpec.from_info(_info({"slow": ("ab", {}), "fast": ("bce", {})}))
    info = _info(THREE)
    info["likelihood"]["other"] = {"class": "one"}       # a foreign class beside the functions
    with pytest.raises(UnsupportedModel, match="must be the only likelihood"):
        ProblemSpec.from_info(info)
    info = _info(THREE)
    info["likelihood"]["g"] = {"class": "gaussian", "mean": [0], "cov": [[1]], "input_params": ["a"]}
    with pytest.raises(UnsupportedModel, match="must be the only likelihood"):
        ProblemSpec.from_info(info)
    with pytest.raises(UnsupportedModel, match="its inputs must be one or more of the sampled"):
        ProblemSpec.from_info(_info({"slow": ("az", {}), "fast": ("bcef", {})}))
    with pytest.raises(UnsupportedModel, match="its inputs must be one or more of the sampled"):
        ProblemSpec.from_info(_info({"slow": ("aab", {}), "fast": ("bcef", {})}))


def test_sampler_refuses_by_name_and_accepts_blocks_before_the_engine():
    from cobaya_amd.sampler import LoggedError, MCMCHip

    class Stop(Exception):
        pass

    def no_engine(*a, **k):
        raise Stop()
    no_engine.max_dim = lambda: 256

    class NoEngine(MCMCHip):
        _engine_factory = staticmethod(no_engine)

    base = {"seed": 1, "n_walkers": 128, "group_size": 64, "max_samples": 100}
    blocking = [[1, ["a"]], [1, ["b"]], [7, ["f"]], [57, ["c", "e"]]]

    def refused(match, info=None, **opts):
        with pytest.raises(LoggedError, match=match):
            NoEngine({**base, **opts}, ProblemSpec.from_info(info or _info(THREE)))

    refused("drag: True is not served", drag=True, blocking=blocking)
    refused("periodic parameters are not served", info=_info(THREE, b={"periodic": True}))
    refused("emit: chains is not served", emit="chains")
    refused("evaluation: incremental is not served", evaluation="incremental")
    # blocks and oversampling pass every check: the sampler goes on to create the engine
    for opts in ({"blocking": blocking}, {"oversample_power": 1.0}, {}):
        with pytest.raises(Stop):
            NoEngine({**base, **opts}, ProblemSpec.from_info(_info(
                {"slow": ("ab", {"speed": 1}), "fast": ("bce", {"speed": 50}), "mid": ("af", {"speed": 7})})))


def test_component_loglikes_call_the_functions_on_their_inputs():
    spec = ProblemSpec.from_info(_info(THREE))
    x = np.random.default_rng(3).uniform(-1, 1, (7, 5))
    got = spec.component_loglikes(x)
    for k, (_, _, idx) in enumerate(spec.functions):
        np.testing.assert_allclose(got[:, k], -0.5 * (x[:, idx] ** 2).sum(1), rtol=1e-15)


# ------------------------------------------------------------------------------ 2. the reference
def _problem(d, blocks, over, rng, gs=64, seed=11, temperature=1.5):
    kinds = np.array([1 if i % 3 == 1 else 0 for i in range(d)], np.int32)
    a = np.where(kinds == 1, 0.5, 0.0)
    b = np.where(kinds == 1, 0.3, 1.0)
    A = rng.standard_normal((d, d)) / np.sqrt(d)
    cov = 0.01 * (A @ A.T + np.eye(d))
    order = [i for blk in blocks for i in blk] if blocks else list(range(d))
    T = np.linalg.cholesky(cov[np.ix_(order, order)]) * (2.4 / np.sqrt(d))
    return FB.problem(d, kinds, a, b, T, blocks=blocks, oversampling=over, group_size=gs, seed=seed,
                      temperature=temperature), cov


def _bowl(centre):
    return lambda p: -0.5 * (((p - centre) / 0.2) ** 2).sum(1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _start(d, W, cov, rng):
    x0 = np.clip(0.5 + 0.3 * rng.standard_normal((W, d)) * np.sqrt(np.diag(cov)), 0.01, 0.99)
    x0[::4, 0] = 0.001
    return x0


@pytest.mark.parametrize("d", [1, 2, 5, 40])
def test_one_block_one_function_equals_function_ref(d):
    """One block with factor 1 and one function of all parameters: the blocked reference, taking
    its directions from orc_basis_blocked through the shared schedule, IS FunctionRef."""
    rng = np.random.default_rng(200 + d)
    prob_b, cov = _problem(d, [list(range(d))], [1], rng)
    prob_1 = FR.problem(d, prob_b.kind, np.where(prob_b.kind == 1, 0.5, 0.0), np.where(prob_b.kind == 1, 0.3, 1.0),
                        prob_b.T, group_size=64, seed=11, temperature=1.5)
    W, f = 128, _bowl(0.45)
    x0 = _start(d, W, cov, rng)
    new = FB.FunctionBlocksRef(prob_b, x0, [list(range(d))], [f(x0)], blocks=[list(range(d))], burn_in=3)
    old = FR.FunctionRef(prob_1, x0, f(x0), burn_in=3)
    n = 2 * d + 3
    new.run(n, [f])
    old.run(n, f)
    assert np.array_equal(_bits(new.x), _bits(old.x)) and old.n_accept.sum() > 0
    for k in ("logpost", "logprior", "loglike"):
        assert np.array_equal(_bits(getattr(new, k)), _bits(getattr(old, k))), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(getattr(new, k), getattr(old, k)), k
    assert np.array_equal(_bits(new.ll_c[0]), _bits(old.loglike)) and new.calls == [n]


def test_carrying_equals_calling_every_function_at_every_step():
    """Three blocks 2 + 1 + 2 with factors 1, 2, 3, overlapping footprints, a one-parameter block, two
    groups (the second one's own schedule differs from the shared one): the state after 2 L + 3 steps
    with carried values equals, bit for bit, the state when every function is called at every step."""
    d, W = 5, 128
    blocks, over = [[3, 0], [2], [4, 1]], [1, 2, 3]
    inputs = [[0, 3], [3, 2, 0], [1, 4, 2]]            # ends in block 0, block 1, block 2
    fns = [_bowl(0.4), _bowl(0.5), _bowl(0.45)]
    rng = np.random.default_rng(77)
    prob, cov = _problem(d, blocks, over, rng)
    L = prob.cycle_length()
    assert L == 2 + 2 + 6
    assert any(not np.array_equal(prob.schedule(0, c)[0], prob.schedule(1, c)[0]) for c in range(3))
    x0 = _start(d, W, cov, rng)
    ll0 = [f(x0[:, idx]) for f, idx in zip(fns, inputs)]
    a = FB.FunctionBlocksRef(prob, x0, inputs, ll0, blocks=blocks, burn_in=3)
    b = FB.FunctionBlocksRef(prob, x0, inputs, ll0, blocks=blocks, burn_in=3)
    n = 2 * L + 3
    a.run(n, fns, carry=True)
    b.run(n, fns, carry=False)
    assert a.n_accept.sum() > 0 and (a.weight > 1).any()
    for k in ("x", "logpost", "logprior", "loglike", "ll_c"):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    for k in ("weight", "prior_rej", "burn_left", "n_accept"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    # the calls: function c at the slots of the blocks up to its last one
    per_cycle = [2, 2 + 2, 2 + 2 + 6]
    assert b.calls == [n] * 3
    assert all(a.calls[c] <= 3 * per_cycle[c] and a.calls[c] >= 2 * per_cycle[c] for c in range(3))
    assert a.calls[2] == n and a.calls[0] < a.calls[1] < n

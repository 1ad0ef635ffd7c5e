#!/usr/bin/env python3
"""Generate golden G15 (tests/golden/g15_function_blocking.json) by IMPORTING the Python reference:
the blocks and oversampling factors `Model.get_param_blocking_for_sampler` (model.py:1340-1467)
gives for three EXTERNAL likelihood functions with OVERLAPPING inputs -- slow(a, b), fast(b, c, e),
mid(a, f) -- at the speeds [1, 50, 7], [30, 2, 500], [5, 5, 5] and oversample_power 0, 0.4 and 1.
Parameters are grouped by footprint (the set of likelihoods they feed).

Like tests/golden/make_golden.py this runs only where the reference tree is mounted and stores
decisions only: names, speeds, blocks and factors.

    python tests/golden/make_golden_g15.py
"""
import json
import logging
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("COBAYA_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_getdist_stub"), REF]

from cobaya.model import get_model  # noqa: E402

logging.disable(logging.CRITICAL)

NAMES = ["slow", "fast", "mid"]
INPUTS = {"slow": ["a", "b"], "fast": ["b", "c", "e"], "mid": ["a", "f"]}
SAMPLED = ["a", "b", "c", "e", "f"]


def slow(a, b):
    return -0.5 * (a ** 2 + b ** 2)


def fast(b, c, e):
    return -0.5 * (b ** 2 + c ** 2 + e ** 2)


def mid(a, f):
    return -0.5 * (a ** 2 + f ** 2)


def main():
    cases = []
    for speeds in ([1, 50, 7], [30, 2, 500], [5, 5, 5]):
        for power in (0.0, 0.4, 1.0):
            info = {"likelihood": {n: {"external": fn, "speed": s}
                                   for n, fn, s in zip(NAMES, (slow, fast, mid), speeds)},
                    "params": {p: {"prior": {"min": -3, "max": 3}} for p in SAMPLED}}
            model = get_model(info)
            blocks, factors = model.get_param_blocking_for_sampler(oversample_power=power)
            cases.append({"speeds": speeds, "oversample_power": power,
                          "blocks": [list(b) for b in blocks], "factors": [int(f) for f in factors]})
    path = os.path.join(HERE, "g15_function_blocking.json")
    with open(path, "w") as f:
        json.dump({"likelihoods": NAMES, "inputs": INPUTS, "sampled": SAMPLED, "cases": cases}, f, indent=1)
    print("wrote", os.path.relpath(path), len(cases), "cases")
    for c in cases:
        print(c)


if __name__ == "__main__":
    main()

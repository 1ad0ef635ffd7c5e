#!/usr/bin/env python3
"""Generate golden G14 (tests/golden/g14_external_function.npz) by IMPORTING the Python reference:
`Model.logposterior` of a model whose likelihood is an EXTERNAL PYTHON FUNCTION
(LikelihoodExternalFunction, cobaya/likelihood.py:150-255) -- the banana of the README example --
with mixed uniform / normal priors, at about 50 points, some of them outside the prior support.

Like tests/golden/make_golden.py this runs only where the reference tree is mounted (it never
travels to the GPU box) and stores numbers only: the points, the priors' constants, and the
log-prior / log-likelihood the reference returned.

    python tests/golden/make_golden_g14.py
"""
import logging
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("COBAYA_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_getdist_stub"), REF]

import numpy as np  # noqa: E402

from cobaya.model import get_model  # noqa: E402

logging.disable(logging.CRITICAL)

BETA, S = 0.5, 0.5


def banana(a, b, c):
    return -0.5 * (a ** 2 + ((b - BETA * a ** 2) / S) ** 2) - 0.5 * ((c - 0.25) / 0.75) ** 2


def main():
    # kinds: 0 uniform [a, b], 1 normal(loc = a, scale = b)
    kinds = np.array([0, 1, 0], dtype=np.int32)
    pa = np.array([-8.0, 0.4, -2.0])
    pb = np.array([8.0, 3.0, 3.0])
    info = {"likelihood": {"banana": banana},
            "params": {"a": {"prior": {"min": pa[0], "max": pb[0]}},
                       "b": {"prior": {"dist": "norm", "loc": pa[1], "scale": pb[1]}},
                       "c": {"prior": {"min": pa[2], "max": pb[2]}}}}
    model = get_model(info)
    rng = np.random.default_rng(14)
    pts = np.column_stack([rng.uniform(-8, 8, 52), rng.normal(0.4, 3.0, 52), rng.uniform(-2, 3, 52)])
    # outside the support: beyond one bound, beyond both parameters' bounds, exactly ON a bound
    pts[5, 0] = 8.5
    pts[11, 2] = -2.25
    pts[17, 0], pts[17, 2] = -9.0, 3.5
    pts[23, 2] = 3.0000001
    pts[29, 0] = -8.0          # on the bound: inside (prior.py:733-763, <= and >=)
    pts[31, 2] = 3.0
    logprior, loglike = np.empty(len(pts)), np.empty(len(pts))
    for k, p in enumerate(pts):
        r = model.logposterior(p)
        logprior[k] = np.sum(r.logpriors)
        # (outside the support the reference skips the likelihood, model.py:650-653: no loglikes)
        loglike[k] = np.sum(r.loglikes) if len(r.loglikes) else -np.inf
    assert np.sum(np.isinf(logprior)) >= 4 and np.sum(np.isfinite(logprior)) >= 40
    path = os.path.join(HERE, "g14_external_function.npz")
    np.savez_compressed(path, points=pts, kinds=kinds, a=pa, b=pb, beta=BETA, s=S,
                        c_loc=0.25, c_scale=0.75, logprior=logprior, loglike=loglike)
    print("wrote", os.path.relpath(path), os.path.getsize(path), "bytes")
    print(logprior[[5, 11, 17, 23, 29, 31]], loglike[[5, 11, 17, 23, 29, 31]])


if __name__ == "__main__":
    main()

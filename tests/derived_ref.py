"""THE REFERENCE of the derived parameters' sums (tests/test_derived_host.py, tests/test_gpu_derived.py):
the rule of DESIGN.md section 2 ("Derived") in numpy.  Every sum is compared bit for bit.

    a_j = z_j - shift_j,   b_c = x_{cross[c]} - xshift_{cross[c]}   (float64, one rounding each)
    a walker is USED iff all m of its derived values are finite
    per group g of group_size walkers, over its used walkers in ascending order, every sum ONE chain
    from +0.0 with the product and the addition as separate roundings:
        N[g]            an integer
        A[g][j]       = sum a_j
        B[g][j][k]    = sum a_j * a_k   (k <= j; packed: (j, k) at j (j + 1) / 2 + k)
        C[g][j][c]    = sum a_j * b_c
        X[g][c]       = sum b_c,   V[g][c] = sum b_c * b_c   (the sampled parameters over the same walkers)
    the pooled accumulators add the group values in ascending g, starting from their current value
    per name, exact: bad[j] counts the non-finite values, min[j] / max[j] over the finite ones (NaN: none)
"""
import warnings

import numpy as np


def zero(m, nc):
    return {"N": 0, "A": np.zeros(m), "B": np.zeros(m * (m + 1) // 2), "C": np.zeros((m, nc)), "X": np.zeros(nc),
            "V": np.zeros(nc), "bad": np.zeros(m, np.uint64), "min": np.full(m, np.nan), "max": np.full(m, np.nan),
            "n": 0}


def group_sums(a, b, used, dtype=np.float64):
    """(N, A, B packed, C, X, V) of ONE group: chains over its walkers in ascending order from +0.0.
    `dtype`: float64 is the rule; np.longdouble restates it for the host test."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    m, nc = a.shape[1], b.shape[1]
    tj, tk = np.tril_indices(m)
    A, B, C = np.zeros(m, dtype), np.zeros(len(tj), dtype), np.zeros((m, nc), dtype)
    X, V = np.zeros(nc, dtype), np.zeros(nc, dtype)
    N = 0
    with np.errstate(all="ignore"):
        for l in range(len(a)):
            if not used[l]:
                continue
            al, bl = a[l], b[l]
            N += 1
            A = A + al
            B = B + al[tj] * al[tk]
            C = C + al[:, None] * bl[None, :]
            X = X + bl
            V = V + bl * bl
    return N, A, B, C, X, V


class Rule:
    """The pooled accumulators of one engine (or one shard)."""

    def __init__(self, W, group_size, m, cross, shift, xshift):
        self.W, self.gs, self.m = int(W), int(group_size), int(m)
        self.cross = [int(c) for c in cross]
        self.shift = np.asarray(shift, dtype=np.float64).reshape(m)
        self.xshift = np.asarray(xshift, dtype=np.float64)
        self.acc = zero(m, len(self.cross))

    def accumulate(self, x, z):
        """x: [W, d] the state, z: [W, m] the derived values."""
        x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64).reshape(self.W, self.m)
        with np.errstate(all="ignore"):
            a = z - self.shift
            b = x[:, self.cross] - self.xshift[self.cross]
        fin = np.isfinite(z)
        used = fin.all(axis=1)
        acc = self.acc
        with np.errstate(all="ignore"):
            for g in range(self.W // self.gs):
                sl = slice(g * self.gs, (g + 1) * self.gs)
                N, A, B, C, X, V = group_sums(a[sl], b[sl], used[sl])
                acc["N"] += N
                acc["A"] = acc["A"] + A
                acc["B"] = acc["B"] + B
                acc["C"] = acc["C"] + C
                acc["X"] = acc["X"] + X
                acc["V"] = acc["V"] + V
        acc["bad"] = acc["bad"] + np.count_nonzero(~fin, axis=0).astype(np.uint64)
        zf = np.where(fin, z, np.nan)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # (a column without a finite value)
            acc["min"] = np.fmin(acc["min"], np.nanmin(zf, axis=0) if len(zf) else np.nan)
            acc["max"] = np.fmax(acc["max"], np.nanmax(zf, axis=0) if len(zf) else np.nan)
        acc["n"] += 1

    def request(self):
        """The read-out; the accumulators are zeroed."""
        out, self.acc = self.acc, zero(self.m, len(self.cross))
        return out

    def set(self, part):
        self.acc = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in part.items()}


def same(got, want):
    """A read-out of the engine against the rule's, bit for bit (min / max: -0.0 and +0.0 differ)."""
    assert (got["N"], got["n"]) == (want["N"], want["n"]), (got["N"], got["n"], want["N"], want["n"])
    for k in ("A", "B", "C", "X", "V", "min", "max"):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        # (the payload of a NaN is not part of the rule: NaN equals NaN)
        gb, wb = g.view(np.uint64), w.view(np.uint64)
        ok = (gb == wb) | (np.isnan(g) & np.isnan(w))
        assert ok.all(), (k, g[~ok], w[~ok])
    assert np.array_equal(np.asarray(got["bad"], np.uint64), want["bad"]), (got["bad"], want["bad"])

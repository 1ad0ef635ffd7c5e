"""The reference of a function target with SEVERAL functions over parameter blocks (DESIGN.md
section 2, "Function targets with parameter blocks"), built on tests/function_ref.py,
tests/function_step_ref.c and the oracle's exports only.

The slot schedule is the one of GLOBAL group 0 (`Problem.schedule(0, cycle)`); the direction of
slot s in group g is the slot of `Problem.basis_blocked(g, cycle)` whose (block, basis, column) in
`Problem.schedule(g, cycle)` equals that of slot s in the shared schedule -- the group's own Haar
basis, taken in the shared order.  A slot of a one-parameter block carries the oracle's flag: its
variates are the RandProposer1D ones, which fn_ref_propose forms at d = 1 -- so the trial of such
a slot is formed one dimension at a time (the variates depend on (seed, walker, step) only).
Function c is due at a slot of sorted block b iff it has an input in a block >= b; the others keep
their carried ll_c."""
import ctypes as C

import numpy as np

from oracle import cbind as O
from tests import function_ref as FR

_p = FR._p


def problem(d, kinds, a, b, T, blocks=None, oversampling=None, group_size=64, seed=1, temperature=1.0,
            max_tries=None, derived=None):
    """FR.problem with the parameter blocks (lists of sampler indices, slow -> fast); T: the
    transform of the covariance in sorted order (Engine.get_proposal_transform)."""
    return O.Problem(d, kinds, a, b, T=T, group_size=group_size, seed=seed, temperature=temperature,
                     max_tries=max_tries, derived=derived, blocks=blocks, oversampling=oversampling)


def due_table(blocks, inputs):
    """due[b] = the functions called at a slot of sorted block b: those with an input in a block >= b."""
    block_of = {i: b for b, blk in enumerate(blocks) for i in blk}
    last = [max(block_of[i] for i in idx) for idx in inputs]
    return [[c for c in range(len(inputs)) if last[c] >= b] for b in range(len(blocks))]


def total(comps):
    """The sum over the functions ascending, left to right."""
    ll = np.array(comps[0], dtype=np.float64)
    for v in comps[1:]:
        ll = ll + v
    return ll


class FunctionBlocksRef(FR.FunctionRef):
    """Walker state of such a target: FunctionRef + the carried ll_c[n_fn][W]."""

    def __init__(self, prob, x0, inputs, ll_c0, blocks=None, burn_in=0, walker0=0):
        self.inputs = [list(idx) for idx in inputs]
        self.blocks = [list(b) for b in blocks] if blocks is not None else None
        self.ll_c = np.array(ll_c0, dtype=np.float64)
        super().__init__(prob, x0, total(self.ll_c), burn_in=burn_in, walker0=walker0)
        assert self.ll_c.shape == (len(self.inputs), self.W)
        self.ll_c[:, np.isinf(self.logprior)] = -np.inf
        self.due = list(range(len(self.inputs)))
        self._due = due_table(self.blocks, self.inputs) if self.blocks is not None else None
        self.calls = [0] * len(self.inputs)

    def slot(self):
        """(cycle, slot) of the current step."""
        return divmod(self.step, self.p.cycle_length() if self.blocks is not None else self.d)

    def _slot_columns(self):
        """(v[G][d], flag, block) of the current slot in the shared schedule."""
        cyc, s = self.slot()
        cyc &= 0xFFFFFFFF   # (the cycle index is kept modulo 2^32: oracle, orc_run)
        gs = self.p.group_size
        g0, G = self.walker0 // gs, self.W // gs
        if cyc != self._cycle:
            blk0, bas0, col0 = self.p.schedule(0, cyc)
            V, F = [], []
            for g in range(g0, g0 + G):
                blk, bas, col = self.p.schedule(g, cyc)
                own = {(int(blk[k]), int(bas[k]), int(col[k])): k for k in range(len(blk))}
                order = [own[(int(blk0[k]), int(bas0[k]), int(col0[k]))] for k in range(len(blk0))]
                Vg, fg = self.p.basis_blocked(g, cyc)
                V.append(Vg[order])
                F.append(fg[order])
            self._V, self._F, self._blk0, self._cycle = np.array(V), np.array(F), blk0.copy(), cyc
        flags = self._F[:, s]
        assert np.all(flags == flags[0])
        return np.ascontiguousarray(self._V[:, s, :]), int(flags[0]), int(self._blk0[s])

    def propose(self):
        """The trial [W][d] of the current slot; self.due: the functions to call for it."""
        if self.blocks is None:
            self.due = list(range(len(self.inputs)))
            return super().propose()
        v, flag, b = self._slot_columns()
        self.due = self._due[b]
        d, W, gs = self.d, self.W, self.p.group_size
        args = (C.c_int(W), C.c_int(gs), C.c_uint32(self.walker0), C.c_uint64(self.p.seed),
                C.c_uint64(self.step))
        if flag and d > 1:
            for i in range(d):
                vi, xi = np.ascontiguousarray(v[:, i]), np.ascontiguousarray(self.x[:, i])
                ti = np.empty(W)
                FR.lib().fn_ref_propose(C.c_int(1), *args, _p(vi), _p(xi), _p(ti), _p(self.Ea))
                self.t[:, i] = ti
        else:
            assert bool(flag) == (d == 1)
            FR.lib().fn_ref_propose(C.c_int(d), *args, _p(v), _p(self.x), _p(self.t), _p(self.Ea))
        self.lp_t = self.p.evaluate(self.t)[0]
        return self.t

    def gather(self, c):
        """The (W, d_c) input of function c for the current trial."""
        return np.ascontiguousarray(self.t[:, self.inputs[c]])

    def accept(self, ll_new):
        """`ll_new[c]`: what function c returned for the trial, for every c in self.due."""
        comps = [np.asarray(ll_new[c], dtype=np.float64) if c in self.due else self.ll_c[c]
                 for c in range(len(self.inputs))]
        before = self.n_accept.copy()
        acc = super().accept(total(comps))
        took = self.n_accept > before
        for c in self.due:
            self.ll_c[c][took] = comps[c][took]
            self.calls[c] += 1
        return acc

    def run(self, n_steps, fns, carry=True):
        """n_steps with host functions fns[c](inputs[n][d_c]) -> loglike[n]; carry=False: every
        function is called at every step."""
        acc = 0
        for _ in range(n_steps):
            self.propose()
            if not carry:
                self.due = list(range(len(self.inputs)))
            acc += self.accept({c: fns[c](self.gather(c)) for c in self.due})
        return acc

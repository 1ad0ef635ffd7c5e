"""Step kernels FAR OUT: the cases of tests/test_far_steps_host.py (the conditions on the cases, on
the oracle alone) and tests/test_gpu_far_steps.py (device against oracle, bit for bit) at step
indices around 2^31, 2^32 and 2^33, where the Philox counter words (step mod 2^32, step div 2^32),
the index of the paired stream (step div 2), the cycle index (step div L, kept modulo 2^32 by the
specification) and dragging's fast sub-step counter (step * n_drag) carry into their high words.
No GPU needed.

A production run reaches step 2^32 after an hour; a test gets there by `teleport`: the whole state
is read back, its step counter replaced, and written again -- on the engine through
get_full_state / set_full_state, on the oracle by assignment.  Everything in the specification is
keyed on the global step (variates, cycles, the refresh of y every 40 cycle lengths), so nothing
else moves.

Targets are `random_target` of tests/test_gpu_parity.py on the box [0, 1], a few sigma away from
the walls: this file tests indices, tests/support_cases.py the support checks."""
from collections import namedtuple

import numpy as np

P31, P32, P33 = 1 << 31, 1 << 32, 1 << 33
M32 = P32 - 1
CONTROL = 4099                    # a step index the suite covers elsewhere; no multiple of 8
LAUNCHES = (8, 30, 17)            # from B - 21: before B, across it (in mid-octet), beyond it
BEFORE = 21
ON_BOUNDARY = 24                  # second pass: one launch that BEGINS on B
NORMAL_PRIOR = (0.5, 0.3)         # (loc, scale)


def teleport(eng, st, S0, n_accept_base=None):
    """Engine `eng` and oracle state `st` (an `oracle.cbind.State`, or anything with `step` and
    `n_accept`) continue at step S0: the engine's full state -- x, log-posterior parts, weights,
    counters, the carried y, mode log-densities and thinning remainders -- is read back and written
    again with `step` = S0 (Engine.set_full_state), and `st.step` = S0.  n_accept_base: every
    walker's accept count becomes this number on both sides first.

    One carried value is re-anchored, the same way on both sides: an engine that has not stepped
    yet holds no mode log-densities (get_full_state leaves `amode` out), and its next launch forms
    them from y whatever the step -- the oracle does that at step 0 only, so here `anchor_modes`
    does it (as tests/oracle_engine.py does at a resume)."""
    fs = eng.get_full_state()
    if n_accept_base is not None:
        fs["n_accept"][:] = n_accept_base
        st.n_accept[:] = n_accept_base
    fs["step"] = np.uint64(S0)
    eng.set_full_state(fs)
    if getattr(eng, "incremental", False) and eng.carries_modes() and "amode" not in fs:
        st.anchor_modes()
    st.step = int(S0)
    return fs


# ------------------------------------------------------------------ the cases
# name: the test id; variant: what case_setup builds; inc: incremental evaluation; path: the words
# last_step_kernel() must contain; dq, mode: the template arguments step_inc_kernel must report;
# bgs: walkers per Haar basis (two lanes per walker need 128)
Case = namedtuple("Case", "name d W gs bgs K variant inc path dq mode duo")


def _c(name, d, W=128, gs=64, bgs=None, K=1, variant="", inc=False, path=(), dq=None, mode=None,
       duo=False):
    return Case(name, d, W, gs, bgs or gs, K, variant, inc, tuple(path), dq, mode, duo)


def _cases():
    inc = "step_inc_kernel"
    out = [
        # ---- every trial from scratch
        _c("scratch-d1", 1, path=["::step_kernel<false, true>"]),    # the cycle index IS the step index
        _c("scratch-d2", 2, path=["::step_kernel<false, false>"]),
        _c("scratch-d13", 13, path=["::step_kernel<false, false>"]),  # one wave per 64 walkers
        _c("scratch-d16-pair", 16, W=256, path=["step_pair_kernel"]),  # draws step s + 1 ahead
        _c("scratch-d64-mfma", 64, W=256, path=["step_mfma_kernel<false>"]),
        _c("scratch-d40-K2", 40, K=2, path=["step_general_kernel"]),
        _c("scratch-d6-own-basis", 6, variant="own", path=["::step_kernel<false, true, own basis>"]),
        _c("scratch-d8-blocked", 8, variant="blocked", path=["::step_kernel<"]),   # L = 13
        _c("scratch-d40-blocked", 40, variant="blocked", path=["step_general_kernel"]),   # L = 60
        _c("scratch-d6-drag", 6, variant="drag", path=["::drag_kernel<false>"]),
        _c("scratch-d40-drag", 40, variant="drag", path=["drag_general_kernel"]),
        # ---- incremental: step_inc_kernel
        _c("inc-d30-mode0", 30, inc=True, path=[inc], dq=8, mode=0),
        _c("inc-d30-mode1", 30, variant="bounds", inc=True, path=[inc], dq=8, mode=1),
        _c("inc-d27-mode2", 27, variant="normal", inc=True, path=[inc], dq=7, mode=2),
        _c("inc-d100", 100, inc=True, path=[inc], dq=25, mode=0),       # two waves, 32 KiB chunks
        _c("inc-d9-periodic", 9, variant="periodic", inc=True, path=[inc, "periodic"], dq=3, mode=1),
        _c("inc-d8-oned", 8, variant="oned", inc=True, path=[inc, "1-D blocks"], dq=2),
        # (incremental evaluation begins at d = 2: inc_choice.h, inc_shape_valid)
        _c("inc-d2", 2, inc=True, path=[inc], dq=1, mode=0),
        # ---- incremental: the other families
        _c("duo-d30", 30, W=256, bgs=128, inc=True, path=[inc, "two lanes"], dq=8, mode=0, duo=True),
        _c("mix-d30-K3", 30, K=3, inc=True, path=["step_inc_mix_kernel"]),
        _c("duo-mix-d24-K2", 24, W=256, bgs=128, K=2, inc=True, path=["step_duo_mix_kernel"], duo=True),
        # (five modes at d = 30 are the mixture kernel's widest instantiation; the register planes
        # begin where it ends, inc_mix_serves: K = 8 here)
        _c("mix-d30-K5", 30, K=5, inc=True, path=["step_inc_mix_kernel"]),
        _c("regs-d30-K8", 30, K=8, inc=True, path=["step_inc_regs_kernel<8, 8>"]),
        # (a periodic parameter sends a mixture to the general kernels: up to 16 modes the register
        # planes, beyond them the LDS kernel)
        _c("regs-d12-K2-periodic", 12, K=2, variant="periodic", inc=True,
           path=["step_inc_regs_kernel<3, 2, periodic>"]),
        _c("any-d6-K24", 6, K=24, inc=True, path=["step_inc_any_kernel<2>"]),
        _c("drag-inc-d6-oned", 6, variant="drag oned", inc=True, path=["drag_inc_kernel", "1-D blocks"]),
        _c("drag-inc-d40", 40, variant="drag", inc=True, path=["drag_inc_kernel"]),
    ]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# d > 128 (huge_kernels.hip): 160, and 205, where 40 d = 8200 divides 2^33 + 8 -- the refresh of y
# falls into the launch across 2^33 (the engine's refresh period is 40 d, not an option)
HUGE_DIMS = (160, 205)


def case_id(c):
    return c.name


def case_setup(c):
    """kinds, a, b, periodic, blocking of a case; blocking = None or the arguments of set_blocking
    (blocks, oversampling, drag_last_slow, drag_steps)."""
    d, v = c.d, c.variant
    a, b = np.zeros(d), np.ones(d)
    kinds = np.zeros(d, int)
    periodic = blocking = None
    if v == "bounds":                       # bounds of their own: MODE 1
        b = 1.0 + 0.25 * (np.arange(d) % 2)
    elif v == "normal":                     # about half the parameters with normal priors: MODE 2
        kinds = (np.arange(d) % 2 == 1).astype(int)
        a[kinds == 1], b[kinds == 1] = NORMAL_PRIOR
    elif v == "periodic":
        periodic = np.zeros(d, int)
        periodic[d // 2] = 1
    elif v == "oned":
        blocking = ([[3], [0], [1, 2, 4, 5, 6, 7]], [1, 1, 3], -1, 0)
    elif v == "blocked":
        blocks = [[0, 1, 2], [3, 4, 5, 6, 7]] if d == 8 else [list(range(20)), list(range(20, 40))]
        blocking = (blocks, [1, 2], -1, 0)
    elif v == "drag":
        blocks = [[0, 1], [2, 3, 4, 5]] if d == 6 else [list(range(12)), list(range(12, 40))]
        blocking = (blocks, [1, 1] if d == 6 else [1, 2], 0, 3)
    elif v == "drag oned":
        blocking = ([[0, 1], [2], [3, 4, 5]], [1, 1, 2], 0, 3)
    return kinds, a, b, periodic, blocking


def case_problem(c):
    """Everything of a case but engine and oracle: kinds, a, b, periodic, blocking, means, covs, x0."""
    from tests.test_gpu_parity import random_target
    kinds, a, b, periodic, blocking = case_setup(c)
    rng = np.random.default_rng(9000 + 7 * c.d + c.K)
    means, covs = random_target(c.d, c.K, rng)
    x0 = means[0] + rng.normal(size=(c.W, c.d)) * np.sqrt(np.diag(covs[0]))
    x0 = np.clip(x0, 1e-3, 1 - 1e-3)
    for i in np.flatnonzero(kinds == 1):
        x0[:, i] = a[i] + 0.1 * rng.normal(size=c.W) * b[i]
    return kinds, a, b, periodic, blocking, means, covs, x0


def cycle_lengths(c):
    """(L, n_drag, Lf): steps per cycle of the (slow) directions; dragging: interpolation steps per
    step and fast sub-steps per cycle of the fast directions."""
    from oracle import cbind as O
    kinds, a, b, periodic, blocking = case_setup(c)
    if blocking is None:
        return c.d, 0, 0
    blocks, over, last_slow, n_drag = blocking
    p = O.Problem(c.d, kinds.tolist(), a.tolist(), b.tolist(), blocks=blocks, oversampling=over,
                  drag_last_slow=last_slow, drag_steps=n_drag)
    if last_slow < 0:
        return p.cycle_length(0), 0, 0
    return p.cycle_length(1), n_drag, p.cycle_length(2)


def boundaries(c):
    """The step indices B a case is taken across, ascending: 2^31 and 2^32 (the counter's low word
    changes sign and carries); incremental: 2^33 (the paired stream's index step div 2 carries);
    a cycle of L steps: L 2^31 and L 2^32 (the cycle index changes sign and wraps); dragging with n
    interpolation steps: ceil(2^32 / n) and Lf 2^32 / n rounded up to a step (the fast sub-step
    counter step * n carries; the fast cycle index wraps)."""
    L, nd, Lf = cycle_lengths(c)
    out = {P31, P32}
    if c.inc:
        out.add(P33)
    out |= {L * P31, L * P32}
    if nd:
        out |= {-(-P32 // nd), -(-(Lf * P32) // nd)}
    return sorted(out)


def passes(B):
    """[(S0, launches)] of one boundary: one launch of 24 steps that begins on B, and from B - 21
    launches of 8, 30 and 17 steps -- the first ends before B, the second crosses it in the middle
    of a launch and of an octet (B is a multiple of 8, 13 is not), the third lies beyond.  The
    launch on B comes first: step_inc_kernel keeps a direction set over several calls, and a set
    left behind by the launches from B - 21 would reach over B (the engine then reads its columns
    from column 21 on, which is right, but no set would BEGIN on the boundary)."""
    return [(B, (ON_BOUNDARY,)), (B - BEFORE, LAUNCHES)]


# ------------------------------------------------------------------ what a narrowed index would do
def narrowed(step, model):
    """The step index a kernel with a wrong narrowing would use: "low word" keeps step mod 2^32;
    "signed" keeps the low word as an int and widens it again (bit 31 fills the high word);
    "pair low word" keeps 32 bits of the paired stream's index: step mod 2^33."""
    if model == "low word":
        return step & M32
    if model == "signed":
        low = step & M32
        return low if low < P31 else low | (M32 << 32)
    if model == "pair low word":
        return step & (P33 - 1)
    raise ValueError(model)


MODELS = ("low word", "signed", "pair low word")


def run_narrowed(st, S0, n, model):
    """n steps of the oracle from true step S0, every one at its narrowed index (launches cut where
    consecutive steps stop being consecutive under the model)."""
    s, end = S0, S0 + n
    while s < end:
        k = 1
        while s + k < end and narrowed(s + k, model) == narrowed(s, model) + k:
            k += 1
        st.step = narrowed(s, model)
        st.run(k, n_threads=4)
        s += k
    st.step = end


# ------------------------------------------------------------------ the variates, restated
def unpaired_variates(O, seed, gid, step, sub=0, oned=False):
    """(r, E_a) of the un-paired stream (oracle: walker_variates) from the Philox block
    (gid, STREAM_STEP | sub << 16, step mod 2^32, step div 2^32); oned: the column of a
    one-parameter block -- chi(1) as sqrt(2 E) |cos| of a Box-Muller pair, and E_a from a second
    block (| 0x100) on the same counter words."""
    c1, lo, hi = sub << 16, step & M32, step >> 32
    w = O.philox(seed & M32, seed >> 32, gid, c1, lo, hi)
    kr = (w[1] << 20) | (w[2] >> 12)
    ka = (w[3] << 20) | ((w[2] & 0xFFF) << 8) | (w[0] & 0xFF)
    Er = -O.dlog((2 * kr + 1) * 2.0 ** -53)
    expo = (w[0] >> 8) < 5536481
    if oned:
        rr = Er if expo else float(np.sqrt(2.0 * Er)) * abs(O.sincos2pi(ka)[1])
        w2 = O.philox(seed & M32, seed >> 32, gid, c1 | 0x100, lo, hi)
        Ea = -O.dlog((2 * ((w2[0] << 20) | (w2[1] >> 12)) + 1) * 2.0 ** -53)
    else:
        rr = Er if expo else float(np.sqrt(2.0 * Er))
        Ea = -O.dlog((2 * ka + 1) * 2.0 ** -53)
    return (rr if w[0] & 0x80 else -rr), Ea


def paired_variates(O, seed, gid, step):
    """(r, E_a) of the paired stream (oracle: walker_variates_pair) from the Philox block
    (gid, STREAM_STEP | 0x4000, P mod 2^32, P div 2^32), P = step div 2, half step mod 2; None
    where a short uniform fell into its lowest bin (the redraw has a block of its own)."""
    P, h = step >> 1, step & 1
    w = O.philox(seed & M32, seed >> 32, gid, 0x4000, P & M32, P >> 32)
    a, b = w[2 * h], w[2 * h + 1]
    kr, ka = ((a & 0xFFFFF) << 4) | (b >> 28), b & 0x0FFFFFFF
    if kr == 0 or ka == 0:
        return None
    Er = O.neg_log_short(2 * kr + 1, 25)
    rr = Er if ((a >> 20) & 0x7FF) < 676 else float(np.sqrt(2.0 * Er))
    return (rr if a & 0x80000000 else -rr), O.neg_log_short(2 * ka + 1, 29)

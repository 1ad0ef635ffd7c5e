"""Every compiled instantiation of the incremental step kernels ONCE: the names
`Engine.last_step_kernel()` can report, restated from the launch tables of cobaya_amd/csrc, each
marked reachable or not, and for every reachable name the smallest engine configuration that
reaches it.  The conditions on the cases (on the oracle alone): tests/test_instantiations_host.py;
device against oracle, bit for bit: tests/test_gpu_instantiations.py.  No GPU needed.

The step kernels are template matrices and every entry is machine code of its own: its own
register allocation, its own fully unrolled operand loops, its own LDS chunk and its own
hipFuncSetAttribute branch.  One test case runs one entry.

    source                    launcher                               kernel
    incremental_kernels.hip   launch_inc_dq, launch_inc_periodic_dq  step_inc_kernel<DQ, MODE, UNIT_T, ONED, EMIT, PER>
                              launch_drag_dq                         drag_inc_kernel<DQ, MODE, UNIT_T, ONED>
                              launch_inc_mix / dispatch_inc_mix      step_inc_mix_kernel<DQ, KM, UNIT_T, ONED>
    incremental_duo.hip       launch_duo_mix                         step_duo_mix_kernel<DQ, KM, UNIT_T, BOX0>
                              launch_duo1                            step_inc_duo_kernel<DQ, NE, SPLIT, UNIT_T>
    incremental_any.hip       launch_regs (regs_fits, regs_bucket)   step_inc_regs_kernel<DQ, KM, PER>
                              launch_any                             step_inc_any_kernel<DQ>

The kernels that evaluate every trial from scratch -- walker_kernels.hip, one translation unit
per MCMC_D = 1 .. 56, and walker_kernels_big.hip, one per MCMC_DP -- report names that carry no d:
their unit is (name, compiled D or DP), in the second half of this file (SName, scratch_*).

`predict` asks cobaya_amd.engine.incremental_choice -- the library's pure rule, no device -- for
the family; dq is ceil(d / 4) by definition; only the variant suffix is restated here."""
from collections import namedtuple

import numpy as np

from tests.far_steps import NORMAL_PRIOR

FIRST, LONG = 5, 133              # steps of the two launches
DRAG_STEPS = 2
SEED = 7                          # the engine's seed (make_pair's default)
INC_CHOICE = "cobaya_amd/csrc/inc_choice.h"      # (the rules that make a name unreachable)

STEP, PERIODIC, EMIT, DRAG, MIX, DUO_MIX, DUO_ONE, REGS, ANY = (
    "step_inc", "step_inc_periodic", "step_inc_emit", "drag_inc", "step_inc_mix", "step_duo_mix",
    "step_inc_duo", "step_inc_regs", "step_inc_any")
FAMILIES = (STEP, PERIODIC, EMIT, DRAG, MIX, DUO_MIX, DUO_ONE, REGS, ANY)


def teleport_target(L):
    """The long launch begins 70 steps before the refresh of y at 40 L."""
    return 40 * L - 70


# ------------------------------------------------------------------ the names
# name: what last_step_kernel() reports; kernels: the template-ids of the __global__ functions
# behind it, as the demangler prints them (step_inc_duo_kernel: two per name); km: modes of the
# template (0: none); why: "" = reachable, else file:line and the rule that excludes the name
Name = namedtuple("Name", "name family dq km mode unit_t oned periodic emit box kernels why")


def _b(v):
    return "true" if v else "false"


def _name(family, dq, km=0, mode=None, unit_t=True, oned=False, periodic=False, emit=False,
          box=False, why=""):
    if family in (STEP, PERIODIC, EMIT):
        tail = (", periodic" if periodic else "") + (", emit" if emit else "") + (", 1-D blocks" if oned else "")
        name = f"mcmc::step_inc_kernel<{dq}, {mode}, {_b(unit_t)}{tail}>"
        kernels = (f"step_inc_kernel<{dq}, {mode}, {_b(unit_t)}, {_b(oned)}, {_b(emit)}, {_b(periodic)}>",)
    elif family == DRAG:
        name = f"mcmc::drag_inc_kernel<{dq}, {mode}, {_b(unit_t)}{', 1-D blocks' if oned else ''}>"
        kernels = (f"drag_inc_kernel<{dq}, {mode}, {_b(unit_t)}, {_b(oned)}>",)
    elif family == MIX:
        name = f"mcmc::step_inc_mix_kernel<{dq}, {km}, {_b(unit_t)}{', 1-D blocks' if oned else ''}>"
        kernels = (f"step_inc_mix_kernel<{dq}, {km}, {_b(unit_t)}, {_b(oned)}>",)
    elif family == DUO_MIX:
        name = f"mcmc::step_duo_mix_kernel<{dq}, {km}, {_b(unit_t)}{', box' if box else ''}>"
        kernels = (f"step_duo_mix_kernel<{dq}, {km}, {_b(unit_t)}, {_b(box)}>",)
    elif family == DUO_ONE:     # NE = 2 dq - 1 and 2 dq report one name (dq = 1: d = 2 is NE = 1)
        name = f"mcmc::step_inc_kernel<{dq}, 0, {_b(unit_t)}, two lanes>"
        kernels = tuple(f"step_inc_duo_kernel<{dq}, {ne}, true, {_b(unit_t)}>" for ne in (2 * dq - 1, 2 * dq))
    elif family == REGS:        # `emit` is a run-time argument: one kernel behind two names
        name = f"mcmc::step_inc_regs_kernel<{dq}, {km}{', periodic' if periodic else ''}{', emit' if emit else ''}>"
        kernels = (f"step_inc_regs_kernel<{dq}, {km}, {_b(periodic)}>",)
    elif family == ANY:
        name = f"mcmc::step_inc_any_kernel<{dq}{', emit' if emit else ''}>"
        kernels = (f"step_inc_any_kernel<{dq}>",)
    else:
        raise ValueError(family)
    return Name(name, family, dq, km, mode, unit_t, oned, periodic, emit, box, kernels, why)


def regs_fits(dq, km):            # incremental_any.hip: regs_fits
    return dq * (km + 1) <= 208


def regs_bucket(K):               # incremental_any.hip: regs_bucket
    return 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16


def inc_mix_serves(K, dq):        # inc_choice.h: inc_mix_serves
    return K >= 2 and ((K <= 4 and dq <= 16) or (K <= 6 and dq <= 8 and dq * (K + 1) <= 50))


def duo_serves(K, dq):            # inc_choice.h: duo_serves
    return 2 <= K <= 4 and dq <= 12 and 2 * dq * K <= 48


def enumerate_names():
    """Every Name of the families above, in the order of the launch tables."""
    out = []
    for dq in range(1, 33):
        # launch_inc_dq: kerns[12], v = 2 mode + unit_t + 6 oned
        out += [_name(STEP, dq, mode=m, unit_t=t, oned=o)
                for o in (False, True) for m in (0, 1, 2) for t in (False, True)]
        # launch_inc_periodic_dq: kerns[8], v = 2 (mode - 1) + unit_t + 4 oned
        out += [_name(PERIODIC, dq, mode=m, unit_t=t, oned=o, periodic=True)
                for o in (False, True) for m in (1, 2) for t in (False, True)]
        # launch_inc_dq of the MCMC_INC_EMIT_TU build: kerns[6], v = 2 mode + unit_t
        out += [_name(EMIT, dq, mode=m, unit_t=t, emit=True) for m in (0, 1, 2) for t in (False, True)]
    for dq in range(1, 33):           # launch_drag_dq: kerns[12]
        out += [_name(DRAG, dq, mode=m, unit_t=t, oned=o)
                for o in (False, True) for m in (0, 1, 2) for t in (False, True)]
    for dq in range(1, 17):           # dispatch_inc_mix: KM 2..4 to dq 16, 5 and 6 to kMixWideDq = 8
        for km in (2, 3, 4) + ((5, 6) if dq <= 8 else ()):
            why = "" if inc_mix_serves(km, dq) else (
                f"{INC_CHOICE}:27 inc_mix_serves: {km} modes stop at dq ({km} + 1) <= 50; "
                "the shape runs on step_inc_regs_kernel")
            out += [_name(MIX, dq, km=km, unit_t=t, oned=o, why=why)
                    for o in (False, True) for t in (False, True)]
    for dq in range(1, 13):           # dispatch_duo_mix: what duo_serves admits
        for km in (2, 3, 4):
            if duo_serves(km, dq):
                out += [_name(DUO_MIX, dq, km=km, unit_t=t, box=bx)
                        for bx in (False, True) for t in (False, True)]
    for dq in range(1, 9):            # dispatch_duo1: kDuo1MaxDq = 8
        out += [_name(DUO_ONE, dq, mode=0, unit_t=t) for t in (False, True)]
    for km in (2, 4, 8, 16):          # dispatch_regs<1, KM>: every dq that regs_fits
        for dq in range(1, 33):
            if not regs_fits(dq, km):
                continue
            for per in (False, True):
                for emit in (False, True):
                    why = ""
                    if km <= 4 and dq <= 16 and not per and not emit:
                        # one mode reaches the general kernels with emitted rows or periodic
                        # parameters alone; 2..4 modes without either stay on step_inc_mix_kernel
                        why = (f"{INC_CHOICE}:150 inc_choose: without periodic parameters and emitted "
                               f"rows {'1 or 2' if km == 2 else '3 or 4'} modes at dq <= 16 are "
                               "served by step_inc_kernel / step_inc_mix_kernel")
                    out.append(_name(REGS, dq, km=km, periodic=per, emit=emit, why=why))
    for dq in range(1, 33):           # dispatch_any
        out += [_name(ANY, dq, emit=e) for e in (False, True)]
    return out


def by_name():
    return {n.name: n for n in enumerate_names()}


def reachable():
    return [n for n in enumerate_names() if not n.why]


def swept():
    """The reachable names the device sweep runs."""
    return [n for n in reachable() if n.name not in HELD_BACK]


def enumerate_kernels():
    """The template-ids of every kernel behind the names (reachable or not)."""
    return {k for n in enumerate_names() for k in n.kernels}


# ------------------------------------------------------------------ the cases
# prior: 0 the unit box, 1 per-parameter boxes, 2 normal priors on the odd parameters;
# blocks: None or (blocks, oversampling, drag_last_slow, drag_steps); periodic: the periodic indices;
# seed: of the generator that draws target and start (make_pair's rng)
Case = namedtuple("Case", "name family d W gs bgs K prior T blocks periodic emit duo seed")

# (name: seed) where the default 100 + d does not meet the conditions of
# tests/test_instantiations_host.py on the oracle
SEEDS = {}


# Reachable names the device sweep holds back, with the reason.  Their cases stay here and meet the
# conditions on the oracle; tests/test_gpu_instantiations.py does not run them.  Evidence, what has
# been ruled out and the follow-up: docs/KERNELS.md, "Open: faults the instantiation sweep met".
#   step_inc_kernel<29, 1, true, emit> at d = 116 and step_inc_kernel<30, 1, true, emit> at d = 120
#   (64 walkers, per-parameter boxes, T = 1, emit capacity 146, burn-in 2) end with "an illegal
#   memory access was encountered"; cause unknown.  dq = 31 and 32 of the variant: never run.
_WHY_HELD = "MODE 1, UNIT_T, emit at dq >= 29: faulted on the device (illegal memory access), cause not found"
#   step_inc_any_kernel<26> with five modes at d = 101 or 102 (it is not known which): the same
#   fault; cause unknown.  dq = 27 .. 32 reach the kernel with the same five modes: never run.
_WHY_ANY = "five modes at dq >= 26: faulted on the device at dq = 26 (illegal memory access), cause not found"
HELD_BACK = {
    **{f"mcmc::step_inc_any_kernel<{dq}{e}>": _WHY_ANY + ("" if dq == 26 else " (not run: held back with it)")
       for dq in range(26, 33) for e in ("", ", emit")},
    "mcmc::step_inc_kernel<29, 1, true, emit>": _WHY_HELD,
    "mcmc::step_inc_kernel<30, 1, true, emit>": _WHY_HELD,
    "mcmc::step_inc_kernel<31, 1, true, emit>": _WHY_HELD + " (not run: held back with them)",
    "mcmc::step_inc_kernel<32, 1, true, emit>": _WHY_HELD + " (not run: held back with them)",
}


def dims_of(dq):
    return [d for d in range(4 * dq - 3, 4 * dq + 1) if d >= 2]


def _dealt(family):
    """name -> (position among the names of its (family, dq), names there): the round-robin."""
    out, groups = {}, {}
    for n in enumerate_names():
        if n.family == family and not n.why:
            groups.setdefault(n.dq, []).append(n.name)
    for names in groups.values():
        for i, name in enumerate(names):
            out[name] = i
    return out


_DEALT = {}


def _deal(n, d_min):
    if n.family not in _DEALT:
        _DEALT[n.family] = _dealt(n.family)
    ds = dims_of(n.dq)
    i = _DEALT[n.family][n.name]
    for k in range(len(ds)):
        d = ds[(i + k) % len(ds)]
        if d >= d_min:
            return d, i
    raise ValueError(n.name)


def _blocks(n, d):
    if n.family == DRAG:
        # the slow block's parameters are the cycle; `1-D blocks`: the fast block is one parameter
        cut = d - 1 if n.oned else d // 2
        return ([list(range(cut)), list(range(cut, d))], [1, 1], 0, DRAG_STEPS)
    if n.oned:     # a blocking whose last block has one parameter, four times per cycle: at
        # d = 128 the 138 steps are one cycle
        return ([list(range(d - 1)), [d - 1]], [1, 4], -1, 0)
    return None


def _modes_of(n):
    """The mode counts that can reach a name, ascending."""
    if n.family in (MIX, DUO_MIX):
        return [n.km]
    if n.family == REGS:
        return [K for K in range(1, 17) if regs_bucket(K) == n.km]
    if n.family == ANY:
        return list(range(1, 25))
    return [1]


def case_for(name, d=None):
    """The smallest configuration that reaches `name` (a Name or its string); d: one of the
    dimensions of its dq instead of the dealt one (step_inc_duo_kernel runs at all four)."""
    n = by_name()[name] if isinstance(name, str) else name
    if n.why:
        raise ValueError(f"{n.name} is unreachable: {n.why}")
    # dragging: two slow parameters at least (the teleport needs 40 L >= 70 + FIRST), and two fast
    # ones where the fast block is not `1-D`
    d_min = 2 if n.family != DRAG else (3 if n.oned else 4)
    dealt, i = _deal(n, d_min)
    d = dealt if d is None else d
    assert d in dims_of(n.dq) and d >= d_min
    duo = n.family in (DUO_MIX, DUO_ONE)
    if n.mode is not None:
        prior = n.mode
    elif n.family == DUO_MIX:
        prior = 0 if n.box else 1 + i % 2
    else:
        prior = i % 3      # (the name does not say: every prior in turn)
    # (step_inc_any_kernel where the register planes end: more than 16 modes while its LDS holds
    # them, else one mode with every parameter periodic -- their columns of L^-1 do not fit
    # beside the planes)
    tries = [(K, (0,) if n.periodic else ()) for K in _modes_of(n)]
    if n.family == ANY:
        tries.append((1, tuple(range(d))))
    for K, periodic in tries:
        c = Case(n.name, n.family, d, 128 if duo else 64, 64, 128 if duo else 64, K,
                 1 if len(periodic) > 1 else prior, 1.0 if n.unit_t else 2.0, _blocks(n, d), periodic,
                 n.emit, duo, SEEDS.get(n.name, 100 + d))
        if predict(c) == n.name:
            return c
    raise ValueError(f"no configuration reaches {n.name}")


def cases_of(n):
    """The cases of one name: step_inc_duo_kernel at every d of its dq (NE = 2 dq - 1 and 2 dq
    share the name), everything else at its dealt d."""
    if n.family == DUO_ONE:
        return [case_for(n, d) for d in dims_of(n.dq)]
    return [case_for(n)]


def cycle_length(c):
    if c.blocks is None:
        return c.d
    blocks, over, last_slow, _ = c.blocks
    use = blocks if last_slow < 0 else blocks[:last_slow + 1]
    return sum(o * len(b) for o, b in zip(over, use))


def prior_of(c, means, covs):
    """kinds, a, b, periodic of a case (lists, as make_pair takes them)."""
    d = c.d
    kinds, a, b = [0] * d, [0.0] * d, [1.0] * d
    if c.prior == 1:
        b = [1.0 + 0.25 * (i % 2) for i in range(d)]
    elif c.prior == 2:
        kinds = [i % 2 for i in range(d)]
        a = [NORMAL_PRIOR[0] if k else 0.0 for k in kinds]
        b = [NORMAL_PRIOR[1] if k else 1.0 for k in kinds]
    periodic = None
    if c.periodic:                  # intervals about 3 sigma wide around the mode: walkers wrap
        periodic = [int(i in c.periodic) for i in range(d)]
        for p in c.periodic:
            s = float(np.sqrt(covs[0][p, p]))
            a[p], b[p] = float(means[0][p]) - 1.5 * s, float(means[0][p]) + 1.5 * s
    return kinds, a, b, periodic


def target_of(c):
    """(means, covs) make_pair draws first from the case's generator."""
    from tests.test_gpu_parity import random_target
    return random_target(c.d, c.K, np.random.default_rng(c.seed))


def cap_of(c):
    return FIRST + LONG + 8 if c.emit else 0     # (no row is dropped)


def pair_arguments(c):
    """(positional, keyword) arguments of tests/test_gpu_parity.py: make_pair for a case."""
    means, covs = target_of(c)
    kinds, a, b, periodic = prior_of(c, means, covs)
    kw = dict(K=c.K, kinds=kinds, a=a, b=b, periodic=periodic, seed=SEED, T=c.T,
              burn_in=2 if c.emit else 0, cap=cap_of(c), rng=np.random.default_rng(c.seed),
              incremental=True, basis_group_size=c.bgs)
    if c.K > 1:     # unequal weights
        w = np.arange(1.0, c.K + 1.0)
        kw["weights"] = (w / w.sum()).tolist()
    if c.blocks is not None:
        blocks, over, last_slow, n_drag = c.blocks
        kw.update(blocks=blocks, over=over, drag_last_slow=last_slow, drag_steps=n_drag)
    return (c.d, c.W, c.gs), kw


def shape_of(c):
    """The arguments of cobaya_amd.engine.incremental_choice for a case."""
    return dict(d=c.d, n_modes=c.K, n_periodic=len(c.periodic),
                n_drag=c.blocks[3] if c.blocks is not None else 0, n_walkers=c.W,
                basis_group_size=c.bgs, any_normal=c.prior == 2,
                one_box=c.prior == 0 and not c.periodic,
                box_lo_is_zero=c.prior == 0 and not c.periodic,
                has_1d_block=c.blocks is not None and min(len(b) for b in c.blocks[0]) == 1,
                emit=c.emit, duo=1 if c.duo else -1)


def regs_serves(K, dq, n_periodic):     # incremental_any.hip: regs_serves
    if K < 1 or K > 16 or not regs_fits(dq, regs_bucket(K)):
        return False
    return not (n_periodic > 0 and 8 * n_periodic * (64 + K * 4 * dq) > (24 << 10))


def name_of(s, K, T, emit):
    """The name last_step_kernel() reports for a shape `s` (the arguments of incremental_choice),
    K modes and temperature T: the family from the library's rule, the variant suffix restated
    from the launchers.  None: incremental evaluation does not serve the shape."""
    from cobaya_amd import engine as E
    ch = E.incremental_choice(**s)
    fam, dq = ch["family"], (s["d"] + 3) // 4
    t, oned, per = T == 1.0, bool(s["has_1d_block"]), s["n_periodic"] > 0
    box0 = bool(s["one_box"] and s["box_lo_is_zero"])
    mode = 2 if s["any_normal"] else (0 if box0 else 1)
    if fam == E.INC_STEP:     # (a periodic parameter has an interval of its own: never MODE 0)
        return _name(PERIODIC if per else STEP, dq, mode=max(mode, 1) if per else mode, unit_t=t,
                     oned=oned, periodic=per).name
    if fam == E.INC_STEP_EMIT:
        return _name(EMIT, dq, mode=mode, unit_t=t, emit=True).name
    if fam == E.INC_DRAG:     # (launch_drag_dq: MODE 0 is ANY one box)
        mode = 2 if s["any_normal"] else (0 if s["one_box"] else 1)
        return _name(DRAG, dq, mode=mode, unit_t=t, oned=oned).name
    if fam == E.INC_MIX:
        return _name(MIX, dq, km=K, unit_t=t, oned=oned).name
    if fam == E.INC_DUO_MIX:
        return _name(DUO_MIX, dq, km=K, unit_t=t, box=box0).name
    if fam == E.INC_DUO_ONE:
        return _name(DUO_ONE, dq, mode=0, unit_t=t).name
    if fam == E.INC_ANY:
        if regs_serves(K, dq, s["n_periodic"]):
            return _name(REGS, dq, km=regs_bucket(K), periodic=per, emit=emit).name
        return _name(ANY, dq, emit=emit).name
    return None


def predict(c):
    """The name last_step_kernel() reports for a case."""
    return name_of(shape_of(c), c.K, c.T, c.emit)


def predict_arguments(d, W, gs, K=1, kinds=None, a=None, b=None, periodic=None, T=1.0, cap=0,
                      blocks=None, drag_last_slow=-1, drag_steps=0, basis_group_size=None,
                      duo=False, **others):
    """predict for the arguments of make_pair (incremental=True), two lanes where MCMC_HIP_DUO=1."""
    kinds = [0] * d if kinds is None else list(kinds)
    a = [0.0] * d if a is None else list(a)
    b = [1.0] * d if b is None else list(b)
    normal = any(k == 1 for k in kinds)
    one_box = not normal and all((a[i], b[i]) == (a[0], b[0]) for i in range(d))
    s = dict(d=d, n_modes=K, n_periodic=int(sum(periodic)) if periodic is not None else 0,
             n_drag=drag_steps if drag_last_slow >= 0 else 0, n_walkers=W,
             basis_group_size=basis_group_size or gs, any_normal=normal, one_box=one_box,
             box_lo_is_zero=one_box and a[0] == 0.0,
             has_1d_block=blocks is not None and min(len(bl) for bl in blocks) == 1,
             emit=cap > 0, duo=1 if duo else -1)
    return name_of(s, K, T, cap > 0)


# ------------------------------------------------------------------ the oracle alone
def oracle_alone(c):
    """Problem and state of a case with the oracle's OWN constants (the numpy recipe), started
    where make_pair starts engine and oracle: its draws, restated in its order."""
    from oracle import cbind as O
    d, W = c.d, c.W
    rng = np.random.default_rng(c.seed)
    from tests.test_gpu_parity import random_target
    means, covs = random_target(d, c.K, rng)
    kinds, a, b, periodic = prior_of(c, means, covs)
    x0 = start_of(c, rng, means, covs, kinds, a, b, periodic)
    pcov = covs[0] * c.T
    kw, weights = {}, None
    if c.blocks is not None:
        blocks, over, last_slow, n_drag = c.blocks
        kw = dict(blocks=blocks, oversampling=over, drag_last_slow=last_slow, drag_steps=n_drag)
        T = O.blocked_transform(pcov, blocks, 2.4)
    else:
        T = O.proposal_transform(pcov, 2.4)
    if c.K > 1:
        w = np.arange(1.0, c.K + 1.0)
        weights = (w / w.sum()).tolist()
    from cobaya_amd import engine as E
    ch = E.incremental_choice(**shape_of(c))
    prob = O.Problem(d, kinds, a, b, periodic=periodic, means=means, covs=covs, weights=weights,
                     T=T, group_size=c.bgs, seed=SEED, temperature=c.T, incremental=True,
                     carry_modes=bool(ch["carry_modes"]), carry_periodic=bool(ch["carry_periodic"]),
                     **kw)
    st = O.State(prob, x0, burn_in=2 if c.emit else 0, row_cap=cap_of(c))
    return prob, st


def start_of(c, rng, means, covs, kinds, a, b, periodic):
    """x0 of make_pair (its own helper), from the generator as random_target left it."""
    from tests.test_gpu_parity import start_points
    return start_points(rng, c.d, c.W, means, covs, kinds, a, b, periodic)


def one_parameter_column(prob, c, group, step):
    """Does step `step` of basis group `group` fall on the column of a one-parameter block?"""
    L = cycle_length(c)
    blk, _, _ = prob.schedule(group, step // L, 1 if c.blocks[2] >= 0 else 0)
    return len(c.blocks[0][blk[step % L]]) == 1


# ================================================================== every trial from scratch
# walker_kernels.hip (D = 1 .. 32 all of its kernels, D = 33 .. 56 step_pair_kernel alone),
# walker_kernels_big.hip (one translation unit per DP) and general_kernels.hip (one symbol each).
# The names carry no d: the unit is (name, D), D the compiled MCMC_D or MCMC_DP (0: one symbol).
# Which kernel serves a shape is scratch_choose's (cobaya_amd/csrc/scratch_choice.h), asked without
# a device through cobaya_amd.engine.scratch_choice; predict_scratch is its INDEPENDENT restatement
# -- the one the device sweep has verified -- and tests/test_host_logic.py holds one against the other.
BIG_DPS = (48, 56, 64, 72, 80, 88, 96, 100, 112, 120, 128)     # scratch_choice.h: kBigDps
# MCMC_PAIR_MIN, kMaxDimPair, kMaxDimPairNormal, kMaxDimLane, kSweepMaxDim, kLdsMax
PAIR_MIN, PAIR_MAX, PAIR_MAX_NORMAL, LANE_MAX, SWEEP_MAX, LDS_MAX = 14, 56, 54, 32, 112, 160 * 1024
SCRATCH_CHOICE = "scratch_choice.h"      # (the rules that make a name unreachable)
S_STEP, S_OWN, S_DRAG, S_PAIR, S_MFMA, S_BIG = ("scratch_step", "scratch_own", "scratch_drag",
                                                "scratch_pair", "scratch_mfma", "scratch_big_reg")
S_FAMILIES = (S_STEP, S_OWN, S_DRAG, S_PAIR, S_MFMA, S_BIG)
GENERAL_STEP, GENERAL_DRAG = "mcmc::step_general_kernel", "mcmc::drag_general_kernel"
# the refusals of scratch_choose (mcmc_hip_scratch_answer.reason)
(R_BAD_SHAPE, R_EMIT_THIN, R_OWN_BLOCKS, R_GENERAL_LDS, R_CYCLE_LDS, R_SWEEP_SIZE,
 R_SWEEP_NORMAL) = range(1, 8)
# D: the compiled MCMC_D (MCMC_DP for the last two families); flags: the template arguments
SName = namedtuple("SName", "name family D flags kernel why")
# prior: 0 the unit box, 2 normal priors on the odd parameters; periodic: the periodic indices;
# blocks: None, "two" (two blocks of two parameters or more), "one" (the last block is one
# parameter), "over" (two blocks, the second five times per cycle); thin: emit_thin > 1
SCase = namedtuple("SCase", "name family D d W gs K prior T own drag seed periodic emit blocks thin",
                   defaults=((), False, None, False))


def dp_of(d):
    return next(dp for dp in BIG_DPS if dp >= d)      # ctx.h: big_for_dim


def dims_of_dp(dp):
    """The smallest and the largest d that map to a padded size."""
    below = [q for q in BIG_DPS if q < dp]
    return sorted({(below[-1] if below else LANE_MAX) + 1, dp})


def v_slab(cols, d, big):
    """scratch_choice.h: v_slab_cols, v_slab_big (doubles)."""
    ld = (d + 1) & ~1
    return ((d * ld * 8 + 1024 + 1023) // 1024) * 128 if big else ((cols * d * 8 + 1023) // 1024) * 128


def pair_lds(d, gs, normp, cols=None):
    """scratch_choose's pair_lds, with pair_split and pair_xf (kRowBlock = 4) and the slab of the
    directions (cols: columns per cycle at d <= 32, d without blocks)."""
    big = d > LANE_MAX
    h = 4 * ((2 * d + 6) // 12)
    if big:
        h = 24 if d < 37 else 32 if d < 47 else 36 if d < 49 else 40 if d < 53 else 44
    if normp:
        h += 4
    hmax = d - 1 - (d - 1) % 4
    split = 4 if h < 4 else min(h, hmax)
    xf = d - split + (4 if normp else 3) + (3 if big else 0)
    return 8 * (2 * (256 // gs) * v_slab(d if cols is None else cols, d, big) + 2 * xf * 256)


def pair_fits(d, W, gs, multi, normp, cols=None):      # scratch_choose: `pair` (no periodic, rows, 1-D column)
    return (PAIR_MIN <= d <= PAIR_MAX and not multi and W % 256 == 0 and 256 % gs == 0
            and not (d > PAIR_MAX_NORMAL and normp) and pair_lds(d, gs, normp, cols) <= LDS_MAX)


def enumerate_scratch():
    out = []
    for D in range(1, LANE_MAX + 1):
        for multi in (False, True):
            for general in (False, True):      # kScratchStep
                why = ""
                if D == 1 and not general:
                    why = f"{SCRATCH_CHOICE} scratch_choose, kScratchStep: d == 1 always takes the general step"
                out.append(SName(f"mcmc::step_kernel<{_b(multi)}, {_b(general)}>", S_STEP, D, (multi, general),
                                 f"step_kernel<{_b(multi)}, {_b(general)}, false>", why))
            out.append(SName(f"mcmc::step_kernel<{_b(multi)}, true, own basis>", S_OWN, D, (multi,),
                             f"step_kernel<{_b(multi)}, true, true>",
                             f"{SCRATCH_CHOICE} scratch_choose, `own`: a basis per walker needs d > 1" if D == 1 else ""))
            out.append(SName(f"mcmc::drag_kernel<{_b(multi)}>", S_DRAG, D, (multi,), f"drag_kernel<{_b(multi)}>",
                             f"{SCRATCH_CHOICE} ScratchShape::n_drag: dragging needs a slow and a fast parameter"
                             if D == 1 else ""))
    for D in range(1, PAIR_MAX + 1):           # kScratchPair: compiled at every D, served from MCMC_PAIR_MIN on
        for unit_t in (False, True):
            for normp in (False, True):
                why = ""
                if D < PAIR_MIN:
                    why = f"{SCRATCH_CHOICE} scratch_choose, `pair`: d >= MCMC_PAIR_MIN = 14"
                elif D > PAIR_MAX_NORMAL and normp:
                    why = (f"{SCRATCH_CHOICE} scratch_choose, `pair`: with normal priors step_mfma_kernel serves "
                           "d > kMaxDimPairNormal = 54")
                out.append(SName(f"mcmc::step_pair_kernel<{_b(unit_t)}, {_b(normp)}>", S_PAIR, D, (unit_t, normp),
                                 f"step_pair_kernel<{_b(unit_t)}, {_b(normp)}>", why))
    for dp in BIG_DPS:                         # kScratchMfma, kScratchBigReg
        for normp in (False, True):
            out.append(SName(f"mcmc::step_mfma_kernel<{_b(normp)}>", S_MFMA, dp, (normp,),
                             f"step_mfma_kernel<{_b(normp)}>", ""))
        if dp <= SWEEP_MAX:                    # (kSweepMaxDim: no column sweep above)
            out.append(SName("mcmc::step_big_reg_kernel", S_BIG, dp, (), "step_big_reg_kernel", ""))
    return out


def scratch_kernel_counts():
    """kernel template-id -> the number of translation units that compile it."""
    out = {}
    for n in enumerate_scratch():
        out[n.kernel] = out.get(n.kernel, 0) + 1
    return out


def _scratch_case(n, d):
    f = n.family
    W, gs, K, prior, T, own, drag = 64, 64, 1, 0, 1.0, False, False
    if f == S_STEP:
        K, prior = (2 if n.flags[0] else 1), (2 if n.flags[1] and d > 1 else 0)
    elif f == S_OWN:
        K, own = (2 if n.flags[0] else 1), True
    elif f == S_DRAG:
        K, drag = (2 if n.flags[0] else 1), True
    elif f == S_PAIR:          # whole workgroups of 256 walkers; d > 32: one group each (pair_lds)
        W, T, prior = 256, (1.0 if n.flags[0] else 2.0), (2 if n.flags[1] else 0)
        gs = 256 if d > LANE_MAX else 64
    elif f == S_MFMA:          # (up to d = 56: where the two-wave kernel's LDS does not hold four groups)
        W, prior = 256, (2 if n.flags[0] else 0)
    return SCase(n.name, f, n.D, d, W, gs, K, prior, T, own, drag, 300 + d)


def scratch_cases_of(n):
    """walker_kernels.hip at its compiled D; walker_kernels_big.hip at the smallest and the
    largest d of its DP."""
    if n.why:
        raise ValueError(f"{n.name} at D = {n.D} is unreachable: {n.why}")
    if n.family not in (S_MFMA, S_BIG):
        return [_scratch_case(n, n.D)]
    # (DP = 48: step_mfma_kernel begins where step_pair_kernel's LDS ends, d = 36 at four groups
    # of 64 walkers per workgroup -- d = 41 with normal priors)
    lo, hi = dims_of_dp(n.D)[0], n.D
    ds = [d for d in range(lo, hi + 1) if predict_scratch(_scratch_case(n, d)) == (n.name, n.D)]
    return [_scratch_case(n, d) for d in sorted({ds[0], ds[-1]})]


def scratch_blocks(c):
    """(blocks, oversampling, drag_last_slow, drag_steps) of a case, or None."""
    d = c.d
    if c.drag:
        cut = max(1, d // 2)
        return ([list(range(cut)), list(range(cut, d))], [1, 1], 0, DRAG_STEPS)
    if c.blocks == "one":     # the last block has one parameter, four times per cycle
        return ([list(range(d - 1)), [d - 1]], [1, 4], -1, 0)
    if c.blocks in ("two", "over"):
        cut = max(1, d // 2)
        return ([list(range(cut)), list(range(cut, d))], [1, 5 if c.blocks == "over" else 1], -1, 0)
    return None


def scratch_columns(c):
    """Direction columns per cycle (dragging: of the slow blocks), of the fast blocks: capi.hip, block_slots."""
    bl = scratch_blocks(c)
    if bl is None:
        return c.d, 0
    blocks, over, last_slow, _ = bl
    if last_slow >= 0:
        return sum(len(b) for b in blocks[:last_slow + 1]), sum(len(b) for b in blocks[last_slow + 1:])
    return sum(o * len(b) for o, b in zip(over, blocks)), 0


def scratch_prior(c, means=None, covs=None):
    """kinds, a, b (and the periodic flags where the case has periodic parameters)."""
    d = c.d
    kinds, a, b = [0] * d, [0.0] * d, [1.0] * d
    if c.prior == 2:     # normal priors on the odd parameters (d = 1: a general step for D == 1 alone)
        kinds = [i % 2 for i in range(d)]
        a = [NORMAL_PRIOR[0] if k else 0.0 for k in kinds]
        b = [NORMAL_PRIOR[1] if k else 1.0 for k in kinds]
    if not c.periodic:
        return kinds, a, b
    for p in c.periodic:     # intervals about 3 sigma wide around the mode: walkers wrap
        s = float(np.sqrt(covs[0][p, p]))
        kinds[p], a[p], b[p] = 0, float(means[0][p]) - 1.5 * s, float(means[0][p]) + 1.5 * s
    return kinds, a, b, [int(i in c.periodic) for i in range(d)]


def scratch_steps(c):
    return (FIRST, c.d + 7)


def scratch_cap(c):
    return sum(scratch_steps(c)) + 8 if c.emit else 0     # (no row is dropped)


def scratch_pair_arguments(c):
    from tests.test_gpu_parity import random_target
    means, covs = random_target(c.d, max(c.K, 1), np.random.default_rng(c.seed))
    kinds, a, b, *per = scratch_prior(c, means, covs)
    kw = dict(K=c.K, kinds=kinds, a=a, b=b, periodic=per[0] if per else None, seed=SEED, T=c.T,
              rng=np.random.default_rng(c.seed), incremental=False, shared_basis=not c.own,
              burn_in=2 if c.emit else 0, cap=scratch_cap(c))
    if c.K > 1:
        kw["weights"] = [1.0 / 3.0, 2.0 / 3.0]
    bl = scratch_blocks(c)
    if bl is not None:
        kw.update(blocks=bl[0], over=bl[1], drag_last_slow=bl[2], drag_steps=bl[3])
    return (c.d, c.W, c.gs), kw


def predict_scratch(c, pair_big=True):
    """(name, D) a from-scratch case reports, or (None, reason) where mcmc_hip_step refuses it: what
    scratch_choice.h decides, restated on its own.  pair_big: the two-wave kernels of 32 < d <= 56 are there."""
    d, K, W, gs = c.d, c.K, c.W, c.gs
    multi, normal, periodic = K > 1, c.prior == 2 and d > 1, bool(c.periodic)
    unit_t, own, big = c.T == 1.0, c.own and d > 1, d > LANE_MAX
    blocked = c.blocks is not None or c.drag
    cols, _ = scratch_columns(c)
    if c.thin:
        return None, R_EMIT_THIN
    if own and blocked:
        return None, R_OWN_BLOCKS
    wg = 256 if W % 256 == 0 else 128 if W % 128 == 0 else 64
    if big:
        general = (own or blocked or K != 1 or periodic or c.emit
                   or (W % 256 != 0 and (normal or d > SWEEP_MAX)))
        if general and 8 * 64 * (2 * d + max(1, K)) > LDS_MAX:
            return None, R_GENERAL_LDS
        if c.drag:
            return GENERAL_DRAG, 0
        if general:
            return GENERAL_STEP, 0
        if pair_big and pair_fits(d, W, gs, multi, normal):
            return f"mcmc::step_pair_kernel<{_b(unit_t)}, {_b(normal)}>", d
        if W % 256 == 0:     # (group_size 64, 128 or 256: each divides 256)
            return f"mcmc::step_mfma_kernel<{_b(normal)}>", dp_of(d)
        return "mcmc::step_big_reg_kernel", dp_of(d)
    if c.drag:
        return f"mcmc::drag_kernel<{_b(multi)}>", d
    if own:
        return f"mcmc::step_kernel<{_b(multi)}, true, own basis>", d
    if 8 * (2 * (wg // gs) * v_slab(cols, d, False) + (K * wg if multi else 0)) > LDS_MAX:
        return None, R_CYCLE_LDS
    column_1d = c.blocks == "one"
    if not (periodic or c.emit or column_1d) and K == 1 and pair_fits(d, W, gs, multi, normal, cols):
        return f"mcmc::step_pair_kernel<{_b(unit_t)}, {_b(normal)}>", d
    general = normal or periodic or K == 0 or c.emit or d == 1 or column_1d
    return f"mcmc::step_kernel<{_b(multi)}, {_b(general)}>", d


def scratch_shape_of(c):
    """The arguments of cobaya_amd.engine.scratch_choice for a case."""
    cols, cols_f = scratch_columns(c)
    return dict(d=c.d, n_modes=c.K, n_walkers=c.W, group_size=c.gs, any_normal=c.prior == 2 and c.d > 1,
                any_periodic=bool(c.periodic), emit=c.emit, emit_thin=c.thin, unit_t=c.T == 1.0, own_basis=c.own,
                blocked=c.blocks is not None or c.drag, n_drag=DRAG_STEPS if c.drag else 0, cps=cols, cps_f=cols_f,
                has_1d_column=c.blocks == "one")


def scratch_name_of(ch):
    """(name, unit) the launcher reports for an answer of cobaya_amd.engine.scratch_choice -- the
    note_step_kernel strings of the launchers -- or (None, reason)."""
    from cobaya_amd import engine as E
    multi, general, unit_t, normp = (_b(ch[k]) for k in ("multi", "general", "unit_t", "normp"))
    name = {E.SCRATCH_NOT_SERVED: None,
            E.SCRATCH_STEP: f"mcmc::step_kernel<{multi}, {general}>",
            E.SCRATCH_STEP_OWN: f"mcmc::step_kernel<{multi}, true, own basis>",
            E.SCRATCH_PAIR: f"mcmc::step_pair_kernel<{unit_t}, {normp}>",
            E.SCRATCH_MFMA: f"mcmc::step_mfma_kernel<{normp}>",
            E.SCRATCH_BIG_REG: "mcmc::step_big_reg_kernel",
            E.SCRATCH_GENERAL: GENERAL_STEP,
            E.SCRATCH_DRAG: f"mcmc::drag_kernel<{multi}>",
            E.SCRATCH_GENERAL_DRAG: GENERAL_DRAG}[ch["family"]]
    return (name, ch["unit"]) if name else (None, ch["reason"])


def general_cases():
    """step_general_kernel and drag_general_kernel have a run-time d and one symbol each: no unit per
    D.  One case per reason scratch_choose sends a shape to them, at the smallest and the largest d:
    two modes, `one`, a periodic parameter, emitted rows, own bases; an ensemble of 64 walkers with
    normal priors; d = 113 (above the column sweep) with 320 walkers; dragging."""
    def case(name, d, W=64, **kw):
        return SCase(name, "scratch_general", 0, d, W, 64, kw.pop("K", 1), kw.pop("prior", 0), 1.0,
                     kw.pop("own", False), kw.pop("drag", False), 300 + d, **kw)
    out = []
    for d in (33, 128):
        out += [case(GENERAL_STEP, d, K=2), case(GENERAL_STEP, d, K=0), case(GENERAL_STEP, d, periodic=(0,)),
                case(GENERAL_STEP, d, emit=True), case(GENERAL_STEP, d, own=True)]
    out += [case(GENERAL_STEP, 33, prior=2), case(GENERAL_STEP, 113, W=320), case(GENERAL_DRAG, 33, drag=True)]
    return out


# The grid the rule is held against: every d, ensembles on both sides of every workgroup width (and
# 65 792 = 257 workgroups of 256: two per compute unit for the placement request), every group size
# that divides them, `one` / one mode / two, every prior and option, every kind of blocking
GRID_W = (64, 128, 192, 256, 320, 512, 65536, 65792)
GRID_VARIANTS = (None, "drag", "two", "one", "over", "thin")


def scratch_grid():
    for d in range(1, 129):
        for W in GRID_W:
            for gs in (64, 128, 256):
                if W % gs:
                    continue
                for K in (0, 1, 2):
                    for normal in (False, True):
                        for per in (False, True):
                            for emit in (False, True):
                                for own in (False, True):
                                    for var in GRID_VARIANTS:
                                        if d == 1 and var not in (None, "thin"):
                                            continue      # (blocks and dragging need two parameters)
                                        for T in (1.0, 2.0):
                                            yield SCase("", "", 0, d, W, gs, K, 2 if normal else 0, T, own,
                                                        var == "drag", 0, (0,) if per else (), emit,
                                                        var if var in ("two", "one", "over") else None, var == "thin")


_CENSUS = []


def scratch_grid_census():
    """One pass over the grid, shared by the host tests: {(name, unit) or (None, reason): shapes} as
    mcmc_hip_scratch_choice answers, the number of shapes, and the first shapes where predict_scratch
    answers otherwise."""
    if not _CENSUS:
        import ctypes
        from cobaya_amd import engine as E
        lib, shape, out = E.load_library(), E.ScratchShape(), E.ScratchChoice()
        fields = [f for f, _ in E.ScratchChoice._fields_]
        seen, wrong, n = {}, [], 0
        for c in scratch_grid():
            for k, v in scratch_shape_of(c).items():
                setattr(shape, k, int(v))
            assert lib.mcmc_hip_scratch_choice(ctypes.byref(shape), ctypes.byref(out)) == 0
            got = scratch_name_of({f: getattr(out, f) for f in fields})
            seen[got] = seen.get(got, 0) + 1
            n += 1
            if got != predict_scratch(c) and len(wrong) < 5:
                wrong.append((c, got, predict_scratch(c)))
        _CENSUS.append((seen, n, wrong))
    return _CENSUS[0]


def scratch_oracle_alone(c):
    """Problem and state of a from-scratch case with the oracle's own constants."""
    from oracle import cbind as O
    from tests.test_gpu_parity import random_target, start_points
    rng = np.random.default_rng(c.seed)
    means, covs = random_target(c.d, c.K, rng) if c.K else (None, None)
    kinds, a, b, *per = scratch_prior(c, means, covs)
    periodic = per[0] if per else None
    x0 = start_points(rng, c.d, c.W, means, covs, kinds, a, b, periodic)
    pcov = (covs[0] if c.K else np.diag(np.full(c.d, 0.01))) * c.T
    kw, bl = {}, scratch_blocks(c)
    if bl is not None:
        kw = dict(blocks=bl[0], oversampling=bl[1], drag_last_slow=bl[2], drag_steps=bl[3])
        T = O.blocked_transform(pcov, bl[0], 2.4)
    else:
        T = O.proposal_transform(pcov, 2.4)
    prob = O.Problem(c.d, kinds, a, b, periodic=periodic, means=means, covs=covs,
                     weights=[1.0 / 3.0, 2.0 / 3.0] if c.K > 1 else None,
                     T=T, group_size=1 if (c.own and c.d > 1) else c.gs, seed=SEED, temperature=c.T, **kw)
    return prob, O.State(prob, x0, burn_in=2 if c.emit else 0, row_cap=scratch_cap(c))

"""tests/instantiations.py on the CPU: the cases cover exactly the reachable names; every case, on
the oracle alone, meets the conditions that make a wrong kernel visible; the enumeration is the
set of kernel symbols of the library's gfx950 code objects.  The device against the oracle:
tests/test_gpu_instantiations.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import instantiations as I

NAMES = I.enumerate_names()
REACHABLE = [n for n in NAMES if not n.why]
GROUPS = sorted({(n.family, n.dq) for n in REACHABLE}, key=lambda g: (I.FAMILIES.index(g[0]), g[1]))


def test_the_counts_of_the_launch_tables():
    """The tables of the sources, counted: names per family, kernels behind them."""
    assert len({n.name for n in NAMES}) == len(NAMES)
    per = {f: sum(n.family == f for n in NAMES) for f in I.FAMILIES}
    assert per[I.STEP] + per[I.PERIODIC] + per[I.EMIT] == 32 * (12 + 8 + 6) == 832
    assert per[I.DRAG] == 384 and per[I.MIX] == 256 and per[I.DUO_MIX] == 104
    assert per[I.DUO_ONE] == 16 and per[I.REGS] == 396 and per[I.ANY] == 64
    kernels = I.enumerate_kernels()
    assert sum(k.startswith("step_inc_duo_kernel") for k in kernels) == 32
    assert sum(k.startswith("step_inc_regs_kernel") for k in kernels) == 198
    assert sum(k.startswith("step_inc_any_kernel") for k in kernels) == 32
    unreachable = [n for n in NAMES if n.why]
    assert len(unreachable) == 4 + 32
    for n in unreachable:      # file:line of the rule, and the line is there
        m = re.match(r"(\S+):(\d+) ", n.why)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), m.group(1))) as f:
            line = f.read().splitlines()[int(m.group(2)) - 1]
        assert "dq * (K + 1) <= 50" in line or "K > 1 && !inc_mix_serves(K, dq)" in line, n.why
    print(f"{len(NAMES)} names, {len(kernels)} kernels, {len(REACHABLE)} reachable, {len(unreachable)} unreachable")


def test_the_cases_cover_exactly_the_reachable_names():
    got = set()
    for n in REACHABLE:
        for c in I.cases_of(n):
            assert I.predict(c) == n.name, c
            assert c.d in I.dims_of(n.dq) and I.teleport_target(I.cycle_length(c)) >= I.FIRST
            got.add(I.predict(c))
    assert got == {n.name for n in REACHABLE}
    # the device sweep runs all of them but the names held back, each with its reason
    assert set(I.HELD_BACK) <= got and len(I.HELD_BACK) == 4 + 14
    assert {n.name for n in I.swept()} | set(I.HELD_BACK) == got


def test_no_configuration_predicts_an_unreachable_name():
    """The shapes of a grid far wider than the cases: every name they predict is enumerated, and
    none is marked unreachable."""
    known = {n.name: n for n in NAMES}
    seen = set()
    for dq in range(1, 33):
        for d in (4 * dq - 3, 4 * dq):
            if d < 2:
                continue
            for K in range(1, 25):
                for per in (None, [1] + [0] * (d - 1), [1] * d):
                    for cap in (0, 8):
                        for blocks, last, nd in ((None, -1, 0), ([list(range(d - 1)), [d - 1]], -1, 0),
                                                 ([list(range(d - 1)), [d - 1]], 0, 2)):
                            for prior in (0, 1, 2):
                                kw = dict(K=K, periodic=per, cap=cap, blocks=blocks, drag_last_slow=last,
                                          drag_steps=nd, T=1.0)
                                if prior == 1:
                                    kw["b"] = [1.0 + 0.25 * (i % 2) for i in range(d)]
                                elif prior == 2:
                                    kw["kinds"] = [0] + [1] * (d - 1)
                                for duo in (False, True):
                                    name = I.predict_arguments(d, 128, 64, basis_group_size=128, duo=duo, **kw)
                                    if name is not None:
                                        seen.add(name)
    assert seen <= set(known), sorted(seen - set(known))[:5]
    bad = [n for n in seen if known[n].why]
    assert not bad, bad[:5]


def _conditions(c):
    """One case on the oracle alone, stepped one step at a time where a condition needs it.  The
    oracle derives its constants itself here (the device test hands it the engine's, equal to
    rounding): the conditions are counts with margin -- hundreds to thousands of accepted steps, tens
    on the seam or on a one-parameter column -- not properties of single decisions."""
    prob, st = I.oracle_alone(c)
    if prob.c.carry_modes:
        st.anchor_modes()
    W, L = c.W, I.cycle_length(c)
    oned = c.blocks is not None and c.family != I.DRAG and min(len(b) for b in c.blocks[0]) == 1
    single = bool(c.periodic) or oned
    accepted = crossed = on_1d = 0
    rows = np.zeros(W, int)
    for launch, n in enumerate((I.FIRST, I.LONG)):
        if launch == 1:
            st.step = I.teleport_target(L)
        before = int(st.n_accept.sum())
        if single:
            for _ in range(n):
                x0, a0, s = st.x.copy(), st.n_accept.copy(), st.step
                st.run(1, n_threads=1)
                acc = st.n_accept > a0
                if c.periodic:
                    p = list(c.periodic)
                    width = prob.hi[p] - prob.lo[p]
                    crossed += int(np.sum(acc[:, None] & (np.abs(st.x[:, p] - x0[:, p]) > 0.5 * width)))
                if oned:       # (beside `periodic` too: both suffixes, both conditions)
                    for g in range(W // c.bgs):
                        if I.one_parameter_column(prob, c, g, s):
                            on_1d += int(acc[g * c.bgs:(g + 1) * c.bgs].sum())
        else:
            st.run(n, n_threads=4)
        got = int(st.n_accept.sum()) - before
        assert 0 < got < W * n, f"launch {launch}: {got} of {W * n} steps accepted"
        accepted += got
        if c.emit:
            assert np.all(st.n_rows <= st.row_cap), "rows dropped"
            rows += st.n_rows
            st.drain()
    rate = accepted / (W * (I.FIRST + I.LONG))
    assert 0.05 <= rate <= 0.95, f"acceptance {rate:.3f}"
    assert int(st.stuck[0]) == 0
    if c.periodic:
        assert crossed >= 1, "no accepted step crossed the seam"
    if oned:
        assert on_1d >= 1, "no accepted step on a one-parameter column"
    if c.emit:
        assert rows.min() >= 1, f"{int(np.sum(rows == 0))} walkers emitted no row"
    return rate


@pytest.mark.parametrize("family,dq", GROUPS, ids=[f"{f}-dq{q}" for f, q in GROUPS])
def test_every_case_makes_a_wrong_kernel_visible(family, dq):
    """Acceptance within [0.05, 0.95] over the 138 steps; an accepted and a rejected step in
    each launch; `periodic`: an accepted step across the seam; `1-D blocks`: an accepted step on a
    one-parameter column; `emit`: a row of every walker, none dropped; dragging: an accepted
    dragging step (with `1-D blocks` its fast block is the one parameter: every dragging step
    draws the one-parameter variates)."""
    failed = []
    for n in REACHABLE:
        if (n.family, n.dq) != (family, dq):
            continue
        for c in I.cases_of(n):
            try:
                _conditions(c)
            except AssertionError as e:
                failed.append(f"{c.name} d={c.d} seed={c.seed}: {e}")
    assert not failed, "\n".join(failed)


def test_every_padding_occurs_under_three_variants():
    """The instantiations of one dq are dealt round-robin over d = 4 dq - 3 .. 4 dq: every padding
    occurs under floor(n / 4) variants at least, n the reachable names of the (family, dq) -- three
    where there are twelve (step_inc_kernel, drag_inc_kernel, step_inc_mix_kernel with three to five
    KM, step_inc_regs_kernel from dq = 17 on), two for the eight periodic names, one for the six emit
    names and for step_duo_mix_kernel where one KM is left, and for step_inc_any_kernel's two names
    two of the four paddings.  dq = 1 has three paddings (d = 2 .. 4), and dragging at dq = 1 needs
    d >= 3 (d = 4 where the fast block has two parameters).  step_inc_duo_kernel runs at all."""
    for family, dq in GROUPS:
        names = [n for n in REACHABLE if (n.family, n.dq) == (family, dq)]
        ds = [c.d for n in names for c in I.cases_of(n)]
        assert set(ds) <= set(I.dims_of(dq))
        if dq == 1 and family == I.DRAG:
            assert set(ds) == {3, 4}
            continue
        pads = I.dims_of(dq)
        if family == I.DUO_ONE:
            assert all(ds.count(d) == 2 for d in pads)
        elif len(names) >= len(pads):
            assert all(ds.count(d) >= len(names) // len(pads) for d in pads), (family, dq, ds)
            if len(names) >= 12:
                assert all(ds.count(d) >= 3 for d in pads), (family, dq, ds)
        else:
            assert len(set(ds)) == len(names), (family, dq, ds)


# ------------------------------------------------------------------ the enumeration and the build
FAMILY_KERNELS = ("step_inc_kernel", "drag_inc_kernel", "step_inc_mix_kernel", "step_duo_mix_kernel",
                  "step_inc_duo_kernel", "step_inc_regs_kernel", "step_inc_any_kernel")


SCRATCH_KERNELS = ("step_kernel", "drag_kernel", "step_pair_kernel", "step_mfma_kernel", "step_big_reg_kernel")


def _tool(name):
    """An LLVM tool of the ROCm that built the library: beside hipcc, else on the PATH."""
    from cobaya_amd.build import hipcc
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc())))
    for folder in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(folder, name)):
            return os.path.join(folder, name)
    return shutil.which(name)


def kernel_symbols(lib, tmp):
    """The demangled names of the kernels (symbols with a `.kd` descriptor) of every gfx950 code
    object in `lib`: the offload bundles of its .hip_fatbin section, one per translation unit,
    taken apart with clang-offload-bundler.  Symbol tables only (llvm-objdump --syms --demangle,
    which stands in for llvm-nm and llvm-cxxfilt where ROCm ships neither): no disassembly."""
    objcopy, bundler, objdump = (_tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump"))
    assert objcopy and bundler and objdump, "the LLVM tools of ROCm are missing"
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "rest")], check=True)
    with open(fat, "rb") as f:
        blob = f.read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    assert starts
    names = []
    for i, at in enumerate(starts):
        piece, co = os.path.join(tmp, f"bundle{i}"), os.path.join(tmp, f"co{i}")
        with open(piece, "wb") as f:
            f.write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.run([bundler, "--unbundle", "--type=o", f"--input={piece}", f"--output={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
        out = subprocess.run([objdump, "--syms", "--demangle", co], check=True, capture_output=True, text=True).stdout
        os.remove(piece)
        os.remove(co)
        for line in out.splitlines():
            if line.endswith(" (.kd)"):     # (the demangler's spelling of <kernel>.kd)
                names.append(line[:-6].split("\t")[-1].split(" ", 1)[-1])
    return names       # (one entry per kernel and code object)


def test_the_enumeration_is_the_set_of_compiled_kernels(tmp_path):
    """Every kernel of the families in the library's code objects is enumerated, and every
    enumerated kernel (reachable or not) is compiled."""
    from cobaya_amd import engine as E
    lib = E.load_library()._name
    compiled, scratch = set(), {}
    for sym in kernel_symbols(lib, str(tmp_path)):
        m = re.search(r"::(\w+(?:<[^()]*>)?)\(", sym)
        if m and m.group(1).split("<")[0] in FAMILY_KERNELS:
            compiled.add(m.group(1))
        elif m and m.group(1).split("<")[0] in SCRATCH_KERNELS:
            scratch[m.group(1)] = scratch.get(m.group(1), 0) + 1
    want = I.enumerate_kernels()
    assert compiled - want == set(), sorted(compiled - want)[:5]
    assert want - compiled == set(), sorted(want - compiled)[:5]
    # from scratch: the names carry no d -- every kernel in as many code objects as (name, D) units
    assert scratch == I.scratch_kernel_counts()


# ------------------------------------------------------------------ the "before" figure
def suite_before():
    """The names the fixed-seed incremental cases of the committed suite reach, through predict:
    the draws of tests/test_gpu_fuzz.py at their default counts, tests/far_steps.py CASES and the
    parametrised lists of tests/test_gpu_parity.py.  (name or None, where from) per case."""
    from tests import far_steps as F
    from tests import test_gpu_fuzz as Z
    from tests import test_gpu_parity as P
    out = []

    def add(where, d, W, gs, **kw):
        kw.pop("incremental", None)
        out.append((I.predict_arguments(d, W, gs, **kw), where))

    for seed in range(40):
        d, W, gs, K, kw, _ = Z.draw_incremental_case(9000 + seed)
        add("fuzz incremental", d, W, gs, K=K, **kw)
    for seed in range(32):
        d, W, gs, K, kw, _ = Z.draw_general_case(12000 + seed)
        add("fuzz general", d, W, gs, K=K, **kw)
    for seed in range(24):
        d, W, gs, K, kw, _ = Z.draw_two_lane_case(15000 + seed)
        add("fuzz two lanes", d, W, gs, K=K, duo=True, **kw)
    for c in F.CASES:
        if not c.inc:
            continue
        kinds, a, b, periodic, blocking = F.case_setup(c)
        kw = dict(K=c.K, kinds=kinds.tolist(), a=a.tolist(), b=b.tolist(), basis_group_size=c.bgs, duo=c.duo,
                  periodic=None if periodic is None else periodic.tolist())
        if blocking is not None:
            kw.update(blocks=blocking[0], drag_last_slow=blocking[2], drag_steps=blocking[3])
        add("far steps", c.d, c.W, c.gs, **kw)

    def params(fn):
        return [m for m in fn.pytestmark if m.name == "parametrize"][0].args[1]

    def prior(d, normal):
        if normal == "bounds differ":
            return dict(a=[-0.25 * (i % 3) for i in range(d)], b=[1.0 + 0.5 * (i % 2) for i in range(d)])
        if normal == "box off the origin":
            return dict(a=[2.0 ** -12] * d, b=[1.5] * d)
        if normal == "tight":
            return dict(a=[0.44 if i % 5 == 0 else 0.0 for i in range(d)], b=[1.0] * d)
        return dict(kinds=[0] * (d - 1) + [1]) if normal else {}

    for d, W, gs, normal, T in params(P.test_incremental_steps_bit_exact):
        add("parity steps", d, W, gs, T=T, **prior(d, normal))
    for fn in (P.test_directions_computed_ahead_never_change_the_results,
               P.test_calls_of_several_launches_refresh_y_inside_the_step_kernel):
        for d, W, gs, kw in params(fn):
            add("parity " + fn.__name__[5:25], d, W, gs, **kw)
    for d, W, gs, kw in params(P.test_incremental_emitted_rows_bit_exact):
        add("parity rows", d, W, gs, cap=80, **kw)
    for d, W, gs, thin, kw in params(P.test_rows_thinned_on_the_device_bit_exact):
        add("parity thinned rows", d, W, gs, cap=80, **kw)
    for fn, duo in ((P.test_incremental_mixture_steps_bit_exact, False), (P.test_two_lane_mixture_steps_bit_exact, True)):
        for d, W, gs, K, normal, T in params(fn):
            add("parity mixtures", d, W, gs, K=K, T=T, duo=duo, **prior(d, normal))
    for fn in (P.test_incremental_general_kernel_steps_bit_exact, P.test_incremental_periodic_steps_bit_exact):
        for p in params(fn):
            d, W, gs = p[:3]
            K, per, extra = (p[3], p[4], dict(p[5])) if len(p) == 6 else (1, p[3], dict(p[4]))
            periodic = [int(i in per) for i in range(d)]
            kw = dict(a=[0.42 if q else 0.0 for q in periodic], b=[0.58 if q else 1.0 for q in periodic])
            if extra.pop("normal", False):
                kw["kinds"] = [int(not q) for q in periodic]
            if "bgs" in extra:
                kw["basis_group_size"] = extra.pop("bgs")
            add("parity general / periodic", d, W, gs, K=K, periodic=periodic if per else None, **kw, **extra)
    for d, W, gs, K, blocks, over in params(P.test_incremental_blocked_oversampled_steps_bit_exact):
        add("parity blocks", d, W, gs, K=K, blocks=blocks)
    for d, W, gs, blocks, last_slow, n_drag, extra in params(P.test_incremental_dragging_steps_bit_exact):
        add("parity dragging", d, W, gs, blocks=blocks, drag_last_slow=last_slow, drag_steps=n_drag, **extra)
    for d, W, gs, bgs, kw in params(P.test_wide_basis_groups_bit_exact):
        add("parity wide groups", d, W, gs, basis_group_size=bgs, **kw)
    return out


def test_the_suite_before_this_sweep_reports_its_coverage():
    """Reported, not asserted (docs/MEASUREMENTS.md, "Every instantiation once"): how many of the
    reachable names the fixed-seed incremental cases of the suite had reached."""
    cases = suite_before()
    known = {n.name for n in NAMES}
    names = {n for n, _ in cases if n is not None}
    assert names <= known, sorted(names - known)
    kernels = {k for n in NAMES if n.name in names for k in n.kernels}
    print(f"before: {len(cases)} fixed-seed incremental cases reach {len(names)} distinct names of "
          f"{len(REACHABLE)} reachable ({len(NAMES)} enumerated), at most {len(kernels)} kernels of "
          f"{len(I.enumerate_kernels())}")
    assert len(cases) > 200 and len(names) > 50


# ------------------------------------------------------------------ every trial from scratch
SNAMES = I.enumerate_scratch()
SREACHABLE = [n for n in SNAMES if not n.why]
SGROUPS = sorted({(n.family, n.D) for n in SREACHABLE}, key=lambda g: (I.S_FAMILIES.index(g[0]), g[1]))


def test_the_from_scratch_tables_and_their_cases():
    """(name, compiled D or DP): 32 x 8 of walker_kernels.hip's lane-per-walker kernels, 56 x 4
    two-wave kernels, 11 x 2 + 9 of walker_kernels_big.hip; the cases cover exactly the reachable."""
    assert len({(n.name, n.D) for n in SNAMES}) == len(SNAMES) == 32 * 8 + 56 * 4 + 11 * 2 + 9
    assert len(SNAMES) - len(SREACHABLE) == 6 + 13 * 4 + 2 * 2
    # unreachable is proved by exhaustion: over the grid of tests/instantiations.py (every d, so every
    # shape of a unit's D or DP) mcmc_hip_scratch_choice never answers a unit marked unreachable, and
    # answers every other one at least once
    seen, _, _ = I.scratch_grid_census()
    for n in SNAMES:
        assert ((n.name, n.D) in seen) == (not n.why), (n.name, n.D, n.why)
        assert not n.why or n.why.startswith(I.SCRATCH_CHOICE + " "), n.why
    assert {u for u in seen if u[0] and "general" not in u[0]} == {(n.name, n.D) for n in SREACHABLE}
    got = set()
    for n in SREACHABLE:
        for c in I.scratch_cases_of(n):
            assert I.predict_scratch(c) == (n.name, n.D), c
            got.add(I.predict_scratch(c))
        ds = [c.d for c in I.scratch_cases_of(n)]
        if n.family in (I.S_MFMA, I.S_BIG):      # the smallest and the largest d of the DP that reach it
            lo, hi = I.dims_of_dp(n.D)[0], n.D
            assert ds[-1] == hi and lo <= ds[0] and (ds[0] == lo or (n.D == 48 and n.family == I.S_MFMA))
            for d in range(lo, ds[0]):
                assert I.predict_scratch(I._scratch_case(n, d))[0].startswith("mcmc::step_pair_kernel")
        else:
            assert ds == [n.D]
    assert got == {(n.name, n.D) for n in SREACHABLE}
    print(f"from scratch: {len(SNAMES)} (name, D) units, {len(SREACHABLE)} reachable, "
          f"{sum(len(I.scratch_cases_of(n)) for n in SREACHABLE)} cases")


@pytest.mark.parametrize("family,D", SGROUPS, ids=[f"{f}-D{q}" for f, q in SGROUPS])
def test_every_from_scratch_case_makes_a_wrong_kernel_visible(family, D):
    """Acceptance within [0.05, 0.95] over the 5 + (d + 7) steps, an accepted and a rejected step
    in each launch (dragging: an accepted dragging step)."""
    failed = []
    for n in SREACHABLE:
        if (n.family, n.D) != (family, D):
            continue
        for c in I.scratch_cases_of(n):
            prob, st = I.scratch_oracle_alone(c)
            total = 0
            for launch, steps in enumerate(I.scratch_steps(c)):
                before = int(st.n_accept.sum())
                st.run(steps, n_threads=4)
                got = int(st.n_accept.sum()) - before
                total += got
                if not 0 < got < c.W * steps:
                    failed.append(f"{c.name} d={c.d}: launch {launch}: {got} of {c.W * steps} accepted")
            rate = total / (c.W * sum(I.scratch_steps(c)))
            if not 0.05 <= rate <= 0.95:
                failed.append(f"{c.name} d={c.d}: acceptance {rate:.3f}")
    assert not failed, "\n".join(failed)


def test_the_general_kernel_cases_reach_them_and_make_a_wrong_kernel_visible():
    """tests/instantiations.py: general_cases (run by tests/test_gpu_scratch_general.py): the rule and its
    restatement send each to step_general_kernel / drag_general_kernel; on the oracle alone each
    launch accepts and rejects, acceptance within [0.05, 0.95]; the emitting ones emit."""
    from cobaya_amd import engine as E
    cases = I.general_cases()
    assert len(cases) == 13 and {c.d for c in cases} == {33, 113, 128}
    for c in cases:
        assert I.predict_scratch(c) == (c.name, 0) == I.scratch_name_of(E.scratch_choice(**I.scratch_shape_of(c))), c
        prob, st = I.scratch_oracle_alone(c)
        total = 0
        for steps in I.scratch_steps(c):
            before = int(st.n_accept.sum())
            st.run(steps, n_threads=4)
            got = int(st.n_accept.sum()) - before
            total += got
            assert 0 < got < c.W * steps, c
        assert 0.05 <= total / (c.W * sum(I.scratch_steps(c))) <= 0.95, c
        if c.emit:
            assert len(st.drain()) > c.W

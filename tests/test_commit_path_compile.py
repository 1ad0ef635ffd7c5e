"""The commit of step_inc_duo_kernel (incremental_duo.hip: one mode, two lanes per walker) as the compiler lays it
out (round 20): it runs under the accept mask -- x takes the trial by 64-bit moves, y moves on by one FMA per dimension
with r itself --, its block lies in front of the loop's latch and falls through into it, and nothing between the step's
reads and the latch jumps backwards or unconditionally.  Read off the assembly with tools/check_step_path.py and
tools/check_duo1_spills.py.  CPU only: hipcc cross-compiles."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FMA = re.compile(r"^v_(?:fma|fmac)_f64(?:_e32|_e64)?\s+v\[(\d+):\d+\],\s*(.*)$")
MOV = re.compile(r"^v_mov_b64(?:_e32|_e64)?\s+v\[(\d+):\d+\],\s*v\[(\d+):\d+\]")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")


@pytest.fixture(scope="module")
def asm():
    import check_step_path as C
    return C.compile_to_asm(1, 8)


def _registers(asm_text):
    import check_duo1_spills as S
    return {(r["dq"], r["ne"], r["unit_t"]): r for r in S.report(asm_text)}


def _branch_shape(lines, p):
    """every conditional branch between the reads and the latch is forward, the latch is the one backward branch, and
    there is no s_branch"""
    at = {LABEL.match(t).group(1): i for i, t in lines if LABEL.match(t)}
    seen = 0
    for i, t in lines:
        b = BRANCH.match(t)
        if not b:
            continue
        seen += 1
        assert b.group(1) != "s_branch", t
        if i == p["back_edge"]:
            continue
        # forward: to a label further down in this stretch, or to a block behind the latch (not in `at`: a rare case)
        assert at.get(b.group(2), 1 << 60) > i, (t, "jumps backwards")
    assert seen >= 1 and lines[-1][0] == p["back_edge"]


def test_the_headline_commit_moves_x_and_runs_in_front_of_the_latch(asm):
    import check_step_path as C
    NE = 15
    regs = _registers(asm)[(8, NE, True)]
    assert regs["spilled"] == 0 and regs["scratch_in_loop"] == 0, regs
    assert regs["vgprs"] <= 256, regs   # two waves per SIMD
    p, lines = C.step_lines(asm, 8, NE, True)
    assert p is not None
    print(p)
    _branch_shape(lines, p)
    assert p["s_branch"] == [] and p["taken"] == [] and p["s_load"] == []
    fmas = [(i, FMA.match(t)) for i, t in lines if FMA.match(t)]
    # NE trials, NE y . u, NE of the commit's y, two of the log-likelihood (the parent: 4 NE + 2 = 62)
    assert len(fmas) == 3 * NE + 2, [t for i, t in lines if FMA.match(t)]
    # the commit: the block of the one guard, from its s_cbranch_execz to its label
    assert len(p["guards"]) == 1, p
    g0 = next(i for i, t in lines if t == p["guards"][0])
    g1 = next(i for i, t in lines if LABEL.match(t) and LABEL.match(t).group(1) == BRANCH.match(p["guards"][0]).group(2))
    assert g0 < g1 <= p["back_edge"]
    block = [(i, t) for i, t in lines if g0 < i < g1]
    moved = {int(MOV.match(t).group(1)): int(MOV.match(t).group(2)) for i, t in block if MOV.match(t)}
    in_block = [m for i, m in fmas if g0 < i < g1]
    # (the trials stand in the ladder of waits, in front of the support test's branch; the log-likelihood's two FMAs,
    # whose result the block also moves, behind it)
    support = next(i for i, t in lines if BRANCH.match(t))
    assert support < g0
    trials = [m for i, m in fmas if i < support]
    # x: the addend of a trial FMA (the third source) that the block overwrites with that FMA's result
    x_regs = set()
    for m in trials:
        srcs = re.findall(r"v\[(\d+):\d+\]", m.group(2))
        if len(srcs) == 3 and moved.get(int(srcs[2])) == int(m.group(1)):
            x_regs.add(int(srcs[2]))
    assert len(x_regs) == NE, (sorted(x_regs), moved)
    assert len(in_block) == NE and not {int(m.group(1)) for m in in_block} & x_regs
    # nothing is selected lane by lane inside the block, and the block falls through into the latch's block
    assert not [t for i, t in block if t.startswith("v_cndmask")]
    assert not [t for i, t in block if BRANCH.match(t) or LABEL.match(t)]


@pytest.mark.parametrize("dq,ne", [(1, 1), (1, 2), (4, 7)])
@pytest.mark.parametrize("unit_t", [True, False])
def test_the_smallest_and_an_odd_instantiation_keep_the_shape(asm, dq, ne, unit_t):
    import check_step_path as C
    regs = _registers(asm)[(dq, ne, unit_t)]
    assert regs["spilled"] == 0 and regs["scratch_in_loop"] == 0, regs
    p, lines = C.step_lines(asm, dq, ne, unit_t)
    assert p is not None
    _branch_shape(lines, p)
    assert p["s_branch"] == [] and p["taken"] == [], p

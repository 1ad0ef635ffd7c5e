"""The common path of a step of step_inc_duo_kernel (incremental_duo.hip: one mode, two lanes per walker) is
straight-line code from the step's LDS reads to the back-edge of the step loop: no scalar load (|u|^2 comes from the
chunk's LDS), no unconditional branch, and no conditional branch that a common step takes -- the rare cases (a trial in
doubt at the wall, an accept in doubt, a burning wave) are laid out behind the loop (tools/check_step_path.py).
CPU only: hipcc cross-compiles."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAME = "_ZN4mcmc12_GLOBAL__N_119step_inc_duo_kernelILi8ELi15ELb1ELb1EEEvNS_11IncStepArgsE"


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_step_path as C
    return C


def test_the_headline_step_runs_straight_from_its_reads_to_the_back_edge():
    C = _tool()
    rows = C.report(C.compile_to_asm(1, 8))
    assert {r["dq"] for r in rows} == set(range(1, 9))
    head = [r for r in rows if C.is_headline(r)]
    assert len(head) == 1
    p = head[0]["path"]
    assert p is not None, "no run of 16 ds_read_b128 with a back-edge behind it in the step loop"
    print(p)
    assert p["s_load"] == [], p
    assert p["s_branch"] == [], p
    assert p["taken"] == [], p
    assert C.straight(head[0])
    # every instantiation has a step loop the tool can read
    assert [(r["dq"], r["ne"], r["unit_t"]) for r in rows if r["path"] is None] == []


def _kernel(step_blocks, reads=16):
    rd = "".join(f"\tds_read_b128 v[{4 * i}:{4 * i + 3}], v192 offset:{32 * i}\n" for i in range(reads))
    return (f"{NAME}:                    ; @{NAME}\n"
            "\ts_nop 0\n"
            ".LBB0_3:        ; =>This Loop Header: Depth=1\n"
            "\ts_nop 0\n" + step_blocks.format(reads=rd) + "\ts_endpgm\n")


def test_a_taken_branch_a_scalar_load_and_a_rotated_loop_are_told_apart():
    C = _tool()
    # the wanted shape: the header holds the reads, rare blocks lie behind the back-edge and jump back
    good = _kernel(".LBB0_5:        ;   Parent Loop BB0_3 Depth=1\n"
                   "                ; =>  This Inner Loop Header: Depth=2\n"
                   "\tds_read_b64 v[200:201], v190\n{reads}"
                   "\ts_waitcnt lgkmcnt(11)\n\tv_fma_f64 v[100:101], v[0:1], v[4:5], v[8:9]\n"
                   "\ts_cbranch_scc0 .LBB0_7\n"
                   ".LBB0_6:        ;   in Loop: Header=BB0_5 Depth=2\n"
                   "\tv_add_f64 v[0:1], v[0:1], v[2:3]\n"
                   "\ts_cbranch_scc0 .LBB0_5\n"
                   "\ts_branch .LBB0_8\n"
                   ".LBB0_7:        ;   in Loop: Header=BB0_5 Depth=2\n"
                   "\ts_load_dwordx2 s[0:1], s[2:3], 0x0\n"
                   "\ts_branch .LBB0_6\n"
                   ".LBB0_8:\n")
    r, = C.report(good)
    assert C.is_headline(r) and C.straight(r), r
    assert r["path"]["instructions"] == 5 and r["path"]["taken"] == [] and r["path"]["s_load"] == []
    # a join of the common path reached by a taken branch, with a scalar load and a jump on the way
    bad = _kernel(".LBB0_5:        ;   Parent Loop BB0_3 Depth=1\n"
                  "                ; =>  This Inner Loop Header: Depth=2\n"
                  "{reads}"
                  "\ts_waitcnt lgkmcnt(11)\n"
                  "\ts_load_dwordx2 s[0:1], s[2:3], 0x0\n"
                  "\ts_cbranch_scc1 .LBB0_7\n"
                  "; %bb.6:        ;   in Loop: Header=BB0_5 Depth=2\n"
                  "\tv_cmp_ge_f64_e32 vcc, s[58:59], v[6:7]\n"
                  "\ts_branch .LBB0_7\n"
                  ".LBB0_7:        ;   in Loop: Header=BB0_5 Depth=2\n"
                  "\tv_add_f64 v[0:1], v[0:1], v[2:3]\n"
                  "\ts_cbranch_scc0 .LBB0_5\n")
    r, = C.report(bad)
    assert not C.straight(r)
    assert r["path"]["s_load"] == ["s_load_dwordx2 s[0:1], s[2:3], 0x0"]
    assert r["path"]["s_branch"] == ["s_branch .LBB0_7"]
    assert r["path"]["taken"] == ["s_cbranch_scc1 .LBB0_7"]
    # a rotated loop (the commit block on top, entered by a backward branch from the bottom): the back-edge is the
    # first backward branch to the run or in front of it, and the forward join in front of it counts as taken
    rotated = _kernel(".LBB0_4:        ;   in Loop: Header=BB0_5 Depth=2\n"
                      "\tv_add_f64 v[0:1], v[0:1], v[2:3]\n"
                      "\ts_cbranch_scc1 .LBB0_9\n"
                      ".LBB0_5:        ;   Parent Loop BB0_3 Depth=1\n"
                      "                ; =>  This Loop Header: Depth=2\n"
                      "{reads}"
                      "\ts_cbranch_scc1 .LBB0_7\n"
                      "; %bb.6:        ;   in Loop: Header=BB0_5 Depth=2\n"
                      "\tv_cmp_ge_f64_e32 vcc, s[58:59], v[6:7]\n"
                      ".LBB0_7:        ;   in Loop: Header=BB0_5 Depth=2\n"
                      "\ts_cbranch_execz .LBB0_4\n"
                      "; %bb.8:        ;   in Loop: Header=BB0_5 Depth=2\n"
                      "\ts_branch .LBB0_4\n"
                      ".LBB0_9:\n")
    r, = C.report(rotated)
    assert r["path"]["taken"] == ["s_cbranch_scc1 .LBB0_7"] and not C.straight(r)
    # no run of the expected length (fifteen reads where the instantiation has sixteen): nothing to read off
    r, = C.report(_kernel(".LBB0_5:        ; =>  This Loop Header: Depth=2\n{reads}\ts_cbranch_scc0 .LBB0_5\n", reads=15))
    assert r["path"] is None and not C.straight(r)

"""The variate burst of step_inc_duo_kernel (incremental_duo.hip, det_math.h OctetRng) as compiled for the headline
instantiation <8, 15, true, true>: between the octet test and the first step's run of reads the lane half's two Philox
blocks and four variates are ONE straight-line block -- no branch between the first Philox multiply and the variate
stores --, the four reads of the short-log table stand in one run and are retired by counted waits, not by
lgkmcnt(0) each, and the lowest-bin test is one conditional branch behind the stores to a block laid out further
down.  At most 256 VGPRs, no scratch (tools/check_burst.py).  CPU only: hipcc cross-compiles."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAME = "_ZN4mcmc12_GLOBAL__N_119step_inc_duo_kernelILi8ELi15ELb1ELb1EEEvNS_11IncStepArgsE"


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_burst as C
    return C


def test_the_headline_burst_is_one_straight_line_block_with_its_table_reads_in_one_run():
    C = _tool()
    rows = C.report(C.compile_to_asm(1, 8))
    assert {r["dq"] for r in rows} == set(range(1, 9))
    head = [r for r in rows if C.is_headline(r)]
    assert len(head) == 1
    r = head[0]
    b = r["burst"]
    print(r)
    assert b is not None, "no variate stores in front of the step's run of reads"
    # both Philox blocks in the block that ends in the stores -- rounds 3 to 10 of two blocks are 32 products of each
    # kind, the rounds before share some (tools/check_burst.py) --, none of them in front of it: no branch from the
    # first multiply on; the pair v_mul_hi_u32 / v_mul_lo_u32 kept
    assert b["mul_hi"] >= 32 and b["mul_lo"] >= 32 and b["mul_hi_in_front"] == 0 and b["mad_u64"] == 0, b
    assert b["stores"] == 4, b
    # the four table reads: one run (so no wait between them), retired by counted waits
    assert b["table_reads"] == 4 and b["one_run"], b
    assert len(b["waits"]) >= 2 and all(n > 0 for n in b["waits"][:-1]), b
    assert b["rsq"] == 4 and b["logf"] == 4, b
    # the lowest-bin test: behind the stores, conditional, forward
    assert b["low_bin"] is not None and b["low_bin"]["conditional"] and b["low_bin"]["forward"], b
    assert r["vgprs"] <= 256 and r["scratch"] == 0 and b["scratch_insts"] == 0, r
    assert C.interleaved(r)
    # every instantiation draws this way, within the registers
    for r in rows:
        assert r["burst"] is not None and r["burst"]["table_reads"] == 4 and r["burst"]["one_run"], r
        assert r["burst"]["mul_hi"] >= 32 and r["burst"]["mul_hi_in_front"] == 0 and r["burst"]["stores"] == 4, r
        assert r["vgprs"] <= 256 and r["scratch"] == 0 and r["burst"]["scratch_insts"] == 0, r


def _kernel(burst, vgprs=214, scratch=0):
    rd = "".join(f"\tds_read_b128 v[{4 * i}:{4 * i + 3}], v192 offset:{32 * i}\n" for i in range(16))
    return (f"{NAME}:                    ; @{NAME}\n"
            "\ts_nop 0\n"
            ".LBB0_3:        ; =>This Loop Header: Depth=1\n"
            "\ts_cmp_eq_u64 s[72:73], s[70:71]\n"
            "\ts_cbranch_scc1 .LBB0_5\n"
            "; %bb.4:        ;   in Loop: Header=BB0_3 Depth=1\n" + burst +
            ".LBB0_5:        ;   Parent Loop BB0_3 Depth=1\n"
            "                ; =>  This Inner Loop Header: Depth=2\n" + rd +
            "\ts_waitcnt lgkmcnt(11)\n\tv_fma_f64 v[100:101], v[0:1], v[4:5], v[8:9]\n"
            "\ts_cbranch_scc0 .LBB0_5\n"
            "\ts_branch .LBB0_3\n"
            ".LBB0_9:\n\tv_rsq_f64_e32 v[2:3], v[0:1]\n\ts_branch .LBB0_5\n"
            "\ts_endpgm\n"
            "\t.amdhsa_kernel " + NAME + "\n"
            f"\t\t.amdhsa_next_free_vgpr {vgprs}\n\t\t.amdhsa_private_segment_fixed_size {scratch}\n"
            "\t.end_amdhsa_kernel\n")


PHILOX = "\tv_mul_hi_u32 v2, v2, s79\n\tv_mul_lo_u32 v0, v0, s79\n" * 40
TAIL = ("\tv_log_f32_e32 v2, v2\n" * 4 + "\ts_waitcnt lgkmcnt(3)\n\tv_fma_f64 v[4:5], v[4:5], v[20:21], -1.0\n"
        "\ts_waitcnt lgkmcnt(0)\n" + "\tv_rsq_f64_e32 v[26:27], v[8:9]\n" * 4 +
        "".join(f"\tds_write_b128 v193, v[{4 * i}:{4 * i + 3}] offset:{528 * i}\n" for i in range(4)) +
        "\ts_cbranch_vccnz .LBB0_9\n")


def test_a_split_run_a_branch_in_the_burst_and_a_wait_per_read_are_told_apart():
    C = _tool()
    reads = "".join(f"\tds_read_b128 v[{20 + 4 * i}:{23 + 4 * i}], v{6 + i}\n" for i in range(4))
    r, = C.report(_kernel(PHILOX + reads + TAIL))
    assert C.is_headline(r) and C.interleaved(r), r
    assert r["burst"]["waits"] == [3, 0] and r["burst"]["block"] == 80 + 4 + 4 + 3 + 4 + 4
    # an instruction between the reads: no run
    split = reads.replace("\tds_read_b128 v[28:31], v8\n", "\tv_and_b32_e32 v8, 0x7f, v8\n\tds_read_b128 v[28:31], v8\n")
    r, = C.report(_kernel(PHILOX + split + TAIL))
    assert r["burst"]["table_reads"] == 4 and not r["burst"]["one_run"] and not C.interleaved(r)
    # a branch between the Philox rounds and the stores (the rolled loop's lowest-bin test): the block begins behind it
    r, = C.report(_kernel(PHILOX + "\ts_cbranch_vccz .LBB0_8\n.LBB0_8:\n" + reads + TAIL))
    assert r["burst"]["mul_hi"] == 0 and r["burst"]["mul_hi_in_front"] == 40 and not C.interleaved(r)
    # every read waited for by lgkmcnt(0)
    r, = C.report(_kernel(PHILOX + reads + TAIL.replace("lgkmcnt(3)", "lgkmcnt(0)")))
    assert r["burst"]["waits"] == [0, 0] and not C.interleaved(r)
    # a lowest-bin branch that jumps back, scratch, too many registers
    r, = C.report(_kernel(PHILOX + reads + TAIL.replace(".LBB0_9", ".LBB0_3")))
    assert not r["burst"]["low_bin"]["forward"] and not C.interleaved(r)
    r, = C.report(_kernel(PHILOX + reads + TAIL, scratch=16))
    assert not C.interleaved(r)
    r, = C.report(_kernel(PHILOX + reads + TAIL, vgprs=260))
    assert not C.interleaved(r)

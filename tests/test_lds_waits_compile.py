"""step_inc_duo_kernel (incremental_duo.hip: one mode, two lanes per walker) issues the LDS reads of a step up
front and must wait for them by their count -- its first fma behind the first two reads, not behind all
sixteen --, which it does as long as the compiler counts neither the staging's LDS-DMA nor a scalar load
across them (incremental_common.h: stage16_dma; tools/check_lds_waits.py).  CPU only: hipcc cross-compiles."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_headline_step_waits_for_its_lds_reads_by_count():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_waits as C
    rows = C.report(C.compile_to_asm(1, 8))
    assert {r["dq"] for r in rows} == set(range(1, 9))
    head = [r for r in rows if C.is_headline(r)]
    assert len(head) == 1
    ladders = head[0]["ladders"]
    # the step's run: the variate pair and the 15 (v, u) pairs of d = 30
    step = [(label, reads, waits) for label, reads, waits in ladders if reads == 16]
    assert len(step) == 1, ladders
    waits = step[0][2]
    assert waits[0] >= 11 and waits == sorted(waits, reverse=True) and 0 in waits, waits
    # the compiler waits for no vector-memory operation inside the chunk loop: the DMA of the next chunk travels
    # through the whole chunk (every instantiation)
    assert [(r["dq"], r["ne"], r["chunk_vmcnt"]) for r in rows if r["chunk_vmcnt"]] == []
    # no instantiation waits with lgkmcnt(0) alone behind a run of six reads or more
    assert [r for r in rows if any(reads >= 6 for _, reads, _ in r["ladders"]) and not C.counted(r)] == []


def test_a_run_waited_for_with_zero_alone_is_told_apart():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_waits as C
    name = "_ZN4mcmc12_GLOBAL__N_119step_inc_duo_kernelILi8ELi15ELb1ELb1EEEvNS_11IncStepArgsE"
    reads = "".join(f"\tds_read_b128 v[{4 * i}:{4 * i + 3}], v192 offset:{32 * i}\n" for i in range(16))
    body = lambda waits: (f"{name}:                    ; @{name}\n.LBB0_1:        ; =>  This Loop Header: Depth=2\n" + reads +
                          "".join(f"\ts_waitcnt lgkmcnt({n})\n\tv_fma_f64 v[100:101], v[0:1], v[4:5], v[8:9]\n" for n in waits) +
                          "\ts_endpgm\n")
    flat, = C.report(body([0]))
    ladder, = C.report(body([14, 13, 0]))
    assert C.is_headline(flat) and not C.counted(flat) and flat["ladders"] == [(".LBB0_1", 16, [0])]
    chunk = ("\ts_nop 0\n.LBB0_7:       ; =>This Loop Header: Depth=1\n        ;     Child Loop BB0_9 Depth 2\n\ts_nop 0\n"
             "; %bb.8:        ;   in Loop: Header=BB0_7 Depth=1\n{}\ts_branch .LBB0_9\n")
    assert C.chunk_vmcnt(chunk.format("\ts_waitcnt vmcnt(0)\n")) == ["s_waitcnt vmcnt(0)"]
    assert C.chunk_vmcnt(chunk.format("\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\ts_waitcnt lgkmcnt(0)\n")) == []
    assert C.counted(ladder) and ladder["ladders"] == [(".LBB0_1", 16, [14, 13, 0])]

"""step_inc_duo_kernel (incremental_duo.hip, round 7: one mode, two lanes per walker) keeps x, y and the
step's (v, u) pairs of up to 16 dimensions per lane in registers at two waves per SIMD; its step loop must
compile without scratch traffic (tools/check_duo1_spills.py).  CPU only: hipcc cross-compiles."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_mode_two_lane_step_loops_do_not_touch_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_duo1_spills as C
    rows = C.report(C.compile_to_asm(1, 8))
    # every dq = 1 .. 8 with both temperatures; d = 30 (dq = 8, 15 dimensions per lane) among them
    assert {r["dq"] for r in rows} == set(range(1, 9))
    assert any(r["dq"] == 8 and r["ne"] in (15, 16) and r["unit_t"] for r in rows)
    assert [r for r in rows if r["scratch_in_loop"] or r["scratch_stores_in_loop"]] == []
    assert all(r["vgprs"] is not None and r["vgprs"] <= 256 for r in rows)

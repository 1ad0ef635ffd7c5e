"""What the register allocator did to step_inc_duo_kernel (incremental_duo.hip, one mode on two lanes per
walker): the kernel runs at 256 VGPRs per lane (two waves per SIMD) with x, y and the step's (v, u) pairs
-- 8 NE doubles, NE = ceil(d / 2) or 2 dq dimensions per lane -- in them.  Compiles the kernels of
dq = 1 .. 8 to assembly with the build's flags and reports, per instantiation, VGPRs, spilled registers
and the scratch instructions inside the step loop (every block the compiler marks `Depth=2` or deeper).
    python tools/check_duo1_spills.py        exit code 1 if a step loop touches scratch"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_asm import duo_to_asm as compile_to_asm, kernels_matching  # noqa: E402


def report(asm_text):
    """[{dq, ne, split, unit_t, vgprs, spilled, scratch_in_loop, scratch_stores_in_loop}]"""
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S*step_inc_duo_kernel\S+)\n(?:.*\n){0,10}?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", asm_text):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    out = []
    for m, lines in kernels_matching(asm_text, r"(_ZN4mcmc\S*step_inc_duo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E\S*)$"):
        in_loop, n, n_st = False, 0, 0
        for line in lines:
            b = re.match(r"^\.LBB\d+_\d+:.*Depth=(\d+)", line)
            if b or re.match(r"^\.LBB\d+_\d+:", line):
                in_loop = bool(b) and int(b.group(1)) >= 2
            elif re.match(r"^\s*;\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", line):
                # (a loop header inside other loops: the label's line names the outermost parent's depth)
                in_loop = int(re.search(r"Depth=(\d+)", line).group(1)) >= 2
            elif in_loop and line.strip().startswith("scratch_"):
                n += 1
                n_st += line.strip().startswith("scratch_store")
        vg, sp = meta.get(m.group(1), (None, None))
        out.append({"dq": int(m.group(2)), "ne": int(m.group(3)), "split": m.group(4) == "1",
                    "unit_t": m.group(5) == "1", "vgprs": vg, "spilled": sp, "scratch_in_loop": n,
                    "scratch_stores_in_loop": n_st})
    return out


if __name__ == "__main__":
    rows = report(compile_to_asm(1, 8))
    for r in rows:
        print(r)
    sys.exit(1 if any(r["scratch_in_loop"] for r in rows) or not rows else 0)

"""The variate burst of step_inc_duo_kernel (incremental_duo.hip; det_math.h OctetRng), read off the assembly: between
the octet test and the first step's run of reads a lane half draws the four variates of its two Philox blocks as ONE
straight-line block that ends in the four variate stores.  Reports, per instantiation:
    block         instructions of the straight-line block in front of the variate stores (from the last label or branch)
    mul_hi/lo     v_mul_hi_u32 / v_mul_lo_u32 in it.  Two Philox blocks of ten rounds have 40 products; the compiler
                  hoists the first round's product with the walker id out of the step loop and forms once what the
                  two blocks share while their counter words agree (the first two rounds): rounds 3 to 10 of both
                  blocks are 32 of each kind.  `mul_hi_in_front`: those between the loop header in front of the
                  block and the block (a branch between the first multiply and the stores would leave some there);
                  `mad_u64`: v_mad_u64_u32 in the block (the 64-bit form measured slower: det_math.h, StepRng::round)
    table_reads   the ds_read_b128 in it (the short-log table: four), `one_run` if nothing stands between them
    waits         the s_waitcnt lgkmcnt(n) between the reads and the stores: counted (n > 0) but the last
    rsq, logf     v_rsq_f64 / v_log_f32 in it (four each)
    stores        the run of ds_write_b128 at its end (four)
    low_bin       the first branch behind the stores: the lowest-bin test -- conditional, to a label laid out behind it
    vgprs, scratch   of the kernel (next_free_vgpr, private_segment_fixed_size) and its scratch_ instructions
    python tools/check_burst.py        exit code 1 if the headline instantiation <8, 15, true, true> misses the shape"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_asm import duo_to_asm as compile_to_asm, split_kernels  # noqa: E402
from check_step_path import BRANCH, HEADER, LABEL  # noqa: E402

KERNEL = re.compile(r"_ZN4mcmc\S*step_inc_duo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E")
WAIT = re.compile(r"^s_waitcnt\b.*lgkmcnt\((\d+)\)")


def burst(kernel_text, reads):
    """The straight-line block that ends in the variate stores -- the first run of four ds_write_b128, with the step's
    run of `reads` ds_read_b128 behind it --, as the dict of the module's docstring; None without such stores or run."""
    rows = [(i, ln.split(";")[0].strip(), ln.strip()) for i, ln in enumerate(kernel_text.split("\n"))]
    at = {m.group(1): i for i, _, full in rows for m in [LABEL.match(full)] if m}
    code = [(i, t) for i, t, full in rows if t and not t.startswith(".") or LABEL.match(full)]

    def runs(prefix):   # [(first, last)] of the runs of consecutive instructions that begin with `prefix`, as indices of `code`
        out, k = [], 0
        while k < len(code):
            if code[k][1].startswith(prefix):
                j = k
                while j + 1 < len(code) and code[j + 1][1].startswith(prefix):
                    j += 1
                out.append((k, j))
                k = j
            k += 1
        return out
    # the variate stores: the first run of four ds_write_b128 with the step's run of `reads` ds_read_b128 behind it (at
    # NE = 3 the step has four reads, as the burst has table reads: the step's are those behind the stores)
    four = [(a, b) for a, b in runs("ds_write_b128") if b - a == 3]
    if not four or not any(a > four[0][1] and b - a == reads - 1 for a, b in runs("ds_read_b128")):
        return None
    before = code[:four[0][1] + 1]
    end = len(before) - 1
    k = end
    while k > 0 and not (BRANCH.match(before[k - 1][1]) or LABEL.match(before[k - 1][1])):
        k -= 1
    block = before[k:end + 1]
    texts = [t for _, t in block]
    head = max((i for i, _, full in rows if i < block[0][0] and HEADER.match(full)), default=0)
    in_front = sum(t.startswith("v_mul_hi_u32") for i, t in code if head < i < block[0][0])
    rd = [n for n, t in enumerate(texts) if t.startswith("ds_read_b128")]
    stores = 0
    while stores < len(texts) and texts[-1 - stores].startswith("ds_write_b128"):
        stores += 1
    waits = [int(WAIT.match(t).group(1)) for t in texts[(rd[-1] if rd else 0):] if WAIT.match(t)]
    behind = [(i, t) for i, t in code if i > block[-1][0]]
    low = next(((i, t) for i, t in behind if BRANCH.match(t)), None)
    low_bin = None
    if low is not None:
        b = BRANCH.match(low[1])
        low_bin = {"branch": low[1], "conditional": b.group(1) != "s_branch", "forward": at.get(b.group(2), -1) > low[0],
                   "instructions_between": sum(1 for i, t in behind if i < low[0] and not LABEL.match(t))}
    return {"block": len(texts),
            "mul_hi": sum(t.startswith("v_mul_hi_u32") for t in texts),
            "mul_lo": sum(t.startswith("v_mul_lo_u32") for t in texts), "mul_hi_in_front": in_front,
            "mad_u64": sum(t.startswith("v_mad_u64_u32") for t in texts),
            "table_reads": len(rd), "one_run": bool(rd) and rd[-1] - rd[0] == len(rd) - 1,
            "waits": waits,
            "rsq": sum(t.startswith("v_rsq_f64") for t in texts), "logf": sum(t.startswith("v_log_f32") for t in texts),
            "stores": stores, "low_bin": low_bin,
            "scratch_insts": sum(t.startswith("scratch_") for _, t in code)}


def report(asm_text):
    """[{dq, ne, split, unit_t, vgprs, scratch, burst}] of every step_inc_duo_kernel in the text"""
    out = []
    for name, lines in split_kernels(asm_text, descriptor=True).items():
        m = KERNEL.match(name)
        if not m:
            continue
        text = "\n".join(lines)
        v = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)
        s = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
        out.append({"dq": int(m.group(1)), "ne": int(m.group(2)), "split": m.group(3) == "1", "unit_t": m.group(4) == "1",
                    "vgprs": int(v.group(1)) if v else None, "scratch": int(s.group(1)) if s else None,
                    "burst": burst(text, int(m.group(2)) + 1)})
    return out


def is_headline(r):
    return r["dq"] == 8 and r["ne"] == 15 and r["split"] and r["unit_t"]


def interleaved(r):
    """the shape of the module's docstring"""
    b = r["burst"]
    return (b is not None and b["mul_hi"] >= 32 and b["mul_lo"] >= 32 and b["mul_hi_in_front"] == 0
            and b["mad_u64"] == 0 and b["table_reads"] == 4 and b["one_run"]
            and len(b["waits"]) >= 2 and all(n > 0 for n in b["waits"][:-1]) and b["rsq"] == 4 and b["logf"] == 4
            and b["stores"] == 4 and b["low_bin"] is not None and b["low_bin"]["conditional"]
            and b["low_bin"]["forward"]
            and r["vgprs"] is not None and r["vgprs"] <= 256 and r["scratch"] == 0 and b["scratch_insts"] == 0)


if __name__ == "__main__":
    rows = report(compile_to_asm(1, 8))
    for r in rows:
        print(r)
    head = [r for r in rows if is_headline(r)]
    sys.exit(0 if head and all(interleaved(r) for r in head) else 1)

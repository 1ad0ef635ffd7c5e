"""How step_inc_duo_kernel (incremental_duo.hip, one mode on two lanes per walker) waits for the LDS reads of a
step: a step issues its (r, ea_f|ka) read and its NE reads of (v, u) pairs up front; LDS answers a wave in
order, so the first fma needs the first two reads only.  With the chunk staging's LDS-DMA in flight beside the
steps AND counted by the compiler, every such wait was `s_waitcnt lgkmcnt(0)`; with the DMA where the compiler
does not count it (incremental_common.h: stage16_dma) the waits are counted: lgkmcnt(14), (13), ...  The same
happens with a scalar load left in flight across the reads.  Compiles the kernels of dq = 1 .. 8 to assembly
with the build's flags and reports, per instantiation and per block of the step loop (`Depth=2` or deeper), the
lgkmcnt(N) of the waits that follow a run of at least four ds_read_b128, and the compiler's own vmcnt waits in the
chunk loop around the step loop (chunk_vmcnt: each would retire the next chunk's DMA at the chunk's start).
    python tools/check_lds_waits.py        exit code 1 if the headline instantiation <8, 15, true, true> waits with lgkmcnt(0) alone
                                           or has a compiler vmcnt wait in its chunk loop"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_asm import duo_to_asm as compile_to_asm, kernels_matching  # noqa: E402

MIN_RUN = 4


def report(asm_text):
    """[{dq, ne, split, unit_t, ladders}], ladders = [(block label, reads in the run, [N of each lgkmcnt(N) behind it])]"""
    out = []
    for m, lines in kernels_matching(asm_text, r"_ZN4mcmc\S*step_inc_duo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E"):
        ladders, in_loop, label, run, cur = [], False, None, 0, None
        for line in lines:
            text = line.strip()
            b = re.match(r"^(\.LBB\d+_\d+):(?:.*Depth=(\d+))?", line)
            if b:
                in_loop, label, run, cur = bool(b.group(2)) and int(b.group(2)) >= 2, b.group(1), 0, None
            elif re.match(r"^;\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", text):
                # (a loop header inside other loops: its label's own line names the outermost parent's depth, this
                # line of the label's comment its own)
                in_loop = int(re.search(r"Depth=(\d+)", text).group(1)) >= 2
            elif not in_loop or not text or text.startswith(";"):
                continue
            elif text.startswith("ds_read_b128"):
                run, cur = run + 1, None
            else:
                w = re.match(r"s_waitcnt\b.*lgkmcnt\((\d+)\)", text)
                if w and cur is None and run >= MIN_RUN:
                    cur = (label, run, [])
                    ladders.append(cur)
                if w and cur is not None:
                    cur[2].append(int(w.group(1)))
                run = 0
        out.append({"dq": int(m.group(1)), "ne": int(m.group(2)), "split": m.group(3) == "1",
                    "unit_t": m.group(4) == "1", "ladders": ladders, "chunk_vmcnt": chunk_vmcnt("\n".join(lines))})
    return out


def chunk_vmcnt(kernel_text):
    """The compiler's own `s_waitcnt vmcnt(N)` (outside asm statements) in the blocks of the chunk loop around the step
    loop (`Depth=1`, the loop with child loops): a chunk's steps run beside the DMA of the next chunk, which only the
    hand-written wait at the chunk's end may retire; a compiler wait there (it drained vmcnt in the step loop's preheader
    while it held a load of the prologue as pending) waits for the DMA at once."""
    heads = set(re.findall(r"^\.L(BB\d+_\d+):\s*; =>This Loop Header: Depth=1\n\s*;\s+Child Loop", kernel_text, re.M))
    found, inside, in_asm = [], False, False
    for line in kernel_text.split("\n"):
        text = line.strip()
        b = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", line)
        if b:
            rest = b.group(2)
            h = re.search(r"Header=(BB\d+_\d+) Depth=1", rest)
            inside = (b.group(1) in heads and "Depth=1" in rest) or bool(h and h.group(1) in heads)
        elif text.startswith(";;#ASMSTART"):
            in_asm = True
        elif text.startswith(";;#ASMEND"):
            in_asm = False
        elif inside and not in_asm and re.match(r"s_waitcnt\b.*vmcnt\(", text):
            found.append(text)
    return found


def is_headline(r):
    return r["dq"] == 8 and r["ne"] == 15 and r["split"] and r["unit_t"]


def counted(r):
    """the step loop has a run of reads, and a wait behind one that is not lgkmcnt(0)"""
    return any(n > 0 for _, _, waits in r["ladders"] for n in waits)


if __name__ == "__main__":
    rows = report(compile_to_asm(1, 8))
    for r in rows:
        print({k: v for k, v in r.items() if k != "ladders"}, "counted" if counted(r) else "lgkmcnt(0) only")
        for label, reads, waits in r["ladders"]:
            print(f"    {label}: {reads} ds_read_b128, lgkmcnt {waits}")
    head = [r for r in rows if is_headline(r)]
    sys.exit(0 if head and all(counted(r) and not r["chunk_vmcnt"] for r in head) else 1)

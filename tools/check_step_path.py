"""The common path of a step of step_inc_duo_kernel (incremental_duo.hip, one mode on two lanes per walker), read off
the assembly: from the step's run of ds_read_b128 (the variate pair and the lane's NE (v, u) pairs) to the back-edge of
the step loop a step that meets none of its rare cases -- a trial in doubt at the wall of the box, an accept in doubt,
a wave still burning in -- should run straight-line code: the project's own measurement of a taken branch in this
kernel is profiles/r12_lazy_accept.txt (the same instructions gained 0.4 % over two taken branches and 2.2 % without),
and a scalar load there stands in the serial chain pair sum -> ll -> delta -> accept (round 17).  Compiles the kernels
of dq = 1 .. 8 to assembly with the build's flags and reports, per instantiation, between the run and the back-edge:
    s_load     scalar loads (|u|^2 came by one until round 17)
    s_branch   unconditional branches
    taken      conditional branches that are not the back-edge and target a block laid out at or in front of it
               (a branch to a block BEHIND the back-edge leaves the common path: a rare case, which jumps back)
    python tools/check_step_path.py        exit code 1 if the headline instantiation <8, 15, true, true> has any of them,
                                           or its step loop has no run of 16 reads with a back-edge behind it"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_duo_spills import compile_to_asm  # noqa: E402

LABEL = re.compile(r"^(\.LBB\d+_\d+):(?:.*Depth=(\d+))?")
HEADER = re.compile(r"^;\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")


def step_path(kernel_text, reads):
    """The instructions between the first run of exactly `reads` ds_read_b128 inside a loop of depth >= 2 and the first
    backward branch behind it whose target lies at or in front of the run (the back-edge), as
    {run_at, back_edge, instructions, s_load, s_branch, taken}; None if there is no such run or no such branch."""
    lines = [(i, ln.strip()) for i, ln in enumerate(kernel_text.split("\n"))]
    at = {}   # label -> line
    for i, text in lines:
        m = LABEL.match(text)
        if m:
            at[m.group(1)] = i
    in_loop, run, run_start, found = False, 0, None, None
    for i, text in lines:
        m = LABEL.match(text)
        if m:
            # (a loop header inside other loops: the label's line names the outermost parent's depth, the line
            # `=> This Inner Loop Header` of its comment its own)
            in_loop, run = bool(m.group(2)) and int(m.group(2)) >= 2, 0
        elif HEADER.match(text):
            in_loop = int(HEADER.match(text).group(1)) >= 2
        elif not text or text.startswith(";"):
            continue
        elif in_loop and text.startswith("ds_read_b128"):
            run_start = i if run == 0 else run_start
            run += 1
        else:
            if run == reads:
                found = (run_start, i)
                break
            run = 0
    if found is None:
        return None
    run_start, behind = found
    out = {"run_at": run_start, "back_edge": None, "instructions": 0, "s_load": [], "s_branch": [], "taken": []}
    path = []
    for i, text in lines:
        if i < behind or not text or text.startswith(";") or LABEL.match(text):
            continue
        path.append((i, text))
        b = BRANCH.match(text)
        if b and at.get(b.group(2), 1 << 60) <= run_start:
            out["back_edge"] = i
            break
    if out["back_edge"] is None:
        return None
    out["instructions"] = len(path)
    for i, text in path:
        b = BRANCH.match(text)
        if text.startswith("s_load_"):
            out["s_load"].append(text)
        elif b and b.group(1) == "s_branch":
            out["s_branch"].append(text)
        elif b and i != out["back_edge"] and at.get(b.group(2), -1) <= out["back_edge"]:
            out["taken"].append(text)
    return out


def report(asm_text):
    """[{dq, ne, split, unit_t, path}] for every step_inc_duo_kernel in the text (path: step_path for NE + 1 reads)"""
    out = []
    for m in re.finditer(r"^(_ZN4mcmc\S*step_inc_duo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E\S*):\s.*?^\s*s_endpgm",
                         asm_text, re.S | re.M):
        ne = int(m.group(3))
        out.append({"dq": int(m.group(2)), "ne": ne, "split": m.group(4) == "1", "unit_t": m.group(5) == "1",
                    "path": step_path(m.group(0), ne + 1)})
    return out


def is_headline(r):
    return r["dq"] == 8 and r["ne"] == 15 and r["split"] and r["unit_t"]


def straight(r):
    """a run with a back-edge behind it, and nothing between them but the common path"""
    p = r["path"]
    return p is not None and not p["s_load"] and not p["s_branch"] and not p["taken"]


if __name__ == "__main__":
    rows = report(compile_to_asm(1, 8))
    for r in rows:
        p = r["path"]
        print({k: v for k, v in r.items() if k != "path"},
              "no run of reads with a back-edge behind it" if p is None else
              f"{p['instructions']} instructions to the back-edge; s_load {p['s_load']}, s_branch {p['s_branch']}, "
              f"taken {p['taken']}")
    head = [r for r in rows if is_headline(r)]
    sys.exit(0 if head and all(straight(r) for r in head) else 1)

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
    guards     s_cbranch_execz over ONE straight-line block to the label right behind it (round 20: the commit runs on
               the accepting lanes alone, exec narrowed around it).  Such a branch is taken only by a wave NONE of whose
               lanes enters the block -- of 32 walkers at an acceptance of 0.3 one wave-step in 10^5 --: the common
               step falls through it, it is reported apart and is not `taken`.  A guard is no licence: the instructions
               of its block count as the common path's (tests/test_commit_path_compile.py says what the block may hold)
    python tools/check_step_path.py        exit code 1 if the headline instantiation <8, 15, true, true> has any of them,
                                           or its step loop has no run of 16 reads with a back-edge behind it"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_asm import duo_to_asm as compile_to_asm, kernels_matching  # noqa: E402

LABEL = re.compile(r"^(\.LBB\d+_\d+):(?:.*Depth=(\d+))?")
HEADER = re.compile(r"^;\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")


def step_path(kernel_text, reads):
    """The instructions between the first run of exactly `reads` ds_read_b128 inside a loop of depth >= 2 and the first
    backward branch behind it whose target lies at or in front of the run (the back-edge), as
    {run_at, back_edge, instructions, s_load, s_branch, taken, guards}; None if there is no such run or no such branch."""
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
    out = {"run_at": run_start, "back_edge": None, "instructions": 0, "s_load": [], "s_branch": [], "taken": [],
           "guards": []}
    labels = sorted(at.values())
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
            target = at.get(b.group(2), -1)
            # (a guard: the target is the first label behind the branch and no branch stands in the block it skips)
            if (b.group(1) == "s_cbranch_execz" and target > i and not any(i < ln < target for ln in labels)
                    and not any(BRANCH.match(t) for j, t in path if i < j < target)):
                out["guards"].append(text)
            else:
                out["taken"].append(text)
    return out


def kernels(asm_text):
    """(dq, ne, split, unit_t, text) of every step_inc_duo_kernel in the text"""
    for m, lines in kernels_matching(asm_text, r"_ZN4mcmc\S*step_inc_duo_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E"):
        yield int(m.group(1)), int(m.group(2)), m.group(3) == "1", m.group(4) == "1", "\n".join(lines)


def report(asm_text):
    """[{dq, ne, split, unit_t, path}] for every step_inc_duo_kernel in the text (path: step_path for NE + 1 reads)"""
    out = []
    for dq, ne, split, unit_t, text in kernels(asm_text):
        out.append({"dq": dq, "ne": ne, "split": split, "unit_t": unit_t, "path": step_path(text, ne + 1)})
    return out


def step_lines(asm_text, dq, ne, unit_t):
    """(path, [(line, instruction)] from the first instruction behind the run of reads to the back-edge, labels as
    `.LBBn_m:`) of the instantiation <dq, ne, true, unit_t>; (None, []) where step_path finds none"""
    for k_dq, k_ne, k_split, k_unit_t, text in kernels(asm_text):
        if (k_dq, k_ne, k_split, k_unit_t) != (dq, ne, True, bool(unit_t)):
            continue
        p = step_path(text, ne + 1)
        if p is None:
            break
        rows = [(i, ln.strip()) for i, ln in enumerate(text.split("\n"))]
        first = next(i for i, t in rows if i > p["run_at"] and t and not t.startswith(("ds_read_b128", ";")))
        return p, [(i, t.split(";")[0].strip()) for i, t in rows
                   if first <= i <= p["back_edge"] and t and not t.startswith(";")]
    return None, []


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
              f"taken {p['taken']}, guards {p['guards']}")
    head = [r for r in rows if is_headline(r)]
    sys.exit(0 if head and all(straight(r) for r in head) else 1)

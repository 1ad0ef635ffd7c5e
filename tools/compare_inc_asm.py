#!/usr/bin/env python3
"""Do two source trees compile the step kernels to the same machine code?

    git worktree add ../parent HEAD~1
    python tools/compare_inc_asm.py ../parent . [--jobs 8] [--units PREFIX ...] > profiles/<name>.txt

Compiles every translation unit that cobaya_amd/build.py lists and whose name begins with one of the prefixes
(default `incremental_`: incremental_<lo>, incremental_emit_<lo>, incremental_any_<part>, incremental_duo_<lo>; the
from-scratch kernels: `--units walker_d walker_big general blocked`) from both trees to assembly (tools/hip_asm.py) and
compares, kernel by kernel, the instruction text: labels, instructions and the `.amdhsa_*` kernel descriptor; comments, blank lines and
`.loc` / `.file` / `.ident` directives are dropped.  Prints the number of identical kernels per unit and, for every
kernel that differs, VGPRs and scratch bytes on both sides and the first differing lines.  Exit code 1 if any differs."""
import argparse
import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_asm import compile_to_asm, split_kernels  # noqa: E402
from cobaya_amd.build import ALL_DIMS, translation_units  # noqa: E402


def instruction_text(lines):
    out = []
    for line in lines:
        text = line.split(";")[0].strip()
        if text and not re.match(r"\.(loc|file|ident)\b", text):
            out.append(text)
    return out


def kernels_of(root, source, defines):
    """{mangled name: instruction text} of one translation unit of the tree `root`"""
    asm = compile_to_asm(source, defines, root=root)
    return {name: instruction_text(lines) for name, lines in split_kernels(asm, descriptor=True).items()}


def registers(text):
    """'vgpr N scratch M' from a kernel's descriptor lines"""
    get = lambda key: next((ln.split()[1] for ln in text if ln.startswith(key + " ")), "?")  # noqa: E731
    return f"vgpr {get('.amdhsa_next_free_vgpr')} scratch {get('.amdhsa_private_segment_fixed_size')}"


def demangled(name):
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(anonymous namespace\)::|mcmc::|void |\(.*", "", dem)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--lines", type=int, default=12, help="differing lines shown per kernel")
    ap.add_argument("--units", nargs="+", default=["incremental_"], metavar="PREFIX",
                    help="compare the translation units whose names begin with one of these")
    args = ap.parse_args()
    units = [(src, name, defines) for src, name, defines in translation_units(ALL_DIMS, big=True)
             if name.startswith(tuple(args.units))]
    tasks = [(os.path.abspath(root), src, defines) for root in (args.old, args.new) for src, _, defines in units]
    with ThreadPoolExecutor(max(1, min(args.jobs, 16))) as ex:
        sides = list(ex.map(lambda t: kernels_of(*t), tasks))
    same = differing = 0
    for (_, unit, _), old, new in zip(units, sides[:len(units)], sides[len(units):]):
        diff = [k for k in sorted(set(old) | set(new)) if old.get(k) != new.get(k)]
        print(f"{unit}: {len(new)} kernels, {len(new) - sum(k in new for k in diff)} identical, {len(diff)} differ")
        same += len(new) - sum(k in new for k in diff)
        differing += len(diff)
        for k in diff:
            if k not in old or k not in new:
                print(f"  {demangled(k)}: only in the {'new' if k in new else 'old'} tree")
                continue
            print(f"  {demangled(k)}: {registers(old[k])} -> {registers(new[k])}; "
                  f"{len(old[k])} -> {len(new[k])} lines")
            delta = [ln for ln in difflib.unified_diff(old[k], new[k], lineterm="", n=0) if ln[:2] not in ("--", "++")]
            for ln in delta[:args.lines]:
                print("      " + ln)
    print(f"total: {same} kernels identical, {differing} differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())

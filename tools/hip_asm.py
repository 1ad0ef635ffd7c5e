"""The one place where the developer tools compile a .hip file to gfx950 assembly (hipcc -S --cuda-device-only with
the flags of cobaya_amd/build.py) and cut the assembly into kernels."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compile_to_asm(source, defines=(), root=ROOT):
    """The device assembly of cobaya_amd/csrc/<source> of the tree `root`, compiled with the build's flags and `defines`"""
    from cobaya_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"]
        res = subprocess.run([B.hipcc(), *flags, *defines, "-S", "--cuda-device-only", "-o", out,
                              os.path.join(root, "cobaya_amd", "csrc", source)], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {source} {' '.join(defines)}\n{res.stderr}")
        with open(out) as f:
            return f.read()


def duo_to_asm(dq_lo=6, dq_hi=8, extra=()):
    """incremental_duo.hip for dq_lo <= dq <= dq_hi (what the four tools of the two-lane kernels read)"""
    return compile_to_asm("incremental_duo.hip", [*extra, f"-DMCMC_DUO_DQ_LO={dq_lo}", f"-DMCMC_DUO_DQ_HI={dq_hi}"])


def split_kernels(asm_text, descriptor=False):
    """{mangled name: lines} of every kernel in the text, from its label to its last s_endpgm; with `descriptor`
    followed by the lines of its `.amdhsa_kernel` block"""
    out, name, body, desc, in_desc = {}, None, [], [], False

    def close():
        ends = [i for i, x in enumerate(body) if x.strip().startswith("s_endpgm")]
        if name is not None and ends:   # (a device function has no s_endpgm)
            out[name] = body[:ends[-1] + 1] + (desc if descriptor else [])

    for line in asm_text.split("\n"):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m or re.match(r"^\.Lfunc_end\d+:", line):
            close()
            name, body, desc, in_desc = (m.group(1) if m else None), [line], [], False
        elif in_desc or line.strip().startswith(".amdhsa_kernel"):
            desc.append(line)
            in_desc = not line.strip().startswith(".end_amdhsa_kernel")
        elif name is not None:
            body.append(line)
    close()
    return out


def kernels_matching(asm_text, pattern):
    """(match, lines) of every kernel whose mangled name `pattern` matches from its start"""
    for name, lines in split_kernels(asm_text).items():
        m = re.match(pattern, name)
        if m:
            yield m, lines

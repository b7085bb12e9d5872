"""DEV TOOL: are kernels of one translation unit the same instructions in two trees?  Compiles hagrid_amd/csrc/UNIT.hip of this tree and of OTHER (a checkout
of another commit) to gfx950 assembly with the product's flags, takes the body of every kernel whose name contains one of KERNEL..., drops comments and
directives, replaces mangled symbols and local labels by placeholders (a struct that moved to another namespace changes the mangling, not the code) and
compares line by line.  Prints the number of instructions on either side and `identical` or `DIFFER`; exit status 1 when any differs.

usage: python tools/dev_kernel_diff.py OTHER UNIT KERNEL [KERNEL ...]        e.g.  python tools/dev_kernel_diff.py ../parent overlap overlap_boxes_kernel obb_tris_kernel"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hagrid_amd import build as B

other, unit, kernels = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3:]


def bodies(root):
    flags = [f.replace(ROOT, root) for f in B.FLAGS]
    r = subprocess.run([B.HIPCC, *flags, "--cuda-device-only", "-S", "-o", "-", os.path.join(root, "hagrid_amd", "csrc", unit + ".hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, out = r.stdout.splitlines(), {}
    for name in kernels:
        start = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % name, l)][0]
        end = [i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end")][0]
        body = [re.sub(r";.*", "", l).strip() for l in lines[start + 1:end]]
        out[name] = [re.sub(r"\.L\w+", "L", re.sub(r"_Z\w+", "SYM", l)) for l in body if l and not l.startswith(".")]
    return out


here, there = bodies(ROOT), bodies(other)
same = True
for name in kernels:
    eq = here[name] == there[name]
    same &= eq
    print(f"{name}: {len(here[name])} instructions here, {len(there[name])} there: {'identical' if eq else 'DIFFER'}")
sys.exit(0 if same else 1)

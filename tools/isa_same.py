"""Is the device code of two source trees the same?  Compiles every unit of build.units() that has device
code (the .hip sources) to gfx950 assembly with that unit's own flags (hipcc --cuda-device-only -S), once
from each tree's csrc/ (the unit's name as its compilation-unit id, so that the trees' paths do not enter),
drops the .ident line and compares the two files byte for byte.  One line per unit:
`identical`, or the first differing line; exit status 1 on any difference.  A unit whose source only one of the
trees has (a unit the change adds) is named as such and is no difference.  The check for a change that
only moves or tidies kernel source (profiles/header_split_isa.txt, profiles/dense_sample_split_isa.txt, profiles/kernel_split_isa.txt).

    python tools/isa_same.py TREE_A TREE_B [--extra "FLAGS"] [-j 8]

The unit list and the flags are those of the repository this tool lies in (irm_motion_planning_amd/build.py).
"""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # this tool's own repository
from irm_motion_planning_amd import build  # noqa: E402

args = sys.argv[1:]
extra = args[args.index("--extra") + 1].split() if "--extra" in args else []
jobs = int(args[args.index("-j") + 1]) if "-j" in args else 8
trees = [a for i, a in enumerate(args) if not a.startswith("-") and (i == 0 or args[i - 1] not in ("--extra", "-j"))]
assert len(trees) == 2, __doc__
tmp = tempfile.mkdtemp()


def asm(tree, tag, unit):
    name, src, flags = unit
    csrc = os.path.join(os.path.abspath(tree), "irm_motion_planning_amd", "csrc")
    out = os.path.join(tmp, f"{name}.{tag}.s")
    # -cuid: the compilation unit's id symbol (__hip_cuid_*), which hipcc otherwise hashes from the source's path
    r = subprocess.run([build.HIPCC] + build.CFLAGS + extra + flags +
                       [f"-cuid={name}", "--cuda-device-only", "-S", "-o", out, src], cwd=csrc, capture_output=True, text=True)
    if r.returncode:  # the compiler's own words, then stop
        sys.exit(f"{name} from {tree}: hipcc failed\n{r.stderr}")
    lines = [ln for ln in open(out, "rb").read().split(b"\n") if not ln.lstrip().startswith(b".ident")]
    os.remove(out)
    return lines


def one(unit):
    have = [os.path.exists(os.path.join(t, "irm_motion_planning_amd", "csrc", unit[1])) for t in trees]
    if not all(have):
        where = f"only in {trees[have.index(True)]}" if any(have) else "in neither tree"
        return f"{unit[0]}: {unit[1]} {where}"
    a, b = asm(trees[0], "a", unit), asm(trees[1], "b", unit)
    if a == b:
        return f"{unit[0]}: identical ({len(a)} lines)"
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    show = lambda ls: ls[i].decode(errors="replace").strip() if i < len(ls) else "<end of file>"  # noqa: E731
    return f"{unit[0]}: DIFFERS at line {i + 1}: {show(a)!r} / {show(b)!r}"


print(f"isa_same {' '.join(extra) or '(no extra flags)'}", flush=True)
with ThreadPoolExecutor(jobs) as ex:
    res = list(ex.map(one, [u for u in build.units() if u[1].endswith(".hip")]))
print("\n".join(res))
sys.exit(any("DIFFERS" in r for r in res))

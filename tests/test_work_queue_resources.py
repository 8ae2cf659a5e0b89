"""Register / scratch budget of the work queue's k_lean instantiations as hipcc builds them for gfx950
(device assembly only, no GPU), like tests/test_kernel_resources.py for the static launch's kernels: the
queue flag adds a claim and a load step to the per-trajectory state machine, and must not push the
variants it is built for into scratch."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

UNITS = ("opt_fixq3_128", "opt_fixq7_128")


def _kernels(asm):
    """(demangled name, vgpr, spill, scratch) of every kernel in a hipcc -S device assembly file."""
    meta = asm[asm.index("amdhsa.kernels:"):]
    rows = []
    for blk in re.split(r"\n  - ", meta)[1:]:
        kv = dict(re.findall(r"^\s*\.(\w+):\s+(\S.*)$", blk, re.M))
        if "name" in kv:
            rows.append((kv["name"], int(kv.get("vgpr_count", 0)), int(kv.get("vgpr_spill_count", 0)),
                         int(kv.get("private_segment_fixed_size", 0))))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True,
                           text=True).stdout.split("\n")
    return [(nm,) + r[1:] for r, nm in zip(rows, names)]


@pytest.fixture(scope="module")
def queue_kernels():
    from irm_motion_planning_amd import build
    units = {u[0]: u for u in build.units()}
    tmp = tempfile.mkdtemp()
    procs = {}
    for name in UNITS:
        if name not in units:  # (a shape left on the static launch has no unit)
            continue
        _, src, flags = units[name]
        out = os.path.join(tmp, name + ".s")
        procs[name] = (out, subprocess.Popen([build.HIPCC] + build.CFLAGS + flags + ["--cuda-device-only", "-S", "-o", out, src],
                                             cwd=build.CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL))
    res = {}
    for name, (out, p) in procs.items():
        assert p.wait(timeout=600) == 0, name
        with open(out) as f:
            res[name] = [k for k in _kernels(f.read()) if "k_lean" in k[0]]
    shutil.rmtree(tmp, ignore_errors=True)
    return res


def test_c3_queue_kernels_spill_free_without_scratch(queue_kernels):
    ks = queue_kernels["opt_fixq3_128"]
    assert len(ks) == 4, ks  # the GD dual loop and BLS, 256- and 512-thread workgroups
    for name, vgpr, spill, scratch in ks:
        assert name.rstrip().endswith("true>(irm::KParams)"), name  # the queue flag is on
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)


def test_c7_queue_kernels_spill_free(queue_kernels):
    """7-DoF runs the queue only if its variants do not spill; left on the static launch, the unit is absent."""
    from irm_motion_planning_amd import build
    if (7, 128) not in build.QUEUE_SHAPES:
        assert "opt_fixq7_128" not in {u[0] for u in build.units()}
        assert "opt_fixq7_128" not in queue_kernels
        return
    ks = queue_kernels["opt_fixq7_128"]
    assert len(ks) == 4, ks
    for name, vgpr, spill, scratch in ks:
        assert spill == 0, (name, vgpr, spill, scratch)

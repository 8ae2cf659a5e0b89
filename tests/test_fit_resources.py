"""Register / scratch budget of the fitting and re-timing kernels (csrc/irm_fit.hip) as hipcc builds them for
gfx950 (device assembly only, no GPU), like tests/test_dense_resources.py: the fp64 accumulators of every problem
of a workgroup and the prefetched operator values must stay in registers at every D."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


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
def fit_kernels():
    from irm_motion_planning_amd import build
    _, src, flags = {u[0]: u for u in build.units()}["irm_fit"]
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "irm_fit.s")
    try:
        subprocess.run([build.HIPCC] + build.CFLAGS + flags + ["--cuda-device-only", "-S", "-o", out, src],
                       cwd=build.CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        with open(out) as f:
            return _kernels(f.read())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.parametrize("kernel", ["k_fit_alpha", "k_transfer_alpha"])
def test_every_instance_spill_free_without_scratch(fit_kernels, kernel):
    from irm_motion_planning_amd import build
    ks = [k for k in fit_kernels if f"irm::{kernel}<" in k[0]]
    assert len(ks) == build.MAX_D, ks  # one instance per D = 1..8 (dispatch_d)
    assert {any(f"irm::{kernel}<{d}>" in k[0] for k in ks) for d in range(1, build.MAX_D + 1)} == {True}
    for name, vgpr, spill, scratch in ks:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)


def test_no_other_kernels_in_the_unit(fit_kernels):
    """The unit instantiates its own kernels only: the optimiser templates of the shared header stay in their units."""
    assert fit_kernels and all("k_fit_alpha" in k[0] or "k_transfer_alpha" in k[0] for k in fit_kernels), fit_kernels

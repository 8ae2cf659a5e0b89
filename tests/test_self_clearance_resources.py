"""Register / scratch budget of the self-clearance kernel (csrc/irm_self_clearance.hip) as hipcc builds it for gfx950
(device assembly only, no GPU), like tests/test_clearance_resources.py: the FK prefix, the link directions and the
per-pair minima (21 at D = 8) must stay in registers at every D."""
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from test_dense_resources import _kernels  # noqa: E402


@pytest.fixture(scope="module")
def self_clearance_kernels():
    from irm_motion_planning_amd import build
    _, src, flags = {u[0]: u for u in build.units()}["irm_self_clearance"]
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "irm_self_clearance.s")
    try:
        subprocess.run([build.HIPCC] + build.CFLAGS + flags + ["--cuda-device-only", "-S", "-o", out, src],
                       cwd=build.CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        with open(out) as f:
            return _kernels(f.read())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_every_instance_spill_free_without_scratch(self_clearance_kernels):
    from irm_motion_planning_amd import build
    names = " ".join(k[0] for k in self_clearance_kernels)
    assert len(self_clearance_kernels) == build.MAX_D, self_clearance_kernels  # one instance per D = 1..8 (dispatch_d)
    for d in range(1, build.MAX_D + 1):
        assert f"irm::k_self_clearance<{d}>" in names, (d, names)
    for name, vgpr, spill, scratch in self_clearance_kernels:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= 256, (name, vgpr)  # 256 threads: at least two workgroups per CU


def test_no_other_kernels_in_the_unit(self_clearance_kernels):
    assert all("irm::k_self_clearance<" in k[0] for k in self_clearance_kernels), self_clearance_kernels

"""Register / scratch budget of C3's 512-thread GD single-loop kernel as hipcc builds it for gfx950 (device
assembly only, no GPU), like tests/test_work_queue_resources.py: the kernel carries two round bodies (the
all-live loop and the general one), and both together must stay within the 256 VGPRs a 512-thread workgroup
has per lane, without scratch."""
import os
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from test_work_queue_resources import _kernels  # noqa: E402

UNIT = "opt_fix3_128"
KERNEL = "void irm::k_lean<irm::FixShape<3, 128, 32>, 512, 1, true, 0, false>(irm::KParams)"


@pytest.fixture(scope="module")
def gd1_kernel():
    from irm_motion_planning_amd import build
    _, src, flags = {u[0]: u for u in build.units()}[UNIT]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, UNIT + ".s")
        subprocess.run([build.HIPCC] + build.CFLAGS + flags + ["--cuda-device-only", "-S", "-o", out, src], cwd=build.CSRC,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        with open(out) as f:
            asm = f.read()
    ks = [k for k in _kernels(asm) if k[0].strip() == KERNEL]
    assert len(ks) == 1, [k[0] for k in _kernels(asm)]
    return ks[0], asm


def test_no_scratch_no_spills(gd1_kernel):
    (name, vgpr, spill, scratch), _ = gd1_kernel
    assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)


def test_vgpr_budget(gd1_kernel):
    (name, vgpr, spill, scratch), _ = gd1_kernel
    print(name, "VGPRs", vgpr)
    assert vgpr <= 256, (name, vgpr)


def test_both_round_bodies_are_built(gd1_kernel):
    """The all-live loop reads the flag word under its own marker comment."""
    _, asm = gd1_kernel
    assert "flag word, stage-1 waves (all-live)" in asm and "flag word, stage-1 waves\n" in asm

"""Register / scratch budget of the multi-start kernels (csrc/irm_multistart.hip) as hipcc builds them for gfx950
(device assembly only, no GPU), like tests/test_clearance_resources.py: the seed kernel carries fit_alpha's fp64
accumulators and its waypoint row in registers at every D; replicate, rank and gather are small."""
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from test_dense_resources import _kernels  # noqa: E402

OTHERS = ("irm::k_replicate(", "irm::k_rank_candidates(", "irm::k_gather_winner(")


@pytest.fixture(scope="module")
def multistart_kernels():
    from irm_motion_planning_amd import build
    _, src, flags = {u[0]: u for u in build.units()}["irm_multistart"]
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "irm_multistart.s")
    try:
        subprocess.run([build.HIPCC] + build.CFLAGS + flags + ["--cuda-device-only", "-S", "-o", out, src],
                       cwd=build.CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        with open(out) as f:
            return _kernels(f.read())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_every_kernel_spill_free_without_scratch(multistart_kernels):
    from irm_motion_planning_amd import build
    names = " ".join(k[0] for k in multistart_kernels)
    assert len(multistart_kernels) == build.MAX_D + len(OTHERS), multistart_kernels
    for d in range(1, build.MAX_D + 1):  # one seed kernel per D = 1..8 (dispatch_d)
        assert f"irm::k_seed_ensemble<{d}>" in names, (d, names)
    for other in OTHERS:
        assert other in names, (other, names)
    for name, vgpr, spill, scratch in multistart_kernels:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= 256, (name, vgpr)


def test_no_other_kernels_in_the_unit(multistart_kernels):
    assert all("irm::k_seed_ensemble<" in k[0] or any(o in k[0] for o in OTHERS) for k in multistart_kernels), \
        multistart_kernels

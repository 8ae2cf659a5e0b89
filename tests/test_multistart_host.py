"""Multi-start planning without a GPU: the numpy twin of tests/multistart_cases.py against hand-computed hashes,
exact arithmetic and a brute-force sort, and the C ABI's new symbols and structs against their ctypes mirrors."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import multistart_cases as mc
from conftest import REPO

f32 = np.float32


# ------------------------------------------------------------------ hash and amplitudes
def test_fmix32_matches_hand_computed_values():
    """MurmurHash3's finaliser: 1, 2 and 0xFFFFFFFF worked through the five steps by hand (0 is its fixed point)."""
    assert int(mc.fmix32(np.uint32(0))) == 0
    assert int(mc.fmix32(np.uint32(1))) == 0x514E28B7
    assert int(mc.fmix32(np.uint32(2))) == 0x30F4C306
    assert int(mc.fmix32(np.uint32(0xFFFFFFFF))) == 0x81F16F39


def _fmix_int(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def test_seed_hash_is_the_nested_finaliser_in_wrapping_uint32():
    for seed, b, s, d in ((0, 0, 0, 0), (5, 2, 3, 1), (0xFFFFFFFF, 0xFFFFFFF0, 63, 7), (123456789, 1000000, 11, 2)):
        want = _fmix_int(_fmix_int(_fmix_int(_fmix_int(seed ^ mc.HASH_SALT) + b) + s) + d)
        assert int(mc.seed_hash(seed, np.uint64(b), np.uint64(s), np.uint64(d))) == want


def _round_f32(x):
    """A Fraction to the nearest float32, ties to even."""
    c = f32(float(x))
    cands = sorted({float(np.nextafter(c, f32(-np.inf))), float(c), float(np.nextafter(c, f32(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - x), int(np.array(v, f32).view(np.uint32)) & 1))
    return f32(best)


def test_fmaf32_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a = rng.uniform(-2, 2, 400).astype(f32)
    b = rng.uniform(-2, 2, 400).astype(f32)
    c = rng.uniform(-2, 2, 400).astype(f32)
    # cancellation and half-way cases: c close to −a·b, and products that need more than 53 bits with c
    c[:100] = (-(a[:100].astype(np.float64) * b[:100])).astype(f32)
    a[100:150] = f32(1) + f32(2.0 ** -23)
    b[100:150] = f32(1) + f32(2.0 ** -23)
    c[100:150] = rng.choice(np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** 30, 1.0], f32), 50)
    got = mc.fmaf32(a, b, c)
    for i in range(a.shape[0]):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


def test_amplitudes_are_bounded_and_zero_at_zero_amplitude():
    for A in (0.25, 1.0, 4.0):
        a = mc.amplitudes(7, 5, 64, 8, A)
        assert a.dtype == f32 and a.shape == (5, 64, 8)
        assert np.all(np.abs(a) <= f32(A))
    assert np.all(mc.amplitudes(7, 5, 64, 8, 0.0) == 0)


def test_every_candidate_has_a_nonzero_bump_at_unit_amplitude():
    for seed in (0, 1, 12345):
        a = mc.amplitudes(seed, 16, 64, 3, 1.0)
        assert np.all(np.any(a[:, 1:] != 0, axis=2))
    t = mc.support_times(33)
    assert mc.bump(t)[0] == 0 and mc.bump(t)[-1] == 0 and mc.bump(t)[16] == 1  # t = 0.5: the peak


def test_ensembles_nest_and_shards_reproduce_the_unsharded_rows():
    rng = np.random.default_rng(3)
    start, goal = (rng.uniform(-0.9, 1.9, (3, 3)).astype(f32) for _ in range(2))
    t = mc.support_times(33)
    lo, hi = mc.clamp_bounds(0.98, -1.0, 2.0)
    w8 = mc.waypoints(start, goal, 8, 11, 1.0, lo, hi, t)
    w4 = mc.waypoints(start, goal, 4, 11, 1.0, lo, hi, t)
    np.testing.assert_array_equal(w8[:, :4], w4)
    shard = mc.waypoints(start[1:], goal[1:], 8, 11, 1.0, lo, hi, t, problem_offset=1)
    np.testing.assert_array_equal(shard, w8[1:])
    assert not np.array_equal(mc.waypoints(start[1:], goal[1:], 8, 11, 1.0, lo, hi, t), w8[1:])  # the offset matters
    np.testing.assert_array_equal(mc.amplitudes(11, 3, 8, 3, 1.0)[:, :4], mc.amplitudes(11, 3, 4, 3, 1.0))


def test_waypoints_candidate_zero_is_the_line_and_the_rest_are_clamped():
    start = np.array([[0.0, 0.0, 0.0], [-0.9, 1.9, 0.5]], f32)
    goal = np.array([[1.2, 0.8, 0.3], [1.9, -0.9, 0.5]], f32)
    t = mc.support_times(33)
    lo, hi = mc.clamp_bounds(0.98, -1.0, 2.0)
    assert lo == f32(-0.98) and hi == f32(1.96)
    w = mc.waypoints(start, goal, 6, 0, 4.0, lo, hi, t)
    c = mc.smooth_step(t).astype(np.float64)
    line = start[:, None, :] + c[None, :, None] * (goal - start)[:, None, :].astype(np.float64)
    np.testing.assert_allclose(w[:, 0], line, rtol=0, atol=2e-7)
    np.testing.assert_array_equal(w[:, :, 0], np.clip(np.broadcast_to(start[:, None], w[:, :, 0].shape), lo, hi))
    assert w[:, 1:].min() == lo and w[:, 1:].max() == hi  # A = 4 reaches both bounds
    assert np.all(w[:, 1:] >= lo) and np.all(w[:, 1:] <= hi)
    np.testing.assert_array_equal(mc.replicate(start, 3), start[[0, 0, 0, 1, 1, 1]])


# ------------------------------------------------------------------ the ranking twin
@pytest.mark.parametrize("kind", ["random", "ties", "nan", "allfail", "classes"])
@pytest.mark.parametrize("S", [1, 2, 5, 33, 64])
@pytest.mark.parametrize("reports", [False, True])
def test_ranking_twin_matches_brute_force(kind, S, reports):
    rng = np.random.default_rng(S * 7 + len(kind))
    ok, loss, ncol = mc.random_tables(rng, 4, S, kind)
    nc = ncol if reports else None
    winner, rank = mc.rank_lexsort(ok, loss, nc)
    bw, br = mc.rank_brute(ok, loss, nc)
    np.testing.assert_array_equal(rank, br)
    np.testing.assert_array_equal(winner, bw)
    assert np.all(np.sort(rank, axis=1) == np.arange(S))  # a permutation per problem
    assert np.all(rank[np.arange(4), winner] == 0)


def test_ranking_key_order_by_hand():
    #            ok  loss  ncol      class
    ok = np.array([[1, 1, 0, 0, 1, 1]])
    loss = np.array([[3.0, 1.0, 0.1, 0.1, np.nan, 1.0]], f32)
    ncol = np.array([[0, 2, 0, 1, 0, 0]])
    winner, rank = mc.rank_lexsort(ok, loss, ncol)
    # classes 0, 1, 2, 3, 4 (NaN), 0 → order: s5 (0, 1.0), s0 (0, 3.0), s1 (1), s2 (2), s3 (3), s4 (NaN)
    np.testing.assert_array_equal(rank, [[1, 2, 3, 4, 5, 0]])
    assert winner[0] == 5
    winner, rank = mc.rank_lexsort(ok, loss)  # without reports: classes 0, 0, 2, 2, 4, 0
    np.testing.assert_array_equal(rank, [[2, 0, 3, 4, 5, 1]])  # s1 and s5 tie at 1.0: the lower s first
    assert winner[0] == 1
    cls, ls = mc.keys(np.zeros((1, 3)), np.array([[np.inf, np.nan, -np.inf]], f32))
    np.testing.assert_array_equal(cls, [[2, 4, 2]])
    np.testing.assert_array_equal(ls, [[np.inf, np.inf, -np.inf]])


def test_study_scenes_are_nine_positions_within_reach():
    assert mc.STUDY_SCENES.shape == (9, 2) and mc.STUDY_S == 12
    assert np.all(np.linalg.norm(mc.STUDY_SCENES, axis=1) < 3.0)
    assert mc.study_counts([1, 0, 1], [0, 0, 3]) == (2, 1)


# ------------------------------------------------------------------ the C ABI
def test_abi_version_stays_three_and_the_mirror_binds_the_header():
    import re

    from irm_motion_planning_amd import _abi
    src = open(os.path.join(REPO, "include", "irm.h")).read()
    assert re.search(r"#define IRM_ABI_VERSION 3\b", src)
    assert _abi.IRM_ABI_VERSION == 3
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(irm_[a-z0-9_]+)\s*\(", code)))
    assert sorted(_abi.PROTOTYPES) == declared
    for name in ("irm_seed_ensemble", "irm_seed_ensemble_dev", "irm_rank_candidates", "irm_rank_candidates_dev",
                 "irm_multistart_workspace", "irm_optimize_multistart", "irm_optimize_multistart_dev"):
        assert name in declared, name
    assert re.search(r"#define IRM_MAX_SEEDS 64\b", src)
    from irm_motion_planning_amd.multistart import IRM_MAX_SEEDS
    assert IRM_MAX_SEEDS == mc.MAX_SEEDS == 64


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "irm.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("sizeof irm_multistart %zu\nsizeof irm_multistart_out %zu\n", sizeof(irm_multistart), sizeof(irm_multistart_out));
  %FIELDS%
  return 0;
}
"""


def test_new_structs_match_their_ctypes_mirrors(tmp_path):
    from irm_motion_planning_amd.multistart import IrmMultistart, IrmMultistartOut
    structs = {"irm_multistart": IrmMultistart, "irm_multistart_out": IrmMultistartOut}
    fields = "\n".join(f"F({cn}, {f})" for cn, cls in structs.items() for f, _ in cls._fields_)
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C.replace("%FIELDS%", fields))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            a, b, c = ln.split()
            got[(a, b)] = int(c)
    for cn, cls in structs.items():
        assert got[("sizeof", cn)] == ctypes.sizeof(cls), cn
        for f, _ in cls._fields_:
            assert got[(cn, f)] == getattr(cls, f).offset, (cn, f)


def test_library_exports_the_new_symbols_and_refuses_a_null_context():
    from irm_motion_planning_amd._abi import load_library
    lib = load_library()
    assert lib.irm_multistart_workspace(None, 4, 6, 3, 0) == -22
    assert b"irm_multistart_workspace" in lib.irm_last_error()
    assert lib.irm_seed_ensemble(None, None, None, 1, 1, 0, 1.0, 0, None, None) == -22
    assert b"irm_seed_ensemble" in lib.irm_last_error()
    assert lib.irm_rank_candidates(None, None, None, 1, 1, None, None) == -22
    assert b"irm_rank_candidates" in lib.irm_last_error()


# ------------------------------------------------------------------ CLI flags and sharding
def test_cli_flags_parse_and_default_to_off():
    from irm_motion_planning_amd import main as irm_main
    a = irm_main.parse_args([])
    assert a.multi_start == 0 and a.multi_start_amplitude == 1.0 and a.multi_start_seed == 0
    a = irm_main.parse_args(["--multi-start", "12", "--multi-start-amplitude", "1.2", "--multi-start-seed", "7"])
    assert a.multi_start == 12 and a.multi_start_amplitude == 1.2 and a.multi_start_seed == 7
    for bad in (["--multi-start", "65"], ["--multi-start", "-1"], ["--multi-start-amplitude", "-0.5"]):
        with pytest.raises(SystemExit):
            irm_main.parse_args(bad)


def test_a_shards_problem_offset_is_its_first_global_row():
    from irm_motion_planning_amd import distributed
    for B, world in ((10, 1), (10, 3), (7, 4), (3, 5)):
        rows = []
        for rank in range(world):
            lo, hi = distributed.shard(B, world, rank)
            assert distributed.problem_offset(B, world, rank) == lo
            rows += list(range(lo, hi))
        assert rows == list(range(B))
    # ... so the shards' waypoints are the unsharded batch's rows
    rng = np.random.default_rng(1)
    start, goal = (rng.uniform(-0.9, 1.9, (7, 3)).astype(f32) for _ in range(2))
    t = mc.support_times(33)
    lo_, hi_ = mc.clamp_bounds(0.98, -1.0, 2.0)
    whole = mc.waypoints(start, goal, 5, 2, 1.0, lo_, hi_, t)
    for rank in range(4):
        lo, hi = distributed.shard(7, 4, rank)
        part = mc.waypoints(start[lo:hi], goal[lo:hi], 5, 2, 1.0, lo_, hi_, t,
                            problem_offset=distributed.problem_offset(7, 4, rank))
        np.testing.assert_array_equal(part, whole[lo:hi])

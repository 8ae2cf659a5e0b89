"""Clearance of the links against each other, everything that needs no GPU: the fp64 restatement of
tests/self_clearance_cases.py against brute force on every scene, its ties and no-pair case, the error bound, the
C-ABI symbols (declared, exported, bound with the declared types), the report's layout, the IRM_EINVAL paths that need
no device, the CLI flag, the summary file's extra column and the new compilation unit's place in the build."""
import ctypes
import os
import re

import numpy as np
import pytest

import self_clearance_cases as sc
from conftest import REPO

HEADER = os.path.join(REPO, "include", "irm.h")
IRM_EINVAL = -22
SYMBOLS = ["irm_self_clearance", "irm_self_clearance_dev"]


# ------------------------------------------------- the yardstick
@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_restatement_against_brute_force(name):
    """Pairs that do not cross: the restatement may not exceed the nearest pair of 401 × 401 points on the two links,
    and falls short of it by at most half a spacing on either link.  Pairs that cross: the two links meet, so the
    nearest pair of samples lies within the same bound of each other."""
    link = sc.SCENES[name][0]
    q = sc.line(name, 65)
    g, x, _ = sc.self_clearance64(q, link)
    brute = sc.brute_force(q, link)
    slack = sc.brute_spacing(link)[None, :]
    assert np.all(g[~x] <= brute[~x] + 1e-12), (name, float((g - brute)[~x].max()))
    assert np.all((brute - g <= slack)[~x]), (name, float((brute - g)[~x].max()))
    assert np.all((brute <= slack)[x]), (name, float((brute - slack)[x].max()) if x.any() else None)
    assert np.all(g[x] == 0.0)
    print(f"{name}: brute force exceeds the restatement by at most {float((brute - g)[~x].max()):.2e}; "
          f"{int(x.any(axis=1).sum())} crossing samples")


def test_restatement_hand_cases_ties_and_no_pairs():
    # a 4-link arm of unit links folded at right angles: (0,0)→(1,0)→(1,1)→(0,1)→(0,0) closes the square
    g, x, _ = sc.self_clearance64(np.array([[0.0, np.pi / 2, np.pi / 2, np.pi / 2]]), (1.0,) * 4)
    assert sc.pairs(4) == [(0, 2), (0, 3), (1, 3)]
    np.testing.assert_allclose(g[0], [1.0, 0.0, 1.0], atol=1e-15)  # link 3's tip touches link 0's start: no crossing
    assert not x.any()
    # three quarters of a turn further in: link 3 ends on the far side of link 0
    q = np.array([[0.0, np.pi / 2, np.pi / 2, 2.0]])
    g, x, margin = sc.self_clearance64(q, (1.0, 1.0, 0.5, 2.0))
    assert x[0].tolist() == [False, True, False] and g[0, 1] == 0.0 and margin[0, 1] > 0.0
    s = sc.summary64(g, x, 4)
    assert s["argmin"] == (0, 0, 3) and s["n_crossing"] == s["n_colliding"] == 1 and s["first_colliding"] == 0
    # capsules: g = d − 2·link_radius; touching (g = 0 without a crossing) does not collide
    g, x, _ = sc.self_clearance64(np.array([[0.0, np.pi / 2, np.pi / 2]]), (1.0, 1.0, 1.0), link_radius=0.25)
    np.testing.assert_allclose(g, [[0.5]], atol=1e-15)
    s = sc.summary64(np.array([[0.0]]), np.array([[False]]), 3)
    assert s["collision_free"] and s["n_colliding"] == 0
    # two equal minima: the lower (i, a, b)
    s = sc.summary64(np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.5]]), np.zeros((2, 3), bool), 4)
    assert s["argmin"] == (0, 0, 3) and s["min_clearance"] == 0.25
    # no pairs
    for D in (1, 2):
        g, x, _ = sc.self_clearance64(np.zeros((3, D)), (1.0,) * D)
        assert g.shape == (3, 0) and sc.pairs(D) == []
        s = sc.summary64(g, x, D)
        assert s["min_clearance"] == np.inf and s["argmin"] == (-1, -1, -1) and s["collision_free"]
        assert np.all(s["clearance"] == np.inf) and s["first_colliding"] == -1
    assert len(sc.pairs(8)) == 21 and sc.pairs(3) == [(0, 2)]


def test_what_the_scenes_show():
    """self_clearance_cases asserts these at import; here with the numbers."""
    for (name, M), (count, first, which) in sorted(sc.EXPECTED.items(), key=str):
        link = sc.SCENES[name][0]
        g, x, margin = sc.self_clearance64(sc.line(name, M), link)
        s = sc.summary64(g, x, len(link))
        assert (s["n_crossing"], s["first_colliding"]) == (count, first)
        print(f"{name} M={M}: {count} crossing samples from {first}, pairs {sorted(which)}, smallest crossing margin "
              f"{float(margin[x].min()) if x.any() else float('nan'):.2e}, smallest other distance "
              f"{float(g[~x].min()):.2e}")
    g, _, _ = sc.self_clearance64(np.asarray(sc.SCENES["lim3"][1])[None, :], sc.LINKS3)
    assert abs(g.min() - sc.LIM3_MIN_DISTANCE) < 5e-4


def test_tolerance_is_small_and_grows_with_its_inputs():
    for name, (link, _) in sc.SCENES.items():
        for M in (64, 65, 300):
            tol = sc.tolerance(link, sc.max_angle(sc.line(name, M)))
            assert 1e-6 < tol < 1e-5, (name, M, tol)
    base = sc.tolerance(sc.LINKS3, 6.0)
    assert sc.tolerance(sc.LINKS3, 1e4) > base and sc.tolerance(sc.LINKS3, 6.0, link_radius=0.3) > base
    assert sc.tolerance((3.0, 2.0, 1.0), 6.0) > base and sc.tolerance(sc.LINKS7, 6.0) > base
    # the geometry term is clearance_cases.tolerance's: what that bound holds beyond its own arithmetic term
    import clearance_cases as cc
    R, r2 = 3.0, np.sqrt(2.0)
    arithmetic = cc.U32 * ((4.0 * r2 + 4.0) * R + 3.0 * 1.5)
    assert abs((cc.tolerance(sc.LINKS3, 6.0, 0.0) - arithmetic) - sc.geometry_error(sc.LINKS3, 6.0)) < 1e-15


# ------------------------------------------------- the C ABI
def _c_types():
    from irm_motion_planning_amd import _abi, clearance
    return {"irm_ctx*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "float": ctypes.c_float,
            "float*": _abi.c_float_p, "const float*": _abi.c_float_p,
            "irm_self_clearance_report*": ctypes.POINTER(clearance.IrmSelfClearanceReport), "void*": ctypes.c_void_p}


def _declaration(name):
    """(return type, [argument types]) of `name` as include/irm.h declares it."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w[\w\s\*]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, src, re.M)
    assert m, f"{name} is not declared in include/irm.h"
    args = []
    for a in m.group(2).split(","):
        words = a.replace("*", "* ").split()
        args.append(" ".join(words[:-1]).replace(" *", "*"))  # drop the parameter's name
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", SYMBOLS)
def test_declared_exported_and_bound(name):
    from irm_motion_planning_amd._abi import PROTOTYPES, load_library
    types = _c_types()
    ret, args = _declaration(name)
    assert name in PROTOTYPES
    res, argtypes = PROTOTYPES[name]
    assert res is types[ret]
    assert argtypes == [types[a] for a in args], (args, argtypes)
    fn = getattr(load_library(), name)
    assert fn.argtypes == argtypes and fn.restype is res


def test_declared_signatures():
    host = ["irm_ctx*", "const float*", "float", "int32_t", "irm_self_clearance_report*", "float*", "float*", "float*"]
    assert _declaration("irm_self_clearance") == ("int", host)
    assert _declaration("irm_self_clearance_dev") == ("int", host + ["void*"])


def test_report_layout():
    from irm_motion_planning_amd.clearance import (SELF_CLEARANCE_REPORT_FIELDS, IrmClearanceReport,
                                                   IrmSelfClearanceReport)
    assert ctypes.sizeof(IrmSelfClearanceReport) == 32
    f, i = ctypes.c_float, ctypes.c_int32
    assert IrmSelfClearanceReport._fields_ == [
        ("min_clearance", f), ("argmin_time", i), ("argmin_link_a", i), ("argmin_link_b", i), ("n_colliding", i),
        ("first_colliding", i), ("collision_free", i), ("n_crossing", i)]
    assert [getattr(IrmSelfClearanceReport, n).offset for n, _ in IrmSelfClearanceReport._fields_] == list(range(0, 32, 4))
    # n_crossing takes the slot that is padding in irm_clearance_report; what the two share lies at the same offsets
    assert IrmSelfClearanceReport.n_crossing.offset == IrmClearanceReport.pad_.offset
    for name in ("min_clearance", "argmin_time", "n_colliding", "first_colliding", "collision_free"):
        assert getattr(IrmSelfClearanceReport, name).offset == getattr(IrmClearanceReport, name).offset
    assert SELF_CLEARANCE_REPORT_FIELDS == [n for n, _ in IrmSelfClearanceReport._fields_]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct irm_self_clearance_report \{(.*?)\} irm_self_clearance_report;", src, re.S).group(1)
    declared = []
    for stmt in body.split(";"):
        words = stmt.replace(",", " ").split()
        if words:
            declared += [(w, {"float": f, "int32_t": i}[words[0]]) for w in words[1:]]
    assert declared == IrmSelfClearanceReport._fields_


def test_pair_order_of_the_binding():
    from irm_motion_planning_amd.clearance import self_pairs
    for D in range(1, 9):
        assert self_pairs(D) == sc.pairs(D) and len(self_pairs(D)) == max((D - 1) * (D - 2) // 2, 0)


def test_abi_version_unchanged():
    from irm_motion_planning_amd import _abi
    from irm_motion_planning_amd.clearance import IrmClearanceReport
    from irm_motion_planning_amd.multistart import IrmMultistart
    assert _abi.IRM_ABI_VERSION == 3
    assert re.search(r"#define IRM_ABI_VERSION 3\b", open(HEADER).read())
    assert ctypes.sizeof(_abi.IrmDenseReport) == 40 and ctypes.sizeof(IrmClearanceReport) == 32  # no struct moved
    assert "rank_self_clearance" not in [n for n, _ in IrmMultistart._fields_]  # the descriptor keeps its layout


def test_null_arguments_are_einval_and_name_the_function():
    from irm_motion_planning_amd._abi import c_float_p, load_library
    from irm_motion_planning_amd.clearance import IrmSelfClearanceReport
    lib = load_library()
    x = np.zeros(8, np.float32)
    p = x.ctypes.data_as(c_float_p)
    rep = (IrmSelfClearanceReport * 1)()
    assert lib.irm_self_clearance(None, p, 0.0, 1, rep, None, None, None) == IRM_EINVAL
    assert b"irm_self_clearance:" in lib.irm_last_error()
    assert lib.irm_self_clearance_dev(None, p, 0.0, 1, rep, None, None, None, None) == IRM_EINVAL
    assert b"irm_self_clearance_dev:" in lib.irm_last_error()


# ------------------------------------------------- CLI, files, build
def test_cli_flag():
    from irm_motion_planning_amd import main
    assert main.parse_args([]).self_clearance == 0
    a = main.parse_args(["--self-clearance", "65", "--link-radius", "0.05"])
    assert (a.self_clearance, a.link_radius, a.clearance) == (65, 0.05, 0)
    for bad in (["--self-clearance", "-3"], ["--self-clearance", "1.5"], ["--self-clearance", "x"]):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
    # the same sample-count type as --clearance
    actions = {a.dest: a for a in main.build_parser()._actions}
    assert actions["self_clearance"].type is actions["clearance"].type


def test_summary_file_gains_a_column_only_with_the_flag(tmp_path):
    from irm_motion_planning_amd import batch_io
    stats = {k: np.array([3, 4]) for k in ("inner_iterations", "outer_iterations", "grad_evals")}
    args = ([0.5, 0.25], [1.5, 1.25], [True, False], stats)
    batch_io.write_summary(tmp_path / "plain.txt", *args)
    batch_io.write_summary(tmp_path / "none.txt", *args, min_self_clearance=None)
    batch_io.write_summary(tmp_path / "self.txt", *args, min_self_clearance=np.array([0.125, 0.0], np.float32))
    batch_io.write_summary(tmp_path / "both.txt", *args, min_clearance=np.array([0.25, -0.5], np.float32),
                           min_self_clearance=np.array([0.125, np.inf], np.float32))
    plain = (tmp_path / "plain.txt").read_text()
    assert plain == "# avg_cost max_cost constraints_ok inner_iterations outer_iterations grad_evals\n" \
                    "0.5 1.5 1 3 3 3\n0.25 1.25 0 4 4 4\n"
    assert (tmp_path / "none.txt").read_text() == plain
    assert (tmp_path / "self.txt").read_text() == \
        "# avg_cost max_cost constraints_ok inner_iterations outer_iterations grad_evals min_self_clearance\n" \
        "0.5 1.5 1 3 3 3 0.125\n0.25 1.25 0 4 4 4 0\n"
    assert (tmp_path / "both.txt").read_text() == \
        "# avg_cost max_cost constraints_ok inner_iterations outer_iterations grad_evals min_clearance " \
        "min_self_clearance\n0.5 1.5 1 3 3 3 0.25 0.125\n0.25 1.25 0 4 4 4 -0.5 inf\n"


def test_self_clearance_unit_is_built():
    from irm_motion_planning_amd import build
    units = {u[0]: u for u in build.units()}
    assert units["irm_self_clearance"][1:] == ("irm_self_clearance.hip", [])
    assert units["irm_clearance"][1:] == ("irm_clearance.hip", [])
    for f in ("irm_self_clearance.hip", "irm_fk_prefix.hpp"):
        assert os.path.join(build.CSRC, f) in build.source_files()
    assert os.path.join(build.CSRC, "irm_fk_prefix.hpp") in build.HEADERS
    full = build.source_hash()
    orig = build._units
    try:
        build._units = lambda: [u for u in orig() if u[0] != "irm_self_clearance"]
        assert build.source_hash() != full
    finally:
        build._units = orig


def test_shared_fk_prefix_header_is_used_by_both_units():
    """fk_prefix lives in one header; neither clearance unit keeps a copy of the two-sum prefix."""
    from irm_motion_planning_amd import build
    read = lambda f: open(os.path.join(build.CSRC, f)).read()  # noqa: E731
    shared = read("irm_fk_prefix.hpp")
    assert "void fk_prefix(" in shared and "sincos_poly(" in shared
    for unit in ("irm_clearance.hip", "irm_self_clearance.hip"):
        src = read(unit)
        assert '#include "irm_fk_prefix.hpp"' in src and '#include "irm_dense_sample.hpp"' in src
        assert "fk_prefix<D>(" in src
        assert "void fk_prefix(" not in src and "sincos_poly(" not in src and "tail[" not in src


def test_launcher_is_declared_beside_the_clearance_launcher():
    from irm_motion_planning_amd import build
    src = open(os.path.join(build.CSRC, "irm_kernels.hpp")).read()
    assert src.index("launch_clearance(") < src.index("launch_self_clearance(") < src.index("launch_fit_alpha(")

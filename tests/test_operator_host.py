"""The library's own operator build on a CPU: csrc/irm_operator.cpp (build_operators, fill_kparams,
choose_shape — what irm_ctx_create uploads and passes to every kernel) compiled with a plain host
compiler together with tests/host/operator_dump.cpp, no HIP and no library, and its dumps checked
against numpy: the fragment layouts, the zeroed endpoint columns, the rank slots, the endpoint
operator columns, the initTrajectory basis, the fp32 constants of KParams and the workgroup shapes.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(REPO, "tests", "host", "operator_dump.cpp"),
           os.path.join(REPO, "irm_motion_planning_amd", "csrc", "irm_operator.cpp")]
U = 2.0 ** -24  # fp32 unit roundoff

# (N, D, rank, sigma, cvdl): the smallest configurations that reach each path
C18 = (18, 2, 0, 0.1, 1)      # R = 18 < RP = 32, N not a multiple of 16, padding rows
C50 = (50, 3, 0, 0.1, 1)      # R = 32, NK = 64
C50R16 = (50, 3, 16, 0.1, 1)  # explicit rank: R = RP = 16, trunc = λ16/λ0
C128F = (128, 3, 0, 0.07, 1)  # flat spectrum: all 32 components above fp64 noise, lean_ok = 0
C128D7 = (128, 7, 0, 0.1, 0)  # 7-DoF J, cvdl = false thresholds, lean_ok = 1
CDENSE = (40, 3, -1, 0.1, 1)  # dense operator: V = I, RP = 48, v_ident = 1
CONFIGS = [C18, C50, C50R16, C128F, C128D7, CDENSE]
SIGMA01 = [c for c in CONFIGS if c[3] == 0.1]
IDS = lambda c: "N%d-D%d-r%d-s%g-c%d" % c  # noqa: E731

INTS = {"R", "RP", "NK", "MP", "p.max_inner_iteration", "p.max_outer_iteration"} | {"kp." + k for k in (
    "N", "D", "R", "NK", "MP", "RP", "v_ident", "O", "optimizer", "max_inner", "max_outer", "max_bls", "cvdl",
    "record_series", "max_series", "lean_ok", "lean_wpl", "lean_nohelp", "trace_b", "whole_robot", "queue_groups")}
UINTS = {"kp.Nmagic", "kp.NDmagic"}


def _compile(out, flags):
    """g++ of the dump program and irm_operator.cpp.  No g++: skip; a compile error: failure."""
    try:
        subprocess.run(["g++", "--version"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except OSError:
        pytest.skip("no g++")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out] + SOURCES)
    return out


def _env():
    """The environment without the library's switches (read_env_switches, IRM_PAD_WAVES)."""
    return {k: v for k, v in os.environ.items() if not k.startswith("IRM_")}


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("operator_dump") / "operator_dump"), ["-O2"])


def _read(path):
    d, b, i = {}, open(path, "rb").read(), 0
    while i < len(b):
        j = b.index(b"\n", i)
        name, n = b[i:j].split()
        d[name.decode()] = b[j + 1:j + 1 + int(n)]
        i = j + 1 + int(n) + 1
    return d


def _decode(raw):
    """Records as numpy values: int32 / uint32 for the names listed above, float32 otherwise; one element: a scalar."""
    out = {}
    for k, v in raw.items():
        a = np.frombuffer(v, np.int32 if k in INTS else np.uint32 if k in UINTS else np.float32)
        out[k] = a[0] if a.size == 1 else a
    return out


@functools.lru_cache(maxsize=None)
def _dump_cached(exe, cfg, tmp):
    path = os.path.join(tmp, IDS(cfg) + ".bin")
    subprocess.check_call([exe, "ops", path] + [str(x) for x in cfg], env=_env(), timeout=120)
    return _decode(_read(path))


@pytest.fixture(scope="module")
def ops_of(dump_exe):
    """cfg -> the decoded dump, built once per configuration and shared (read-only) by the tests."""
    tmp = os.path.dirname(dump_exe)
    return lambda cfg: _dump_cached(dump_exe, cfg, tmp)


def frag_decode(buf, M, K, kperm):
    """Row-major M×K matrix out of a 16x16x4 A-fragment buffer (frag_index / frag_index_kp of irm_layout.hpp);
    asserts that every float no (row, k) maps to is 0."""
    KQ = (K + 15) // 16
    r, k = np.meshgrid(np.arange(M), np.arange(K), indexing="ij")
    mt, kq, kk = r // 16, k // 16, k % 16
    lane = np.where(kperm, (r % 16) + 16 * (kk // 4), (r % 16) + 16 * (kk % 4))
    j = np.where(kperm, kk % 4, kk // 4)
    idx = ((mt * KQ + kq) * 64 + lane) * 4 + j
    assert buf.size == ((M + 15) // 16) * KQ * 256
    used = np.zeros(buf.size, bool)
    used[idx.ravel()] = True
    assert used.sum() == M * K and not buf[~used].any(), "fragment padding is not zero"
    return buf[idx]


class Ops:
    """Decoded views of one dump."""

    def __init__(self, d):
        self.d = d
        self.N, self.D = int(d["kp.N"]), int(d["kp.D"])
        self.R, self.RP, self.NK, self.MP = int(d["R"]), int(d["RP"]), int(d["NK"]), int(d["MP"])
        N, RP, NK, MP = self.N, self.RP, self.NK, self.MP
        self.K, self.dK = d["K"].reshape(N, N), d["dK"].reshape(N, N)
        self.F2 = frag_decode(d["F2"], MP, RP, False)
        self.F1 = frag_decode(d["F1"], RP, MP, False)
        self.Vr = d["Vr"].reshape(N, RP)
        self.L = np.vstack([self.K, self.dK]).astype(np.float64)
        self.F = np.vstack([self.F2[:N], self.F2[NK:NK + N]]).astype(np.float64)
        self.V = self.Vr.astype(np.float64)
        self.J = d["p.jac"][:self.D * self.D].reshape(self.D, self.D).astype(np.float64)


@pytest.fixture(scope="module")
def view(ops_of):
    cache = {}

    def get(cfg):
        if cfg not in cache:
            cache[cfg] = Ops(ops_of(cfg))
        return cache[cfg]
    return get


EXPECT_SHAPES = {C18: (18, 32, 32, 64), C50: (32, 32, 64, 128), C50R16: (16, 16, 64, 128),
                 C128F: (32, 32, 128, 256), C128D7: (32, 32, 128, 256), CDENSE: (40, 48, 48, 96)}


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_layouts_are_exact(view, cfg):
    """Bit-equal: transposes, the two fragment layouts of each matrix, the zeroed endpoint columns of Fᵀ, the
    padding rows, Fbot, the four V_R fragment buffers."""
    o = view(cfg)
    d, N, RP, NK, MP = o.d, o.N, o.RP, o.NK, o.MP
    assert (o.R, RP, NK, MP) == EXPECT_SHAPES[cfg]
    assert (int(d["kp.R"]), int(d["kp.RP"]), int(d["kp.NK"]), int(d["kp.MP"])) == (o.R, RP, NK, MP)
    assert np.array_equal(d["Kt"].reshape(N, N), o.K.T) and np.array_equal(d["dKt"].reshape(N, N), o.dK.T)
    assert np.array_equal(o.F2, frag_decode(d["F2p"], MP, RP, True))
    assert np.array_equal(o.F1, frag_decode(d["F1p"], RP, MP, True))
    F1x = o.F2.T.copy()
    F1x[:, NK] = 0
    F1x[:, NK + N - 1] = 0
    assert np.array_equal(o.F1, F1x)
    assert o.F2[NK].any() and o.F2[NK + N - 1].any()  # (the columns that F1 leaves out are not zero in F)
    assert not o.F2[N:NK].any() and not o.F2[NK + N:].any()
    assert np.array_equal(d["Fbot"].reshape(N, RP), o.F2[NK:NK + N])
    for name, M_, K_, kperm, tr in (("VTp", RP, NK, True, True), ("VTs", RP, NK, False, True),
                                    ("VNp", NK, RP, True, False), ("VNs", NK, RP, False, False)):
        m = frag_decode(d[name], M_, K_, kperm)
        m = m.T if tr else m
        assert np.array_equal(m[:N], o.Vr) and not m[N:].any(), name
    assert np.count_nonzero(np.abs(o.Vr).sum(0)) == o.R  # exactly R columns of V_R are used
    assert d["u"].shape == (N,) and d["w"].shape == (N,) and d["H"].shape == (2 * MP,) and d["HV"].shape == (2 * NK,)


def test_dense_operator_is_the_kernel_matrices(view):
    o = view(CDENSE)
    assert np.array_equal(o.Vr[:, :o.N], np.eye(o.N, dtype=np.float32)) and not o.Vr[:, o.N:].any()
    assert np.array_equal(o.F2[:o.N, :o.N], o.K) and np.array_equal(o.F2[o.NK:o.NK + o.N, :o.N], o.dK)
    assert not o.F2[:, o.N:].any()
    assert o.d["trunc"] == 0 and o.d["lam16"] == 0 and o.d["lam24"] == 0
    assert int(o.d["kp.v_ident"]) == 1
    assert all(int(view(c).d["kp.v_ident"]) == 0 for c in CONFIGS if c != CDENSE)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_factorisation(view, cfg):
    """V_R orthonormal, F = L·V_R, and the rank-R operator in the α-space update (test_host.py's assertion
    on the library's F)."""
    o = view(cfg)
    cols = np.flatnonzero(np.abs(o.V).sum(0) > 0)
    Vc = o.V[:, cols]
    # each entry of V_R carries one fp32 rounding: a unit column pair moves by ≤ 2u; 4u leaves a factor 2
    orth = np.abs(Vc.T @ Vc - np.eye(len(cols))).max()
    fv = np.abs(o.F - o.L @ o.V).max() / np.abs(o.F).max()
    rng = np.random.default_rng(o.N)
    ab = rng.standard_normal((2 * o.N, o.D))
    a, b = ab[:o.N], ab[o.N:]
    K, dK, J = o.K.astype(np.float64), o.dK.astype(np.float64), o.J
    G_alpha = (K.T @ a + dK.T @ b) @ J.T  # trajectory.py:284-297
    full = o.L @ (G_alpha @ J)
    low = o.F @ (o.F.T @ ab) @ (J.T @ J)
    lowrank = np.abs(full - low).max() / np.abs(full).max()
    print(f"{IDS(cfg)}: |VtV-I| {orth:.2e}  |F-LV|/|F| {fv:.2e}  low-rank update {lowrank:.2e}")
    assert orth <= 4 * U
    assert fv <= 1e-6
    assert lowrank <= 1e-6


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_endpoint_columns(view, cfg):
    """Hend and HV against F·F[NK]ᵀ, F·F[NK+N−1]ᵀ, V_R·F[NK]ᵀ, V_R·F[NK+N−1]ᵀ in fp64 from the decoded values."""
    o = view(cfg)
    N, NK, MP = o.N, o.NK, o.MP
    Fk = o.F2.astype(np.float64)
    H, HV = o.d["H"].reshape(2, MP), o.d["HV"].reshape(2, NK)
    Hx = np.stack([Fk @ Fk[NK], Fk @ Fk[NK + N - 1]])
    HVx = np.stack([o.V @ Fk[NK], o.V @ Fk[NK + N - 1]])
    herr = np.abs(H - Hx).max() / np.abs(Hx).max()
    hverr = np.abs(HV[:, :N] - HVx).max() / np.abs(HVx).max()
    print(f"{IDS(cfg)}: H {herr:.2e}  HV {hverr:.2e}")
    assert herr <= 1e-6 and hverr <= 1e-6
    assert not HV[:, N:].any() and not H[:, N:NK].any() and not H[:, NK + N:].any()


def slot(r, RP):
    """Rank slot of component r (build_operators): at RP = 32 the second k-quad interleaves 16-23 and 24-31."""
    if RP != 32 or r < 16:
        return r
    j = r - 16
    q = j & 7
    return 16 + 4 * (q >> 1) + (q & 1) + (2 if j >= 8 else 0)


def test_slot_order_and_spectrum_ratios(view):
    """N = 128, σ = 0.07: every one of the 32 components is above fp64 noise, and ‖F[:, slot(r)]‖² is within 10 %
    of numpy's r-th eigenvalue of LᵀL for every r < 32.  Among the permuted components (r ≥ 16) neighbouring
    eigenvalues differ by ≥ 2.5×, so 10 % pins each of them to its slot (the leading eigenvalues come in
    near-equal pairs, but slot(r) = r there)."""
    o = view(C128F)
    w = np.linalg.eigvalsh(o.L.T @ o.L)[::-1]
    assert np.all(w[15:32] / w[16:33] >= 2.5)
    nrm = (o.F ** 2).sum(0)
    comp = np.array([nrm[slot(r, o.RP)] for r in range(o.R)])
    dev = np.abs(comp / w[:32] - 1).max()
    ratios = {"trunc": w[32] / w[0], "lam16": w[16] / w[0], "lam24": w[24] / w[0]}
    print(f"slot deviation {dev:.2e}; " + "  ".join(f"{k} {float(o.d[k]):.3e} (numpy {v:.3e})" for k, v in ratios.items()))
    assert dev <= 0.1
    for k, v in ratios.items():
        assert abs(float(o.d[k]) / v - 1) <= 0.01, k
    assert int(o.d["kp.lean_ok"]) == 0  # λ16/λ0 ≈ 4e-4: the lean kernel's rank cuts do not hold


@pytest.mark.parametrize("cfg", [c for c in SIGMA01 if c != CDENSE], ids=IDS)
def test_lean_gate_at_sigma_01(view, cfg):
    """σ = 0.1: the tail of the spectrum is fp64 noise, only the gate is asserted."""
    d = view(cfg).d
    assert d["lam16"] <= 1e-6 and d["lam24"] <= 1e-14
    assert int(d["kp.lean_ok"]) == 1
    if cfg == C50R16:
        # λ16/λ0 ≈ 1.5e-7 is far above the eigenvalues' fp64 error (≈ 1e-16·λ0, relative 1e-9): 1 % as above
        o = view(cfg)
        w = np.linalg.eigvalsh(o.L.T @ o.L)[::-1]
        assert abs(float(d["trunc"]) / (w[16] / w[0]) - 1) <= 0.01
        assert d["lam16"] == 0 and d["lam24"] == 0  # components 16, 24 are not in a rank-16 operator


@pytest.mark.parametrize("cfg", SIGMA01, ids=IDS)
def test_init_trajectory_basis(view, cfg):
    """K is singular, so only K·u, K·w are meaningful: within 1e-3 of 1 − c, c (twice DESIGN's 5e-4 bound)."""
    o = view(cfg)
    cc = np.linspace(0, 1, o.N, dtype=np.float32).astype(np.float64)
    cv = 6 * cc ** 5 - 15 * cc ** 4 + 10 * cc ** 3
    K = o.K.astype(np.float64)
    ru = np.abs(K @ o.d["u"].astype(np.float64) - (1 - cv)).max()
    rw = np.abs(K @ o.d["w"].astype(np.float64) - cv).max()
    print(f"{IDS(cfg)}: |K·u − (1 − c)| {ru:.2e}  |K·w − c| {rw:.2e}")
    assert ru <= 1e-3 and rw <= 1e-3


# Worst |J⁻¹·J − I| and |(JᵀJ)⁻¹·JᵀJ − I| (fp64 products of the stored fp32 values) over CONFIGS, measured on the
# commit before the split (from the KParams block of its contexts, created behind a stub HIP header): 1.31e-7 and
# 7.2e-8, both at D = 7 (D = 3: 1.7e-8 and 4.3e-8; D = 2: 9.4e-9 and 1.8e-8).  J⁻¹ is a D×D fp32 LU, (JᵀJ)⁻¹ an
# fp64 Gauss-Jordan stored in fp32; the bounds are 4× the measured.
JINV_BOUND, MINV_BOUND = 4 * 1.31e-7, 4 * 7.2e-8


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_kparams_scalars(view, cfg):
    """Every derived fp32 constant equals its numpy float32 restatement, exactly."""
    o = view(cfg)
    d, N, D = o.d, o.N, o.D
    f32, f64 = np.float32, np.float64
    kp = lambda k: d["kp." + k]  # noqa: E731
    lreg, lr = f32(d["p.lambda_reg"]), d["p.gd_lr"]
    for i in range(lr.size):
        prod = f32(lreg * f32(lr[i]))  # the product rounds to fp32 first, then the difference
        assert kp("gd_c")[i] == f32(f32(1) - prod), i
    assert np.array_equal(kp("gd_lr"), lr)
    pmax, pmin, vmax = f32(d["p.max_joint_position"]), f32(d["p.min_joint_position"]), f32(d["p.max_joint_velocity"])
    jsl = f32(d["p.joint_safety_limit"])
    mean = 0.5 * (f64(pmax) + f64(pmin))
    assert kp("mean_pos") == f32(mean) and kp("std_pos") == f32(0.5 * (f64(pmax) - mean))
    assert kp("std2") == f32(kp("std_pos") * kp("std_pos")) and kp("vmax2") == f32(vmax * vmax)
    if cfg[4]:
        want = (f32(f64(jsl) * f64(pmax)), f32(f64(jsl) * f64(pmin)), f32(f64(jsl) * f64(vmax)))
    else:
        want = (f32(-np.inf), f32(np.inf), f32(-1))
    assert (kp("thr_hi"), kp("thr_lo"), kp("thr_v")) == want
    assert int(kp("cvdl")) == cfg[4]
    assert kp("invN") == f32(1) / f32(N)
    assert kp("inv_std_pos") == f32(1) / kp("std_pos") and kp("inv_vmax") == f32(1) / vmax
    assert kp("inv_std2") == f32(1) / kp("std2") and kp("inv_vmax2") == f32(1) / kp("vmax2")
    assert int(kp("Nmagic")) == -(-2 ** 32 // N) and int(kp("NDmagic")) == -(-2 ** 32 // (N * D))
    assert kp("one_m_lmax") == f32(1.0 - f64(f32(d["p.lambda_max_cost"]))) and kp("lam_max") == d["p.lambda_max_cost"]
    assert int(kp("max_series")) == 1 + int(d["p.max_outer_iteration"]) * int(d["p.max_inner_iteration"])
    assert (int(kp("lean_wpl")), int(kp("lean_nohelp")), int(kp("trace_b")), int(kp("queue_groups"))) == (0, 0, 0, 0)
    J32 = d["p.jac"][:D * D].reshape(D, D)
    assert np.array_equal(kp("J")[:D * D].reshape(D, D), J32) and np.array_equal(kp("link"), d["p.link_length"])
    JtJ = np.zeros((D, D))
    for k in range(D):  # Σ_k J[k][a]·J[k][b] in fp64, k ascending as fill_kparams sums it
        JtJ += np.outer(o.J[k], o.J[k])
    assert np.array_equal(kp("JtJ")[:D * D].reshape(D, D), JtJ.astype(f32))
    Jinv = kp("Jinv")[:D * D].reshape(D, D).astype(f64)
    Minv = kp("Minv")[:D * D].reshape(D, D).astype(f64)
    ej = np.abs(Jinv @ o.J - np.eye(D)).max()
    em = np.abs(Minv @ JtJ - np.eye(D)).max()
    ew = np.abs(kp("wal")[:D] - Minv @ (o.J.T @ np.ones(D))).max()
    print(f"{IDS(cfg)}: |Jinv·J − I| {ej:.2e}  |Minv·JtJ − I| {em:.2e}  |wal − Minv·Jt1| {ew:.2e}")
    assert ej <= JINV_BOUND and em <= MINV_BOUND


# choose_shape for num_cus = 256, optimiser launches, RP = 32, traj_per_block = 0:
# (N, D, B, O) -> "TB BT nsplit regops ops_in_lds lds_bytes".  The table was produced from the commit before the
# split (its choose_shape called through a stub-HIP harness), not from this code.
SHAPES = {
    (128, 3, 1, 10): "1 512 2 1 1 43408",       # bench C2
    (128, 3, 1024, 11): "4 512 2 1 1 43408",    # C3
    (256, 3, 1024, 50): "4 1024 4 0 0 82896",   # C4
    (256, 7, 512, 11): "2 512 4 0 0 82576",     # C5
    (128, 7, 1024, 11): "2 256 2 1 1 43408",    # C7
    (128, 3, 8192, 11): "4 512 2 1 1 43408",    # C3 at B = 8192
    (50, 3, 256, 11): "1 256 1 1 1 23824",
    (64, 3, 256, 11): "1 256 1 1 1 23824",
    (512, 3, 1, 11): "1 512 8 0 0 160912",
}


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "N%d-D%d-B%d-O%d" % s)
def test_choose_shape(dump_exe, shape):
    N, D, B, O = shape
    out = subprocess.check_output([dump_exe, "shape", str(N), str(D), "32", str(B), str(O), "0", "256"], env=_env(),
                                  timeout=60)
    assert out.decode().strip() == SHAPES[shape]


def test_operator_build_is_clean_under_sanitizers(tmp_path):
    """The same two sources with AddressSanitizer and UBSan, stand-alone (the runtimes are linked into the
    program, nothing is preloaded), on the N = 18, N = 50 and dense configurations."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    try:
        r = subprocess.run(["g++"] + san + ["-o", str(tmp_path / "probe"), str(probe)], stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
    except OSError:
        pytest.skip("no g++")
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime cannot be linked")
    exe = _compile(str(tmp_path / "operator_dump_san"), ["-O1", "-g"] + san)
    for cfg in (C18, C50, CDENSE):
        r = subprocess.run([exe, "ops", str(tmp_path / "san.bin")] + [str(x) for x in cfg], env=_env(), timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, (cfg, r.stdout.decode()[-2000:])

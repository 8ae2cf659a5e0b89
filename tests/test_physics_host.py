"""sincos_poly (irm_physics.hpp) on the CPU: its C restatement (tests/physics_cases.py, SINCOS_C; fmaf,
-ffp-contract=off) measured against double sin / cos, the committed bit-pattern fixture regenerated, two mutants
of the restatement shown to miss the bounds, and the references and inputs of tests/test_gpu_physics.py checked
where that needs no device.

Measured on the full probe set (1.07e8 angles with |x| ≤ 1e4): sin 1.560 ulp at x = −922.8229, cos 1.560 ulp at
x = 5427.910, both next to an odd multiple of π/4 (a run with other random draws: 1.558 at −2006.658, 1.562 at
1840.216; next to multiples of π/2 the worst are 1.30 and 1.40 ulp); |sin² + cos² − 1| ≤ 1.63e-7 = 2.74·2⁻²⁴."""
import numpy as np
import pytest

import physics_cases as pc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = pc.compile_sincos(tmp_path_factory.mktemp("sincos"))
    if e is None:
        pytest.skip("no host C compiler")
    return e


def test_sincos_poly_is_within_two_ulp_of_double(exe):
    """< 2 ulp of the correctly rounded fp32 result for sin and for cos, and sin² + cos² within 4·2⁻²⁴ of 1 per
    input, over: every fp32 within ±64 ulps of every multiple of π/2 and of every odd multiple of π/4 with
    |x| ≤ 1e4, 2²⁶ random bit patterns (those with |x| ≤ 1e4: denormals, ±0, tiny values), 2²⁵ uniform draws in
    [−1e4, 1e4] and 2²⁵ in [−8, 8].  The maximum is a sampled one; the margin up to 2 covers that."""
    m = pc.measure(exe)
    print(f"{m['n']} angles: sin {m['sin_ulp']:.3f} ulp at x = {m['sin_at']!r}, cos {m['cos_ulp']:.3f} ulp at "
          f"x = {m['cos_at']!r}, |sin² + cos² − 1| ≤ {m['identity']:.3e} = {m['identity'] * 2 ** 24:.2f}·2⁻²⁴ at "
          f"x = {m['identity_at']!r} ({m['identity_bad']} above the bound)")
    assert m["n"] > 1.0e8
    pc.assert_sincos_bounds(m)


@pytest.mark.parametrize("mutant", sorted(pc.MUTANTS))
def test_mutants_of_the_restatement_miss_the_bounds(tmp_path, mutant):
    """The sine's sign taken from q + 1 instead of q, and the second reduction constant dropped: each, compiled
    from the same source with a -D switch, fails the assertions of the test above (on a 2²⁰-pattern share of its
    probes: a mutant need not be hunted for)."""
    e = pc.compile_sincos(tmp_path, mutant)
    if e is None:
        pytest.skip("no host C compiler")
    m = pc.measure(e, log2_patterns=20, parts=2)
    print(f"{mutant}: sin {m['sin_ulp']:.3g} ulp at {m['sin_at']!r}, cos {m['cos_ulp']:.3g} ulp at {m['cos_at']!r}, "
          f"identity off by {m['identity']:.3g}")
    with pytest.raises(AssertionError):
        pc.assert_sincos_bounds(m)


def test_unmutated_restatement_meets_the_bounds_on_the_mutants_probe_set(exe):
    """The guard of the test above: on that reduced probe set the restatement itself passes."""
    pc.assert_sincos_bounds(pc.measure(exe, log2_patterns=20, parts=2))


def test_committed_fixture_is_what_the_restatement_writes(exe):
    """tests/golden/physics_sincos.npz regenerated: the same angles and the same sin / cos bit patterns."""
    new, old = pc.make_fixture(exe), pc.load_fixture()
    assert sorted(old) == sorted(new) == ["cos_bits", "sin_bits", "x"]
    for k in new:
        assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape, k
    np.testing.assert_array_equal(old["x"].view(np.uint32), new["x"].view(np.uint32))
    np.testing.assert_array_equal(old["sin_bits"], new["sin_bits"])
    np.testing.assert_array_equal(old["cos_bits"], new["cos_bits"])


def test_fixture_angles_are_the_stated_ones():
    fx = pc.load_fixture()
    x = fx["x"]
    assert x.dtype == np.float32 and 4000 < x.shape[0] <= 8192 and np.abs(x).max() == np.float32(1e4)
    have = set(x.view(np.uint32).tolist())
    f32 = np.float32
    top = f32(1e4)
    for v in (f32(0.0), f32(-0.0), f32(2.0 ** -149), f32(-2.0 ** -149), f32(2.0 ** -126), f32(-2.0 ** -126), top, -top,
              np.nextafter(top, f32(0)), -np.nextafter(top, f32(0))):
        assert int(np.array(v, f32).view(np.uint32)) in have, v
    for k in (-40, -3, 0, 1, 2, 40):
        for c in (k * np.pi / 2, (2 * k + 1) * np.pi / 4):
            c32 = f32(c)
            for y in (c32, np.nextafter(np.nextafter(c32, f32(np.inf)), f32(np.inf)),
                      np.nextafter(np.nextafter(c32, f32(-np.inf)), f32(-np.inf))):
                assert int(np.array(y, f32).view(np.uint32)) in have, (k, y)
    # against double: the fixture's values are sin / cos within the measured bound
    s, c = fx["sin_bits"].view(np.float32), fx["cos_bits"].view(np.float32)
    x64 = x.astype(np.float64)
    es, ec = pc.ulp_error(s, np.sin(x64)), pc.ulp_error(c, np.cos(x64))
    print(f"{x.shape[0]} angles: sin {es.max():.3f} ulp, cos {ec.max():.3f} ulp")
    assert es.max() < pc.ULP_BOUND and ec.max() < pc.ULP_BOUND
    # every quadrant, both signs of k
    k = pc.quadrants(x)
    assert {(int(q), bool(neg)) for q, neg in zip(k % 4, k < 0)} >= {(q, neg) for q in range(4) for neg in (False, True)}
    fb = pc.fallback_angles()
    assert fb.dtype == np.float32 and np.all(np.abs(fb) > top) and np.abs(fb).max() == f32(1e7)
    assert np.nextafter(top, f32(np.inf)) in fb and -np.nextafter(top, f32(np.inf)) in fb


# ---------------------------------------------------------------- the device tests' references, on the CPU
def test_references_agree_with_ref64_at_small_angles():
    """CumRef64 with an fp64 cumulative sum in place of the fp32 one is Ref64 (λsg = λjl = 0); with the fp32 one it
    stays within the sum's rounding at small angles.  End effector and whole robot (MovingRef64)."""
    import moving_cases as mc
    for whole in (False, True):
        R, o = mc.restatement(*mc.shape_argv(50, 3), whole_robot=whole)
        t, K, dK, J = o.kernel_matrices()
        link = [float(o.params.link_length[i]) for i in range(3)]
        C = pc.CumRef64(link, K, dK, J, whole)
        rng = np.random.default_rng(2)
        a = (0.2 * rng.standard_normal((50, 3))).astype(np.float32)
        obs = pc.sweep_obstacles(13, (9.0, 9.0))[2:-2]  # the ordinary obstacles
        obs = obs[np.abs(obs).max(1) < 10]
        T, V = R.traj_vel(a)
        T32 = T.astype(np.float32)
        T64, V64 = T32.astype(np.float64), V
        s = g = np.zeros(3)
        for lmax in (0.0, 0.5):
            want = R.cost_tv(T64, V64, obs, s, g, 0.0, 0.0, lmax)
            assert abs(C.cost(T32, obs, lmax) - want) <= 2e-6 * abs(want)
            ga, gb = R.grad_ab(T64, V64, obs, s, g, 0.0, 0.0, lmax)
            assert not gb.any()
            Gw = (R.K.T @ ga) @ R.J.T
            assert np.abs(C.grad(T32, obs, lmax) - Gw).max() <= 2e-6 * np.abs(Gw).max()


def test_potential64_degenerate_geometry():
    """An obstacle on the point gives 1.6 and no gradient; at 1e6 it adds 1.6e-12; beyond 1e19 it adds less than
    1e-37 (the device: exactly 0); an empty table gives zeros."""
    on = np.array([0.25, -1.5], np.float32)
    x, y = np.array([0.25]), np.array([-1.5])
    obs = pc.sweep_obstacles(4, on)
    assert np.array_equal(obs[0], on) and abs(np.hypot(*obs[3].astype(np.float64)) - 1e6) < 1
    assert np.abs(obs[2]).min() >= 1e19
    cv, gx, gy = pc.potential64(x, y, obs[:1])
    assert cv[0] == 1.6 and gx[0] == 0 and gy[0] == 0
    assert abs(pc.potential64(x, y, obs[3:4])[0][0] - 1.6e-12) < 1e-16
    assert pc.potential64(x, y, obs[2:3])[0][0] < 1e-37
    assert not any(v.any() for v in pc.potential64(x, y, np.zeros((0, 2))))
    for O in pc.OBSTACLE_COUNTS:
        t, w = pc.sweep_obstacles(O, on), pc.sweep_velocities(O)
        assert t.shape == w.shape == (O, 2) and np.isfinite(t).all()
        if O >= 2:
            assert np.array_equal(t[0], on) and not w[0].any()
        if O >= 3:
            assert (np.abs(t) > 1e19).any()


def test_wave_kinds():
    c = np.zeros((1, 200, 3), np.float32)
    c[0, 64:128, 1] = 2e4          # every lane above
    c[0, 130, 2] = -2e4            # one lane above
    c[0, 192:, 0] = 1.0001e4       # the ragged wave, all above
    assert pc.wave_kinds(c).tolist() == [[0, 2, 1, 2]]

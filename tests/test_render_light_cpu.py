"""The light-sampled render in its float64 restatement (tests/light_ref.py): the light density of a map is a density, the sample table
carries the pdf of its own directions, and on a map with a sun a few texels wide the multiple-importance-sampling estimator reaches the
project's convergence bar where the plain quadrature is more than 5 % off.  No GPU.

The sun scene and its texel-sum references live in tests/golden/render_light_sun.npz (tools/make_golden_light.py).  Figures of the scene
(R = 8, S = 2, rel-L2 against the supersample-4 texel sum), for z = (0, .7, .5, .3, .5, .6) / (.4, .7, .5, .3, 1, .2):
    plain quadrature Q = 32        1.7e-1 / 1.6e-1
    light samples M = 256          5.0e-3 / 4.9e-3
    light samples M = 1024         1.3e-3 / 1.3e-3
    light samples M = 4096         4.0e-4 / 4.1e-4
The supersample-4 and supersample-8 texel sums agree to 7e-5 on these z (roughness >= 0.5: 6.9e-5 and 7.5e-5); rows with roughness <= 0.3 are left out of
the accuracy bar: there the texel sum itself is only good to 1.5e-3."""
import os

import numpy as np
import pytest

import light_ref as lr
import render_ref as rr
from conftest import rel_l2

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sun():
    return np.load(os.path.join(GOLD, "render_light_sun.npz"))


def random_env(EH, EW, seed, hot=()):
    """random-valued texels (no CDF boundary lands on a dyadic sample) with hot texels (i, j, scale)"""
    env = np.random.default_rng(seed).uniform(0.2, 1.5, size=(EH, EW, 3))
    for i, j, s in hot:
        env[i, j] *= s
    return env


def test_hammersley_and_the_linear_inverse():
    u1, u2 = lr.hammersley(64)
    assert np.array_equal(np.sort(u2), u1) and u2[1] == 0.5 + 0.5 / 64 and u2[2] == 0.25 + 0.5 / 64 and u2[3] == 0.75 + 0.5 / 64
    assert int(lr.bitreverse32(1)) == 1 << 31 and int(lr.bitreverse32(0x80000001)) == 0x80000001
    # cdf(x) = (a x + (b - a) x^2 / 2) / ((a + b) / 2)
    g = np.random.default_rng(0)
    a, b, u = g.uniform(0, 2, 1000), g.uniform(0, 2, 1000), g.uniform(0, 1, 1000)
    a[:50], b[50:100] = 0.0, 0.0
    x = lr.lininv(u, a, b)
    np.testing.assert_allclose((a * x + 0.5 * (b - a) * x * x) / (0.5 * (a + b)), u, rtol=0, atol=1e-12)
    assert np.array_equal(lr.lininv(u, np.zeros(1000), np.zeros(1000)), u)


def test_the_density_integrates_to_one():
    """p_L sin(theta) is bilinear in (theta, psi) inside a cell, so a midpoint rule on a grid that refines the cells integrates it exactly"""
    env = random_env(8, 16, 1, hot=[(2, 5, 400.0), (0, 11, 50.0)])
    env[4, 3] = -1.0  # a negative texel: its luminance is clamped at 0
    den = lr.Density(env)
    d, dw = rr.env_dirs(8 * 8, 16 * 8)
    assert abs(float((lr.light_pdf(den, d) * dw).sum()) - 1.0) <= 1e-9
    assert abs(den.cdf[-1] - den.mass.sum()) <= 1e-12 * den.tot and den.mass.shape == (9,) and den.mean4.shape == (9, 16)
    # the polar rows are half cells of one texel row
    assert den.hi[0] - den.lo[0] == pytest.approx(np.pi / 16) and den.i0[0] == den.i1[0] == 0 and den.i0[8] == den.i1[8] == 7


@pytest.mark.parametrize("M", [64, 1024])
def test_the_table_carries_the_pdf_of_its_directions(M):
    env = random_env(8, 16, 2, hot=[(3, 9, 1000.0), (7, 0, 30.0)])
    den = lr.Density(env)
    d, L, pdf = lr.light_table(den, M)
    np.testing.assert_allclose(np.linalg.norm(d, axis=-1), 1.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(lr.light_pdf(den, d), pdf, rtol=1e-12, atol=0)
    np.testing.assert_allclose(rr.env_lookup(env, d), L, rtol=1e-9, atol=1e-12)
    # the hot texel's four cells hold most of the mass, and so most of the samples
    near = np.arccos(np.clip(d @ rr.env_dirs(8, 16)[0][3, 9], -1, 1)) < 1.5 * np.pi / 8
    assert near.mean() > 0.5


def test_accuracy_on_the_sun_scene(sun):
    env, R, S = sun["env"], int(sun["R"]), int(sun["S"])
    for k, z in enumerate(sun["z"]):
        assert z[4] >= 0.5
        ref = rr.render_texel_sum(z, env, R, S, supersample=4)
        np.testing.assert_allclose(ref, sun["texel4"][k], rtol=1e-12, atol=0)  # the stored reference is this one
        # "agree to 7e-5": a one-figure statement of the reference's own error (6.9e-5 and 7.5e-5 on the two z), held as one
        assert rel_l2(ref, sun["texel8"][k]) < 7.5e-5
        plain = rr.render_quadrature(z, env, R, 32, S)
        lit = lr.render_mis(z, env, R, 32, S, 1024)
        print(f"z {z.tolist()}: plain {rel_l2(plain, ref):.3e}  M = 1024 {rel_l2(lit, ref):.3e}")
        assert rel_l2(lit, ref) <= 2e-3
        assert rel_l2(plain, ref) > 5e-2


def test_without_light_samples_or_without_light_it_is_the_quadrature(sun):
    z = sun["z"][0]
    env = random_env(8, 16, 3)
    plain = rr.render_quadrature(z, env, 4, 8, 2)
    assert rel_l2(lr.render_mis(z, env, 4, 8, 2, 0), plain) <= 1e-14
    black = np.zeros((8, 16, 3))
    assert np.array_equal(lr.render_mis(z, black, 4, 8, 2, 64), np.zeros((3, 4, 4)))
    dark = -env  # all non-positive: no light technique, the plain (negative) render
    assert rel_l2(lr.render_mis(z, dark, 4, 8, 2, 64), rr.render_quadrature(z, dark, 4, 8, 2)) <= 1e-14


def test_a_view_turns_the_environment(sun):
    """a view turned about +y by whole texel columns sees the rolled map: the two renders use different sample tables (the conditional CDF
    starts at another column) and agree as two estimates of one integral do"""
    env = random_env(16, 32, 4, hot=[(5, 20, 3000.0)])
    z, k = sun["z"][0], 5
    a = 2 * np.pi * k / 32
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    turned = lr.render_mis(z, env, 6, 16, 2, 1024, rot=rot)
    err = [rel_l2(turned, lr.render_mis(z, np.roll(env, s, axis=1), 6, 16, 2, 1024)) for s in (k, -k)]
    # (each M = 1024 estimate is held to 2e-3 of the integral; a turn the wrong way moves the light across the film)
    assert err[0] <= 4e-3 and err[1] > 0.1, err


def test_the_interfaces_carry_light_samples():
    import inspect

    from drmnet_amd import _lib, validate as V
    from drmnet_amd.render import RefMapRenderer, render

    assert inspect.signature(render).parameters["light_samples"].default == 0
    assert RefMapRenderer(16).light_samples == 0 and RefMapRenderer(16, light_samples=256).light_samples == 256
    for bad in (100, 32, 1 << 17, -64):
        with pytest.raises(ValueError):
            RefMapRenderer(16, light_samples=bad)
    assert "light_samples" in {n for n, _ in _lib.Shading._fields_} and "drm_render_refmap" in _lib.SYMBOLS and "drm_render_light_workspace_bytes" in _lib.SYMBOLS
    plain, lit = V.make_parser().description, V.make_parser(1024).description
    assert V.QUADRATURE_NOTE in plain and V.make_parser(0).description == plain
    assert V.QUADRATURE_NOTE not in lit and "M = 1024" in lit
    assert V.make_parser().parse_args(["--base", "x.yaml"]).light_samples == 0
    assert V.make_parser().parse_args(["--base", "x.yaml", "--light_samples", "512"]).light_samples == 512

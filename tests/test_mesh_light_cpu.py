"""Light sampling on mesh object images without a GPU: the float64 restatement tests/mesh_light_ref.py (the composition of light_ref,
shadow_ref and render_ref.lobes that drm_render_mesh with light samples is held to), the interfaces that carry `light_samples`, and the entry's argument
checks that return before anything touches a GPU.

Convergence.  The sun scene of tests/golden/mesh_light_sun.npz (tools/make_golden_mesh_light.py): shadow_ref.two_spheres() from +z on a
12 x 12 film, S = 1, Q = 32, the ROUGH row, under smooth_env(32, 64) with texel [11, 19] = (3e4, 2.5e4, 2e4); 34 lit film samples.  The truth
is mesh_light_ref.texel_sum at supersample 4, every direction traced with the occlusion rule; shadows move it by 37.0 % rel-L2.  On the film
rows 3 .. 5, where the ball's shadow of the sun falls, it agrees with supersample 8 to 1.79e-3 of those rows, which is 1.51e-3 of the whole
film's norm (the grid blurs shadow edges; without shadows the two texel sums agree to 7e-5, tests/test_render_light_cpu.py).
Figures, rel-L2 against that truth over the film:
    plain quadrature Q = 32, shadowed            3.30e-1   (unshadowed against the unshadowed truth: 3.11e-1)
    light samples M = 1024, traced               2.40e-3   (unshadowed: 1.98e-3)
The bars: the plain error is >= 5e-2, the lit one <= a tenth of it and <= LIT_BAR = 4.8e-3, twice what this restatement gives."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_light_ref as mlr
import mesh_ref as mr
import shadow_ref as sr
from conftest import ROOT, rel_l2
from test_render_light_cpu import random_env
from test_shadow_cpu import ROUGH, flat_icosphere

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METAL = [1.0, 0.9, 0.6, 0.3, 0.3, 1.0]
LIT_BAR = 4.8e-3
SCENE = sr.two_spheres()
ENV = random_env(8, 16, 31, [(2, 5, 2e3)])


# ---------------------------------------------------------------------------------------------- the restatement's own checks
@pytest.mark.parametrize("shadows", [False, True])
def test_without_light_samples_or_without_light_it_is_shadow_ref(shadows):
    Rot = mr.look_at((0.6, 0.3, 1.0))
    for z in (ROUGH, METAL):
        want = sr.render(*SCENE, z, ENV, Rot, 8, 8, 2, 4, shadows=shadows)
        got = mlr.render(*SCENE, z, ENV, Rot, 8, 8, 2, 4, 0, shadows=shadows)
        assert np.array_equal(got["image"], want["image"]) and np.array_equal(got["slack"], want["slack"]) and want["image"].max() > 0.1
        assert np.array_equal(got["unsafe_pixel"], want["unsafe_pixel"])
        # a black map, and one that is all non-positive, have no light technique
        tr = got["trace"]
        assert np.array_equal(mlr.shade(tr, np.zeros_like(ENV), 64, SCENE[0], SCENE[2])["image"], np.zeros((3, 8, 8)))
        assert np.array_equal(mlr.shade(tr, -ENV, 64, SCENE[0], SCENE[2])["image"], sr.shade(tr, -ENV)["image"])
        # with light samples it is another estimate of the same integral
        lit = mlr.shade(tr, ENV, 64, SCENE[0], SCENE[2])
        assert rel_l2(lit["image"], want["image"]) > 1e-3 and lit["light_traced"] > 1000
        assert (lit["light_occluded"] > 0) == shadows and (shadows or not lit["slack"].any())


def test_the_unshadowed_restatement_on_a_sphere_is_the_lit_sphere_render():
    """a mesh point is shaded as the sphere point with the same normal: on the film samples of an icosphere the per-sample radiance is
    light_ref's, normal by normal (light_ref._mis_rows takes any normals)"""
    import light_ref as lr

    p, n, f = mr.icosphere(2)
    Rot = mr.look_at((0.6, 0.3, 1.0))
    tr = mlr.trace(p, n, f, ROUGH, Rot, 6, 6, 2, 8, shadows=False)
    got = mlr.shade(tr, ENV, 64)
    den = lr.Density(ENV)
    normals = tr["normal"][tr["lit"]]
    want = lr._mis_rows(ROUGH, den, normals[None, :, None, :], 8, 64, Rot, lr.light_table(den, 64))[:, 0].T  # [K, 3]
    assert rel_l2(got["image"], mlr.film(tr, want)) <= 1e-12 and got["image"].max() > 0.1


def test_shadowed_is_never_brighter_and_the_ball_shadows_the_body():
    env = random_env(16, 32, 21, [(4, 11, 3e4)])
    tr_s, tr_u = (mlr.trace(*SCENE, ROUGH, None, 12, 12, 2, 4, shadows=s) for s in (True, False))
    dark, lit = mlr.shade(tr_s, env, 256, SCENE[0], SCENE[2]), mlr.shade(tr_u, env, 256)
    assert np.all(dark["image"] <= lit["image"]) and np.all(dark["image"] >= 0) and (dark["image"] < lit["image"]).sum() >= 50
    moved = rel_l2(dark["image"], lit["image"])
    print(f"light rays occluded {dark['light_occluded'] / dark['light_traced']:.3f}, image moved by {moved:.3f}")
    assert dark["light_occluded"] >= 0.01 * dark["light_traced"] and moved > 0.05


def test_a_flat_shaded_convex_mesh_has_no_shadow_beyond_the_slack():
    mesh = flat_icosphere()
    env = random_env(16, 32, 21, [(4, 11, 3e4)])
    for view in (None, (0.6, 0.3, 1.0)):
        Rot = None if view is None else mr.look_at(view)
        dark = mlr.render(*mesh, ROUGH, env, Rot, 12, 12, 2, 4, 256, shadows=True)
        lit = mlr.render(*mesh, ROUGH, env, Rot, 12, 12, 2, 4, 256, shadows=False)
        diff = lit["image"] - dark["image"]
        assert np.all(diff >= 0) and np.all(diff <= dark["slack"] * (1 + 1e-12)) and lit["image"].max() > 0.1 and dark["light_traced"] > 10000


# ---------------------------------------------------------------------------------------------- convergence
def test_traced_light_samples_converge_where_the_quadrature_does_not():
    gold = np.load(os.path.join(GOLD, "mesh_light_sun.npz"))
    env, z, film, S = gold["env"], gold["z"], int(gold["film"]), int(gold["S"])
    p, n, f = SCENE
    tr = mlr.trace(p, n, f, z, None, film, film, S, 32)
    K, D = int(tr["lit"].sum()), 4 * 32 * 4 * 64
    open4 = np.unpackbits(gold["open4"], axis=1)[:, :D].astype(bool)
    assert z.tolist() == ROUGH and open4.shape == (K, D) and K == 34
    # the stored mask: a seeded subset of its rays traced again
    import render_ref as rr

    d = rr.env_dirs(4 * 32, 4 * 64)[0].reshape(-1, 3)
    rng = np.random.default_rng(5)
    k, j = rng.integers(0, K, 4000), rng.integers(0, D, 4000)
    up = np.sum(tr["normal"][tr["lit"]][k] * d[j], axis=1) > 0
    k, j = k[up], j[up]
    again = ~sr.occluded(p, f, tr["origin"][k], d[j], tr["face"][k])
    assert np.array_equal(again, open4[k, j]) and len(k) >= 1500 and 20 <= (~again).sum()
    # the truth, recomputed from the mask, is the stored one; what it is good to
    truth = mlr.film(tr, mlr.texel_sum(tr, env, 4, open_rays=open4)[0])
    np.testing.assert_allclose(truth, gold["truth4"], rtol=1e-12, atol=1e-14)
    rows8 = list(gold["rows8"])
    own_rows, own_film = rel_l2(truth[:, rows8], gold["truth8"]), float(np.linalg.norm(truth[:, rows8] - gold["truth8"]) / np.linalg.norm(truth))
    moved = rel_l2(gold["plain4"], truth)
    print(f"supersample 4 against 8 on the rows {rows8}: {own_rows:.2e} of those rows, {own_film:.2e} of the film; the shadows move the truth by {moved:.3f}")
    assert own_rows <= 1.8e-3 and moved > 0.3
    # the renders
    plain = sr.shade(tr, env)["image"]
    lit = mlr.shade(tr, env, 1024, p, f)
    e_plain, e_lit = rel_l2(plain, truth), rel_l2(lit["image"], truth)
    print(f"shadowed, against the traced texel sum: plain Q = 32 {e_plain:.3e}  M = 1024 {e_lit:.3e}  ({e_plain / e_lit:.0f} x); "
          f"{lit['light_occluded']} of {lit['light_traced']} light rays occluded")
    assert e_plain >= 5e-2
    assert e_lit <= 0.1 * e_plain
    assert e_lit <= LIT_BAR


# ---------------------------------------------------------------------------------------------- interfaces
def test_the_interfaces_carry_light_samples():
    import inspect

    from drmnet_amd import _lib, config, synthesize
    from drmnet_amd.mesh import MeshRenderer, render_mesh

    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    assert "drm_render_mesh(const drm_shading*" in header and "drm_render_mesh" in _lib.SYMBOLS and hasattr(_lib.lib(), "drm_render_mesh")
    assert "int32_t light_samples;" in header and "light_samples" in {n for n, _ in _lib.Shading._fields_}
    assert "light_samples is not offered" not in header and _lib.lib().drm_abi_version() == 4
    assert inspect.signature(render_mesh).parameters["light_samples"].default == 0
    assert MeshRenderer(16).light_samples == 0 and MeshRenderer(16, light_samples=256, shadows=True).light_samples == 256
    for bad in (100, 32, 1 << 17, -64):
        with pytest.raises(ValueError):
            MeshRenderer(16, light_samples=bad)
    # a YAML `params:` reaches the constructor
    r = config.instantiate_from_config({"target": "drmnet_amd.mesh.MeshRenderer", "params": {"image_size": 16, "light_samples": 128, "shadows": True}})
    assert isinstance(r, MeshRenderer) and r.light_samples == 128 and r.shadows
    assert "--light_samples" in inspect.getsource(synthesize.main)
    with pytest.raises(RuntimeError, match="GPU only"):
        render_mesh({k: torch.zeros(3, 3) for k in ("vertex_positions", "vertex_normals", "faces")}, torch.zeros(1, 6), ["a"] * 6, image_size=8,
                    light_samples=64)


def test_argument_errors_return_before_anything_touches_a_gpu():
    """host buffers stand in for device memory: every case returns from the checks, which dereference nothing"""
    import abi_call
    from drmnet_amd import _lib

    lib = _lib.lib()
    p, n, f = mr.icosphere(0)
    pos, nrm, faces = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(n, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    V, F, B, H, W, EH, EW, M = len(pos), len(faces), 1, 4, 4, 8, 16, 64
    z = np.array([ROUGH], dtype=np.float32)
    env = np.ones((B, EH, EW, 3), dtype=np.float32)
    outs = [np.full(s, -7.0, dtype=np.float32) for s in ((B, 3, H, W), (B, 3, H, W), (B, 1, H, W), (B, H, W))]
    need, light_need = int(lib.drm_render_mesh_workspace_bytes(F, B, H, W, 2)), int(lib.drm_render_light_workspace_bytes(B, EH, EW, M))
    assert need > 0 and light_need == (3 * EH + 4) * 8 + 8 + 28 * M
    ws, lws = np.zeros(need // 8 + 2, dtype=np.float64), np.zeros(light_need // 8 + 2, dtype=np.float64)
    ws_ptr = (ws.ctypes.data + 15) & ~15

    def call(light_samples=M, lws_ptr=lws.ctypes.data, lws_bytes=light_need, bvh=None, bvh_bytes=0, ws_bytes=need, env_ptr=env.ctypes.data):
        sh = abi_call.shading(B, z=z.ctypes.data, env=env_ptr, EH=EH, EW=EW, quad=8, light_samples=light_samples, lws=lws_ptr, lws_bytes=lws_bytes)
        # shadows: what the blob and its length say together
        return abi_call.render_mesh(sh, abi_call.mesh_render(pos.ctypes.data, nrm.ctypes.data, faces.ctypes.data, V, F, [o.ctypes.data for o in outs], H, W, 2,
                                                             ws_ptr, ws_bytes, shadows=int(bvh is not None or bvh_bytes != 0), bvh=bvh, bvh_bytes=bvh_bytes))

    INVALID, WORKSPACE = 1, 3
    for want, over in [(INVALID, dict(light_samples=-64)), (INVALID, dict(light_samples=100)), (INVALID, dict(light_samples=32)),
                       (INVALID, dict(light_samples=1 << 17)), (INVALID, dict(lws_bytes=light_need - 8)), (INVALID, dict(lws_ptr=None)),
                       (INVALID, dict(lws_ptr=lws.ctypes.data + 4)), (INVALID, dict(bvh=None, bvh_bytes=64)),  # a length without a blob
                       (INVALID, dict(bvh=ctypes.c_void_p(ws_ptr), bvh_bytes=16)),                             # a blob shorter than its header
                       (INVALID, dict(light_samples=-1, env_ptr=None)), (WORKSPACE, dict(ws_bytes=need - 1))]:
        status = call(**over)
        assert status == want and lib.drm_last_error(), (want, status, over)
        assert all(np.all(o == -7.0) for o in outs)

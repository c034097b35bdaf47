"""One-bounce interreflection without a GPU: the float64 restatement in tests/bounce_ref.py checked against itself and against
tests/shadow_ref.py, the new symbols, and the argument errors of the Python surface and of the two entries (drm_mesh_closest_hit,
drm_render_mesh with bounces = 1) that return before anything touches a GPU.

The contract, restated (include/drmnet_hip.h): a lobe direction w of a hit sample whose ray is occluded reads, instead of the map,
L_b = (pi / K) sum_k V_k L(w_k) E(n_y, w_o, w_k) / cos_k at its closest hit y -- the candidate of shadow_ref's rule least under (t, face index),
t = T / det rounded to float32 -- with K = bounce_quad^2 cosine-weighted directions about the interpolated normal n_y; everything else is the
shadowed render."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import bounce_ref as br
import mesh_ref as mr
import shadow_ref as sr
from conftest import ROOT
from test_shadow_cpu import ROUGH, as_obj, flat_icosphere

METAL = [1.0, 0.9, 0.6, 0.3, 0.3, 1.0]
BLACK = [0.0, 0.0, 0.0, 0.0, 0.5, 0.0]  # base colour 0, specular 0 (eta = 1: no dielectric Fresnel): E is 0 for every pair of directions
H, S, Q, BQ = 10, 2, 6, 3
ENV = np.random.default_rng(0).uniform(0.5, 1.5, (8, 16, 3))
SCENE = sr.two_spheres()


# ---------------------------------------------------------------------------------------------- the closest hit, restated
def test_the_closest_hit_on_hand_made_rays():
    # two parallel unit triangles at z = 1 and z = 2, the lower one twice (faces 0 and 2)
    tri = np.array([(0, 0, 1), (1, 0, 1), (0, 1, 1)], dtype=np.float64)
    p = np.concatenate([tri, tri + (0, 0, 1), tri])
    f = np.arange(9).reshape(3, 3)
    o = np.array([(0.25, 0.5, 0), (0.25, 0.5, 0), (0.25, 0.5, 0), (0.25, 0.5, 1), (0.25, 0.5, 3), (0.6, 0.6, 0), (0.25, 0.5, 0)], dtype=np.float64)
    d = np.array([(0, 0, 2), (0, 0, 2), (0, 0, 2), (0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, -1)], dtype=np.float64)
    ex = np.array([-1, 0, 2, -1, -1, -1, -1])
    face, t, u, v, marg = br.closest(p, f, o, d, ex, marginal=True)
    # the duplicate pair ties at t = 1/2: the lower index; excluded: the other; both behind or on the origin: the upper face; none; none; none
    assert face.tolist() == [0, 2, 0, 1, -1, -1, -1]
    assert t.tolist() == [0.5, 0.5, 0.5, 1.0, 0, 0, 0] and u.tolist() == [0.25, 0.25, 0.25, 0.25, 0, 0, 0] and v.tolist() == [0.5, 0.5, 0.5, 0.5, 0, 0, 0]
    assert marg[0] and marg[3]  # a tie within the guard; an origin on a face
    # a ray is occluded iff it has a closest hit, on a mesh with faces the rule leaves out
    sp, sf, _ = sr.soup(300)
    rng = np.random.default_rng(1)
    oo, dd = rng.uniform(-1, 1, (2000, 3)), rng.normal(size=(2000, 3))
    exx = rng.integers(-1, 300, 2000)
    g, tt, uu, vv = br.closest(sp, sf, oo, dd, exx)
    assert np.array_equal(g >= 0, sr.occluded(sp, sf, oo, dd, exx)) and 0.05 < (g >= 0).mean() < 0.95 and not np.any((g == exx) & (g >= 0))
    hit = g >= 0
    tri_hit = np.asarray(sp)[np.asarray(sf)[g[hit]]]
    y = (1 - uu[hit] - vv[hit])[:, None] * tri_hit[:, 0] + uu[hit][:, None] * tri_hit[:, 1] + vv[hit][:, None] * tri_hit[:, 2]
    assert np.allclose(y, oo[hit] + tt[hit][:, None] * dd[hit], atol=1e-9) and np.all(tt[hit] > 0)


def test_the_frame_is_orthonormal_for_every_normal():
    n = np.random.default_rng(2).normal(size=(500, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = np.concatenate([n, [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0), (0.6, 0, -0.8)]])
    t, bt = br.frame(n)
    for a, b, want in ((t, t, 1), (bt, bt, 1), (t, bt, 0), (t, n, 0), (bt, n, 0)):
        assert np.allclose(np.sum(a * b, axis=1), want, atol=1e-12)
    assert np.allclose(np.cross(t, bt), n, atol=1e-12)


# ---------------------------------------------------------------------------------------------- the render, restated
@pytest.fixture(scope="module")
def scene_rough():
    return br.render(*SCENE, ROUGH, ENV, mr.look_at((0.6, 0.3, 1.0)), H, H, S, Q, bounce_quad=BQ)


def test_without_bounces_it_is_shadow_ref(scene_rough):
    Rot = mr.look_at((0.6, 0.3, 1.0))
    want = sr.render(*SCENE, ROUGH, ENV, Rot, H, H, S, Q)
    got = br.render(*SCENE, ROUGH, ENV, Rot, H, H, S, Q, bounces=0)
    for k in ("image", "slack", "unsafe_pixel"):
        assert np.array_equal(got[k], want[k])
    assert np.array_equal(scene_rough["shadowed"], want["image"]) and want["image"].max() > 0.1


def test_bounced_is_never_darker_and_the_bounce_is_there(scene_rough):
    tr = scene_rough["trace"]
    assert np.all(scene_rough["image"] >= scene_rough["shadowed"]) and np.all(scene_rough["slack"] >= 0)
    move = np.linalg.norm(scene_rough["image"] - scene_rough["shadowed"]) / np.linalg.norm(scene_rough["shadowed"])
    print(f"bounced rays {tr['bounced']} of {tr['traced']}, inner rays {tr['inner_traced']} ({tr['inner_occluded']} occluded), the image moves by {move:.4f}")
    assert tr["bounced"] == tr["occluded"] >= 100 and 0.05 < tr["inner_occluded"] / tr["inner_traced"] < 0.5 and move > 0.01
    # the body's bounced rays end on the ball and the other way round, or on the same sphere past a silhouette: never on the excluded face
    for name in ("spec", "diff"):
        b = tr["bounce_" + name]
        assert not np.any(b["face"] == tr["face"][b["at"][0]])


def test_a_flat_shaded_convex_mesh_has_no_bounce_beyond_the_slack():
    mesh = flat_icosphere()
    Rot = mr.look_at((0.6, 0.3, 1.0))
    out = br.render(*mesh, ROUGH, ENV, Rot, 12, 12, S, 8, bounce_quad=BQ)
    diff = out["image"] - out["shadowed"]
    assert np.all(diff >= 0) and np.all(diff <= out["slack"] * (1 + 1e-12)) and np.all(diff[out["slack"] == 0] == 0)
    assert (out["slack"] == 0).mean() > 0.5 and out["shadowed"].max() > 0.1


def test_a_row_that_reflects_nothing_bounces_nothing(scene_rough):
    """E = 0 for every pair of directions needs base colour 0 AND no Fresnel term: the dielectric with specular 0 (index-matched).  (A metal
    with base colour 0 still reflects its Schlick term (1 - v.h)^5, so its bounce is small but not 0.)"""
    tr = scene_rough["trace"]
    b = tr["bounce_diff"]
    o, w, g = tr["origin"][b["at"][0]], tr["l_diff"][b["at"]] @ np.asarray(tr["Rot"]).T, tr["face"][b["at"][0]]
    black = br.bounce_terms(*SCENE, BLACK, o, w, g, BQ)
    assert np.all(black["coef"] == 0) and not black["open"].any() and black["alive"].mean() > 0.5
    assert np.any(b["coef"] > 0) and np.array_equal(black["face"], b["face"])
    metal = br.bounce_terms(*SCENE, [1.0, 0.0, 0.0, 0.0, 0.3, 1.0], o, w, g, BQ)
    assert metal["coef"].max() > 0
    out = br.render(*SCENE, BLACK, ENV, None, 8, 8, 1, 4, bounce_quad=2)
    assert np.array_equal(out["image"], out["shadowed"]) and out["trace"]["bounced"] > 0


# ---------------------------------------------------------------------------------------------- interfaces
def test_header_and_symbol_list_carry_the_new_entry_points():
    from drmnet_amd import _lib, synthesize
    from drmnet_amd.mesh import MeshRenderer, closest_hit, render_mesh

    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    for name in ("drm_mesh_closest_hit", "drm_render_mesh"):
        assert name + "(" in header and name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert {"bounces", "bounce_quad"} <= {n for n, _ in _lib.MeshRender._fields_} and "int32_t bounces, bounce_quad;" in header
    assert _lib.lib().drm_abi_version() == 4
    sig = inspect.signature(render_mesh).parameters
    assert sig["bounces"].default == 0 and sig["bounce_quad"].default == 4
    assert inspect.signature(closest_hit).parameters["bvh"].default == "auto"
    assert "--bounces" in inspect.getsource(synthesize.main) and "--bounce_quad" in inspect.getsource(synthesize.main)
    r = MeshRenderer(16)
    assert r.bounces == 0 and r.bounce_quad == 4


def test_python_argument_errors_raise_before_anything_touches_a_gpu(tmp_path):
    from drmnet_amd import config, synthesize
    from drmnet_amd.mesh import MeshRenderer, closest_hit, render_mesh

    p, n, f = mr.icosphere(0)
    obj = as_obj(p, f)
    z = torch.zeros(1, 6)
    for kw, why in ((dict(bounces=1), "shadows"), (dict(bounces=2, shadows=True), "0 or 1"), (dict(bounces=-1, shadows=True), "0 or 1"),
                    (dict(bounces=1, shadows=True, light_samples=64), "light_samples"), (dict(bounces=1, shadows=True, bounce_quad=0), "bounce_quad"),
                    (dict(bounces=1, shadows=True, bounce_quad=17), "bounce_quad"), (dict(bounces=1.5, shadows=True), "0 or 1")):
        with pytest.raises(ValueError, match=why):
            render_mesh(obj, z, ["a"] * 6, image_size=8, **kw)
        with pytest.raises(ValueError, match=why):
            MeshRenderer(8, **kw)
    # a valid combination passes the check and stops where the GPU would be needed
    with pytest.raises(RuntimeError, match="GPU only"):
        render_mesh(obj, z, ["a"] * 6, image_size=8, shadows=True, bounces=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        closest_hit(obj, torch.zeros(4, 3), torch.ones(4, 3))
    r = MeshRenderer(8, shadows=True, bounces=1, bounce_quad=6)
    assert (r.bounces, r.bounce_quad, r.shadows) == (1, 6, True)
    r = config.instantiate_from_config({"target": "drmnet_amd.mesh.MeshRenderer", "params": {"image_size": 8, "shadows": True, "bounces": 1, "bounce_quad": 2}})
    assert isinstance(r, MeshRenderer) and (r.bounces, r.bounce_quad) == (1, 2)
    with pytest.raises(ValueError, match="shadows"):
        config.instantiate_from_config({"target": "drmnet_amd.mesh.MeshRenderer", "params": {"image_size": 8, "bounces": 1}})
    base = ["--mesh", str(tmp_path / "none.obj"), "--z", "0", "1", "1", "1", "0.5", "0.5", "--output_dir", str(tmp_path)]
    for extra, why in ((["--bounces", "1"], "shadows"), (["--bounces", "2", "--shadows"], "0 or 1"),
                       (["--bounces", "1", "--shadows", "--light_samples", "64"], "light_samples"),
                       (["--bounces", "1", "--shadows", "--bounce_quad", "32"], "bounce_quad")):
        with pytest.raises(ValueError, match=why):
            synthesize.main(base + extra)
    assert not list(tmp_path.iterdir())


def test_entry_argument_errors_return_before_any_hip_call():
    """host buffers stand in for device memory: every case returns from the checks, which dereference nothing"""
    import abi_call
    from drmnet_amd import _lib

    lib = _lib.lib()
    p, n, f = mr.icosphere(0)
    pos, nrm, faces = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(n, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    V, F, B, HH, W, EH, EW = len(pos), len(faces), 1, 4, 4, 8, 16
    z = np.array([ROUGH], dtype=np.float32)
    env = np.ones((B, EH, EW, 3), dtype=np.float32)
    outs = [np.full(s, -7.0, dtype=np.float32) for s in ((B, 3, HH, W), (B, 3, HH, W), (B, 1, HH, W), (B, HH, W))]
    need = int(lib.drm_render_mesh_workspace_bytes(F, B, HH, W, 2))
    ws = np.zeros(need // 8 + 2, dtype=np.float64)
    ws_ptr = (ws.ctypes.data + 15) & ~15
    INVALID, WORKSPACE = 1, 3

    def render(bounce_quad=4, bvh=None, bvh_bytes=0, ws_bytes=need, quad=8, pos_ptr=pos.ctypes.data, Fn=F):
        sh = abi_call.shading(B, z=z.ctypes.data, env=env.ctypes.data, EH=EH, EW=EW, quad=quad)
        return abi_call.render_mesh(sh, abi_call.mesh_render(pos_ptr, nrm.ctypes.data, faces.ctypes.data, V, Fn, [o.ctypes.data for o in outs], HH, W, 2, ws_ptr,
                                                             ws_bytes, shadows=1, bvh=bvh, bvh_bytes=bvh_bytes, bounces=1, bounce_quad=bounce_quad))

    for want, over in [(INVALID, dict(bounce_quad=0)), (INVALID, dict(bounce_quad=17)), (INVALID, dict(bounce_quad=-4)), (INVALID, dict(quad=0)),
                       (INVALID, dict(pos_ptr=None)), (INVALID, dict(Fn=0)), (INVALID, dict(bvh=None, bvh_bytes=0)),   # shadows are required
                       (INVALID, dict(bvh=None, bvh_bytes=64)), (INVALID, dict(bvh=ctypes.c_void_p(ws_ptr), bvh_bytes=16)),  # shorter than a header
                       (INVALID, dict(bvh=ctypes.c_void_p(ws_ptr + 4), bvh_bytes=4096)),                                  # misaligned
                       (WORKSPACE, dict(ws_bytes=need - 1))]:
        status = render(**over)
        assert status == want and lib.drm_last_error(), (want, status, over)
        assert all(np.all(o == -7.0) for o in outs)

    N = 8
    o, d = np.zeros((N, 3), dtype=np.float32), np.ones((N, 3), dtype=np.float32)
    face, tuv = np.full(N, -7, dtype=np.int32), np.full((N, 3), -7.0, dtype=np.float32)

    def query(Nn=N, Fn=F, Vn=V, o_ptr=o.ctypes.data, face_ptr=face.ctypes.data, tuv_ptr=tuv.ctypes.data, bvh=None):
        return lib.drm_mesh_closest_hit(pos.ctypes.data, faces.ctypes.data, Vn, Fn, bvh, o_ptr, d.ctypes.data, None, face_ptr, tuv_ptr, Nn, None)

    for over in (dict(Nn=-1), dict(Nn=(1 << 31) + 1), dict(Fn=0), dict(Fn=1 << 24), dict(Vn=0), dict(o_ptr=None), dict(face_ptr=None), dict(tuv_ptr=None),
                 dict(bvh=ctypes.c_void_p(ws_ptr + 4))):  # a misaligned blob
        assert query(**over) == INVALID and lib.drm_last_error(), over
        assert np.all(face == -7) and np.all(tuv == -7.0)
    assert query(Nn=0) == 0  # no ray: nothing to do, nothing read

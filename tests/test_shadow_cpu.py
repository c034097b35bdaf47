"""Self-shadowing without a GPU: the host BVH builder (drm_mesh_bvh_build through drmnet_amd.mesh.build_bvh / decode_bvh) and the float64
restatement in tests/shadow_ref.py.

The rule, restated (include/drmnet_hip.h): a ray (o, d) in object space is occluded iff some face g != exclude with its vertex indices in
[0, V) has, with e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1.pv, tv = o - p0, qv = tv x e1, U = tv.pv, V = d.qv, T = e2.qv, s = sign(det):
det != 0 and finite, s U >= 0, s V >= 0, s (U + V) <= |det|, s T > 0."""
import time

import numpy as np
import pytest
import torch

import mesh_ref as mr
import shadow_ref as sr
from conftest import rel_l2

ROUGH = [0.0, 0.8, 0.5, 0.2, 0.5, 0.5]


def as_obj(p, f):
    p = np.asarray(p, dtype=np.float32)
    return {"vertex_positions": torch.from_numpy(p.copy()), "vertex_normals": torch.zeros(p.shape), "faces": torch.tensor(np.asarray(f), dtype=torch.int32)}


def small_meshes():
    rng = np.random.default_rng(3)
    one = (rng.uniform(-1, 1, (3, 3)), np.array([[0, 1, 2]], dtype=np.int32), np.zeros(1, dtype=bool))
    five = (rng.uniform(-1, 1, (15, 3)), np.arange(15, dtype=np.int32).reshape(5, 3), np.zeros(5, dtype=bool))
    return {"single": one, "five": five}


def meshes():
    p, _, f = sr.two_spheres()
    out = {"two_spheres": (p, f, np.zeros(len(f), dtype=bool)), "soup": sr.soup()}
    out.update(small_meshes())
    return out


MESHES = meshes()


def test_header_and_symbol_list_carry_the_shadow_entry_points():
    from drmnet_amd import _lib
    from conftest import ROOT
    import os

    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    for name in ("drm_mesh_bvh_bytes", "drm_mesh_bvh_build", "drm_mesh_occluded", "drm_render_mesh"):
        assert name + "(" in header and name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert {"shadows", "bvh", "bvh_bytes"} <= {n for n, _ in _lib.MeshRender._fields_} and _lib.lib().drm_abi_version() == 4


@pytest.mark.parametrize("name", sorted(MESHES))
def test_builder_invariants(name):
    from drmnet_amd.mesh import build_bvh, decode_bvh

    p, f, left_out = MESHES[name]
    p32 = np.asarray(p, dtype=np.float32)
    blob = build_bvh(as_obj(p, f))
    t = decode_bvh(blob)
    F, nodes = len(f), len(t["skip"])
    assert t["faces"] == F and blob.numel() == 32 + 32 * nodes + 4 * len(t["order"])
    # every kept face in exactly one leaf, every left-out face in none
    leaves = np.nonzero(t["count"] > 0)[0]
    held = np.concatenate([t["order"][t["first"][i]:t["first"][i] + t["count"][i]] for i in leaves]) if len(leaves) else np.zeros(0, dtype=np.int64)
    assert sorted(held.tolist()) == np.nonzero(~left_out)[0].tolist()
    assert len(held) == len(t["order"]) and sorted(t["order"].tolist()) == sorted(held.tolist())
    assert np.all(t["count"] <= 4)
    # every face's vertices inside its leaf box
    for i in leaves:
        for g in t["order"][t["first"][i]:t["first"][i] + t["count"][i]]:
            v = p32[f[g]]
            assert np.all(v >= t["box_min"][i]) and np.all(v <= t["box_max"][i]), (i, g)
    # depth-first layout: an inner node's children are i + 1 and skip[i + 1], their subtrees end at skip[i]; every child box inside its parent's
    assert np.all(t["skip"] > np.arange(nodes)) and np.all(t["skip"] <= nodes)
    assert np.all(t["skip"][leaves] == leaves + 1)
    for i in np.nonzero(t["count"] == 0)[0]:
        a, b = i + 1, t["skip"][i + 1]
        assert b < t["skip"][i] and t["skip"][b] == t["skip"][i]
        for c in (a, b):
            assert np.all(t["box_min"][c] >= t["box_min"][i]) and np.all(t["box_max"][c] <= t["box_max"][i]), (i, c)
    # the miss chain from the root: strictly increasing, ends at node_count
    i, steps = 0, 0
    while i < nodes:
        assert t["skip"][i] > i
        i, steps = t["skip"][i], steps + 1
    assert i == nodes and steps <= max(nodes, 1)
    if nodes:
        assert t["skip"][0] == nodes
    # two builds give identical bytes
    assert torch.equal(blob, build_bvh(as_obj(p, f)))


def test_bvh_bytes_is_enough_and_bad_sizes_are_errors():
    from drmnet_amd import _lib

    lib = _lib.lib()
    for name, (p, f, _) in MESHES.items():
        pos = np.ascontiguousarray(p, dtype=np.float32)
        faces = np.ascontiguousarray(f, dtype=np.int32)
        V, F = len(pos), len(faces)
        need = lib.drm_mesh_bvh_bytes(F)
        assert need == 32 + 36 * F
        guard = 64
        buf = np.full(need + guard, 0xAB, dtype=np.uint8)
        args = (pos.ctypes.data, faces.ctypes.data, V, F, buf.ctypes.data)
        assert lib.drm_mesh_bvh_build(*args, need) == 0, name
        assert np.all(buf[need:] == 0xAB)  # nothing written past the documented size
        full = buf[:need].copy()
        buf[:] = 0xCD
        assert lib.drm_mesh_bvh_build(*args, need) == 0 and np.array_equal(buf[:need], full)  # the same bytes, padding included
        buf[:] = 0xEE
        assert lib.drm_mesh_bvh_build(*args, need - 1) != 0 and np.all(buf == 0xEE)
        assert lib.drm_mesh_bvh_build(pos.ctypes.data, faces.ctypes.data, V, 0, buf.ctypes.data, need) != 0
        assert lib.drm_mesh_bvh_build(pos.ctypes.data, faces.ctypes.data, V, 1 << 24, buf.ctypes.data, need) != 0 and np.all(buf == 0xEE)
    assert lib.drm_mesh_bvh_bytes(0) == 0 and lib.drm_mesh_bvh_bytes(1 << 24) == 0 and lib.drm_mesh_bvh_bytes((1 << 24) - 1) > 0


def test_a_hundred_thousand_faces_build_in_well_under_a_second():
    from drmnet_amd.mesh import build_bvh, decode_bvh

    rng = np.random.default_rng(0)
    F = 100001
    p = (rng.uniform(-0.9, 0.9, (F, 1, 3)) + rng.uniform(-0.01, 0.01, (F, 3, 3))).reshape(-1, 3)
    f = np.arange(3 * F, dtype=np.int32).reshape(-1, 3)
    obj = as_obj(p, f)
    build_bvh(obj)  # (loads the library)
    t0 = time.perf_counter()
    blob = build_bvh(obj)
    dt = time.perf_counter() - t0
    t = decode_bvh(blob)
    print(f"{len(f)} faces: {len(t['skip'])} nodes in {dt * 1e3:.1f} ms")
    assert len(f) > 100000 and len(t["order"]) == len(f) and dt < 0.5


def test_occluded_and_render_mesh_reject_cpu_tensors():
    from drmnet_amd.mesh import occluded, render_mesh

    p, n, f = mr.icosphere(0)
    obj = as_obj(p, f)
    with pytest.raises(RuntimeError, match="GPU only"):
        occluded(obj, torch.zeros(4, 3), torch.ones(4, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        render_mesh(obj, torch.zeros(1, 6), ["a"] * 6, image_size=8, shadows=True)


# ---------------------------------------------------------------------------------------------- the restatement's own checks
def test_the_rule_on_hand_made_rays():
    tri = np.array([(0, 0, 1), (1, 0, 1), (0, 1, 1)], dtype=np.float64)
    f = np.array([[0, 1, 2]])
    o = np.array([(0.25, 0.25, 0), (0.25, 0.25, 2), (0, 0, 0), (0.5, 0.5, 0), (0.6, 0.6, 0), (-1, 0.2, 1), (0.25, 0.25, 1), (0.25, 0.25, 0)], dtype=np.float64)
    d = np.array([(0, 0, 3), (0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 0, 1), (0, 0, 1)], dtype=np.float64)
    ex = np.array([-1, -1, -1, -1, -1, -1, -1, 0])
    # inside; behind the origin; through a vertex; on the hypotenuse; just outside; in the plane; origin on the face; excluded
    assert sr.occluded(tri, f, o, d, ex).tolist() == [True, False, True, True, False, False, False, False]
    assert sr.occluded(tri, np.array([[0, 1, 3]]), o[:1], d[:1]).tolist() == [False]  # an index = V


def test_a_point_under_a_plate_that_covers_its_hemisphere_renders_black():
    # a small upward triangle at the origin under a plate at z = 1/4 spanning [-64, 64]^2: every direction with l.z > 0 meets the plate
    p = np.array([(-0.3, -0.3, 0), (0.3, -0.3, 0), (0, 0.3, 0), (-64, -64, 0.25), (64, -64, 0.25), (64, 64, 0.25), (-64, 64, 0.25)], dtype=np.float64)
    n = np.array([(0, 0, 1)] * 3 + [(0, 0, -1)] * 4, dtype=np.float64)
    f = np.array([(0, 1, 2), (3, 4, 5), (3, 5, 6)], dtype=np.int32)
    # (the plate would hide the triangle from the viewer as well: the film samples are taken from the triangle alone, and their lobe
    # directions are then traced against the triangle and the plate)
    open_all = sr.trace(p[:3], n[:3], f[:1], ROUGH, None, 16, 16, 1, 8, shadows=True)
    assert open_all["occluded"] == 0 and sr.shade(open_all, None)["image"].max() > 0.1
    tr = sr.trace(p[:3], n[:3], f[:1], ROUGH, None, 16, 16, 1, 8, shadows=False)
    for name in ("spec", "diff"):
        hit = sr.occluded(p, f, np.repeat(tr["origin"], 64, axis=0), tr["l_" + name].reshape(-1, 3), np.repeat(tr["face"], 64))
        tr["open_" + name] = ~hit.reshape(-1, 64)
    assert len(tr["face"]) >= 1 and np.all(sr.shade(tr, None)["image"] == 0.0)


@pytest.mark.parametrize("view", [None, (0.6, 0.3, 1.0)])
def test_the_unshadowed_restatement_is_mesh_ref(view):
    p, n, f = sr.two_spheres()
    Rot = None if view is None else mr.look_at(view)
    env = np.random.default_rng(0).uniform(0.5, 1.5, (8, 16, 3))
    for z in (ROUGH, [1.0, 0.9, 0.6, 0.3, 0.3, 1.0]):
        want = mr.render(p, n, f, z, env, Rot, 8, 8, 2, 4)
        got = sr.render(p, n, f, z, env, Rot, 8, 8, 2, 4, shadows=False)
        assert rel_l2(got["image"], want["image"]) <= 1e-12 and want["image"].max() > 0.1
        assert np.array_equal(got["unsafe_pixel"], want["unsafe_pixel"]) and not got["slack"].any()


def flat_icosphere():
    """icosphere(1) with per-face vertices and the face's own normal: a convex mesh whose shading normals are its geometric normals"""
    p, _, f = mr.icosphere(1)
    tri = p[f]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    return tri.reshape(-1, 3), np.repeat(fn, 3, axis=0), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


def test_a_flat_shaded_convex_mesh_occludes_no_ray_that_is_not_marginal():
    p, n, f = flat_icosphere()
    assert np.all(np.sum(n * p, axis=1) > 0)
    tr = sr.trace(p, n, f, ROUGH, mr.look_at((0.6, 0.3, 1.0)), 12, 12, 2, 8)
    for name in ("spec", "diff"):
        assert not (~tr["open_" + name] & ~tr["marginal_" + name]).any()
    assert tr["traced"] > 10000


def test_the_ball_casts_a_shadow_on_the_body():
    p, n, f = sr.two_spheres()
    tr = sr.trace(p, n, f, ROUGH, None, 16, 16, 2, 8)
    body = tr["face"] < 320
    ball_only = sr.occluded(p, f[320:], np.repeat(tr["origin"][body], 64, axis=0), tr["l_diff"][body].reshape(-1, 3)).reshape(-1, 64).mean(axis=1)
    print(f"body samples losing more than 10 % of their diffuse rays to the ball: {(ball_only > 0.1).sum()}, the most {ball_only.max():.2f}")
    assert (ball_only > 0.1).sum() >= 5 and ball_only.max() <= 0.5 + 1e-12

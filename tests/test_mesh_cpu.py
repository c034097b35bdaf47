"""CPU-side checks of the mesh object-image renderer: the ABI additions, the workspace formula, the OBJ reader and the mesh helpers of
drmnet_amd.mesh, the config mapping, and the float64 restatement (tests/mesh_ref.py) on a case small enough to work out by hand."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as mr
from conftest import ROOT


def test_header_and_symbol_list_carry_the_mesh_entry_points():
    from drmnet_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drmnet_hip.h")).read(), flags=re.S)
    for name in ("drm_render_mesh_workspace_bytes", "drm_render_mesh"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)


def test_workspace_bytes_is_the_documented_formula():
    from drmnet_amd import _lib

    ws = _lib.lib().drm_render_mesh_workspace_bytes
    for F, B, H, W, S in ((320, 3, 16, 16, 2), (1, 1, 1, 1, 1), (100000, 2, 12, 20, 4)):
        assert ws(F, B, H, W, S) == 80 * B * F + 16 * B * (H * S) * (W * S)
    assert ws(320, 1, 16, 16, 5) == 0
    assert ws(0, 1, 16, 16, 2) == 0
    assert ws(320, 1, 0, 16, 2) == 0
    assert ws(1 << 24, 1, 16, 16, 2) == 0 and ws(320, 0, 16, 16, 2) == 0 and ws(320, 1, 16, 4097, 2) == 0


def _write(tmp_path, text, name="m.obj"):
    p = tmp_path / name
    p.write_text(text)
    return p


def _check(obj, positions, normals, faces):
    assert obj["vertex_positions"].dtype == torch.float32 and obj["vertex_normals"].dtype == torch.float32 and obj["faces"].dtype == torch.int32
    np.testing.assert_array_equal(obj["faces"].numpy(), np.array(faces, dtype=np.int32))
    np.testing.assert_allclose(obj["vertex_positions"].numpy(), np.array(positions, dtype=np.float32), rtol=0, atol=0)
    np.testing.assert_allclose(obj["vertex_normals"].numpy(), np.array(normals, dtype=np.float32), rtol=0, atol=1e-7)


def test_load_obj_quad_with_normals(tmp_path):
    from drmnet_amd.mesh import load_obj

    obj = load_obj(_write(tmp_path, "# a quad\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1 4//1\n"))
    _check(obj, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 0, 1]] * 4, [[0, 1, 2], [0, 2, 3]])


def test_load_obj_fan_triangulates_a_pentagon_and_reads_every_corner_form(tmp_path):
    from drmnet_amd.mesh import load_obj

    text = "v 0 0 0\nv 2 0 0\nv 3 1 0\nv 1 2 0\nv -1 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1 4/1/1 5/1/1\n"
    obj = load_obj(_write(tmp_path, text))
    _check(obj, [[0, 0, 0], [2, 0, 0], [3, 1, 0], [1, 2, 0], [-1, 1, 0]], [[0, 0, 1]] * 5, [[0, 1, 2], [0, 2, 3], [0, 3, 4]])
    # a/b corners carry no normal: the file as a whole has none, and the normals are computed
    plain = load_obj(_write(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/1\n", "b.obj"))
    _check(plain, [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1]] * 3, [[0, 1, 2]])


def test_load_obj_negative_indices(tmp_path):
    from drmnet_amd.mesh import load_obj

    # -1 is the last element read so far: the second face sees the fourth vertex and the second normal
    text = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf -3//-1 -2//-1 -1//-1\nv 0 0 1\nvn 1 0 0\nf -4//-1 -1//-1 -2//-1\n"
    obj = load_obj(_write(tmp_path, text))
    _check(obj, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1], [0, 1, 0]], [[0, 0, 1]] * 3 + [[1, 0, 0]] * 3, [[0, 1, 2], [3, 4, 5]])


def test_load_obj_without_normals_computes_area_weighted_ones(tmp_path):
    from drmnet_amd.mesh import load_obj

    # vertex 0 is shared by a face of area 1/2 in the z = 0 plane (normal +z, cross product (0, 0, 1)) and a face of area 1 in the
    # x = 0 plane (normal +x, cross product (2, 0, 0)): its normal is (2, 0, 1) / sqrt 5
    obj = load_obj(_write(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 2 0\nv 0 0 1\nf 1 2 3\nf 1 4 5\n"))
    s5 = np.sqrt(5.0)
    _check(obj, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 2, 0], [0, 0, 1]], [[2 / s5, 0, 1 / s5], [0, 0, 1], [0, 0, 1], [1, 0, 0], [1, 0, 0]],
           [[0, 1, 2], [0, 3, 4]])
    assert "area-weighted" in load_obj.__doc__


def test_load_obj_splits_a_vertex_per_distinct_position_normal_pair(tmp_path):
    from drmnet_amd.mesh import load_obj

    # two faces share positions 1 and 3 but not their normals: v 1 appears with vn 1 and vn 2 and becomes two vertices; v 3 keeps vn 1 in both
    text = "v 0 0 0\nv 1 0 0\nv 0 1 0\nv -1 0 0\nvn 0 0 1\nvn 0 1 0\nf 1//1 2//1 3//1\nf 1//2 3//1 4//2\n"
    obj = load_obj(_write(tmp_path, text))
    _check(obj, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [-1, 0, 0]], [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 0], [0, 1, 0]],
           [[0, 1, 2], [3, 2, 4]])
    with pytest.raises(ValueError):
        load_obj(_write(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2 3\n", "mixed.obj"))


def test_normalize_mesh():
    from drmnet_amd.mesh import normalize_mesh

    obj = {"vertex_positions": torch.tensor([[3.0, 4.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]]), "vertex_normals": torch.eye(3),
           "faces": torch.tensor([[0, 1, 2]], dtype=torch.int32)}
    out = normalize_mesh(obj)
    np.testing.assert_allclose(out["vertex_positions"].numpy(), np.array([[0.54, 0.72, 0], [0, 0, 0.18], [-0.18, 0, 0]], dtype=np.float32), rtol=1e-6)
    assert float(torch.linalg.vector_norm(out["vertex_positions"], dim=-1).max()) == pytest.approx(0.9, rel=1e-6)
    assert out["faces"] is obj["faces"] and torch.equal(obj["vertex_positions"][0], torch.tensor([3.0, 4.0, 0.0]))  # the input is not touched


def test_load_mesh_round_trips_a_pt_dict(tmp_path):
    from drmnet_amd.mesh import load_mesh

    p, n, f = mr.icosphere(0)
    blob = {"vertex_positions": torch.tensor(p, dtype=torch.float32), "vertex_normals": torch.tensor(n, dtype=torch.float32), "faces": torch.tensor(f)}
    torch.save(blob, tmp_path / "Shape__0.pt")
    obj = load_mesh(tmp_path / "Shape__0.pt")
    for k in blob:
        assert torch.equal(obj[k], blob[k]) and obj[k].dtype == blob[k].dtype
    with pytest.raises(ValueError):
        load_mesh(tmp_path / "Shape__0.ply")


def test_config_maps_the_ortho_renderer_to_the_mesh_renderer():
    from drmnet_amd.config import instantiate_from_config
    from drmnet_amd.mesh import MeshRenderer

    node = {"target": "utils.mitsuba3_utils.MitsubaOrthoRenderer",
            "params": {"image_size": [12, 20], "spp": 64, "denoise": "optix", "return_normal": True, "init_view_from": [1.0, 0.5, -0.2],
                       "brdf_param_names": ["metallic", "roughness"]}}
    r = instantiate_from_config(node)
    assert isinstance(r, MeshRenderer) and r.image_size == (12, 20) and r.return_normal and not r.return_depth
    with pytest.raises(ValueError):
        MeshRenderer(16, init_view_from=[0, 1, 0])
    with pytest.raises(ValueError):  # no mesh given and none kept: before anything touches a GPU
        r.rendering(torch.zeros(2), ["metallic", "roughness"])


def test_render_mesh_rejects_cpu_tensors():
    from drmnet_amd.mesh import render_mesh
    from drmnet_amd.render import canonical_rows
    from drmnet_amd.synthesize import NAMES

    row = torch.tensor([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    assert torch.equal(canonical_rows(row, NAMES), row)  # synthesize's --z is the canonical row
    p, n, f = mr.icosphere(0)
    obj = {"vertex_positions": torch.tensor(p), "vertex_normals": torch.tensor(n), "faces": torch.tensor(f)}
    with pytest.raises(RuntimeError):
        render_mesh(obj, torch.zeros(1, 6), NAMES, None, image_size=8)
    with pytest.raises(RuntimeError):
        render_mesh(obj, torch.zeros(1, 6), NAMES, torch.ones(1, 4, 8, 3), image_size=8)


def test_restatement_on_a_screen_filling_triangle():
    """One triangle that covers the whole 4 x 6 film (x in [-1, 1], y in [-2/3, 2/3]): every sample sees face 0.  Its depth is the plane
    z = 0.25 x - 0.5 y through the three vertices; its vertex normals are chosen affine in (x, y) too, n = (0.1 x, 0.1 y, 1), so the
    shading normal of a sample is that vector normalised."""
    pos = np.array([[-4.0, -3.0, 0.5], [4.0, -3.0, 2.5], [0.0, 5.0, -2.5]])
    assert np.allclose(pos[:, 2], 0.25 * pos[:, 0] - 0.5 * pos[:, 1])
    nrm = np.stack([0.1 * pos[:, 0], 0.1 * pos[:, 1], np.ones(3)], axis=-1)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    H, W, S = 4, 6, 2
    out = mr.render(pos, nrm, faces, [0.0, 0.5, 0.5, 0.5, 0.5, 0.5], None, None, H, W, S, 4)
    xs, ys = mr.film_samples(H, W, S)
    assert xs[0] == pytest.approx(-1 + 1 / 12) and ys[0] == pytest.approx((4 / 6) * (1 - 1 / 8)) and ys[-1] == -ys[0]
    X, Y = np.meshgrid(xs, ys)
    assert np.all(out["face"] == 0) and not out["unsafe"].any()
    np.testing.assert_allclose(out["z"], 0.25 * X - 0.5 * Y, atol=1e-14)
    want = np.stack([0.1 * X, 0.1 * Y, np.ones_like(X)], axis=-1)
    want /= np.linalg.norm(want, axis=-1, keepdims=True)
    np.testing.assert_allclose(out["normal"], want, atol=1e-14)
    # barycentrics reproduce the sample position
    w0 = 1 - out["u"] - out["v"]
    np.testing.assert_allclose(w0 * pos[0, 0] + out["u"] * pos[1, 0] + out["v"] * pos[2, 0], X, atol=1e-14)
    # pixel outputs: full coverage, depth = mean of 1.1 - z, normal = mean of the unit normals
    assert np.all(out["alpha"] == 1.0)
    np.testing.assert_allclose(out["depth"][0], (1.1 - (0.25 * X - 0.5 * Y)).reshape(H, S, W, S).mean(axis=(1, 3)), atol=1e-14)
    np.testing.assert_allclose(out["normal_mean"], want.reshape(H, S, W, S, 3).mean(axis=(1, 3)).transpose(2, 0, 1), atol=1e-14)
    # a flat white-lit patch facing the viewer shades as the sphere's centre does
    import render_ref as rr

    flat = mr.render(pos, np.tile([0.0, 0.0, 1.0], (3, 1)), faces, [0.0, 0.5, 0.5, 0.5, 0.5, 0.5], None, None, 2, 2, 1, 4)
    centre = rr._quadrature([0.0, 0.5, 0.5, 0.5, 0.5, 0.5], None, np.array([0.0, 0.0, 1.0]).reshape(1, 1, 1, 3), 4)[:, 0, 0]
    np.testing.assert_allclose(flat["image"], np.broadcast_to(centre[:, None, None], (3, 2, 2)), rtol=1e-14)
    # a view from +x sees the same triangle edge-on through its rotated vertices: Rot^T p
    Rot = mr.look_at([1.0, 0.0, 0.0])
    np.testing.assert_allclose(Rot, np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), atol=1e-15)


def test_icosphere():
    p, n, f = mr.icosphere(2)
    assert f.shape == (320, 3) and p.shape == (162, 3)
    np.testing.assert_allclose(np.linalg.norm(p, axis=1), 0.9, rtol=1e-14)
    np.testing.assert_allclose(p, 0.9 * n)
    # outward-facing, consistently wound
    c = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert np.all(np.sum(c * p[f[:, 0]], axis=1) > 0)

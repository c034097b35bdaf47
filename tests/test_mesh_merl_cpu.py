"""CPU-only checks of mesh object images under measured BRDFs (drm_render_mesh_tables: csrc/mesh_table.hip, drmnet_amd.mesh.render_mesh_measured,
synthesize --merl): the float64 restatement tests/mesh_merl_ref.py against the restatements it is made of, the entry's refusals on host
buffers (in the style of tests/test_abi_structs_cpu.py: every case returns from checks that dereference nothing and leaves the sentinel-filled
outputs alone), and the argument errors of the Python surface.  Nothing here needs a GPU.

The restatement's own checks: without shadows a pixel is the mean over its samples of merl_ref.sample_radiance at the samples' shading
normals (to 1e-12: the same sample sets and weights, reached through shadow_ref.trace instead of render_ref.lobes directly); its sample
sets are those of the proxy row, so the traced, marginal and occluded counts are shadow_ref's for that row; a shadowed image is <= the plain
one everywhere, strictly somewhere, and differs by the weights of the occluded samples alone."""
import ctypes as C
import os

import numpy as np
import pytest

import merl_ref as mr
import mesh_merl_ref as mm
import mesh_ref as mesh_r
import shadow_ref as sr
from drmnet_amd import _lib
from test_abi_structs_cpu import INVALID, WORKSPACE, Scene, wrong_size

FILM, S, Q = 10, 2, 8
ALPHA = 0.45
I, J, K = np.meshgrid(np.arange(90.0), np.arange(90.0), np.arange(180.0), indexing="ij")


def smooth_table():
    """a smooth isotropic table (a broad lobe in theta_h, a rising term in theta_d, an azimuthal term of period 180 that vanishes at
    theta_h = 0 and theta_d = 0) with its last theta_d rows marked unmeasured, so the dropped-corner rule is in play"""
    base = 0.25 + 0.6 * np.exp(-(I / 35.0) ** 2) + 0.15 * (J / 90.0) ** 2 + 0.1 * (I / 90.0) * (J / 90.0) * np.cos(2 * np.pi * K / 180.0)
    t = np.stack([base, 0.8 * base + 0.05, 0.6 * base + 0.02 * (J / 90.0)])
    t[:, :, 88:, :] = -1.0
    return t


TABLE = smooth_table()
SCENE = sr.two_spheres()
ENV = np.random.default_rng(3).uniform(0.5, 1.5, (8, 16, 3))


# ---------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("view", [None, (0.6, 0.3, 1.0)])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_the_unshadowed_restatement_is_the_table_render_at_the_shading_normals(view, mode):
    Rot = None if view is None else mesh_r.look_at(view)
    out = mm.render(*SCENE, TABLE, ALPHA, ENV, Rot, FILM, FILM, S, Q, shadows=False, mode=mode)
    tr = out["trace"]
    assert tr["occluded"] == 0 and tr["marginal"] == 0 and not out["slack"].any()
    rad = np.zeros((FILM * S, FILM * S, 3))
    rad[tr["lit"]] = mr.sample_radiance(TABLE, ALPHA, ENV, tr["normal"][tr["lit"]], Q, Rot, mode)
    want = rad.reshape(FILM, S, FILM, S, 3).mean(axis=(1, 3)).transpose(2, 0, 1)
    assert tr["lit"].sum() >= 80 and want.max() > 0.3
    np.testing.assert_allclose(out["image"], want, rtol=1e-12, atol=1e-14)


def test_the_sample_sets_and_masks_are_those_of_the_proxy_row():
    tr = mm.trace(*SCENE, TABLE, ALPHA, None, FILM, FILM, S, Q)
    ref = sr.trace(*SCENE, mm.proxy_row(ALPHA), None, FILM, FILM, S, Q)
    for key in ("l_spec", "l_diff", "open_spec", "open_diff", "marginal_spec", "marginal_diff", "traced_spec", "face", "origin"):
        assert np.array_equal(tr[key], ref[key]), key
    assert (tr["traced"], tr["marginal"], tr["occluded"]) == (ref["traced"], ref["marginal"], ref["occluded"])
    assert tr["occluded"] >= 0.01 * tr["traced"] and tr["traced"] >= 10000
    # a weight is 0 exactly where the sample is not used: a GGX sample outside its branch; every cosine sample is used
    assert tr["w_spec"].shape == tr["l_spec"].shape and not tr["w_spec"][~tr["traced_spec"]].any()
    assert (tr["w_spec"][tr["traced_spec"]] > 0).all() and (tr["w_diff"] > 0).all()


def test_the_shadowed_restatement_only_darkens_by_its_occluded_samples():
    plain = mm.render(*SCENE, TABLE, ALPHA, ENV, None, FILM, FILM, S, Q, shadows=False)
    dark = mm.render(*SCENE, TABLE, ALPHA, ENV, None, FILM, FILM, S, Q, shadows=True)
    assert np.all(dark["image"] <= plain["image"]) and np.all(dark["image"] >= 0) and (dark["image"] < plain["image"]).sum() >= 30
    rel = np.linalg.norm(dark["image"] - plain["image"]) / np.linalg.norm(plain["image"])
    print(f"float64 shadowed against plain under the table: rel-L2 {rel:.4f}")
    assert rel > 1e-2
    # the weights do not know about the shadow: only the open masks differ
    for key in ("w_spec", "w_diff", "l_spec", "l_diff"):
        assert np.array_equal(plain["trace"][key], dark["trace"][key])


def test_an_exported_table_restates_the_principled_shadowed_image_to_its_discretisation():
    row = [0.0, 0.7, 0.5, 0.3, 0.5, 0.6]
    table = mr.export(row)
    alpha = mr.proxy_alpha(table)
    got = mm.render(*SCENE, table, alpha, ENV, None, FILM, FILM, S, Q)["image"]
    want = sr.render(*SCENE, row, ENV, None, FILM, FILM, S, Q)["image"]
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"exported dielectric table against its principled row, shadowed, Q = {Q}: rel-L2 {rel:.4f} (proxy alpha {alpha:.3f})")
    assert 1e-4 < rel <= 5e-2


# ---------------------------------------------------------------------------------------------- 2. the entry's refusals, on host buffers
@pytest.fixture(scope="module")
def scene():
    return Scene()


def call(scene, sh, m):
    return _lib.lib().drm_render_mesh_tables(sh, m, None), scene.mesh_outs


def refused(result, word=None, want=INVALID):
    status, outs = result
    message = (_lib.lib().drm_last_error() or b"").decode()
    assert status == want and message and (word is None or word in message), (status, message)
    assert all(np.all(o == -7.0) for o in outs)
    return message


def test_header_symbol_list_and_build_carry_the_entry():
    from conftest import ROOT
    from drmnet_amd import build

    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    L = _lib.lib()
    assert "drm_render_mesh_tables(" in header and "drm_render_mesh_tables" in _lib.SYMBOLS and hasattr(L, "drm_render_mesh_tables")
    assert L.drm_render_mesh_tables.argtypes is not None and L.drm_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert "tables are DRM_ERR_INVALID" in header  # (drm_render_mesh still says so, and points here)
    assert "mesh_table.hip" in build.SOURCES and {"mesh_shade.h", "brdf_table.h"} <= set(build.HEADERS)


def test_structs_are_checked_by_size_first(scene):
    blob = dict(shadows=1, bvh=scene.bvh.ctypes.data, bvh_bytes=16)  # (would fail on its blob: the size checks come first)
    message = refused(call(scene, wrong_size(scene.shading(measured=True)), scene.mesh(**blob)), "drm_shading")
    assert str(C.sizeof(_lib.Shading)) in message and str(C.sizeof(_lib.Shading) + 4) in message
    message = refused(call(scene, scene.shading(measured=True), wrong_size(scene.mesh(**blob))), "drm_mesh_render")
    assert str(C.sizeof(_lib.MeshRender)) in message and str(C.sizeof(_lib.MeshRender) + 4) in message
    assert "struct_bytes" not in refused(call(scene, _lib.sized(_lib.Shading), _lib.sized(_lib.MeshRender)))
    assert _lib.lib().drm_render_mesh_tables(None, scene.mesh(), None) == INVALID
    assert _lib.lib().drm_render_mesh_tables(scene.shading(measured=True), None, None) == INVALID


def test_what_is_not_built_under_a_table_is_refused_without_touching_memory(scene):
    tables = dict(tables=(scene.tables.ctypes.data + 15) & ~15, NT=1, alpha=scene.lws.ctypes.data)
    blob = dict(shadows=1, bvh=scene.bvh.ctypes.data, bvh_bytes=16)
    # the material: principled rows belong to drm_render_mesh; both, or none, is no material at all
    refused(call(scene, scene.shading(), scene.mesh()), "tables")
    refused(call(scene, scene.shading(**tables), scene.mesh()), "material")
    refused(call(scene, scene.shading(z=None), scene.mesh()), "material")
    # light samples under a map (a white environment has none: that call would go on to check_tables, which reads device memory)
    refused(call(scene, scene.shading(measured=True, lit=True), scene.mesh()), "light")
    # bounces, whatever goes with them
    for over in (dict(bounces=1, bounce_quad=4, **blob), dict(bounces=1, bounce_quad=4), dict(bounces=2, bounce_quad=4, **blob), dict(bounces=-1)):
        refused(call(scene, scene.shading(measured=True), scene.mesh(**over)), "bounces")
    # the quadrature and the limits
    refused(call(scene, scene.shading(measured=True, quad=0), scene.mesh()), "quad")
    refused(call(scene, scene.shading(measured=True, quad=1025), scene.mesh()), "quad")
    for field, value in (("subpixel", 5), ("subpixel", 0), ("H", 0), ("W", 4097), ("F", 0), ("F", 1 << 24), ("V", 0)):
        m = scene.mesh()
        setattr(m, field, value)
        refused(call(scene, scene.shading(measured=True), m))
    big = scene.shading(measured=True)
    big.B = 65536
    refused(call(scene, big, scene.mesh()))
    for field in ("vertex_positions", "vertex_normals", "faces", "image"):
        m = scene.mesh()
        setattr(m, field, None)
        refused(call(scene, scene.shading(measured=True), m), "null")


def test_workspace_and_blob_are_checked_before_device_memory_is_read(scene):
    sh = scene.shading(measured=True)
    for over in (dict(workspace=None), dict(workspace=scene.ws_ptr + 8), dict(workspace_bytes=scene.need - 1), dict(workspace_bytes=0)):
        m = scene.mesh()
        for k, v in over.items():
            setattr(m, k, v)
        assert str(scene.need) in refused(call(scene, sh, m), "workspace", want=WORKSPACE)
    # shadows: a missing, misaligned or short blob (its header and the tables are the only things read from the device, after all this)
    refused(call(scene, sh, scene.mesh(shadows=1, bvh=None, bvh_bytes=64)), "bvh")
    refused(call(scene, sh, scene.mesh(shadows=1, bvh=scene.bvh.ctypes.data + 4, bvh_bytes=60)), "bvh")
    refused(call(scene, sh, scene.mesh(shadows=1, bvh=scene.bvh.ctypes.data, bvh_bytes=16)), "bvh")
    # the workspace comes first, with its own code
    m = scene.mesh(shadows=1, bvh=None)
    m.workspace_bytes = 0
    refused(call(scene, sh, m), "workspace", want=WORKSPACE)


# ---------------------------------------------------------------------------------------------- 3. the Python surface
def test_synthesize_takes_exactly_one_material_and_names_what_is_not_built(tmp_path, capsys):
    from drmnet_amd import synthesize

    base = ["--mesh", str(tmp_path / "none.obj"), "--output_dir", str(tmp_path / "out")]
    z = ["--z", "0", "0.8", "0.5", "0.2", "0.5", "0.5"]
    merl = ["--merl", str(tmp_path / "none.binary")]
    for extra, words in ((z + merl, ("exactly one", "--merl")), ([], ("exactly one", "--z")),
                         (merl + ["--light_samples", "64"], ("not built", "--light_samples")),
                         (merl + ["--shadows", "--bounces", "1"], ("not built", "--bounces")),
                         (merl + ["--merl_lookup", "cubic"], ("--merl_lookup",))):
        with pytest.raises(SystemExit) as e:
            synthesize.main(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (extra, err)
    assert not (tmp_path / "out").exists()


def test_render_mesh_measured_refuses_bad_arguments_before_the_gpu():
    import torch

    from drmnet_amd.merl import MeasuredBSDF
    from drmnet_amd.mesh import render_mesh_measured

    p, n, f = mesh_r.icosphere(0)
    obj = {"vertex_positions": torch.tensor(p, dtype=torch.float32), "vertex_normals": torch.tensor(n, dtype=torch.float32),
           "faces": torch.tensor(f, dtype=torch.int32)}
    bsdf = MeasuredBSDF(np.full((3, 90, 90, 180), 0.2, dtype=np.float32), alpha=1.0)
    env = torch.ones(2, 4, 8, 3)
    with pytest.raises(ValueError, match="lookup"):
        render_mesh_measured(obj, bsdf, None, image_size=8, lookup="cubic")
    with pytest.raises(RuntimeError, match="GPU only"):
        render_mesh_measured(obj, bsdf, env, image_size=8)
    with pytest.raises(ValueError, match="envmaps"):
        render_mesh_measured(obj, bsdf, torch.ones(4, 8, 3), image_size=8)
    with pytest.raises(ValueError, match="quad"):
        render_mesh_measured(obj, bsdf, None, image_size=8, quad=0)
    with pytest.raises(ValueError, match="view_from"):
        render_mesh_measured(obj, [bsdf, bsdf], None, image_size=8, view_from=[(0.0, 0.0, 1.0)])
    with pytest.raises(ValueError, match="B = 0"):
        render_mesh_measured(obj, [], None, image_size=8)

"""The mesh object-image renderer on the GPU (drm_render_mesh: csrc/mesh.hip for visibility, mesh_shade_kernel in csrc/render.hip, through
drmnet_amd.mesh and drmnet_amd.synthesize) against the float64 restatement in tests/mesh_ref.py.

Tolerances.  Visibility is compared only where float32 cannot see another face than float64: either every edge function is exact in float32
(vertex coordinates multiples of 1/64 on a film whose sample positions are multiples of 1/32: the exact cases, compared everywhere), or the
sample is not `unsafe` in the restatement's sense (1e-4 view units from every edge and depth tie, 100 times the float32 rounding of a rotated
vertex).  On those pixels normal, depth and alpha are float32 evaluations of O(1) quantities: 1e-5 absolute.  The image is held to the
1e-5 rel-L2 bar the plain sphere render holds against its own restatement (test_gpu_render.py)."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as mr
import render_ref as rr
from conftest import rel_l2
from test_render_cpu import NAMES6

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Q = 8
ROUGH, METAL, DIFFUSE = [0.0, 0.8, 0.5, 0.2, 0.5, 0.5], [1.0, 0.9, 0.6, 0.3, 0.3, 1.0], [0.0, 0.8, 0.5, 0.2, 0.6, 0.0]
# (H, W, view_from) of the rotated-view cases; the restatement alone puts 0 %, 0.6 % and 0.4 % of their film samples in the unsafe set
VIEWS = [(16, 16, (0.6, 0.3, 1.0)), (12, 20, (-1.0, 0.2, 0.4)), (16, 16, (0.0, 0.0, 1.1))]
UNSAFE_CAP = 0.02
# the closed loop (test 6): rel-L2 over the observed texels between the 16 x 16 reflectance map gathered from the synthesized object image and
# the reflectance map rendered at 16 x 16, computed in float64 on the CPU (mesh_ref + render_ref + oracle.refmap.refmap_mask_make) for
# icosphere(3), 64 x 64, S = 2, Q = 16, ROUGH, smooth_env(16, 32), view (0.6, 0.3, 1.0).  It is discretisation error -- a point sample near
# the texel centre against a box-filtered texel, and interpolated normals -- that the float64 pipeline shares.  Perturbing the float64
# normals by 1e-6 (three draws) changes none of the 256 texels of the float64 mask, so the 2 % allowed between the masks is not used up there.
D64 = 0.0674183


def smooth_env(EH, EW, seed=0):
    """the smooth environment of test_gpu_render.py"""
    d, _ = rr.env_dirs(EH, EW)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k = 0.1 * seed
    return np.stack([1 + 0.5 * x + 0.3 * y * y + k, 0.8 + 0.4 * z - 0.2 * x * y, 1.2 + 0.6 * y + 0.1 * x + k * z], -1)


ENV = smooth_env(16, 32)


def as_obj(p, n, f):
    return {"vertex_positions": torch.tensor(np.asarray(p), dtype=torch.float32), "vertex_normals": torch.tensor(np.asarray(n), dtype=torch.float32),
            "faces": torch.tensor(np.asarray(f), dtype=torch.int32)}


def rotation(view_from):
    """the float32 matrix the kernel is given, as float64: the restatement and the kernel see the same view"""
    from drmnet_amd.render import view_rotation

    return view_rotation(torch.tensor([view_from], dtype=torch.float32))[0].double().numpy()


def gpu_render(mesh, z_rows, envs, views, H, W, S, quad=Q):
    from drmnet_amd.mesh import render_mesh

    z = torch.tensor(z_rows, dtype=torch.float32, device=DEV)
    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    view = None if views is None else torch.tensor(views, dtype=torch.float32)
    return [t.cpu().numpy().astype(np.float64) for t in render_mesh(as_obj(*mesh), z, NAMES6, env, image_size=(H, W), view_from=view, quad=quad, subpixel=S)]


# ---------------------------------------------------------------------------------------------- 1. exact visibility
def flat_faces(tris, normals=None):
    """triangles [F][3][3] in units of 1/64 -> a mesh whose every face has its own three vertices and its own flat normal (so the normal output
    names the face): normal k = normalize(0.3 cos k, 0.3 sin k, 1) unless given"""
    tris = np.asarray(tris, dtype=np.float64) / 64.0
    F = len(tris)
    if normals is None:
        k = np.arange(F, dtype=np.float64)
        normals = np.stack([0.3 * np.cos(k), 0.3 * np.sin(k), np.ones(F)], axis=-1)
    normals = np.asarray(normals, dtype=np.float64)
    normals = normals / np.linalg.norm(normals, axis=-1, keepdims=True)
    return tris.reshape(-1, 3), np.repeat(normals, 3, axis=0), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


EXACT = {
    # two triangles crossing each other in depth
    "two_triangles": flat_faces([[(-48, -40, -5), (40, -24, 24), (-8, 44, 8)], [(-36, 36, 20), (44, 28, -12), (4, -46, 4)]]),
    # two faces in the plane z = 1/4 sharing the edge x = 1/16, which runs through the sample centres of column 8 at 16 x 16, S = 1: both cover
    # those samples at the same depth and the lower index is seen; behind them a larger face that must not show through
    "shared_edge": flat_faces([[(4, -40, 16), (40, 0, 16), (4, 40, 16)], [(4, -40, 16), (4, 40, 16), (-40, 0, 16)],
                               [(-60, -60, 0), (60, -60, 0), (0, 60, 0)]]),
    # coplanar duplicates: faces 1 and 2 are the same triangle (the same arithmetic, so the same depth to the bit) behind a part of face 0
    "duplicates": flat_faces([[(-20, -50, 30), (50, -50, 30), (50, 20, 30)], [(-44, -38, 12), (42, -30, -4), (-6, 46, 20)],
                              [(-44, -38, 12), (42, -30, -4), (-6, 46, 20)]]),
    # a tetrahedron, apex toward the viewer, its base (face 3) hidden behind the three sides; no edge of it runs through a sample centre (a
    # side and the base would tie there in exact arithmetic only), which the test checks through the depth gaps
    "tetrahedron": flat_faces([[(3, 5, 40), (-46, -32, -10), (48, -27, -10)], [(3, 5, 40), (48, -27, -10), (2, 51, -10)],
                               [(3, 5, 40), (2, 51, -10), (-46, -32, -10)], [(-46, -32, -10), (2, 51, -10), (48, -27, -10)]]),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_visibility(name):
    p, n, f = EXACT[name]
    z = [ROUGH]
    for S in (1, 2):
        ref = mr.render(p, n, f, ROUGH, None, None, 16, 16, S, Q)
        # the case is exact: wherever two faces cover a sample their depths are equal to the bit (a tie the index rule settles) or far apart
        gap = ref["gap"]
        assert np.all((gap == 0.0) | (gap > 1e-3)), name
        image, normal, depth, alpha = gpu_render((p, n, f), z, None, None, 16, 16, S)
        assert np.array_equal(alpha[0], ref["alpha"]), (name, S)
        if S == 1:
            face_normal = n[::3]
            seen = np.where(alpha[0] > 0, np.argmax(np.einsum("chw,fc->fhw", normal[0], face_normal), axis=0), -1)
            assert np.array_equal(seen, ref["face"]), (name, np.argwhere(seen != ref["face"]))
            assert np.abs(normal[0] - ref["normal_mean"]).max() <= 1e-6
            assert np.abs(depth[0] - ref["depth"]).max() <= 1e-6
    if name == "shared_edge":
        ref = mr.visibility(p, f, None, 16, 16, 1)
        on_edge = ref["gap"][:, 8] == 0.0
        assert on_edge.sum() >= 8 and np.all(ref["face"][on_edge, 8] == 0)  # the tie is there, and the lower index has it
    if name == "duplicates":
        ref = mr.visibility(p, f, None, 16, 16, 1)
        assert (ref["face"] == 1).sum() >= 20 and not (ref["face"] == 2).any() and np.all(ref["gap"][ref["face"] == 1] == 0.0)


# ---------------------------------------------------------------------------------------------- 2 - 4. the icosphere from three views
SPHERE = mr.icosphere(2)
ROWS = [ROUGH, METAL, DIFFUSE]


@functools.lru_cache(maxsize=None)
def sphere_ref(case, row, white=False):
    """the restatement of one (view case, BSDF row), computed once"""
    H, W, view = VIEWS[case]
    return mr.render(*SPHERE, ROWS[row], None if white else ENV, rotation(view), H, W, 2, Q)


@functools.lru_cache(maxsize=None)
def sphere_gpu(case, white=False):
    """the three BSDF rows of a view case in one call"""
    H, W, view = VIEWS[case]
    return gpu_render(SPHERE, ROWS, None if white else [ENV] * 3, [view] * 3, H, W, 2)


@pytest.mark.parametrize("case", range(len(VIEWS)))
def test_rotated_views_match_the_restatement(case):
    ref = sphere_ref(case, 0)
    assert ref["unsafe"].mean() <= UNSAFE_CAP  # (a changed mesh or film cannot silently empty the comparison)
    safe = ~ref["unsafe_pixel"]
    assert safe.mean() >= 0.9 and (ref["alpha"][safe] > 0).sum() >= 100 and ((ref["alpha"] > 0) & (ref["alpha"] < 1) & safe).sum() >= 10
    _, normal, depth, alpha = sphere_gpu(case)
    for b in range(3):  # (visibility does not depend on the BSDF row)
        assert np.abs(alpha[b] - ref["alpha"])[safe].max() <= 1e-5
        assert np.abs(normal[b] - ref["normal_mean"])[:, safe].max() <= 1e-5
        assert np.abs(depth[b] - ref["depth"])[:, safe].max() <= 1e-5


@pytest.mark.parametrize("case", range(len(VIEWS)))
def test_shading_matches_the_restatement(case):
    image = sphere_gpu(case)[0]
    for b in range(3):
        ref = sphere_ref(case, b)
        safe = ~ref["unsafe_pixel"]
        err = rel_l2(image[b][:, safe], ref["image"][:, safe])
        print(f"case {case} row {b}: image rel-L2 on safe pixels {err:.3g}")
        assert err <= 1e-5, (case, b, err)
        assert ref["image"][:, safe].max() > 0.1
    # a white environment (envmap = NULL): the view then only moves the geometry
    white = sphere_gpu(case, True)[0]
    ref = sphere_ref(case, 0, True)
    safe = ~ref["unsafe_pixel"]
    assert rel_l2(white[0][:, safe], ref["image"][:, safe]) <= 1e-5
    assert rel_l2(white[0], image[0]) > 1e-2


def test_mesh_render_of_a_sphere_is_the_sphere_render_and_rows_are_independent():
    # the per-sample normals of the restatement, shaded by the sphere's per-normal sum (render_ref._quadrature), are the mesh image: case 3 above
    # states it per pixel; here directly, for the metal row of the first view, without mesh_ref.render in between
    H, W, view = VIEWS[0]
    Rot = rotation(view)
    vis = mr.visibility(SPHERE[0], SPHERE[2], Rot, H, W, 2)
    n = mr.shading_normals(vis, SPHERE[1], SPHERE[2], Rot)
    rad = mr.sample_radiance(METAL, ENV, n, Q, Rot).reshape(H, 2, W, 2, 3).mean(axis=(1, 3)).transpose(2, 0, 1)
    safe = ~vis["unsafe"].reshape(H, 2, W, 2).any(axis=(1, 3))
    assert rel_l2(sphere_gpu(0)[0][1][:, safe], rad[:, safe]) <= 1e-5
    # B = 3 rows under three views and three maps in one call equal the three single-row calls bit for bit; a repeated call is bit-identical
    views = [v for _, _, v in VIEWS]
    envs = [smooth_env(16, 32, s) for s in range(3)]
    stacked = gpu_render(SPHERE, ROWS, envs, views, 16, 16, 2)
    again = gpu_render(SPHERE, ROWS, envs, views, 16, 16, 2)
    for a, b in zip(stacked, again):
        assert np.array_equal(a, b)
    for r in range(3):
        one = gpu_render(SPHERE, ROWS[r:r + 1], envs[r:r + 1], views[r:r + 1], 16, 16, 2)
        for a, b in zip(stacked, one):
            assert np.array_equal(a[r], b[0]), r
    assert not np.array_equal(stacked[1][0], stacked[1][1])


# ---------------------------------------------------------------------------------------------- 5. degenerate input
def degenerate_mesh():
    """a plate z = 0 over [-1/2, 1/2]^2 whose normals point away from the viewer, a small front-facing triangle above one corner of it, and three
    faces that must be skipped: zero area (a repeated vertex), a vertex index = V, a negative vertex index.  Coordinates in 1/64."""
    p = np.array([(-32, -32, 0), (32, -32, 0), (32, 32, 0), (-32, 32, 0), (-40, -40, 8), (-8, -40, 8), (-40, -8, 8)], dtype=np.float64) / 64.0
    n = np.array([(0, 0, -1)] * 4 + [(0, 0, 1)] * 3, dtype=np.float64)
    f = np.array([(0, 0, 1), (0, 1, 2), (0, 1, 7), (0, 2, 3), (-1, 1, 2), (4, 5, 6), (1, 3, 1)], dtype=np.int32)
    return p, n, f


def test_degenerate_input_matches_the_restatement():
    mesh = degenerate_mesh()
    ref = mr.render(*mesh, ROUGH, ENV, None, 16, 16, 2, Q)
    assert set(np.unique(ref["face"])) == {-1, 1, 3, 5}
    image, normal, depth, alpha = gpu_render(mesh, [ROUGH], [ENV], None, 16, 16, 2)
    assert np.array_equal(alpha[0], ref["alpha"])
    assert np.abs(normal[0] - ref["normal_mean"]).max() <= 1e-6 and np.abs(depth[0] - ref["depth"]).max() <= 1e-6
    plate = np.all(np.isin(ref["face"], (1, 3)).reshape(16, 2, 16, 2), axis=(1, 3))
    assert plate.sum() >= 30 and np.all(image[0][:, plate] == 0.0) and np.abs(normal[0][2][plate] + 1.0).max() <= 1e-6 and np.all(alpha[0][plate] == 1.0)
    lit = image[0].sum(axis=0) > 0
    assert lit.sum() >= 5 and rel_l2(image[0][:, lit], ref["image"][:, lit]) <= 1e-5 and np.array_equal(lit, ref["image"].sum(axis=0) > 0)


def raw_call(mesh, **over):
    """drm_render_mesh through ctypes on sentinel-filled outputs: (status, outputs)"""
    import abi_call
    from drmnet_amd import _lib

    obj = {k: v.to(DEV) for k, v in as_obj(*mesh).items()}
    a = dict(V=obj["vertex_positions"].shape[0], F=obj["faces"].shape[0], B=1, H=8, W=8, EH=16, EW=32, quad=Q, subpixel=2)
    a.update({k: v for k, v in over.items() if k in a})
    need = 80 * 320 + 16 * 16 * 16  # enough for every call made here that is to pass the size check
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    zrow = torch.tensor([ROUGH], dtype=torch.float32, device=DEV)
    env = torch.tensor(ENV, dtype=torch.float32, device=DEV)[None].contiguous()
    outs = [torch.full(s, -7.0, device=DEV) for s in ((1, 3, 8, 8), (1, 3, 8, 8), (1, 1, 8, 8), (1, 8, 8))]
    ptrs = [None if over.get("drop_aovs") and k else o.data_ptr() for k, o in enumerate(outs)]
    base = ws.data_ptr() + (-ws.data_ptr()) % 16
    sh = abi_call.shading(a["B"], z=zrow.data_ptr(), env=env.data_ptr(), EH=a["EH"], EW=a["EW"], quad=a["quad"])
    m = abi_call.mesh_render(obj["vertex_positions"].data_ptr(), obj["vertex_normals"].data_ptr(), obj["faces"].data_ptr(), a["V"], a["F"], ptrs, a["H"],
                             a["W"], a["subpixel"], over.get("ws", base + over.get("ws_offset", 0)), over.get("ws_bytes", need))
    status = abi_call.render_mesh(sh, m, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, [o.cpu().numpy() for o in outs]


def test_bad_arguments_launch_nothing():
    mesh = mr.icosphere(0)
    ok, outs = raw_call(mesh)
    assert ok == 0 and all(not np.any(o == -7.0) for o in outs)
    ok, part = raw_call(mesh, drop_aovs=True)  # normal, depth and alpha may be NULL
    assert ok == 0 and np.array_equal(part[0], outs[0]) and all(np.all(o == -7.0) for o in part[1:])
    F = mesh[2].shape[0]
    exact_bytes = 80 * F + 16 * 16 * 16
    assert raw_call(mesh, ws_bytes=exact_bytes)[0] == 0
    INVALID, WORKSPACE = 1, 3
    for want, over in ((INVALID, dict(subpixel=5)), (INVALID, dict(subpixel=0)), (INVALID, dict(quad=0)), (INVALID, dict(quad=1025)), (INVALID, dict(F=0)),
                       (INVALID, dict(F=1 << 24)), (INVALID, dict(V=0)), (INVALID, dict(H=0)), (INVALID, dict(W=4097)), (INVALID, dict(B=0)),
                       (INVALID, dict(EH=0)), (WORKSPACE, dict(ws_bytes=exact_bytes - 1)), (WORKSPACE, dict(ws=None)), (WORKSPACE, dict(ws_offset=4))):
        status, outs = raw_call(mesh, **over)
        assert status == want, (over, status)
        assert all(np.all(o == -7.0) for o in outs), over


# ---------------------------------------------------------------------------------------------- 6. closed loop through the command-line tool
LOOP = dict(subdiv=3, size=64, S=2, quad=16, res=16, view=(0.6, 0.3, 1.0), thr=np.pi / 16 / 2)


def closed_loop_figure(image, normal, mask, refmap, gather):
    """rel-L2 over the observed texels between the gathered reflectance map and the rendered one; also the texel mask"""
    got, refmask = gather(image[mask], normal[mask])
    refmask = np.asarray(refmask, dtype=bool)
    return rel_l2(np.asarray(got)[refmask], np.asarray(refmap)[refmask]), refmask


def test_closed_loop_through_synthesize(tmp_path):
    from drmnet_amd import file_io, synthesize
    from drmnet_amd.img2refmap import refmap_mask_make
    from oracle import refmap as oref

    p, n, f = mr.icosphere(LOOP["subdiv"])
    torch.save({k: v for k, v in as_obj(p, n, f).items()}, tmp_path / "sphere.pt")
    file_io.save_exr(tmp_path / "env.exr", ENV.astype(np.float32))
    out = tmp_path / "out"
    synthesize.main(["--mesh", str(tmp_path / "sphere.pt"), "--envmap", str(tmp_path / "env.exr"), "--z", *[str(v) for v in ROUGH], "--view_from",
                     *[str(v) for v in LOOP["view"]], "--image_size", str(LOOP["size"]), "--refmap_res", str(LOOP["res"]), "--quad", str(LOOP["quad"]),
                     "--output_dir", str(out)])
    image = file_io.load_exr(out / "image.exr", as_torch=True).to(DEV)
    normal = torch.from_numpy(np.load(out / "normal.npy")).to(DEV)
    mask = file_io.load_png(out / "mask.png", as_torch=True)
    mask = (mask[:, :, 0] if mask.ndim == 3 else mask).to(DEV) > 0.5
    refmap = file_io.load_exr(out / "refmap.exr")
    assert image.shape == (64, 64, 3) and normal.shape == (64, 64, 3) and normal.dtype == torch.float32 and refmap.shape == (16, 16, 3)
    assert torch.equal(mask, torch.linalg.norm(normal, dim=-1) > 0.5) and 0.55 < float(mask.float().mean()) < 0.7

    def gather(c, nrm):
        rm, mk = refmap_mask_make(c, nrm, res=LOOP["res"], angle_threshold=LOOP["thr"])
        return rm.cpu().numpy(), mk.cpu().numpy()

    d_gpu, mask_gpu = closed_loop_figure(image, normal, mask, refmap, gather)
    # the float64 texel mask depends on the normals alone: visibility and interpolation in float64, no shading
    Rot = rotation(LOOP["view"])
    vis = mr.visibility(p, f, Rot, LOOP["size"], LOOP["size"], LOOP["S"])
    n64 = mr.shading_normals(vis, n, f, Rot).reshape(LOOP["size"], LOOP["S"], LOOP["size"], LOOP["S"], 3).mean(axis=(1, 3))
    m64 = np.linalg.norm(n64, axis=-1) > 0.5
    _, mask64 = oref.refmap_mask_make(np.zeros((int(m64.sum()), 3), np.float32), n64[m64], LOOP["res"], LOOP["thr"])
    print(f"closed loop: d_gpu {d_gpu:.6g}, d64 {D64:.6g}, observed texels {int(mask_gpu.sum())}, mask differences {int((mask_gpu != mask64).sum())}")
    assert mask_gpu.sum() >= 150
    assert (mask_gpu != mask64).sum() <= 0.02 * 256
    assert d_gpu <= 1.5 * D64 + 1e-4, (d_gpu, D64)


# ---------------------------------------------------------------------------------------------- 7. MeshRenderer.rendering
def test_mesh_renderer_rendering_keeps_its_scene():
    from drmnet_amd.mesh import MeshRenderer, render_mesh

    obj = as_obj(*SPHERE)
    env = torch.tensor(ENV, dtype=torch.float32)
    z = torch.tensor(ROUGH)
    view = (0.6, 0.3, 1.0)
    direct = render_mesh(obj, z[None].to(DEV), NAMES6, env[None].to(DEV), image_size=(12, 20), view_from=torch.tensor([view]), quad=Q)
    r = MeshRenderer((12, 20), spp=16, denoise="optix", return_normal=True, return_depth=True, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q)
    with pytest.raises(ValueError):
        r.rendering(z, NAMES6, env)
    img, nrm, dep = r.rendering(z, NAMES6, env, obj=obj)
    assert img.shape == (12, 20, 3) and nrm.shape == (12, 20, 3) and dep.shape == (12, 20, 1)
    assert torch.equal(img, direct[0][0].permute(1, 2, 0)) and torch.equal(nrm, direct[1][0].permute(1, 2, 0)) and torch.equal(dep, direct[2][0].permute(1, 2, 0))
    # a second call without obj / envmap reuses the scene's; channel_first
    img2, nrm2, dep2 = r.rendering(z, NAMES6, channel_first=True)
    assert img2.shape == (3, 12, 20) and dep2.shape == (1, 12, 20) and torch.equal(img2, direct[0][0]) and torch.equal(nrm2, direct[1][0])
    # a view given to a call stays with the scene
    moved = r.rendering(z, NAMES6, view_from=torch.tensor([-1.0, 0.2, 0.4]), channel_first=True)[0]
    assert not torch.equal(moved, img2) and torch.equal(r.rendering(z, NAMES6, channel_first=True)[0], moved)
    # new_scene: map, view and mesh hold for that call only
    small = as_obj(*mr.icosphere(1))
    fresh = r.rendering(z, NAMES6, 2 * env, view_from=torch.tensor(view), obj=small, new_scene=True, channel_first=True)[0]
    want = render_mesh(small, z[None].to(DEV), NAMES6, 2 * env[None].to(DEV), image_size=(12, 20), view_from=torch.tensor([view]), quad=Q)[0][0]
    assert torch.equal(fresh, want)
    assert torch.equal(r.rendering(z, NAMES6, channel_first=True)[0], moved)
    with pytest.raises(ValueError):
        r.rendering(z, NAMES6, obj=small, new_scene=True)
    # the image alone when no AOV is asked for
    plain = MeshRenderer(8, brdf_param_names=list(NAMES6), quad=Q)
    only = plain.rendering(z, NAMES6, env, obj=obj)
    assert isinstance(only, torch.Tensor) and only.shape == (8, 8, 3)

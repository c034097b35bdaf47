"""One-bounce interreflection on the GPU (drm_mesh_closest_hit, drm_render_mesh with bounces = 1: csrc/bvh.h, csrc/bvh.hip,
mesh_shade_kernel<VIEW, true, false, true> in csrc/render.hip, through drmnet_amd.mesh and drmnet_amd.synthesize) against the float64 restatement in
tests/bounce_ref.py.

The closest hit, restated (include/drmnet_hip.h): a face is a candidate of a ray iff the any-hit rule accepts it; t = T / det, u = U / det,
v = V / det are correctly rounded fp32 quotients; the hit is the candidate least under (t, face index); none: face -1.  On the exact case of
tests/test_gpu_shadow.py det, U, V and T are exact in float32, so face, t, u and v are compared everywhere, as float32 values.  With and
without the BVH the query must give the same face and the same bits, for every ray.

The image is compared as the shadowed image is: the two-sphere scene on its 16 x 16 film, S = 2, Q = 8, bounce_quad = 4, on the pixels that
are not `unsafe_pixel`, after taking off `slack` (shadow_ref's, plus |w L_b| of the bounced rays whose closest hit is marginal, plus the
marginal inner rays' terms), at the 1e-5 rel-L2 bar of the mesh images.  What keeps the comparison from emptying itself is asserted on the
restatement alone (caps 2 % each).  The restatement gives, over the nine (view, row) cases and the two environments: marginal rays (lobe,
closest-hit and inner) 0.18 % ... 1.50 % of all traced rays (view 0, METAL; the lobe rays alone, also capped: <= 1.58 % of the lobe rays), unsafe samples <= 0.59 %, slack 0.02 % ... 1.72 % of the image sum
(view 0, METAL, white); 1.5 % ... 4.2 % of the lobe rays are occluded and bounce, 18.8 % ... 25.2 % of their inner rays are occluded, and the
bounce moves the float64 image by 2.5 % ... 10.6 % rel-L2 (bar: >= 1 %).  On an MI355X the image meets the restatement at 3.4e-8 ... 7.9e-8
rel-L2 beyond the slack on the safe pixels of the eighteen cases."""
import functools

import numpy as np
import pytest
import torch

import bounce_ref as br
import mesh_ref as mr
import shadow_ref as sr
import test_gpu_shadow as tgs
from conftest import rel_l2
from test_gpu_mesh import ENV, as_obj, rotation
from test_gpu_shadow import CAP, FILM, Q, ROUGH, ROWS, S, SCENE, SOUP, VIEWS, bare
from test_render_cpu import NAMES6

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BQ = 4


def gpu_closest(mesh, o, d, ex, bvh):
    """-> face [N] int32 and (t, u, v) [N, 3] float32, on the host"""
    from drmnet_amd.mesh import closest_hit

    o, d = (torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV) for a in (o, d))
    face, t, u, v = closest_hit(mesh, o, d, None if ex is None else torch.tensor(np.asarray(ex), dtype=torch.int32, device=DEV), bvh=bvh)
    assert face.dtype == torch.int32 and t.dtype == u.dtype == v.dtype == torch.float32 and face.is_cuda and t.shape == face.shape
    return face.cpu().numpy(), torch.stack([t, u, v], dim=1).cpu().numpy()


def gpu_render(mesh, z_rows, envs, views, bounces=1, bq=BQ, H=FILM, W=FILM, bvh=None):
    from drmnet_amd.mesh import render_mesh

    z = torch.tensor(z_rows, dtype=torch.float32, device=DEV)
    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    view = None if views is None else torch.tensor(views, dtype=torch.float32)
    return [t.cpu().numpy().astype(np.float64) for t in render_mesh(as_obj(*mesh), z, NAMES6, env, image_size=(H, W), view_from=view, quad=Q, subpixel=S,
                                                                  shadows=True, bvh=bvh, bounces=bounces, bounce_quad=bq)]


# ---------------------------------------------------------------------------------------------- 1. exact queries
def test_exact_queries_equal_the_float64_rule_everywhere():
    from drmnet_amd.mesh import build_bvh

    p, f, o, d, ex, _ = tgs.exact_case()
    face, t, u, v = br.closest(p, f, o, d, ex)
    want = np.stack([t, u, v], axis=1).astype(np.float32)
    # the named ties, derived by hand: the ray from the origin along +z meets A (face 0) and B (face 1) on their shared edge x = 0, both at
    # t = 1/4: the lower index, and B with A excluded; the ray from (1/4, -1/2, 1/4) along +z meets D (face 3) and its duplicate (face 4) at the
    # same t: 3, and 4 with 3 excluded
    assert (o[0] == 0).all() and d[0].tolist() == [0, 0, 1] and ex[:2].tolist() == [-1, 0] and face[:2].tolist() == [0, 1] and t[0] == t[1] == 0.25
    assert o[12].tolist() == [0.25, -0.5, 0.25] and ex[12:14].tolist() == [-1, 3] and face[12:14].tolist() == [3, 4] and t[12] == t[13] > 0
    assert 0.1 <= (face >= 0).mean() <= 0.9 and len(np.unique(face)) == 7
    mesh = bare(p, f)
    for bvh in (build_bvh(mesh), None):
        got_face, got = gpu_closest(mesh, o, d, ex, bvh)
        assert np.array_equal(got_face, face), (bvh is None, np.nonzero(got_face != face)[0][:10])
        # (equal as float32 values: the sign of a zero u or v, the sign of a sum of products that cancel, is not part of the rule)
        assert np.array_equal(got, want), (bvh is None, np.nonzero((got != want).any(axis=1))[0][:10])
        assert got_face[0] == 0 and got_face[1] == 1 and got_face[12] == 3 and got_face[13] == 4
    # no exclusion at all (a NULL exclude array)
    face, t, u, v = br.closest(p, f, o, d)
    for bvh in ("auto", None):
        got_face, got = gpu_closest(mesh, o, d, None, bvh)
        assert np.array_equal(got_face, face) and np.array_equal(got, np.stack([t, u, v], axis=1).astype(np.float32))


# ---------------------------------------------------------------------------------------------- 2. the BVH changes nothing
@pytest.mark.parametrize("name", ["soup", "two_spheres"])
def test_the_bvh_changes_no_answer(name):
    from drmnet_amd.mesh import build_bvh

    p, f = (SOUP[0], SOUP[1]) if name == "soup" else (SCENE[0], SCENE[2])
    mesh = bare(p, f)
    blob = build_bvh(mesh)
    o, d, ex = tgs.rays_for(p, f, blob)
    assert len(o) >= 50000 and (d == 0).any(axis=1).sum() >= 10000
    for exclude in (None, ex):
        (tree_face, tree), (brute_face, brute) = gpu_closest(mesh, o, d, exclude, blob), gpu_closest(mesh, o, d, exclude, None)
        print(f"{name}: {len(o)} rays, {(brute_face >= 0).mean():.3f} with a closest hit")
        assert np.array_equal(tree_face, brute_face), np.nonzero(tree_face != brute_face)[0][:10]
        assert np.array_equal(tree.view(np.uint32), brute.view(np.uint32)), np.nonzero((tree.view(np.uint32) != brute.view(np.uint32)).any(axis=1))[0][:10]
        assert 0.1 <= (brute_face >= 0).mean() <= 0.9 and np.all(brute[brute_face < 0] == 0) and np.all(brute_face < len(f))
        if exclude is not None:
            assert not np.any(brute_face[brute_face >= 0] == exclude[brute_face >= 0])
        # a ray is occluded iff it has a closest hit
        assert np.array_equal(tree_face >= 0, tgs.gpu_occluded(mesh, o, d, exclude, blob))


# ---------------------------------------------------------------------------------------------- 3. the image against the restatement
def view_rot(v):
    return None if VIEWS[v] is None else rotation(VIEWS[v])


@functools.lru_cache(maxsize=None)
def scene_trace(v, r):
    """what the restatement of a (view, row) holds apart from the environment, on the shadow tests' own trace (shared, not changed)"""
    return br.trace(*SCENE, ROWS[r], view_rot(v), FILM, FILM, S, Q, BQ, shadow_trace=tgs.scene_trace(v, r))


@functools.lru_cache(maxsize=None)
def scene_ref(v, r, white):
    return br.shade(scene_trace(v, r), None if white else ENV)


@functools.lru_cache(maxsize=None)
def scene_gpu(v, white, bounces=1):
    """the three BSDF rows of a view in one call"""
    views = None if VIEWS[v] is None else [VIEWS[v]] * 3
    return gpu_render(SCENE, ROWS, None if white else [ENV] * 3, views, bounces)[0]


@pytest.mark.parametrize("v,r", tgs.SHADING)
def test_bounced_shading_matches_the_restatement(v, r):
    tr = scene_trace(v, r)
    # the comparison cannot empty itself: measured on the restatement alone
    rays = tr["traced"] + tr["inner_traced"]
    marginal = (tr["marginal"] + tr["hit_marginal"] + tr["inner_marginal"]) / rays
    unsafe, bounced, inner = tr["vis"]["unsafe"].mean(), tr["bounced"] / tr["traced"], tr["inner_occluded"] / tr["inner_traced"]
    assert tr["marginal"] / tr["traced"] <= CAP  # (the lobe rays alone: the larger count of inner rays must not dilute their share)
    assert marginal <= CAP and unsafe <= CAP and bounced >= 0.01 and tr["inner_traced"] >= 2000 and 0.05 <= inner <= 0.5
    for white in (False, True):
        ref = scene_ref(v, r, white)
        share = ref["slack"].sum() / ref["image"].sum()
        moved = rel_l2(ref["image"], ref["shadowed"])
        safe = ~ref["unsafe_pixel"]
        gpu = scene_gpu(v, white)[r]
        over = np.maximum(np.abs(gpu - ref["image"]) - ref["slack"], 0.0)[:, safe]
        err = float(np.linalg.norm(over) / np.linalg.norm(ref["image"][:, safe]))
        print(f"view {v} row {r} white {white}: marginal rays {marginal:.4f}, unsafe samples {unsafe:.4f}, bounced {bounced:.4f}, inner rays occluded "
              f"{inner:.3f}, slack share {share:.4f}, the bounce moves the image by {moved:.4f}, rel-L2 beyond the slack on safe pixels {err:.3g}, "
              f"without the bounce {rel_l2(scene_gpu(v, white, 0)[r][:, safe], ref['image'][:, safe]):.3g}")
        assert share <= CAP and safe.mean() >= 0.9 and (ref["image"][:, safe].sum(axis=0) > 0).sum() >= 50
        assert moved >= 0.01, (v, r, white, moved)
        assert err <= 1e-5, (v, r, white, err)


# ---------------------------------------------------------------------------------------------- 4. properties of the output
@pytest.mark.parametrize("v", range(len(VIEWS)))
def test_bounced_is_never_darker_and_no_bounce_is_the_shadowed_render(v):
    for white in (False, True):
        dark, lit = tgs.scene_gpu(v, white), scene_gpu(v, white)
        assert np.all(lit >= dark) and np.all(dark >= 0)
        for r in range(3):
            assert rel_l2(lit[r], dark[r]) > 1e-2, (v, r, white)
        assert np.array_equal(scene_gpu(v, white, 0), dark)
    if v == 1:
        # bounces=0 makes the shadowed entry's call: byte for byte its output, all four planes
        views, envs = [VIEWS[1]] * 3, [ENV] * 3
        status, direct = tgs.raw_call(SCENE, rows=ROWS, envs=envs, views=views)
        assert status == 0
        for a, b in zip(gpu_render(SCENE, ROWS, envs, views, bounces=0), direct):
            assert np.array_equal(a, b.astype(np.float64))


def test_a_flat_shaded_convex_mesh_has_no_bounce():
    from test_shadow_cpu import flat_icosphere

    mesh = flat_icosphere()
    for view in (None, (0.6, 0.3, 1.0)):
        views = None if view is None else [view] * 3
        dark, lit = (gpu_render(mesh, ROWS, [ENV] * 3, views, b)[0] for b in (0, 1))
        for r in range(3):
            slack = br.render(*mesh, ROWS[r], ENV, None if view is None else rotation(view), FILM, FILM, S, Q, bounce_quad=BQ)["slack"]
            diff = lit[r] - dark[r]
            assert np.all(diff >= 0) and np.all(diff <= slack * (1 + 1e-5) + 1e-7 * (slack > 0)) and np.all(diff[slack == 0] == 0), (view, r)
            assert (slack == 0).mean() > 0.5 and dark[r].max() > 0.1


def test_bounced_renders_are_reproducible_and_rows_are_independent():
    views = [(0.0, 0.0, 1.1), VIEWS[1], VIEWS[2]]
    envs = [ENV, 1.5 * ENV, ENV[:, ::-1].copy()]
    stacked = gpu_render(SCENE, ROWS, envs, views)
    again = gpu_render(SCENE, ROWS, envs, views)
    for a, b in zip(stacked, again):
        assert np.array_equal(a, b)
    for r in range(3):
        one = gpu_render(SCENE, ROWS[r:r + 1], envs[r:r + 1], views[r:r + 1])
        for a, b in zip(stacked, one):
            assert np.array_equal(a[r], b[0]), r
    assert not np.array_equal(stacked[0][0], stacked[0][1])
    # more directions per bounce: another estimate of the same light, never darker than the shadowed image either
    fine, dark = gpu_render(SCENE, ROWS, envs, views, bq=8)[0], gpu_render(SCENE, ROWS, envs, views, bounces=0)[0]
    assert not np.array_equal(fine, stacked[0]) and np.all(fine >= dark) and np.all(stacked[0] >= dark)


# ---------------------------------------------------------------------------------------------- 5. arguments and surface
def raw_bounced(mesh, bounce_quad=BQ, blob="build", blob_bytes=None, ws_bytes=None, H=FILM, W=FILM):
    """drm_render_mesh with bounces = 1 through ctypes on sentinel-filled outputs: (status, outputs)"""
    import abi_call
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    lib = _lib.lib()
    obj = {k: t.to(DEV) for k, t in as_obj(*mesh).items()}
    V, F = obj["vertex_positions"].shape[0], obj["faces"].shape[0]
    need = lib.drm_render_mesh_workspace_bytes(F, 1, H, W, S)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    z = torch.tensor([ROUGH], dtype=torch.float32, device=DEV)
    env = torch.tensor(ENV[None], dtype=torch.float32, device=DEV).contiguous()
    outs = [torch.full(s, -7.0, device=DEV) for s in ((1, 3, H, W), (1, 3, H, W), (1, 1, H, W), (1, H, W))]
    if isinstance(blob, str):
        blob = build_bvh(as_obj(*mesh))
    dev_blob = None if blob is None else blob.to(DEV)
    nbytes = (0 if blob is None else blob.numel()) if blob_bytes is None else blob_bytes
    sh = abi_call.shading(1, z=z.data_ptr(), env=env.data_ptr(), EH=env.shape[1], EW=env.shape[2], quad=Q)
    m = abi_call.mesh_render(obj["vertex_positions"].data_ptr(), obj["vertex_normals"].data_ptr(), obj["faces"].data_ptr(), V, F,
                             [o.data_ptr() for o in outs], H, W, S, ws.data_ptr(), need if ws_bytes is None else ws_bytes, shadows=1,
                             bvh=_lib.ptr(dev_blob), bvh_bytes=nbytes, bounces=1, bounce_quad=bounce_quad)
    status = abi_call.render_mesh(sh, m, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, [o.cpu().numpy() for o in outs]


def test_bad_arguments_launch_nothing():
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    ok, outs = raw_bounced(SCENE)
    assert ok == 0 and all(not np.any(o == -7.0) for o in outs)
    assert np.array_equal(outs[0][0].astype(np.float64), gpu_render(SCENE, [ROUGH], [ENV], None)[0][0])
    good = build_bvh(as_obj(*SCENE))
    other = build_bvh(as_obj(*mr.icosphere(1)))  # built for another F
    damaged = good.clone()
    damaged[0] ^= 0xFF  # the magic
    need = _lib.lib().drm_render_mesh_workspace_bytes(len(SCENE[2]), 1, FILM, FILM, S)
    INVALID, WORKSPACE = 1, 3
    for want, over in ((INVALID, dict(bounce_quad=0)), (INVALID, dict(bounce_quad=17)), (INVALID, dict(bounce_quad=-1)), (INVALID, dict(blob=None)),
                       (INVALID, dict(blob=other)), (INVALID, dict(blob=damaged)), (INVALID, dict(blob=good[:len(good) - 4].clone())),
                       (INVALID, dict(blob=good, blob_bytes=len(good) - 1)), (INVALID, dict(blob=good[:16].clone())), (WORKSPACE, dict(ws_bytes=need - 1))):
        status, outs = raw_bounced(SCENE, **over)
        assert status == want, (want, status, {k: (v if not torch.is_tensor(v) else len(v)) for k, v in over.items()})
        assert all(np.all(o == -7.0) for o in outs)
    # the closest-hit query checks its blob as well, and a bad one leaves the outputs alone
    lib = _lib.lib()
    obj = {k: t.to(DEV) for k, t in as_obj(*SCENE).items()}
    o = torch.zeros(8, 3, device=DEV)
    d = torch.ones(8, 3, device=DEV)
    face = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    tuv = torch.full((8, 3), -7.0, device=DEV)
    for blob in (other, damaged):
        b = blob.to(DEV)
        status = lib.drm_mesh_closest_hit(obj["vertex_positions"].data_ptr(), obj["faces"].data_ptr(), obj["vertex_positions"].shape[0], len(SCENE[2]),
                                          b.data_ptr(), o.data_ptr(), d.data_ptr(), None, face.data_ptr(), tuv.data_ptr(), 8, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert status == INVALID and bool((face == -7).all()) and bool((tuv == -7.0).all())
    with pytest.raises(RuntimeError):
        gpu_render(SCENE, [ROUGH], [ENV], None, bvh=other)
    from drmnet_amd.mesh import closest_hit

    with pytest.raises(ValueError):
        closest_hit(as_obj(*SCENE), o, d[:4])
    with pytest.raises(ValueError):
        closest_hit(as_obj(*SCENE), o, d, torch.zeros(3, dtype=torch.int32))


def test_mesh_renderer_keeps_the_bvh_with_its_scene(monkeypatch):
    from drmnet_amd import mesh as mesh_mod
    from drmnet_amd.mesh import MeshRenderer, render_mesh

    builds = []
    real = mesh_mod.build_bvh
    monkeypatch.setattr(mesh_mod, "build_bvh", lambda obj: builds.append(1) or real(obj))
    obj = as_obj(*SCENE)
    env = torch.tensor(ENV, dtype=torch.float32)
    z = torch.tensor(ROUGH)
    view = (0.6, 0.3, 1.0)
    r = MeshRenderer(FILM, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q, shadows=True, bounces=1, bounce_quad=BQ)
    first = r.rendering(z, NAMES6, env, obj=obj, channel_first=True)
    blob = r._bvh
    assert len(builds) == 1 and blob is not None and blob.is_cuda
    second = r.rendering(z, NAMES6, channel_first=True)
    assert len(builds) == 1 and r._bvh is blob and torch.equal(first, second)
    want = render_mesh(obj, z[None].to(DEV), NAMES6, env[None].to(DEV), image_size=FILM, view_from=torch.tensor([view]), quad=Q, shadows=True, bounces=1,
                       bounce_quad=BQ)[0][0]
    assert len(builds) == 2 and torch.equal(first, want)
    assert torch.equal(first, torch.tensor(scene_gpu(1, False)[0], dtype=torch.float32, device=DEV))
    dark = MeshRenderer(FILM, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q, shadows=True).rendering(z, NAMES6, env, obj=obj, channel_first=True)
    assert bool((first >= dark).all()) and not torch.equal(first, dark)


def test_synthesize_with_a_bounce(tmp_path):
    from drmnet_amd import file_io, synthesize
    from drmnet_amd.mesh import normalize_mesh, render_mesh

    obj = as_obj(*SCENE)
    torch.save(dict(obj), tmp_path / "scene.pt")
    file_io.save_exr(tmp_path / "env.exr", ENV.astype(np.float32))
    out = {}
    for flags in (["--shadows"], ["--shadows", "--bounces", "1", "--bounce_quad", str(BQ)]):
        d = tmp_path / ("out" + str(len(flags)))
        synthesize.main(["--mesh", str(tmp_path / "scene.pt"), "--envmap", str(tmp_path / "env.exr"), "--z", *[str(x) for x in ROUGH], "--view_from", "0.6",
                         "0.3", "1.0", "--image_size", str(FILM), "--refmap_res", "8", "--quad", str(Q), "--output_dir", str(d), *flags])
        assert all((d / n).exists() for n in ("image.exr", "normal.npy", "mask.png", "refmap.exr"))
        out[len(flags) > 1] = (file_io.load_exr(d / "image.exr"), file_io.load_exr(d / "refmap.exr"), np.load(d / "normal.npy"))
    # (synthesize scales the mesh to radius 0.9: compare with a render of the same normalised mesh)
    image = render_mesh(normalize_mesh(obj), torch.tensor([ROUGH], device=DEV), NAMES6, torch.tensor(ENV[None], dtype=torch.float32, device=DEV),
                        image_size=FILM, view_from=torch.tensor([(0.6, 0.3, 1.0)]), quad=Q, shadows=True, bounces=1, bounce_quad=BQ)[0][0]
    assert np.array_equal(out[True][0], image.permute(1, 2, 0).cpu().numpy())
    assert np.array_equal(out[True][1], out[False][1]) and np.array_equal(out[True][2], out[False][2])
    assert np.all(out[True][0] >= out[False][0]) and rel_l2(out[True][0], out[False][0]) > 1e-2

"""Light sampling on mesh object images on the GPU (drm_render_mesh with light samples: mesh_shade_kernel<VIEW, SHADOW, true> in csrc/render.hip, through
drmnet_amd.mesh and drmnet_amd.synthesize) against the float64 restatement tests/mesh_light_ref.py.

The scene is the two-sphere scene of tests/test_gpu_shadow.py (a ball over a body) on its 16 x 16 film, S = 2, Q = 8, with M = 64 light
samples, under a random-valued 16 x 32 map (no CDF boundary lands on a dyadic sample) with one hot texel placed so that the ball's shadow
falls on the body.  The image is compared as the shadowed image is: on the pixels that are not `unsafe_pixel`, after taking off `slack`, the
absolute contributions of the pixel's marginal lobe and light rays, at the 1e-5 rel-L2 bar of the shadowed mesh image and the lit sphere
render.  What keeps that comparison from emptying itself is asserted on the restatement alone, over the nine (view, row) cases: marginal rays
<= 2 % of the traced rays (lobe and light), slack <= 2 % of the image sum, unsafe samples <= 2 %, safe pixels >= 90 %, occluded light rays
>= 1 %.  On the committed map the restatement gives: marginal rays <= 1.15 %, slack share <= 0.59 % (single pixels up to 8 %), unsafe samples
<= 0.59 %, safe pixels >= 97.7 %, 2.7 % ... 4.8 % of the 6 586 ... 13 843 light rays occluded; the float64 image moves by 4.8 % ... 14.9 % when
the shadows are traced from the views that see the lit side (the view from (-1, 0.2, 0.4) looks at the far side: under 1 %)."""
import functools

import numpy as np
import pytest
import torch

import mesh_light_ref as mlr
from conftest import rel_l2
from test_gpu_mesh import as_obj, rotation
from test_gpu_shadow import CAP, FILM, Q, ROUGH, ROWS, S, SCENE, VIEWS, raw_call
from test_render_cpu import NAMES6
from test_render_light_cpu import random_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
M = 64
SUN = (4, 11)  # the texel nearest to (0.66, 0.57, 0.49), the direction of the ball from the centre of the body


def f32(a):
    """what the GPU is given, as float64 for the restatement"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


ENV = f32(random_env(16, 32, 21, [(SUN[0], SUN[1], 3e4)]))
SHADING = [(v, r) for v in range(len(VIEWS)) for r in range(len(ROWS))]


def view_rot(v):
    return None if VIEWS[v] is None else rotation(VIEWS[v])


@functools.lru_cache(maxsize=None)
def scene_trace(v, r, shadows):
    """what the restatement of a (view, row) holds apart from the environment, computed once"""
    return mlr.trace(*SCENE, ROWS[r], view_rot(v), FILM, FILM, S, Q, shadows)


@functools.lru_cache(maxsize=None)
def scene_ref(v, r, shadows):
    return mlr.shade(scene_trace(v, r, shadows), ENV, M, SCENE[0], SCENE[2])


def gpu_render(mesh, z_rows, envs, views, shadows, light_samples=M, H=FILM, W=FILM, bvh=None):
    from drmnet_amd.mesh import render_mesh

    z = torch.tensor(z_rows, dtype=torch.float32, device=DEV)
    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    view = None if views is None else torch.tensor(views, dtype=torch.float32)
    return [t.cpu().numpy().astype(np.float64) for t in render_mesh(as_obj(*mesh), z, NAMES6, env, image_size=(H, W), view_from=view, quad=Q, subpixel=S,
                                                                  shadows=shadows, bvh=bvh, light_samples=light_samples)]


@functools.lru_cache(maxsize=None)
def scene_gpu(v, shadows, light_samples=M):
    """the three BSDF rows of a view in one call"""
    views = None if VIEWS[v] is None else [VIEWS[v]] * 3
    return gpu_render(SCENE, ROWS, [ENV] * 3, views, shadows, light_samples)[0]


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("v,r", SHADING)
def test_lit_mesh_images_match_the_restatement(v, r):
    ref = scene_ref(v, r, True)
    # the comparison cannot empty itself: measured on the restatement alone
    traced = ref["lobe_traced"] + ref["light_traced"]
    marginal = (ref["lobe_marginal"] + ref["light_marginal"]) / traced
    unsafe = scene_trace(v, r, True)["vis"]["unsafe"].mean()
    occl = ref["light_occluded"] / ref["light_traced"]
    safe = ~ref["unsafe_pixel"]
    share = ref["slack"].sum() / ref["image"].sum()
    moved = rel_l2(ref["image"], scene_ref(v, r, False)["image"])
    print(f"view {v} row {r}: marginal rays {marginal:.4f}, slack share {share:.4f}, unsafe samples {unsafe:.4f}, safe pixels {safe.mean():.4f}, "
          f"light rays occluded {occl:.4f} of {ref['light_traced']}, image moved by the shadows {moved:.3f}")
    assert marginal <= CAP and share <= CAP and unsafe <= CAP and safe.mean() >= 0.9 and occl >= 0.01
    assert ref["light_traced"] >= 5000 and (ref["image"][:, safe].sum(axis=0) > 0).sum() >= 50
    for shadows in (False, True):
        ref = scene_ref(v, r, shadows)
        assert shadows or not ref["slack"].any()
        gpu = scene_gpu(v, shadows)[r]
        over = np.maximum(np.abs(gpu - ref["image"]) - ref["slack"], 0.0)[:, safe]
        err = float(np.linalg.norm(over) / np.linalg.norm(ref["image"][:, safe]))
        print(f"view {v} row {r} shadows {shadows}: rel-L2 beyond the slack on safe pixels {err:.3g}")
        assert err <= 1e-5, (v, r, shadows, err)


# ---------------------------------------------------------------------------------------------- 2. neutral and monotonic
def raw_lit(mesh, shadowed=True, rows=(ROUGH,), envs=(ENV,), views=None, light_samples=M, blob="build", blob_bytes=None, ws_bytes=None, lws_bytes=None,
            lws_offset=0, H=FILM, W=FILM):
    """drm_render_mesh with light samples through ctypes on sentinel-filled outputs: (status, outputs)"""
    import abi_call
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh
    from drmnet_amd.render import view_rotation

    lib = _lib.lib()
    obj = {k: t.to(DEV) for k, t in as_obj(*mesh).items()}
    B, V, F = len(rows), obj["vertex_positions"].shape[0], obj["faces"].shape[0]
    need = lib.drm_render_mesh_workspace_bytes(F, B, H, W, S)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    z = torch.tensor(rows, dtype=torch.float32, device=DEV)
    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV).contiguous()
    EH, EW = (0, 0) if env is None else (env.shape[1], env.shape[2])
    view = None if views is None else view_rotation(torch.tensor(views, dtype=torch.float32)).to(DEV).contiguous()
    outs = [torch.full(s, -7.0, device=DEV) for s in ((B, 3, H, W), (B, 3, H, W), (B, 1, H, W), (B, H, W))]
    light_need = int(lib.drm_render_light_workspace_bytes(B, max(EH, 1), max(EW, 1), M))
    lws = torch.zeros(light_need // 8 + 2, dtype=torch.float64, device=DEV)
    if shadowed and isinstance(blob, str):
        blob = build_bvh(as_obj(*mesh))
    dev_blob = None if (blob is None or not shadowed) else blob.to(DEV)
    nbytes = (0 if dev_blob is None else dev_blob.numel()) if blob_bytes is None else blob_bytes
    sh = abi_call.shading(B, z=z.data_ptr(), env=_lib.ptr(env), EH=EH, EW=EW, view=_lib.ptr(view), quad=Q, light_samples=light_samples,
                          lws=lws.data_ptr() + lws_offset, lws_bytes=light_need if lws_bytes is None else lws_bytes)
    # shadows: what the blob and its length say together (a blob without a length, or a length without a blob, asks for shadows)
    m = abi_call.mesh_render(obj["vertex_positions"].data_ptr(), obj["vertex_normals"].data_ptr(), obj["faces"].data_ptr(), V, F,
                             [o.data_ptr() for o in outs], H, W, S, ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                             shadows=int(dev_blob is not None or nbytes != 0), bvh=_lib.ptr(dev_blob), bvh_bytes=nbytes)
    status = abi_call.render_mesh(sh, m, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, [o.cpu().numpy() for o in outs]


def test_without_light_samples_it_is_the_old_entries_byte_for_byte():
    views = [(0.0, 0.0, 1.1), VIEWS[1], VIEWS[2]]
    envs = [ENV, 1.5 * ENV, ENV[:, ::-1].copy()]
    for shadowed in (False, True):
        status, old = raw_call(SCENE, shadowed=shadowed, rows=ROWS, envs=envs, views=views)
        assert status == 0
        # light_samples = 0: the light workspace is not read
        status, new = raw_lit(SCENE, shadowed=shadowed, rows=ROWS, envs=envs, views=views, light_samples=0, lws_bytes=0)
        assert status == 0
        for a, b in zip(old, new):
            assert np.array_equal(a, b)
        got = gpu_render(SCENE, ROWS, envs, views, shadowed, light_samples=0)
        for a, b in zip(old, got):
            assert np.array_equal(a.astype(np.float64), b)
        assert not np.array_equal(old[0], raw_lit(SCENE, shadowed=shadowed, rows=ROWS, envs=envs, views=views)[1][0])
    # no map: the white environment, whatever light_samples says
    from drmnet_amd.mesh import render_mesh

    obj, z = as_obj(*SCENE), torch.tensor(ROWS, dtype=torch.float32, device=DEV)
    for shadowed in (False, True):
        white = [render_mesh(obj, z, NAMES6, None, image_size=FILM, quad=Q, subpixel=S, shadows=shadowed, light_samples=m)[0] for m in (0, M)]
        assert torch.equal(white[0], white[1])
        status, raw = raw_lit(SCENE, shadowed=shadowed, rows=ROWS, envs=None, light_samples=M, lws_bytes=0)
        assert status == 0 and np.array_equal(raw[0], white[0].cpu().numpy())


def test_a_black_map_in_the_batch_renders_as_without_light_samples():
    """the standard of the sphere's black-map case"""
    envs = np.stack([ENV, np.zeros_like(ENV), -ENV])  # black; all non-positive: no light technique either
    for shadowed in (False, True):
        lit = gpu_render(SCENE, ROWS, envs, None, shadowed)[0]
        plain = gpu_render(SCENE, ROWS, envs, None, shadowed, light_samples=0)[0]
        assert np.isfinite(lit).all()
        assert np.all(lit[1] == 0) and np.abs(lit[1] - plain[1]).max() <= 1e-6
        assert rel_l2(lit[2], plain[2]) <= 1e-6
        assert rel_l2(lit[0], plain[0]) > 1e-3  # the lit map of the batch did get its light samples


@pytest.mark.parametrize("v", range(len(VIEWS)))
def test_shadowed_is_never_brighter(v):
    lit, dark = scene_gpu(v, False), scene_gpu(v, True)
    assert ENV.min() >= 0 and np.all(dark <= lit) and np.all(dark >= 0) and (dark < lit).sum() >= 100


# ---------------------------------------------------------------------------------------------- 3. determinism
def test_lit_mesh_renders_are_reproducible_and_rows_are_independent():
    views = [(0.0, 0.0, 1.1), VIEWS[1], VIEWS[2]]
    envs = [ENV, f32(random_env(16, 32, 22, [(9, 25, 1e4)])), ENV[:, ::-1].copy()]
    for shadowed in (False, True):
        stacked = gpu_render(SCENE, ROWS, envs, views, shadowed)
        again = gpu_render(SCENE, ROWS, envs, views, shadowed)
        for a, b in zip(stacked, again):
            assert np.array_equal(a, b)
        for r in range(3):
            one = gpu_render(SCENE, ROWS[r:r + 1], envs[r:r + 1], views[r:r + 1], shadowed)
            for a, b in zip(stacked, one):
                assert np.array_equal(a[r], b[0]), (shadowed, r)
        assert not np.array_equal(stacked[0][0], stacked[0][1])
        # render_mesh(light_samples = M) is drm_render_mesh with light samples itself
        status, direct = raw_lit(SCENE, shadowed=shadowed, rows=ROWS, envs=envs, views=views)
        assert status == 0
        for a, b in zip(stacked, direct):
            assert np.array_equal(a, b.astype(np.float64))


# ---------------------------------------------------------------------------------------------- 4. arguments
def test_bad_light_arguments_launch_nothing():
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    lib = _lib.lib()
    ok, outs = raw_lit(SCENE)
    assert ok == 0 and all(not np.any(o == -7.0) for o in outs)
    assert np.array_equal(outs[0][0].astype(np.float64), gpu_render(SCENE, [ROUGH], [ENV], None, True)[0][0])
    ok, outs = raw_lit(SCENE, shadowed=False)
    assert ok == 0 and np.array_equal(outs[0][0].astype(np.float64), gpu_render(SCENE, [ROUGH], [ENV], None, False)[0][0])
    good = build_bvh(as_obj(*SCENE))
    damaged = good.clone()
    damaged[0] ^= 0xFF  # the magic
    need = lib.drm_render_mesh_workspace_bytes(len(SCENE[2]), 1, FILM, FILM, S)
    light_need = int(lib.drm_render_light_workspace_bytes(1, 16, 32, M))
    INVALID, WORKSPACE = 1, 3
    cases = [(INVALID, dict(light_samples=m)) for m in (100, 32, 1 << 17, -64)]
    cases += [(INVALID, dict(lws_bytes=light_need - 8)), (INVALID, dict(lws_bytes=0)), (INVALID, dict(lws_offset=4)),  # short, none, misaligned
              (INVALID, dict(blob=damaged)), (INVALID, dict(blob=good[:len(good) - 4].clone())), (INVALID, dict(blob=good, blob_bytes=len(good) - 1)),
              (INVALID, dict(blob=good, blob_bytes=0)),              # a blob without a length
              (INVALID, dict(shadowed=False, blob_bytes=len(good))),  # a length without a blob
              (WORKSPACE, dict(ws_bytes=need - 1))]
    for want, over in cases:
        status, outs = raw_lit(SCENE, **over)
        assert status == want and lib.drm_last_error(), (want, status, {k: (v if not torch.is_tensor(v) else len(v)) for k, v in over.items()})
        assert all(np.all(o == -7.0) for o in outs), over
    with pytest.raises(ValueError):
        gpu_render(SCENE, [ROUGH], [ENV], None, True, light_samples=100)
    with pytest.raises(ValueError):
        gpu_render(SCENE, [ROUGH], [ENV], None, False, light_samples=-64)


# ---------------------------------------------------------------------------------------------- 5. surface
def test_mesh_renderer_and_synthesize_carry_light_samples(tmp_path):
    from drmnet_amd import file_io, synthesize
    from drmnet_amd.mesh import MeshRenderer, render_mesh
    from drmnet_amd.render import render

    obj = as_obj(*SCENE)
    env = torch.tensor(ENV, dtype=torch.float32)
    z = torch.tensor(ROUGH)
    view = (0.6, 0.3, 1.0)
    r = MeshRenderer(FILM, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q, shadows=True, light_samples=M)
    first = r.rendering(z, NAMES6, env, obj=obj, channel_first=True)
    want = render_mesh(obj, z[None].to(DEV), NAMES6, env[None].to(DEV), image_size=FILM, view_from=torch.tensor([view]), quad=Q, shadows=True,
                       light_samples=M)[0][0]
    assert torch.equal(first, want) and torch.equal(first, torch.tensor(scene_gpu(1, True)[0], dtype=torch.float32, device=DEV))
    unlit = MeshRenderer(FILM, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q, shadows=True).rendering(z, NAMES6, env, obj=obj, channel_first=True)
    assert not torch.equal(first, unlit)

    torch.save(dict(obj), tmp_path / "scene.pt")
    file_io.save_exr(tmp_path / "env.exr", ENV.astype(np.float32))
    out = {}
    for flags in ([], ["--light_samples", str(M), "--shadows"]):
        d = tmp_path / ("out" + str(len(flags)))
        synthesize.main(["--mesh", str(tmp_path / "scene.pt"), "--envmap", str(tmp_path / "env.exr"), "--z", *[str(x) for x in ROUGH], "--view_from", "0.6",
                         "0.3", "1.0", "--image_size", str(FILM), "--refmap_res", "8", "--quad", str(Q), "--output_dir", str(d), *flags])
        assert all((d / n).exists() for n in ("image.exr", "normal.npy", "mask.png", "refmap.exr"))
        out[bool(flags)] = (file_io.load_exr(d / "image.exr"), file_io.load_exr(d / "refmap.exr"))
    # both files are the lit renders: the image (the mesh was already radius <= 0.9: synthesize's scaling moves it, so compare by a render of
    # the same normalised mesh) and the reflectance map
    from drmnet_amd.mesh import normalize_mesh

    zd, envd, vf = z[None].to(DEV), env[None].to(DEV), torch.tensor([view])
    image = render_mesh(normalize_mesh(obj), zd, NAMES6, envd, image_size=FILM, view_from=vf, quad=Q, shadows=True, light_samples=M)[0][0]
    refmap = render(zd, NAMES6, envd, res=8, quad=Q, view_from=vf, light_samples=M)[0]
    assert np.array_equal(out[True][0], image.permute(1, 2, 0).cpu().numpy()) and np.array_equal(out[True][1], refmap.permute(1, 2, 0).cpu().numpy())
    assert rel_l2(out[True][0], out[False][0]) > 1e-2 and rel_l2(out[True][1], out[False][1]) > 1e-2

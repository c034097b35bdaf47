"""Object images from a normal map on the GPU (drm_render_normals: normals_pixel_kernel in csrc/render_shared.h; drm_image_from_refmap:
image_from_refmap_kernel in csrc/refmap.hip; through drmnet_amd.relight and the two command lines) against the float64 restatement
tests/relight_ref.py.

Bars.  A shaded image is held to the 1e-5 rel-L2 of the sphere and mesh images against their restatements (the kernel shares their
per-normal sum).  The lookup is compared outside the restatement's marginal set (a coordinate within 1e-4 texel of an integer, where fp32
may take other taps): the fp32 coordinates are off by a few ulp of R, about 1e-5 texel, on a map whose texel-to-texel change is a fraction
of its value, so 1e-5 rel-L2 again.  The measured figures are in DESIGN.md 6f.  All shaded comparisons use quad 8."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import relight_ref as rl
import render_ref as rr
from conftest import GOLD, gold, rel_l2
from test_gpu_mesh import ENV, ROWS, ROUGH, SPHERE, as_obj, rotation, smooth_env
from test_render_cpu import NAMES6
from test_render_light_cpu import random_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Q = 8
VIEW = (0.6, 0.3, 1.0)  # the oblique view of the mesh tests
NORMALS, MASK = rl.normal_map(5)
M = 64
HOT = np.asarray(random_env(16, 32, 21, [(4, 11, 3e4)]), dtype=np.float32).astype(np.float64)  # one hot texel, as the GPU is given it


def gpu_shade(normals, mask, rows, envs, views, light_samples=0):
    from drmnet_amd.relight import render_normals

    z = torch.tensor(rows, dtype=torch.float32, device=DEV)
    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    view = None if views is None else torch.tensor(views, dtype=torch.float32)
    image, alpha = render_normals(torch.as_tensor(normals).to(DEV), z, NAMES6, env, mask=None if mask is None else torch.as_tensor(mask).to(DEV),
                                  view_from=view, quad=Q, light_samples=light_samples)
    return image.cpu().numpy(), alpha.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. shading against the restatement
@pytest.mark.parametrize("with_env", [False, True])
@pytest.mark.parametrize("with_view", [False, True])
def test_shading_matches_the_restatement(with_env, with_view):
    image, alpha = gpu_shade(NORMALS, MASK, ROWS, [ENV] * 3 if with_env else None, [VIEW] * 3 if with_view else None)
    _, drawn = rl.unit_normals(NORMALS, MASK)
    assert 60 <= drawn.sum() <= 110 and (NORMALS[..., 2] <= 0).sum() >= 36  # (a third of 144, within its sampling spread)
    assert not drawn[0, :4].any() and drawn[0, 4] and drawn[0, 5] and drawn[1, 4] and drawn[1, 5]
    for b in range(3):
        ref, _ = rl.shade(ROWS[b], ENV if with_env else None, NORMALS, MASK, Q, rotation(VIEW) if with_view else None)
        err = rel_l2(image[b], ref)
        print(f"env {with_env} view {with_view} row {b}: image rel-L2 {err:.3g}")
        assert err <= 1e-5, (b, err)
        assert ref[:, drawn].min() > 0
        # the pixels that are not drawn are exactly 0 with alpha 0
        assert np.array_equal(alpha[b], drawn.astype(np.float32)) and not image[b][:, ~drawn].any() and (image[b][:, drawn] > 0).all()
        # a normal scaled by a power of two is its unit twin bit for bit
        assert np.array_equal(image[b][:, 0, 4], image[b][:, 1, 4]) and np.array_equal(image[b][:, 0, 5], image[b][:, 1, 5])
    assert rel_l2(image[0], image[1]) > 1e-2
    if with_env and with_view:
        assert rel_l2(image, gpu_shade(NORMALS, MASK, ROWS, [ENV] * 3, None)[0]) > 1e-2  # the view did turn the environment
    if with_view and not with_env:
        assert np.array_equal(image, gpu_shade(NORMALS, MASK, ROWS, None, None)[0])  # under a white environment it changes nothing


# ---------------------------------------------------------------------------------------------- 2. consistency with the mesh render
def test_a_mesh_image_is_its_normal_map_shaded():
    from drmnet_amd.mesh import render_mesh
    from drmnet_amd.relight import render_normals

    z = torch.tensor(ROWS, dtype=torch.float32, device=DEV)
    env = torch.tensor(np.stack([ENV] * 3), dtype=torch.float32, device=DEV)
    for view in (None, torch.tensor([VIEW] * 3, dtype=torch.float32)):
        image, normal, _, alpha = render_mesh(as_obj(*SPHERE), z, NAMES6, env, image_size=16, view_from=view, quad=Q, subpixel=1)
        again, alpha2 = render_normals(normal.permute(0, 2, 3, 1), z, NAMES6, env, mask=alpha > 0, view_from=view, quad=Q)
        err = rel_l2(again.cpu(), image.cpu())
        away = (alpha > 0) & (normal[:, 2] <= 0)
        print(f"view {view is not None}: mesh image against its shaded normal map: rel-L2 {err:.3g}, bits equal: {torch.equal(again, image)}, "
              f"hits facing away {int(away.sum())}")
        # The mesh's alpha says "hit", this one "drawn".  From +z every hit of the sphere faces the viewer (the restatement: 0 of 156 hits face
        # away) and the two are the same exactly; from the oblique view the coarse sphere's silhouette faces reach behind the horizon (2 of
        # 164 hits have n.z <= 0): the mesh leaves those black with alpha 1, here they are not drawn.
        assert torch.equal(alpha2, alpha * (normal[:, 2] > 0)) and 100 <= int((alpha[0] > 0).sum()) <= 256
        assert not image.permute(0, 2, 3, 1)[away].any()
        if view is None:
            assert torch.equal(alpha2, alpha) and not away.any()
        assert err <= 1e-5


# ---------------------------------------------------------------------------------------------- 3. light samples
def test_light_samples_match_the_restatement_and_are_neutral_where_they_must_be():
    lit, alpha = gpu_shade(NORMALS, MASK, ROWS, [HOT] * 3, [VIEW] * 3, light_samples=M)
    unlit, alpha0 = gpu_shade(NORMALS, MASK, ROWS, [HOT] * 3, [VIEW] * 3)
    assert np.array_equal(alpha, alpha0)
    for b in range(3):
        ref, _ = rl.shade_lit(ROWS[b], HOT, NORMALS, MASK, Q, M, rotation(VIEW))
        err = rel_l2(lit[b], ref)
        print(f"row {b}: lit image rel-L2 {err:.3g}; lit against unlit {rel_l2(lit[b], unlit[b]):.3g}")
        assert err <= 1e-5, (b, err)
        assert rel_l2(lit[b], unlit[b]) > 1e-3  # a kernel that ignores the table fails here
        assert rel_l2(unlit[b], rl.shade(ROWS[b], HOT, NORMALS, MASK, Q, rotation(VIEW))[0]) <= 1e-5
    # a black map, and one that is nowhere positive, in a batch of three render as without light samples
    envs = np.stack([HOT, np.zeros_like(HOT), -HOT])
    lit3, plain3 = gpu_shade(NORMALS, MASK, ROWS, envs, None, light_samples=M)[0], gpu_shade(NORMALS, MASK, ROWS, envs, None)[0]
    assert np.isfinite(lit3).all() and np.all(lit3[1] == 0) and np.abs(lit3[1] - plain3[1]).max() <= 1e-6 and rel_l2(lit3[2], plain3[2]) <= 1e-6
    assert rel_l2(lit3[0], plain3[0]) > 1e-3
    # no map: the white environment, whatever light_samples says
    assert np.array_equal(gpu_shade(NORMALS, MASK, ROWS, None, None, light_samples=M)[0], gpu_shade(NORMALS, MASK, ROWS, None, None)[0])


# ---------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("light_samples", [0, M])
def test_renders_are_reproducible_and_rows_are_independent(light_samples):
    envs = [HOT, smooth_env(16, 32, 1), HOT[:, ::-1].copy()]
    views = [(0.0, 0.0, 1.1), VIEW, (-1.0, 0.2, 0.4)]
    maps = np.stack([NORMALS, rl.normal_map(6)[0], rl.normal_map(7)[0]])
    masks = np.stack([MASK, MASK, np.ones_like(MASK)])
    stacked = gpu_shade(maps, masks, ROWS, envs, views, light_samples)
    again = gpu_shade(maps, masks, ROWS, envs, views, light_samples)
    assert np.array_equal(stacked[0], again[0]) and np.array_equal(stacked[1], again[1])
    for r in range(3):
        one = gpu_shade(maps[r], masks[r], ROWS[r:r + 1], envs[r:r + 1], views[r:r + 1], light_samples)
        assert np.array_equal(stacked[0][r], one[0][0]) and np.array_equal(stacked[1][r], one[1][0]), r
    assert not np.array_equal(stacked[0][0], stacked[0][1])
    # Bn = 1: one normal map relit three ways is the map repeated three times
    shared = gpu_shade(NORMALS, MASK, ROWS, envs, views, light_samples)
    repeated = gpu_shade(np.stack([NORMALS] * 3), np.stack([MASK] * 3), ROWS, envs, views, light_samples)
    assert np.array_equal(shared[0], repeated[0]) and np.array_equal(shared[1], repeated[1])


# ---------------------------------------------------------------------------------------------- 5. the lookup
R = 16


@functools.lru_cache(maxsize=None)
def smooth_refmaps():
    """reflectance maps of the ROUGH row under two smooth environments, as the GPU renders them: [2, 3, R, R] float32"""
    from drmnet_amd.render import render

    env = torch.tensor(np.stack([ENV, smooth_env(16, 32, 2)]), dtype=torch.float32, device=DEV)
    return render(torch.tensor([ROUGH, ROUGH], dtype=torch.float32, device=DEV), NAMES6, env, res=R, quad=Q)


def gpu_lookup(refmap, normals, mask=None, refmask=None):
    from drmnet_amd.relight import image_from_refmap

    image, alpha = image_from_refmap(refmap, torch.as_tensor(normals).to(DEV), mask=None if mask is None else torch.as_tensor(mask).to(DEV),
                                     refmask=None if refmask is None else torch.as_tensor(refmask).to(DEV))
    return image.cpu().numpy(), alpha.cpu().numpy()


def test_the_lookup_matches_the_restatement():
    refmaps = smooth_refmaps()
    v = refmaps.cpu().numpy().astype(np.float64)
    refmask = np.random.default_rng(11).uniform(size=(R, R)) < 0.7
    for masked in (False, True):
        image, alpha = gpu_lookup(refmaps[0], NORMALS, MASK, refmask if masked else None)
        ref, valid, marginal = rl.lookup(v[0], refmask if masked else None, NORMALS, MASK)
        _, drawn = rl.unit_normals(NORMALS, MASK)
        share = marginal.sum() / drawn.sum()
        print(f"refmask {masked}: marginal pixels {share:.4f} of {int(drawn.sum())}, valid {int(valid.sum())}")
        assert share <= 0.02 and valid.sum() >= (10 if masked else 60) and (not masked or (drawn & ~valid).sum() >= 20)
        keep = ~marginal
        assert np.array_equal(alpha[0][keep], valid[keep].astype(np.float32)) and not image[0][:, alpha[0] == 0].any()
        err = rel_l2(image[0][:, keep], ref[:, keep])
        print(f"refmask {masked}: lookup rel-L2 outside the marginal set {err:.3g}")
        assert err <= 1e-5 and ref[:, keep & valid].min() > 0
        assert not alpha[0][0, :4].any() and np.array_equal(image[0][:, 0, 4], image[0][:, 1, 4]) and np.array_equal(image[0][:, 0, 5], image[0][:, 1, 5])
    # Br = 2 maps on one normal map, Bn = 2 normal maps on one map, and both: every row is the single call
    two = np.stack([NORMALS, rl.normal_map(6)[0]])
    one = [gpu_lookup(refmaps[r], two[n], MASK) for r, n in ((0, 0), (1, 0), (0, 1), (1, 1))]
    for got, rows in ((gpu_lookup(refmaps, NORMALS, MASK), (0, 1)), (gpu_lookup(refmaps[0], two, np.stack([MASK] * 2)), (0, 2)),
                      (gpu_lookup(refmaps, two, np.stack([MASK] * 2)), (0, 3))):
        for b, k in enumerate(rows):
            assert np.array_equal(got[0][b], one[k][0][0]) and np.array_equal(got[1][b], one[k][1][0])
    assert not np.array_equal(one[0][0], one[1][0]) and not np.array_equal(one[0][0], one[2][0])


def test_the_lookup_at_the_texel_centres_returns_the_map():
    refmaps = smooth_refmaps()
    centres = rr.sensor_normals(R, 1, False)[:, :, 0].astype(np.float32)
    image, alpha = gpu_lookup(refmaps[0], centres)
    err = rel_l2(image[0], refmaps[0].cpu().numpy())
    print(f"texel-centre round trip: rel-L2 {err:.3g}")
    assert alpha.all() and err <= 1e-5


# ---------------------------------------------------------------------------------------------- 6. arguments
def raw_normals(B=3, Bn=1, H=12, W=12, EH=16, EW=32, quad=Q, light_samples=0, env=True, lws="ok", lws_bytes=None, lws_offset=0):
    """drm_render_normals through ctypes on sentinel-filled outputs of the good sizes: (status, outputs)"""
    import abi_call
    from drmnet_amd import _lib

    lib = _lib.lib()
    nrm = torch.tensor(np.stack([NORMALS] * 3), device=DEV)
    z = torch.tensor(ROWS, dtype=torch.float32, device=DEV)
    e = torch.tensor(np.stack([HOT] * 3), dtype=torch.float32, device=DEV)
    outs = [torch.full((3, 3, 12, 12), -7.0, device=DEV), torch.full((3, 12, 12), -7.0, device=DEV)]
    need = int(lib.drm_render_light_workspace_bytes(3, 16, 32, M))
    ws = torch.zeros(need // 8 + 2, dtype=torch.float64, device=DEV)
    sh = abi_call.shading(B, z=z.data_ptr(), env=e.data_ptr() if env else None, EH=EH, EW=EW, quad=quad, light_samples=light_samples,
                          lws=None if lws is None else ws.data_ptr() + lws_offset, lws_bytes=need if lws_bytes is None else lws_bytes)
    status = abi_call.render_normals(sh, nrm.data_ptr(), None, Bn, H, W, outs[0].data_ptr(), outs[1].data_ptr(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, [o.cpu().numpy() for o in outs]


def raw_lookup(B=2, Bn=1, Br=2, H=12, W=12, size=R):
    from drmnet_amd import _lib

    nrm = torch.tensor(np.stack([NORMALS] * 2), device=DEV)
    outs = [torch.full((2, 3, 12, 12), -7.0, device=DEV), torch.full((2, 12, 12), -7.0, device=DEV)]
    status = _lib.lib().drm_image_from_refmap(smooth_refmaps().data_ptr(), None, Br, size, nrm.data_ptr(), None, Bn, outs[0].data_ptr(), outs[1].data_ptr(),
                                              B, H, W, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, [o.cpu().numpy() for o in outs]


def test_bad_arguments_launch_nothing():
    from drmnet_amd import _lib

    lib = _lib.lib()
    need = int(lib.drm_render_light_workspace_bytes(3, 16, 32, M))
    for over in (dict(), dict(Bn=3), dict(light_samples=M), dict(light_samples=M, lws_bytes=need), dict(light_samples=0, lws=None, lws_bytes=0),
                 dict(env=False, light_samples=M, lws=None, lws_bytes=0)):
        ok, outs = raw_normals(**over)
        assert ok == 0 and all(not np.any(o == -7.0) for o in outs), over
    assert np.array_equal(raw_normals(light_samples=M)[1][0], gpu_shade(NORMALS, None, ROWS, [HOT] * 3, None, light_samples=M)[0])
    assert np.array_equal(raw_normals()[1][0], gpu_shade(NORMALS, None, ROWS, [HOT] * 3, None)[0])
    INVALID = 1
    cases = [dict(Bn=2), dict(Bn=0), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(B=0), dict(B=65536), dict(quad=0), dict(quad=1025), dict(EH=0),
             dict(light_samples=-64), dict(light_samples=-64, env=False)]
    cases += [dict(light_samples=m) for m in (100, 32, 1 << 17)]
    cases += [dict(light_samples=M, lws_bytes=need - 8), dict(light_samples=M, lws_bytes=0), dict(light_samples=M, lws=None), dict(light_samples=M, lws_offset=4)]
    for over in cases:
        status, outs = raw_normals(**over)
        assert status == INVALID and lib.drm_last_error(), (over, status)
        assert all(np.all(o == -7.0) for o in outs), over
    ok, outs = raw_lookup()
    assert ok == 0 and all(not np.any(o == -7.0) for o in outs)
    assert raw_lookup(Br=1)[0] == 0 and raw_lookup(Bn=2)[0] == 0
    for over in (dict(Bn=3), dict(Br=3), dict(Br=0), dict(H=0), dict(W=4097), dict(B=0), dict(B=65536), dict(size=0), dict(size=8193)):
        status, outs = raw_lookup(**over)
        assert status == INVALID and lib.drm_last_error(), (over, status)
        assert all(np.all(o == -7.0) for o in outs), over


# ---------------------------------------------------------------------------------------------- 7. plumbing
def test_rerender_is_render_normals_under_the_warped_map():
    from drmnet_amd.relight import render_normals, rerender
    from test_gpu_render import tiny_drmnet

    m = tiny_drmnet(16)
    Lr0 = smooth_refmaps()[0] + 0.1
    zK = torch.tensor(ROUGH, device=DEV)
    nrm, mask = torch.tensor(NORMALS, device=DEV), torch.tensor(MASK, device=DEV)
    image, alpha = rerender(m, Lr0, zK, nrm, mask, quad=Q)
    env = m.r0toenvmap(Lr0[None], (16, 32))
    want = render_normals(nrm, zK[None], NAMES6, env, mask=mask, quad=Q)
    assert image.shape == (1, 3, 12, 12) and torch.equal(image, want[0]) and torch.equal(alpha, want[1]) and float(image.max()) > 0.1
    other = rerender(m, Lr0, zK, nrm, mask, envshape=(8, 16), quad=Q, light_samples=M)[0]
    assert torch.equal(other, render_normals(nrm, zK[None], NAMES6, m.r0toenvmap(Lr0[None], (8, 16)), mask=mask, quad=Q, light_samples=M)[0])
    assert not torch.equal(other, image)


def test_the_relight_command_line_closes_the_loop_on_synthesized_files(tmp_path):
    import mesh_ref as mr
    from drmnet_amd import file_io, relight, synthesize

    torch.save(dict(as_obj(*mr.icosphere(3))), tmp_path / "sphere.pt")
    file_io.save_exr(tmp_path / "env.exr", ENV.astype(np.float32))
    scene = ["--envmap", str(tmp_path / "env.exr"), "--z", *[str(v) for v in ROUGH], "--view_from", *[str(v) for v in VIEW], "--quad", str(Q)]
    synthesize.main(["--mesh", str(tmp_path / "sphere.pt"), "--image_size", "32", "--refmap_res", "8", "--output_dir", str(tmp_path / "in"), *scene])
    out = tmp_path / "out"
    relight.main(["--input_normal", str(tmp_path / "in" / "normal.npy"), "--input_mask", str(tmp_path / "in" / "mask.png"), "--input_img",
                  str(tmp_path / "in" / "image.exr"), "--output_dir", str(out), *scene])
    normal = torch.from_numpy(np.load(tmp_path / "in" / "normal.npy")).to(DEV)
    mask = torch.linalg.norm(normal, dim=-1) > 0.5
    want, _ = relight.render_normals(normal, torch.tensor([ROUGH], device=DEV), synthesize.NAMES, torch.tensor(ENV, dtype=torch.float32, device=DEV)[None],
                                     mask=mask, view_from=torch.tensor([VIEW]), quad=Q)
    assert np.array_equal(file_io.load_exr(out / "image.exr"), want[0].permute(1, 2, 0).cpu().numpy())
    from PIL import Image

    png = np.asarray(Image.open(out / "image.png"))
    assert png.shape == (32, 32, 4) and np.array_equal(png[..., 3] == 255, mask.cpu().numpy()) and 0.55 < float(mask.float().mean()) < 0.7
    errors = json.loads((out / "errors.json").read_text())
    print("closed loop, icosphere(3) at 32 x 32 through synthesize and relight:", errors)
    assert errors == relight.image_errors(want[0].permute(1, 2, 0), file_io.load_exr(tmp_path / "in" / "image.exr"), mask)
    assert errors["n"] == int(mask.sum()) and np.isfinite(errors["rel_l2"]) and np.isfinite(errors["rel_l2_scaled"])
    # without --input_img there is no errors.json; relit under another map and BRDF the image moves
    relight.main(["--input_normal", str(tmp_path / "in" / "normal.npy"), "--z", "1.0", "0.9", "0.6", "0.3", "0.3", "1.0", "--quad", str(Q), "--output_dir",
                  str(tmp_path / "white")])
    assert not (tmp_path / "white" / "errors.json").exists()
    assert rel_l2(file_io.load_exr(tmp_path / "white" / "image.exr"), file_io.load_exr(out / "image.exr")) > 1e-2


def test_estimate_rerender_adds_its_files_and_leaves_the_others_alone(tmp_path):
    from drmnet_amd import estimate, file_io
    from test_gpu_estimate import tiny_models

    g = gold("estimate_chain")
    models = tiny_models(g, DEV)
    for m in models:
        m.set_precision("fp32")
    d = os.path.join(GOLD, "sample")
    argv = ["--input_img", os.path.join(d, "image.exr"), "--input_normal", os.path.join(d, "normal.npy"), "--input_mask", os.path.join(d, "mask.png")]
    old, new = ("sample_env.png", "sample_brdf.png", "sample_brdf.npy"), ("sample_rerender.exr", "sample_rerender.png", "sample_refmap_image.exr",
                                                                         "sample_errors.json")
    for name, flags in (("plain", []), ("rerender", ["--rerender"])):
        hooks = {k: torch.from_numpy(g[s]).to(DEV) for k, s in (("cond_noise", "cond"), ("x_T", "x_T"), ("noise", "noise"), ("noise0", "noise0"),
                                                                ("step_noise", "step_noise"))}
        estimate.main(argv + ["--output_dir", str(tmp_path / name)] + flags, models=models, hooks=hooks)
        assert all((tmp_path / name / f).exists() for f in old)
        assert all((tmp_path / name / f).exists() == bool(flags) for f in new)
    for f in old:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "rerender" / f).read_bytes(), f
    errors = json.loads((tmp_path / "rerender" / "sample_errors.json").read_text())
    print("estimate --rerender on the tiny networks:", errors)
    image = file_io.load_exr(os.path.join(d, "image.exr"))
    assert set(errors) == {"estimate", "inpainted_refmap"} and all(e["n"] > 100 and e["n"] == errors["estimate"]["n"] for e in errors.values())
    assert file_io.load_exr(tmp_path / "rerender" / "sample_rerender.exr").shape == image.shape
    assert file_io.load_exr(tmp_path / "rerender" / "sample_refmap_image.exr").shape == image.shape

"""The sphere / envmap warps of csrc/sphere_warp.hip (drm_envmap2mirmap / drm_rotate_envmap / drm_mirimg2envmap / drm_refmap2refimg) behind
drmnet_amd.transform, the ground-truth maps of drmnet_amd.groundtruth built on them, and ``estimate --gt_envmap``: against the reference's
own outputs (tests/golden/warps.npz), against the float64 restatement tests/warp_ref.py where there is no golden, and against closed forms
that involve neither."""
import json
import os

import numpy as np
import pytest
import torch

import warp_ref as wr
from conftest import GOLD, gold, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# the project's stated tolerance for this arithmetic chain: device trig (an ulp or two from the host's), scaled by W / 2 texels, then
# grid_sample on white noise (tests/test_gpu_transforms.py)
WARP_TOL = 1e-5
VIEWS = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.6, 0.3, 0.742))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def texel_directions(H, W):
    """the direction of every texel of a lat-long map in mirmap2envmap's convention (zenith +y, left edge -z, azimuth reversed) [H, W, 3]"""
    theta, phi = np.meshgrid((np.arange(H) + 0.5) * (np.pi / H), -(np.arange(W) + 0.5) * (2 * np.pi / W), indexing="ij")
    return np.stack([-np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=-1)


def test_all_four_entries_match_the_reference():
    from drmnet_amd import transform

    worst = {}
    for case, x, kw, want, mask in wr.golden_cases(gold("warps")):
        got = getattr(transform, case["fn"])(T(x), **kw)
        if isinstance(got, tuple):
            assert got[1].dtype == torch.bool and np.array_equal(got[1].cpu().numpy(), mask)
            got = got[0]
        err = rel_l2(got.cpu(), want)
        print(f"{case['out']}: rel-L2 {err:.2e}")
        worst[case["fn"]] = max(worst.get(case["fn"], 0.0), err)
        assert tuple(got.shape) == want.shape and err < WARP_TOL, (case, err)
    print("worst rel-L2 per entry:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert len(worst) == 4


@pytest.mark.parametrize("shape, hw", [((10, 10), (32, 64)), ((4, 4), (32, 64)), ((48, 48), (32, 64))])  # uneven windows, 8 x 8 windows (the wave form), no pool
def test_a_batch_equals_its_items_bit_for_bit(shape, hw):
    from drmnet_amd.transform import envmap2mirmap, mirimg2envmap, rotate_envmap

    g = torch.Generator().manual_seed(4)
    env = torch.exp(0.5 * torch.randn((3, 3) + hw, generator=g)).to(DEV)
    views = torch.nn.functional.normalize(torch.tensor(VIEWS), dim=-1)
    for kw in ({}, {"log_scale_interpolation": True}):
        batched = envmap2mirmap(env, shape, view_from=views, **kw)
        for i in range(3):
            assert torch.equal(batched[i:i + 1], envmap2mirmap(env[i:i + 1].contiguous(), shape, view_from=views[i], **kw)), (i, kw)
        assert torch.equal(batched, envmap2mirmap(env.permute(0, 2, 3, 1).contiguous(), shape, view_from=views, channels_last=True, **kw))
        assert not torch.equal(batched[0], envmap2mirmap(env[:1].contiguous(), shape, view_from=views[1], **kw)[0])  # (the view matters)
    # the other warps with per-item frames
    up = torch.nn.functional.normalize(torch.linalg.cross(torch.linalg.cross(views[2], torch.tensor([0.0, 1.0, 0.0])), views[2]), dim=-1)
    zen, left = torch.stack([torch.tensor([0.0, 1.0, 0.0])] * 2 + [up]), torch.stack([torch.tensor([0.0, 0.0, -1.0]), -views[1], -views[2]])
    rot = rotate_envmap(env, tgt_envmap_zenith=zen, tgt_envmap_left_edge=left, out_shape=shape)
    img = mirimg2envmap(env, shape, view_from=views)
    for i in range(3):
        one = env[i:i + 1].contiguous()
        assert torch.equal(rot[i:i + 1], rotate_envmap(one, tgt_envmap_zenith=zen[i], tgt_envmap_left_edge=left[i], out_shape=shape))
        assert torch.equal(img[i:i + 1], mirimg2envmap(one, shape, view_from=views[i]))
    nhwc = env.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(rot, rotate_envmap(nhwc, tgt_envmap_zenith=zen, tgt_envmap_left_edge=left, out_shape=shape, channels_last=True))
    assert torch.equal(img, mirimg2envmap(nhwc, shape, view_from=views, channels_last=True))
    assert tuple(rotate_envmap(env[:1].contiguous(), tgt_envmap_zenith=zen[0], tgt_envmap_left_edge=left[0]).shape) == (1, 3) + hw  # (out_shape defaults to the input's)


def test_the_wave_form_at_a_real_pool_ratio():
    """256 x 512 -> (32, 32): S = 256, every window 8 x 8 = 64 samples, so one wave gathers and reduces each output pixel.  The map is a smooth
    function of direction (continuous across the azimuth seam), so the position error of the device's trig does not dominate."""
    from drmnet_amd.transform import envmap2mirmap

    d = texel_directions(256, 512)
    base = 1.0 + d @ np.array([0.3, -0.2, 0.35]) + 0.3 * (d @ np.array([0.5, 0.5, -0.7])) ** 2
    env = np.stack([np.stack([base, 0.5 * base + 0.2, base**2]), np.stack([base**2, base, 2.0 * base])]).astype(np.float32)  # [2, 3, 256, 512]
    views = np.asarray(torch.nn.functional.normalize(torch.tensor(VIEWS[1:]), dim=-1))
    for kw in ({}, {"log_scale_interpolation": True}):
        got = envmap2mirmap(T(env), (32, 32), view_from=torch.from_numpy(views), **kw)
        again = envmap2mirmap(T(env), (32, 32), view_from=torch.from_numpy(views), **kw)
        err = rel_l2(got.cpu(), wr.envmap2mirmap(env, (32, 32), view_from=views, **kw))
        print(f"wave form, 256 x 512 -> 32 x 32 {kw}: rel-L2 {err:.2e}")
        assert torch.equal(got, again)
        assert err < WARP_TOL


@pytest.mark.parametrize("view", VIEWS)
def test_ground_truth_maps_against_closed_forms(view):
    """No reference involved: under the map 1 + d . a the mirror map is 1 + reflect(back, n) . a and the camera-frame map 1 + (R d) . a.
    The bar is 0.03 (the bilinear error at the unwrapped seam is below 0.01; a mirrored or transposed convention gives 0.1 or more)."""
    from drmnet_amd.groundtruth import gt_camera_envmap, gt_mirror_map
    from drmnet_amd.render import view_rotation

    a = np.array([0.3, -0.2, 0.35])
    H, W, res = 64, 128, 16
    env = T(np.repeat((1.0 + texel_directions(H, W) @ a)[..., None], 3, axis=-1).astype(np.float32))  # [H, W, 3]
    R = view_rotation(view)[0].double().numpy()  # columns (right, up', back)
    back = R[:, 2]
    theta, phi = np.meshgrid((np.arange(res) + 0.5) * (np.pi / res), (np.arange(res) - (res - 1) / 2) * (np.pi / res), indexing="ij")
    n = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), np.sin(theta) * np.cos(phi)], axis=-1) @ R.T  # camera frame -> world
    reflected = 2 * (n @ back)[..., None] * n - back
    mirror = gt_mirror_map(env, view, res)
    assert tuple(mirror.shape) == (1, 3, res, res)
    e_mir = float(np.abs(mirror[0].cpu().double().numpy() - (1.0 + reflected @ a)[None]).max())
    camera = gt_camera_envmap(env, view, (H, W))
    assert tuple(camera.shape) == (1, H, W, 3)
    e_env = float(np.abs(camera[0].cpu().double().numpy() - (1.0 + (texel_directions(H, W) @ R.T) @ a)[..., None]).max())
    print(f"view {view}: max abs error, mirror map {e_mir:.2e}, camera-frame envmap {e_env:.2e}")
    assert e_mir < 0.03 and e_env < 0.03
    # and the two agree with each other: the rotated map seen from +z is the world map seen from `view`
    from drmnet_amd.transform import envmap2mirmap

    seen = envmap2mirmap(camera, (res, res), view_from=[0.0, 0.0, 1.0], channels_last=True)
    assert float((seen - mirror).abs().max()) < 0.03


def test_refmap2refimg_draws_the_disc_and_nothing_else():
    from drmnet_amd.transform import refmap2refimg_torch

    g = gold("warps")
    refmap = T(g["refmap"])
    for radius, res in ((None, 32), (12, 24), (5, 10)):
        img, mask = refmap2refimg_torch(refmap, radius=radius, return_mask=True)
        want, disc = wr.refmap2refimg(g["refmap"], radius)
        assert tuple(img.shape) == (2, 3, res, res) and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), disc)
        assert bool((img[:, :, ~mask] == 0).all()) and bool((img[:, :, mask] > 0).all()) and 0.7 < float(mask.float().mean()) < 0.85
        assert rel_l2(img.cpu(), want) < WARP_TOL
    assert np.array_equal(refmap2refimg_torch(refmap, return_mask=True)[1].cpu().numpy(), g["refmap2refimg_torch_25_mask"])
    one = refmap2refimg_torch(refmap[0], radius=12)  # a 3-D input comes back 3-D
    assert tuple(one.shape) == (3, 24, 24) and torch.equal(one, refmap2refimg_torch(refmap, radius=12)[0])
    assert torch.equal(refmap2refimg_torch(refmap.permute(0, 2, 3, 1).contiguous(), channels_last=True), refmap2refimg_torch(refmap))


def test_bad_arguments_launch_nothing():
    from drmnet_amd import _lib
    from drmnet_amd.transform import envmap2mirmap, envmap2mirmap_frames

    lib = _lib.lib()
    env = torch.ones((1, 3, 8, 16), device=DEV)
    frames = envmap2mirmap_frames(1).to(DEV)
    out = torch.full((1, 3, 4, 4), -1.0, device=DEV)
    s = _lib.stream_ptr(DEV)
    ok = dict(env=env.data_ptr(), frames=frames.data_ptr(), out=out.data_ptr(), B=1, C=3, H=8, W=16, OH=4, OW=4)

    def e2m(**kw):
        a = {**ok, **kw}
        return lib.drm_envmap2mirmap(a["env"], a["frames"], a["out"], a["B"], a["C"], a["H"], a["W"], a["OH"], a["OW"], 1, 0, 0, s)

    for bad in (dict(env=None), dict(frames=None), dict(out=None), dict(B=0), dict(C=0), dict(H=0), dict(OW=0), dict(W=16385), dict(OH=-1)):
        assert e2m(**bad) == 1 and b"envmap2mirmap" in lib.drm_last_error(), bad  # DRM_ERR_INVALID
    assert lib.drm_rotate_envmap(None, frames.data_ptr(), out.data_ptr(), 1, 3, 8, 16, 4, 4, 0, s) == 1
    assert lib.drm_mirimg2envmap(env.data_ptr(), None, out.data_ptr(), 1, 3, 8, 16, 4, 4, 0, 0, s) == 1
    assert lib.drm_refmap2refimg(env.data_ptr(), None, None, 1, 3, 8, 16, 2, 0, s) == 1
    assert lib.drm_refmap2refimg(env.data_ptr(), out.data_ptr(), None, 1, 3, 8, 16, 0, 0, s) == 1
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert e2m() == 0  # and the good call draws
    torch.cuda.synchronize()
    assert float((out - 1.0).abs().max()) < 1e-6  # (a map of ones stays ones, to the rounding of the four weights)
    with pytest.raises(RuntimeError):
        envmap2mirmap(env.cpu(), (4, 4))  # GPU only


def test_estimate_gt_envmap_adds_its_files_and_leaves_the_others_alone(tmp_path):
    from drmnet_amd import estimate, file_io
    from test_gpu_estimate import tiny_models

    g = gold("estimate_chain")
    models = tiny_models(g, DEV)
    for m in models:
        m.set_precision("fp32")
    d = os.path.join(GOLD, "sample")
    d64 = texel_directions(16, 32)
    file_io.save_exr(tmp_path / "env.exr", np.stack([1.0 + d64 @ np.array([0.3, -0.2, 0.35]), 0.8 + 0.5 * d64[..., 1], 1.2 - 0.4 * d64[..., 0]], axis=-1).astype(np.float32))
    argv = ["--input_img", os.path.join(d, "image.exr"), "--input_normal", os.path.join(d, "normal.npy"), "--input_mask", os.path.join(d, "mask.png")]
    old = ("sample_env.png", "sample_brdf.png", "sample_brdf.npy")
    new = ("sample_gt_mirmap.exr", "sample_gt_env.exr", "sample_Lr0.exr", "sample_gt_errors.json")
    for name, flags in (("plain", []), ("gt", ["--gt_envmap", str(tmp_path / "env.exr"), "--gt_view_from", "0.6", "0.3", "1.0"])):
        hooks = {k: torch.from_numpy(g[s]).to(DEV) for k, s in (("cond_noise", "cond"), ("x_T", "x_T"), ("noise", "noise"), ("noise0", "noise0"),
                                                                ("step_noise", "step_noise"))}
        estimate.main(argv + ["--output_dir", str(tmp_path / name)] + flags, models=models, hooks=hooks)
        assert all((tmp_path / name / f).exists() for f in old)
        assert all((tmp_path / name / f).exists() == bool(flags) for f in new)
    for f in old:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "gt" / f).read_bytes(), f
    errors = json.loads((tmp_path / "gt" / "sample_gt_errors.json").read_text())
    print("estimate --gt_envmap on the tiny networks:", errors)
    assert set(errors) == {"mirror_map", "envmap"}
    assert all(np.isfinite(v) for e in errors.values() for v in e.values())
    S, R = models[0].image_size, file_io.load_exr(tmp_path / "gt" / "sample_Lr0.exr").shape[0]
    assert errors["mirror_map"]["n"] == R * R and errors["envmap"]["n"] == S * 2 * S
    assert file_io.load_exr(tmp_path / "gt" / "sample_gt_mirmap.exr").shape == file_io.load_exr(tmp_path / "gt" / "sample_Lr0.exr").shape == (R, R, 3)
    assert file_io.load_exr(tmp_path / "gt" / "sample_gt_env.exr").shape == (S, 2 * S, 3)
    with pytest.raises(SystemExit):
        estimate.main(argv + ["--output_dir", str(tmp_path / "half"), "--gt_envmap", str(tmp_path / "env.exr")], models=models)
    assert not (tmp_path / "half").exists()

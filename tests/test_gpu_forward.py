"""The forward process and the validation losses on the GPU: per-row views and stacked rows of the renderer (csrc/render.hip) against the
float64 restatement tests/render_ref.py, the loss reduction (csrc/losses.hip) against tests/forward_ref.py, and DRMNet.get_input / p_losses /
validation_step / drmnet_amd.validate against the reference's recorded run (tests/golden/forward_losses.npz, tools/make_golden_forward.py)."""
import json
import math

import numpy as np
import pytest
import torch

import forward_ref as fr
import render_ref as rr
from conftest import ACCURATE_MODES, GOLD, NET_TOL, gold, rel_l2
from test_forward_cpu import ENC_T, NAMES6, UNET_T, tiny_drmnet, write_datalist
from test_gpu_render import smooth_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def lit_env(EH, EW, seed=0):
    """smooth, with a sharp-edged light off to one side: nothing about it repeats along the azimuth"""
    env = smooth_env(EH, EW, seed)
    d = rr.env_dirs(EH, EW)[0]
    return env + 4.0 * ((d[..., 0:1] > 0.6) & (d[..., 1:2] > 0.2))


def t32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ renderer: views and stacked rows
Z_ROWS = [[0.0, 0.8, 0.5, 0.2, 0.3, 0.5], [1.0, 0.9, 0.6, 0.3, 0.05, 1.0], [0.4, 0.2, 0.7, 0.9, 0.8, 0.2]]


@pytest.mark.parametrize("flip", [False, True])
def test_view_on_the_horizontal_circle_is_a_roll_of_the_map(flip):
    """view_from = (sin phi, 0, cos phi), phi = n 2 pi / EW: the environment is looked up at Rot l, whose azimuth is that of l minus phi --
    the +z render of np.roll(env, +n, axis=1).  Bar: the 1e-5 the +z renders meet against the same restatement."""
    from drmnet_amd.render import render

    EH, EW, R = 32, 64, 32
    env = lit_env(EH, EW)
    shifts = [23, 5, 50]  # (the near-mirror row gets the smallest turn)
    phi = [n * 2 * math.pi / EW for n in shifts]
    views = torch.tensor([[math.sin(p), 0.0, math.cos(p)] for p in phi]) * torch.tensor([[1.1], [0.7], [3.0]])  # (the distance does not matter)
    out = render(t32(Z_ROWS), NAMES6, t32(env)[None].expand(3, -1, -1, -1), res=R, flip=flip, view_from=views).cpu().numpy()
    for b, n in enumerate(shifts):
        want = rr.render_quadrature(Z_ROWS[b], np.roll(env, n, axis=1), R, flip=flip)
        err = rel_l2(out[b], want)
        print(f"flip {flip} shift {n}: rel_l2 {err:.3e}")
        assert err <= 1e-5, (n, err)
        assert rel_l2(out[b], rr.render_quadrature(Z_ROWS[b], np.roll(env, -n, axis=1), R, flip=flip)) > 1e-2  # (the sign matters)


def test_view_off_the_horizontal_circle_is_no_roll():
    from drmnet_amd.render import render

    EH, EW, R = 32, 64, 32
    env = lit_env(EH, EW)
    z = t32(Z_ROWS[2:3])
    tilted = render(z, NAMES6, t32(env)[None], res=R, view_from=torch.tensor([[0.5, 0.6, 0.7]])).cpu()
    rolls = t32(np.stack([np.roll(env, n, axis=1) for n in range(EW)]))
    flat = render(z.expand(EW, -1), NAMES6, rolls, res=R).cpu()
    errs = [rel_l2(tilted[0], flat[n]) for n in range(EW)]
    assert min(errs) > 1e-2, min(errs)
    assert torch.isfinite(tilted).all()


def test_stacked_rows_equal_single_rows_bit_for_bit():
    import abi_call
    from drmnet_amd import _lib
    from drmnet_amd.render import RefMapRenderer, render, view_rotation

    L, B, R = 3, 4, 16
    g = torch.Generator().manual_seed(5)
    z = torch.rand((L, B, 6), generator=g)
    env = t32(np.stack([lit_env(16, 32, s) for s in range(B)])).to(DEV)
    views = torch.tensor([[0.3, 0.0, 0.9], [0.0, 0.0, 1.1], [-0.8, 0.2, -0.4], [0.1, -0.7, 0.5]])
    stacked = render(z, NAMES6, env, res=R, view_from=views)
    assert stacked.shape == (L, B, 3, R, R)
    for l in range(L):
        for b in range(B):
            one = render(z[l, b][None], NAMES6, env[b][None], res=R, view_from=views[b][None])
            assert torch.equal(stacked[l, b], one[0]), (l, b)
    # no view == the view from +z == identity matrices handed to the kernel, bit for bit; and L = 1 without a view
    plain = render(z, NAMES6, env, res=R)
    assert torch.equal(plain, render(z, NAMES6, env, res=R, view_from=torch.tensor([[0.0, 0.0, 1.1]] * B)))
    assert torch.equal(plain[1], render(z[1], NAMES6, env, res=R))
    eye = torch.eye(3, device=DEV)[None].expand(B, 3, 3).contiguous()
    rows = z.reshape(-1, 6).to(DEV).contiguous()
    out = torch.empty((L, B, 3, R, R), device=DEV)
    sh = abi_call.shading(B, z=rows.data_ptr(), env=env.data_ptr(), EH=16, EW=32, view=eye.data_ptr(), quad=32)
    _lib.check(abi_call.render_refmap(sh, L, R, 2, 0, out.data_ptr(), _lib.stream_ptr(DEV)))
    assert torch.equal(out, plain)
    old = torch.empty((B, 3, R, R), device=DEV)
    sh = abi_call.shading(B, z=rows.data_ptr(), env=env.data_ptr(), EH=16, EW=32, quad=32)  # (one set of rows, no view)
    _lib.check(abi_call.render_refmap(sh, 1, R, 2, 0, old.data_ptr(), _lib.stream_ptr(DEV)))
    assert torch.equal(old, plain[0])
    assert not torch.equal(stacked[:, 0], plain[:, 0]) and torch.equal(stacked[:, 1], plain[:, 1])  # (views[1] is +z)
    # the scene object keeps the view it was given, like the map
    r = RefMapRenderer(R, brdf_param_names=NAMES6)
    a = r.rendering(z[0, 0], NAMES6, env[0], view_from=views[0], channel_first=True)
    assert torch.equal(a, stacked[0, 0]) and torch.equal(r.rendering(z[0, 0], NAMES6, channel_first=True), a)
    assert torch.equal(view_rotation(views[1]), torch.eye(3)[None])


def test_rendering_refmaps_does_not_copy_the_maps():
    m = tiny_drmnet().to(DEV)
    L, B = 4, 2
    env = torch.rand((B, 512, 1024, 3), device=DEV) + 0.1
    z = torch.rand((L, B, 6), device=DEV)
    views = torch.tensor([[0.6, 0.0, 0.8], [-1.0, 0.0, 0.2]])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m.rendering_refmaps(env, z, view_from=views)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert out.shape == (L, B, 3, 16, 16) and torch.isfinite(out).all()
    assert rise < env.numel() * 4, (rise, env.numel() * 4)
    for l in range(L):  # every row of an item under that item's map and view
        assert torch.equal(out[l], m.renderer.render(z[l], NAMES6, env, view_from=views))


# ------------------------------------------------------------------------------------------------ the loss reduction
def random_loss_inputs(B, shape, seed, masked):
    g = np.random.default_rng(seed)
    maps = [g.normal(size=(B,) + shape).astype(np.float32) for _ in range(3)]
    codes = [g.uniform(-0.3, 1.3, size=(B, 6)).astype(np.float32) for _ in range(3)]
    K = g.integers(1, 120, size=B).astype(np.int32)
    K[list(masked)] = 0
    rk = g.integers(0, 100, size=B).astype(np.int32)
    z0 = np.array([1, 1, 1, 1, 0, 1], dtype=np.float32)
    return maps, K, codes, rk, z0


def gpu_losses(maps, K, codes, rk, z0, gamma, loss_type, w1, w2):
    from drmnet_amd import ops

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return ops.validation_losses(d(maps[0]), d(maps[1]), d(maps[2]), d(K), d(codes[0]), d(codes[1]), d(codes[2]), d(rk), d(z0), gamma, loss_type, w1, w2)


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 128, 128)])
@pytest.mark.parametrize("B", [1, 6, 32])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_losses_match_the_restatement(loss_type, B, shape):
    """fp64 arithmetic on both sides: what is left is the fp32 rounding of the three outputs (6e-8 each) -> rtol 1e-6"""
    masked = [] if B == 1 else [1, B - 1]
    maps, K, codes, rk, z0 = random_loss_inputs(B, shape, 100 + B, masked)
    for row in masked:  # what the dataset writes into a row with K == 0
        maps[2][row] = np.nan
    want = fr.validation_losses(*maps, K, *codes, rk, z0, 0.95, loss_type, 10.0, 0.1)
    got = gpu_losses(maps, K, codes, rk, z0, 0.95, loss_type, 10.0, 0.1)
    assert got.dtype == torch.float32 and got.shape == (3,) and torch.isfinite(got).all()
    print(f"{loss_type} B={B} {shape}: rel err {np.abs(got.cpu().numpy() / want - 1).max():.2e}")
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6)
    assert torch.equal(got, gpu_losses(maps, K, codes, rk, z0, 0.95, loss_type, 10.0, 0.1))  # fixed summation order: bitwise repeatable


def test_losses_masked_rows_and_the_empty_selection():
    maps, K, codes, rk, z0 = random_loss_inputs(6, (3, 16, 16), 9, [0, 3])
    base = gpu_losses(maps, K, codes, rk, z0, 0.9, "l2", 10.0, 0.1)
    for t in maps:  # NaN everywhere in the masked rows, in all three maps
        t[[0, 3]] = np.nan
    poisoned = gpu_losses(maps, K, codes, rk, z0, 0.9, "l2", 10.0, 0.1)
    assert torch.isfinite(poisoned).all() and torch.equal(poisoned, base)
    none = gpu_losses(maps, np.zeros(6, dtype=np.int32), codes, rk, z0, 0.9, "l1", 10.0, 0.1).cpu()
    assert torch.isnan(none[0]) and torch.isfinite(none[1]) and torch.isnan(none[2])
    with pytest.raises(NotImplementedError):
        gpu_losses(maps, K, codes, rk, z0, 0.9, "huber", 1.0, 1.0)


# ------------------------------------------------------------------------------------------------ DRMNet surface
def fixture_model(g, **kw):
    """the tiny DRMNet the fixture's reference run used: same constants, same seeded synthetic weights"""
    from drmnet_amd import synth
    from drmnet_amd.dataset import BaseDataset

    m = tiny_drmnet(gamma=float(g["gamma"]), epsilon=float(g["epsilon"]), z0=g["z0"].tolist(), sigma=float(g["sigma"]),
                    refmap_input_scaler=float(g["refmap_input_scaler"]), l_refmap_weight=float(g["l_refmap_weight"]),
                    l_refcode_weight=float(g["l_refcode_weight"]), loss_type="l2", **kw)
    synth.load_synth(m.illnet_model.diffusion_model, 21)
    synth.load_synth(m.refnet_model.diffusion_model, 22)
    zman = [(k, tuple(v.shape)) for k, v in m.illnet_model.z_emb_layer.state_dict().items()]
    m.illnet_model.z_emb_layer.load_state_dict(synth.synth_state_dict(zman, synth.SEED_ZEMB))
    m.ds = BaseDataset(16, "log", clamp_before_exp=20)
    return m.to(DEV)


def fixture_batch(g):
    batch = {k: torch.from_numpy(g[k]) for k in ("zK", "K", "k", "zk", "zkm1", "LrK", "Lrk", "Lrkm1", "view_from", "envmap")}
    batch["envmap_name"] = [f"env{i}" for i in range(len(g["zK"]))]
    return batch


def test_get_input_on_the_cached_batch_matches_the_reference():
    g = gold("forward_losses")
    m = fixture_model(g)
    K, k, Lr_K, Lr_k, Lr_km1, zK, zk, illnet_c, refnet_c = m.get_input(fixture_batch(g))
    assert m.batch_size == 6 and illnet_c is refnet_c and illnet_c[0] is Lr_K
    for got, key in ((K, "out_K"), (k, "out_k"), (zK, "out_zK"), (zk, "out_zk")):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), g[key]) and got.cpu().numpy().dtype == g[key].dtype, key
    # the bars test_gpu_transforms.py holds get_input_for_predict to
    for got, key in ((Lr_K, "out_Lr_K"), (Lr_k, "out_Lr_k"), (Lr_km1, "out_Lr_km1")):
        np.testing.assert_allclose(got.cpu().numpy(), g[key], rtol=1e-5, atol=2e-6, equal_nan=True, err_msg=key)
    np.testing.assert_allclose(m.normalizing_scale.cpu().numpy(), g["normalizing_scale"], rtol=2e-6)
    masked = g["out_K"] == 0
    assert torch.isnan(Lr_km1[torch.from_numpy(masked)]).all() and torch.isfinite(Lr_km1[torch.from_numpy(~masked)]).all()
    short = m.get_input(fixture_batch(g), bs=4)
    assert m.batch_size == 4 and short[2].shape[0] == 4 and torch.equal(short[2], Lr_K[:4])


def test_get_input_renders_what_the_batch_does_not_bring(tmp_path):
    from drmnet_amd import file_io, ops
    from drmnet_amd.render import render

    g = gold("forward_losses")
    m = fixture_model(g, envmap_dir=str(tmp_path))
    batch = fixture_batch(g)
    B = 5
    batch = {k: (v[:B].clone() if isinstance(v, torch.Tensor) else v[:B]) for k, v in batch.items() if k not in ("Lrk", "Lrkm1")}
    batch["view_from"][1] = torch.tensor([0.2, 0.5, -0.8])  # one view off the circle
    batch["LrK"][1:, 0, 0, 0] = float("nan")  # item 0 brings its LrK; the others are marked "not cached"
    file_io.save_exr(tmp_path / "env3.exr", batch["envmap"][3].numpy())  # item 3's map is marked missing and comes from envmap_dir
    env = batch["envmap"].clone()
    env[3] = file_io.load_exr(tmp_path / "env3.exr", as_torch=True)
    batch["envmap"][3, 0, 0, 0] = float("nan")
    out = m.get_input(batch, return_Lr_zero=True, return_envmap=True, return_envmap_name=True, return_view_from=True)
    assert len(out) == 13
    K, k, Lr_K, Lr_k, Lr_km1, zK, zk, illnet_c, refnet_c, Lr_0, envmap, names, view_from = out
    assert names == [f"env{i}" for i in range(B)] and torch.equal(view_from, batch["view_from"]) and torch.equal(envmap.cpu(), env)
    # by hand: one render of the stack, the exposure scale of LrK, the dataset's transform
    stack = torch.stack([batch["zK"], batch["zk"], batch["zkm1"], torch.from_numpy(g["z0"])[None].expand(B, -1)])
    rendered = render(stack, NAMES6, env.to(DEV), res=16, view_from=batch["view_from"])
    rendered[2, 2] = float("nan")  # zkm1 of the K == 0 row is NaN: no map
    LrK_hdr = rendered[0].clone()
    LrK_hdr[0] = torch.from_numpy(g["LrK"][0]).to(DEV)  # the cached item is not overwritten
    scale = ops.luminance_scale(LrK_hdr, 0.12)
    hand = lambda x: m.ds.transform(ops.map_chain(x.contiguous(), [("img_mul", 0.0)], scale=scale))
    assert torch.equal(m.normalizing_scale, scale)
    assert torch.equal(Lr_K, hand(LrK_hdr)) and torch.equal(Lr_k, hand(rendered[1])) and torch.equal(Lr_0, hand(rendered[3]))
    assert torch.equal(Lr_km1.nan_to_num(-7.0), hand(rendered[2]).nan_to_num(-7.0)) and torch.isnan(Lr_km1[2]).all()
    assert rel_l2(Lr_K[0].cpu(), g["out_Lr_K"][0]) <= 1e-5 and rel_l2(Lr_K[1].cpu(), g["out_Lr_K"][1]) > 1e-2
    assert torch.isfinite(Lr_K).all() and torch.isfinite(Lr_k).all() and torch.isfinite(Lr_0).all()
    # without the z0 row the stack is three deep and the rest is unchanged
    plain = m.get_input(batch)
    assert len(plain) == 9 and torch.equal(plain[2], Lr_K) and torch.equal(plain[3], Lr_k)


@pytest.mark.parametrize("mode", ACCURATE_MODES)
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_p_losses_on_the_reference_tensors(loss_type, mode):
    """The reference's network-space tensors and recorded noise through both networks and the loss kernels.  Target: the float64 restatement
    on the REFERENCE's model_out / z_out.  Bars from the network bar rho = NET_TOL[mode] (rms(out - out_ref) <= rho rms(out_ref)):
      l1: |d loss| <= mean |delta| <= rms(delta) <= rho rms(out_ref)
      l2: |d loss| <= 2 rms(pred - target) rms(delta) + rms(delta)^2
    for the refmap loss with model_out and for each code loss with z_out (the clamp and the gamma power are 1-Lipschitz), plus rtol 1e-6 for
    the reduction.  The rms values are the fixture's (float64, selected rows)."""
    g = gold("forward_losses")
    m = fixture_model(g)
    m.validation_params["loss_type"] = loss_type
    m.set_precision(mode)
    d = lambda key: torch.from_numpy(g[key]).to(DEV)
    loss, out = m.p_losses(d("out_Lr_k"), d("out_Lr_km1"), d("out_zk"), d("out_zK"), d("out_K"), d("out_k"), [d("out_Lr_K")], [d("out_Lr_K")],
                           noise=d("noise"))
    assert sorted(out) == ["val/loss", "val/loss_refcode", "val/loss_refmap"] and loss.dim() == 0 and loss.is_cuda
    assert torch.equal(loss, out["val/loss"])
    noised = g["out_Lr_k"] + np.float32(g["sigma"]) * g["noise"]
    w1, w2 = float(g["l_refmap_weight"]), float(g["l_refcode_weight"])
    want = fr.validation_losses(g["model_out"], noised, g["out_Lr_km1"], g["out_K"], g["z_out"], g["out_zk"], g["out_zK"], g["out_K"] - g["out_k"] - 1,
                                g["z0"], float(g["gamma"]), loss_type, w1, w2)
    rho = NET_TOL[mode]
    e_map, e_code = rho * float(g["rms_model_out"]), rho * float(g["rms_z_out"])
    if loss_type == "l1":
        bar_map, bar_code = e_map, e_code
    else:
        bar_map = 2 * float(g["rms_refmap_residual"]) * e_map + e_map**2
        bar_code = 0.5 * sum(2 * float(g[key]) * e_code + e_code**2 for key in ("rms_zk_residual", "rms_zK_residual"))
    bars = np.array([bar_map, bar_code, w1 * bar_map + w2 * bar_code]) + 1e-6 * np.abs(want)
    got = np.array([float(out[key]) for key in ("val/loss_refmap", "val/loss_refcode", "val/loss")])
    print(f"{loss_type} {mode}: |got - want| {np.abs(got - want)} bars {bars} want {want}")
    assert (np.abs(got - want) <= bars).all(), (got, want, bars)
    # Philox noise: keyed by the seed
    a = m.p_losses(d("out_Lr_k"), d("out_Lr_km1"), d("out_zk"), d("out_zK"), d("out_K"), d("out_k"), [d("out_Lr_K")], [d("out_Lr_K")], seed=3)[0]
    b = m.p_losses(d("out_Lr_k"), d("out_Lr_km1"), d("out_zk"), d("out_zK"), d("out_K"), d("out_k"), [d("out_Lr_K")], [d("out_Lr_K")], seed=3)[0]
    c = m.p_losses(d("out_Lr_k"), d("out_Lr_km1"), d("out_zk"), d("out_zK"), d("out_K"), d("out_k"), [d("out_Lr_K")], [d("out_Lr_K")], seed=4)[0]
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(c)


def ema_model_and_batch():
    from drmnet_amd.dataset import BaseDataset

    m = tiny_drmnet(gamma=0.9, epsilon=1e-3, max_timesteps=6, use_ema=True, sigma=0.02, refmap_input_scaler=0.12, loss_type="l2",
                    l_refmap_weight=10.0, l_refcode_weight=0.1)
    m.init_from_ckpt(f"{GOLD}/drmnet_tiny_ema.ckpt", verbose=False)
    m.ds = BaseDataset(16, "log", clamp_before_exp=20)
    m = m.to(DEV).set_precision("f16x3")
    B = 4
    gen = torch.Generator().manual_seed(77)
    zK = torch.rand((B, 6), generator=gen)
    K, k, zk, zkm1 = m.get_schedule(zK, z0=m._z0, normalized_k=torch.rand((B,), generator=gen), return_zkm1=True)
    phi = torch.rand((B,), generator=gen) * 2 * math.pi
    batch = {"zK": zK, "K": K, "k": k, "zk": zk, "zkm1": zkm1, "envmap_name": [f"e{i}" for i in range(B)],
             "view_from": torch.stack([torch.sin(phi), torch.zeros(B), torch.cos(phi)], dim=-1),
             "envmap": t32(np.stack([lit_env(8, 16, s) for s in range(B)]))}
    return m, batch


def test_validation_step_live_and_ema():
    m, batch = ema_model_and_batch()
    out = m.validation_step(batch, 0, seed=11)
    keys = ["val/loss", "val/loss_refcode", "val/loss_refmap"]
    assert sorted(out) == sorted(keys + [k + "_ema" for k in keys])
    assert all(v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)) for v in out.values())
    assert all(not torch.equal(out[k], out[k + "_ema"]) for k in keys)
    again = m.validation_step(batch, 0, seed=11)
    assert all(torch.equal(out[k], again[k]) for k in out)
    other = m.validation_step(batch, 0, seed=12)
    assert not torch.equal(out["val/loss_refmap"], other["val/loss_refmap"])
    assert m._weight_set == "live" and m.batch_size == 4
    loss, d = m.shared_step(batch, seed=11)
    assert torch.equal(loss, out["val/loss"]) and torch.equal(d["val/loss_refcode"], out["val/loss_refcode"])


def test_validate_end_to_end(tmp_path, capsys):
    import yaml

    from drmnet_amd import file_io
    from drmnet_amd import validate as V

    maps = tmp_path / "maps"
    maps.mkdir()
    for i in range(3):
        file_io.save_exr(maps / f"env{i:03d}.exr", lit_env(8, 16, i).astype(np.float32))
    datalist = write_datalist(tmp_path / "envs.txt", 3)
    cfg = {"model": {"target": "models.drmnet.DRMNet", "params": {
               "illnet_config": UNET_T, "refnet_config": ENC_T, "max_timesteps": 8, "image_size": 16, "concat_mode": True, "use_ema": True, "loss_type": "l2",
               "sigma": 0.02, "gamma": 0.95, "epsilon": 0.01, "l_refmap_weight": 10.0, "l_refcode_weight": 0.1, "brdf_param_names": NAMES6,
               "z0": [1, 1, 1, 1, 0, 1], "refmap_input_scaler": 0.12,
               "renderer_config": {"target": "utils.mitsuba3_utils.MitsubaRefMapRenderer", "params": {"refmap_res": 16, "spp": 256, "denoise": "simple"}}}},
           "data": {"target": "main.DataModuleFromConfig", "params": {"batch_size": 2, "validation": {
               "target": "dataset.parametricrefmap.ParametricRefmapDataset",
               "params": {"size": 16, "split": "val", "data_root": str(maps), "transform_func": "log", "zdim": 6, "return_envmap": True,
                          "refmap_cache_root": "./data/cache/refmap/", "datalist": datalist}}}}}
    path = tmp_path / "tiny.yaml"
    path.write_text(yaml.safe_dump(cfg))
    result = V.main(["--base", str(path), "--batch_size", "2", "--precision", "f16x3", "--seed", "5"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    keys = ["val/loss", "val/loss_refcode", "val/loss_refmap"]
    assert sorted(result) == sorted(keys + [k + "_ema" for k in keys] + ["items", "batches"]) and (result["items"], result["batches"]) == (3, 2)
    assert all(math.isfinite(result[k]) for k in keys)
    # the epoch mean weights every batch by its size (3 items in batches of 2 and 1), and --limit cuts the epoch
    from drmnet_amd.config import instantiate_from_config, load_config

    config = load_config(str(path))
    model = instantiate_from_config(config["model"]).to(DEV)
    ds = V.build_dataset(config, V.make_parser().parse_args(["--base", str(path)]))
    full = V.validate(model, ds, 2, precision="f16x3", seed=5)
    sizes = [r["batch_size"] for r in full["per_batch"]]
    assert sizes == [2, 1]
    for key in keys + [k + "_ema" for k in keys]:
        assert full[key] == pytest.approx(sum(r[key] * r["batch_size"] for r in full["per_batch"]) / 3, rel=1e-12)
        assert full[key] != pytest.approx(sum(r[key] for r in full["per_batch"]) / 2, rel=1e-9)
    cut = V.validate(model, ds, 2, limit=2, seed=5)
    assert (cut["items"], cut["batches"]) == (2, 1) and cut["val/loss"] == full["per_batch"][0]["val/loss"]

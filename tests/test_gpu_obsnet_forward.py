"""ObsNet's validation pass on the GPU: the forward-process kernel and the loss reduction (csrc/obs_forward.hip) against the float64
restatement tests/obsnet_forward_ref.py, and ObsNetDiffusion.get_input / p_losses / shared_step / validation_step / drmnet_amd.validate against
the reference's recorded run (tests/golden/obsnet_forward.npz, tools/make_golden_obsnet_forward.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import obsnet_forward_ref as ofr
from conftest import ACCURATE_MODES, GOLD, NET_TOL, gold
from test_forward_cpu import NAMES6, UNET_T, write_datalist
from test_gpu_forward import lit_env, t32
from test_obsnet_forward_cpu import RENDERER_T, TRANSFORM, blob, tiny_obsnet, write_masks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0**-24
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the forward-process kernel
def forward_inputs(shape, seed, T=50):
    r = np.random.default_rng(seed)
    B, C, H, W = shape
    x = r.uniform(-1, 1, size=shape).astype(np.float32)
    mask = (r.uniform(size=(B, 1, H, W)) > 0.7).astype(np.float32)
    t = r.integers(0, T, size=B).astype(np.int32)
    t[0], t[-1] = 0, T - 1
    abar = np.cumprod(1 - np.linspace(1e-2, 0.3, T) ** 2)
    sa, s1 = np.sqrt(abar).astype(np.float32), np.sqrt(1 - abar).astype(np.float32)
    e = [r.normal(size=shape).astype(np.float32) for _ in range(3)]
    return x, mask, t, sa, s1, e


@pytest.mark.parametrize("shape", [(6, 3, 16, 16), (20, 3, 128, 128), (5, 3, 24, 40), (3, 3, 5, 7)])
def test_forward_process_matches_the_restatement(shape):
    """Injected draws.  fp32 arithmetic against float64: cond = mask x + n e1 + (1 - mask) e2 takes three product roundings, two sum roundings
    and one more should a product be contracted into a sum -> 6 2^-24 (|mask x| + |n e1| + |(1 - mask) e2|) per element; x_noisy = a x + s e3
    two products, one sum, one contraction -> 4 2^-24 (|a x| + |s e3|).  The last shape has planes of 35 floats: the unaligned path."""
    from drmnet_amd import ops

    x, mask, t, sa, s1, e = forward_inputs(shape, 7)
    n_obs = 0.04
    want = ofr.forward_process(x, mask, t, sa, s1, n_obs, "noise", *e)
    run = lambda n, pad, **kw: ops.obs_forward_process(d(x), d(mask), d(t), d(sa), d(s1), n, pad, e_observe=d(e[0]), e_padding=d(e[1]), e_q=d(e[2]), **kw)
    cond, x_noisy, noise = run(n_obs, "noise")
    err_c, err_q = np.abs(cond.cpu().numpy() - want[0]), np.abs(x_noisy.cpu().numpy() - want[1])
    print(f"{shape}: cond max err / bar {np.max(err_c / (6 * EPS * want[3] + 1e-300)):.3f}, x_noisy {np.max(err_q / (4 * EPS * want[4] + 1e-300)):.3f}")
    assert (err_c <= 6 * EPS * want[3]).all() and (err_q <= 4 * EPS * want[4]).all()
    assert torch.equal(noise, d(e[2]))  # bit for bit
    # dropped terms drop exactly
    zeros = run(n_obs, "zeros")[0].cpu().numpy()
    w0 = ofr.forward_process(x, mask, t, sa, s1, n_obs, "zeros", *e)
    assert (np.abs(zeros - w0[0]) <= 6 * EPS * w0[3]).all() and np.array_equal(zeros[np.broadcast_to(mask == 0, shape)], (np.float32(n_obs) * e[0])[np.broadcast_to(mask == 0, shape)])
    assert np.array_equal(run(0.0, "zeros")[0].cpu().numpy(), mask * x)
    quiet = run(0.0, "noise")[0].cpu().numpy()
    assert np.array_equal(quiet, mask * x + (1 - mask) * e[1])  # (mask is 0 / 1: one of the two products is an exact zero)
    # the halves of one call
    assert torch.equal(run(n_obs, "noise", want_q=False)[0], cond) and run(n_obs, "noise", want_q=False)[1] is None
    half = run(n_obs, "noise", want_cond=False)
    assert half[0] is None and torch.equal(half[1], x_noisy) and torch.equal(half[2], noise)


def test_forward_process_argument_errors():
    from drmnet_amd import ops

    x, mask, t, sa, s1, e = forward_inputs((2, 3, 8, 8), 1)
    with pytest.raises(RuntimeError, match="size of x"):  # a mask of another size is an error, not a resize
        ops.obs_forward_process(d(x), d(mask[..., :4, :4]), d(t), d(sa), d(s1), 0.04, "noise")
    with pytest.raises(NotImplementedError):
        ops.obs_forward_process(d(x), d(mask), d(t), d(sa), d(s1), 0.04, "reflect")
    with pytest.raises(RuntimeError):
        ops.obs_forward_process(torch.from_numpy(x), d(mask), d(t), d(sa), d(s1))
    with pytest.raises(RuntimeError):
        ops.obs_forward_process(d(x), d(mask), d(t), d(sa), d(s1), e_q=d(e[2][:1]))
    bad_t = t.copy()
    bad_t[1] = 50  # outside the tables: not looked up, the row is NaN
    out = ops.obs_forward_process(d(x), d(mask), d(bad_t), d(sa), d(s1), 0.04, "noise")
    assert torch.isnan(out[1][1]).all() and torch.isfinite(out[1][0]).all() and torch.isfinite(out[0]).all()


def test_forward_process_philox_streams():
    """Philox mode: keyed by the seed; the three draws are elements [0, n), [n, 2 n), [2 n, 3 n) of the library's stream (what ops.randn returns
    at those offsets), pairwise distinct, and each N(0, 1): over n samples the mean is within 5 / sqrt(n) and the variance within 5 sqrt(2 / n)."""
    from drmnet_amd import ops

    shape = (20, 3, 128, 128)
    n = int(np.prod(shape))
    x, mask, t, sa, s1, _ = forward_inputs(shape, 3)
    run = lambda seed, xx=x, mm=mask, obs=0.04, pad="noise": ops.obs_forward_process(d(xx), d(mm), d(t), d(sa), d(s1), obs, pad, seed=seed)
    a, b, c = run(11), run(11), run(12)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and all(not torch.equal(p, q) for p, q in zip(a, c))
    zero, ones = np.zeros(shape, dtype=np.float32), np.ones((shape[0], 1) + shape[2:], dtype=np.float32)
    e1 = run(11, zero, ones, 1.0, "zeros")[0]       # 1 * 0 + 1 * e1
    e2 = run(11, zero, 0 * ones, 0.0, "noise")[0]   # 0 * 0 + (1 - 0) * e2
    e3 = a[2]
    for k, e in enumerate((e1, e2, e3)):
        assert torch.equal(e, ops.randn(shape, 11, k * n, DEV)), k
    assert not torch.equal(e1, e2) and not torch.equal(e1, e3) and not torch.equal(e2, e3)
    for name, e in (("observe", e1), ("padding", e2), ("q", e3)):
        v = e.double()
        mean, var = float(v.mean()), float(v.var())
        print(f"{name}: mean {mean:+.2e} (5 sigma {5 / math.sqrt(n):.2e}), var - 1 {var - 1:+.2e} (5 sigma {5 * math.sqrt(2 / n):.2e})")
        assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
        assert abs(float((v[..., :-1] * v[..., 1:]).mean())) <= 5 / math.sqrt(n)  # neighbours are uncorrelated
    # the unaligned path draws the same stream
    small = (3, 3, 5, 7)
    xs, ms, ts, _, _, _ = forward_inputs(small, 4)
    got = ops.obs_forward_process(d(xs), d(ms), d(ts), d(sa), d(s1), 0.04, "noise", seed=11)[2]
    assert torch.equal(got, ops.randn(small, 11, 2 * int(np.prod(small)), DEV))


# ------------------------------------------------------------------------------------------------ the loss reduction
def loss_inputs(B, shape, seed, T=40):
    r = np.random.default_rng(seed)
    out, tgt = (r.normal(size=(B,) + shape).astype(np.float32) for _ in range(2))
    invmask = (r.uniform(size=(B, 1) + shape[1:]) > 0.3).astype(np.float32)
    t = r.integers(0, T, size=B).astype(np.int32)
    logvar = r.uniform(-0.5, 0.5, size=T).astype(np.float32)
    lvlb = r.uniform(0.01, 3.0, size=T).astype(np.float32)
    return out, tgt, invmask, t, logvar, lvlb


def gpu_losses(out, tgt, invmask, t, logvar, lvlb, loss_type, w1=2.0, w2=0.5, **kw):
    from drmnet_amd import ops

    return ops.diffusion_losses(d(out), d(tgt), d(t), d(logvar), d(lvlb), loss_type, w1, w2, invmask=None if invmask is None else d(invmask), **kw)


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 128, 128), (3, 24, 40), (2, 5, 7)])
@pytest.mark.parametrize("B", [1, 6, 20, 33])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_diffusion_losses_match_the_restatement(loss_type, masked, B, shape):
    """fp64 arithmetic on both sides: what is left is the fp32 rounding of the outputs (6e-8 each) -> rtol 1e-6"""
    out, tgt, invmask, t, logvar, lvlb = loss_inputs(B, shape, 100 + B)
    im = invmask if masked else None
    want = ofr.diffusion_losses(out, tgt, t, logvar, lvlb, loss_type, 2.0, 0.5, invmask=im)
    got, rows = gpu_losses(out, tgt, im, t, logvar, lvlb, loss_type, return_rows=True)
    assert got.dtype == torch.float32 and got.shape == (3,) and torch.isfinite(got).all() and rows.shape == (B,)
    print(f"{loss_type} masked={masked} B={B} {shape}: rel err {np.abs(got.cpu().numpy() / want - 1).max():.2e}")
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6)
    np.testing.assert_allclose(rows.cpu().numpy(), ofr.per_row_loss(out, tgt, loss_type, im), rtol=1e-6)
    again = gpu_losses(out, tgt, im, t, logvar, lvlb, loss_type)
    assert torch.equal(got, again)  # fixed summation order: bitwise repeatable
    # ... whatever the alignment of the pointers: the same tensors one float into a larger buffer
    shifted = lambda a: torch.cat([torch.zeros(1, device=DEV), d(a).flatten()])[1:].view(a.shape)
    from drmnet_amd import ops

    moved = ops.diffusion_losses(shifted(out), shifted(tgt), d(t), d(logvar), d(lvlb), loss_type, 2.0, 0.5, invmask=None if im is None else shifted(im))
    assert shifted(out).data_ptr() % 16 != 0 and torch.equal(moved, got)


def test_diffusion_losses_edges():
    out, tgt, invmask, t, logvar, lvlb = loss_inputs(6, (3, 16, 16), 9)
    invmask[4] = 0.0  # row 4's mask is all ones: nothing unobserved
    masked, rows = gpu_losses(out, tgt, invmask, t, logvar, lvlb, "l2", return_rows=True)
    assert torch.isnan(masked).all() and torch.isnan(rows).tolist() == [False, False, False, False, True, False]
    assert torch.isfinite(gpu_losses(out, tgt, None, t, logvar, lvlb, "l2")).all()
    with pytest.raises(NotImplementedError):
        gpu_losses(out, tgt, None, t, logvar, lvlb, "huber")
    with pytest.raises(RuntimeError):
        gpu_losses(out, tgt[:, :2], None, t, logvar, lvlb, "l2")
    with pytest.raises(RuntimeError):
        gpu_losses(out, tgt, invmask[:3], t, logvar, lvlb, "l2")
    # the raw entry point refuses a loss type it does not know and a workspace that is too small
    from drmnet_amd import _lib

    a = [d(v) for v in (out, tgt, t, logvar, lvlb)]
    ws = torch.empty(_lib.diffusion_loss_workspace_bytes(6), dtype=torch.uint8, device=DEV)
    res = torch.empty(3, device=DEV)
    call = lambda loss_type, ws_bytes: _lib.lib().drm_diffusion_losses(a[0].data_ptr(), a[1].data_ptr(), None, a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(),
                                                                     40, loss_type, 1.0, 0.0, 6, 3 * 256, 3, ws.data_ptr(), ws_bytes, res.data_ptr(), None,
                                                                     _lib.stream_ptr(DEV))
    assert call(1, ws.numel()) == 0 and call(7, ws.numel()) != 0 and call(1, ws.numel() - 8) != 0
    # a step outside the tables is not looked up
    bad_t = t.copy()
    bad_t[2] = 40
    got = gpu_losses(out, tgt, None, bad_t, logvar, lvlb, "l1").cpu()
    assert torch.isfinite(got[0]) and torch.isnan(got[1]) and torch.isnan(got[2])


# ------------------------------------------------------------------------------------------------ ObsNetDiffusion surface
def fixture_model(g, **kw):
    """the tiny ObsNet the fixture's reference run used: same constants, same seeded synthetic weights"""
    from drmnet_amd import synth
    from drmnet_amd.dataset import BaseDataset

    m = tiny_obsnet(g, **kw)
    synth.load_synth(m.model.diffusion_model, 21)
    m.ds = BaseDataset(16, TRANSFORM)
    return m.to(DEV)


def fixture_batch(g, prefix=""):
    batch = {k: torch.from_numpy(g[prefix + k]) for k in ("zK", "view_from", "LrK", "mask")}
    batch["envmap_name"] = [f"env{i}" for i in range(len(batch["zK"]))]
    noise = {k: d(g[f"{prefix}e_{k}"]) for k in ("observe", "padding", "q")}
    return batch, noise


def test_get_input_on_the_recorded_batch_matches_the_reference():
    g = gold("obsnet_forward")
    m = fixture_model(g)
    batch, noise = fixture_batch(g)
    out = m.get_input(batch, "LrK", noise=noise)
    assert len(out) == 3 and m.batch_size == 6
    LrK_z, c, mask = out
    # the bars test_gpu_forward.py holds DRMNet.get_input to for the same transforms
    np.testing.assert_allclose(LrK_z.cpu().numpy(), g["out_LrK_z"], rtol=1e-5, atol=2e-6, err_msg="LrK_z")
    np.testing.assert_allclose(c.cpu().numpy(), g["out_c"], rtol=1e-5, atol=2e-6, err_msg="c")
    assert mask.shape == (6, 1, 16, 16) and np.array_equal(mask.cpu().numpy(), g["out_mask"])
    short = m.get_input(batch, "LrK", noise={k: v[:4] for k, v in noise.items()}, bs=4)
    assert m.batch_size == 4 and all(a.shape[0] == 4 for a in short) and torch.equal(short[0], LrK_z[:4]) and torch.equal(short[1], c[:4])
    full = m.get_input(batch, "LrK", return_first_stage_outputs=True, return_original_cond=True, noise=noise)
    assert len(full) == 6 and all(torch.equal(a, b) for a, b in zip(full[:3], out))
    assert torch.equal(full[3], LrK_z) and torch.equal(full[4], LrK_z) and torch.equal(full[5], c)  # LrK, LrK_rec, cond (the padding lands in c)
    assert len(m.get_input(batch, "LrK", return_original_cond=True, noise=noise)) == 4
    # Philox draws: keyed by the seed, and the first two ranges of the stream p_losses takes the third of
    a, b, other = (m.get_input(batch, "LrK", seed=s)[1] for s in (5, 5, 6))
    assert torch.equal(a, b) and not torch.equal(a, other) and torch.equal(m.get_input(batch, "LrK", seed=5)[0], LrK_z)


def test_get_input_renders_what_the_batch_does_not_bring(tmp_path):
    from drmnet_amd import file_io, ops
    from drmnet_amd.render import render

    g = gold("obsnet_forward")
    m = fixture_model(g, envmap_dir=str(tmp_path))
    batch, noise = fixture_batch(g)
    B = 6
    batch["view_from"][1] = torch.tensor([0.2, 0.5, -0.8])  # one view off the circle
    batch["LrK"][1:, 0, 0, 0] = float("nan")  # item 0 brings its LrK; the others are marked "not cached"
    env = t32(np.stack([lit_env(8, 16, s) for s in range(B)]))
    file_io.save_exr(tmp_path / "env3.exr", env[3].numpy())  # item 3's map is marked missing and comes from envmap_dir
    env[3] = file_io.load_exr(tmp_path / "env3.exr", as_torch=True)
    batch["envmap"] = env.clone()
    batch["envmap"][3, 0, 0, 0] = float("nan")
    LrK_z, c, mask = m.get_input(batch, "LrK", noise=noise)
    # by hand: one render of the five rows, the dataset's masked transform, the forward-process kernel
    rows = [1, 2, 3, 4, 5]
    rendered = render(batch["zK"][rows], NAMES6, env[rows].to(DEV), res=16, view_from=batch["view_from"][rows])
    hdr = torch.cat([torch.from_numpy(g["LrK"][:1]).to(DEV), rendered])
    hand_mask = d(g["mask"])[:, None].float()
    hand_x = m.ds.transform(hdr, dynamic_normalize=True, mask=hand_mask)
    hand_c = ops.obs_forward_process(hand_x, hand_mask, None, None, None, float(g["noisy_observe"]), "noise", e_observe=noise["observe"],
                                     e_padding=noise["padding"], want_q=False)[0]
    assert torch.equal(LrK_z, hand_x) and torch.equal(c, hand_c) and torch.equal(mask, hand_mask) and torch.isfinite(c).all()
    np.testing.assert_allclose(LrK_z[0].cpu().numpy(), g["out_LrK_z"][0], rtol=1e-5, atol=2e-6)
    assert not np.allclose(LrK_z[1].cpu().numpy(), g["out_LrK_z"][1], atol=1e-2)
    # a batch without the key: every row is rendered, every map comes from the batch
    del batch["LrK"]
    batch["envmap"] = env.clone()
    every = m.get_input(batch, "LrK", noise=noise)[0]
    assert torch.equal(every[1:], LrK_z[1:]) and not torch.equal(every[0], LrK_z[0])
    # a missing map without an envmap_dir: the reference's message
    m2 = fixture_model(g)
    batch["envmap"][2, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="envmap_dir is needed, but not set"):
        m2.get_input(batch, "LrK", noise=noise)
    del batch["envmap"]
    with pytest.raises(AssertionError, match="envmap_dir is needed, but not set"):
        m2.get_input(batch, "LrK", noise=noise)


def loss_bars(rho, loss_type, masked, rms_out, rms_res, max_lvlb, w_simple, w_elbo, exp_neg_logvar, want):
    """Bars from the network bar rho = NET_TOL[mode] (rms(out - out_ref) <= rho rms(out_ref)), e = rho rms(model_out):
      loss_simple, l1: |d L| <= mean |delta| <= rms(delta) <= e
      loss_simple, l2: |d L| <= 2 rms(model_out - noise) e + e^2
      loss_vlb: the loss_simple bar times max_b lvlb[t_b];  loss: l_simple_weight exp(-logvar_init) times the loss_simple bar + original_elbo_weight
      times the loss_vlb bar;  plus rtol 1e-6 for the reduction.  The rms values are the fixture's (float64); for the masked loss they are taken
      under its own weighting, sum(a^2 invmask) / (sum(invmask) C) per row."""
    e = rho * rms_out
    simple = e if loss_type == "l1" else 2 * rms_res * e + e**2
    vlb = simple * max_lvlb
    return np.array([simple, vlb, w_simple * exp_neg_logvar * simple + w_elbo * vlb]) + 1e-6 * np.abs(want)


@pytest.mark.parametrize("mode", ACCURATE_MODES)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_p_losses_on_the_reference_tensors(loss_type, masked, mode):
    """The reference's network-space tensors and recorded draws through q_sample, the network and the loss kernel.  Target: the float64
    restatement on the REFERENCE's model_out; bars: loss_bars."""
    g = gold("obsnet_forward")
    m = fixture_model(g, loss_type=loss_type, masked_loss=masked)
    m.set_precision(mode)
    args = (d(g["out_LrK_z"]), d(g["out_c"]), d(g["out_mask"]), d(g["t"]))
    loss, out = m.p_losses(*args, noise=d(g["e_q"]))
    assert sorted(out) == ["val/loss", "val/loss_simple", "val/loss_vlb"] and loss.dim() == 0 and loss.is_cuda and torch.equal(loss, out["val/loss"])
    w1, w2 = float(g["l_simple_weight"]), float(g["original_elbo_weight"])
    want = ofr.diffusion_losses(g["model_out"], g["e_q"], g["t"], g["logvar"], g["lvlb_weights"], loss_type, w1, w2,
                                invmask=1 - g["out_mask"] if masked else None)
    sfx = "_masked" if masked else ""
    bars = loss_bars(NET_TOL[mode], loss_type, masked, float(g["rms_model_out" + sfx]), float(g["rms_residual" + sfx]), float(g["max_lvlb_t"]), w1, w2,
                     float(g["exp_neg_logvar_init"]), want)
    got = np.array([float(out[key]) for key in ("val/loss_simple", "val/loss_vlb", "val/loss")])
    print(f"{loss_type} masked={masked} {mode}: got {got} want {want} |got - want| {np.abs(got - want)} bars {bars}")
    assert (np.abs(got - want) <= bars).all(), (got, want, bars)
    # Philox noise: keyed by the seed
    a, b, c = (m.p_losses(*args, seed=s)[0] for s in (3, 3, 4))
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(c)
    # forward draws t itself: from the seed, or given
    f1, f2, f3 = m(*args[:3], seed=3)[0], m(*args[:3], seed=3)[0], m(*args[:3], seed=4)[0]
    assert torch.equal(f1, f2) and not torch.equal(f1, f3)
    assert torch.equal(m(*args[:3], t=args[3], seed=3)[0], a) and torch.isfinite(m(*args[:3])[0])


def ema_model(g):
    from drmnet_amd.dataset import BaseDataset

    m = tiny_obsnet(g, log_every_t=2000, ddim_steps=50, masked_loss=True, use_ema=True, ckpt_path=os.path.join(GOLD, "obsnet_tiny_ema.ckpt"),
                    init_from_ckpt_verbose=False)
    m.ds = BaseDataset(16, TRANSFORM)
    return m.to(DEV).set_precision("f16x3")


def test_shared_step_live_and_ema_match_the_reference():
    g = gold("obsnet_forward")
    m = ema_model(g)
    batch, noise = fixture_batch(g, "ema_")
    t = d(g["ema_t"])
    _, live = m.shared_step(batch, noise=noise, t=t)
    with m.ema_scope():
        _, ema = m.shared_step(batch, noise=noise, t=t)
    w1, w2 = float(g["l_simple_weight"]), float(g["original_elbo_weight"])
    for name, out in (("live", live), ("ema", ema)):
        want = g[f"ema_loss_{name}"].astype(np.float64)
        bars = loss_bars(NET_TOL["f16x3"], "l2", True, float(g[f"ema_{name}_rms_model_out_masked"]), float(g[f"ema_{name}_rms_residual_masked"]),
                         float(g["ema_max_lvlb_t"]), w1, w2, float(g["exp_neg_logvar_init"]), want)
        got = np.array([float(out[key]) for key in ("val/loss_simple", "val/loss_vlb", "val/loss")])
        print(f"{name}: got {got} want {want} |got - want| {np.abs(got - want)} bars {bars}")
        assert (np.abs(got - want) <= bars).all(), (name, got, want, bars)
    assert not np.allclose(g["ema_loss_live"], g["ema_loss_ema"], rtol=1e-4) and m._weight_set == "live"


def test_validation_step_live_and_ema():
    g = gold("obsnet_forward")
    m = ema_model(g)
    batch, _ = fixture_batch(g, "ema_")
    out = m.validation_step(batch, 0, seed=11)
    keys = ["val/loss", "val/loss_simple", "val/loss_vlb"]
    assert sorted(out) == sorted(keys + [k + "_ema" for k in keys])
    assert all(v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)) for v in out.values())
    assert all(not torch.equal(out[k], out[k + "_ema"]) for k in keys)
    again = m.validation_step(batch, 0, seed=11)
    assert all(torch.equal(out[k], again[k]) for k in out)
    other = m.validation_step(batch, 0, seed=12)
    assert not torch.equal(out["val/loss_simple"], other["val/loss_simple"])
    assert m._weight_set == "live" and m.batch_size == 4
    loss, live = m.shared_step(batch, seed=11)
    assert torch.equal(loss, out["val/loss"]) and all(torch.equal(live[k], out[k]) for k in keys)
    with m.ema_scope():
        assert torch.equal(m.shared_step(batch, seed=12)[0], out["val/loss_ema"])  # the EMA pass is keyed by seed + 1


def test_validate_end_to_end(tmp_path, capsys):
    import yaml

    from drmnet_amd import file_io
    from drmnet_amd import validate as V

    maps = tmp_path / "maps"
    maps.mkdir()
    for i in range(3):
        file_io.save_exr(maps / f"env{i:03d}.exr", lit_env(8, 16, i).astype(np.float32))
    datalist = write_datalist(tmp_path / "envs.txt", 3)
    mask_list = write_masks(tmp_path / "masks", [blob(16, 16, k) for k in range(3)])
    cfg = {"model": {"target": "models.obsnet.ObsNetDiffusion", "params": {
               "unet_config": UNET_T, "linear_start": 1e-4, "linear_end": 0.09, "timesteps": 1000, "loss_type": "l2", "first_stage_key": "LrK",
               "cond_stage_key": "masked_LrK", "padding_mode": "noise", "image_size": 16, "channels": 3, "concat_mode": True, "ddim_steps": 50,
               "monitor": "val/loss", "clip_denoised": False, "masked_loss": False, "noisy_observe": 0.04, "cache_data": False, "use_ema": True,
               "refmap_cache_root": None, "objimg_cache_root": None, "envmap_dir": None, "ckpt_path": os.path.join(GOLD, "obsnet_tiny_ema.ckpt"),
               "init_from_ckpt_verbose": False, "renderer_config": RENDERER_T}},
           "data": {"target": "main.DataModuleFromConfig", "params": {"batch_size": 2, "validation": {
               "target": "dataset.parametricrefmap.ParametricRefmapDataset",
               "params": {"size": 16, "split": "val", "return_envmap": True, "data_root": str(maps), "mask_root": str(tmp_path / "masks"),
                          "transform_func": TRANSFORM, "zdim": 6, "epoch_cycle": 1000, "refmap_cache_root": "./data/cache/refmap", "datalist": datalist,
                          "mask_list": mask_list}}}}}
    path = tmp_path / "tiny_obs.yaml"
    path.write_text(yaml.safe_dump(cfg))
    argv = ["--base", str(path), "--batch_size", "2", "--precision", "f16x3", "--seed", "5"]
    result = V.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == result
    keys = ["val/loss", "val/loss_simple", "val/loss_vlb"]
    assert sorted(result) == sorted(keys + [k + "_ema" for k in keys] + ["items", "batches"]) and (result["items"], result["batches"]) == (3, 2)
    assert all(math.isfinite(result[k]) for k in keys + [k + "_ema" for k in keys])
    assert all(result[k] != result[k + "_ema"] for k in keys)
    V.main(argv)
    again = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert again == lines
    assert V.main(argv[:-1] + ["6"])["val/loss"] != result["val/loss"]

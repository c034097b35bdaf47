#!/usr/bin/env python3
"""Generate tests/golden/forward_dataset.npz and forward_losses.npz by running the REFERENCE's own Python on the CPU (tools/refharness.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_forward.py

Needs the reference checkout refharness.REFERENCE_ROOT names (read-only).  Writes arrays only.

forward_dataset   dataset/parametricrefmap.py's items 0..31 of the splits "val" and "test" (zdim 6), with a tiny reference DRMNet attached
                  (gamma 0.95, epsilon 0.01, z0 = [1, 1, 1, 1, 0, 1]) and return_cache=True over an EMPTY cache directory -- the one branch
                  on which the reference's dataset computes the schedule (:134-193).  Keys <split>_{zK, normalized_k, view_from, K, k, zk, zkm1}.
forward_losses    the tiny reference DRMNet in eval mode (the seeded synthetic weights of the other tiny fixtures; sigma 0.02,
                  refmap_input_scaler 0.12, weights 10 / 0.1, BaseDataset("log", clamp_before_exp=20)) on a batch of 6 items at 16 x 16 whose
                  three reflectance maps are given (positive HDR values, used as they are: :531-539); row 2 is forced to K = 0 with NaN
                  zkm1 / Lrkm1, which get_input reads as "not cached" and hands to the renderer -- Mitsuba is absent, so a stand-in renderer
                  answers that one call with a NaN map (an undefined code has no reflectance map).  torch.randn_like (:416) is replaced by a
                  recorded draw.  Stored: the batch, get_input's outputs and normalizing_scale, the noise, model_out and z_out of the
                  reference's forward, the three loss scalars for l1 and for l2, and float64 rms values over the selected rows that the
                  GPU tests derive their bars from.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import refharness as rh  # noqa: E402
from drmnet_amd import synth  # noqa: E402
from oracle import unet as ou  # (the tiny network configs)  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GAMMA, EPSILON, Z0 = 0.95, 0.01, [1, 1, 1, 1, 0, 1]
N_ITEMS, B, RES = 32, 6, 16
MASKED_ROW = 2
torch.set_num_threads(8)


def save(name, **arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()})
    print(f"  wrote {name}.npz ({os.path.getsize(path) / 1024:.0f} KiB)")


def tiny_drmnet(**extra):
    DRM, _, _, _ = rh.ref_classes()
    cfg = rh.load_yaml_params("configs/drmnet/eval_drmnet.yaml")["model"]["params"]
    cfg.pop("ckpt_path")
    cfg["illnet_config"] = {"target": cfg["illnet_config"]["target"], "params": dict(ou.TINY_UNET_CFG)}
    cfg["refnet_config"] = {"target": cfg["refnet_config"]["target"], "params": dict(ou.TINY_ENC_CFG)}
    cfg.update(image_size=RES, gamma=GAMMA, epsilon=EPSILON, max_timesteps=8, z0=list(Z0), use_ema=False)
    cfg.update(extra)
    m = DRM(**cfg).eval()
    synth.load_synth(m.illnet_model.diffusion_model, 21)
    synth.load_synth(m.refnet_model.diffusion_model, 22)
    zsd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in m.illnet_model.z_emb_layer.state_dict().items()], synth.SEED_ZEMB)
    m.illnet_model.z_emb_layer.load_state_dict(zsd)
    return m


def make_dataset():
    m = tiny_drmnet()
    # what the dataset reads of the renderer to name its cache directory (:135-139); nothing is rendered
    m.renderer = types.SimpleNamespace(brdf_param_names=None, refmap_res=RES, spp=1, denoise=None, image_size=(RES, RES), envmap_size=(8, 16))
    from dataset.parametricrefmap import ParametricRefmapDataset

    out = {}
    cwd = os.getcwd()
    os.chdir(rh.REFERENCE_ROOT)  # the reference opens data/datalists/... relative to its root
    try:
        with tempfile.TemporaryDirectory() as cache:
            for split in ("val", "test"):
                ds = ParametricRefmapDataset(size=RES, split=split, data_root="./data/LavalIndoor+PolyHaven_2k/", zdim=6, return_envmap=False,
                                             return_cache=True, refmap_cache_root=cache)
                ds.model = m
                items = [ds[i] for i in range(N_ITEMS)]
                for key in ("zK", "normalized_k", "view_from", "K", "k", "zk", "zkm1"):
                    out[f"{split}_{key}"] = torch.stack([torch.as_tensor(it[key]) for it in items])
    finally:
        os.chdir(cwd)
    save("forward_dataset", gamma=GAMMA, epsilon=EPSILON, z0=np.array(Z0, dtype=np.float32), **out)


def rms(x):
    return float(torch.as_tensor(x).double().pow(2).mean().sqrt())


def make_losses():
    from dataset.basedataset import BaseDataset

    m = tiny_drmnet(sigma=0.02, refmap_input_scaler=0.12, l_refmap_weight=10.0, l_refcode_weight=0.1, envmap_dir=".")
    m.ds = BaseDataset(RES, "log", clamp_before_exp=20)
    calls = []

    def rendering(z, brdf_param_names, envmap=None, view_from=None, channel_first=False, **kw):
        calls.append(z.clone())
        return torch.full((3, RES, RES), torch.nan)

    m.renderer = types.SimpleNamespace(image_size=(RES, RES), envmap_size=(8, 16), refmap_res=RES, spp=1, denoise=None, rendering=rendering)
    g = torch.Generator().manual_seed(20261017)
    zK = torch.rand((B, 6), generator=g)
    normalized_k = torch.rand((B,), generator=g)
    K, k, zk, zkm1 = m.get_schedule(zK, normalized_k=normalized_k, return_zkm1=True)
    K, k, zkm1 = K.clone(), k.clone(), zkm1.clone()
    K[MASKED_ROW], k[MASKED_ROW] = 0, -1  # reversed_k = K - k - 1 = 0: a step count the networks accept
    zkm1[MASKED_ROW] = torch.nan
    exposure = (0.4 + 0.7 * torch.arange(B))[:, None, None, None]  # a different exposure per item, for normalizing_scale to undo
    hdr = lambda seed, gain: ((10.0 ** (synth.synth_refmaps(B, RES, RES, seed) - 1.0) - 0.1).clamp_min(1e-4) * gain * exposure).contiguous()
    LrK, Lrk, Lrkm1 = hdr(71, 3.0), hdr(72, 2.5), hdr(73, 2.0)
    Lrkm1[MASKED_ROW] = torch.nan
    phi = torch.rand((B,), generator=g) * 2 * torch.pi
    view_from = torch.stack([torch.sin(phi), torch.zeros(B), torch.cos(phi)], dim=-1)
    envmap = 0.5 + torch.rand((B, 8, 16, 3), generator=g)
    batch = {"zK": zK, "envmap_name": [f"env{i}" for i in range(B)], "view_from": view_from, "K": K, "k": k, "zk": zk, "zkm1": zkm1, "LrK": LrK,
             "Lrk": Lrk, "Lrkm1": Lrkm1, "envmap": envmap}
    oK, ok, Lr_K, Lr_k, Lr_km1, ozK, ozk, illnet_c, refnet_c = m.get_input(batch)
    assert len(calls) == 1 and torch.isnan(calls[0]).all()  # the masked row's zkm1 alone went to the renderer
    noise = torch.randn(Lr_k.shape, generator=g)
    captured = {}
    forward = m.forward

    def recording_forward(*a, **kw):
        captured["model_out"], captured["z_out"] = forward(*a, **kw)
        return captured["model_out"], captured["z_out"]

    m.forward = recording_forward
    orig = torch.randn_like
    torch.randn_like = lambda t, **kw: noise.clone()
    out = {}
    try:
        with torch.no_grad():
            for loss_type in ("l1", "l2"):
                m.loss_type = loss_type
                loss, d = m.p_losses(Lr_k, Lr_km1, ozk, ozK, oK, ok, illnet_c, refnet_c)
                out[f"loss_{loss_type}"] = torch.stack([d["val/loss_refmap"], d["val/loss_refcode"], d["val/loss"]])
                assert torch.equal(loss, d["val/loss"])
    finally:
        torch.randn_like = orig
    model_out, z_out = captured["model_out"], captured["z_out"]
    sel = oK != 0
    noised = Lr_k + m.sigma * noise
    target = (Lr_km1 - noised)[sel]
    zk_out, zK_out = m.get_brdf_out(z_out, oK - ok - 1)
    save("forward_losses", gamma=GAMMA, epsilon=EPSILON, z0=np.array(Z0, dtype=np.float32), sigma=m.sigma, refmap_input_scaler=0.12,
         l_refmap_weight=10.0, l_refcode_weight=0.1, zK=zK, K=K, k=k, zk=zk, zkm1=zkm1, LrK=LrK, Lrk=Lrk, Lrkm1=Lrkm1, view_from=view_from, envmap=envmap,
         out_K=oK, out_k=ok, out_Lr_K=Lr_K, out_Lr_k=Lr_k, out_Lr_km1=Lr_km1, out_zK=ozK, out_zk=ozk, normalizing_scale=m.normalizing_scale,
         noise=noise, model_out=model_out, z_out=z_out, rms_model_out=rms(model_out[sel]), rms_z_out=rms(z_out),
         rms_refmap_residual=rms(model_out[sel] - target), rms_zk_residual=rms(zk_out - ozk), rms_zK_residual=rms(zK_out - ozK), **out)


if __name__ == "__main__":
    rh.install_stubs()
    make_dataset()
    make_losses()

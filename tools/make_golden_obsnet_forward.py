#!/usr/bin/env python3
"""Generate tests/golden/obsnet_forward.npz by running the REFERENCE's own Python on the CPU (tools/refharness.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_obsnet_forward.py

Needs the reference checkout refharness.REFERENCE_ROOT names (read-only) and tests/golden/obsnet_tiny_ema.ckpt (tools/make_golden.py).  Writes
arrays only.

First block (no prefix): the tiny reference ObsNetDiffusion in eval mode (ou.TINY_UNET_CFG at 16 x 16, the seeded synthetic weights of the other
tiny fixtures, T = 1000, linear_end 0.09 as in configs/obsnet/train_obsnet.yaml, cond_stage_key "masked_LrK", noisy_observe 0.04, padding_mode
"noise", l_simple_weight 2.0, original_elbo_weight 0.5, logvar_init 0.3) with BaseDataset(16, "0p1tom1p1_normalizedLogarithmic_lowerbound1e-6")
on a batch of 6 items whose LrK is given (positive HDR values at a different exposure per row, used as they are: models/obsnet.py:148-153),
binary masks that each hold zeros and ones, and t spread over [0, T) with both ends.  Every torch.randn_like / torch.randint of get_input
(:385, :398), forward (:421) and p_losses (:454) is replaced by a recorded draw.  Stored: the batch, the four draws, get_input's outputs,
x_noisy, model_out, the three loss scalars for l1 and l2 each with masked_loss off and on, lvlb_weights, logvar and the two q_sample tables,
and the float64 figures the GPU tests derive their bars from (rms of model_out and of the residual, plain and under the masked loss's
weighting; max_b lvlb_weights[t_b]; exp(-logvar_init)).

Second block (prefix ema_): the model of tests/golden/obsnet_tiny_ema.ckpt (the constructor arguments of tests/test_gpu_round4.py's ObsNet
checkpoint test, plus the validation keys above with loss_type l2 and masked_loss on) and the reference's shared_step dicts outside and inside
its own ``with model.ema_scope():`` on one batch of 4 with the same draws in both passes.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import refharness as rh  # noqa: E402
from drmnet_amd import synth  # noqa: E402
from oracle import unet as ou  # (the tiny network config)  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
RES, T = 16, 1000
TRANSFORM = "0p1tom1p1_normalizedLogarithmic_lowerbound1e-6"
KEYS = dict(linear_start=1e-4, linear_end=0.09, timesteps=T, first_stage_key="LrK", cond_stage_key="masked_LrK", padding_mode="noise",
            noisy_observe=0.04, l_simple_weight=2.0, original_elbo_weight=0.5, logvar_init=0.3, image_size=RES, channels=3, concat_mode=True,
            clip_denoised=False)
torch.set_num_threads(8)


def rms(x):
    return float(torch.as_tensor(x).double().pow(2).mean().sqrt())


def masked_rms(a, invmask):
    """sqrt(mean_b sum(a^2 invmask) / (sum(invmask) C)), float64: the rms under the weighting of the masked loss (models/obsnet.py:471-473)"""
    a, w = torch.as_tensor(a).double(), torch.as_tensor(invmask).double()
    rows = (a.pow(2) * w).sum(dim=(1, 2, 3)) / (w.sum(dim=(1, 2, 3)) * a.size(1))
    return float(rows.mean().sqrt())


def tiny_obsnet(**extra):
    _, OBS, _, _ = rh.ref_classes()
    cfg = dict(KEYS, unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(ou.TINY_UNET_CFG)},
               loss_type="l2", masked_loss=False, use_ema=False)
    cfg.update(extra)
    return OBS(**cfg).eval()


def make_batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    exposure = (0.3 + 0.9 * torch.arange(B))[:, None, None, None]  # a different exposure per row, for dynamic_normalize to undo
    LrK = ((10.0 ** (synth.synth_refmaps(B, RES, RES, seed) - 1.0) - 0.1).clamp_min(1e-4) * 2.5 * exposure).contiguous()
    mask = (torch.rand((B, RES, RES), generator=g) > 0.7).double()  # (the dataset stores mask / 255 as float64)
    for b in range(B):
        assert 0 < mask[b].sum() < RES * RES  # zeros and ones in every row: the masked loss stays finite
    phi = torch.rand((B,), generator=g) * 2 * torch.pi
    batch = {"zK": torch.rand((B, 6), generator=g), "envmap_name": [f"env{i}" for i in range(B)],
             "view_from": torch.stack([torch.sin(phi), torch.zeros(B), torch.cos(phi)], dim=-1), "LrK": LrK, "mask": mask}
    draws = {"observe": torch.randn(LrK.shape, generator=g), "padding": torch.randn(LrK.shape, generator=g),
             "q": torch.randn(LrK.shape, generator=g)}
    return batch, draws


class RecordedDraws:
    """torch.randn_like / torch.randint answer from a queue, in the order the reference asks: observe, padding, t, q-noise"""

    def __init__(self):
        self.queue = []

    def __enter__(self):
        self._randn_like, self._randint = torch.randn_like, torch.randint
        torch.randn_like = lambda ref, **kw: self._pop(tuple(ref.shape))
        torch.randint = lambda lo, hi, size, **kw: self._pop(tuple(size))
        return self

    def __exit__(self, *exc):
        torch.randn_like, torch.randint = self._randn_like, self._randint

    def _pop(self, shape):
        out = self.queue.pop(0)
        assert tuple(out.shape) == shape, (tuple(out.shape), shape)
        return out.clone()


def make():
    from dataset.basedataset import BaseDataset

    B = 6
    m = tiny_obsnet()
    synth.load_synth(m.model.diffusion_model, 21)
    m.ds = BaseDataset(RES, TRANSFORM)
    batch, draws = make_batch(B, 81)
    t = torch.tensor([0, T - 1, 17, 250, 500, 873])
    out = {}
    with RecordedDraws() as rd, torch.no_grad():
        rd.queue = [draws["observe"], draws["padding"]]
        LrK_z, c, mask, LrK_t, LrK_rec, cond = m.get_input({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}, "LrK",
                                                            return_first_stage_outputs=True, return_original_cond=True)
        assert not rd.queue and c is cond and torch.equal(LrK_t, LrK_z) and torch.equal(LrK_rec, LrK_z)  # (the in-place padding lands in c)
        x_noisy = m.q_sample(x_start=LrK_z, t=t, noise=draws["q"])
        captured = {}
        apply_model = m.apply_model

        def recording_apply_model(*a, **kw):
            captured["model_out"] = apply_model(*a, **kw)
            return captured["model_out"]

        m.apply_model = recording_apply_model
        for loss_type in ("l1", "l2"):
            for masked in (False, True):
                m.loss_type, m.masked_loss = loss_type, masked
                loss, d = m.p_losses(LrK_z, c, mask, t, noise=draws["q"])
                assert torch.equal(loss, d["val/loss"])
                out[f"loss_{loss_type}_{'masked' if masked else 'plain'}"] = torch.stack([d["val/loss_simple"], d["val/loss_vlb"], d["val/loss"]])
        # the whole chain once through shared_step with every draw from the queue: the same numbers as the pieces above
        m.loss_type, m.masked_loss = "l2", False
        rd.queue = [draws["observe"], draws["padding"], t, draws["q"]]
        loss, d = m.shared_step({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()})
        assert not rd.queue and torch.equal(torch.stack([d["val/loss_simple"], d["val/loss_vlb"], d["val/loss"]]), out["loss_l2_plain"])
    model_out = captured["model_out"]
    invmask = 1 - mask
    residual = model_out - draws["q"]
    out.update(zK=batch["zK"], view_from=batch["view_from"], LrK=batch["LrK"], mask=batch["mask"], e_observe=draws["observe"],
               e_padding=draws["padding"], e_q=draws["q"], t=t, out_LrK_z=LrK_z, out_c=c, out_mask=mask, x_noisy=x_noisy, model_out=model_out,
               lvlb_weights=m.lvlb_weights, logvar=m.logvar, sqrt_alphas_cumprod=m.sqrt_alphas_cumprod,
               sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod, rms_model_out=rms(model_out), rms_residual=rms(residual),
               rms_model_out_masked=masked_rms(model_out, invmask), rms_residual_masked=masked_rms(residual, invmask),
               max_lvlb_t=float(m.lvlb_weights[t].double().max()), exp_neg_logvar_init=float(np.exp(-np.float64(np.float32(KEYS["logvar_init"])))),
               **{k: v for k, v in KEYS.items() if isinstance(v, float)})

    # ---- the reference-written EMA checkpoint: shared_step outside and inside the reference's own ema_scope, same draws
    B = 4
    e = tiny_obsnet(log_every_t=2000, ddim_steps=50, masked_loss=True, use_ema=True, ckpt_path=os.path.join(GOLD, "obsnet_tiny_ema.ckpt"))
    e.ds = BaseDataset(RES, TRANSFORM)
    batch, draws = make_batch(B, 82)
    t = torch.tensor([3, 410, 777, T - 1])
    dicts = {}
    with RecordedDraws() as rd, torch.no_grad():
        for name in ("live", "ema"):
            rd.queue = [draws["observe"], draws["padding"], t, draws["q"]]
            fresh = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
            if name == "live":
                loss, d = e.shared_step(fresh)
            else:
                with e.ema_scope("golden"):
                    loss, d = e.shared_step(fresh)
            assert not rd.queue
            dicts[name] = torch.stack([d["val/loss_simple"], d["val/loss_vlb"], d["val/loss"]])
        # the figures of the bars, per weight set (model_out of each pass)
        rd.queue = [draws["observe"], draws["padding"]]
        x, c, mask = e.get_input({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}, "LrK")
        x_noisy = e.q_sample(x_start=x, t=t, noise=draws["q"])
        invmask = 1 - mask
        figures = {}
        for name in ("live", "ema"):
            if name == "live":
                mo = e.apply_model(x_noisy, t, c)
            else:
                with e.ema_scope():
                    mo = e.apply_model(x_noisy, t, c)
            figures[f"ema_{name}_rms_model_out_masked"] = masked_rms(mo, invmask)
            figures[f"ema_{name}_rms_residual_masked"] = masked_rms(mo - draws["q"], invmask)
    assert not torch.equal(dicts["live"], dicts["ema"])
    out.update(ema_zK=batch["zK"], ema_view_from=batch["view_from"], ema_LrK=batch["LrK"], ema_mask=batch["mask"], ema_e_observe=draws["observe"],
               ema_e_padding=draws["padding"], ema_e_q=draws["q"], ema_t=t, ema_loss_live=dicts["live"], ema_loss_ema=dicts["ema"],
               ema_max_lvlb_t=float(e.lvlb_weights[t].double().max()), **figures)

    path = os.path.join(GOLD, "obsnet_forward.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()})
    print(f"  wrote obsnet_forward.npz ({os.path.getsize(path) / 1024:.0f} KiB)")
    for k in sorted(out):
        if k.startswith("loss_") or k.startswith("ema_loss"):
            print(f"  {k}: {out[k].tolist()}")


if __name__ == "__main__":
    rh.install_stubs()
    make()

"""``ObsNetDiffusion`` -- host-side operator surface of the reference's conditional DDPM, sampling on the HIP engine.

Mirrors (inference half only; training, VQ/KL first stages, patch fold/unfold are out of scope):
  DDPM.__init__/register_schedule/ema_scope/init_from_ckpt        ldm/models/diffusion/ddpm.py:59-231
  DDPM.predict_start_from_noise / q_posterior / q_sample          ddpm.py:233-246, :306-312
  LatentDiffusion.__init__/apply_model/p_mean_variance/p_sample/sample/decode_first_stage
                                                                  ddpm.py:439-488, :916-1023, :1079-1167, :1315-1350, :731-789
  ObsNetDiffusion.__init__/p_sample_loop/sample_log/get_cond_for_predict   models/obsnet.py:35-137, :500-583, :656-704
and for the validation pass of ``python main.py --base ...`` without ``-t`` (drmnet_amd.validate):
  DDPM.get_loss, lvlb_weights, logvar                              ddpm.py:296-309, :179-187, :133
  ObsNetDiffusion.get_input (cond_key "masked_LrK") / shared_step / forward / p_losses (eval mode)
                                                                  models/obsnet.py:139-413, :415-429, :453-498
  validation_step                                                 ddpm.py:373-379
with the forward process and the loss reduction on csrc/obs_forward.hip.  The object-image branch of get_input (cond_key "raw_refmap", the
Mitsuba mesh renderer) and the .pt caches stay out of scope.
``state_dict()`` keys equal the reference's (schedule buffers, ``model.diffusion_model.*``, ``model_ema.*``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .autoprec import ChainProbe
from .config import instantiate_from_config
from .ddim import DDIMSampler
from .wrappers import DiffusionWrapper, IdentityFirstStage, LitEma, ema_weights, load_checkpoint


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2):
    """The beta tables of ldm/modules/diffusionmodules/util.py:21-43 that are spaced between two end points, in fp64: "linear" (every shipped
    config) is linear in sqrt(beta), "sqrt_linear" in beta, "sqrt" is the square root of a linear ramp.  (The cosine table is training-side.)"""
    def ramp(lo, hi):
        return torch.linspace(lo, hi, n_timestep, dtype=torch.float64)

    tables = {"linear": lambda: ramp(linear_start**0.5, linear_end**0.5) ** 2, "sqrt_linear": lambda: ramp(linear_start, linear_end),
              "sqrt": lambda: ramp(linear_start, linear_end) ** 0.5}
    if schedule not in tables:
        raise ValueError(f"schedule '{schedule}' unknown.")
    return tables[schedule]().numpy()


def extract_into_tensor(a, t, x_shape):
    """Per-sample table entries a[t] shaped to broadcast against x (util.py:96-99)."""
    return a[t].reshape((t.shape[0],) + (1,) * (len(x_shape) - 1))


# Constructor / YAML keys of the reference beyond the sampling path (ldm/models/diffusion/ddpm.py:60-135, :442-512; models/obsnet.py:38-137).
# They are ACCEPTED, so configs/**.yaml and reference-style constructor calls load unchanged.  Those the validation pass reads
# (_VALIDATION_DEFAULTS) are kept in ``validation_params``; the rest steer only training, logging, the caches or the out-of-scope mesh renderer
# and are never read.  Any other unknown key is an error.
_TRAINING_ONLY = frozenset({
    "loss_type", "monitor", "original_elbo_weight", "l_simple_weight", "scheduler_config", "use_positional_encodings", "logvar_init", "cosine_s",
    "first_stage_key", "cond_stage_trainable", "masked_loss", "obj_img_key", "cache_data", "refmap_cache_root", "objimg_cache_root", "envmap_dir",
    "img_renderer_config",
})


# the reference's defaults (ddpm.py:64, :80-88, :447; models/obsnet.py:53, :60) of the keys get_input / p_losses read
_VALIDATION_DEFAULTS = {"loss_type": "l2", "l_simple_weight": 1.0, "original_elbo_weight": 0.0, "logvar_init": 0.0, "masked_loss": True,
                        "first_stage_key": "image", "envmap_dir": None}


def _drop_training_only(kwargs: dict, who: str) -> None:
    unknown = sorted(set(kwargs) - _TRAINING_ONLY)
    if unknown:
        raise TypeError(f"{who}: unexpected parameter(s) {unknown}")


class DDPM(nn.Module):
    """The noise schedule + the wrapped eps-network (ddpm.py:59-231), without training.  ``loss_type``, ``l_simple_weight``,
    ``original_elbo_weight``, ``logvar_init``, ``masked_loss``, ``first_stage_key`` and ``envmap_dir`` are kept in the dict ``validation_params``
    under their own names (not as attributes of those names: the module keeps the attribute surface of the sampling path it had)."""

    def __init__(self, unet_config, timesteps=1000, beta_schedule="linear", *, ckpt_path=None, ignore_keys=(), load_only_unet=False, use_ema=True,
                 image_size=256, channels=3, log_every_t=100, clip_denoised=True, linear_start=1e-4, linear_end=2e-2, given_betas=None,
                 v_posterior=0.0, conditioning_key=None, parameterization="eps", learn_logvar=False, **training_only):
        super().__init__()
        _drop_training_only(training_only, type(self).__name__)
        if parameterization != "eps":
            raise NotImplementedError('only the "eps" parameterization is on the shipped path')
        if learn_logvar:
            raise NotImplementedError("learn_logvar is training-only")
        self.parameterization = parameterization
        self.validation_params = {k: training_only.get(k, d) for k, d in _VALIDATION_DEFAULTS.items()}
        self.image_size, self.channels = image_size, channels
        self.clip_denoised, self.log_every_t, self.v_posterior = clip_denoised, log_every_t, v_posterior
        self.cond_stage_model = None
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self._weight_set = "live"
        self.use_ema = use_ema
        if use_ema:
            self.model_ema = LitEma(self.model)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=list(ignore_keys), only_model=load_only_unet)
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps, linear_start=linear_start, linear_end=linear_end)
        # ddpm.py:133: a plain tensor attribute there (learn_logvar raises above); here a buffer outside state_dict(), so that it follows .to()
        self.register_buffer("logvar", torch.full(fill_value=float(self.validation_params["logvar_init"]), size=(self.num_timesteps,)), persistent=False)

    @property
    def device(self):
        return self.betas.device

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4, linear_end=2e-2):
        """ldm/models/diffusion/ddpm.py:137-187: every table of the forward / posterior process is computed in fp64 numpy from the
        betas and registered as an fp32 buffer -- same names, same order, so ``state_dict()`` matches the reference's checkpoints
        (tests/golden/ddpm_schedule.npz pins the values bit for bit).  abar_t = prod(1 - beta); posterior q(x_{t-1} | x_t, x_0)
        has variance beta_t (1 - abar_{t-1}) / (1 - abar_t) (mixed with beta_t by v_posterior) and mean coefficients
        beta_t sqrt(abar_{t-1}) / (1 - abar_t) on x_0 and (1 - abar_{t-1}) sqrt(alpha_t) / (1 - abar_t) on x_t."""
        beta = given_betas if given_betas is not None else make_beta_schedule(beta_schedule, timesteps, linear_start, linear_end)
        (n_steps,) = beta.shape
        self.num_timesteps = int(n_steps)
        self.linear_start, self.linear_end = linear_start, linear_end
        alpha = 1.0 - beta
        abar = np.cumprod(alpha, axis=0)
        abar_prev = np.append(1.0, abar[:-1])
        post_var = (1 - self.v_posterior) * beta * (1.0 - abar_prev) / (1.0 - abar) + self.v_posterior * beta
        tables = (  # (buffer name, fp64 table) in the reference's registration order
            ("betas", beta),
            ("alphas_cumprod", abar),
            ("alphas_cumprod_prev", abar_prev),
            ("sqrt_alphas_cumprod", np.sqrt(abar)),
            ("sqrt_one_minus_alphas_cumprod", np.sqrt(1.0 - abar)),
            ("log_one_minus_alphas_cumprod", np.log(1.0 - abar)),
            ("sqrt_recip_alphas_cumprod", np.sqrt(1.0 / abar)),
            ("sqrt_recipm1_alphas_cumprod", np.sqrt(1.0 / abar - 1)),
            ("posterior_variance", post_var),
            ("posterior_log_variance_clipped", np.log(np.maximum(post_var, 1e-20))),  # the variance is 0 at t = 0
            ("posterior_mean_coef1", beta * np.sqrt(abar_prev) / (1.0 - abar)),
            ("posterior_mean_coef2", (1.0 - abar_prev) * np.sqrt(alpha) / (1.0 - abar)),
        )
        for name, table in tables:
            self.register_buffer(name, torch.tensor(table, dtype=torch.float32))
        # ddpm.py:179-187 ("eps"): the weight of the variational bound's term t, in fp32 from the fp32 buffers as the reference computes it;
        # posterior_variance[0] is 0, so entry 0 takes entry 1.  persistent=False: not in state_dict(), as there
        lvlb_weights = self.betas**2 / (2 * self.posterior_variance * torch.tensor(alpha, dtype=torch.float32) * (1 - self.alphas_cumprod))
        lvlb_weights[0] = lvlb_weights[1]
        self.register_buffer("lvlb_weights", lvlb_weights, persistent=False)
        assert not torch.isnan(self.lvlb_weights).all()

    def ema_scope(self, context=None):
        """ldm/models/diffusion/ddpm.py:189-202 -- ``with model.ema_scope(): ...`` samples with the EMA weights (wrappers.ema_weights)."""
        return ema_weights(self, [(self.model, self.model_ema)] if self.use_ema else [], context)

    def init_from_ckpt(self, path, ignore_keys=list(), only_model=False, verbose=True):
        """ddpm.py:204-231 / models/obsnet.py:139-160 (``only_model`` loads into the wrapped U-Net alone)."""
        load_checkpoint(self, path, ignore_keys, into=self.model if only_model else None, verbose=verbose)

    def predict_start_from_noise(self, x_t, t, noise):
        return (extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                - extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t):
        mean = (extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start
                + extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        return mean, extract_into_tensor(self.posterior_variance, t, x_t.shape), extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape)

    def q_sample(self, x_start, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        return (extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def get_loss(self, pred, target, mean=True):
        """ddpm.py:296-309 on torch tensors (the validation pass itself reduces on the device through ops.diffusion_losses)."""
        loss_type = self.validation_params["loss_type"]
        if loss_type == "l1":
            loss = (target - pred).abs()
        elif loss_type == "l2":
            loss = (target - pred) ** 2
        else:
            raise NotImplementedError(f"unknown loss type '{loss_type}'")
        return loss.mean() if mean else loss


class LatentDiffusion(DDPM):
    """DDPM + conditioning by concatenation behind an identity first stage (ddpm.py:439-512), inference half."""

    def __init__(self, first_stage_config, cond_stage_config, num_timesteps_cond=None, cond_stage_key="image", *, concat_mode=True, cond_stage_forward=None,
                 conditioning_key=None, scale_factor=1.0, scale_by_std=False, ckpt_path=None, ignore_keys=(), **ddpm_kwargs):
        if scale_by_std:
            raise NotImplementedError("scale_by_std is training-only")
        if (num_timesteps_cond or 1) != 1:
            raise NotImplementedError("num_timesteps_cond > 1 (shortened conditioning schedule) is not on the shipped path")
        if cond_stage_config not in ("__is_first_stage__", "__is_unconditional__"):
            raise NotImplementedError("a separate cond_stage_config is not on the shipped path")
        if conditioning_key is None:
            conditioning_key = "concat" if concat_mode else "crossattn"
        if cond_stage_config == "__is_unconditional__":
            conditioning_key = None
        super().__init__(conditioning_key=conditioning_key, **ddpm_kwargs)  # (the checkpoint is read below, once the whole module exists)
        self.num_timesteps_cond = 1
        self.concat_mode, self.cond_stage_key, self.cond_stage_forward, self.scale_factor = concat_mode, cond_stage_key, cond_stage_forward, scale_factor
        self.first_stage_model = instantiate_from_config(first_stage_config).eval()
        if not isinstance(self.first_stage_model, IdentityFirstStage):
            raise NotImplementedError("only IdentityFirstStage is used by the shipped configs")
        self.cond_stage_model = self.first_stage_model if cond_stage_config == "__is_first_stage__" else None
        self.clip_denoised = False  # (ddpm.py:492: LatentDiffusion overrides the DDPM default)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, list(ignore_keys))
        self._ws = _lib.Workspace()

    def set_precision(self, precision: str, probe=None):
        """Conv arithmetic of the U-Net: "fp32" (exact fp32 MFMA), "f16x3" (split fp16, fp32-accurate, ~2.5x faster), "f16mx" (f16x3 with
        fp8 cross terms on the 3x3 convs: ~4e-5 per forward, ~3x faster) or "f16" (reduced precision)."""
        self.model.diffusion_model.set_precision(precision)
        # "auto": the per-network probe (unet.py) + a chain probe before f16mx is kept (autoprec.ChainProbe over _auto_chain_probe)
        # ``probe`` [n,3,H,W]: conditioning refmaps of the CALLER for the chain probe; without it the first batch a sampler sees is handed to it
        self._auto_chain = ChainProbe(self.AUTO_CHAIN_TOLERANCE, self.AUTO_CHAIN_STEPS, None if probe is None else _lib.require_gpu_tensor(probe, "probe").detach(),
                                      step_name="DDIM steps", probe_text="{dims} {rows}: first {steps} steps of the DDIM-50 chain (eta 1), worst row",
                                      caller_rows="conditioning rows of the caller") if precision == "auto" else None
        return self

    AUTO_CHAIN_TOLERANCE = 5e-5  # half the 1e-4 contract, like the per-network probe
    AUTO_CHAIN_STEPS = 8
    _auto_chain: Optional[ChainProbe] = None  # None outside auto mode (assigning None switches the chain probe off, the network's mode stays)

    @property
    def auto_chain_report(self):
        return None if self._auto_chain is None else self._auto_chain.report

    def calibrate_precision(self, probe=None):
        """Auto mode: runs the network's probe and the chain probe now (weights on a GPU); returns the chain report.  ``probe``: conditioning refmaps
        of the caller to run the chain on (re-measured for these rows)."""
        if self._auto_chain is not None and probe is not None:
            self._auto_chain.set_probe(_lib.require_gpu_tensor(probe, "probe").detach())
        self.model.diffusion_model.calibrate_precision()
        self._auto_chain_probe()
        return self.auto_chain_report

    def _auto_chain_probe(self, data=None) -> None:
        """The chain of autoprec.ChainProbe: the first eight steps of the DDIM-50 chain (eta = 1, Philox noise from a fixed key: the steps with the
        largest 1 / sqrt(alpha_bar) amplification) from a seeded x_T, conditioned on rows of ``data``.  (ddim_sampling comes back here through _engine: the
        probe is busy then and returns at once.)"""
        ac, unet = self._auto_chain, self.model.diffusion_model
        if ac is None:
            return

        def run_chain(cond):
            x_T = torch.randn((cond.shape[0], 3, *cond.shape[2:]), generator=torch.Generator().manual_seed(20261004)).to(cond.device)
            smp = DDIMSampler(self)
            smp.make_schedule(50, ddim_eta=1.0, verbose=False)
            return smp.ddim_sampling(cond, tuple(x_T.shape), x_T=x_T, seed=20261004, num_steps=ac.steps, log_every_t=0, verbose=False)[0]

        ac.measure({"unet": unet}, unet._active_set, run_chain, data, next(unet.parameters()).device)

    def _engine(self, cond=None):
        """The U-Net's engine handle behind the auto mode's chain probe (which may move the network to f16x3 for these weights); ``cond``: the
        conditioning the caller is about to sample with -- the chain probe runs on rows of it (once per weight signature)."""
        unet = self.model.diffusion_model
        h = unet.engine_handle()
        if self._auto_chain is not None:
            self._auto_chain_probe(cond)
            h = unet.engine_handle()
        return h

    def get_learned_conditioning(self, c):
        if self.cond_stage_forward is None:
            if hasattr(self.cond_stage_model, "encode") and callable(self.cond_stage_model.encode):
                return self.cond_stage_model.encode(c)
            return self.cond_stage_model(c)
        return getattr(self.cond_stage_model, self.cond_stage_forward)(c)

    @torch.no_grad()
    def encode_first_stage(self, x):
        return self.first_stage_model.encode(x)

    def get_first_stage_encoding(self, encoder_posterior):
        assert isinstance(encoder_posterior, torch.Tensor)
        return self.scale_factor * encoder_posterior

    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        return self.first_stage_model.decode(1.0 / self.scale_factor * z)

    def apply_model(self, x_noisy, t, cond, return_ids=False):
        """ddpm.py:916-926,1017-1023: one U-Net forward on cat([x, cond], 1) (the cat is folded into the engine)."""
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            key = "c_concat" if self.model.conditioning_key == "concat" else "c_crossattn"
            cond = {key: cond}
        return self.model(x_noisy, t, **cond)

    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_x0=False, **unused):
        model_out = self.apply_model(x, t, c)
        x_recon = self.predict_start_from_noise(x, t=t, noise=model_out)
        if clip_denoised:
            x_recon.clamp_(-1.0, 1.0)
        model_mean, posterior_variance, posterior_log_variance = self.q_posterior(x_start=x_recon, x_t=x, t=t)
        if return_x0:
            return model_mean, posterior_variance, posterior_log_variance, x_recon
        return model_mean, posterior_variance, posterior_log_variance

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_x0=False, temperature=1.0, noise=None, **unused):
        """Single ancestral step (ddpm.py:1120-1167) -- per-step drop-in; the fused loop is ``p_sample_loop``."""
        b = x.shape[0]
        outs = self.p_mean_variance(x=x, c=c, t=t, clip_denoised=clip_denoised, return_x0=return_x0)
        model_mean, _, model_log_variance = outs[:3]
        noise = (torch.randn_like(x) if noise is None else noise) * temperature
        nonzero_mask = (1 - (t == 0).float()).reshape(b, *((1,) * (len(x.shape) - 1)))
        out = model_mean + nonzero_mask * (0.5 * model_log_variance).exp() * noise
        return (out, outs[3]) if return_x0 else out

    def ddpm_coef_table(self) -> np.ndarray:
        """[T,5] fp32: sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1/2, exp(0.5*logvar)."""
        tab = torch.stack([self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.posterior_mean_coef1,
                           self.posterior_mean_coef2, (0.5 * self.posterior_log_variance_clipped).exp()], dim=1)
        return np.ascontiguousarray(tab.detach().cpu().numpy().astype(np.float32))

    @torch.no_grad()
    def _ddpm_loop(self, cond, shape, x_T=None, timesteps=None, start_T=None, noise=None, seed=None, mask=None, x0=None, mask_noise=None, blend_when=1,
                   temperature=1.0, noise_dropout=0.0, dropout_keep=None):
        """The ancestral chain on the device (drm_ddpm_sample).  mask / x0: the known-region blending of the reference's two loops --
        ``blend_when`` 1 = LatentDiffusion.p_sample_loop (after p_sample, q_sample(x0, t): ddpm.py:1300-1302), 0 = ObsNetDiffusion.p_sample_loop (before
        p_sample, x0 itself at t == 0, else q_sample(x0, t - 1): models/obsnet.py:545-547); ``mask_noise`` [T,N,C,H,W] injects q_sample's draws.
        ``temperature`` scales the step noise (ddpm.py:1157: the exp(0.5 logvar) column); ``noise_dropout`` is p_sample's F.dropout on it (ddpm.py:1158-1159;
        ``dropout_keep`` [T,N,C,H,W] injects the 0 / 1 masks).  (The reference's p_sample_loop passes neither to p_sample: knobs of p_sample itself.)"""
        if (mask is None) != (x0 is None):
            raise ValueError("mask and x0 go together (ddpm.py:1286-1288)")
        dev = self.betas.device
        c = cond[0] if isinstance(cond, (list, tuple)) else cond
        c = _lib.require_gpu_tensor(c, "cond")
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        from . import ops

        img = ops.randn(shape, seed, 0, dev) if x_T is None else _lib.require_gpu_tensor(x_T, "x_T").clone()
        T = self.num_timesteps if timesteps is None else timesteps
        if start_T is not None:
            T = min(T, start_T)
        noise = None if noise is None else _lib.require_gpu_tensor(noise, "noise")
        h = self._engine(c)
        L = _lib.lib()
        n, _, hh, ww = shape
        ws = self._ws.get(int(L.drm_sampler_workspace_bytes(h, n, hh, ww)), dev)
        pred_x0 = torch.empty_like(img)
        coef = self.ddpm_coef_table()
        if temperature != 1.0:
            coef = coef.copy()
            coef[:, 4] = (torch.from_numpy(coef[:, 4]) * float(temperature)).numpy()
        if not 0.0 <= noise_dropout < 1.0:
            raise ValueError("noise_dropout: 0 <= p < 1")
        blend = None
        if mask is not None:
            sa = self.sqrt_alphas_cumprod.detach().cpu().float().numpy()
            s1 = self.sqrt_one_minus_alphas_cumprod.detach().cpu().float().numpy()
            q = np.zeros((T, 2), dtype=np.float32)
            for j in range(T):
                t = T - 1 - j
                if blend_when == 1:
                    q[j] = (sa[t], s1[t])
                else:
                    q[j] = (1.0, 0.0) if t == 0 else (sa[t - 1], s1[t - 1])
            blend = _lib.make_mask_blend(mask, x0, q, mask_noise, blend_when, tuple(img.shape))
        opt, keep = _lib.make_sampler_options(tuple(img.shape), T, blend=blend, noise_dropout=noise_dropout, dropout_keep=dropout_keep)
        with torch.cuda.device(dev):
            _lib.check(L.drm_ddpm_sample(h, img.data_ptr(), pred_x0.data_ptr(), c.data_ptr(), coef.ctypes.data_as(C.POINTER(C.c_float)), T,
                                         int(bool(self.clip_denoised)), _lib.ptr(noise), seed, C.byref(opt), n, hh, ww, ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr(dev)))
        if any(k is not None for k in keep) or noise_dropout > 0.0:
            torch.cuda.current_stream(dev).synchronize()  # (the options' tensors stay alive until the chain has run)
        return img, pred_x0

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None, noise=None, seed=None,
                      mask_noise=None, temperature=1.0, noise_dropout=0.0, dropout_keep=None):
        """ddpm.py:1253-1313 -> final img.  (intermediates: only the endpoints are kept; the loop runs on the device.)  mask / x0: ddpm.py:1300-1302."""
        if callback is not None or img_callback is not None or quantize_denoised:
            raise NotImplementedError("callbacks / quantize are not on the shipped path")
        img, _ = self._ddpm_loop(cond, shape, x_T, timesteps, start_T, noise, seed, mask, x0, mask_noise, 1, temperature, noise_dropout, dropout_keep)
        if return_intermediates:
            return img, [img]
        return img

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None, quantize_denoised=False,
               mask=None, x0=None, shape=None, **kwargs):
        if shape is None:
            shape = (batch_size, self.channels, self.image_size, self.image_size)
        if cond is not None:
            cond = [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose, timesteps=timesteps,
                                  quantize_denoised=quantize_denoised, mask=mask, x0=x0, **kwargs)


class ObsNetDiffusion(LatentDiffusion):
    """inpainting class (models/obsnet.py:35)."""

    def __init__(self, renderer_config=None, img_renderer_config=None, num_timesteps_cond=None, cond_stage_key="image", padding_mode="noise", *,
                 ddim_steps: Optional[int] = None, ddim_eta: float = 1.0, noisy_observe: float = 0.0, init_from_ckpt_verbose=True, first_stage_config=None,
                 cond_stage_config="__is_first_stage__", ckpt_path=None, ignore_keys=(), **kwargs):
        # (the leading five parameters keep the reference's positional order, models/obsnet.py:38-44; img_renderer_config renders training
        # images only and is never read)
        if first_stage_config is None:
            first_stage_config = {"target": "ldm.models.autoencoder.IdentityFirstStage"}
        super().__init__(first_stage_config, cond_stage_config, num_timesteps_cond, cond_stage_key, **kwargs)
        self.renderer = instantiate_from_config(renderer_config) if renderer_config is not None else None
        self.padding_mode, self.noisy_observe = padding_mode, noisy_observe
        self.ddim_steps, self.ddim_eta = ddim_steps, ddim_eta
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, list(ignore_keys), verbose=init_from_ckpt_verbose)
        self.eval()

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None, noise=None, seed=None,
                      mask_noise=None, temperature=1.0, noise_dropout=0.0, dropout_keep=None):
        """models/obsnet.py:500-564: like LatentDiffusion.p_sample_loop but returns pred_x0 of the LAST step; mask / x0 blend BEFORE p_sample
        (x0 itself at t == 0, else q_sample(x0, t - 1): models/obsnet.py:545-547)."""
        if callback is not None or img_callback is not None or quantize_denoised:
            raise NotImplementedError("callbacks / quantize are not on the shipped path")
        img, pred_x0 = self._ddpm_loop(cond, shape, x_T, timesteps, start_T, noise, seed, mask, x0, mask_noise, 0, temperature, noise_dropout, dropout_keep)
        if return_intermediates:
            return pred_x0, {"x_inter": [img], "pred_x0": [pred_x0]}
        return pred_x0

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        """models/obsnet.py:566-583."""
        if ddim:
            ddim_sampler = DDIMSampler(self)
            shape = (self.channels, self.image_size, self.image_size)
            samples, intermediates = ddim_sampler.sample(
                ddim_steps, batch_size, shape, cond, verbose=False,
                log_every_t=kwargs.pop("log_every_t", None) or max(self.log_every_t * ddim_steps // self.num_timesteps, 1), **kwargs)
        else:
            samples, intermediates = self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)
        return samples, intermediates

    # ------------------------------------------------------------------ the validation pass (forward process + losses)
    def _refmap_renderer(self):
        from .render import RefMapRenderer

        if not isinstance(self.renderer, RefMapRenderer) or not self.renderer.brdf_param_names:
            raise NotImplementedError("rendering LrK needs a renderer_config of drmnet_amd.render.RefMapRenderer with brdf_param_names, got "
                                      f"{type(self.renderer).__name__}")
        return self.renderer

    def _load_envmaps(self, names) -> torch.Tensor:
        """envmap_dir/<name>.exr for every name, stacked [n, H, W, 3] on the host (models/obsnet.py:157-169)."""
        from pathlib import Path

        from . import file_io

        root = self.validation_params["envmap_dir"]
        assert root is not None, "envmap_dir is needed, but not set"
        return torch.stack([file_io.load_exr(Path(root) / f"{name}.exr", as_torch=True) for name in names])

    @torch.no_grad()
    def get_input(self, batch, k, return_first_stage_outputs=False, force_c_encode=False, cond_key=None, return_original_cond=False, bs=None, *,
                  noise=None, seed=None):
        """models/obsnet.py:139-413 for cond_key "masked_LrK" (any other key raises, as :373 does for the shipped "raw_refmap" configs: the
        reference compares against " raw_refmap" with a leading space, and that branch needs the Mitsuba object-image renderer): the first ``bs``
        items of a MaskedRefmapDataset batch -> [LrK_z, c, mask(, LrK, LrK_rec)(, cond)].  Rows whose ``batch[k]`` has a NaN [b, 0, 0, 0], or every
        row when the batch has no ``k``, are rendered from zK under batch["envmap"][b] (read from envmap_dir/<name>.exr where missing or NaN-marked)
        seen from batch["view_from"][b], all of them in one drm_render_refmap launch.  Then ``ds.transform(LrK, dynamic_normalize=True,
        mask=mask)`` and one drm_obs_forward_process launch: c = mask LrK + noisy_observe e1 + (1 - mask) e2.  The reference's in-place
        ``cond += ...`` also lands in c (IdentityFirstStage.encode returns its argument); restated explicitly: c and cond are the padded tensor.
        The .pt caches are neither read nor written.

        Keyword-only, not in the reference: ``noise`` = {"observe": e1, "padding": e2} injects the draws (parity runs); one that is not injected
        comes from the library's Philox stream keyed by ``seed`` (drawn from torch's generator when None), e1 and e2 from the first two of its
        three ranges (p_losses takes the third)."""
        from . import ops

        cond_key = cond_key if cond_key is not None else self.cond_stage_key
        if cond_key != "masked_LrK":
            raise NotImplementedError(f'cond_key {cond_key!r}: only "masked_LrK" is implemented (the reference itself raises for "raw_refmap", '
                                      "models/obsnet.py:373)")
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("get_input runs on the GPU: move the model there first (drmnet_amd has no CPU path)")
        zK = batch["zK"]
        bs = min(len(zK), bs) if bs is not None else len(zK)
        self.batch_size = bs
        zK = zK[:bs].to(dev, torch.float32)
        envmap_name = list(batch["envmap_name"][:bs])
        view_from = batch.get("view_from")[:bs]
        given = batch[k][:bs].to(dev, torch.float32) if k in batch else None
        not_cached = torch.ones(bs, dtype=torch.bool) if given is None else torch.isnan(given[:, 0, 0, 0]).cpu()
        if bool(not_cached.any()):
            renderer = self._refmap_renderer()
            rows = torch.nonzero(not_cached).flatten().tolist()
            have = batch["envmap"][:bs] if "envmap" in batch else None
            load = [b for b in rows if have is None or bool(torch.isnan(have[b, 0, 0, 0]))]
            loaded = self._load_envmaps([envmap_name[b] for b in load]) if load else None
            maps = [loaded[load.index(b)] if b in load else have[b] for b in rows]
            envmap = torch.stack([m.to(dev, torch.float32) for m in maps])
            rendered = renderer.render(zK[rows], None, envmap, view_from=torch.as_tensor(view_from)[rows])
            if given is None:
                LrK = rendered
            else:
                LrK = given.clone().index_copy_(0, torch.tensor(rows, device=dev), rendered)
        else:
            LrK = given
        mask = batch["mask"][:bs, None].to(dev, torch.float32).contiguous()  # [BS, 1, H, W]
        LrK = self.ds.transform(LrK.contiguous(), dynamic_normalize=True, mask=mask)
        LrK_z = self.get_first_stage_encoding(self.encode_first_stage(LrK)).detach()
        if self.model.conditioning_key is not None:
            if tuple(mask.shape[-2:]) != (self.image_size, self.image_size):  # :396 (default mode: nearest); a no-op on the shipped configs
                mask = ops.resize(mask, (self.image_size, self.image_size), "nearest")
            if self.padding_mode not in ("noise", "zeros"):
                raise NotImplementedError()
            noise = noise or {}
            if seed is None:
                seed = int(torch.randint(0, 2**62, (1,)).item())
            cond = ops.obs_forward_process(LrK, mask, None, None, None, self.noisy_observe, self.padding_mode, e_observe=noise.get("observe"),
                                           e_padding=noise.get("padding"), seed=seed, want_q=False)[0]
            c = self.get_learned_conditioning(cond)
        else:
            cond = c = None
        out = [LrK_z, c, mask]
        if return_first_stage_outputs:
            out.extend([LrK, self.decode_first_stage(LrK_z)])
        if return_original_cond:
            out.append(cond)
        return out

    def _draw_t(self, n, seed):
        """forward's draw of the steps (models/obsnet.py:421): torch's global generator as in the reference, or a CPU generator seeded by ``seed``"""
        if seed is None:
            return torch.randint(0, self.num_timesteps, (n,), device=self.device).long()
        return torch.randint(0, self.num_timesteps, (n,), generator=torch.Generator().manual_seed(int(seed))).long().to(self.device)

    def shared_step(self, batch, *, seed=None, noise=None, t=None, **kwargs):
        """models/obsnet.py:415-418.  ``seed`` keys the steps t and the three noise draws; ``noise`` = {"observe", "padding", "q"} and ``t``
        inject them instead (parity runs)."""
        noise = noise or {}
        x, c, mask = self.get_input(batch, self.validation_params["first_stage_key"], noise=noise, seed=seed)
        return self(x, c, mask, noise.get("q"), t=t, seed=seed)

    def forward(self, x, c, mask, *args, t=None, seed=None, **kwargs):
        """models/obsnet.py:420-429: t ~ randint(0, num_timesteps) per row unless ``t`` is given (``seed``: from a CPU generator seeded by it)."""
        if t is None:
            t = self._draw_t(x.shape[0], seed)
        if self.model.conditioning_key is not None:
            assert c is not None
        return self.p_losses(x, c, mask, t, *args, seed=seed, **kwargs)

    @torch.no_grad()
    def p_losses(self, x_start, cond, mask, t, noise=None, *, seed=None):
        """models/obsnet.py:453-498 in eval mode: q_sample at each row's t (``noise`` [B, 3, H, W] if given, else the q-noise range of the
        library's Philox stream keyed by ``seed``, drawn from torch's generator when None), one pass of the network, and the three losses from
        drm_diffusion_losses.  Returns (loss, {"val/loss_simple", "val/loss_vlb", "val/loss"}), 0-dim device tensors.  There is no backward on
        this engine: training mode raises."""
        from . import ops

        if self.training:
            raise NotImplementedError("p_losses in training mode: the HIP engine has no backward (validation only)")
        vp = self.validation_params
        x_start = _lib.require_gpu_tensor(x_start, "x_start")
        dev = x_start.device
        t = t.to(dev)
        if noise is not None:
            noise = _lib.require_gpu_tensor(noise, "noise")
        elif seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        _, x_noisy, noise = ops.obs_forward_process(x_start, None, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, e_q=noise,
                                                    seed=seed or 0, want_cond=False)
        model_output = self.apply_model(x_noisy, t.long(), cond)
        invmask = (1 - _lib.require_gpu_tensor(mask, "mask")) if vp["masked_loss"] else None
        out = ops.diffusion_losses(model_output, noise, t, self.logvar, self.lvlb_weights, vp["loss_type"], vp["l_simple_weight"],
                                   vp["original_elbo_weight"], invmask=invmask)
        return out[2], {"val/loss_simple": out[0], "val/loss_vlb": out[1], "val/loss": out[2]}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx, *, seed=None):
        """ddpm.py:373-379: the losses on the live weights and, under ema_scope, on the EMA weights (keys + "_ema").  The reference logs the
        two dicts; there is no logger here, so the merged six-key dict is returned (0-dim device tensors).  ``seed``: the draws of the live pass
        are keyed by it, those of the EMA pass by seed + 1 (the reference draws twice from one generator)."""
        _, loss_dict = self.shared_step(batch, seed=seed)
        with self.ema_scope():
            _, loss_dict_ema = self.shared_step(batch, seed=None if seed is None else seed + 1)
        merged = dict(loss_dict)
        merged.update({key + "_ema": v for key, v in loss_dict_ema.items()})
        return merged

    @torch.no_grad()
    def get_cond_for_predict(self, batch: Dict[str, Union[torch.Tensor, str]], bs: Optional[int] = None, force_c_encode: bool = False,
                             noise: Optional[torch.Tensor] = None):
        """models/obsnet.py:656-704 (cond_stage_key == 'raw_refmap').  The reference's in-place ``cond += ...`` also mutates
        ``c`` because IdentityFirstStage.encode returns the same tensor (SURVEY.md 7 'bug-compat aliasing'); restated explicitly:
        c = raw_refmap*mask + (1-mask)*noise."""
        if self.model.conditioning_key is None:
            mask = batch.get("mask")
            return None, (mask[:bs, None].float() if mask is not None else None), batch["tag"][:bs]
        if self.cond_stage_key != "raw_refmap":
            raise NotImplementedError(self.cond_stage_key)
        mask = batch["raw_refmask"][:bs, None].float()
        raw_refmap = self.ds.transform(batch["raw_refmap"][:bs], dynamic_normalize=True, mask=mask)
        cond = raw_refmap * mask
        if self.noisy_observe > 0:
            cond = self.noisy_observe * torch.randn_like(cond) + cond
        c = self.get_learned_conditioning(cond.to(self.device))
        if tuple(mask.shape[-2:]) != (self.image_size, self.image_size):  # :691 (default mode: nearest); a no-op on the shipped configs
            mask = ops.resize(mask, (self.image_size, self.image_size), "nearest")
        if self.padding_mode == "noise":
            nz = torch.randn_like(c) if noise is None else noise
            c = c + (1 - mask) * nz
        elif self.padding_mode != "zeros":
            raise NotImplementedError()
        return c, mask, batch["tag"][:bs]

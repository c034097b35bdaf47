"""``DRMNet`` -- host-side operator surface of the reference LightningModule, sampling on the HIP engine.

Mirrors models/drmnet.py of the reference by name, signature and return values for everything the
inference path touches (scripts/estimate.py:84-100):
  __init__ params (configs/drmnet/eval_drmnet.yaml), ema_scope :242-258, init_from_ckpt :260-277,
  apply_model :376-388, get_brdf_out :390-396, forward :452-456, get_schedule :458-501,
  check_convergence :747-750, p_mean_variance :752-770, p_sample (stub) :772-780,
  p_sample_loop :782-847, get_input_for_predict :1011-1045, decode_first_stage, r0toenvmap :931-941, the forward model on
  csrc/render.hip: basis_r0 :328-347, rendering_refmaps :667-696, get_visualized_brdf_grid :916-929, reconstruct :943-953,
and for the validation pass of ``python main.py --base ...`` without ``-t`` (drmnet_amd.validate):
  get_loss :398-411, p_losses :413-450 (eval mode, losses on csrc/losses.hip), get_input :503-651, shared_step :707-710,
  validation_step :731-740.
Training (backward, the EMA update, train_with_zk_gt), log_images and the .pt refmap cache are out of scope.

The module is a plain ``nn.Module`` (pytorch_lightning is not needed for inference); ``state_dict()`` has the
reference's keys, so ``drmnet.ckpt`` loads with ``init_from_ckpt``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .autoprec import ChainProbe, tensor_sig
from .config import instantiate_from_config
from .wrappers import DiffusionWrapper, IdentityFirstStage, LitEma, ZEmbDiffusionWrapper, ema_weights, load_checkpoint


# Constructor / YAML keys of the reference (models/drmnet.py:79-240) beyond the sampling path: accepted so that configs/drmnet/*.yaml load
# unchanged.  Those the validation pass reads (_VALIDATION_DEFAULTS) are kept in ``validation_params``; the rest steer only training, logging
# or the refmap cache and are never read.  Any other unknown key is an error.
_TRAINING_ONLY = frozenset({
    "loss_type", "monitor", "scheduler_config", "cond_stage_trainable", "l_refmap_weight", "l_refcode_weight", "sigma",
    "train_with_zk_gt", "train_with_zk_gt_switch_epoch", "cache_refmap", "refmap_cache_root", "envmap_dir",
})


# the reference's defaults (models/drmnet.py:85, 104-106, 121) of the keys get_input / p_losses read
_VALIDATION_DEFAULTS = {"loss_type": "l1", "sigma": 0.01, "l_refmap_weight": 1.0, "l_refcode_weight": 1.0, "envmap_dir": None}


class DRMNet(nn.Module):
    """The reference's constructor surface.  ``loss_type``, ``sigma``, ``l_refmap_weight``, ``l_refcode_weight`` and ``envmap_dir`` are kept
    in the dict ``validation_params`` under their own names (not as attributes of those names: the module keeps the attribute surface of the
    sampling path it had).  ``cache_refmap`` / ``refmap_cache_root`` stay accepted and unused: a reflectance map is one deterministic kernel
    launch here, cheaper than reading a .pt file back, so nothing is cached."""

    def __init__(self, illnet_config, refnet_config, renderer_config=None, max_timesteps: int = 250, *, ckpt_path: Optional[str] = None,
                 init_from_ckpt_verbose: bool = True, ignore_keys=(), use_ema: bool = True, input_key: str = "LrK", sigma_for_cond_xK: float = 0.0,
                 image_size: int = 128, channels: int = 3, log_every_k: int = 5, parameterization: str = "residual", concat_mode: bool = False,
                 conditioning_key: Optional[str] = None, scale_factor: float = 1.0, scale_by_std: bool = False, delta: float = 0.0125,
                 gamma: float = 0.9, epsilon: float = 0.001, brdf_param_names=("specular",), z0=(1.0,), model_emb_z: bool = True,
                 emb_z_crossattn: bool = False, refmap_input_scaler: Optional[float] = None, first_stage_config=None,
                 cond_stage_config="__is_first_stage__", basis_r0: Union[torch.Tensor, str, None] = None, cond_stage_forward: Optional[str] = None,
                 **training_only):
        # (the leading four parameters keep the reference's positional order, models/drmnet.py:79-85: DRMNet(ill, ref, renderer_cfg, 250))
        super().__init__()
        unknown = sorted(set(training_only) - _TRAINING_ONLY)
        if unknown:
            raise TypeError(f"DRMNet: unexpected parameter(s) {unknown}")
        if parameterization != "residual":
            raise NotImplementedError('only the "residual" parameterization exists (models/drmnet.py:121)')
        if not concat_mode:
            raise AssertionError("This model only supports concat mode")
        if scale_by_std:
            raise NotImplementedError("scale_by_std is training-only")
        if cond_stage_forward is not None:
            # the reference reads it in get_learned_conditioning on the sampling path (models/drmnet.py:366-373): a config that sets it must
            # not silently behave differently
            raise NotImplementedError("cond_stage_forward: only the default (cond_stage_model.encode of the identity first stage) is on the shipped path")
        if cond_stage_config not in ("__is_first_stage__", "__is_unconditional__"):
            raise NotImplementedError("a separate cond_stage_config is not on the shipped path")
        # sampler constants (models/drmnet.py:782-847 reads them per step) and estimate.py's attribute surface
        self.parameterization = parameterization
        self.max_timesteps, self.gamma, self.epsilon, self.delta = max_timesteps, gamma, epsilon, delta
        self.log_every_k, self.input_key, self.sigma_for_cond_xK = log_every_k, input_key, sigma_for_cond_xK
        self.image_size, self.channels, self.scale_factor = image_size, channels, scale_factor
        self.brdf_param_names = list(brdf_param_names)
        self.refmap_input_scaler = refmap_input_scaler
        self.validation_params = {k: training_only.get(k, d) for k, d in _VALIDATION_DEFAULTS.items()}
        self.concat_mode = concat_mode
        self._z0 = torch.tensor(list(z0), dtype=torch.float32)
        self.zdim = len(self._z0)
        self.register_buffer("z0", self._z0)
        self.instantiate_brdf_model(renderer_config, basis_r0)
        # the two networks behind the reference's wrappers (state_dict keys illnet_model.* / refnet_model.* [+ *_ema.*])
        if conditioning_key is None:
            conditioning_key = "concat"
        if cond_stage_config == "__is_unconditional__":
            conditioning_key = None
        self.illnet_model = ZEmbDiffusionWrapper(illnet_config, conditioning_key, self.zdim, model_emb_z, emb_z_crossattn)
        self.refnet_model = DiffusionWrapper(refnet_config, conditioning_key)
        self.use_ema = use_ema
        if use_ema:
            self.illnet_model_ema = LitEma(self.illnet_model)
            self.refnet_model_ema = LitEma(self.refnet_model)
        self.first_stage_model = instantiate_from_config(first_stage_config or {"target": "ldm.models.autoencoder.IdentityFirstStage"}).eval()
        if not isinstance(self.first_stage_model, IdentityFirstStage):
            raise NotImplementedError("only IdentityFirstStage is used by the shipped configs")
        self.cond_stage_model = self.first_stage_model if cond_stage_config == "__is_first_stage__" else None
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=list(ignore_keys), verbose=init_from_ckpt_verbose)
        self.eval()
        self._samplers = {}  # weight set ("live" / "ema") -> (drm_drmnet handle, signature it was built from)
        self._weight_set = "live"
        self._ws = _lib.Workspace()

    # ------------------------------------------------------------------ plumbing kept from the reference
    @property
    def device(self):
        return self.z0.device

    def instantiate_brdf_model(self, config, basis_r0=None):
        """The reference renders basis_r0 (white envmap, BRDF z0) at construction (drmnet.py:328-347).  Here basis_r0 is ones by default
        (None), a tensor the caller supplies, or "render": the basis rendered from z0 by csrc/render.hip on first GPU use (r0toenvmap,
        reconstruct or render_basis_r0()) -- construction never touches the GPU.  For the shipped z0 = [1, 1, 1, 1, 0, 1] (white, fully
        metallic, roughness 0) the rendered basis is 1 on the sphere up to the grazing rim, so ones is its noise-free value; any other z0
        needs the rendered basis (first screen)."""
        self.renderer = instantiate_from_config(config) if config is not None else None
        self._basis_pending = isinstance(basis_r0, str)
        if self._basis_pending and basis_r0 != "render":
            raise ValueError(f'basis_r0 must be None, a tensor or "render", got {basis_r0!r}')
        if basis_r0 is None or self._basis_pending:
            basis_r0 = torch.ones(3, self.image_size, self.image_size)
        self.register_buffer("basis_r0", basis_r0.float(), persistent=False)

    def _renderer(self):
        """The reflectance-map renderer: the configured one, else one at image_size made on first use."""
        from .render import RefMapRenderer

        if self.renderer is None:
            self.renderer = RefMapRenderer(self.image_size, brdf_param_names=self.brdf_param_names)
        if not isinstance(self.renderer, RefMapRenderer):
            raise NotImplementedError(f"rendering needs drmnet_amd.render.RefMapRenderer, not {type(self.renderer).__name__}")
        return self.renderer

    @torch.no_grad()
    def render_basis_r0(self) -> torch.Tensor:
        """drmnet.py:328-347: basis_r0 = the reflectance map of z0 under a white environment at image_size x image_size ([3, S, S]),
        rendered on the model's GPU and stored in the basis_r0 buffer."""
        if not self.z0.is_cuda:
            raise RuntimeError("render_basis_r0 renders on the GPU: move the model there first (drmnet_amd has no CPU path)")
        basis = self._renderer().render(self.z0[None], self.brdf_param_names, None, res=self.image_size)[0]
        self.basis_r0 = basis.contiguous()
        self._basis_pending = False
        return self.basis_r0

    @torch.no_grad()
    def rendering_refmaps(self, envmaps, z: torch.Tensor, brdf_param_names=None, transform: bool = True, view_from=None,
                          new_scene: bool = False) -> torch.Tensor:
        """drmnet.py:667-696: envmaps [B, H, W, 3], z [L, B, P], view_from [B, 3] or None (+z) -> reflectance maps [L, B, 3, R, R], every
        (list, batch) item under envmaps[b] seen from view_from[b] -- one drm_render_refmap launch; the L rows of an item read the same
        map (no copies).  Envmap names (a list of str) are read from ``envmap_dir``."""
        assert len(envmaps) == z.size(1)
        if isinstance(envmaps, (list, tuple)):
            envmaps = self._load_envmaps(list(envmaps)).to(z.device if z.is_cuda else self.device)
        r = self._renderer()
        out = r.render(z, brdf_param_names or self.brdf_param_names, envmaps, view_from=view_from)
        if not new_scene:  # the scene keeps the last map and view it was given, as the reference's does
            r._envmap = envmaps[-1].to(out.device)
            if view_from is not None:
                r._view_from = torch.as_tensor(view_from)[-1].detach().to("cpu", torch.float32)
        return out

    def _load_envmaps(self, names) -> torch.Tensor:
        """envmap_dir/<name>.exr for every name, stacked [n, H, W, 3] on the host (drmnet.py:551-555, 685-689)."""
        from pathlib import Path

        from . import file_io

        root = self.validation_params["envmap_dir"]
        assert root is not None, "envmap_dir was needed, but was not specified"
        return torch.stack([file_io.load_exr(Path(root) / f"{name}.exr", as_torch=True) for name in names])

    def reconstruct(self, Lr_0: torch.Tensor, z: torch.Tensor, brdf_param_names=None, transform: bool = True) -> torch.Tensor:
        """drmnet.py:943-953: the estimate re-rendered -- Lr_0 (network space, [B, 3, S, S]) rescaled, warped to an envmap through
        basis_r0 (r0toenvmap), and rendered back through z [B, P] -> [B, 3, R, R]."""
        r0 = self.ds.rescale(Lr_0)
        envmap = self.r0toenvmap(r0, (self.image_size, self.image_size * 2))
        return self.rendering_refmaps(envmap, z[None], new_scene=True, brdf_param_names=brdf_param_names, transform=transform)[0]

    def get_visualized_brdf_grid(self, zs: torch.Tensor, brdf_param_names=None) -> np.ndarray:
        """drmnet.py:916-929: visualize_bsdf (128 x 128 spheres) of every row of zs [B, P], stacked -> [B * 128, 448, 3]."""
        from .render import get_bsdf, visualize_bsdf

        rows = [visualize_bsdf(get_bsdf(z, brdf_param_names or self.brdf_param_names), imsize=(128, 128))[0] for z in zs]
        return np.concatenate(rows, axis=0)

    def ema_scope(self, context=None):
        """models/drmnet.py:242-258 -- ``with model.ema_scope(): ...`` samples with the EMA weights of both networks (and of the
        z-embedding MLP, which lives in illnet_model); see wrappers.ema_weights."""
        pairs = [(self.illnet_model, self.illnet_model_ema), (self.refnet_model, self.refnet_model_ema)] if self.use_ema else []
        return ema_weights(self, pairs, context)

    def init_from_ckpt(self, path, ignore_keys=list(), only_model=False, verbose=True):
        """models/drmnet.py:260-277 (``only_model`` loads into illnet_model alone, as there)."""
        load_checkpoint(self, path, ignore_keys, into=self.illnet_model if only_model else None, verbose=verbose)

    @torch.no_grad()
    def encode_first_stage(self, x):
        return self.first_stage_model.encode(x)

    def get_first_stage_encoding(self, encoder_posterior):
        assert isinstance(encoder_posterior, torch.Tensor)
        return self.scale_factor * encoder_posterior

    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        z = 1.0 / self.scale_factor * z  # LatentDiffusion.decode_first_stage, ddpm.py:731-789 (identity first stage)
        return self.first_stage_model.decode(z)

    # ------------------------------------------------------------------ per-step pieces (reference semantics)
    def apply_model(self, model: DiffusionWrapper, input_refmap: torch.Tensor, k: Union[torch.Tensor, int], cond, rows=None):
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            key = "c_concat" if model.conditioning_key == "concat" else "c_crossattn"
            cond = {key: cond}
        if isinstance(k, int):
            n = input_refmap.size(0) if rows is None else rows.numel()
            k = torch.full((n,), k, device=input_refmap.device)
        return model(input_refmap, k, rows=rows, **cond)

    def get_schedule(self, zK, z0=None, reversed_k=None, normalized_k=None, return_zkm1=False, power_precision=torch.double):
        """models/drmnet.py:458-501.  The BRDF code decays geometrically from zK towards the mirror code z0: after ``r`` reverse
        steps the offset is gamma^r (zK - z0), with gamma^r evaluated as exp(r ln gamma) in ``power_precision`` (fp64) and cast to
        fp32 before the multiply.  K = int(log_gamma(epsilon / |zK - z0|)) + 2 is the step count at which the offset falls below
        epsilon.  Exactly one of ``reversed_k`` (steps done) / ``normalized_k`` (fraction of K) selects the point.
        Returns (K, k, zk[, zk one step later]).  Tiny [n, z_dim] host-side math; the sampler kernels restate the reversed_k branch."""
        if (normalized_k is None) == (reversed_k is None):
            raise AssertionError("normalized_k and reversed_k are exclusive")
        anchor = self.z0 if z0 is None else z0.to(zK.device)
        offset = zK - anchor
        ln_gamma = math.log(self.gamma)
        K = (torch.log(self.epsilon / torch.linalg.norm(offset, dim=-1)) / ln_gamma).int() + 2
        if normalized_k is None:
            k = K - reversed_k - 1
            steps = torch.tensor([reversed_k], device=zK.device) if isinstance(reversed_k, int) else reversed_k
        else:
            K = K.clip(min=1).int()
            k = (normalized_k * K).int()
            steps = K - k - 1
        steps = steps.to(power_precision)

        def code_after(r):
            return torch.exp(r.unsqueeze(-1) * ln_gamma).float() * offset + anchor

        if return_zkm1:
            return K, k, code_after(steps), code_after(steps + 1)
        return K, k, code_after(steps)

    def get_brdf_out(self, brdf_model_out, reversed_k=None):
        zK = brdf_model_out
        _, _, zk = self.get_schedule(zK, reversed_k=reversed_k)
        if not self.training:
            zk = zk.clamp(0, 1)
            zK = zK.clamp(0, 1)
        return zk, zK

    def check_convergence(self, zk):
        distance = torch.linalg.norm((zk - self.z0).abs(), dim=-1)
        return torch.logical_or(distance < self.epsilon, distance == 0)

    def forward(self, Lr_k, illnet_cond, refnet_cond, reversed_k):
        z_out = self.apply_model(self.refnet_model, Lr_k, reversed_k, refnet_cond)
        zk, _ = self.get_brdf_out(z_out, reversed_k=reversed_k)
        Delta = zk - self.z0
        return self.apply_model(self.illnet_model, Lr_k, Delta, illnet_cond), z_out

    def p_mean_variance(self, Lr_k, illnet_cond, refnet_cond, reversed_k, return_model_out=False):
        model_out, z_out = self(Lr_k, illnet_cond, refnet_cond, reversed_k)
        model_mean = Lr_k + model_out
        if return_model_out:
            return model_mean, self.delta, z_out, model_out
        return model_mean, self.delta, z_out

    def p_sample(self, Lr_k, illnet_cond, refnet_cond, reversed_k, return_model_out=False):
        raise NotImplementedError("")  # the reference leaves this unimplemented too (drmnet.py:772-780)

    def set_precision(self, precision: str, probe: Optional[torch.Tensor] = None) -> "DRMNet":
        """Conv arithmetic of both networks: "fp32" (exact fp32 MFMA), "f16x3" (split fp16, fp32-accurate, ~2.5x faster), "f16mx" (f16x3 with
        fp8 cross terms on the 3x3 convs: ~3e-5 per network, ~3x faster), "auto" (f16mx per network only where a probe forward on the loaded
        weights agrees with f16x3 to 5e-5, else f16x3: unet.set_precision_auto), "f16" / "bf16" (reduced precision)."""
        self.illnet_model.diffusion_model.set_precision(precision)
        self.refnet_model.diffusion_model.set_precision(precision)
        # "auto": besides the per-network probes (unet.py), the CHAIN is measured before f16mx is kept (autoprec.ChainProbe over _run_probe_chain)
        # ``probe`` [n,3,H,W]: refmaps of the CALLER to measure the chain on (the first and the middle row are used) instead of the seeded synthetic
        # pair; without it the first batch p_sample_loop sees is handed to the probe (once per weight signature)
        self._auto_chain = ChainProbe(self.AUTO_CHAIN_TOLERANCE, self.AUTO_CHAIN_STEPS, None if probe is None else _lib.require_gpu_tensor(probe, "probe").detach(),
                                      step_name="DRMNet steps", probe_text="{dims} {rows}, {steps} reverse steps, worst row") if precision == "auto" else None
        return self

    AUTO_CHAIN_TOLERANCE = 5e-5  # half the 1e-4 contract, like the per-network probe
    AUTO_CHAIN_STEPS = 8
    _auto_chain: Optional[ChainProbe] = None  # None outside auto mode (assigning None switches the chain probe off, the networks' modes stay)

    @property
    def auto_chain_report(self) -> Optional[dict]:
        """{"kept", "rel_l2_chain_vs_f16x3" (worst row), "steps", "tolerance", "modes"} of the last chain probe; None outside auto mode / before it ran"""
        return None if self._auto_chain is None else self._auto_chain.report

    def calibrate_precision(self, probe: Optional[torch.Tensor] = None) -> Optional[dict]:
        """Auto mode: runs the per-network probes and the chain probe now (weights on a GPU) and returns the chain report.  ``probe``: refmaps of the
        caller to run the chain on (re-measured for these rows even if a probe of these weights is on record)."""
        if self._auto_chain is not None and probe is not None:
            self._auto_chain.set_probe(_lib.require_gpu_tensor(probe, "probe").detach())
        self._engine()
        return self.auto_chain_report

    def _run_probe_chain(self, x: torch.Tensor) -> torch.Tensor:
        """The chain of autoprec.ChainProbe: eight reverse steps (RefNet -> schedule -> z-MLP -> IllNet -> update, Philox noise from a fixed key, every
        row active: drm_drmnet_step) from the refmaps ``x``, on the handle of the modes the networks are in when it runs."""
        (B, _, H, W), dev, L = x.shape, x.device, _lib.lib()
        h = self._engine_raw()
        ws = self._ws.get(int(L.drm_drmnet_workspace_bytes(h, B, H, W)), dev)
        Lr_k = x.clone()
        with torch.cuda.device(dev):
            for i in range(self._auto_chain.steps):
                _lib.check(L.drm_drmnet_step(h, Lr_k.data_ptr(), x.data_ptr(), None, B, i, None, 20261004, None, None, None, B, H, W, ws.data_ptr(),
                                             ws.numel(), _lib.stream_ptr(dev)))
        return Lr_k

    # ------------------------------------------------------------------ the device sampler
    def _engine(self, data: Optional[torch.Tensor] = None):
        """_engine_raw() behind the auto mode's chain probe (which may move both networks to f16x3 for the current weights); ``data``: the refmaps
        the caller is about to sample from -- the chain probe runs on rows of them (once per weight signature)."""
        h = self._engine_raw()
        if self._auto_chain is not None and not self._auto_chain.busy:
            ill, ref = self.illnet_model.diffusion_model, self.refnet_model.diffusion_model
            self._auto_chain.measure({"illnet": ill, "refnet": ref}, getattr(self, "_weight_set", "live"), self._run_probe_chain, data, next(ill.parameters()).device)
            h = self._engine_raw()
        return h

    def _engine_raw(self):
        """The device sampler handle for the weight set that is live right now ("live" parameters, or the EMA shadow inside
        ``ema_scope``): one handle per set, rebuilt only when something it was built from changes."""
        which = getattr(self, "_weight_set", "live")
        ill, ref = self.illnet_model.diffusion_model, self.refnet_model.diffusion_model
        hi, hr = ill.engine_handle(), ref.engine_handle()
        if which == "ema":
            zp = self.illnet_model_ema.shadow_for(self.illnet_model.z_emb_param_names())
        else:
            zp = [p.detach() for p in self.illnet_model.z_emb_params()]
        for p in zp:
            _lib.require_gpu_tensor(p, "z_emb_layer parameter")
        sig = (hi.value, hr.value, ill.precision, ref.precision, tensor_sig(zp), float(self.gamma), float(self.epsilon),
               float(self.delta), int(self.max_timesteps), tuple(self._z0.tolist()))
        cached = self._samplers.get(which)
        if cached is not None and cached[1] == sig:
            return cached[0]
        self._free_sampler(which)
        cfg = _lib.DrmnetCfg()
        cfg.z_dim = self.zdim
        cfg.max_timesteps = int(self.max_timesteps)
        cfg.gamma = float(self.gamma)
        cfg.epsilon = float(self.epsilon)
        cfg.delta = float(self.delta)
        for i, v in enumerate(self._z0.tolist()):
            cfg.z0[i] = v
        h = C.c_void_p()
        torch.cuda.current_stream(zp[0].device).synchronize()
        with torch.cuda.device(zp[0].device):
            _lib.check(_lib.lib().drm_drmnet_create(hi, hr, _lib.ptr_array(zp), C.byref(cfg), C.byref(h)))
        if getattr(self, "_batch_parts", None) is not None:
            _lib.check(_lib.lib().drm_drmnet_set_batch_parts(h, int(self._batch_parts)))
        if getattr(self, "_batch_part_min", None) is not None:
            _lib.check(_lib.lib().drm_drmnet_set_batch_part_min(h, int(self._batch_part_min)))
        self._samplers[which] = (h, sig)
        return h

    def set_batch_parts(self, parts: int, min_rows: int = None):
        """Row ranges a reverse step is forked into on internal streams (drm_drmnet_set_batch_parts; library default 2 from 64 rows per part, 1 = off).
        min_rows: rows per part from which the fork engages (drm_drmnet_set_batch_part_min; tests pass 1)."""
        self._batch_parts = int(parts)
        if min_rows is not None:
            self._batch_part_min = int(min_rows)
        for h, _ in getattr(self, "_samplers", {}).values():
            _lib.check(_lib.lib().drm_drmnet_set_batch_parts(h, int(parts)))
            if min_rows is not None:
                _lib.check(_lib.lib().drm_drmnet_set_batch_part_min(h, int(min_rows)))
        return self

    def _free_sampler(self, which=None):
        for k in ([which] if which else list(getattr(self, "_samplers", {}))):
            entry = self._samplers.pop(k, None)
            if entry is not None:
                _lib.lib().drm_drmnet_destroy(entry[0])

    def __del__(self):
        try:
            self._free_sampler()
        except Exception:
            pass

    @staticmethod
    def _one_cond(cond, LrK):
        c = cond[0] if isinstance(cond, (list, tuple)) else cond
        if isinstance(cond, (list, tuple)) and len(cond) != 1:
            raise NotImplementedError("one concat conditioning tensor expected")
        return _lib.require_gpu_tensor(c, "cond")

    @torch.no_grad()
    def p_sample_loop(self, Lr_K, illnet_cond, refnet_cond, return_intermediates=False, verbose=True, log_every_k=None,
                      noise0=None, step_noise=None, seed=None, early_exit=True):
        """drmnet.py:782-847.  Extra keyword-only knobs (not in the reference): ``noise0`` [B,3,H,W] and ``step_noise``
        [max_timesteps,B,3,H,W] inject the random draws (parity mode; row b of step_noise[i] is used by sample b iff it is
        still active and not converged at step i); otherwise noise comes from the library's Philox stream keyed by ``seed``
        (drawn from torch's generator when None).  ``early_exit=False`` keeps every sample active for max_timesteps steps.
        Returns (Lr_0, zK, K[, intermediates]) exactly as the reference."""
        log_every_k = log_every_k or self.log_every_k
        LrK = _lib.require_gpu_tensor(Lr_K, "Lr_K")
        dev = LrK.device
        cond = self._one_cond(illnet_cond, LrK)
        cond_r = self._one_cond(refnet_cond, LrK)
        if cond_r.data_ptr() != cond.data_ptr() and not torch.equal(cond_r, cond):
            raise NotImplementedError("illnet_cond and refnet_cond are the same tensor on the shipped path (drmnet.py:1043)")
        B, _, H, W = LrK.shape
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        noise0 = None if noise0 is None else _lib.require_gpu_tensor(noise0, "noise0")
        step_noise = None if step_noise is None else _lib.require_gpu_tensor(step_noise, "step_noise")
        if step_noise is not None and tuple(step_noise.shape) != (self.max_timesteps, B, 3, H, W):
            raise RuntimeError("step_noise must be [max_timesteps, B, 3, H, W]")
        h = self._engine(LrK)
        L = _lib.lib()
        ws = self._ws.get(int(L.drm_drmnet_workspace_bytes(h, B, H, W)), dev)
        Lr0 = torch.empty_like(LrK)
        zK = torch.empty((B, self.zdim), dtype=torch.float32, device=dev)
        K = torch.empty((B,), dtype=torch.int32, device=dev)
        if not return_intermediates:
            steps = C.c_int32(0)
            with torch.cuda.device(dev):
                _lib.check(L.drm_drmnet_sample(h, LrK.data_ptr(), cond.data_ptr(), _lib.ptr(noise0), _lib.ptr(step_noise), seed, int(bool(early_exit)),
                                               Lr0.data_ptr(), zK.data_ptr(), K.data_ptr(), C.byref(steps), B, H, W, ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(dev)))
            self.last_steps = int(steps.value)
            return Lr0, zK, K
        # intermediates requested: drive the loop from the host, one drm_drmnet_step per iteration (same kernels)
        from . import ops

        n0 = noise0 if noise0 is not None else ops.randn(LrK.shape, seed, 0, dev)
        Lr_k = LrK + self.delta * n0
        intermediates = {"Lrk_inter": [Lr_k.clone()], "zk_inter": []}
        zK.fill_(float("nan"))
        K.fill_(self.max_timesteps)
        active = torch.arange(B, dtype=torch.int32, device=dev)
        for i in range(self.max_timesteps):
            n = active.numel()
            zk = torch.empty((n, self.zdim), device=dev)
            zKc = torch.empty((n, self.zdim), device=dev)
            conv = torch.empty((n,), dtype=torch.int32, device=dev)
            nz = None if step_noise is None else step_noise[i]
            with torch.cuda.device(dev):
                _lib.check(L.drm_drmnet_step(h, Lr_k.data_ptr(), cond.data_ptr(), active.data_ptr(), n, i, _lib.ptr(nz), seed, zk.data_ptr(),
                                             zKc.data_ptr(), conv.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
            if i % log_every_k == 0:
                z_log = torch.full((B, self.zdim), float("nan"), device=dev)
                z_log[active.long()] = zk
                intermediates["zk_inter"].append(z_log)
                Lr_log = torch.zeros_like(Lr_k)
                Lr_log[active.long()] = Lr_k[active.long()]
                intermediates["Lrk_inter"].append(Lr_log)
            if early_exit:
                cb = conv.bool()
                done = active[cb].long()
                K[done] = i + 1
                zK[done] = zKc[cb]
                active = active[~cb].contiguous()
                if active.numel() == 0:
                    break
        return Lr_k, zK, K, intermediates

    # ------------------------------------------------------------------ the validation pass (forward process + losses)
    def get_loss(self, pred: torch.Tensor, target: torch.Tensor, mean=True):
        """drmnet.py:398-411 on torch tensors (the validation pass itself reduces on the device through ops.validation_losses)."""
        loss_type = self.validation_params["loss_type"]
        if loss_type == "l1":
            loss = (target - pred).abs()
        elif loss_type == "l2":
            loss = (target - pred) ** 2
        else:
            raise NotImplementedError(f"unknown loss type '{loss_type}'")
        return loss.mean() if mean else loss

    @torch.no_grad()
    def p_losses(self, Lr_k, Lr_km1, z_k, z_K, K, k, illnet_cond, refnet_cond, *, noise=None, seed=None):
        """drmnet.py:413-450 in eval mode: the forward noise (sigma > 0: ``noise`` [B, 3, H, W] if given, else the library's Philox stream
        keyed by ``seed``, drawn from torch's generator when None), one pass of both networks at each row's own reversed_k = K - k - 1, and
        the three losses from drm_validation_losses.  Returns (loss, {"val/loss_refmap", "val/loss_refcode", "val/loss"}), 0-dim device
        tensors.  There is no backward on this engine: training mode raises."""
        from . import ops

        if self.training:
            raise NotImplementedError("p_losses in training mode: the HIP engine has no backward (validation only)")
        vp = self.validation_params
        Lr_k = _lib.require_gpu_tensor(Lr_k, "Lr_k")
        dev = Lr_k.device
        K, k = K.to(dev), k.to(dev)
        reversed_k = K - k - 1
        if vp["sigma"] > 0:
            if noise is None:
                if seed is None:
                    seed = int(torch.randint(0, 2**62, (1,)).item())
                noise = ops.randn(Lr_k.shape, seed, 0, dev)
            Lr_k = Lr_k + vp["sigma"] * _lib.require_gpu_tensor(noise, "noise")
        model_out, z_out = self(Lr_k, illnet_cond, refnet_cond, reversed_k.long())
        out = ops.validation_losses(model_out, Lr_k, Lr_km1.to(dev), K, z_out, z_k.to(dev), z_K.to(dev), reversed_k, self.z0, self.gamma,
                                    vp["loss_type"], vp["l_refmap_weight"], vp["l_refcode_weight"])
        return out[2], {"val/loss_refmap": out[0], "val/loss_refcode": out[1], "val/loss": out[2]}

    @torch.no_grad()
    def get_input(self, batch, return_Lr_zero=False, return_envmap=False, return_envmap_name=False, return_view_from=False,
                  bs: Optional[int] = None):
        """drmnet.py:503-651: the first ``bs`` items of a ParametricRefmapDataset batch -> [K, k, Lr_K, Lr_k, Lr_km1, zK, zk, illnet_c,
        refnet_c(, Lr_0)(, envmap)(, envmap_name)(, view_from)].  A reflectance map the batch brings ("LrK", "Lrk", "Lrkm1", "r0") with a
        finite [b, 0, 0, 0] is used as it is; every other one is rendered from its code of the stack (zK, zk, zkm1[, z0]) under
        batch["envmap"][b] (read from envmap_dir/<name>.exr where missing or NaN-marked) seen from batch["view_from"][b], all of them in one
        drm_render_refmap launch (a NaN code, zkm1 where K == 0, gives a NaN map).  Then the exposure scale of LrK (``normalizing_scale``) is applied to every map, then
        ``ds.transform``.  Nothing is written to a refmap cache."""
        from . import ops

        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("get_input runs on the GPU: move the model there first (drmnet_amd has no CPU path)")
        zK = batch["zK"]
        bs = min(len(zK), bs) if bs is not None else len(zK)
        self.batch_size = bs
        zK = zK[:bs].to(dev, torch.float32)
        envmap_name = list(batch["envmap_name"][:bs])
        view_from = batch.get("view_from")[:bs]
        K, k = batch["K"][:bs].to(dev), batch["k"][:bs].to(dev)
        zk, zkm1 = batch["zk"][:bs].to(dev, torch.float32), batch["zkm1"][:bs].to(dev, torch.float32)
        keys, codes = ["LrK", "Lrk", "Lrkm1"], [zK, zk, zkm1]
        if return_Lr_zero:
            keys.append("r0")
            codes.append(self.z0[None].expand(bs, -1))
        stacked_z = torch.stack(codes)  # [L, B, P]
        res = self._renderer().refmap_res
        given = [batch[key][:bs].to(dev, torch.float32) if key in batch else None for key in keys]
        not_cached = torch.stack([torch.ones(bs, dtype=torch.bool, device=dev) if r is None else torch.isnan(r[:, 0, 0, 0]) for r in given])
        envmap = None
        if bool(not_cached.any()):
            rows = torch.nonzero(not_cached.any(dim=0)).flatten().tolist()  # the batch items with something to render
            have = batch["envmap"][:bs] if "envmap" in batch else None
            load = [b for b in rows if have is None or bool(torch.isnan(have[b, 0, 0, 0]))]
            loaded = self._load_envmaps([envmap_name[b] for b in load]) if load else None
            if have is None:
                envmap = torch.full((bs, *loaded.shape[1:]), float("nan"))
            else:
                envmap = have.clone() if load else have
            for b, em in zip(load, loaded if load else ()):
                envmap[b] = em.to(envmap.device)
            envmap = envmap.to(dev, torch.float32)
            all_rows = len(rows) == bs
            pick = None if all_rows else torch.tensor(rows, device=dev)
            rendered = self._renderer().render(stacked_z if all_rows else stacked_z[:, pick], self.brdf_param_names,
                                               envmap if all_rows else envmap[pick], res=res,
                                               view_from=view_from if all_rows else torch.as_tensor(view_from)[rows])
            stacked_Lr = []
            for l, r in enumerate(given):
                full = rendered[l] if all_rows else torch.full((bs, 3, res, res), float("nan"), device=dev).index_copy_(0, pick, rendered[l])
                # a code that is not a number (zkm1 where K == 0) has no reflectance map: NaN, as the item's Lrkm1 says, not a render of clipped NaNs
                full = torch.where(torch.isnan(stacked_z[l]).any(dim=-1)[:, None, None, None], float("nan"), full)
                stacked_Lr.append(full if r is None else torch.where(not_cached[l][:, None, None, None], full, r))
        else:
            stacked_Lr = given
        if self.refmap_input_scaler is not None:
            self.normalizing_scale = ops.luminance_scale(stacked_Lr[0].contiguous(), self.refmap_input_scaler)
            stacked_Lr = [ops.map_chain(Lr.contiguous(), [("img_mul", 0.0)], scale=self.normalizing_scale) for Lr in stacked_Lr]
        stacked_Lr = [self.get_first_stage_encoding(self.encode_first_stage(self.ds.transform(Lr))) for Lr in stacked_Lr]
        Lr_K, Lr_k, Lr_km1 = stacked_Lr[:3]
        cond_LrK = Lr_K if self.sigma_for_cond_xK <= 0 else self.sigma_for_cond_xK * torch.randn_like(Lr_K) + Lr_K
        illnet_c = [cond_LrK]
        out = [K, k, Lr_K, Lr_k, Lr_km1, zK, zk, illnet_c, illnet_c]
        if return_Lr_zero:
            out.append(stacked_Lr[3])
        if return_envmap:
            out.append(envmap)
        if return_envmap_name:
            out.append(batch["envmap_name"][:bs])
        if return_view_from:
            out.append(view_from)
        return out

    def shared_step(self, batch, *, seed=None):
        """drmnet.py:707-710 (``seed`` keys the forward noise of p_losses)."""
        K, k, Lr_K, Lr_k, Lr_km1, zK, zk, illnet_c, refnet_c = self.get_input(batch)
        return self.p_losses(Lr_k, Lr_km1, zk, zK, K, k, illnet_c, refnet_c, seed=seed)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx, *, seed=None):
        """drmnet.py:731-740: the losses on the live weights and, under ema_scope, on the EMA weights (keys + "_ema").  The reference logs
        the two dicts; there is no logger here, so the merged six-key dict is returned (0-dim device tensors).  ``seed``: the forward noise
        of the live pass is keyed by it, that of the EMA pass by seed + 1 (the reference draws twice from one generator)."""
        _, loss_dict = self.shared_step(batch, seed=seed)
        with self.ema_scope():
            _, loss_dict_ema = self.shared_step(batch, seed=None if seed is None else seed + 1)
        merged = dict(loss_dict)
        merged.update({key + "_ema": v for key, v in loss_dict_ema.items()})
        return merged

    # ------------------------------------------------------------------ estimate.py glue
    @torch.no_grad()
    def get_input_for_predict(self, batch, bs: Optional[int] = None):
        """models/drmnet.py:1011-1045: the first ``bs`` refmaps are exposure-normalised (each scaled so the geometric mean of its
        luminance over lit pixels equals ``refmap_input_scaler``; the factors are kept in ``self.normalizing_scale`` for the way
        back, scripts/estimate.py:99-100), mapped to network space by ``ds.transform`` and returned with the conditioning lists
        of the two networks (the same tensor, optionally jittered by ``sigma_for_cond_xK``).  The luminance reduction and the
        scale + log map run as two HIP launches (csrc/transform.hip)."""
        from . import ops

        src = batch[self.input_key]
        n = len(src) if bs is None else min(len(src), bs)
        scaled = self.refmap_input_scaler is not None

        def to_network_space(x):
            x = _lib.require_gpu_tensor(x[:n], self.input_key)
            if scaled:
                x = ops.map_chain(x, [("img_mul", 0.0)], scale=self.normalizing_scale)
            return self.ds.transform(x)

        if scaled:
            self.normalizing_scale = ops.luminance_scale(_lib.require_gpu_tensor(src[:n], self.input_key), self.refmap_input_scaler)
        LrK = self.get_first_stage_encoding(self.encode_first_stage(to_network_space(src)))
        Lr0 = to_network_space(batch["Lr0"]) if batch.get("Lr0") is not None else None
        cond = LrK if self.sigma_for_cond_xK <= 0 else self.sigma_for_cond_xK * torch.randn_like(LrK) + LrK
        illnet_c = [cond]
        return LrK, Lr0, illnet_c, illnet_c, batch["tag"][:n]

    def r0toenvmap(self, r0: torch.Tensor, envshape: Optional[Tuple[int]] = None) -> torch.Tensor:
        """models/drmnet.py:931-941: r0 / basis_r0, warped from the mirror-ball parametrisation to a lat-long map, channels last
        ([B, H, W, 3]) -- one HIP gather kernel (division fused into the fetch)."""
        from . import ops

        if envshape is None:
            envshape = (self.image_size, self.image_size * 2)
        if self._basis_pending:
            self.render_basis_r0()
        return ops.mirmap2envmap(r0, envshape, basis=self.basis_r0.to(r0.device), channels_last=True)

"""Host-side mirror of the reference U-Net modules, backed by the HIP engine.

Drop-in for ``ldm.modules.diffusionmodules.openaimodel.UNetModel`` /
``EncoderUNetModel`` (reference openaimodel.py:422-768, :771-991): same constructor
parameters, same ``state_dict()`` keys/shapes/order (so reference checkpoints and EMA
buffers load unchanged), same ``forward`` signatures.  The modules hold only
``nn.Parameter`` storage; all arithmetic runs in libdrmnet_hip.so on the tensors'
device.  There is no PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from .autoprec import ProbeState, tensor_sig, worst_row_rel_l2

_ZERO_INIT_SUFFIXES = (".out_layers.3.weight", ".out_layers.3.bias", ".proj_out.weight", ".proj_out.bias")


def _reject_unsupported(kind: str, **kw) -> None:
    """Only the configuration space the shipped YAMLs use is implemented."""
    bad = []
    if kw.get("use_spatial_transformer"):
        bad.append("use_spatial_transformer=True")
    if kw.get("context_dim") is not None:
        bad.append("context_dim")
    if kw.get("resblock_updown"):
        bad.append("resblock_updown=True")
    if kw.get("conv_resample", True):
        bad.append("conv_resample=True (the shipped configs set False)")
    if kw.get("use_scale_shift_norm"):
        bad.append("use_scale_shift_norm=True")
    if kw.get("dims", 2) != 2:
        bad.append("dims != 2")
    if kw.get("use_fp16"):
        bad.append("use_fp16=True")
    if kw.get("num_classes") is not None:
        bad.append("num_classes")
    if kw.get("num_heads", 1) not in (1,) or kw.get("num_head_channels", -1) != -1:
        bad.append("num_heads != 1 / num_head_channels")
    if kw.get("num_heads_upsample", -1) not in (-1, 1):
        bad.append("num_heads_upsample")
    if kw.get("use_new_attention_order"):
        bad.append("use_new_attention_order=True")
    if kw.get("use_positional_embedded_attention"):
        bad.append("use_positional_embedded_attention=True")
    if kw.get("n_embed") is not None:
        bad.append("n_embed")
    if kw.get("dropout", 0) not in (0, 0.0):
        bad.append("dropout != 0 (inference only)")
    if kind == "encoder" and kw.get("pool", "adaptive") != "adaptive":
        bad.append("pool != 'adaptive'")
    if bad:
        raise NotImplementedError(f"drmnet_amd {kind}: unsupported parameters: " + ", ".join(bad))


class _Holder(nn.Module):
    """Pure parameter container; never called."""


def _attach(root: nn.Module, key: str, param: nn.Parameter) -> None:
    parts = key.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, _Holder())
        m = m._modules[p]
    m.register_parameter(parts[-1], param)


class _HipUNetBase(nn.Module):
    _kind = 0

    def _setup(self, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, channel_mult):
        self.in_channels = int(in_channels)
        self.model_channels = int(model_channels)
        self.out_channels = int(out_channels)
        self.num_res_blocks = int(num_res_blocks)
        self.attention_resolutions = [int(a) for a in attention_resolutions]
        self.channel_mult = [int(m) for m in channel_mult]
        self.dtype = torch.float32
        d = _lib.UNetDesc()
        d.kind = self._kind
        d.in_channels, d.model_channels, d.out_channels = self.in_channels, self.model_channels, self.out_channels
        d.num_res_blocks = self.num_res_blocks
        if len(self.channel_mult) > _lib.MAX_LEVELS or len(self.attention_resolutions) > _lib.MAX_LEVELS:
            raise NotImplementedError("more than 8 levels")
        d.n_levels = len(self.channel_mult)
        for i, m in enumerate(self.channel_mult):
            d.channel_mult[i] = m
        d.n_attn = len(self.attention_resolutions)
        for i, a in enumerate(self.attention_resolutions):
            d.attention_resolutions[i] = a
        L = _lib.lib()
        h = C.c_void_p()
        _lib.check(L.drm_unet_create(C.byref(d), C.byref(h)))
        self._h = h
        self._ws = _lib.Workspace()
        # engine-side weight sets (include/drmnet_hip.h "Weight sets"): 0 = this module's parameters, 1 = an EMA shadow
        self._set_sig = {"live": None, "ema": None}
        self._active_set = "live"
        self._ema_source: Optional[List[torch.Tensor]] = None
        self.precision = "fp32"
        self._auto: Optional[ProbeState] = None  # set in auto mode (autoprec.py)
        # parameter table straight from the engine == reference state_dict() order
        n = L.drm_unet_param_count(h)
        self._keys: List[str] = []
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            _lib.check(L.drm_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
            key = name.value.decode()
            shp = tuple(int(shape[k]) for k in range(nd.value))
            _attach(self, key, nn.Parameter(self._init_tensor(key, shp), requires_grad=False))
            self._keys.append(key)

    @staticmethod
    def _init_tensor(key: str, shape: Tuple[int, ...]) -> torch.Tensor:
        if key.endswith(_ZERO_INIT_SUFFIXES) or key.startswith(("out.2.", "out.3.")):
            return torch.zeros(shape)  # zero_module(...) in the reference (openaimodel.py:229-231,314,706,927)
        if len(shape) >= 2:
            bound = 1.0 / math.sqrt(max(1, int(torch.tensor(shape[1:]).prod())))
            return torch.empty(shape).uniform_(-bound, bound)
        return torch.ones(shape) if key.endswith("weight") else torch.zeros(shape)

    def __del__(self):
        try:  # (at interpreter shutdown module globals may already be gone)
            h = self.__dict__.get("_h")
            if h is not None and h.value:
                _lib.lib().drm_unet_destroy(h)
                self.__dict__["_h"] = None
        except Exception:
            pass

    # ------------------------------------------------------------------ arithmetic mode
    PRECISIONS = {"fp32": 0, "f16x3": 1, "f16": 2, "f16mx": 3, "bf16": 4}

    def set_precision(self, precision: str) -> "._HipUNetBase":
        """"fp32": exact fp32 products on v_mfma_f32_32x32x2_f32 (default).
        "f16x3": fp32 operands split into fp16 hi+lo, 3 MFMAs per product, fp32 accumulation (fp32-level accuracy,
        16/3 x the fp32 matrix rate).
        "f16mx": f16x3 with the GroupNorm-fed 3x3 convs on fp16 hi*hi + one block-scaled fp8 MFMA for both cross terms (2/3 of the matrix-pipe
        cycles; 2.4e-5 .. 4e-5 rel-L2 per network against the reference: inside the 1e-4 contract, tests/test_gpu_f16mx.py).
        "f16" / "bf16": REDUCED precision (fp16 / bf16 operands, ~1e-3 / ~1e-2; bf16 is BASELINE configs[2] as written).  Weights are
        re-packed on the next forward."""
        if precision == "auto":
            return self.set_precision_auto()
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {list(self.PRECISIONS) + ['auto']}")
        self._auto = None
        return self._set_mode(precision)

    def _set_mode(self, precision: str) -> "._HipUNetBase":
        _lib.check(_lib.lib().drm_unet_set_precision(self._h, self.PRECISIONS[precision]))
        self.precision = precision
        self._set_sig = {"live": None, "ema": None}
        return self

    # "auto": f16mx only where it demonstrably holds.  f16mx carries about twenty times the rounding noise of exact fp32 (its cross terms keep four
    # significant bits); on the shipped architectures with O(1) GroupNorm gains that is 2e-5 .. 4e-5 per network, but a network that amplifies rounding
    # noise -- GroupNorm gains x 10 take RefNet from 3e-6 to 9e-4 (tests/test_gpu_auto_precision.py) -- leaves the 1e-4 contract in f16mx while f16x3 stays at
    # 1e-5.  So the choice is MEASURED on the weights actually loaded: a seeded probe batch in f16x3 and in f16mx -- two refmap-like inputs x three
    # timesteps / embeddings spread over the schedule, six rows at 128x128, a batch that runs the kernels of production batches (GroupNorm tables from
    # their own launch, the conv-pipeline attention) rather than the sparse-launch forms of a single image; f16mx is kept only if EVERY row agrees with
    # f16x3 to `tolerance` (default 5e-5, half the contract), otherwise the network runs in f16x3.  Re-measured when the weights change; the reports are
    # kept per (weight set, weight signature), so entering / leaving ema_scope does not repeat a measurement.  The model classes add a chain probe on
    # top (DRMNet: eight reverse steps; ObsNet: eight DDIM steps).  The protocol of both layers (state, signature, worst-row figure, the chain probe's
    # records and override) is autoprec.py; _auto_resolve below keeps what is this network's own: its probe batch and its forward.
    AUTO_TOLERANCE = 5e-5
    AUTO_PROBE_HW = (128, 128)

    def set_precision_auto(self, tolerance: Optional[float] = None, probe_hw: Optional[Tuple[int, int]] = None) -> "._HipUNetBase":
        self._auto = ProbeState(self.AUTO_TOLERANCE if tolerance is None else tolerance, self.AUTO_PROBE_HW if probe_hw is None else probe_hw)
        if self.precision not in ("f16x3", "f16mx"):
            self._set_mode("f16x3")  # (until the first forward has weights on a GPU to measure with)
        return self

    @property
    def auto_report(self) -> Optional[dict]:
        """{"chosen", "rel_l2_f16mx_vs_f16x3" (worst row), "rows", "tolerance", "probe"} of the last calibration, or None (not in auto mode / not yet measured)"""
        return None if self._auto is None else self._auto.report

    @property
    def auto_sig(self) -> Optional[tuple]:  # signature of the weights ``auto_report`` was measured on: a model's chain probe keys its records by it
        return None if self._auto is None else self._auto.sig

    def calibrate_precision(self) -> Optional[dict]:
        """Runs the auto-mode measurement now (weights must be on a GPU) and returns its report; None outside auto mode."""
        self._auto_resolve()
        return self.auto_report

    def auto_override(self, mode: str, why: str) -> None:
        """A model-level chain probe (DRMNet / ObsNet calibrate_precision) overrules the per-network choice for the current weights."""
        a = self._auto
        if a is None or a.report is None:
            return
        a.report = dict(a.report, chosen=mode, overridden_by=why)
        a.cache[(self._active_set, a.sig)] = a.report
        if self.precision != mode:
            self._set_mode(mode)

    @torch.no_grad()
    def _auto_resolve(self) -> None:
        a = self._auto
        if a is None or a.busy:
            return
        ps = self.param_tensors() if self._active_set == "live" else self._ema_source
        if not ps or not ps[0].is_cuda:
            return
        sig = tensor_sig(ps)
        if sig == a.sig:
            return
        known = a.cache.get((self._active_set, sig))
        if known is not None:  # measured before on exactly these tensors (live <-> EMA toggling)
            a.sig, a.report = sig, known
            if self.precision != known["chosen"]:
                self._set_mode(known["chosen"])
            return
        a.busy = True
        try:
            from . import synth

            dev = ps[0].device
            h, w = a.probe_hw
            down = 2 ** (len(self.channel_mult) - 1)
            h, w = max(down, h // down * down), max(down, w // down * down)
            gen = torch.Generator().manual_seed(20261003)
            n_in, n_t = 2, 3
            if self.in_channels == 6:  # [noised refmap | conditioning refmap], what all three shipped networks see
                ref = synth.synth_refmaps(n_in, h, w, 4321)
                x2 = torch.cat([ref + 0.025 * torch.randn(ref.shape, generator=gen), ref], 1)
            else:
                x2 = torch.randn((n_in, self.in_channels, h, w), generator=gen)
            x = x2.repeat_interleave(n_t, 0).contiguous().to(dev)  # rows: (input 0, t0..t2), (input 1, t0..t2)
            if self._kind == 0:  # embeddings of three magnitudes (IllNet's z-embedding shrinks along the chain; ObsNet's sinusoid is O(1))
                t_emb = (torch.randn((n_in * n_t, self.model_channels), generator=gen) * torch.tensor([0.5, 1.0, 2.0]).repeat(n_in)[:, None]).to(dev)
                ts = None
            else:
                t_emb = None
                ts = torch.tensor([1, 60, 140] * n_in, dtype=torch.int64, device=dev)
            outs = {}
            for mode in ("f16x3", "f16mx"):
                self._set_mode(mode)
                outs[mode] = self._run(x, None, t_emb, ts).double().flatten(1)
            err, rows = worst_row_rel_l2(outs["f16mx"], outs["f16x3"])
            chosen = "f16mx" if err <= a.tolerance and bool(torch.isfinite(outs["f16mx"]).all()) else "f16x3"
            self._set_mode(chosen)
            a.sig = sig
            a.report = {"chosen": chosen, "rel_l2_f16mx_vs_f16x3": err, "rows": [float(f"{r:.3e}") for r in rows], "tolerance": a.tolerance,
                           "probe": f"{n_in * n_t}x{self.in_channels}x{h}x{w}: {n_in} seeded refmap-like inputs x {n_t} timesteps / embeddings, worst row"}
            a.cache[(self._active_set, sig)] = a.report
        finally:
            a.busy = False

    # ------------------------------------------------------------------ weights
    def param_tensors(self) -> List[torch.Tensor]:
        # the Parameter objects are stable (load_state_dict copies in place, .to() / .cuda() swap their .data): looked up once
        ps = self.__dict__.get("_param_list")
        if ps is None or len(ps) != len(self._keys):
            sd = dict(self.named_parameters())
            ps = [sd[k] for k in self._keys]
            self.__dict__["_param_list"] = ps
        return ps

    def _apply(self, fn, *args, **kwargs):  # .to() / .cuda() / .float(): drop the memoised parameter list with the old storage
        self.__dict__.pop("_param_list", None)
        return super()._apply(fn, *args, **kwargs)

    SETS = {"live": 0, "ema": 1}

    def use_weights(self, which: str, tensors: Optional[Sequence[torch.Tensor]] = None) -> None:
        """Selects the packed weight image the next forwards read.  "live" = this module's own parameters; "ema" = ``tensors``
        (the LitEma shadow buffers in parameter order).  Each image is packed once and re-packed only when its source tensors
        change (storage or in-place version), so ``ema_scope`` enter / exit moves no weights -- the engine-side answer to the
        reference's copy-in / copy-back (ldm/modules/ema.py:46-76)."""
        if which not in self.SETS:
            raise ValueError(f"weight set must be one of {list(self.SETS)}")
        if which == "ema":
            if tensors is None or len(tensors) != len(self._keys):
                raise RuntimeError("use_weights('ema') needs one shadow tensor per parameter, in parameter order")
            self._ema_source = list(tensors)
        self._active_set = which

    def sync_weights(self, force: bool = False) -> None:
        """Makes the engine's active weight image current: (re)packs it when its source tensors changed (load_state_dict,
        .to(device), an optimizer step, a new EMA shadow) and selects it."""
        self._auto_resolve()
        which = self._active_set
        ps = self.param_tensors() if which == "live" else self._ema_source
        sig = (self.precision,) + tensor_sig(ps)
        L = _lib.lib()
        if force or sig != self._set_sig[which]:
            dev = ps[0].device
            for k, p in zip(self._keys, ps):
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                    raise RuntimeError(f"parameter {k} must be a contiguous fp32 tensor on one GPU (got {p.device}, {p.dtype}); call .cuda() first")
            arr = _lib.ptr_array(ps)
            with torch.cuda.device(dev):
                _lib.check(L.drm_unet_load_params_set(self._h, self.SETS[which], arr, len(ps), _lib.stream_ptr(dev)))
            self._set_sig[which] = sig
        _lib.check(L.drm_unet_use_set(self._h, self.SETS[which]))

    def engine_handle(self):
        self.sync_weights()
        return self._h

    def workspace_bytes(self, n: int, h: int, w: int) -> int:
        """Arena size of one forward (a sizing pass of the whole schedule inside the library): memoised per (shape, precision)."""
        key = (n, h, w, self.precision)
        cache = self.__dict__.setdefault("_ws_bytes", {})
        if key not in cache:
            cache[key] = int(_lib.lib().drm_unet_workspace_bytes(self._h, n, h, w))
        return cache[key]

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def _run(self, x, cond, t_emb, timesteps, rows=None):
        x = _lib.require_gpu_tensor(x, "x")
        dev = x.device
        n = x.shape[0] if rows is None else rows.shape[0]
        cx, hh, ww = x.shape[1], x.shape[2], x.shape[3]
        cc = 0
        if cond is not None:
            cond = _lib.require_gpu_tensor(cond, "cond")
            cc = cond.shape[1]
            if cond.shape[0] != x.shape[0] or cond.shape[2:] != x.shape[2:]:
                raise RuntimeError("x / cond shape mismatch")
        if cx + cc != self.in_channels:
            raise RuntimeError(f"expected {self.in_channels} input channels, got {cx}+{cc}")
        tf = None
        ti = None
        if timesteps is not None:
            if timesteps.dtype == torch.int64:
                ti = _lib.require_gpu_tensor(timesteps, "timesteps", torch.int64)
            else:
                tf = _lib.require_gpu_tensor(timesteps.float(), "timesteps")
        if t_emb is not None:
            t_emb = _lib.require_gpu_tensor(t_emb, "t_emb")
            if tuple(t_emb.shape) != (n, self.model_channels):
                raise RuntimeError(f"t_emb must be [{n}, {self.model_channels}]")
        if rows is not None:
            rows = _lib.require_gpu_tensor(rows, "rows", torch.int32)
        if self._kind == 0:
            out = torch.empty((n, self.out_channels, hh, ww), dtype=torch.float32, device=dev)
        else:
            out = torch.empty((n, self.out_channels), dtype=torch.float32, device=dev)
        if n == 0:  # an empty batch is an empty result, as in the reference (every row of a DRMNet batch may have converged)
            return out
        self.sync_weights()
        L = _lib.lib()
        ws = self._ws.get(self.workspace_bytes(n, hh, ww), dev)
        with torch.cuda.device(dev):
            _lib.check(
                L.drm_unet_forward(self._h, x.data_ptr(), cx, _lib.ptr(cond), cc, _lib.ptr(rows), _lib.ptr(t_emb), _lib.ptr(ti), _lib.ptr(tf),
                                   out.data_ptr(), n, hh, ww, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
            )
        return out


class UNetModel(_HipUNetBase):
    """``UNetModel(image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, ...)``
    -- reference openaimodel.py:452-478 (same parameter names and defaults)."""

    _kind = 0

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=-1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False,
                 use_spatial_transformer=False, transformer_depth=1, context_dim=None, n_embed=None, legacy=True,
                 use_positional_embedded_attention=False):
        super().__init__()
        if num_heads == -1:
            assert num_head_channels != -1, "Either num_heads or num_head_channels has to be set"
        _reject_unsupported("UNetModel", dropout=dropout, conv_resample=conv_resample, dims=dims, num_classes=num_classes, use_fp16=use_fp16,
                            num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
                            use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown,
                            use_new_attention_order=use_new_attention_order, use_spatial_transformer=use_spatial_transformer,
                            context_dim=context_dim, n_embed=n_embed, use_positional_embedded_attention=use_positional_embedded_attention)
        self.image_size = image_size
        self.num_classes = None
        self._setup(in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, channel_mult)

    def forward(self, x, timesteps=None, context=None, y=None, t_emb=None, **kwargs):
        """openaimodel.py:731-768. ``x`` is the already-concatenated [N, in_channels, H, W] tensor."""
        assert y is None, "must specify y if and only if the model is class-conditional"
        if (timesteps is None) == (t_emb is None):
            raise ValueError("timesteps and t_emb cannot be specified at the same time")
        if context is not None:
            raise NotImplementedError("cross-attention context (use_spatial_transformer) is not supported")
        return self._run(x, None, t_emb, timesteps)

    def forward_parts(self, x, cond, timesteps=None, t_emb=None, rows=None):
        """Same as forward(cat([x, cond], 1), ...) without materialising the concat; ``rows`` gathers samples."""
        if (timesteps is None) == (t_emb is None):
            raise ValueError("timesteps and t_emb cannot be specified at the same time")
        return self._run(x, cond, t_emb, timesteps, rows)


class EncoderUNetModel(_HipUNetBase):
    """Reference openaimodel.py:777-802 (same parameter names and defaults)."""

    _kind = 1

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, use_checkpoint=False, use_fp16=False, num_heads=1, num_head_channels=-1,
                 num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False, pool="adaptive",
                 use_positional_embedded_attention=False, *args, **kwargs):
        super().__init__()
        _reject_unsupported("encoder", dropout=dropout, conv_resample=conv_resample, dims=dims, use_fp16=use_fp16, num_heads=num_heads,
                            num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample, use_scale_shift_norm=use_scale_shift_norm,
                            resblock_updown=resblock_updown, use_new_attention_order=use_new_attention_order, pool=pool,
                            use_positional_embedded_attention=use_positional_embedded_attention)
        self.image_size = image_size
        self.pool = pool
        self._setup(in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, channel_mult)

    def forward(self, x, timesteps):
        """openaimodel.py:969-991 -> [N, out_channels]."""
        return self._run(x, None, None, timesteps)

    def forward_parts(self, x, cond, timesteps, rows=None):
        return self._run(x, cond, None, timesteps, rows)

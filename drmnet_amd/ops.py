"""Primitive ops of the HIP library on reference-layout tensors (NCHW activations, PyTorch-layout weights).

Per-module drop-ins for the reference's L1/L2 pieces (GroupNorm32+SiLU+conv_nd chains, ResBlock,
AttentionBlock, linear/SiLU embeddings, timestep_embedding).  GPU only.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib


def set_precision(precision: str) -> None:
    """Arithmetic of the drm_op_* entry points: "fp32" (default), "f16x3" (split fp16, fp32-accurate), "f16mx" (f16x3 with the res blocks'
    3x3 convs on fp16 hi*hi + a block-scaled fp8 MFMA for the cross terms, ~7e-6 per block), "f16" or "bf16" (reduced precision)."""
    modes = {"fp32": 0, "f16x3": 1, "f16": 2, "f16mx": 3, "bf16": 4}
    if precision not in modes:
        raise ValueError(f"precision must be one of {list(modes)}")
    _lib.check(_lib.lib().drm_set_op_precision(modes[precision]))


def set_graph_replay(on: bool) -> None:
    """DDIM / DDPM chains replay one captured hipGraph of a step (default off); see include/drmnet_hip.h."""
    _lib.check(_lib.lib().drm_set_graph_replay(int(bool(on))))


def set_upconv_split(mode: int) -> None:
    """in_layers conv over cat(nearest_x2(x0), x1) as a 4-tap conv on the stored x0 + a 3x3 conv on x1: 0 = never, 1 = by the measured per-level
    rule (default), 2 = wherever the form applies; see include/drmnet_hip.h.  For tests and A/B measurements."""
    _lib.check(_lib.lib().drm_set_upconv_split(int(mode)))


# parity of the output row (column) -> window position dy (dx) -> the 3x3 taps ky (kx) that land on that stored pixel of a nearest-x2 input
UPCONV_TAP_GROUPS = {0: {0: (0,), 1: (1, 2)}, 1: {0: (0, 1), 1: (2,)}}


def fold_upconv_weight(w: torch.Tensor, c0: int):
    """What csrc/conv_split.hip fold_upconv_weight_kernel computes, in torch (any device): w [Cout, C0 + C1, 3, 3] ->
    (wa [4 * Cout, C0, 2, 2], parity-major p = 2a + b, tap sums in fp64 rounded once; wb [Cout, C1, 3, 3]).  Output pixel (2i + a, 2j + b) of
    conv3x3(nearest_x2(x)) is sum wa[p][dy, dx] * x[i + a - 1 + dy, j + b - 1 + dx] with zero padding outside the stored map."""
    cout = w.shape[0]
    w0 = w[:, :c0].double()
    wa = torch.zeros((4, cout, c0, 2, 2), dtype=torch.float64, device=w.device)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    for ky in UPCONV_TAP_GROUPS[a][dy]:
                        for kx in UPCONV_TAP_GROUPS[b][dx]:
                            wa[2 * a + b, :, :, dy, dx] += w0[:, :, ky, kx]
    return wa.reshape(4 * cout, c0, 2, 2).to(w.dtype), w[:, c0:].contiguous()


def graph_launches() -> int:
    return int(_lib.lib().drm_graph_launches())


def _dev(t: torch.Tensor):
    return torch.cuda.device(t.device)


@torch.no_grad()
def linear(x, weight, bias=None, silu_in=False, silu_out=False):
    """act_out(F.linear(act_in(x), weight, bias)) -- openaimodel.py:218-224,521-526; models/drmnet.py:38-45."""
    x = _lib.require_gpu_tensor(x, "x")
    weight = _lib.require_gpu_tensor(weight, "weight")
    bias = None if bias is None else _lib.require_gpu_tensor(bias, "bias")
    n, i = x.shape
    o = weight.shape[0]
    out = torch.empty((n, o), dtype=torch.float32, device=x.device)
    with _dev(x):
        _lib.check(_lib.lib().drm_linear_forward(x.data_ptr(), weight.data_ptr(), _lib.ptr(bias), out.data_ptr(), n, i, o, int(silu_in), int(silu_out), _lib.stream_ptr(x.device)))
    return out


@torch.no_grad()
def timestep_embedding(timesteps, dim):
    """ldm/modules/diffusionmodules/util.py:151-171."""
    t = _lib.require_gpu_tensor(timesteps.long(), "timesteps", torch.int64)
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    with _dev(t):
        _lib.check(_lib.lib().drm_timestep_embedding(t.data_ptr(), out.data_ptr(), t.shape[0], dim, _lib.stream_ptr(t.device)))
    return out


@torch.no_grad()
def norm_act_conv(x, weight, bias=None, gamma=None, beta=None, silu=False, emb=None, residual=None):
    """[GroupNorm32 -> [SiLU] ->] conv2d(k in {1,3}, pad k//2) [+ emb[:, :, None, None]] [+ residual]."""
    x = _lib.require_gpu_tensor(x, "x")
    weight = _lib.require_gpu_tensor(weight, "weight")
    n, cin, h, w = x.shape
    cout, k = weight.shape[0], weight.shape[-1]
    ts = [None if t is None else _lib.require_gpu_tensor(t, "arg") for t in (bias, gamma, beta, emb, residual)]
    bias, gamma, beta, emb, residual = ts
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    with _dev(x):
        _lib.check(_lib.lib().drm_op_norm_act_conv(x.data_ptr(), _lib.ptr(gamma), _lib.ptr(beta), int(silu), weight.data_ptr(), _lib.ptr(bias), k,
                                                    _lib.ptr(emb), _lib.ptr(residual), out.data_ptr(), n, cin, cout, h, w, _lib.stream_ptr(x.device)))
    return out


@torch.no_grad()
def resblock(params: Sequence[torch.Tensor], x0, emb, x1=None, up0=False):
    """ResBlock._forward (openaimodel.py:255-275) on cat([up(x0), x1], 1); params in state_dict order."""
    x0 = _lib.require_gpu_tensor(x0, "x0")
    emb = _lib.require_gpu_tensor(emb, "emb")
    params = [_lib.require_gpu_tensor(p, "param") for p in params]
    n, c0 = x0.shape[0], x0.shape[1]
    h, w = x0.shape[2] * (2 if up0 else 1), x0.shape[3] * (2 if up0 else 1)
    c1 = 0
    if x1 is not None:
        x1 = _lib.require_gpu_tensor(x1, "x1")
        c1 = x1.shape[1]
    cout = params[2].shape[0]
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x0.device)
    arr = _lib.ptr_array(params)
    with _dev(x0):
        _lib.check(_lib.lib().drm_op_resblock(x0.data_ptr(), c0, int(up0), _lib.ptr(x1), c1, emb.data_ptr(), emb.shape[1], arr, len(params),
                                               out.data_ptr(), n, cout, h, w, _lib.stream_ptr(x0.device)))
    return out


@torch.no_grad()
def attention_block(params: Sequence[torch.Tensor], x):
    """AttentionBlock._forward (openaimodel.py:325-333); params = norm.w, norm.b, qkv.w, qkv.b, proj_out.w, proj_out.b."""
    x = _lib.require_gpu_tensor(x, "x")
    params = [_lib.require_gpu_tensor(p, "param") for p in params]
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    arr = _lib.ptr_array(params)
    with _dev(x):
        _lib.check(_lib.lib().drm_op_attention_block(x.data_ptr(), arr, out.data_ptr(), n, c, h, w, _lib.stream_ptr(x.device)))
    return out


@torch.no_grad()
def stem_conv(x, cond, weight, bias=None, rows=None, want_stats=False):
    """input_blocks.0.0 on the stem kernel of its own (csrc/stemhead.hip; drm_op_stem_conv): conv3x3(cat([x, cond], 1)[rows]) with x [B, Cx, H, W],
    cond [B, Cc, H, W] or None, weight [128, Cx + Cc, 3, 3], rows int32 [N] or None -> out [N, 128, H, W]; with ``want_stats`` also the fused
    GroupNorm table [N, 128, 2] fp64 = (sum, sum of squares) of each output channel.  ops.set_precision("fp32") runs the exact fp32 form, every
    other mode the fp16 hi / lo split."""
    x = _lib.require_gpu_tensor(x, "x")
    weight = _lib.require_gpu_tensor(weight, "weight")
    cond = None if cond is None else _lib.require_gpu_tensor(cond, "cond")
    bias = None if bias is None else _lib.require_gpu_tensor(bias, "bias")
    if x.ndim != 4 or weight.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise RuntimeError(f"stem_conv expects x [B, Cx, H, W] and weight [Cout, Cin, 3, 3], got {tuple(x.shape)} and {tuple(weight.shape)}")
    b, cx, h, w = x.shape
    cc = 0 if cond is None else cond.shape[1]
    if cond is not None and (cond.ndim != 4 or cond.shape[0] != b or tuple(cond.shape[2:]) != (h, w)):
        raise RuntimeError(f"cond must be [B={b}, Cc, {h}, {w}], got {tuple(cond.shape)}")
    cout = weight.shape[0]
    if weight.shape[1] != cx + cc:
        raise RuntimeError(f"weight must have Cx + Cc = {cx + cc} input channels, got {weight.shape[1]}")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise RuntimeError(f"bias must be [{cout}], got {tuple(bias.shape)}")
    n = b
    if rows is not None:
        rows = _lib.require_gpu_tensor(rows.to(torch.int32), "rows", torch.int32)
        n = rows.numel()
        if rows.ndim != 1 or n < 1 or int(rows.min()) < 0 or int(rows.max()) >= b:
            raise RuntimeError(f"rows must be a non-empty int32 vector of indices into the {b} rows of x")
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    stat = torch.empty((n, cout, 2), dtype=torch.float64, device=x.device) if want_stats else None
    with _dev(x):
        _lib.check(_lib.lib().drm_op_stem_conv(x.data_ptr(), cx, _lib.ptr(cond), cc, _lib.ptr(rows), weight.data_ptr(), _lib.ptr(bias), out.data_ptr(),
                                                _lib.ptr(stat), n, cout, h, w, _lib.stream_ptr(x.device)))
    return (out, stat) if want_stats else out


@torch.no_grad()
def avgpool2(x, want_stats=False):
    """Downsample without conv = AvgPool2d(2, 2) (openaimodel.py:154-160; csrc/misc.hip avgpool2_kernel, drm_op_avgpool2): x [N, C, H, W] ->
    out [N, C, H/2, W/2]; with ``want_stats`` also the fused GroupNorm table [N, C, 2] fp64 = (sum, sum of squares) of each output channel."""
    x = _lib.require_gpu_tensor(x, "x")
    if x.ndim != 4:
        raise RuntimeError(f"avgpool2 expects x [N, C, H, W], got {tuple(x.shape)}")
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    stat = torch.empty((n, c, 2), dtype=torch.float64, device=x.device) if want_stats else None
    with _dev(x):
        _lib.check(_lib.lib().drm_op_avgpool2(x.data_ptr(), out.data_ptr(), _lib.ptr(stat), n, c, h, w, _lib.stream_ptr(x.device)))
    return (out, stat) if want_stats else out


@torch.no_grad()
def encoder_head(x, scale, shift, weight, bias):
    """The tail of EncoderUNetModel's head, pool="adaptive" (openaimodel.py:922-929; csrc/misc.hip encoder_head_kernel, drm_op_encoder_head):
    mean_hw(silu(x * scale + shift)) @ weight.T + bias with x [N, C, H, W], scale, shift [N, C] (the GroupNorm tables), weight [O, C], bias [O]
    -> [N, O]."""
    x = _lib.require_gpu_tensor(x, "x")
    if x.ndim != 4:
        raise RuntimeError(f"encoder_head expects x [N, C, H, W], got {tuple(x.shape)}")
    n, c, h, w = x.shape
    scale, shift = _lib.require_gpu_tensor(scale, "scale"), _lib.require_gpu_tensor(shift, "shift")
    weight, bias = _lib.require_gpu_tensor(weight.reshape(weight.shape[0], -1), "weight"), _lib.require_gpu_tensor(bias, "bias")
    o = weight.shape[0]
    if tuple(scale.shape) != (n, c) or tuple(shift.shape) != (n, c):
        raise RuntimeError(f"scale and shift must be [N={n}, C={c}], got {tuple(scale.shape)} and {tuple(shift.shape)}")
    if tuple(weight.shape) != (o, c) or tuple(bias.shape) != (o,):
        raise RuntimeError(f"weight must be [O, C={c}] and bias [O], got {tuple(weight.shape)} and {tuple(bias.shape)}")
    out = torch.empty((n, o), dtype=torch.float32, device=x.device)
    with _dev(x):
        _lib.check(_lib.lib().drm_op_encoder_head(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                   n, c, h, w, o, _lib.stream_ptr(x.device)))
    return out


@torch.no_grad()
def randn(shape, seed: int, offset: int = 0, device="cuda"):
    """Standard normal from the library's Philox4x32-10 stream."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().drm_randn(out.data_ptr(), out.numel(), seed, offset, _lib.stream_ptr(out.device)))
    return out


# ------------------------------------------------------------------------------------------------ validation losses (csrc/losses.hip)

LOSS_TYPES = {"l1": 0, "l2": 1}


@torch.no_grad()
def validation_losses(model_out, Lr_k, Lr_km1, K, z_out, z_k, z_K, reversed_k, z0, gamma: float, loss_type: str = "l2", l_refmap_weight: float = 1.0,
                      l_refcode_weight: float = 1.0) -> torch.Tensor:
    """models/drmnet.py:432-450 in eval mode (drm_validation_losses): model_out, Lr_k (as the networks saw it), Lr_km1 [B, 3, H, W]; K,
    reversed_k [B] int32; z_out, z_k, z_K [B, P]; z0 [P] -> fp32 [3] on the device = (loss_refmap, loss_refcode, loss).  Rows with K == 0 are
    selected out of loss_refmap.  Two launches, no host synchronisation; fp64 sums in a fixed order."""
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError(f"unknown loss type '{loss_type}'")
    model_out = _lib.require_gpu_tensor(model_out, "model_out")
    dev = model_out.device
    B = model_out.shape[0]
    maps = [model_out] + [_lib.require_gpu_tensor(t, n) for t, n in ((Lr_k, "Lr_k"), (Lr_km1, "Lr_km1"))]
    if any(t.shape != model_out.shape for t in maps):
        raise RuntimeError(f"model_out, Lr_k and Lr_km1 must share one shape, got {[tuple(t.shape) for t in maps]}")
    codes = [_lib.require_gpu_tensor(t, n) for t, n in ((z_out, "z_out"), (z_k, "z_k"), (z_K, "z_K"))]
    P = codes[0].shape[-1]
    if any(tuple(t.shape) != (B, P) for t in codes):
        raise RuntimeError(f"z_out, z_k and z_K must be [B={B}, P], got {[tuple(t.shape) for t in codes]}")
    ints = [_lib.require_gpu_tensor(t.to(torch.int32), n, torch.int32) for t, n in ((K, "K"), (reversed_k, "reversed_k"))]
    if any(tuple(t.shape) != (B,) for t in ints):
        raise RuntimeError(f"K and reversed_k must be [B={B}]")
    z0 = _lib.require_gpu_tensor(z0.to(dev, torch.float32), "z0")
    if z0.numel() != P:
        raise RuntimeError(f"z0 must have {P} entries")
    ws = torch.empty(_lib.LOSS_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_validation_losses(maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), ints[0].data_ptr(), codes[0].data_ptr(),
                                                    codes[1].data_ptr(), codes[2].data_ptr(), ints[1].data_ptr(), z0.data_ptr(), float(gamma),
                                                    LOSS_TYPES[loss_type], float(l_refmap_weight), float(l_refcode_weight), B,
                                                    model_out.numel() // B, P, ws.data_ptr(), ws.numel() * 8, out.data_ptr(), _lib.stream_ptr(dev)))
    return out


# ------------------------------------------------------------------------------------------------ ObsNet's forward process and losses (csrc/obs_forward.hip)

PADDING_MODES = {"zeros": 0, "noise": 1}


@torch.no_grad()
def obs_forward_process(x, mask, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, noisy_observe: float = 0.0, padding_mode: str = "noise", *,
                        e_observe=None, e_padding=None, e_q=None, seed: int = 0, want_cond: bool = True, want_q: bool = True):
    """models/obsnet.py:375-398 and ddpm.py:288-294 in one launch (drm_obs_forward_process): x [B, C, H, W] (the transformed LrK), mask
    [B, 1, H, W], t [B] -> (cond, x_noisy, noise) with cond = mask x + noisy_observe e1 + (1 - mask) e2 (the e1 term only when noisy_observe > 0,
    the e2 term only for padding_mode "noise"), x_noisy = a[t] x + s[t] e3 and noise = e3.  e_observe / e_padding / e_q inject e1 / e2 / e3; a draw
    that is not injected comes from the Philox stream of ``seed`` at offsets 0, n and 2 n (n = x.numel()).  ``want_cond=False`` leaves the
    conditioning out (cond is None; mask may be None), ``want_q=False`` the q_sample (x_noisy and noise are None; t and the tables may be None):
    the two halves of one seed, run in two calls, are what one call returns."""
    if padding_mode not in PADDING_MODES:
        raise NotImplementedError(f"padding_mode {padding_mode!r}")
    if not (want_cond or want_q):
        raise ValueError("obs_forward_process: nothing asked for")
    x = _lib.require_gpu_tensor(x, "x")
    if x.ndim != 4:
        raise RuntimeError("obs_forward_process expects x [B, C, H, W]")
    dev = x.device
    B, C, H, W = x.shape
    mh = mw = 0
    if want_cond:
        mask = _lib.require_gpu_tensor(mask, "mask")
        if mask.ndim != 4 or mask.shape[0] != B or mask.shape[1] != 1:
            raise RuntimeError(f"mask must be [B={B}, 1, H, W], got {tuple(mask.shape)}")
        mh, mw = int(mask.shape[2]), int(mask.shape[3])
    else:
        mask = None
    sa = s1 = None
    if want_q:
        t = _lib.require_gpu_tensor(t.to(torch.int32), "t", torch.int32)
        if tuple(t.shape) != (B,):
            raise RuntimeError(f"t must be [B={B}]")
        sa = _lib.require_gpu_tensor(sqrt_alphas_cumprod, "sqrt_alphas_cumprod")
        s1 = _lib.require_gpu_tensor(sqrt_one_minus_alphas_cumprod, "sqrt_one_minus_alphas_cumprod")
        if sa.ndim != 1 or sa.shape != s1.shape:
            raise RuntimeError("the two schedule tables must be [T]")
    else:
        t = None
    draws = [None if e is None else _lib.require_gpu_tensor(e, n) for e, n in ((e_observe, "e_observe"), (e_padding, "e_padding"), (e_q, "e_q"))]
    if any(e is not None and e.shape != x.shape for e in draws):
        raise RuntimeError(f"injected draws must have the shape of x {tuple(x.shape)}")
    cond = torch.empty_like(x) if want_cond else None
    x_noisy, noise = (torch.empty_like(x), torch.empty_like(x)) if want_q else (None, None)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_obs_forward_process(x.data_ptr(), _lib.ptr(mask), _lib.ptr(t), _lib.ptr(sa), _lib.ptr(s1), 0 if sa is None else sa.numel(),
                                                      float(noisy_observe), PADDING_MODES[padding_mode], _lib.ptr(draws[0]), _lib.ptr(draws[1]),
                                                      _lib.ptr(draws[2]), int(seed), _lib.ptr(cond), _lib.ptr(x_noisy), _lib.ptr(noise), B, C, H, W,
                                                      mh, mw, _lib.stream_ptr(dev)))
    return cond, x_noisy, noise


@torch.no_grad()
def diffusion_losses(model_out, target, t, logvar, lvlb_weights, loss_type: str = "l2", l_simple_weight: float = 1.0, original_elbo_weight: float = 0.0,
                     invmask=None, return_rows: bool = False):
    """models/obsnet.py:469-498 in eval mode (drm_diffusion_losses): model_out, target [B, C, H, W]; t [B]; logvar, lvlb_weights [T];
    invmask [B, 1, H, W] (1 - mask) for masked_loss or None -> fp32 [3] on the device = (loss_simple, loss_vlb, loss), with ``return_rows`` also
    the per-row loss_simple [B].  Two launches, no host synchronisation; fp64 sums in a fixed order."""
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError(f"unknown loss type '{loss_type}'")
    model_out = _lib.require_gpu_tensor(model_out, "model_out")
    dev = model_out.device
    target = _lib.require_gpu_tensor(target, "target")
    if target.shape != model_out.shape or model_out.ndim < 2:
        raise RuntimeError(f"model_out and target must share one [B, C, ...] shape, got {tuple(model_out.shape)} and {tuple(target.shape)}")
    B, C = model_out.shape[0], model_out.shape[1]
    per_row = model_out.numel() // B
    if invmask is not None:
        invmask = _lib.require_gpu_tensor(invmask, "invmask")
        if invmask.numel() != B * (per_row // C) or invmask.shape[0] != B:
            raise RuntimeError(f"invmask must be [B={B}, 1, ...] with one plane per row, got {tuple(invmask.shape)}")
    t = _lib.require_gpu_tensor(t.to(torch.int32), "t", torch.int32)
    if tuple(t.shape) != (B,):
        raise RuntimeError(f"t must be [B={B}]")
    logvar = _lib.require_gpu_tensor(logvar, "logvar")
    lvlb_weights = _lib.require_gpu_tensor(lvlb_weights, "lvlb_weights")
    if logvar.ndim != 1 or logvar.shape != lvlb_weights.shape:
        raise RuntimeError("logvar and lvlb_weights must be [T]")
    ws = torch.empty(_lib.diffusion_loss_workspace_bytes(B) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev) if return_rows else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_diffusion_losses(model_out.data_ptr(), target.data_ptr(), _lib.ptr(invmask), t.data_ptr(), logvar.data_ptr(),
                                                   lvlb_weights.data_ptr(), logvar.numel(), LOSS_TYPES[loss_type], float(l_simple_weight),
                                                   float(original_elbo_weight), B, per_row, C, ws.data_ptr(), ws.numel() * 8, out.data_ptr(),
                                                   _lib.ptr(rows), _lib.stream_ptr(dev)))
    return (out, rows) if return_rows else out


# ------------------------------------------------------------------------------------------------ boundary maps (csrc/transform.hip)

MAP_CODES = {"log_p1": 0, "log10": 1, "lowerbound": 2, "unit_to_signed": 3, "norm_log": 4, "exp_m1": 5, "exp10": 6, "signed_to_unit": 7,
             "denorm_log": 8, "img_mul": 9, "img_div": 10, "clip0": 11}
MAX_CHAIN = 8


def _per_image(x: torch.Tensor):
    """[B, C, H, W] -> (B, C*H*W); a 3-D [C, H, W] tensor is one image (the reference reduces over the last three dims)."""
    if x.ndim < 3:
        raise RuntimeError("expected a [(B,) C, H, W] tensor")
    b = 1
    for d in x.shape[:-3]:
        b *= int(d)
    return b, x.numel() // max(b, 1)


@torch.no_grad()
def map_chain(x, steps, lo=None, hi=None, scale=None, out=None):
    """Applies ``steps`` = [(map name, scalar argument), ...] to every element in ONE pass (drm_map_chain).
    lo / hi / scale: per-image fp32 vectors for the maps that need them.  Longer chains are cut into passes of 8."""
    import ctypes as C

    x = _lib.require_gpu_tensor(x, "x")
    b, per = _per_image(x)
    vec = lambda t, n: None if t is None else _lib.require_gpu_tensor(t.reshape(-1), n)
    lo, hi, scale = vec(lo, "lo"), vec(hi, "hi"), vec(scale, "scale")
    for n, t in (("lo", lo), ("hi", hi), ("scale", scale)):
        if t is not None and t.numel() != b:
            raise RuntimeError(f"{n} must have one entry per image ({b}), got {t.numel()}")
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()):
        raise RuntimeError(f"out must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on {x.device}; got {out.dtype} "
                           f"{tuple(out.shape)} on {out.device}, contiguous: {out.is_contiguous()}")
    res = torch.empty_like(x) if out is None else out
    src = x
    steps = list(steps)
    if not steps:
        res.copy_(x)
        return res
    with _dev(x):
        for k in range(0, len(steps), MAX_CHAIN):
            part = steps[k:k + MAX_CHAIN]
            ops_arr = (C.c_int32 * len(part))(*[MAP_CODES[n] for n, _ in part])
            arg_arr = (C.c_float * len(part))(*[float(a) for _, a in part])
            _lib.check(_lib.lib().drm_map_chain(src.data_ptr(), res.data_ptr(), per, b, ops_arr, arg_arr, len(part), _lib.ptr(lo), _lib.ptr(hi),
                                                _lib.ptr(scale), _lib.stream_ptr(x.device)))
            src = res
    return res


@torch.no_grad()
def masked_log_range(x, mask):
    """(log10 min, log10 max) per image of x under mask, the dynamic_normalize statistics of basedataset.py:63-69 -> two [B] tensors."""
    x = _lib.require_gpu_tensor(x, "x")
    b, per = _per_image(x)
    hw = x.shape[-1] * x.shape[-2]
    mask = _lib.require_gpu_tensor(mask.to(torch.float32), "mask")
    if mask.numel() != b * hw:
        raise NotImplementedError("mask must be [B, 1, H, W] (one plane per image, broadcast over channels)")
    lo = torch.empty((b,), dtype=torch.float32, device=x.device)
    hi = torch.empty_like(lo)
    with _dev(x):
        _lib.check(_lib.lib().drm_masked_log_range(x.data_ptr(), mask.data_ptr(), b, per // hw, hw, lo.data_ptr(), hi.data_ptr(), _lib.stream_ptr(x.device)))
    return lo, hi


@torch.no_grad()
def luminance_scale(x, scaler: float):
    """models/drmnet.py:1020-1026: scaler / geometric-mean luminance over the lit pixels, per image of x [B, 3, H, W] -> [B]."""
    x = _lib.require_gpu_tensor(x, "x")
    if x.ndim != 4 or x.shape[1] != 3:
        raise RuntimeError("luminance_scale expects [B, 3, H, W]")
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    with _dev(x):
        _lib.check(_lib.lib().drm_luminance_scale(x.data_ptr(), x.shape[0], x.shape[2] * x.shape[3], float(scaler), out.data_ptr(), _lib.stream_ptr(x.device)))
    return out


@torch.no_grad()
def mirmap2envmap(mirmap, output_shape, basis=None, log_scale_interpolation=False, channels_last=False):
    """utils/transform.py:106-144 (+ the basis_r0 division of DRMNet.r0toenvmap when ``basis`` [C, H, W] is given)."""
    mirmap = _lib.require_gpu_tensor(mirmap, "mirmap")
    b, c, h, w = mirmap.shape
    oh, ow = int(output_shape[0]), int(output_shape[1])
    if basis is not None:
        basis = _lib.require_gpu_tensor(basis.expand(c, h, w), "basis_r0")
    out = torch.empty((b, oh, ow, c) if channels_last else (b, c, oh, ow), dtype=torch.float32, device=mirmap.device)
    with _dev(mirmap):
        _lib.check(_lib.lib().drm_mirmap2envmap(mirmap.data_ptr(), _lib.ptr(basis), out.data_ptr(), b, c, h, w, oh, ow, int(bool(log_scale_interpolation)),
                                                int(bool(channels_last)), _lib.stream_ptr(mirmap.device)))
    return out


@torch.no_grad()
def hdr2ldr(x, mask=None, alpha: float = 0.18, gamma: float = 2.2):
    """utils/tonemap.py:4-9 on a [H, W, 3] device tensor (mask: optional [H, W] bool / uint8)."""
    x = _lib.require_gpu_tensor(x, "x")
    if x.ndim != 3 or x.shape[2] != 3:
        raise RuntimeError("hdr2ldr expects [H, W, 3]")
    m = None if mask is None else _lib.require_gpu_tensor(mask.to(torch.uint8), "mask", torch.uint8)
    out = torch.empty_like(x)
    with _dev(x):
        _lib.check(_lib.lib().drm_hdr2ldr(x.data_ptr(), _lib.ptr(m), x.shape[0] * x.shape[1], float(alpha), float(gamma), out.data_ptr(), _lib.stream_ptr(x.device)))
    return out


RESIZE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}


@torch.no_grad()
def resize(x, size, mode: str = "bilinear"):
    """dataset/basedataset.py:44-50 (anti-aliased bilinear / bicubic, align_corners=False) and models/obsnet.py:691 (nearest) on the last
    two dimensions of a device tensor; every leading dimension is a plane."""
    x = _lib.require_gpu_tensor(x, "x")
    if mode not in RESIZE_MODES:
        raise NotImplementedError(f"resize mode {mode!r} (drm_resize implements {sorted(RESIZE_MODES)})")
    oh, ow = int(size[0]), int(size[1])
    ih, iw = int(x.shape[-2]), int(x.shape[-1])
    planes = x.numel() // (ih * iw)
    out = torch.empty(tuple(x.shape[:-2]) + (oh, ow), dtype=torch.float32, device=x.device)
    with _dev(x):
        _lib.check(_lib.lib().drm_resize(x.data_ptr(), out.data_ptr(), planes, ih, iw, oh, ow, RESIZE_MODES[mode], _lib.stream_ptr(x.device)))
    return out


def _warp_input(x, name: str, channels_last: bool):
    """x [B, C, H, W] (or [B, H, W, C] with channels_last) on the GPU -> (x, B, C, H, W)"""
    x = _lib.require_gpu_tensor(x, name)
    if x.ndim != 4:
        raise RuntimeError(f"{name} must be [B, C, H, W]" + (" ([B, H, W, C] with channels_last)" if channels_last else "") + f", got {tuple(x.shape)}")
    b, c, h, w = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if channels_last else x.shape
    return x, int(b), int(c), int(h), int(w)


def _warp_frames(frames, b: int, k: int, dev):
    f = torch.as_tensor(frames, dtype=torch.float32)
    if tuple(f.shape) != (b, k, 3):
        raise RuntimeError(f"frames must be [B={b}, {k}, 3], got {tuple(f.shape)}")
    return f.to(dev).contiguous()


@torch.no_grad()
def envmap2mirmap(envmap, output_shape, frames, mitigate_aliasing=True, log_scale_interpolation=False, channels_last=False):
    """drm_envmap2mirmap (utils/transform.py:201-242) on frames [B, 6, 3] (include/drmnet_hip.h names the rows) -> [B, C, OH, OW]"""
    envmap, b, c, h, w = _warp_input(envmap, "envmap", channels_last)
    oh, ow = int(output_shape[0]), int(output_shape[1])
    frames = _warp_frames(frames, b, 6, envmap.device)
    out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=envmap.device)
    with _dev(envmap):
        _lib.check(_lib.lib().drm_envmap2mirmap(envmap.data_ptr(), frames.data_ptr(), out.data_ptr(), b, c, h, w, oh, ow, int(bool(mitigate_aliasing)),
                                                int(bool(log_scale_interpolation)), int(bool(channels_last)), _lib.stream_ptr(envmap.device)))
    return out


@torch.no_grad()
def rotate_envmap(envmap, output_shape, frames, channels_last=False):
    """drm_rotate_envmap (utils/transform.py:317-363) on frames [B, 6, 3] -> [B, C, OH, OW]"""
    envmap, b, c, h, w = _warp_input(envmap, "envmap", channels_last)
    oh, ow = int(output_shape[0]), int(output_shape[1])
    frames = _warp_frames(frames, b, 6, envmap.device)
    out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=envmap.device)
    with _dev(envmap):
        _lib.check(_lib.lib().drm_rotate_envmap(envmap.data_ptr(), frames.data_ptr(), out.data_ptr(), b, c, h, w, oh, ow, int(bool(channels_last)),
                                                _lib.stream_ptr(envmap.device)))
    return out


@torch.no_grad()
def mirimg2envmap(refimg, output_shape, frames, log_scale_interpolation=False, channels_last=False):
    """drm_mirimg2envmap (utils/transform.py:245-284) on frames [B, 7, 3] -> [B, C, OH, OW]"""
    refimg, b, c, h, w = _warp_input(refimg, "refimg", channels_last)
    oh, ow = int(output_shape[0]), int(output_shape[1])
    frames = _warp_frames(frames, b, 7, refimg.device)
    out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=refimg.device)
    with _dev(refimg):
        _lib.check(_lib.lib().drm_mirimg2envmap(refimg.data_ptr(), frames.data_ptr(), out.data_ptr(), b, c, h, w, oh, ow, int(bool(log_scale_interpolation)),
                                                int(bool(channels_last)), _lib.stream_ptr(refimg.device)))
    return out


@torch.no_grad()
def refmap2refimg(refmap, radius: int, channels_last=False):
    """drm_refmap2refimg (utils/transform.py:170-198) -> (image [B, C, 2 radius, 2 radius], zero outside the disc; mask [2 radius, 2 radius] bool)"""
    refmap, b, c, h, w = _warp_input(refmap, "refmap", channels_last)
    res = 2 * int(radius)
    out = torch.empty((b, c, res, res), dtype=torch.float32, device=refmap.device)
    mask = torch.empty((res, res), dtype=torch.uint8, device=refmap.device)
    with _dev(refmap):
        _lib.check(_lib.lib().drm_refmap2refimg(refmap.data_ptr(), out.data_ptr(), mask.data_ptr(), b, c, h, w, int(radius), int(bool(channels_last)),
                                                _lib.stream_ptr(refmap.device)))
    return out, mask.bool()

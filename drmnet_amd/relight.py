"""Object images from a normal map -- the forward model pointed at ``estimate``'s own inputs -- on normals_pixel_kernel (csrc/render_shared.h)
and image_from_refmap_kernel (csrc/refmap.hip).

    python -m drmnet_amd.relight --input_normal N.npy [--input_mask M.png] [--envmap E.exr] (--z m R G B r s | --merl material.binary)
        [--view_from x y z] [--quad Q] [--light_samples M] [--input_img I.exr] --output_dir D

``estimate`` turns an object image, its normal map and a mask into an illumination map and a BRDF; nothing in the reference turns those
back into an image of the same object without its mesh (MitsubaOrthoRenderer, utils/mitsuba3_utils.py:433-564, needs the mesh;
DRMNet.reconstruct, models/drmnet.py:943-953, renders the estimate onto the sphere).  ``render_normals`` shades every pixel's normal
exactly as ``render.render`` shades the sphere point and ``mesh.render_mesh`` the mesh hit with that normal: direct light from the
environment map, no shadows, no interreflection.  That re-renders an estimate on the object it came from (``rerender``: the only check
there is on a photograph, which has no ground-truth reflectance map), relights the object under another map, or edits its material.
``image_from_refmap`` reads a reflectance map at every pixel's normal instead: the image the reflectance-map model itself stands for, the
inverse of ``img2refmap.refmap_mask_make``.  ``image_errors`` reports how far two images are apart on a mask.  The command line writes
``image.exr`` and the tone-mapped ``image.png`` (the mask as alpha), and with ``--input_img`` also ``errors.json`` against that image.
``render_normals_measured`` (``--merl``) shades the normal map under a measured BRDF, a MERL table (``merl.MeasuredBSDF``), instead of a
principled row; light samples under a table are not built.
Rendering runs on the GPU (no CPU path); argument errors are raised before it is touched.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .render import QUAD, _device, _env_and_view, canonical_rows, check_light_samples, view_rotation
from .synthesize import NAMES


def _normal_maps(who: str, normals, mask, B: Optional[int]):
    """what both functions ask of ``normals`` ([H, W, 3] or [Bn, H, W, 3]) and ``mask`` (None, [H, W] or [Bn, H, W]) before anything else:
    -> (Bn, H, W); with B given, Bn must be 1 or B.  A ValueError names what is wrong."""
    if not isinstance(normals, torch.Tensor):
        raise ValueError(f"{who}: normals must be a tensor [H, W, 3] or [Bn, H, W, 3]")
    if normals.dim() not in (3, 4) or normals.shape[-1] != 3:
        raise ValueError(f"{who}: normals must be [H, W, 3] or [Bn, H, W, 3], got {tuple(normals.shape)}")
    Bn, H, W = (1,) + tuple(normals.shape[:2]) if normals.dim() == 3 else tuple(normals.shape[:3])
    if not (1 <= H <= 4096 and 1 <= W <= 4096):
        raise ValueError(f"{who}: H and W must be in [1, 4096], got {(H, W)}")
    if mask is not None:
        m = torch.as_tensor(mask)
        if tuple(m.shape) not in ((H, W), (Bn, H, W)) or (m.dim() == 2 and Bn != 1):
            raise ValueError(f"{who}: mask must be [Bn={Bn}, H={H}, W={W}] like normals, got {tuple(m.shape)}")
    if B is not None and Bn not in (1, B):
        raise ValueError(f"{who}: normals holds {Bn} maps: 1 (shared) or B = {B}")
    return int(Bn), int(H), int(W)


def _gpu_only(who: str, **tensors) -> None:
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError(f"{who} runs on the GPU only (drmnet_amd has no CPU path): {name} is on {t.device}")


def _mask_on(mask, Bn: int, H: int, W: int, dev) -> Optional[torch.Tensor]:
    return None if mask is None else (torch.as_tensor(mask).to(dev) != 0).to(torch.uint8).reshape(Bn, H, W).contiguous()


@torch.no_grad()
def render_normals(normals, z, brdf_param_names: Sequence[str], envmaps: Optional[torch.Tensor] = None, *, mask=None, view_from=None,
                   quad: int = QUAD, light_samples: int = 0):
    """One call of drm_render_normals: a normal map shaded B ways.  normals [H, W, 3] or [Bn, H, W, 3] (channel-last, view frame: right, up,
    back; any length, normalised by the kernel), Bn = 1 (one map relit B ways) or B; z [B, P]; envmaps [B, EH, EW, 3] (or None: white);
    mask [Bn, H, W] (or None); view_from [B, 3] (or None: +z), which turns the environment only -> (image [B, 3, H, W], alpha [B, H, W]).
    A pixel is drawn (alpha 1) where the mask is set, the normal is neither zero nor NaN and it faces the viewer (n.z > 0); the others
    are 0 with alpha 0.  ``light_samples`` = M > 0 (a power of two in [64, 65536]) adds the light samples of ``render.render``; 0, or no
    envmaps, is the render without them bit for bit.  A bad combination is a ValueError before anything touches the GPU; a ``normals``,
    ``z`` or ``envmaps`` tensor on the CPU, or a machine without a GPU, is a RuntimeError."""
    zt = torch.as_tensor(z)
    if zt.dim() != 2 or zt.shape[-1] != len(list(brdf_param_names)):
        raise ValueError(f"render_normals: z must be [B, P = {len(list(brdf_param_names))}], got {tuple(zt.shape)}")
    B = int(zt.shape[0])
    if not 1 <= B <= 65535:
        raise ValueError(f"render_normals: B = {B} rows in [1, 65535]")
    Bn, H, W = _normal_maps("render_normals", normals, mask, B)
    light_samples = check_light_samples(light_samples)
    if isinstance(quad, bool) or not 1 <= int(quad) <= 1024:
        raise ValueError(f"render_normals: quad in [1, 1024], got {quad!r}")
    if isinstance(envmaps, torch.Tensor) and (envmaps.dim() != 4 or envmaps.shape[0] != B or envmaps.shape[3] != 3):
        raise ValueError(f"envmaps must be [B={B}, H, W, 3], got {tuple(envmaps.shape)}")
    if view_from is not None and view_rotation(view_from).shape[0] != B:
        raise ValueError(f"view_from must be [B={B}, 3], got {tuple(torch.as_tensor(view_from).shape)}")
    _gpu_only("render_normals", normals=normals, z=z, envmaps=envmaps)
    dev = _device(normals, z, envmaps)
    rows = canonical_rows(zt.to(dev), brdf_param_names).reshape(-1, 6).contiguous()
    nrm = normals.to(dev, torch.float32).reshape(Bn, H, W, 3).contiguous()
    m8 = _mask_on(mask, Bn, H, W, dev)
    env, view = _env_and_view(envmaps, view_from, B, dev)
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    shading, _keep = _lib.make_shading(B, z=rows, env=env, view=view, quad=quad, light_samples=light_samples)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_render_normals(shading, nrm.data_ptr(), _lib.ptr(m8), Bn, H, W, image.data_ptr(), alpha.data_ptr(), _lib.stream_ptr(dev)))
    return image, alpha


@torch.no_grad()
def render_normals_measured(normals, bsdfs, envmaps: Optional[torch.Tensor] = None, *, mask=None, view_from=None, quad: int = QUAD, lookup: str = "linear"):
    """One call of drm_render_normals under tables: ``render_normals`` under measured BRDFs.  ``bsdfs`` is one merl.MeasuredBSDF, shared by all rows,
    or a list of B (equal objects share one device table); B is the number of envmaps [B, EH, EW, 3], or of bsdfs under a white environment
    (None).  normals, mask and view_from as in ``render_normals``; ``lookup`` is "linear" or "nearest" -> (image [B, 3, H, W], alpha [B, H, W]),
    what ``render_normals`` returns.  There are no light samples under a table."""
    from .merl import MeasuredBSDF, device_tables, lookup_mode

    linear = lookup_mode(lookup)
    if isinstance(envmaps, torch.Tensor):
        if envmaps.dim() != 4 or envmaps.shape[3] != 3:
            raise ValueError(f"envmaps must be [B, H, W, 3], got {tuple(envmaps.shape)}")
        B = int(envmaps.shape[0])
    else:
        B = 1 if isinstance(bsdfs, MeasuredBSDF) else len(list(bsdfs))
    if not 1 <= B <= 65535:
        raise ValueError(f"render_normals_measured: B = {B} rows in [1, 65535]")
    Bn, H, W = _normal_maps("render_normals_measured", normals, mask, B)
    if isinstance(quad, bool) or not 1 <= int(quad) <= 1024:
        raise ValueError(f"render_normals_measured: quad in [1, 1024], got {quad!r}")
    if view_from is not None and view_rotation(view_from).shape[0] != B:
        raise ValueError(f"view_from must be [B={B}, 3], got {tuple(torch.as_tensor(view_from).shape)}")
    _gpu_only("render_normals_measured", normals=normals, envmaps=envmaps)
    dev = _device(normals, envmaps)
    tables, table_of, alpha = device_tables(bsdfs, B, dev)
    nrm = normals.to(dev, torch.float32).reshape(Bn, H, W, 3).contiguous()
    m8 = _mask_on(mask, Bn, H, W, dev)
    env, view = _env_and_view(envmaps, view_from, B, dev)
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    drawn = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    shading, _keep = _lib.make_shading(B, tables=(tables, table_of, alpha, linear), env=env, view=view, quad=quad)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_render_normals(shading, nrm.data_ptr(), _lib.ptr(m8), Bn, H, W, image.data_ptr(), drawn.data_ptr(), _lib.stream_ptr(dev)))
    return image, drawn


@torch.no_grad()
def image_from_refmap(refmap, normals, *, mask=None, refmask=None):
    """One call of drm_image_from_refmap: a reflectance map read at every pixel's normal.  refmap [3, R, R] or [Br, 3, R, R] (channel-first,
    as ``render.render`` and the networks give it); normals and mask as in ``render_normals``; refmask [R, R] or [Br, R, R] (or None: every
    texel observed).  B = max(Bn, Br), each of them 1 or B -> (image [B, 3, H, W], alpha [B, H, W]).  The texel coordinates are the inverse
    of the sensor's parametrisation, read bilinearly over four clamped taps (include/drmnet_hip.h states the order); with a refmask a pixel
    is drawn only if all four taps are observed.  Errors as in ``render_normals``."""
    if not isinstance(refmap, torch.Tensor) or refmap.dim() not in (3, 4) or refmap.shape[-3] != 3 or refmap.shape[-1] != refmap.shape[-2]:
        raise ValueError(f"image_from_refmap: refmap must be [3, R, R] or [Br, 3, R, R], got {tuple(getattr(refmap, 'shape', ()))}")
    Br, R = (1 if refmap.dim() == 3 else int(refmap.shape[0])), int(refmap.shape[-1])
    if not 1 <= R <= 8192:
        raise ValueError(f"image_from_refmap: R = {R} in [1, 8192]")
    if refmask is not None:
        rm = torch.as_tensor(refmask)
        if tuple(rm.shape) not in ((R, R), (Br, R, R)) or (rm.dim() == 2 and Br != 1):
            raise ValueError(f"image_from_refmap: refmask must be [Br={Br}, R={R}, R={R}] like refmap, got {tuple(rm.shape)}")
    Bn, H, W = _normal_maps("image_from_refmap", normals, mask, None)
    B = max(Bn, Br)
    if Bn not in (1, B) or Br not in (1, B) or not 1 <= B <= 65535:
        raise ValueError(f"image_from_refmap: {Bn} normal maps and {Br} reflectance maps: each 1 or B = {B} in [1, 65535]")
    _gpu_only("image_from_refmap", refmap=refmap, normals=normals)
    dev = _device(refmap, normals)
    ref = refmap.to(dev, torch.float32).reshape(Br, 3, R, R).contiguous()
    nrm = normals.to(dev, torch.float32).reshape(Bn, H, W, 3).contiguous()
    m8 = _mask_on(mask, Bn, H, W, dev)
    r8 = _mask_on(refmask, Br, R, R, dev)
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_image_from_refmap(ref.data_ptr(), _lib.ptr(r8), Br, R, nrm.data_ptr(), _lib.ptr(m8), Bn, image.data_ptr(),
                                                    alpha.data_ptr(), B, H, W, _lib.stream_ptr(dev)))
    return image, alpha


@torch.no_grad()
def rerender(DRMNet_model, Lr0: torch.Tensor, zK: torch.Tensor, normals, mask=None, *, envshape=None, quad: int = QUAD, light_samples: int = 0):
    """``estimate``'s result as an image of the object it came from: the statement order of the reference's reconstruct
    (models/drmnet.py:943-953) with the normal map in place of the sphere.  Lr0 [3, S, S] (linear, as ``estimate`` returns it) is warped to
    an environment map through r0toenvmap and ``normals`` [H, W, 3] is shaded under it with the BRDF zK [P], seen from +z
    -> (image [1, 3, H, W], alpha [1, H, W])."""
    envmap = DRMNet_model.r0toenvmap(Lr0[None], envshape or (DRMNet_model.image_size, DRMNet_model.image_size * 2))
    return render_normals(normals, zK.reshape(1, -1), DRMNet_model.brdf_param_names, envmap, mask=mask, quad=quad, light_samples=light_samples)


def _host64(a) -> np.ndarray:
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def image_errors(a, b, mask) -> Dict[str, float]:
    """How far image ``a`` is from image ``b`` on ``mask``: a, b [..., 3] (channel-last), mask [...] (non-zero = counted).  Reporting, not a
    hot path: both are brought to the host and reduced in numpy float64.
      n              the masked pixels
      rel_l2         |a - b| / |b| over their three channels (0 where both norms are 0)
      scale          <a, b> / <a, a>, the factor that brings a closest to b (0 where a is 0 everywhere)
      rel_l2_scaled  |scale a - b| / |b|: illumination and albedo share a scale ambiguity, so this is the fairer figure
      rmse_log10     root mean square of log10 a - log10 b over the n_log entries where both are > 0 (0 where there are none)"""
    a, b = _host64(a), _host64(b)
    m = _host64(mask) != 0
    if a.shape != b.shape or a.shape[-1:] != (3,) or m.shape != a.shape[:-1]:
        raise ValueError(f"image_errors: a and b must be [..., 3] and mask [...], got {a.shape}, {b.shape}, {m.shape}")
    a, b = a[m], b[m]
    nb = float(np.linalg.norm(b))

    def rel(d) -> float:
        d = float(np.linalg.norm(d))
        return d / nb if nb > 0 else (0.0 if d == 0 else float("inf"))

    aa = float(np.sum(a * a))
    scale = float(np.sum(a * b)) / aa if aa > 0 else 0.0
    both = (a > 0) & (b > 0)
    log = np.log10(a[both]) - np.log10(b[both])
    return {"n": int(m.sum()), "rel_l2": rel(a - b), "scale": scale, "rel_l2_scaled": rel(scale * a - b),
            "rmse_log10": float(np.sqrt(np.mean(log * log))) if log.size else 0.0, "n_log": int(both.sum())}


# the sums of drm_image_error_sums, in the order of include/drmnet_hip.h (DRM_IMAGE_ERROR_*)
IMAGE_SUM_NAMES = ("n", "aa", "bb", "ab", "l2", "n_log", "d", "dd", "l2_scaled", "dd_centred")


def _image_stack(who: str, name: str, x, H: int, W: int):
    """``x`` as drm_image_error_sums reads a stack: [3, H, W] / [B, 3, H, W] (channel-first) or [H, W, 3] / [B, H, W, 3] (channel-last; a
    shape that is both, H = W = 3, is read channel-last as ``image_errors`` reads it) -> (tensor [B, ., ., .] fp32, count, (batch, pixel,
    channel) strides in elements).  The tensor is ``x`` itself wherever its rows of pixels lie at one stride; it is copied only if not."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise ValueError(f"{who}: {name} must be a tensor [3, H, W], [H, W, 3] or a stack of either, got {type(x).__name__} {tuple(getattr(x, 'shape', ()))}")
    t = x if x.dim() == 4 else x[None]
    if tuple(t.shape[1:]) == (H, W, 3):
        c, h, w = 3, 1, 2
    elif tuple(t.shape[1:]) == (3, H, W):
        c, h, w = 1, 2, 3
    else:
        raise ValueError(f"{who}: {name} must be [.., 3, H={H}, W={W}] or [.., H={H}, W={W}, 3] like the mask, got {tuple(x.shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if not (H == 1 or W == 1 or t.stride(h) == W * t.stride(w)):
        t = t.contiguous()
    pixel = t.stride(w) if W > 1 else (t.stride(h) if H > 1 else 1)
    return t, int(t.shape[0]), (int(t.stride(0)), int(pixel), int(t.stride(c)))


def _check_pairs(who: str, pairs, counts) -> np.ndarray:
    """``pairs`` as int32 [P, 3] on the host, every triple inside ``counts`` = (Ba, Bb, Bm); None: row i against row i, a stack of one shared"""
    if pairs is None:
        P = max(counts)
        if any(n not in (1, P) for n in counts):
            raise ValueError(f"{who}: without pairs the stacks hold 1 or P = {P} rows each, got a {counts[0]}, b {counts[1]}, mask {counts[2]}")
        table = np.stack([np.arange(P) if n > 1 else np.zeros(P, dtype=np.int64) for n in counts], axis=1)
    else:
        table = np.asarray(pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs)
        if table.ndim != 2 or table.shape[1] != 3 or table.dtype.kind not in "iu":
            raise ValueError(f"{who}: pairs must be integers [P, 3] = (ia, ib, im), got {table.dtype} {table.shape}")
    P = int(table.shape[0])
    if not 1 <= P <= _lib.IMAGE_ERROR_MAX_PAIRS:
        raise ValueError(f"{who}: P = {P} pairs in [1, {_lib.IMAGE_ERROR_MAX_PAIRS}]")
    for col, (name, n) in enumerate(zip(("ia", "ib", "im"), counts)):
        if table[:, col].min() < 0 or table[:, col].max() >= n:
            raise ValueError(f"{who}: pairs[:, {col}] ({name}) must be in [0, {n}), got {int(table[:, col].min())} .. {int(table[:, col].max())}")
    return np.ascontiguousarray(table, dtype=np.int32)


@torch.no_grad()
def image_error_sums(a, b, mask, *, pairs=None) -> torch.Tensor:
    """One call of drm_image_error_sums (csrc/image_error.hip): P pairs of images scored on a mask in one launch sequence, nothing brought to
    the host.  a, b: [B, 3, H, W] (as ``render_normals`` returns) or [B, H, W, 3] (as ``load_exr`` gives), each its own layout, or single
    images; a strided batch goes in without a copy.  mask [H, W] or [Bm, H, W] (non-zero = counted).  pairs: integers [P, 3] = (ia, ib, im),
    1 <= P <= 4096, checked against the stacks on the host; None: row i against row i, a stack of one shared by all
    -> torch.float64 [P, 10] on the device, the sums of IMAGE_SUM_NAMES (include/drmnet_hip.h states them).  A pair gives the same bits
    alone, anywhere in any list of pairs, and in two calls.  A bad argument is a ValueError before anything touches the GPU; a tensor on
    the CPU is a RuntimeError."""
    who = "image_error_sums"
    m = torch.as_tensor(mask)
    if m.dim() not in (2, 3) or m.numel() == 0:
        raise ValueError(f"{who}: mask must be [H, W] or [Bm, H, W], got {tuple(m.shape)}")
    H, W = int(m.shape[-2]), int(m.shape[-1])
    Bm = 1 if m.dim() == 2 else int(m.shape[0])
    ta, Ba, sa = _image_stack(who, "a", a, H, W)
    tb, Bb, sb = _image_stack(who, "b", b, H, W)
    table = _check_pairs(who, pairs, (Ba, Bb, Bm))
    _gpu_only(who, a=a, b=b)
    dev = _device(a, b)
    m8 = (m.to(dev) != 0).to(torch.uint8).reshape(Bm, H * W).contiguous()
    P = int(table.shape[0])
    triples = torch.from_numpy(table).to(dev)
    nbytes = _lib.image_error_workspace_bytes(P)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    sums = torch.empty((P, _lib.IMAGE_ERROR_SUMS), dtype=torch.float64, device=dev)
    args = _lib.sized(_lib.ImageError, a=ta.data_ptr(), a_count=Ba, a_batch_stride=sa[0], a_pixel_stride=sa[1], a_channel_stride=sa[2],
                      b=tb.data_ptr(), b_count=Bb, b_batch_stride=sb[0], b_pixel_stride=sb[1], b_channel_stride=sb[2],
                      mask=m8.data_ptr(), mask_count=Bm, HW=H * W, pairs=triples.data_ptr(), P=P, workspace=ws.data_ptr(), workspace_bytes=nbytes,
                      sums=sums.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_image_error_sums(args, _lib.stream_ptr(dev)))
    return sums


def errors_from_image_sums(s) -> Dict[str, float]:
    """the figures of ``image_errors`` from one row of the ten sums, with its zero-denominator rules, and ``rmse_log10_scaled``: the log
    error once the best common factor is removed (the root mean square of d about its mean)"""
    s = np.asarray(s, dtype=np.float64)
    if s.shape != (len(IMAGE_SUM_NAMES),):
        raise ValueError(f"errors_from_image_sums: one row of {len(IMAGE_SUM_NAMES)} sums, got {s.shape}")
    n, aa, bb, ab, l2, n_log, _, dd, l2_scaled, dd_centred = (float(v) for v in s)
    nb = float(np.sqrt(bb))

    def rel(dsq: float) -> float:
        d = float(np.sqrt(dsq))
        return d / nb if nb > 0 else (0.0 if d == 0 else float("inf"))

    return {"n": int(n), "rel_l2": rel(l2), "scale": ab / aa if aa > 0 else 0.0, "rel_l2_scaled": rel(l2_scaled),
            "rmse_log10": float(np.sqrt(dd / n_log)) if n_log > 0 else 0.0, "n_log": int(n_log),
            "rmse_log10_scaled": float(np.sqrt(dd_centred / n_log)) if n_log > 0 else 0.0}


def image_errors_batch(a, b, mask, *, pairs=None):
    """``image_errors`` for P pairs at once on the GPU (``image_error_sums`` takes the arguments; one device-to-host copy of [P, 10] doubles)
    -> a list of P dicts with the keys of ``image_errors`` and ``rmse_log10_scaled``."""
    return [errors_from_image_sums(row) for row in image_error_sums(a, b, mask, pairs=pairs).cpu().numpy()]


def object_mask(input_normal: torch.Tensor, input_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """the mask rule of ``estimate``'s command line (scripts/estimate.py:127-135): |normal| > 0.5, and the PNG mask where one is given"""
    normal_mask = torch.linalg.norm(input_normal, dim=-1) > 0.5
    if input_mask is None:
        return normal_mask
    if input_mask.ndim == 3:
        input_mask = input_mask[:, :, 0]
    if input_mask.shape != normal_mask.shape:
        raise ValueError(f"the mask is {tuple(input_mask.shape)}, the normal map {tuple(normal_mask.shape)}")
    return torch.logical_and(input_mask.to(normal_mask.device), normal_mask)


def save_image(stem: Path, image: torch.Tensor, mask: torch.Tensor) -> None:
    """image [3, H, W] -> ``stem``.exr (linear) and ``stem``.png (hdr2ldr, the mask as alpha)"""
    from . import file_io
    from .transform import hdr2ldr

    hwc = image.permute(1, 2, 0).contiguous()
    file_io.save_exr(stem.with_suffix(".exr"), hwc)
    file_io.save_png(stem.with_suffix(".png"), hdr2ldr(hwc), mask=mask.to(torch.float32))


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="shade a normal map under an environment map with a principled or a measured BRDF")
    p.add_argument("--input_normal", type=Path, required=True, help="normal map of the object (.npy, H x W x 3, view frame)")
    p.add_argument("--input_mask", type=Path, default=None, help="mask of the object (.png); default: |normal| > 0.5 alone")
    p.add_argument("--envmap", type=Path, default=None, help="lat-long environment map (.exr); default: white")
    material = p.add_mutually_exclusive_group(required=True)
    material.add_argument("--z", type=float, nargs=6, metavar=("m", "R", "G", "B", "r", "s"), help="metallic, base colour R G B, roughness, specular")
    material.add_argument("--merl", type=Path, default=None, help="a measured BRDF instead: a MERL table (.binary), read trilinearly")
    p.add_argument("--view_from", type=float, nargs=3, default=None, metavar=("x", "y", "z"),
                   help="viewer position the environment is turned for (off the +-y axis); default: +z")
    p.add_argument("--quad", type=int, default=QUAD)
    p.add_argument("--light_samples", type=int, default=0, help="light samples drawn from the environment map: a power of two in [64, 65536] (default 0)")
    p.add_argument("--input_img", type=Path, default=None, help="HDR image of the object (.exr) to compare against: writes errors.json")
    p.add_argument("--output_dir", type=Path, required=True)
    return p


def main(argv=None):
    from . import file_io

    ap = parser()
    args = ap.parse_args(argv)
    if args.merl is not None and args.light_samples != 0:
        ap.error("--light_samples with --merl: light samples under a table are not built")
    check_light_samples(args.light_samples)
    if not 1 <= args.quad <= 1024:
        raise ValueError(f"quad in [1, 1024], got {args.quad}")
    view = None if args.view_from is None else torch.tensor([args.view_from], dtype=torch.float32)
    if view is not None:
        view_rotation(view)  # (a view along +-y is a ValueError here)
    normal = torch.from_numpy(np.load(args.input_normal)).to(torch.float32)
    if normal.dim() != 3 or normal.shape[-1] != 3:
        raise ValueError(f"{args.input_normal}: a normal map is [H, W, 3], got {tuple(normal.shape)}")
    mask = object_mask(normal, None if args.input_mask is None else file_io.load_png(args.input_mask, as_torch=True))
    target = None if args.input_img is None else file_io.load_exr(args.input_img, as_torch=True)
    if target is not None and target.shape != normal.shape:
        raise ValueError(f"{args.input_img} is {tuple(target.shape)}, the normal map {tuple(normal.shape)}")
    env = None if args.envmap is None else file_io.load_exr(args.envmap, as_torch=True)
    if not torch.cuda.is_available():
        raise RuntimeError("relight renders on the GPU (drmnet_amd has no CPU path) and no GPU is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.merl is not None:
        from .merl import MeasuredBSDF

        image, _ = render_normals_measured(normal.to(dev), MeasuredBSDF.from_file(args.merl), None if env is None else env.to(dev)[None],
                                           mask=mask.to(dev), view_from=view, quad=args.quad)
    else:
        image, _ = render_normals(normal.to(dev), torch.tensor([args.z], dtype=torch.float32, device=dev), NAMES, None if env is None else env.to(dev)[None],
                                  mask=mask.to(dev), view_from=view, quad=args.quad, light_samples=args.light_samples)
    args.output_dir.mkdir(parents=True, exist_ok=True)
    save_image(args.output_dir / "image", image[0], mask.to(dev))
    print(f"wrote image.exr and image.png ({int(mask.sum())} of {mask.numel()} pixels) to {args.output_dir}")
    if target is not None:
        errors = image_errors(image[0].permute(1, 2, 0), target, mask)
        (args.output_dir / "errors.json").write_text(json.dumps(errors, indent=1) + "\n")
        print("errors against", args.input_img, json.dumps(errors))


if __name__ == "__main__":
    main()

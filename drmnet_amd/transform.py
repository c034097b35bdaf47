"""The sphere / environment-map warps and the LDR tone map, on the HIP kernels.

``mirmap2envmap`` / ``hdr2ldr`` keep the reference's names and arguments (utils/transform.py:106-144, utils/tonemap.py:4-9);
the work is done by csrc/transform.hip: one gather kernel that evaluates the warp geometry per envmap texel and fetches with
grid_sample's bilinear / border / align_corners=False arithmetic, and one reduce-then-map kernel for the tone map.

``envmap2mirmap``, ``rotate_envmap``, ``mirimg2envmap`` and ``refmap2refimg_torch`` are the rest of the reference's warp family
(utils/transform.py:170-363) on csrc/sphere_warp.hip, with the reference's names, argument names and defaults.  Their frame vectors are
built here, on the host in fp32 torch ops as the reference builds them (``top`` re-orthogonalised against ``view_from``, a binormal =
cross(normal, tangent), negated for reverse_phi) and handed to the kernel per item, so every frame the reference accepts works.  Like the
reference (``assume_normalized``) the vectors are used as given: pass unit vectors.  Two extensions: a frame argument may be [B, 3], one
frame per item (the reference handles [3] only; a batched call equals the per-item calls bit for bit, the re-orthogonalisation being
decided per item), and ``channels_last=True`` reads the input as [B, H, W, C], what ``file_io.load_exr`` and the renderers give.  The
output is [B, C, OH, OW] either way.  GPU only, like the rest of the package.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops


def mirmap2envmap(mirmap: torch.Tensor, output_shape: Tuple[int, int], view: Union[torch.Tensor, List[float]] = [0, 0, 1],
                  top: Union[torch.Tensor, List[float]] = [0, 1, 0], envmap_zenith: Union[torch.Tensor, List[float]] = [0, 1, 0],
                  envmap_left_edge: Union[torch.Tensor, List[float]] = [0, 0, -1], reverse_azimuth: bool = True,
                  log_scale_interpolation: bool = False) -> torch.Tensor:
    """mirmap [B, C, H, W] -> envmap [B, C, OH, OW].  Only the geometry the reference itself supports and uses is built into the
    kernel (``assert view == [0, 0, 1]`` at utils/transform.py:117 and the default frame everywhere it is called)."""
    as_list = lambda v: [float(t) for t in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    assert as_list(view) == [0, 0, 1], "now support [0,0,1] view direction"
    if as_list(top) != [0, 1, 0] or as_list(envmap_zenith) != [0, 1, 0] or as_list(envmap_left_edge) != [0, 0, -1] or not reverse_azimuth:
        raise NotImplementedError("only the default frame (top/zenith +y, left edge -z, reversed azimuth) is built into the kernel")
    return ops.mirmap2envmap(mirmap, output_shape, log_scale_interpolation=log_scale_interpolation)


def hdr2ldr(x, mask=None, alpha: float = 0.18, gamma: float = 2.2):
    """utils/tonemap.py:4-9.  Accepts what the reference is given (a [H, W, 3] numpy array -> numpy array) as well as a device
    tensor (-> device tensor); numpy input is staged through the current GPU."""
    if isinstance(x, torch.Tensor):
        return ops.hdr2ldr(x, mask, alpha, gamma)
    dev = torch.device("cuda", torch.cuda.current_device())
    m = None if mask is None else torch.as_tensor(np.asarray(mask)).to(dev)
    return ops.hdr2ldr(torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(dev), m, alpha, gamma).cpu().numpy()


Vector = Union[torch.Tensor, np.ndarray, List[float]]


def _vectors(v, B: int, name: str) -> torch.Tensor:
    """a frame argument, [3] (shared) or [B, 3] (per item) -> [B, 3] fp32 on the host"""
    t = torch.as_tensor(np.asarray(v.detach().cpu()) if isinstance(v, torch.Tensor) else np.asarray(v), dtype=torch.float32)
    if tuple(t.shape) not in ((3,), (B, 3)):
        raise ValueError(f"{name} must be [3] or [B={B}, 3], got {tuple(t.shape)}")
    return t.reshape(-1, 3).expand(B, 3).contiguous()


def _reorthogonalised(view_from: torch.Tensor, top: torch.Tensor) -> torch.Tensor:
    """utils/transform.py:217-218 per item: top <- normalize(cross(cross(view_from, top), view_from)) where dot(view_from, top) != 0"""
    dot = torch.einsum("...i, ...i -> ...", view_from, top)
    cross = torch.linalg.cross
    fixed = torch.nn.functional.normalize(cross(cross(view_from, top, dim=-1), view_from, dim=-1), dim=-1, eps=1e-12)
    return torch.where((dot != 0)[:, None], fixed, top)


def _frame(normal: torch.Tensor, tangent: torch.Tensor, reverse_phi: bool) -> List[torch.Tensor]:
    """the three rows thetaphi2xyz / xyz2thetaphi use (utils/transform.py:45-47, 84-86)"""
    binormal = torch.linalg.cross(normal, tangent, dim=-1)
    if reverse_phi:
        binormal = binormal * -1
    return [normal, tangent, binormal]


def envmap2mirmap_frames(B: int, flip_horizontal=False, view_from: Vector = [1, 0, 0], top: Vector = [0, 1, 0], envmap_zenith: Vector = [0, 1, 0],
                         envmap_left_edge: Vector = [0, 0, -1], reverse_azimuth_envmap=True) -> torch.Tensor:
    """the [B, 6, 3] frames of drm_envmap2mirmap (host tensor)"""
    view_from, top = _vectors(view_from, B, "view_from"), _vectors(top, B, "top")
    top = _reorthogonalised(view_from, top)
    return torch.stack(_frame(top, view_from, flip_horizontal)
                       + _frame(_vectors(envmap_zenith, B, "envmap_zenith"), _vectors(envmap_left_edge, B, "envmap_left_edge"), reverse_azimuth_envmap), dim=1)


def rotate_envmap_frames(B: int, src_envmap_zenith: Vector, src_envmap_left_edge: Vector, tgt_envmap_zenith: Vector,
                         tgt_envmap_left_edge: Vector) -> torch.Tensor:
    """the [B, 6, 3] frames of drm_rotate_envmap (host tensor)"""
    return torch.stack(_frame(_vectors(tgt_envmap_zenith, B, "tgt_envmap_zenith"), _vectors(tgt_envmap_left_edge, B, "tgt_envmap_left_edge"), True)
                       + _frame(_vectors(src_envmap_zenith, B, "src_envmap_zenith"), _vectors(src_envmap_left_edge, B, "src_envmap_left_edge"), True), dim=1)


def mirimg2envmap_frames(B: int, view_from: Vector = [0, 0, 1], top: Vector = [0, 1, 0], envmap_zenith: Vector = [0, 1, 0],
                         envmap_left_edge: Vector = [0, 0, -1], reverse_azimuth=True) -> torch.Tensor:
    """the [B, 7, 3] frames of drm_mirimg2envmap (host tensor)"""
    view_from, top = _vectors(view_from, B, "view_from"), _vectors(top, B, "top")
    top = _reorthogonalised(view_from, top)
    return torch.stack(_frame(_vectors(envmap_zenith, B, "envmap_zenith"), _vectors(envmap_left_edge, B, "envmap_left_edge"), reverse_azimuth)
                       + _frame(top, torch.linalg.cross(view_from, top, dim=-1), False) + [view_from], dim=1)


def _items(x: torch.Tensor, name: str) -> int:
    if not isinstance(x, torch.Tensor) or x.ndim != 4:
        raise ValueError(f"{name} must be a 4-D tensor, got {tuple(getattr(x, 'shape', ()))}")
    return int(x.shape[0])


def envmap2mirmap(envmap: torch.Tensor, output_shape: Tuple[int, int], flip_horizontal: bool = False, view_from: Vector = [1, 0, 0],
                  top: Vector = [0, 1, 0], envmap_zenith: Vector = [0, 1, 0], envmap_left_edge: Vector = [0, 0, -1],
                  reverse_azimuth_envmap: bool = True, mitigate_aliasing: bool = True, log_scale_interpolation: bool = False, *,
                  channels_last: bool = False) -> torch.Tensor:
    """utils/transform.py:201-242: envmap [B, C, H, W] seen in a mirror ball from ``view_from`` -> the mirror reflectance map
    [B, C, OH, OW].  The reference's grid_sample on an S x S grid and its adaptive_avg_pool2d are one kernel; S x S is never stored."""
    frames = envmap2mirmap_frames(_items(envmap, "envmap"), flip_horizontal, view_from, top, envmap_zenith, envmap_left_edge, reverse_azimuth_envmap)
    return ops.envmap2mirmap(envmap, output_shape, frames, mitigate_aliasing, log_scale_interpolation, channels_last)


def mirimg2envmap(refimg: torch.Tensor, output_shape: Tuple[int, int], view_from: Vector = [0, 0, 1], top: Vector = [0, 1, 0],
                  envmap_zenith: Vector = [0, 1, 0], envmap_left_edge: Vector = [0, 0, -1], reverse_azimuth: bool = True,
                  log_scale_interpolation: bool = False, *, channels_last: bool = False) -> torch.Tensor:
    """utils/transform.py:245-284: the orthographic mirror-ball image refimg [B, C, H, W] -> the lat-long map [B, C, OH, OW]"""
    frames = mirimg2envmap_frames(_items(refimg, "refimg"), view_from, top, envmap_zenith, envmap_left_edge, reverse_azimuth)
    return ops.mirimg2envmap(refimg, output_shape, frames, log_scale_interpolation, channels_last)


def rotate_envmap(envmap: torch.Tensor, src_envmap_zenith: Vector = [0, 1, 0], src_envmap_left_edge: Vector = [0, 0, -1],
                  tgt_envmap_zenith: Optional[Vector] = None, tgt_envmap_left_edge: Optional[Vector] = None, out_shape: Optional[Tuple] = None, *,
                  channels_last: bool = False) -> torch.Tensor:
    """utils/transform.py:317-363: envmap [B, C, H, W], given in the source frame, re-expressed in the target frame -> [B, C, OH, OW]
    (``out_shape``, default (H, W)).  The target frame has no default that works in the reference either: leaving it None is a ValueError."""
    if tgt_envmap_zenith is None or tgt_envmap_left_edge is None or src_envmap_zenith is None or src_envmap_left_edge is None:
        raise ValueError("rotate_envmap needs both frames: src_envmap_zenith / _left_edge and tgt_envmap_zenith / _left_edge")
    B = _items(envmap, "envmap")
    frames = rotate_envmap_frames(B, src_envmap_zenith, src_envmap_left_edge, tgt_envmap_zenith, tgt_envmap_left_edge)
    if out_shape is None:
        out_shape = tuple(envmap.shape[1:3]) if channels_last else tuple(envmap.shape[-2:])
    return ops.rotate_envmap(envmap, out_shape, frames, channels_last)


def refmap2refimg_torch(refmap: torch.Tensor, radius: Optional[int] = None, return_mask: bool = False, *, channels_last: bool = False):
    """utils/transform.py:170-198: a reflectance map [(B), C, H, W] -> the ball image [(B), C, 2 radius, 2 radius] (``radius`` defaults
    to max(H, W)), zero outside the disc; with ``return_mask`` also the disc [2 radius, 2 radius] (bool)."""
    if not isinstance(refmap, torch.Tensor) or refmap.ndim not in (3, 4):
        raise ValueError(f"refmap must be [C, H, W] or [B, C, H, W], got {tuple(getattr(refmap, 'shape', ()))}")
    batched = refmap.ndim == 4
    x = refmap if batched else refmap[None]
    if radius is None:
        radius = max(x.shape[1:3]) if channels_last else max(x.shape[-2:])
    image, mask = ops.refmap2refimg(x, int(radius), channels_last)
    if not batched:
        image = image[0]
    return (image, mask) if return_mask else image

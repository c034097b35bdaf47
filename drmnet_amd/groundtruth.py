"""The true illumination in the two forms ``estimate`` answers in, and how far an estimate is from it.

``synthesize`` makes an object image from a mesh, a BRDF and a world-frame environment map seen from ``view_from``; ``estimate`` recovers
``Lr0``, the mirror reflectance map, and through ``r0toenvmap`` an environment map in the camera's frame.  With the map and the view that
made the image, ``gt_mirror_map`` is the map ``Lr0`` should equal and ``gt_camera_envmap`` the one the estimated map should equal; both are
warps of csrc/sphere_warp.hip (``transform.envmap2mirmap`` / ``rotate_envmap``).  ``illumination_errors`` compares the two pairs with
``relight.image_errors``, whose ``scale``, ``rel_l2_scaled`` and ``rmse_log10`` allow for the scale ambiguity between illumination and
albedo.  The warps run on the GPU; the figures are reporting, reduced on the host in float64.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .relight import image_errors
from .render import view_rotation
from .transform import envmap2mirmap, rotate_envmap


def _maps_and_views(envmap: torch.Tensor, view_from) -> Tuple[torch.Tensor, torch.Tensor]:
    """envmap [H, W, 3] or [B, H, W, 3] (channel-last, as file_io.load_exr and the renderers give it) and view_from [3] or [B, 3]
    -> ([B, H, W, 3], the rotations [B, 3, 3] with columns (right, up', back))"""
    if not isinstance(envmap, torch.Tensor) or envmap.dim() not in (3, 4) or envmap.shape[-1] != 3:
        raise ValueError(f"envmap must be [H, W, 3] or [B, H, W, 3], got {tuple(getattr(envmap, 'shape', ()))}")
    env = envmap if envmap.dim() == 4 else envmap[None]
    rot = view_rotation(view_from)
    if rot.shape[0] not in (1, env.shape[0]):
        raise ValueError(f"view_from must be [3] or [B={env.shape[0]}, 3], got {tuple(torch.as_tensor(view_from).shape)}")
    return env.to(torch.float32), rot.expand(env.shape[0], 3, 3)


@torch.no_grad()
def gt_mirror_map(envmap: torch.Tensor, view_from, res: int) -> torch.Tensor:
    """The mirror reflectance map of ``envmap`` for a viewer at ``view_from`` -> [B, 3, res, res], in the orientation ``mirmap2envmap``
    inverts (``flip_horizontal=False``: the round trip returns a smooth map to 2e-3, the flipped one is off by 0.6)."""
    env, rot = _maps_and_views(envmap, view_from)
    return envmap2mirmap(env, (int(res), int(res)), view_from=rot[:, :, 2], flip_horizontal=False, channels_last=True)


@torch.no_grad()
def gt_camera_envmap(envmap: torch.Tensor, view_from, shape: Tuple[int, int]) -> torch.Tensor:
    """``envmap`` (world frame: zenith +y, left edge -z) re-expressed in the camera's frame (zenith up', left edge -back), the frame
    ``r0toenvmap`` answers in -> [B, OH, OW, 3], channel-last like ``r0toenvmap``'s."""
    env, rot = _maps_and_views(envmap, view_from)
    out = rotate_envmap(env, [0, 1, 0], [0, 0, -1], tgt_envmap_zenith=rot[:, :, 1], tgt_envmap_left_edge=-rot[:, :, 2],
                        out_shape=(int(shape[0]), int(shape[1])), channels_last=True)
    return out.permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def illumination_errors(Lr0: torch.Tensor, envmap_est: torch.Tensor, envmap_gt: torch.Tensor, view_from, *,
                        maps: Optional[dict] = None) -> Dict[str, Dict[str, float]]:
    """One estimate against the truth: Lr0 [3, S, S] and envmap_est [H, W, 3] as ``estimate`` and ``r0toenvmap`` return them, envmap_gt
    [EH, EW, 3] in the world frame, view_from [3] -> {"mirror_map": image_errors(Lr0, gt_mirror_map), "envmap": image_errors(envmap_est,
    gt_camera_envmap)}, every texel counted.  ``maps``, if given, receives the two ground-truth maps under the same keys
    ([3, S, S] and [H, W, 3])."""
    if Lr0.dim() != 3 or Lr0.shape[0] != 3 or Lr0.shape[1] != Lr0.shape[2]:
        raise ValueError(f"Lr0 must be [3, S, S], got {tuple(Lr0.shape)}")
    if envmap_est.dim() != 3 or envmap_est.shape[-1] != 3 or envmap_gt.dim() != 3:
        raise ValueError(f"envmap_est and envmap_gt must be [H, W, 3], got {tuple(envmap_est.shape)} and {tuple(envmap_gt.shape)}")
    mirror = gt_mirror_map(envmap_gt, view_from, Lr0.shape[-1])[0]
    camera = gt_camera_envmap(envmap_gt, view_from, envmap_est.shape[:2])[0]
    if maps is not None:
        maps.update(mirror_map=mirror, envmap=camera)
    ones = lambda t: torch.ones(tuple(t.shape[:2]), dtype=torch.bool)
    mirror_hwc = mirror.permute(1, 2, 0)
    return {"mirror_map": image_errors(Lr0.permute(1, 2, 0), mirror_hwc, ones(mirror_hwc)),
            "envmap": image_errors(envmap_est, camera, ones(camera))}

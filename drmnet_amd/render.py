"""The forward model DRMNet inverts -- reflectance maps of a sphere under an environment map -- on csrc/render.hip.

Operator surface of the reference's Mitsuba 3 helpers (utils/mitsuba3_utils.py): ``RefMapRenderer`` stands in for
``MitsubaRefMapRenderer`` (:324-430), ``get_bsdf`` / ``eval_bsdf`` / ``visualize_bsdf`` keep their names and arguments (:528-640).
The BSDF is the ``principled`` subset DRMNet's configs use (metallic, base colour, roughness, specular); a parameter row is mapped
once on the host to the canonical ``(metallic, R, G, B, roughness, specular)`` the kernels read.  Constructing anything here does
not touch the GPU; rendering and evaluation run there (no CPU path).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

# canonical row: (metallic, base colour R, G, B, roughness, specular); unnamed parameters keep the reference scene dict's principled values
CANONICAL = ("metallic", "base_color.R", "base_color.G", "base_color.B", "roughness", "specular")
DEFAULT_ROW = (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
_SCALAR = {"metallic": 0, "metallic.value": 0, "roughness": 4, "roughness.value": 4, "specular": 5}
_RGB = ("base_color.value.R", "base_color.value.G", "base_color.value.B")
QUAD, SUBPIXEL = 32, 2


def canonical_rows(z, brdf_param_names: Sequence[str]) -> torch.Tensor:
    """z [..., P] in the order of ``brdf_param_names`` -> [..., 6] canonical rows, every value clipped to [0, 1] (get_bsdf /
    _render_scene).  Names other than metallic[.value], base_color.value[.R/.G/.B], roughness[.value] and specular raise."""
    z = torch.as_tensor(z, dtype=torch.float32)
    names = list(brdf_param_names)
    if z.shape[-1] != len(names):
        raise ValueError(f"z has {z.shape[-1]} parameters, brdf_param_names {len(names)}")
    rows = torch.tensor(DEFAULT_ROW, dtype=torch.float32, device=z.device).expand(*z.shape[:-1], 6).clone()
    zc = z.clip(0, 1)
    rgb = [n for n in names if n in _RGB]
    if rgb and len(rgb) != 3:
        raise NotImplementedError("base_color.value.R / .G / .B come together")
    for k, name in enumerate(names):
        if name in _SCALAR:
            rows[..., _SCALAR[name]] = zc[..., k]
        elif name == "base_color.value":
            rows[..., 1:4] = zc[..., k:k + 1]
        elif name in _RGB:
            rows[..., 1 + _RGB.index(name)] = zc[..., k]
        else:
            raise NotImplementedError(f"BSDF parameter {name!r}: the renderer models metallic, base_color, roughness and specular "
                                      "(spec_tint, sheen, clearcoat, anisotropic, spec_trans, flatness are 0 in every shipped config)")
    return rows


def _device(*tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("rendering runs on the GPU (drmnet_amd has no CPU path) and no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def view_rotation(view_from) -> torch.Tensor:
    """view_from [B, 3] (or [3]) -> the row-major rotations [B, 3, 3] a drm_shading's view holds: the reference's
    look_at(origin=view_from, target=0, up=+y) (utils/mitsuba3_utils.py:394-396) with columns (right, up', back), back = v / |v|,
    right = normalize(+y x back), up' = back x right.  [0, 0, d > 0] gives the identity exactly; a view along +-y has no right vector and is
    a ValueError.  Built on the host (a [B, 3] input on the GPU is brought over: view positions are per-item metadata)."""
    v = torch.as_tensor(view_from).detach().to("cpu", torch.float32).reshape(-1, 3)
    back = v / torch.linalg.norm(v, dim=-1, keepdim=True)
    right = torch.stack([back[:, 2], torch.zeros_like(back[:, 0]), -back[:, 0]], dim=-1)  # +y x back
    length = torch.linalg.norm(right, dim=-1, keepdim=True)
    if not bool(torch.isfinite(back).all()) or bool((length < 1e-6).any()):
        raise ValueError("view_from must be a non-zero position off the +-y axis (look_at with up = +y has no right vector there)")
    right = right / length
    up = torch.linalg.cross(back, right, dim=-1)
    return torch.stack([right, up, back], dim=-1).contiguous()


def _env_and_view(envmaps, view_from, B: int, dev: torch.device):
    """envmaps [B, H, W, 3] (or None: white) and view_from [B, 3] (or None: +z), checked against B and brought to ``dev`` ->
    (env, view [B, 3, 3]); None for what is not given."""
    env, view = None, None
    if envmaps is not None:
        env = envmaps.to(dev, torch.float32)
        if env.dim() != 4 or env.shape[0] != B or env.shape[3] != 3:
            raise ValueError(f"envmaps must be [B={B}, H, W, 3], got {tuple(env.shape)}")
        env = env.contiguous()
    if view_from is not None:
        view = view_rotation(view_from)
        if view.shape[0] != B:
            raise ValueError(f"view_from must be [B={B}, 3], got {tuple(torch.as_tensor(view_from).shape)}")
        view = view.to(dev)
    return env, view


light_samples_error = _lib.light_samples_error


def check_light_samples(light_samples) -> int:
    """``light_samples`` as an int: 0 (none) or a power of two in [64, 65536]; anything else is a ValueError (a renderer's constructor asks this;
    ``_lib.make_shading`` learns the same from drm_render_light_workspace_bytes, which answers 0 for what the library will not take)"""
    m = int(light_samples)
    if m and (m < 64 or m > 65536 or m & (m - 1)):
        raise light_samples_error(light_samples)
    return m


@torch.no_grad()
def render(z, brdf_param_names: Sequence[str], envmaps: Optional[torch.Tensor] = None, *, res: int = 128, quad: int = QUAD,
           subpixel: int = SUBPIXEL, flip: bool = False, view_from=None, light_samples: int = 0) -> torch.Tensor:
    """One launch of drm_render_refmap: z [B, P] or [L, B, P], envmaps [B, H, W, 3] (or None: white), view_from [B, 3] (or None: +z)
    -> reflectance maps [B, 3, res, res] or [L, B, 3, res, res].  The L rows of a batch item read the same map: nothing is expanded.
    ``light_samples`` = M > 0 (a power of two in [64, 65536]) adds light samples: M directions drawn from each map's own
    light density join the two lobe quadratures by multiple importance sampling, which is what a map with a sun or a lamp a few texels wide
    needs (the plain quadrature can be 10 % off there).  0, or no envmaps, is the plain render bit for bit."""
    dev = _device(z, envmaps)
    z = torch.as_tensor(z).to(dev)
    if z.dim() not in (2, 3):
        raise ValueError(f"z must be [B, P] or [L, B, P], got {tuple(z.shape)}")
    stacked = z.dim() == 3
    L, B = (z.shape[0], z.shape[1]) if stacked else (1, z.shape[0])
    rows = canonical_rows(z, brdf_param_names).reshape(-1, 6).contiguous()
    env, view = _env_and_view(envmaps, view_from, B, dev)
    out = torch.empty((L * B, 3, res, res), dtype=torch.float32, device=dev)
    shading, _keep = _lib.make_shading(B, z=rows, env=env, view=view, quad=quad, light_samples=light_samples)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_render_refmap(shading, L, int(res), int(subpixel), int(bool(flip)), out.data_ptr(), _lib.stream_ptr(dev)))
    return out.reshape(L, B, 3, res, res) if stacked else out


class RefMapRenderer:
    """MitsubaRefMapRenderer (utils/mitsuba3_utils.py:324-430) on drm_render_refmap: the sphere seen from +z under the scene's
    environment map, ``direct`` integration, box-filtered pixels.  The integral is a deterministic quadrature (``quad`` x ``quad``
    points per lobe at ``subpixel`` x ``subpixel`` normals per pixel), so ``spp`` and ``denoise`` are accepted and ignored: there is
    no Monte-Carlo noise to average or denoise.  ``light_samples`` = M > 0 adds M light samples per map (see ``render``; reachable from a YAML
    ``renderer_config``); the default 0 is the plain quadrature.  A per-call ``view_from`` turns the environment (render.view_rotation); a scene whose own
    sensor is off the +z axis (``init_view_from``) and the normal / depth outputs are not implemented.  Construction does not touch the GPU."""

    def __init__(self, refmap_res: int, spp: int = 1024, envmap_size=(1000, 2000), denoise: Optional[str] = None, return_normal: bool = False,
                 return_depth: bool = False, init_view_from=(0, 0, 1.1), brdf_param_names: Optional[List[str]] = None, *, quad: int = QUAD,
                 subpixel: int = SUBPIXEL, light_samples: int = 0):
        if return_normal or return_depth:
            raise NotImplementedError("normal / depth outputs of the reflectance-map renderer")
        view = [float(t) for t in init_view_from]
        if view[0] != 0 or view[1] != 0 or view[2] <= 0:
            raise NotImplementedError("only the view from +z (init_view_from = [0, 0, d > 0]) is modelled")
        self.refmap_res = int(refmap_res)
        self.image_size = (self.refmap_res, self.refmap_res)
        self.envmap_size = tuple(int(s) for s in envmap_size)
        self.spp, self.denoise = spp, denoise
        self.return_normal, self.return_depth = return_normal, return_depth
        self.brdf_param_names = brdf_param_names
        self.quad, self.subpixel = int(quad), int(subpixel)
        self.light_samples = check_light_samples(light_samples)
        self.flip = False
        self._envmap: Optional[torch.Tensor] = None  # the scene's map; None = the initial all-zero bitmap of envmap_size
        self._view_from: Optional[torch.Tensor] = None  # the scene's view; None = the sensor's own (+z)

    def render(self, z, brdf_param_names=None, envmaps=None, *, res: Optional[int] = None, flip: Optional[bool] = None, view_from=None) -> torch.Tensor:
        """Batched form: z [B, P] or [L, B, P], envmaps [B, H, W, 3] or None (white), view_from [B, 3] or None (+z) -> [(L,) B, 3, R, R] in
        one launch."""
        return render(z, brdf_param_names or self.brdf_param_names, envmaps, res=res or self.refmap_res, quad=self.quad, subpixel=self.subpixel,
                      flip=self.flip if flip is None else flip, view_from=view_from, light_samples=self.light_samples)

    def rendering(self, z, brdf_param_names, envmap: Optional[torch.Tensor] = None, view_from=None, flip: Optional[bool] = None, sensor=0,
                  spp: int = 0, new_scene: bool = False, channel_first: bool = False) -> torch.Tensor:
        """utils/mitsuba3_utils.py:416-430: one reflectance map [R, R, 3] ([3, R, R] with channel_first).  ``envmap`` [H, W, 3] replaces
        the scene's map (``new_scene``: for this call only); None reuses it.  ``view_from`` [3] moves the viewer and, like the map, stays
        with the scene for later calls (the reference updates the scene's sensor, :394-396).  ``flip`` mirrors the sensor (kept for later
        calls)."""
        if not (isinstance(sensor, int) and sensor == 0):
            raise NotImplementedError("only the scene's own sensor (sensor=0) is modelled")
        if envmap is not None:
            assert isinstance(envmap, torch.Tensor) and envmap.dim() == 3 and not torch.isnan(envmap[0, 0, 0]), f"envmap [{envmap.shape}]"
        dev = _device(z, envmap)
        if new_scene:
            if envmap is None:
                raise ValueError("new_scene needs an envmap")
            env = envmap.to(dev)
            view = view_from
        else:
            if flip is not None:
                self.flip = bool(flip)
            if envmap is not None:
                self._envmap = envmap.to(dev)
            if self._envmap is None:
                self._envmap = torch.zeros(*self.envmap_size, 3, device=dev)
            env = self._envmap
            if view_from is not None:
                self._view_from = torch.as_tensor(view_from).detach().to("cpu", torch.float32).reshape(3)
            view = self._view_from
        z = torch.as_tensor(z).reshape(1, -1)
        img = self.render(z, brdf_param_names, env[None], flip=flip if new_scene else None,
                          view_from=None if view is None else torch.as_tensor(view).reshape(1, 3))[0]
        return img if channel_first else img.permute(1, 2, 0)


class PrincipledBSDF:
    """get_bsdf's result: one principled BSDF as its canonical row (``row``: metallic, R, G, B, roughness, specular)."""

    def __init__(self, row):
        self.row = [float(v) for v in row]

    def __repr__(self):
        return "PrincipledBSDF(" + ", ".join(f"{k}={v:g}" for k, v in zip(CANONICAL, self.row)) + ")"


def get_bsdf(z, brdf_param_names: Sequence[str]) -> PrincipledBSDF:
    """utils/mitsuba3_utils.py:528-552: the BSDF of parameter vector z [P] (clipped to [0, 1])."""
    return PrincipledBSDF(canonical_rows(torch.as_tensor(z).detach().float().cpu(), brdf_param_names).tolist())


def _as_rows(a, n: int) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.asarray(a, dtype=np.float32).reshape(-1, 3)
    # (a row-major copy, as the kernels read it: copied in "K" order a broadcast view keeps its axis order and comes out column-major)
    return np.array(np.broadcast_to(a, (n, 3)), order="C")


@torch.no_grad()
def eval_bsdf(bsdf, normal, wo, wi, *, lookup: str = "nearest") -> np.ndarray:
    """utils/mitsuba3_utils.py:610-626: f(wi, wo) (n.wo) of Mitsuba's eval for wi toward the viewer and wo toward the light; each of
    normal / wo / wi is one vector [3] or N vectors [N, 3] (unit length).  Returns [N, 3] (numpy), evaluated by drm_brdf_eval for a
    PrincipledBSDF and by drm_merl_eval for a merl.MeasuredBSDF, whose table is read as ``lookup`` says: "nearest" (the default: the MERL
    distribution reader's rule) or "linear"."""
    from .merl import MeasuredBSDF, lookup_mode

    n = max(int(np.size(a) // 3) for a in (normal, wo, wi))
    arrs = [torch.from_numpy(_as_rows(a, n)) for a in (normal, wi, wo)]
    measured = isinstance(bsdf, MeasuredBSDF)
    linear = lookup_mode(lookup) if measured else 0
    dev = _device()
    nrm, v, l = (a.to(dev) for a in arrs)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if measured:
            table = bsdf.device_table(dev)
            _lib.check(_lib.lib().drm_merl_eval(table.data_ptr(), 1, None, nrm.data_ptr(), v.data_ptr(), l.data_ptr(), out.data_ptr(), n, linear,
                                                _lib.stream_ptr(dev)))
        else:
            z = torch.tensor(bsdf.row, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().drm_brdf_eval(z.data_ptr(), 1, nrm.data_ptr(), v.data_ptr(), l.data_ptr(), out.data_ptr(), n, _lib.stream_ptr(dev)))
    return out.cpu().numpy()


@torch.no_grad()
def render_table(bsdfs, envmaps: Optional[torch.Tensor] = None, *, res: int = 128, quad: int = QUAD, subpixel: int = SUBPIXEL, flip: bool = False,
                 view_from=None, lookup: str = "linear") -> torch.Tensor:
    """One launch of drm_render_refmap under tables: the sphere of ``render`` under measured BRDFs.  ``bsdfs`` is one merl.MeasuredBSDF, shared by
    all rows, or a list of B (equal objects share one device table); envmaps [B, H, W, 3] (or None: white, and then B = len(bsdfs), 1 for a
    single one); view_from [B, 3] (or None: +z) -> reflectance maps [B, 3, res, res].  Each table is sampled with its own proxy roughness
    (``MeasuredBSDF.alpha``) and read as ``lookup`` says ("linear" or "nearest")."""
    from .merl import MeasuredBSDF, device_tables, lookup_mode

    linear = lookup_mode(lookup)
    dev = _device(envmaps)
    if envmaps is not None:
        B = int(envmaps.shape[0])
    else:
        B = 1 if isinstance(bsdfs, MeasuredBSDF) else len(list(bsdfs))
    if not 1 <= B <= 65535:
        raise ValueError(f"render_table: B = {B} rows in [1, 65535]")
    tables, table_of, alpha = device_tables(bsdfs, B, dev)
    env, view = _env_and_view(envmaps, view_from, B, dev)
    out = torch.empty((B, 3, res, res), dtype=torch.float32, device=dev)
    shading, _keep = _lib.make_shading(B, tables=(tables, table_of, alpha, linear), env=env, view=view, quad=quad)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_render_refmap(shading, 1, int(res), int(subpixel), int(bool(flip)), out.data_ptr(), _lib.stream_ptr(dev)))
    return out


def visualize_layout(increment_deg: float = 30, imsize=(512, 512), angle_start: float = 0):
    """The geometry of visualize_bsdf's figure: a row of spheres, one per light angle angle_start, angle_start + increment_deg, ... < 180
    degrees, each imsize wide and placed half a width after the previous one (a later sphere covers the earlier one where they overlap);
    sphere k is lit from wo = (-sin a_k, 0, -cos a_k).  Returns (normal [H, W, 3], wo [H, W, 3], mask [H, W] bool), W = imsize[0] (count + 1) // 2."""
    w, h = int(imsize[0]), int(imsize[1])
    angles = np.arange(angle_start, 180, increment_deg)
    W = (w * (len(angles) + 1)) // 2
    # the sphere normals of one imsize tile (both coordinates scaled by the width, as the reference does)
    xs = 2.0 * (np.arange(w) + 0.5) / w - 1.0
    ys = 2.0 * (np.arange(h) + 0.5) / w - 1.0
    X, Y = np.meshgrid(xs, ys)
    R2 = X * X + Y * Y
    disk = R2 <= 1.0
    tile_normal = np.stack([X, Y, -np.sqrt(np.clip(1.0 - R2, 0.0, None))], axis=-1).astype(np.float32)
    normal = np.zeros((h, W, 3), dtype=np.float32)
    light = np.zeros((h, W, 3), dtype=np.float32)
    mask = np.zeros((h, W), dtype=bool)
    for k, deg in enumerate(angles):
        cols = slice((k * w) // 2, (k * w) // 2 + w)
        a = np.radians(deg)
        normal[:, cols][disk] = tile_normal[disk]
        light[:, cols][disk] = (-np.sin(a), 0.0, -np.cos(a))
        mask[:, cols][disk] = True
    return normal, light, mask


def visualize_bsdf(bsdf, increment_deg: float = 30, imsize=(512, 512), angle_start: float = 0, *, lookup: str = "nearest"):
    """utils/mitsuba3_utils.py:629-660: the BSDF (a PrincipledBSDF or a merl.MeasuredBSDF, read as ``lookup`` says) on the spheres of
    visualize_layout, seen along -z (wi = [0, 0, -1]).  Returns (fig [H, W, 3] float32, mask [H, W] bool)."""
    normal, light, mask = visualize_layout(increment_deg, imsize, angle_start)
    fig = np.zeros(normal.shape, dtype=np.float32)
    fig[mask] = eval_bsdf(bsdf, normal[mask], light[mask], (0.0, 0.0, -1.0), lookup=lookup)
    return fig, mask

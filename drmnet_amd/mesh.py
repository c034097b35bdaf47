"""Object images of triangle meshes -- the input side of the chain -- on csrc/mesh.hip (visibility) and csrc/render.hip (shading).

Operator surface of the reference's mesh helpers (utils/mitsuba3_utils.py): ``MeshRenderer`` stands in for ``MitsubaOrthoRenderer``
(:433-564), ``load_mesh`` keeps its name and its result (:690-699: a dict of ``vertex_positions`` [V, 3] float32, ``vertex_normals``
[V, 3] float32 and ``faces`` [F, 3] int32, here torch tensors on the host), ``normalize_mesh`` is the scaling of
scripts/preprocess_shape.py:40.  Every visible point is shaded as the reflectance-map renderer shades the sphere point with the same
normal: direct light from the environment map, no interreflection, black background.  Self-shadowing is opt-in
(``shadows=True``): shadow rays through a bounding-volume hierarchy built on the host (``build_bvh``; csrc/bvh.hip), also offered on their
own as ``occluded``.  One bounce of interreflection is opt-in on top of it (``bounces=1``): a lobe direction the mesh cuts off reads the
light its closest hit reflects back; the closest-hit query is offered on its own as ``closest_hit``.  Light sampling is opt-in too (``light_samples=M``: the light samples of ``render.render``, each traced like a lobe
direction under ``shadows``), for maps with a sun or a lamp a few texels wide.  ``render_mesh_measured`` renders the same mesh under measured
BRDFs (MERL tables, ``merl.MeasuredBSDF``) on csrc/mesh_table.hip, with or without ``shadows``; light samples and bounces under a table are not built.  Loading a mesh, building its BVH and constructing a renderer do not touch the GPU; rendering and ray queries run
there (no CPU path).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .render import QUAD, SUBPIXEL, _device, _env_and_view, canonical_rows, check_light_samples, view_rotation

Mesh = Dict[str, torch.Tensor]
_KEYS = ("vertex_positions", "vertex_normals", "faces")


def _as_mesh(positions, normals, faces) -> Mesh:
    return {"vertex_positions": torch.from_numpy(np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)),
            "vertex_normals": torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)),
            "faces": torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3))}


def area_weighted_normals(positions: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """Unit vertex normals [V, 3]: the sum over a vertex's faces of the face's cross product (e1 x e2: its normal times twice its area),
    normalised; a vertex no face uses gets (0, 0, 0).  float64 on the host."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.divide(n, length, out=np.zeros_like(n), where=length > 0)


def load_obj(path: Union[str, Path]) -> Mesh:
    """A Wavefront OBJ as the reference's mesh dict.  Reads ``v``, ``vn`` and ``f`` (corners written ``a``, ``a/b``, ``a//c`` or ``a/b/c``;
    negative indices count back from the last element read so far; polygons are fan-triangulated around their first corner); everything
    else (``vt``, groups, materials) is ignored.  A vertex is emitted per distinct (v, vn) pair, in order of first use, so a position used
    with two normals is split.  A file without ``vn`` gets area-weighted vertex normals computed here on the host
    (``area_weighted_normals``); a file that gives normals to only some corners is a ValueError."""
    v: List[List[float]] = []
    vn: List[List[float]] = []
    corners: Dict[Tuple[int, int], int] = {}
    faces: List[List[int]] = []
    with_normal = 0
    with open(path) as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                v.append([float(t) for t in tok[1:4]])
            elif tok[0] == "vn":
                vn.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                ids = []
                for c in tok[1:]:
                    part = c.split("/")
                    a = int(part[0])
                    a = a - 1 if a > 0 else len(v) + a
                    b = -1
                    if len(part) == 3 and part[2]:
                        b = int(part[2])
                        b = b - 1 if b > 0 else len(vn) + b
                        with_normal += 1
                        if not 0 <= b < len(vn):
                            raise ValueError(f"{path}: normal index {part[2]} out of range")
                    if not 0 <= a < len(v):
                        raise ValueError(f"{path}: vertex index {part[0]} out of range")
                    ids.append(corners.setdefault((a, b), len(corners)))
                if len(ids) < 3:
                    raise ValueError(f"{path}: a face needs at least three corners")
                faces += [[ids[0], ids[k], ids[k + 1]] for k in range(1, len(ids) - 1)]
    if not faces:
        raise ValueError(f"{path}: no faces")
    if len({b < 0 for _, b in corners}) > 1:
        raise ValueError(f"{path}: some face corners carry a normal index and some do not")
    pairs = sorted(corners, key=corners.get)
    positions = np.array([v[a] for a, _ in pairs], dtype=np.float64)
    f = np.array(faces, dtype=np.int32)
    normals = np.array([vn[b] for _, b in pairs], dtype=np.float64) if with_normal else area_weighted_normals(positions, f)
    return _as_mesh(positions, normals, f)


def normalize_mesh(obj: Mesh) -> Mesh:
    """scripts/preprocess_shape.py:40: the positions scaled by 0.9 / max |v|, so the mesh fits the film (x in [-1, 1]) from every view.
    Returns a new dict; normals and faces are shared."""
    p = obj["vertex_positions"].to(torch.float32)
    return {"vertex_positions": p * (0.9 / torch.linalg.vector_norm(p, dim=-1).max()), "vertex_normals": obj["vertex_normals"], "faces": obj["faces"]}


def load_mesh(path: Union[str, Path]) -> Mesh:
    """utils/mitsuba3_utils.py:690-699: ``.obj`` through ``load_obj``, or a ``.pt`` dict as scripts/preprocess_shape.py:48 writes it."""
    path = Path(path)
    if path.suffix == ".obj":
        return load_obj(path)
    if path.suffix == ".pt":
        blob = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(blob, dict) or any(k not in blob for k in _KEYS):
            raise ValueError(f"{path}: expected a dict with {_KEYS}")
        return _as_mesh(*(torch.as_tensor(blob[k]).detach().cpu().numpy() for k in _KEYS))
    raise ValueError(f"{path}: a mesh is an .obj file or a .pt dict (got {path.suffix!r})")


def _mesh_on(obj: Mesh, dev: torch.device):
    if not obj or any(k not in obj for k in _KEYS):
        raise ValueError(f"a mesh is a dict with {_KEYS}")
    pos = torch.as_tensor(obj["vertex_positions"]).to(dev, torch.float32).reshape(-1, 3).contiguous()
    nrm = torch.as_tensor(obj["vertex_normals"]).to(dev, torch.float32).reshape(-1, 3).contiguous()
    faces = torch.as_tensor(obj["faces"]).to(dev, torch.int32).reshape(-1, 3).contiguous()
    if nrm.shape[0] != pos.shape[0]:
        raise ValueError(f"vertex_normals has {nrm.shape[0]} rows, vertex_positions {pos.shape[0]}")
    return pos, nrm, faces


def build_bvh(obj: Mesh) -> torch.Tensor:
    """drm_mesh_bvh_build: the BVH of a mesh over its object-space positions, as a uint8 host tensor holding exactly the blob (header, nodes,
    face order; layout in include/drmnet_hip.h).  Host code only: needs no GPU.  The same mesh gives the same bytes."""
    pos = torch.as_tensor(obj["vertex_positions"]).detach().to("cpu", torch.float32).reshape(-1, 3).contiguous()
    faces = torch.as_tensor(obj["faces"]).detach().to("cpu", torch.int32).reshape(-1, 3).contiguous()
    lib = _lib.lib()
    V, F = int(pos.shape[0]), int(faces.shape[0])
    nbytes = int(lib.drm_mesh_bvh_bytes(F))
    if nbytes == 0 or V < 1:
        raise ValueError(f"build_bvh: F = {F} faces in [1, 2^24), V = {V} >= 1")
    buf = torch.zeros(nbytes, dtype=torch.uint8)
    _lib.check(lib.drm_mesh_bvh_build(pos.data_ptr(), faces.data_ptr(), V, F, buf.data_ptr(), nbytes))
    head = buf[:16].numpy().view(np.uint32)
    return buf[:BVH_HEADER_BYTES + BVH_NODE_BYTES * int(head[2]) + 4 * int(head[3])].clone()


BVH_MAGIC, BVH_HEADER_BYTES, BVH_NODE_BYTES = 0x31485642, 32, 32


def decode_bvh(blob) -> Dict[str, np.ndarray]:
    """A blob of ``build_bvh`` as numpy arrays, for tests and debugging: ``faces`` (the F it was built for), ``box_min`` / ``box_max``
    [nodes, 3] float32, ``skip`` [nodes] (the node to go to on a box miss or after a leaf), ``first`` / ``count`` [nodes] (count 0 = inner
    node, whose first child is the next node; a leaf holds ``order[first : first + count]``) and ``order`` (face indices).  Needs no GPU."""
    raw = np.ascontiguousarray(torch.as_tensor(blob).detach().cpu().numpy()).view(np.uint8).reshape(-1)
    if raw.size < BVH_HEADER_BYTES:
        raise ValueError("decode_bvh: shorter than the header")
    magic, F, nodes, norder = (int(v) for v in raw[:16].view(np.uint32))
    if magic != BVH_MAGIC or raw.size < BVH_HEADER_BYTES + BVH_NODE_BYTES * nodes + 4 * norder:
        raise ValueError("decode_bvh: not a build_bvh blob, or a truncated one")
    words = raw[BVH_HEADER_BYTES:BVH_HEADER_BYTES + BVH_NODE_BYTES * nodes].view(np.uint32).reshape(nodes, 8)
    order = raw[BVH_HEADER_BYTES + BVH_NODE_BYTES * nodes:][:4 * norder].view(np.int32).copy()
    return {"faces": F, "box_min": words[:, 0:3].copy().view(np.float32), "box_max": words[:, 3:6].copy().view(np.float32),
            "skip": words[:, 6].astype(np.int64), "first": (words[:, 7] >> 3).astype(np.int64), "count": (words[:, 7] & 7).astype(np.int64),
            "order": order}


def _bvh_on(blob, dev: torch.device) -> torch.Tensor:
    t = torch.as_tensor(blob)
    if t.dtype != torch.uint8 or t.dim() != 1:
        raise ValueError("a BVH is the uint8 tensor build_bvh returns")
    return t.to(dev).contiguous()


def _rays_on(who: str, obj: Mesh, origins, dirs, exclude, bvh):
    """what the ray queries share: (device, positions, faces, blob or None, origins, dirs, exclude or None, N), everything on the device"""
    for name, t in (("origins", origins), ("dirs", dirs)):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError(f"{who} runs on the GPU only (drmnet_amd has no CPU path): {name} is on {t.device}")
    dev = _device(origins, dirs)
    o = torch.as_tensor(origins).to(dev, torch.float32).reshape(-1, 3).contiguous()
    d = torch.as_tensor(dirs).to(dev, torch.float32).reshape(-1, 3).contiguous()
    if o.shape != d.shape:
        raise ValueError(f"origins {tuple(o.shape)} and dirs {tuple(d.shape)} must both be [N, 3]")
    N = int(o.shape[0])
    ex = None
    if exclude is not None:
        ex = torch.as_tensor(exclude).to(dev, torch.int32).reshape(-1).contiguous()
        if ex.shape[0] != N:
            raise ValueError(f"exclude must be [N={N}], got {tuple(ex.shape)}")
    pos, _, faces = _mesh_on(obj, dev)
    blob = None if bvh is None else _bvh_on(build_bvh(obj) if isinstance(bvh, str) and bvh == "auto" else bvh, dev)
    return dev, pos, faces, blob, o, d, ex, N


@torch.no_grad()
def occluded(obj: Mesh, origins, dirs, exclude=None, *, bvh="auto") -> torch.Tensor:
    """drm_mesh_occluded: for each of N rays (origins, dirs [N, 3] in object space; dirs of any length) whether some face other than
    ``exclude`` [N] (int32 face indices; None, or -1, for no exclusion) cuts it off -> bool [N] on the GPU.  The intersection rule is stated
    in include/drmnet_hip.h.  ``bvh``: "auto" builds the mesh's BVH, a ``build_bvh`` blob is used as it is, None tests every face for every
    ray (the same answers, slowly).  GPU only: an ``origins`` or ``dirs`` tensor on the CPU is a RuntimeError."""
    dev, pos, faces, blob, o, d, ex, N = _rays_on("occluded", obj, origins, dirs, exclude, bvh)
    out = torch.zeros(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_mesh_occluded(pos.data_ptr(), faces.data_ptr(), int(pos.shape[0]), int(faces.shape[0]), _lib.ptr(blob), o.data_ptr(),
                                                d.data_ptr(), _lib.ptr(ex), out.data_ptr(), N, _lib.stream_ptr(dev)))
    return out != 0


@torch.no_grad()
def closest_hit(obj: Mesh, origins, dirs, exclude=None, *, bvh="auto"):
    """drm_mesh_closest_hit: for each of N rays what is in the way, and where -> (face int32 [N], t, u, v float32 [N]) on the GPU.  ``face``
    is the face that ``occluded`` would call a hit and that is least under the order (t, face index), -1 where there is none (t = u = v = 0
    there); the hit point is origins + t * dirs (t in units of the length of ``dirs``), its barycentric weights (1 - u - v, u, v) on the face's
    three vertices.  The rule is stated in include/drmnet_hip.h.  Arguments and errors as for ``occluded``; with and without the BVH the
    answers are the same bits."""
    dev, pos, faces, blob, o, d, ex, N = _rays_on("closest_hit", obj, origins, dirs, exclude, bvh)
    face = torch.full((N,), -1, dtype=torch.int32, device=dev)
    tuv = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_mesh_closest_hit(pos.data_ptr(), faces.data_ptr(), int(pos.shape[0]), int(faces.shape[0]), _lib.ptr(blob), o.data_ptr(),
                                                   d.data_ptr(), _lib.ptr(ex), face.data_ptr(), tuv.data_ptr(), N, _lib.stream_ptr(dev)))
    return face, tuv[:, 0].contiguous(), tuv[:, 1].contiguous(), tuv[:, 2].contiguous()


def check_bounces(bounces, bounce_quad, shadows, light_samples) -> int:
    """the ``bounces`` / ``bounce_quad`` arguments of render_mesh and MeshRenderer -> bounces as an int; a ValueError names what is wrong"""
    if isinstance(bounces, bool) or not isinstance(bounces, (int, np.integer)) or int(bounces) not in (0, 1):
        raise ValueError(f"bounces must be 0 or 1 (one bounce of interreflection; later bounces are not modelled), got {bounces!r}")
    if int(bounces) == 1:
        if not shadows:
            raise ValueError("bounces=1 needs shadows=True: the bounce replaces what the shadow rays cut off")
        if int(light_samples) > 0:
            raise ValueError("bounces=1 is not combined with light_samples > 0: the bounce's inner sum has no light samples")
        if isinstance(bounce_quad, bool) or not isinstance(bounce_quad, (int, np.integer)) or not 1 <= int(bounce_quad) <= 16:
            raise ValueError(f"bounce_quad must be an integer in [1, 16], got {bounce_quad!r}")
    return int(bounces)


@torch.no_grad()
def render_mesh(obj: Mesh, z, brdf_param_names: Sequence[str], envmaps: Optional[torch.Tensor] = None, *, image_size, view_from=None,
                quad: int = QUAD, subpixel: int = SUBPIXEL, shadows: bool = False, bvh=None, light_samples: int = 0, bounces: int = 0,
                bounce_quad: int = 4):
    """One call of drm_render_mesh (``shadows=True``: with shadow rays, where parts of the mesh cut light off from other parts;
    ``bvh`` is then the mesh's ``build_bvh`` blob, built here when None): one mesh, lit and seen B ways.  z [B, P], envmaps [B, EH, EW, 3] (or None: white), view_from [B, 3] (or
    None: +z), image_size H or (H, W) -> (image [B, 3, H, W], normal [B, 3, H, W] in the view frame, depth [B, 1, H, W], alpha [B, H, W]).
    ``light_samples`` = M > 0 (a power of two in [64, 65536]) adds light samples: M directions drawn from each map's own
    light density join the two lobe quadratures by multiple importance sampling, as in ``render.render``, and with ``shadows`` every light
    sample is traced like a lobe direction, so the cast shadow of a sun is decided by the sun's own samples.  0, or no envmaps, is the
    render without them bit for bit.
    ``bounces`` = 1 (needs ``shadows``; not combined with ``light_samples``) adds one bounce: a lobe direction the
    mesh cuts off reads the radiance its closest hit reflects back under direct light, estimated with ``bounce_quad``^2 traced directions
    (1 <= bounce_quad <= 16); 0 makes exactly the launches above.  A bad combination is a ValueError before anything touches the GPU.
    GPU only: a ``z`` or ``envmaps`` tensor on the CPU, or a machine without a GPU, is a RuntimeError (the mesh itself and ``view_from`` are
    host data and are brought over)."""
    bounces = check_bounces(bounces, bounce_quad, shadows, light_samples)
    for name, t in (("z", z), ("envmaps", envmaps)):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError(f"render_mesh runs on the GPU only (drmnet_amd has no CPU path): {name} is on {t.device}")
    dev = _device(z, envmaps)
    z = torch.as_tensor(z).to(dev)
    if z.dim() != 2:
        raise ValueError(f"z must be [B, P], got {tuple(z.shape)}")
    B = int(z.shape[0])
    rows = canonical_rows(z, brdf_param_names).reshape(-1, 6).contiguous()
    env, view = _env_and_view(envmaps, view_from, B, dev)
    shading, _keep = _lib.make_shading(B, z=rows, env=env, view=view, quad=quad, light_samples=light_samples)
    return _render_call("drm_render_mesh", obj, shading, B, dev, image_size, subpixel, shadows, bvh, bounces=bounces,
                        bounce_quad=int(bounce_quad) if bounces else 0)


def _render_call(entry: str, obj: Mesh, shading, B: int, dev, image_size, subpixel: int, shadows: bool, bvh, **technique):
    """what the two mesh renders share once the shading is made: the mesh on the device, the workspace, the four outputs, the BVH under
    ``shadows`` and the call of ``entry`` -> (image, normal, depth, alpha)"""
    H, W = (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
    pos, nrm, faces = _mesh_on(obj, dev)
    lib = _lib.lib()
    V, F = int(pos.shape[0]), int(faces.shape[0])
    nbytes = int(lib.drm_render_mesh_workspace_bytes(F, B, H, W, int(subpixel)))
    if nbytes == 0 or V < 1:
        raise ValueError(f"{entry[4:]}: F = {F} faces in [1, 2^24), V = {V} >= 1, B = {B} in [1, 65535], image_size {(H, W)} in [1, 4096], "
                         f"subpixel = {subpixel} in [1, 4]")
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    normal = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    ws = torch.empty(((nbytes + 15) // 16, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        blob = _bvh_on(build_bvh(obj) if bvh is None else bvh, dev) if shadows else None
        m = _lib.sized(_lib.MeshRender, vertex_positions=pos.data_ptr(), vertex_normals=nrm.data_ptr(), faces=faces.data_ptr(), V=V, F=F, H=H, W=W,
                       subpixel=int(subpixel), image=image.data_ptr(), normal=normal.data_ptr(), depth=depth.data_ptr(), alpha=alpha.data_ptr(),
                       workspace=ws.data_ptr(), workspace_bytes=nbytes, shadows=int(blob is not None), bvh=_lib.ptr(blob),
                       bvh_bytes=0 if blob is None else int(blob.numel()), **technique)
        _lib.check(getattr(lib, entry)(shading, m, _lib.stream_ptr(dev)))
    return image, normal, depth, alpha


@torch.no_grad()
def render_mesh_measured(obj: Mesh, bsdfs, envmaps: Optional[torch.Tensor] = None, *, image_size, view_from=None, quad: int = QUAD,
                         subpixel: int = SUBPIXEL, shadows: bool = False, bvh=None, lookup: str = "linear"):
    """One call of drm_render_mesh_tables: ``render_mesh`` under measured BRDFs (MERL tables) instead of principled rows, with shadow rays
    under ``shadows=True`` (``bvh`` as in ``render_mesh``).  ``bsdfs`` follows ``relight.render_normals_measured``: one merl.MeasuredBSDF,
    shared by all rows, or a list of B (equal objects share one device table); B is the number of envmaps [B, EH, EW, 3], or of bsdfs under
    a white environment (None).  view_from [B, 3] (or None: +z); ``lookup`` is "linear" or "nearest" -> (image [B, 3, H, W], normal
    [B, 3, H, W] in the view frame, depth [B, 1, H, W], alpha [B, H, W]), what ``render_mesh`` returns.  Every hit is shaded as
    ``render.render_table`` shades the sphere point with the same normal.  There are no light samples and no bounces under a table.
    A bad argument is a ValueError before anything touches the GPU; an ``envmaps`` tensor on the CPU, or a machine without a GPU, is a
    RuntimeError."""
    from .merl import MeasuredBSDF, device_tables, lookup_mode

    linear = lookup_mode(lookup)
    if isinstance(envmaps, torch.Tensor):
        if envmaps.dim() != 4 or envmaps.shape[3] != 3:
            raise ValueError(f"envmaps must be [B, H, W, 3], got {tuple(envmaps.shape)}")
        if not envmaps.is_cuda:
            raise RuntimeError(f"render_mesh_measured runs on the GPU only (drmnet_amd has no CPU path): envmaps is on {envmaps.device}")
        B = int(envmaps.shape[0])
    else:
        B = 1 if isinstance(bsdfs, MeasuredBSDF) else len(list(bsdfs))
    if not 1 <= B <= 65535:
        raise ValueError(f"render_mesh_measured: B = {B} rows in [1, 65535]")
    if isinstance(quad, bool) or not 1 <= int(quad) <= 1024:
        raise ValueError(f"render_mesh_measured: quad in [1, 1024], got {quad!r}")
    if view_from is not None and view_rotation(view_from).shape[0] != B:
        raise ValueError(f"view_from must be [B={B}, 3], got {tuple(torch.as_tensor(view_from).shape)}")
    dev = _device(envmaps)
    tables, table_of, alpha = device_tables(bsdfs, B, dev)
    env, view = _env_and_view(envmaps, view_from, B, dev)
    shading, _keep = _lib.make_shading(B, tables=(tables, table_of, alpha, linear), env=env, view=view, quad=quad)
    return _render_call("drm_render_mesh_tables", obj, shading, B, dev, image_size, subpixel, shadows, bvh)


class MeshRenderer:
    """MitsubaOrthoRenderer (utils/mitsuba3_utils.py:433-564) on drm_render_mesh: an orthographic view of a smooth-shaded triangle mesh under
    the scene's environment map.  Differences from Mitsuba's ``path`` integrator, all by design: direct light only, no
    interreflection, a black background, and self-shadowing only with ``shadows=True`` (the BVH is built once when a mesh becomes the
    scene's and kept with it; a ``new_scene`` mesh gets one for that call).  The integral is the deterministic quadrature of the reflectance-map
    renderer, so ``spp`` and ``denoise`` are accepted and ignored.  ``light_samples`` = M > 0 adds M light samples per map (see
    ``render_mesh``; reachable from a YAML ``params:``); the default 0 renders without them.  ``bounces`` = 1 with ``shadows`` adds one
    bounce of interreflection (``bounce_quad``^2 directions per bounce; see ``render_mesh``; also reachable from ``params:``), checked here.  ``init_view_from`` may be any position off the +-y axis.  The scene
    state -- environment map, view and mesh -- is kept across ``rendering`` calls as the reference's scene keeps it.  Construction does not
    touch the GPU."""

    def __init__(self, image_size, spp: int = 1024, envmap_size=(1000, 2000), denoise: Optional[str] = None, return_normal: bool = False,
                 return_depth: bool = False, init_view_from=(0, 0, 1.1), brdf_param_names: Optional[List[str]] = None, *, quad: int = QUAD,
                 subpixel: int = SUBPIXEL, shadows: bool = False, light_samples: int = 0, bounces: int = 0, bounce_quad: int = 4):
        self.shadows = bool(shadows)
        self.bounces = check_bounces(bounces, bounce_quad, self.shadows, int(light_samples))
        self.bounce_quad = int(bounce_quad)
        self.light_samples = check_light_samples(light_samples)
        self.image_size = (int(image_size), int(image_size)) if isinstance(image_size, int) else tuple(int(s) for s in image_size)
        self.envmap_size = tuple(int(s) for s in envmap_size)
        self.spp, self.denoise = spp, denoise
        self.return_normal, self.return_depth = bool(return_normal), bool(return_depth)
        self.brdf_param_names = brdf_param_names
        self.quad, self.subpixel = int(quad), int(subpixel)
        self._view_from = torch.as_tensor(init_view_from).detach().to("cpu", torch.float32).reshape(3)
        view_rotation(self._view_from)  # (a view along +-y is a ValueError here, not at the first render)
        self._envmap: Optional[torch.Tensor] = None  # the scene's map; None = the initial all-zero bitmap of envmap_size
        self._obj: Optional[Mesh] = None  # the scene's mesh; None = none given yet
        self._bvh: Optional[torch.Tensor] = None  # shadows: the BVH of the scene's mesh, on its device

    def rendering(self, z, brdf_param_names, envmap: Optional[torch.Tensor] = None, view_from=None, obj: Mesh = {}, sensor=0, spp: int = 0,
                  new_scene: bool = False, channel_first: bool = False):
        """utils/mitsuba3_utils.py:543-564: the object image [H, W, 3] ([3, H, W] with channel_first), or the list [image, normal [H, W, 3],
        depth [H, W, 1]] restricted to what ``return_normal`` / ``return_depth`` ask for.  ``envmap`` [EH, EW, 3], ``view_from`` [3] and
        ``obj`` (a mesh dict; {} = none) replace the scene's and stay with it for later calls; with ``new_scene`` they hold for this call
        only (and an envmap is required).  No mesh given and none kept is a ValueError."""
        if not (isinstance(sensor, int) and sensor == 0):
            raise NotImplementedError("only the scene's own sensor (sensor=0) is modelled")
        if envmap is not None:
            assert isinstance(envmap, torch.Tensor) and envmap.dim() == 3 and not torch.isnan(envmap[0, 0, 0]), f"envmap [{envmap.shape}]"
        mesh = obj if obj else self._obj
        if not mesh:
            raise ValueError("no mesh: pass obj = {vertex_positions, vertex_normals, faces} (the scene keeps it for later calls)")
        dev = _device(z, envmap)
        bvh = None  # (a new_scene mesh: render_mesh builds one for this call)
        if new_scene:
            if envmap is None:
                raise ValueError("new_scene needs an envmap")
            env = envmap.to(dev)
            view = self._view_from if view_from is None else view_from
            if not obj:
                bvh = self._bvh
        else:
            if obj:
                self._obj = dict(zip(_KEYS, _mesh_on(obj, dev)))
                mesh = self._obj
                self._bvh = _bvh_on(build_bvh(obj), dev) if self.shadows else None
            bvh = self._bvh
            if envmap is not None:
                self._envmap = envmap.to(dev)
            if self._envmap is None:
                self._envmap = torch.zeros(*self.envmap_size, 3, device=dev)
            env = self._envmap
            if view_from is not None:
                self._view_from = torch.as_tensor(view_from).detach().to("cpu", torch.float32).reshape(3)
            view = self._view_from
        z = torch.as_tensor(z).reshape(1, -1).to(dev)
        image, normal, depth, _ = render_mesh(mesh, z, brdf_param_names or self.brdf_param_names, env[None], image_size=self.image_size,
                                              view_from=torch.as_tensor(view).reshape(1, 3), quad=self.quad, subpixel=self.subpixel,
                                              shadows=self.shadows, bvh=bvh, light_samples=self.light_samples, bounces=self.bounces,
                                              bounce_quad=self.bounce_quad)
        outs = [image[0]] + ([normal[0]] if self.return_normal else []) + ([depth[0]] if self.return_depth else [])
        if not channel_first:
            outs = [o.permute(1, 2, 0) for o in outs]
        return outs[0] if len(outs) == 1 else outs

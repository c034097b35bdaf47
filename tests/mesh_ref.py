"""float64 numpy restatement of the mesh object-image renderer (drm_render_mesh: drmnet_amd/csrc/mesh.hip + mesh_shade_kernel in render.hip),
written from the conventions in include/drmnet_hip.h: brute force over faces, nothing tiled, nothing culled.  Shading goes through
render_ref._quadrature, the restatement of the sphere's per-normal sum.  Used by tests/test_mesh_cpu.py and tests/test_gpu_mesh.py; nothing
here touches a GPU.

A mesh is (positions [V, 3], normals [V, 3], faces [F, 3]); Rot is the row-major view rotation [3, 3] (columns right, up, back) or None."""
import numpy as np

import render_ref as rr

GUARD = 1e-4  # view units: see `unsafe` in visibility()


def look_at(view_from):
    """the rotation render.view_rotation builds, in float64"""
    v = np.asarray(view_from, dtype=np.float64)
    back = v / np.linalg.norm(v)
    right = np.array([back[2], 0.0, -back[0]])
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.stack([right, up, back], axis=-1)


def film_samples(H, W, S):
    """x [W S] and y [H S] of the film's sample columns and rows"""
    x = (2.0 * np.arange(W * S) + 1.0) / (W * S) - 1.0
    y = (H / W) * (1.0 - (2.0 * np.arange(H * S) + 1.0) / (H * S))
    return x, y


def icosphere(subdiv):
    """(positions, normals, faces) of an icosahedron subdivided `subdiv` times onto the sphere of radius 0.9: 20 4^subdiv faces, vertex
    normal = vertex direction"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        g = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    d = np.array(v)
    return 0.9 * d, d.copy(), np.array(f, dtype=np.int32)


def visibility(positions, faces, Rot, H, W, S, guard=GUARD):
    """Which face each film sample sees.  Returns a dict of [H S, W S] arrays: face (int, -1 for a miss), u, v (the point is
    (1 - u - v) p0 + u p1 + v p2), z (view space, 0 for a miss), gap (z minus the next covering depth; inf where there is none) and unsafe.

    Coverage: the three edge functions times the sign of the face's screen area are >= 0.  Ties: larger z, then the lower face index.
    Skipped: faces of zero screen area and faces with a vertex index outside [0, V).
    unsafe: with g = `guard`, some (not skipped) face has |min of its three length-normalised oriented edge functions| < g at the sample,
    or the two nearest covering depths are closer than g.  Only there may a float32 evaluation see another face: float32 rounding of a
    rotated vertex is about 1e-6, so g = 1e-4 carries a x100 margin."""
    p = np.asarray(positions, dtype=np.float64)
    if Rot is not None:
        p = p @ np.asarray(Rot, dtype=np.float64)  # rows Rot^T p
    V = len(p)
    xs, ys = film_samples(H, W, S)
    X, Y = np.meshgrid(xs, ys)
    face = np.full(X.shape, -1, dtype=np.int64)
    bu, bv = np.zeros(X.shape), np.zeros(X.shape)
    z1, z2 = np.full(X.shape, -np.inf), np.full(X.shape, -np.inf)
    unsafe = np.zeros(X.shape, dtype=bool)
    for f, idx in enumerate(np.asarray(faces).reshape(-1, 3)):
        if np.any(idx < 0) or np.any(idx >= V):
            continue
        (x0, y0, d0), (x1, y1, d1), (x2, y2, d2) = p[idx[0]], p[idx[1]], p[idx[2]]
        area2 = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        if area2 == 0.0:
            continue
        sg = 1.0 if area2 > 0 else -1.0
        e0 = ((x2 - x1) * (Y - y1) - (y2 - y1) * (X - x1)) * sg
        e1 = ((x0 - x2) * (Y - y2) - (y0 - y2) * (X - x2)) * sg
        e2 = ((x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0)) * sg
        lens = [np.hypot(x2 - x1, y2 - y1), np.hypot(x0 - x2, y0 - y2), np.hypot(x1 - x0, y1 - y0)]
        with np.errstate(divide="ignore", invalid="ignore"):
            nearest = np.minimum(np.minimum(e0 / lens[0], e1 / lens[1]), e2 / lens[2])
        unsafe |= ~(np.abs(nearest) >= guard)
        cover = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        u, v = e1 / abs(area2), e2 / abs(area2)
        z = d0 + u * (d1 - d0) + v * (d2 - d0)
        win = cover & ((z > z1) | ((z == z1) & (f < face)))
        z2 = np.where(win, z1, np.where(cover, np.maximum(z2, z), z2))
        z1 = np.where(win, z, z1)
        face = np.where(win, f, face)
        bu, bv = np.where(win, u, bu), np.where(win, v, bv)
    with np.errstate(invalid="ignore"):
        gap = np.where(face >= 0, z1 - z2, np.inf)
    unsafe |= gap < guard
    return {"face": face, "u": bu, "v": bv, "z": np.where(face >= 0, z1, 0.0), "gap": gap, "unsafe": unsafe}


def shading_normals(vis, normals, faces, Rot):
    """[H S, W S, 3] unit shading normals in the view frame: the barycentric mix of the view-frame vertex normals, normalised; zero for a
    miss and for a zero mix"""
    n = np.asarray(normals, dtype=np.float64)
    if Rot is not None:
        n = n @ np.asarray(Rot, dtype=np.float64)
    hit = vis["face"] >= 0
    idx = np.asarray(faces).reshape(-1, 3)[np.where(hit, vis["face"], 0)]
    idx = np.where(hit[..., None], idx, 0)
    u, v = vis["u"][..., None], vis["v"][..., None]
    mix = (1.0 - u - v) * n[idx[..., 0]] + u * n[idx[..., 1]] + v * n[idx[..., 2]]
    length = np.linalg.norm(mix, axis=-1, keepdims=True)
    unit = np.divide(mix, length, out=np.zeros_like(mix), where=length > 0)
    return np.where(hit[..., None], unit, 0.0)


def sample_radiance(z, env, n, Q, Rot=None, chunk=2048):
    """[..., 3] radiance toward +z of surface points with unit normals n [..., 3]; zero where n.z <= 0"""
    n = np.asarray(n, dtype=np.float64)
    flat = n.reshape(-1, 3)
    out = np.zeros_like(flat)
    lit = np.nonzero(flat[:, 2] > 0)[0]
    for k in range(0, len(lit), chunk):
        sel = lit[k:k + chunk]
        out[sel] = rr._quadrature(z, env, flat[sel].reshape(-1, 1, 1, 3), Q, Rot)[:, :, 0].T
    return out.reshape(n.shape)


def render(positions, normals, faces, z, env, Rot, H, W, S, Q, guard=GUARD):
    """drm_render_mesh for one row.  Returns the per-sample dict of visibility() with `normal` [H S, W S, 3] added, and the pixel outputs
    image [3, H, W], normal_mean [3, H, W], depth [1, H, W], alpha [H, W] and unsafe_pixel [H, W] (some sample of the pixel is unsafe)."""
    vis = visibility(positions, faces, Rot, H, W, S, guard)
    n = shading_normals(vis, normals, faces, Rot)
    hit = vis["face"] >= 0
    rad = sample_radiance(z, env, n, Q, Rot)

    def pixels(a):  # [H S, W S, ...] -> mean over the S x S samples of every pixel
        return a.reshape((H, S, W, S) + a.shape[2:]).mean(axis=(1, 3))

    count = pixels(hit.astype(np.float64)) * (S * S)
    dsum = pixels(np.where(hit, 1.1 - vis["z"], 0.0)) * (S * S)
    out = dict(vis)
    out.update(normal=n, radiance=rad, image=pixels(rad).transpose(2, 0, 1), normal_mean=pixels(n).transpose(2, 0, 1),
               depth=np.divide(dsum, count, out=np.zeros_like(dsum), where=count > 0)[None], alpha=count / (S * S),
               unsafe_pixel=pixels(vis["unsafe"].astype(np.float64)) > 0)
    return out

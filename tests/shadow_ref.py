"""float64 numpy restatement of the shadow rays of the mesh object-image renderer (drm_mesh_occluded, drm_render_mesh with shadows: csrc/bvh.h,
csrc/bvh.hip and mesh_shade_kernel<VIEW, true> in csrc/render.hip), written from the rule in include/drmnet_hip.h: brute force over faces, no
BVH.  Used by tests/test_shadow_cpu.py and tests/test_gpu_shadow.py; nothing here touches a GPU.

The rule.  A ray (o, d) in object space, d of any length, is occluded iff some face g != exclude with its three vertex indices in [0, V) has,
with e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1.pv, tv = o - p0, qv = tv x e1, U = tv.pv, V = d.qv, T = e2.qv, s = sign(det):
det != 0 and finite, s U >= 0, s V >= 0, s (U + V) <= |det|, s T > 0.

Marginal rays.  With g = mesh_ref.GUARD = 1e-4 view units a ray is marginal if for some non-skipped face other than the excluded one the plane
crossing lies within g of an edge (|min(u, v, 1 - u - v)| times the face's smallest height) and t > -g, or the crossing is inside the face
and |t| < g, or |det| < 1e-9 (t in units of length: t |d|).  Only there may a float32 evaluation decide otherwise than float64: the float32
rounding of a rotated hit point is about 1e-7."""
import numpy as np

import mesh_ref as mr
import render_ref as rr

GUARD = mr.GUARD
DET_GUARD = 1e-9


def two_spheres():
    """the shading scene: a body, icosphere(2) of radius 0.55 at the origin (faces 0 .. 319), and a ball, icosphere(1) of radius 0.22 at
    (0.40, 0.35, 0.30) (faces 320 .. 399): 400 faces within radius 0.9"""
    _, d2, f2 = mr.icosphere(2)
    _, d1, f1 = mr.icosphere(1)
    p = np.concatenate([0.55 * d2, 0.22 * d1 + np.array([0.40, 0.35, 0.30])])
    return p, np.concatenate([d2, d1]), np.concatenate([f2, f1 + len(d2)]).astype(np.int32)


def soup(F=2000, seed=7):
    """a seeded soup of F random triangles in the cube of side 1.8, with faces the builder must leave out: repeated vertices, collinear
    vertices, vertex indices -1 and V, a vertex at infinity and a NaN vertex.  Returns (positions, faces, left_out [F] bool)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.8, 0.8, (F, 1, 3))
    p = (centre + rng.uniform(-0.1, 0.1, (F, 3, 3))).reshape(-1, 3).astype(np.float32).astype(np.float64)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    V = len(p)
    bad = np.zeros(F, dtype=bool)
    f[10] = (30, 30, 31)                  # a repeated vertex
    f[11] = (33, 34, 33)
    p[36:39] = np.array([(0.25, 0.5, -0.125), (0.5, 0.5, -0.125), (0.375, 0.5, -0.125)])  # collinear (exactly, in float32)
    f[13] = (-1, 39, 40)
    f[14] = (42, V, 43)
    p[45] = (np.inf, 0.0, 0.0)
    p[49] = (0.0, np.nan, 0.0)
    bad[[10, 11, 12, 13, 14, 15, 16]] = True
    return p, f, bad


def occluded(positions, faces, origins, dirs, exclude=None, chunk=None, marginal=False):
    """the rule for N rays -> hit [N] bool (and, with `marginal`, the marginal mask [N])"""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    N, F, V = len(o), len(f), len(p)
    ex = np.full(N, -1, dtype=np.int64) if exclude is None else np.asarray(exclude, dtype=np.int64).reshape(-1)
    valid = np.all((f >= 0) & (f < V), axis=1)
    fs = np.where(valid[:, None], f, 0)
    p0, p1, p2 = p[fs[:, 0]], p[fs[:, 1]], p[fs[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        # the smallest height of every face: twice its area over its longest edge
        area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
        longest = np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(p2 - p1, axis=1))
        height = np.where(longest > 0, area2 / longest, 0.0)
        skipped = ~valid | ~np.isfinite(area2) | (area2 == 0)
    hit = np.zeros(N, dtype=bool)
    marg = np.zeros(N, dtype=bool)
    chunk = chunk or max(64, 800000 // F)
    ids = np.arange(F)
    for k in range(0, N, chunk):
        oc, dc = o[k:k + chunk, None, :], d[k:k + chunk, None, :]
        with np.errstate(all="ignore"):
            pv = np.cross(dc, e2[None])
            det = np.sum(e1[None] * pv, axis=-1)
            tv = oc - p0[None]
            qv = np.cross(tv, e1[None])
            U, Vb, T = np.sum(tv * pv, axis=-1), np.sum(dc * qv, axis=-1), np.sum(e2[None] * qv, axis=-1)
            s = np.where(det > 0, 1.0, -1.0)
            other = valid[None] & (ids[None] != ex[k:k + chunk, None])
            yes = other & (det != 0) & np.isfinite(det) & (s * U >= 0) & (s * Vb >= 0) & (s * (U + Vb) <= np.abs(det)) & (s * T > 0)
            hit[k:k + chunk] = yes.any(axis=1)
            if marginal:
                u, v, t = U / det, Vb / det, T / det * np.linalg.norm(dc, axis=-1)
                inner = np.minimum(np.minimum(u, v), 1.0 - u - v)
                near_edge = (np.abs(inner) * height[None] < GUARD) & (t > -GUARD)
                near_origin = (inner >= 0) & (np.abs(t) < GUARD)
                m = other & ~skipped[None] & (near_edge | near_origin | ~(np.abs(det) >= DET_GUARD))
                marg[k:k + chunk] = m.any(axis=1)
    return (hit, marg) if marginal else hit


def trace(positions, normals, faces, z, Rot, H, W, S, Q, shadows=True, guard=GUARD):
    """Everything of one row that does not depend on the environment: mesh_ref's visibility and shading normals, and for the M lit samples
    (a hit with n.z > 0) the lobe directions with their weights, visibility (`open_*`: 1 where the ray is not occluded) and marginal masks.
    The ray of a direction l starts at the sample's view-space hit point (x, y, z_hit) taken to object space with Rot, runs along Rot l and
    excludes the hit face."""
    vis = mr.visibility(positions, faces, Rot, H, W, S, guard)
    n = mr.shading_normals(vis, normals, faces, Rot)
    xs, ys = mr.film_samples(H, W, S)
    X, Y = np.meshgrid(xs, ys)
    lit = (vis["face"] >= 0) & (n[..., 2] > 0)
    R = np.eye(3) if Rot is None else np.asarray(Rot, dtype=np.float64)
    origin = np.stack([X[lit], Y[lit], vis["z"][lit]], axis=-1) @ R.T
    face = vis["face"][lit]
    spec, diff = rr.lobes(z, n[lit], Q)
    M, QQ = spec.ok.shape
    out = dict(vis=vis, normal=n, lit=lit, origin=origin, face=face, Rot=Rot, shape=(H, W, S, Q), traced_spec=spec.ok, traced=0, marginal=0,
               occluded=0)
    for name, lobe in (("spec", spec), ("diff", diff)):
        out["l_" + name], out["w_" + name] = (None, None) if lobe is None else (lobe.l, lobe.w)
        if lobe is None:
            continue
        if shadows:
            hit, marg = occluded(positions, faces, np.repeat(origin, QQ, axis=0), (lobe.l @ R.T).reshape(-1, 3), np.repeat(face, QQ), marginal=True)
            hit, marg = hit.reshape(M, QQ), marg.reshape(M, QQ)
        else:
            hit, marg = np.zeros((M, QQ), dtype=bool), np.zeros((M, QQ), dtype=bool)
        hit, marg = hit & lobe.ok, marg & lobe.ok  # (only directions with a non-zero weight are traced: every diffuse one)
        out["open_" + name], out["marginal_" + name] = ~hit, marg
        out["traced"] += int(lobe.ok.sum())
        out["marginal"] += int(marg.sum())
        out["occluded"] += int(hit.sum())
    return out


def shade(tr, env):
    """The row's pixels under env [EH, EW, 3] (None: white) -> dict of image [3, H, W], slack [3, H, W] (the sum of the absolute contributions
    of the pixel's marginal rays) and unsafe_pixel [H, W] (mesh_ref's: some sample of the pixel is within the guard of an edge or a depth tie)."""
    H, W, S, Q = tr["shape"]
    look = (lambda l: np.ones(l.shape)) if env is None else (lambda l: rr.env_lookup(env, l, tr["Rot"]))
    M = len(tr["face"])
    rad, slack = np.zeros((M, 3)), np.zeros((M, 3))
    for name in ("spec", "diff"):
        if tr["l_" + name] is None:
            continue
        term = tr["w_" + name] * look(tr["l_" + name])
        rad += (term * tr["open_" + name][..., None]).sum(axis=1)
        slack += (np.abs(term) * tr["marginal_" + name][..., None]).sum(axis=1)
    full_r, full_s = np.zeros((H * S, W * S, 3)), np.zeros((H * S, W * S, 3))
    full_r[tr["lit"]], full_s[tr["lit"]] = rad / (Q * Q), slack / (Q * Q)

    def pixels(a):
        return a.reshape(H, S, W, S, -1).mean(axis=(1, 3)).transpose(2, 0, 1)

    return {"image": pixels(full_r), "slack": pixels(full_s), "unsafe_pixel": pixels(tr["vis"]["unsafe"].astype(np.float64)[..., None])[0] > 0}


def render(positions, normals, faces, z, env, Rot, H, W, S, Q, shadows=True):
    """drm_render_mesh with shadows (or, shadows=False, drm_render_mesh) for one row: shade(trace(...)) with the trace added under "trace" """
    tr = trace(positions, normals, faces, z, Rot, H, W, S, Q, shadows)
    out = shade(tr, env)
    out["trace"] = tr
    return out

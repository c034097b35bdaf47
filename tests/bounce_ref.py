"""float64 numpy restatement of the closest-hit query and of the one-bounce render of the mesh object images (drm_mesh_closest_hit,
drm_render_mesh with bounces = 1: csrc/bvh.h, csrc/bvh.hip and mesh_shade_kernel<VIEW, true, false, true> in csrc/render.hip), written from the contract in
include/drmnet_hip.h on top of tests/shadow_ref.py: brute force over faces, no BVH.  Used by tests/test_bounce_cpu.py and
tests/test_gpu_bounce.py; nothing here touches a GPU.

The closest hit.  A face is a candidate of (o, d, exclude) iff shadow_ref's rule accepts it (a face of zero area is none).  A candidate has
t = T / det, u = U / det, v = V / det; the hit is the candidate least under the order (t, g) with t rounded to float32 first (float64 ->
float32 of a quotient of two float32-exact values is the correctly rounded float32 quotient); no candidate: face -1.

Marginal rays.  shadow_ref's conditions (a plane crossing within GUARD of an edge or of the origin, |det| < 1e-9), or a second candidate whose
t |d| lies within GUARD of the closest one's: only there may a float32 evaluation name another face than float64 does.

The bounce.  A lobe direction w of a hit sample (origin o, hit face g) whose ray is occluded reads, instead of the map,
L_b = (pi / K) sum_k V_k L(w_k) E(n_y, w_o, w_k) / cos_k: y = o + t w the closest hit on face g', n_y the normalised barycentric mix of the
vertex normals of g' (zero: L_b = 0), w_o = -w / |w| (n_y.w_o <= 0: L_b = 0), w_k the K = bounce_quad^2 cosine-weighted directions of the
midpoint grid about n_y in the frame of Duff et al. with the sign term, E = render_ref.eval_bsdf (value times cosine), V_k = 0 iff the ray
(y, w_k) excluding g' is occluded, L the map's bilinear radiance along w_k (an object-space direction is the world direction), 1 under a
white environment.  The slack of a pixel is shadow_ref's, plus |w L_b| of the bounced rays whose closest hit is marginal, plus
w sum |inner term| over the marginal inner rays."""
import numpy as np

import render_ref as rr
import shadow_ref as sr

GUARD = sr.GUARD
PI = np.pi


def closest(positions, faces, origins, dirs, exclude=None, chunk=None, marginal=False):
    """the closest hit of N rays -> (face [N] int64, -1 for none, t, u, v [N] float64: the unrounded quotients, 0 where there is no hit) and,
    with `marginal`, the marginal mask [N]"""
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
        area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
        longest = np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(p2 - p1, axis=1))
        height = np.where(longest > 0, area2 / longest, 0.0)
        skipped = ~valid | ~np.isfinite(area2) | (area2 == 0)
    face = np.full(N, -1, dtype=np.int64)
    tuv = np.zeros((N, 3))
    marg = np.zeros(N, dtype=bool)
    chunk = chunk or max(64, 400000 // F)
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
            yes = (other & ~skipped[None] & (det != 0) & np.isfinite(det) & (s * U >= 0) & (s * Vb >= 0) & (s * (U + Vb) <= np.abs(det))
                   & (s * T > 0))
            t, u, v = T / det, U / det, Vb / det
            key = np.where(yes, t.astype(np.float32).astype(np.float64), np.inf)
            best = key.min(axis=1)
            g = np.argmax(yes & (key == best[:, None]), axis=1)  # the lowest index among the candidates at the least t
            hit = yes.any(axis=1)
            rows = np.arange(len(g))
            face[k:k + chunk] = np.where(hit, g, -1)
            for c, a in enumerate((t, u, v)):
                tuv[k:k + chunk, c] = np.where(hit, a[rows, g], 0.0)
            if marginal:
                length = np.linalg.norm(dc, axis=-1)
                inner = np.minimum(np.minimum(u, v), 1.0 - u - v)
                near_edge = (np.abs(inner) * height[None] < GUARD) & (t * length > -GUARD)
                near_origin = (inner >= 0) & (np.abs(t * length) < GUARD)
                m = (other & ~skipped[None] & (near_edge | near_origin | ~(np.abs(det) >= sr.DET_GUARD))).any(axis=1)
                rest = np.where(yes, t * length, np.inf)
                rest[rows, g] = np.inf
                close = hit & (rest.min(axis=1) - tuv[k:k + chunk, 0] * length[:, 0] < GUARD)
                marg[k:k + chunk] = m | close
    out = (face, tuv[:, 0], tuv[:, 1], tuv[:, 2])
    return out + (marg,) if marginal else out


def frame(n):
    """(t, bt) about unit normals n [..., 3]: Duff et al. 2017 with the sign term"""
    s = np.where(n[..., 2] >= 0, 1.0, -1.0)
    a = -1.0 / (s + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    return (np.stack([1 + s * n[..., 0] ** 2 * a, s * b, -s * n[..., 0]], axis=-1),
            np.stack([b, s + n[..., 1] ** 2 * a, -n[..., 1]], axis=-1))


def bounce_terms(positions, normals, faces, z, origins, dirs, exclude, bq):
    """For N occluded rays: everything of L_b that does not depend on the environment -> dict of w [N, K, 3] the directions w_k, coef [N, K, 3]
    = (pi / K) E / cos_k (0 where L_b = 0 by rule), open [N, K] (V_k), marginal_inner [N, K], marginal_hit [N], face [N]."""
    p = np.asarray(positions, dtype=np.float64)
    vn = np.asarray(normals, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    N, K = len(o), bq * bq
    g, t, u, v, marg = closest(p, f, o, d, exclude, marginal=True)
    assert np.all(g >= 0), "bounce_terms is asked about occluded rays only"
    y = o + t[:, None] * d
    tri = vn[f[g]]
    n = (1 - u - v)[:, None] * tri[:, 0] + u[:, None] * tri[:, 1] + v[:, None] * tri[:, 2]
    length = np.linalg.norm(n, axis=1)
    alive = length > 0
    n = np.where(alive[:, None], n / np.where(alive, length, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
    alive &= np.sum(n * wo, axis=1) > 0
    tt, bt = frame(n)
    grid = (np.arange(bq) + 0.5) / bq
    U1, U2 = (a.reshape(-1) for a in np.meshgrid(grid, grid, indexing="ij"))
    rs, ck = np.sqrt(U1), np.sqrt(1 - U1)
    w = ck[None, :, None] * n[:, None] + (rs * np.cos(2 * PI * U2))[None, :, None] * tt[:, None] + (rs * np.sin(2 * PI * U2))[None, :, None] * bt[:, None]
    E = rr.eval_bsdf(z, n[:, None], wo[:, None], w)
    coef = (PI / K) * E / ck[None, :, None] * alive[:, None, None]
    live = np.any(coef != 0, axis=-1)  # (a direction with E = 0 is not traced)
    hit, im = sr.occluded(p, f, np.repeat(y, K, axis=0), w.reshape(-1, 3), np.repeat(g, K), marginal=True)
    return dict(w=w, coef=coef, open=~hit.reshape(N, K) & live, marginal_inner=im.reshape(N, K) & live, marginal_hit=marg, face=g, normal=n, alive=alive)


def trace(positions, normals, faces, z, Rot, H, W, S, Q, bq, shadow_trace=None):
    """shadow_ref.trace (`shadow_trace`: one computed before for the same arguments; it is not changed) with, per lobe, the bounce of every
    occluded direction under "bounce_spec" / "bounce_diff" (bounce_terms plus `at`, the (sample, grid point) indices of the bounced rays), and
    the counts inner_traced, inner_occluded, inner_marginal, hit_marginal, bounced."""
    tr = dict(sr.trace(positions, normals, faces, z, Rot, H, W, S, Q) if shadow_trace is None else shadow_trace)
    R = np.eye(3) if Rot is None else np.asarray(Rot, dtype=np.float64)
    tr.update(bq=bq, bounced=0, inner_traced=0, inner_occluded=0, inner_marginal=0, hit_marginal=0)
    for name in ("spec", "diff"):
        tr["bounce_" + name] = None
        if tr["l_" + name] is None:
            continue
        at = np.nonzero(~tr["open_" + name])
        b = bounce_terms(positions, normals, faces, z, tr["origin"][at[0]], tr["l_" + name][at] @ R.T, tr["face"][at[0]], bq)
        b["at"] = at
        tr["bounce_" + name] = b
        traced = np.any(b["coef"] != 0, axis=-1)
        tr["bounced"] += len(at[0])
        tr["inner_traced"] += int(traced.sum())
        tr["inner_occluded"] += int((traced & ~b["open"]).sum())
        tr["inner_marginal"] += int(b["marginal_inner"].sum())
        tr["hit_marginal"] += int(b["marginal_hit"].sum())
    return tr


def shade(tr, env):
    """shadow_ref.shade of the trace with the bounce added: image, slack [3, H, W], unsafe_pixel [H, W], and "shadowed", the image without it"""
    H, W, S, Q = tr["shape"]
    out = sr.shade(tr, env)
    M = len(tr["face"])
    rad, slack = np.zeros((M, 3)), np.zeros((M, 3))
    for name in ("spec", "diff"):
        b = tr["bounce_" + name]
        if b is None or not len(b["at"][0]):
            continue
        term = b["coef"] * (1.0 if env is None else rr.env_lookup(env, b["w"]))  # [N, K, 3]
        Lb = (term * b["open"][..., None]).sum(axis=1)
        wgt = tr["w_" + name][b["at"]]  # [N, 3]
        np.add.at(rad, b["at"][0], wgt * Lb)
        np.add.at(slack, b["at"][0], np.abs(wgt * Lb) * b["marginal_hit"][:, None] + wgt * (np.abs(term) * b["marginal_inner"][..., None]).sum(axis=1))
    full_r, full_s = np.zeros((H * S, W * S, 3)), np.zeros((H * S, W * S, 3))
    full_r[tr["lit"]], full_s[tr["lit"]] = rad / (Q * Q), slack / (Q * Q)

    def pixels(a):
        return a.reshape(H, S, W, S, -1).mean(axis=(1, 3)).transpose(2, 0, 1)

    return {"image": out["image"] + pixels(full_r), "slack": out["slack"] + pixels(full_s), "unsafe_pixel": out["unsafe_pixel"], "shadowed": out["image"]}


def render(positions, normals, faces, z, env, Rot, H, W, S, Q, bounces=1, bounce_quad=4):
    """drm_render_mesh with bounces = 1 for one row (bounces=0: shadow_ref.render, the shadowed image), with the trace added under "trace" """
    if not bounces:
        return sr.render(positions, normals, faces, z, env, Rot, H, W, S, Q)
    tr = trace(positions, normals, faces, z, Rot, H, W, S, Q, bounce_quad)
    out = shade(tr, env)
    out["trace"] = tr
    return out

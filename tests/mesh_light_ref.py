"""float64 numpy restatement of light sampling on the mesh object images (drm_render_mesh with light samples: mesh_shade_kernel<VIEW, SHADOW, true> in
csrc/render.hip), written from the estimator in include/drmnet_hip.h.  It composes the three restatements it stands on and adds nothing of
its own but the composition: light_ref (Density, light_table, light_pdf, _power), shadow_ref (trace, occluded(..., marginal=True)) and
render_ref.lobes.  Used by tests/test_mesh_light_cpu.py and tests/test_gpu_mesh_light.py; nothing here touches a GPU.

The estimator.  For a hit sample with shading normal n (n.z > 0), origin o (the view-space hit point taken to object space with Rot) and hit
face g the integrand is L(w) V(w) f(w) cos: V(w) = 0 iff the ray (o, w) is occluded by shadow_ref's rule with exclude = g; without shadows
V = 1.  Both techniques of light_ref.render_mis estimate it with the weights they have there (n_s = n_d = Q^2, n_L = M):
  each lobe sample keeps its power-heuristic weight (n p)^2 / ((n p)^2 + (n_L p_L)^2) and contributes only if the ray along Rot l is open;
  each light-table entry k with p_L > 0 and n.l_k > 0 keeps its term L_k [f_s cos n_L p_L / ((n_s p_s)^2 + (n_L p_L)^2) + f_d cos n_L p_L /
  ((n_d p_d)^2 + (n_L p_L)^2)] and contributes only if the ray along its table direction d_k -- a world direction, which is the object-space
  ray direction; l_k = Rot^T d_k for the BSDF -- is open.
p_L knows nothing of occlusion; the weights of a direction still sum to one.  M == 0, or a map without light (tot == 0), is shadow_ref.shade.

Slack: the sum of the absolute contributions of a pixel's marginal rays (shadow_ref's definition), lobe rays and light rays alike."""
import numpy as np

import light_ref as lr
import render_ref as rr
import shadow_ref as sr

PI = np.pi


def light_terms(z, n, table, Q, M, R):
    """the term of every (lit sample, table entry): (term [K, Kl, 3], up [K, Kl] = n.l_k > 0) for normals n [K, 3] and the entries of
    `table` = (d, L, p_L) with p_L > 0; the expressions of light_ref._mis_rows"""
    m, c, r, alpha, eta = rr.params(z)
    d, L, pl = table
    ns = nd = float(Q * Q)
    l = d @ R  # Rot^T d: the table direction in the view frame
    nn = n[:, None, :]
    v = np.array([0.0, 0.0, 1.0])
    cv = nn[..., 2]
    cl = rr._dot(nn, l[None])
    up = cl > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        h = rr._normalize(l + v)[None]
        nh, cd = rr._dot(nn, h), h[..., 2]
        lh = rr._dot(l[None], h)
        D = rr.ggx_d(alpha, nh)
        g1v = rr.ggx_g1(alpha, cv, cd)
        F = (1 - m) * rr.fresnel_dielectric(cd, eta)[..., None] + m * (c + (1 - c) * rr.schlick(cd)[..., None])
        fs = F * (D * g1v * rr.ggx_g1(alpha, cl, lh) / (4 * cv))[..., None]
        fd = (1 - m) * (c / PI) * (cl * rr.diffuse_shape(r, cl, cv, cd))[..., None]
        a = M * pl
        ps = g1v * D / (4 * cv)
        pd = cl / PI if m < 1 else np.zeros_like(cl)
        ws = a / ((ns * ps) ** 2 + a * a)
        wd = a / ((nd * pd) ** 2 + a * a)
        term = L[None] * (fs * ws[..., None] + fd * wd[..., None])
    return np.where(up[..., None], term, 0.0), up


def shade(tr, env, M, positions=None, faces=None):
    """The row's pixels under env [EH, EW, 3] with M light samples, from a `trace` of this module (traced with or without shadows: the light
    rays follow it; `positions` and `faces` are needed when it was traced with them) -> dict of image, slack [3, H, W], unsafe_pixel [H, W]
    like shadow_ref.shade, and the ray counts: lobe_traced / lobe_marginal / lobe_occluded, light_traced / light_marginal / light_occluded."""
    H, W, S, Q = tr["shape"]
    den = lr.Density(env)
    counts = dict(lobe_traced=tr["traced"], lobe_marginal=tr["marginal"], lobe_occluded=tr["occluded"], light_traced=0, light_marginal=0, light_occluded=0)
    if M == 0 or den.tot <= 0:
        return {**sr.shade(tr, env), **counts}
    R = np.eye(3) if tr["Rot"] is None else np.asarray(tr["Rot"], dtype=np.float64)
    n = tr["normal"][tr["lit"]]
    K = len(n)
    rad, slack = np.zeros((K, 3)), np.zeros((K, 3))
    for name in ("spec", "diff"):
        l = tr["l_" + name]
        if l is None:
            continue
        ok = tr["traced_spec"] if name == "spec" else np.ones(l.shape[:-1], dtype=bool)
        w = tr["w_" + name] * np.where(ok, lr._power(float(Q * Q) * tr["pdf_" + name], M * lr.light_pdf(den, l @ R.T)), 0.0)[..., None]
        term = w * rr.env_lookup(den.env, l, tr["Rot"])
        rad += (term * tr["open_" + name][..., None]).sum(axis=1) / (Q * Q)
        slack += (np.abs(term) * tr["marginal_" + name][..., None]).sum(axis=1) / (Q * Q)
    d, L, pl = lr.light_table(den, M)
    keep = pl > 0
    table = (d[keep], L[keep], pl[keep])
    Kl = int(keep.sum())
    term, up = light_terms(tr["z"], n, table, Q, M, R)
    if tr["shadows"]:
        # only the entries past the cheap rejections are traced
        si, ki = np.nonzero(up)
        hit_r, marg_r = sr.occluded(positions, faces, tr["origin"][si], table[0][ki], tr["face"][si], marginal=True)
        hit, marg = np.zeros((K, Kl), dtype=bool), np.zeros((K, Kl), dtype=bool)
        hit[si, ki], marg[si, ki] = hit_r, marg_r
    else:
        hit = marg = np.zeros((K, Kl), dtype=bool)
    rad += (term * (~hit)[..., None]).sum(axis=1)
    slack += (np.abs(term) * marg[..., None]).sum(axis=1)
    counts.update(light_traced=int(up.sum()), light_marginal=int(marg.sum()), light_occluded=int(hit.sum()))
    return {"image": film(tr, rad), "slack": film(tr, slack), "unsafe_pixel": film(tr, None), **counts}


def film(tr, per_sample):
    """per-lit-sample values [K, 3] -> box-filtered pixels [3, H, W]; None: the unsafe-pixel mask [H, W] of shadow_ref.shade"""
    H, W, S, _ = tr["shape"]

    def pixels(a):
        return a.reshape(H, S, W, S, -1).mean(axis=(1, 3)).transpose(2, 0, 1)

    if per_sample is None:
        return pixels(tr["vis"]["unsafe"].astype(np.float64)[..., None])[0] > 0
    full = np.zeros((H * S, W * S, 3))
    full[tr["lit"]] = per_sample
    return pixels(full)


def texel_sum(tr, env, supersample, positions=None, faces=None, open_rays=None, samples=None):
    """An independent estimate of the same pixels: the integral of L V f cos as a sum over the directions of a supersample x supersampled
    lat-long grid (the map read with the same bilinear lookup), every direction above the surface traced with the occlusion rule where `tr`
    was traced with shadows.  -> (per-sample radiance [K, 3], open [K, D] bool: which directions are not cut off).  `open_rays`: a mask
    computed earlier (it depends on the scene, the view and the grid, not on z or the map), used instead of tracing.  `samples`: the lit
    samples to do (others stay 0 / open)."""
    EH, EW = env.shape[:2]
    d, dw = rr.env_dirs(EH * supersample, EW * supersample)
    d, dw = d.reshape(-1, 3), dw.reshape(-1)
    Ldw = rr.env_lookup(np.asarray(env, dtype=np.float64), d) * dw[:, None]
    R = np.eye(3) if tr["Rot"] is None else np.asarray(tr["Rot"], dtype=np.float64)
    l = d @ R
    n = tr["normal"][tr["lit"]]
    K = len(n)
    v = np.array([0.0, 0.0, 1.0])
    rad = np.zeros((K, 3))
    is_open = np.ones((K, len(d)), dtype=bool) if open_rays is None else np.asarray(open_rays, dtype=bool)
    for k in (range(K) if samples is None else samples):
        if open_rays is None and tr["shadows"]:
            up = np.nonzero(l @ n[k] > 0)[0]
            is_open[k, up] = ~sr.occluded(positions, faces, np.repeat(tr["origin"][k:k + 1], len(up), axis=0), d[up], np.full(len(up), tr["face"][k]))
        rad[k] = (rr.eval_bsdf(tr["z"], n[k], v, l) * Ldw * is_open[k][:, None]).sum(axis=0)
    return rad, is_open


def trace(positions, normals, faces, z, Rot, H, W, S, Q, shadows=True):
    """shadow_ref.trace with what the light technique also needs of a row: z, the lobe densities and whether it was traced"""
    tr = sr.trace(positions, normals, faces, z, Rot, H, W, S, Q, shadows)
    spec, diff = rr.lobes(z, tr["normal"][tr["lit"]], Q)
    tr.update(z=z, shadows=bool(shadows), pdf_spec=spec.pdf, pdf_diff=None if diff is None else diff.pdf)
    return tr


def render(positions, normals, faces, z, env, Rot, H, W, S, Q, M, shadows=True):
    """drm_render_mesh with light samples for one row (shadows=False: bvh == NULL): shade(trace(...)) with the trace added under "trace" """
    tr = trace(positions, normals, faces, z, Rot, H, W, S, Q, shadows)
    out = shade(tr, env, M, positions, faces)
    out["trace"] = tr
    return out

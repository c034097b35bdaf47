"""float64 numpy restatement of the measured-BRDF (MERL table) path (drmnet_amd/merl.py, drmnet_amd/csrc/brdf_table.hip), written from its
definition: the export of a principled row to a table, the table coordinates of a direction pair, both lookup modes, the proxy roughness and
the combined quadrature of the renders.  It reuses render_ref (lobes, sensor_normals, env_lookup, eval_bsdf) and takes nothing from
drmnet_amd.  Used by tests/test_merl_cpu.py and tests/test_gpu_merl.py; nothing here touches a GPU.

A table is [3, 90, 90, 180] = (colour, theta_h, theta_d, phi_d), a negative entry marking "no measurement / below the horizon".  Node
(i, j, k) stands for theta_h = (i / 90)^2 pi / 2, theta_d = j pi / 180, phi_d = k pi / 180."""
import numpy as np

import render_ref as rr

PI = np.pi
NH, ND, NP = 90, 90, 180
SCALES = np.array([1.0 / 1500.0, 1.15 / 1500.0, 1.66 / 1500.0])
SNAP = 1e-12  # a cosine of the export grid below this is the rounding of an exact zero (theta_h + theta_d = pi / 2 at phi_d = 0)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def export(z, i=None, j=None, k=None):
    """bsdf_to_merl of the canonical row z [6] -> [3, 90, 90, 180] (or the sub-grid of the index lists i, j, k): in the half-vector frame
    (h = +z) the normal is (-sin theta_h, 0, cos theta_h), the viewer wo = (sin theta_d cos phi_d, sin theta_d sin phi_d, cos theta_d), the
    light wi = wo (-1, -1, 1); entry = eval(n, wo, wi) / (n.wi); -1 where n.wo < 0 or n.wi < 0, 0 where a cosine is exactly 0."""
    i, j, k = np.meshgrid(*(np.arange(full) if sub is None else np.asarray(sub) for sub, full in ((i, NH), (j, ND), (k, NP))), indexing="ij")
    t = i / 90.0
    th, td, pd = t * t * (PI / 2), j * (PI / 180), k * (PI / 180)
    n = np.stack([-np.sin(th), np.zeros_like(th), np.cos(th)], axis=-1)
    wo = np.stack([np.sin(td) * np.cos(pd), np.sin(td) * np.sin(pd), np.cos(td)], axis=-1)
    wi = wo * np.array([-1.0, -1.0, 1.0])
    co, ci = _dot(n, wo), _dot(n, wi)
    co, ci = np.where(np.abs(co) < SNAP, 0.0, co), np.where(np.abs(ci) < SNAP, 0.0, ci)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = rr.eval_bsdf(np.asarray(z, dtype=np.float64), n, wo, wi) / ci[..., None]
    val = np.where(((co > 0) & (ci > 0))[..., None], val, 0.0)
    val = np.where(((co < 0) | (ci < 0))[..., None], -1.0, val)
    return np.ascontiguousarray(val.transpose(3, 0, 1, 2))


def coordinates(n, v, l):
    """(x_h, x_d, x_p) of unit n, v (toward the viewer), l (toward the light) [..., 3]: the continuous table coordinates
    x_h = 90 sqrt(theta_h / (pi / 2)), x_d = 90 theta_d / (pi / 2), x_p = 180 phi_d / pi with phi_d in [0, pi)."""
    n, v, l = (np.asarray(a, dtype=np.float64) for a in (n, v, l))
    h = v + l
    h = h / np.sqrt(_dot(h, h))[..., None]
    nh, lh = _dot(n, h), _dot(l, h)
    th = np.arctan2(np.sqrt(_dot(np.cross(n, h), np.cross(n, h))), nh)
    td = np.arctan2(np.sqrt(_dot(np.cross(l, h), np.cross(l, h))), lh)
    p = n - nh[..., None] * h
    pl = np.sqrt(_dot(p, p))
    with np.errstate(divide="ignore", invalid="ignore"):
        xh = -p / pl[..., None]
        yh = np.cross(h, xh)
        ph = np.arctan2(_dot(v, yh), _dot(v, xh))
    ph = np.where(ph < 0, ph + PI, ph)
    ph = np.where(ph >= PI, ph - PI, ph)
    ph = np.where(pl < 1e-6, 0.0, ph)
    return 90.0 * np.sqrt(th / (PI / 2)), 90.0 * td / (PI / 2), 180.0 * ph / PI


def lookup(table, n, v, l, mode="linear"):
    """f_table(n, v, l) [..., 3]: 0 unless n.v > 0 and n.l > 0.  nearest: floor and clamp, a negative entry reads 0.  linear: trilinear
    between floor and floor + 1 (clamped at 89 in theta_h and theta_d, wrapping 179 -> 0 in phi_d), corners with a negative entry dropped
    and the remaining weights renormalised; 0 where all eight are dropped."""
    T = np.asarray(table, dtype=np.float64)
    n, v, l = (np.asarray(a, dtype=np.float64) for a in (n, v, l))
    ok = (_dot(n, v) > 0) & (_dot(n, l) > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        xh, xd, xp = coordinates(n, v, l)
    xh, xd, xp = (np.where(ok, x, 0.0) for x in (xh, xd, xp))
    fh, fd, fp = np.floor(xh), np.floor(xd), np.floor(xp)
    ih, id_, ip = fh.astype(np.int64), fd.astype(np.int64), fp.astype(np.int64)
    if mode == "nearest":
        e = T[:, np.clip(ih, 0, NH - 1), np.clip(id_, 0, ND - 1), np.clip(ip, 0, NP - 1)]
        val = np.where(e[0] < 0, 0.0, e)
    else:
        assert mode == "linear"
        num, den = 0.0, 0.0
        for a in (0, 1):
            wa = (xh - fh) if a else 1.0 - (xh - fh)
            ia = np.clip(ih + a, 0, NH - 1)
            for b in (0, 1):
                wb = (xd - fd) if b else 1.0 - (xd - fd)
                ib = np.clip(id_ + b, 0, ND - 1)
                for c in (0, 1):
                    wc = (xp - fp) if c else 1.0 - (xp - fp)
                    ic = np.mod(ip + c, NP)
                    e = T[:, ia, ib, ic]
                    w = np.where(e[0] < 0, 0.0, wa * wb * wc)
                    num = num + w * e
                    den = den + w
        with np.errstate(invalid="ignore", divide="ignore"):
            val = np.where(den > 0, num / den, 0.0)
    return np.where(ok, val, 0.0).transpose(*range(1, val.ndim), 0)


def eval_table(table, n, v, l, mode="linear"):
    """Mitsuba's eval convention: the lookup times n.l"""
    return lookup(table, n, v, l, mode) * _dot(np.asarray(n, dtype=np.float64), np.asarray(l, dtype=np.float64))[..., None]


def proxy_alpha(table):
    """The GGX roughness the renders place their specular samples with: the half width at half maximum of the luminance profile along theta_h
    at (theta_d, phi_d) = (0, 0), read as a GGX D (whose half maximum lies at tan^2 theta = alpha^2 (sqrt 2 - 1)); 1 for a profile without a peak."""
    T = np.asarray(table, dtype=np.float64)
    lum = 0.2126 * T[0, :, 0, 0] + 0.7152 * T[1, :, 0, 0] + 0.0722 * T[2, :, 0, 0]
    valid = T[0, :, 0, 0] >= 0
    if not valid[0] or not valid.any():
        return 1.0
    floor = lum[valid].min()
    peak = lum[0] - floor
    if not peak > 1e-6 * floor:
        return 1.0
    half = floor + 0.5 * peak
    x = float(NH - 1)
    for i in range(1, NH):
        if not valid[i] or lum[i] <= half:
            x = float(i) if not valid[i] or lum[i - 1] == lum[i] else (i - 1) + (lum[i - 1] - half) / (lum[i - 1] - lum[i])
            break
    th = (x / 90.0) ** 2 * (PI / 2)
    return float(np.clip(np.tan(th) / np.sqrt(np.sqrt(2.0) - 1.0), 0.005, 1.0))


def sample_radiance(table, alpha, env, n, Q, rot=None, mode="linear"):
    """The combined quadrature at unit normals n [..., 3] with n.z > 0 -> [..., 3]: both sample sets of render_ref.lobes at roughness alpha
    (the GGX visible normals seen from v = +z, and the cosine-weighted directions), each sample l weighted by the balance heuristic:
    L(rot l) f_table(n, v, l) (n.l) / (Q^2 (p_s(l) + p_d(l))), p_s = G1(v) D(h) / (4 n.v) at h = normalize(v + l), p_d = n.l / pi."""
    n = np.asarray(n, dtype=np.float64)
    v = np.array([0.0, 0.0, 1.0])
    spec, diff = rr.lobes([0.0, 1.0, 1.0, 1.0, np.sqrt(alpha), 0.5], n, Q)
    nn = n[..., None, :]
    cv = nn[..., 2]
    acc = 0.0
    for lobe in (spec, diff):
        l = lobe.l
        cl = _dot(nn, l)
        h = l + v
        h = h / np.sqrt(_dot(h, h))[..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            ps = rr.ggx_g1(alpha, cv, h[..., 2]) * rr.ggx_d(alpha, _dot(nn, h)) / (4 * cv)
            use = lobe.ok & (cl > 0)
            f = lookup(table, np.broadcast_to(nn, l.shape), np.broadcast_to(v, l.shape), np.where(use[..., None], l, v), mode)
            w = np.where(use, cl / (ps + cl / PI), 0.0)
        c = f * w[..., None]
        if env is not None:
            c = c * rr.env_lookup(env, l, rot)
        acc = acc + c.sum(axis=-2)
    return acc / (Q * Q)


def render_table(table, alpha, env, R, Q=32, S=2, flip=False, rot=None, mode="linear"):
    """drm_render_refmap under a table for one row in float64: [3, R, R]"""
    n = rr.sensor_normals(R, S, flip)
    rows = max(1, (1 << 18) // (R * S * S * Q * Q))
    out = [sample_radiance(table, alpha, env, n[i:i + rows], Q, rot, mode).mean(axis=2) for i in range(0, R, rows)]
    return np.concatenate(out, axis=0).transpose(2, 0, 1)


def shade(table, alpha, env, normals, mask, Q, rot=None, mode="linear"):
    """drm_render_normals under a table for one row -> (image [3, H, W], drawn [H, W]); normals as relight_ref.unit_normals takes them"""
    import relight_ref as rl

    n, drawn = rl.unit_normals(normals, mask)
    out = np.zeros(n.shape)
    out[drawn] = sample_radiance(table, alpha, env, n[drawn], Q, rot, mode)
    return out.transpose(2, 0, 1), drawn

"""float64 numpy restatement of the reflectance-map forward model (drmnet_amd/csrc/render.hip), written from its definition:
Mitsuba 3's principled BSDF restricted to (metallic, base colour, roughness, specular), the RefMapSensor geometry and the lat-long
envmap lookup.  Used by tests/test_render_cpu.py and tests/test_gpu_render.py; nothing here touches a GPU.

A canonical BSDF row is z = (metallic m, base colour c_R, c_G, c_B, roughness r, specular s).  Vectors are [..., 3] arrays."""
from collections import namedtuple

import numpy as np

PI = np.pi


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _normalize(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def params(z):
    z = np.clip(np.asarray(z, dtype=np.float64), 0.0, 1.0)
    m, c, r, s = z[..., 0], z[..., 1:4], z[..., 4], z[..., 5]
    alpha = np.maximum(0.001, r * r)
    eta = 2.0 / (1.0 - np.sqrt(0.08 * s)) - 1.0
    return m, c, r, alpha, eta


def ggx_d(alpha, nh):
    a2 = alpha * alpha
    d = a2 / (PI * (nh * nh * (a2 - 1.0) + 1.0) ** 2)
    return np.where(d * nh > 1e-20, d, 0.0)


def ggx_g1(alpha, cw, wh):
    """Smith G1 at cos cw = n.w with w.h = wh"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tan2 = np.where(cw != 0.0, (1.0 - cw * cw) / (cw * cw), np.inf)
        g = 2.0 / (1.0 + np.sqrt(1.0 + alpha * alpha * tan2))
    g = np.where(tan2 <= 0.0, 1.0, g)
    return np.where(wh * cw <= 0.0, 0.0, g)


def fresnel_dielectric(cd, eta):
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_t = np.sqrt(np.maximum(1.0 - (1.0 - cd * cd) / (eta * eta), 0.0))
        a_s = (cd - eta * cos_t) / (cd + eta * cos_t)
        a_p = (cos_t - eta * cd) / (cos_t + eta * cd)
        f = 0.5 * (a_s * a_s + a_p * a_p)
    return np.where(eta == 1.0, 0.0, f)


def schlick(c):
    return np.clip(1.0 - c, 0.0, 1.0) ** 5


def diffuse_shape(r, cl, cv, cd):
    fl, fv, rr = schlick(cl), schlick(cv), 2.0 * r * cd * cd
    return (1.0 - 0.5 * fl) * (1.0 - 0.5 * fv) + rr * (fl + fv + fl * fv * (rr - 1.0))


def eval_bsdf(z, n, v, l):
    """f(v, l) (n.l) per channel -> [..., 3]; z [6] or [..., 6] broadcast against the vectors"""
    n, v, l = (np.asarray(a, dtype=np.float64) for a in (n, v, l))
    m, c, r, alpha, eta = params(z)
    m, r, alpha, eta = (np.asarray(a)[..., None] for a in (m, r, alpha, eta))  # [..., 1] against the [..., 3] channel axis
    cv, cl = _dot(n, v)[..., None], _dot(n, l)[..., None]
    ok = (cv > 0) & (cl > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = _normalize(v + l)
        h = np.where(_dot(n, h)[..., None] < 0, -h, h)
        nh, cd, lh = _dot(n, h)[..., None], _dot(h, v)[..., None], _dot(l, h)[..., None]
        D = ggx_d(alpha, nh)
        G = ggx_g1(alpha, cv, cd) * ggx_g1(alpha, cl, lh)
        F = (1.0 - m) * fresnel_dielectric(cd, eta) + m * (c + (1.0 - c) * schlick(cd))
        spec = F * D * G / (4.0 * cv)
        diff = (1.0 - m) * (c / PI) * cl * diffuse_shape(r, cl, cv, cd)
        out = spec + diff
    return np.where(ok, out, 0.0)


def env_dirs(EH, EW):
    """[EH, EW, 3] direction of every texel centre, and its solid angle weight sin(theta) dtheta dpsi"""
    th = (np.arange(EH) + 0.5) * PI / EH
    ps = (np.arange(EW) + 0.5) * 2 * PI / EW
    T, P = np.meshgrid(th, ps, indexing="ij")
    d = np.stack([np.sin(T) * np.sin(P), np.cos(T), -np.sin(T) * np.cos(P)], axis=-1)
    return d, np.sin(T) * (PI / EH) * (2 * PI / EW)


def env_lookup(env, w, rot=None):
    """bilinear radiance of env [EH, EW, 3] toward unit directions w [..., 3] (rot [3, 3]: toward rot w): wraps in psi, clamps in theta"""
    EH, EW = env.shape[:2]
    if rot is not None:
        w = w @ np.asarray(rot, dtype=np.float64).T
    u = np.arctan2(w[..., 0], -w[..., 2]) / (2 * PI)
    t = np.arccos(np.clip(w[..., 1], -1, 1)) / PI
    x = u * EW - 0.5
    y = np.clip(t * EH - 0.5, 0, EH - 1)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    j0 = np.mod(x0.astype(np.int64), EW)
    j1 = np.mod(j0 + 1, EW)
    i0 = y0.astype(np.int64)
    i1 = np.minimum(i0 + 1, EH - 1)
    e = np.asarray(env, dtype=np.float64)
    top = (1 - fx) * e[i0, j0] + fx * e[i0, j1]
    bot = (1 - fx) * e[i1, j0] + fx * e[i1, j1]
    return (1 - fy) * top + fy * bot


def sensor_normals(R, S, flip=False):
    """[R, R, S*S, 3] normals of the S x S sub-pixel positions of every pixel (row i from the top, column j from the left)"""
    off = (np.arange(S) + 0.5) / S
    px = (np.arange(R)[:, None] + off[None, :]).reshape(-1) / R  # [R*S] film x of column j, sub-column sx
    a = (2 * px - 1) * PI / 2
    b = (1 - 2 * px) * PI / 2  # the same positions down the rows
    B_, A_ = np.meshgrid(b, a, indexing="ij")  # [R*S, R*S]
    n = np.stack([np.cos(B_) * np.sin(A_), np.sin(B_), np.cos(B_) * np.cos(A_)], axis=-1)
    if flip:
        n[..., 0] = -n[..., 0]
    return n.reshape(R, S, R, S, 3).transpose(0, 2, 1, 3, 4).reshape(R, R, S * S, 3)


Lobe = namedtuple("Lobe", "l w ok pdf")


def lobes(z, n, Q):
    """The lobe construction, stated once: for unit normals n [..., 3] with n.z > 0 and every point q = q1 Q + q2 of the Q x Q midpoint grid,
    (specular, diffuse) as Lobe(l [..., Q^2, 3] direction, w [..., Q^2, 3] RGB weight, ok [..., Q^2] validity, pdf [..., Q^2] sampling
    density); diffuse is None when m == 1.  The radiance toward +z is (sum w_s L(l_s) + sum w_d L(l_d)) / Q^2.
    Specular: h from the visible normals of GGX seen from v (Heitz 2018), l = reflect(v, h), w = F G1(l) (0 where not ok),
    pdf = G1(v) D / (4 n.v).  Diffuse: cosine-weighted l, w = c (1 - m) shape, pdf = n.l / pi, ok everywhere."""
    m, c, r, alpha, eta = params(z)
    n = np.asarray(n, dtype=np.float64)[..., None, :]
    v = np.array([0.0, 0.0, 1.0])
    cv = n[..., 2]
    ka = -1.0 / (1.0 + n[..., 2])  # the frame (t, bt, n) of Duff et al. 2017
    kb = n[..., 0] * n[..., 1] * ka
    t = np.stack([1 + n[..., 0] ** 2 * ka, kb, -n[..., 0]], axis=-1)
    bt = np.stack([kb, 1 + n[..., 1] ** 2 * ka, -n[..., 1]], axis=-1)
    g = (np.arange(Q) + 0.5) / Q
    U1, U2 = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    cp, sp = np.cos(2 * PI * U2), np.sin(2 * PI * U2)
    V = np.stack([-alpha * n[..., 0], -alpha * n[..., 1], cv], axis=-1)  # v in the (t, bt, n) frame, stretched
    V = V / np.linalg.norm(V, axis=-1, keepdims=True)
    lensq = V[..., 0] ** 2 + V[..., 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        T1 = np.where((lensq > 0)[..., None], np.stack([-V[..., 1], V[..., 0], np.zeros_like(lensq)], axis=-1) / np.sqrt(lensq)[..., None],
                      np.array([1.0, 0.0, 0.0]))
    T2 = np.cross(V, T1)
    rs = np.sqrt(U1)
    t1 = rs * cp
    vs = 0.5 * (1 + V[..., 2])
    t2 = (1 - vs) * np.sqrt(1 - t1 * t1) + vs * rs * sp
    tz = np.sqrt(np.maximum(1 - t1 * t1 - t2 * t2, 0))
    Nh = t1[:, None] * T1 + t2[..., None] * T2 + tz[..., None] * V
    Ne = np.stack([alpha * Nh[..., 0], alpha * Nh[..., 1], np.maximum(Nh[..., 2], 0)], axis=-1)
    Ne = Ne / np.linalg.norm(Ne, axis=-1, keepdims=True)
    h = Ne[..., 0:1] * t + Ne[..., 1:2] * bt + Ne[..., 2:3] * n
    vh = h[..., 2]
    l = 2 * vh[..., None] * h - v
    cl = _dot(n, l)
    D = ggx_d(alpha, Ne[..., 2])
    ok = (vh > 0) & (cl > 0) & (D > 0)
    F = (1 - m) * fresnel_dielectric(vh, eta)[..., None] + m * (c + (1 - c) * schlick(vh)[..., None])
    with np.errstate(divide="ignore", invalid="ignore"):
        spec = Lobe(l, F * np.where(ok, ggx_g1(alpha, cl, vh), 0.0)[..., None], ok, ggx_g1(alpha, cv, vh) * D / (4 * cv))
    if not m < 1:
        return spec, None
    cl = np.sqrt(1 - U1)
    l = cl[:, None] * n + (rs * cp)[:, None] * t + (rs * sp)[:, None] * bt
    cd = _normalize(l + v)[..., 2]
    w = c * ((1 - m) * diffuse_shape(r, cl, cv, cd))[..., None]
    return spec, Lobe(l, w, np.ones(ok.shape, dtype=bool), np.broadcast_to(cl / PI, ok.shape))


def render_quadrature(z, env, R, Q=32, S=2, flip=False):
    """The kernel's quadrature in float64: [3, R, R].  env [EH, EW, 3] or None (white)."""
    n = sensor_normals(R, S, flip)
    rows = max(1, (1 << 19) // (R * S * S * Q * Q))
    return np.concatenate([_quadrature(z, env, n[i:i + rows], Q) for i in range(0, R, rows)], axis=1)


def _quadrature(z, env, n, Q, rot=None):
    """the plain sum over both lobes and the S2 normals of every pixel: n [rows, R, S2, 3] -> [3, rows, R]; the environment is read at rot l"""
    acc = 0.0
    for lobe in lobes(z, n, Q):
        if lobe is not None:
            acc = acc + (lobe.w if env is None else lobe.w * env_lookup(env, lobe.l, rot)).sum(axis=(2, 3))
    return (acc / (n.shape[2] * Q * Q)).transpose(2, 0, 1)


def render_texel_sum(z, env, R, S=2, supersample=4, flip=False, rows=None):
    """An independent estimate of the same pixels: the integral as a sum over the directions of a supersample x supersampled
    lat-long grid (the envmap read with the same bilinear lookup), at the S x S sub-pixel normals.  [3, R, R], or [3, len(rows), R]
    for the pixel rows `rows` only."""
    EH, EW = env.shape[:2]
    d, dw = env_dirs(EH * supersample, EW * supersample)
    d, dw = d.reshape(-1, 3), dw.reshape(-1)
    L = env_lookup(env, d)
    n = sensor_normals(R, S, flip)
    n = (n if rows is None else n[rows]).reshape(-1, 3)
    v = np.array([0.0, 0.0, 1.0])
    out = np.zeros((n.shape[0], 3))
    for k in range(0, n.shape[0], 64):
        nk = n[k:k + 64, None, :]
        f = eval_bsdf(z, nk, v, d[None])
        out[k:k + 64] = (f * (L * dw[:, None])[None]).sum(axis=1)
    return out.reshape(-1, R, S * S, 3).mean(axis=2).transpose(2, 0, 1)

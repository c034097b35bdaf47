"""float64 numpy restatement of the light-sampled render (drmnet_amd/csrc/render_light.hip), written from its definition: the light
density of a lat-long environment map on the dual grid of the bilinear lookup, its Hammersley sample table, and the lobe-separated
multiple-importance-sampling render (power heuristic, beta = 2) that combines the table with the quadrature of render_ref.
Used by tests/test_render_light_cpu.py and tests/test_gpu_render_light.py; nothing here touches a GPU.

Cells: rows c = 0 .. EH, columns j = 0 .. EW - 1.  Cell (c, j) spans theta in [(c - 1/2), (c + 1/2)] pi / EH clipped to [0, pi] (the two
polar rows are half cells) and psi in [(j + 1/2), (j + 3/2)] 2 pi / EW (wrapping); its corners are the texels (clamp(c - 1), clamp(c)) x
(j, j + 1 mod EW), where render_ref.env_lookup is exactly bilinear."""
import numpy as np

import render_ref as rr

PI = np.pi
LUMA = np.array([0.2126, 0.7152, 0.0722])


def luminance(env):
    """Rec. 709 luminance of env [EH, EW, 3], clamped at 0"""
    return np.maximum(np.asarray(env, dtype=np.float64) @ LUMA, 0.0)


class Density:
    """row extents, corner luminances, row masses, marginal CDF and total of one map"""

    def __init__(self, env):
        env = np.asarray(env, dtype=np.float64)
        self.env = env
        EH, EW = env.shape[:2]
        self.EH, self.EW = EH, EW
        c = np.arange(EH + 1)
        self.lo = np.clip((c - 0.5) * PI / EH, 0.0, PI)
        self.hi = np.clip((c + 0.5) * PI / EH, 0.0, PI)
        self.sc = np.sin(0.5 * (self.lo + self.hi))
        self.dpsi = 2 * PI / EW
        self.i0 = np.clip(c - 1, 0, EH - 1)
        self.i1 = np.clip(c, 0, EH - 1)
        lum = luminance(env)
        self.lum = lum
        nxt = np.roll(lum, -1, axis=1)  # column j + 1 mod EW
        # corner luminances of every cell [EH + 1, EW]: v{theta}{psi}
        self.v00, self.v01, self.v10, self.v11 = lum[self.i0], nxt[self.i0], lum[self.i1], nxt[self.i1]
        self.mean4 = 0.25 * (self.v00 + self.v01 + self.v10 + self.v11)
        self.rowsum = self.mean4.sum(axis=1)
        self.mass = self.rowsum * self.sc * (self.hi - self.lo)
        self.cdf = np.concatenate([[0.0], np.cumsum(self.mass)])
        self.tot = self.cdf[-1]


def light_pdf(den, w):
    """solid-angle pdf p_L of unit directions w [..., 3] under Density den (0 everywhere when den.tot == 0)"""
    w = np.asarray(w, dtype=np.float64)
    if den.tot <= 0:
        return np.zeros(w.shape[:-1])
    EH, EW = den.EH, den.EW
    theta = np.arccos(np.clip(w[..., 1], -1, 1))
    u = np.arctan2(w[..., 0], -w[..., 2]) / (2 * PI)
    y = theta / PI * EH - 0.5
    c = np.clip(np.floor(y).astype(np.int64) + 1, 0, EH)
    s = np.where((c > 0) & (c < EH), y - np.floor(y), 0.0)  # (the half cells are constant in theta: both corner rows are one texel row)
    x = u * EW - 0.5
    j = np.mod(np.floor(x).astype(np.int64), EW)
    t = x - np.floor(x)
    val = (1 - s) * ((1 - t) * den.v00[c, j] + t * den.v01[c, j]) + s * ((1 - t) * den.v10[c, j] + t * den.v11[c, j])
    return val * den.sc[c] / (den.tot * den.dpsi) / np.maximum(np.sin(theta), 1e-6)


def lininv(u, a, b):
    """x in [0, 1] with cdf(x) = u under the density proportional to (1 - x) a + x b; x = u where a + b = 0"""
    u, a, b = np.broadcast_arrays(np.asarray(u, dtype=np.float64), a, b)
    den = a + np.sqrt((1 - u) * a * a + u * b * b)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = u * (a + b) / den
    return np.where((a + b > 0) & (den > 0), x, u)


def bitreverse32(k):
    k = np.asarray(k, dtype=np.uint64)
    out = np.zeros_like(k)
    for bit in range(32):
        out |= ((k >> np.uint64(bit)) & np.uint64(1)) << np.uint64(31 - bit)
    return out


def hammersley(M):
    k = np.arange(M)
    return (k + 0.5) / M, bitreverse32(k).astype(np.float64) * 2.0 ** -32 + 0.5 / M


def light_table(den, M):
    """The M light samples of a map: (directions [M, 3], radiance [M, 3], p_L [M]).  Sample k is the Hammersley point (U1, U2): U1 picks the
    cell row through the marginal CDF, U2 the column through the row's conditional CDF, and the remapped pair the position inside the cell
    by inverting the bilinear density (theta from the linear marginal, then psi from the linear conditional)."""
    assert M >= 64 and M <= 65536 and M & (M - 1) == 0 and den.tot > 0
    U1, U2 = hammersley(M)
    t1 = U1 * den.tot
    c = np.clip(np.searchsorted(den.cdf, t1, side="right") - 1, 0, den.EH)
    with np.errstate(divide="ignore", invalid="ignore"):
        u1 = np.clip((t1 - den.cdf[c]) / den.mass[c], 0.0, 1.0)
    cond = np.cumsum(den.mean4[c], axis=1)  # [M, EW]
    t2 = U2 * den.rowsum[c]
    j = np.minimum((cond <= t2[:, None]).sum(axis=1), den.EW - 1)
    before = np.where(j > 0, cond[np.arange(M), np.maximum(j - 1, 0)], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u2 = (t2 - before) / den.mean4[c, j]
    u2 = np.where(np.isfinite(u2), np.clip(u2, 0.0, 1.0), 0.5)
    v00, v01, v10, v11 = den.v00[c, j], den.v01[c, j], den.v10[c, j], den.v11[c, j]
    s = lininv(u1, v00 + v01, v10 + v11)
    t = lininv(u2, (1 - s) * v00 + s * v10, (1 - s) * v01 + s * v11)
    theta = den.lo[c] + s * (den.hi[c] - den.lo[c])
    psi = (j + 0.5 + t) * den.dpsi
    d = np.stack([np.sin(theta) * np.sin(psi), np.cos(theta), -np.sin(theta) * np.cos(psi)], axis=-1)
    val = (1 - s) * ((1 - t) * v00 + t * v01) + s * ((1 - t) * v10 + t * v11)
    pdf = val * den.sc[c] / (den.tot * den.dpsi) / np.maximum(np.sin(theta), 1e-6)
    e = den.env
    j1 = np.mod(j + 1, den.EW)
    i0, i1 = den.i0[c], den.i1[c]
    s_, t_ = s[:, None], t[:, None]
    L = (1 - s_) * ((1 - t_) * e[i0, j] + t_ * e[i0, j1]) + s_ * ((1 - t_) * e[i1, j] + t_ * e[i1, j1])
    return d, L, pdf


def _power(a, b):
    """a^2 / (a^2 + b^2), 1 where b == 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = a * a / (a * a + b * b)
    return np.where(b == 0, 1.0, w)


def render_mis(z, env, R, Q=32, S=2, M=1024, flip=False, rot=None, rows=None):
    """The light-sampled render in float64: [3, R, R] (or [3, len(rows), R] for the pixel rows `rows`).  env [EH, EW, 3]; rot [3, 3] (or
    None: the view from +z): the environment is read at rot @ l.  M == 0, or a map without light (tot == 0), is the plain quadrature."""
    den = Density(env)
    lit = M > 0 and den.tot > 0
    n = rr.sensor_normals(R, S, flip)
    if rows is not None:
        n = n[rows]
    rot = np.eye(3) if rot is None else np.asarray(rot, dtype=np.float64)
    table = light_table(den, M) if lit else None
    per = max(1, (1 << 18) // (R * S * S * Q * Q))
    return np.concatenate([_mis_rows(z, den, n[i:i + per], Q, M if lit else 0, rot, table) for i in range(0, n.shape[0], per)], axis=1)


def _mis_rows(z, den, n, Q, M, rot, table):
    m, c, r, alpha, eta = rr.params(z)
    S2 = n.shape[2]
    ns = nd = float(Q * Q)
    # the lobes of render_ref, each sample weighted by the power heuristic against the light technique
    acc = 0.0
    for lobe in rr.lobes(z, n, Q):
        if lobe is None:
            continue
        w = lobe.w
        if M:
            w = w * np.where(lobe.ok, _power(ns * lobe.pdf, M * light_pdf(den, lobe.l @ rot.T)), 0.0)[..., None]
        acc = acc + (w * rr.env_lookup(den.env, lobe.l, rot)).sum(axis=(2, 3))
    acc = acc / (S2 * Q * Q)
    n = n[..., None, :]  # [rows, R, S2, 1, 3]
    v = np.array([0.0, 0.0, 1.0])
    cv = n[..., 2]
    if M:
        d, L, pl = table
        keep = pl > 0
        d, L, pl = d[keep], L[keep], pl[keep]
        l = d @ rot  # rot^T d: the table direction in the row's frame
        cl = rr._dot(n, l)  # [rows, R, S2, K]
        up = cl > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            h = rr._normalize(l + v)
            nh, cd = rr._dot(n, h), h[..., 2]
            lh = rr._dot(l, h)
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
            term = L * (fs * ws[..., None] + fd * wd[..., None])
        acc = acc + np.where(up[..., None], term, 0.0).sum(axis=(2, 3)) / S2
    return acc.transpose(2, 0, 1)

"""float64 numpy restatement of the normal-map images (drm_render_normals: normals_pixel_kernel in drmnet_amd/csrc/render_shared.h;
drm_image_from_refmap: image_from_refmap_kernel in csrc/refmap.hip), written from include/drmnet_hip.h.  No new physics: shading is
mesh_ref.sample_radiance on the unit normals, the lit form light_ref._mis_rows with light_ref.light_table, and the lookup is the header's
formulas.  Used by tests/test_relight_cpu.py and tests/test_gpu_relight.py; nothing here touches a GPU.

normals [H, W, 3] (any length), mask [H, W] or None; images come back [3, H, W], drawn / alpha [H, W]."""
import numpy as np

import light_ref as lr
import mesh_ref as mr

MARGIN = 1e-4  # texels: see lookup()


def normal_map(seed, H=12, W=12):
    """The normal map of the tests, as the GPU is given it: (normals [H, W, 3] float32, mask [H, W] bool).  Seeded unit normals with
    |n.z| >= 0.05, a third of them facing away (n.z < 0), and in row 0 the planted pixels: a zero normal, a NaN normal, n.z = 0 exactly, a
    masked-out pixel, and the normals of (1, 4) and (1, 5), both facing the viewer, scaled by 0.5 and by 2."""
    g = np.random.default_rng(seed)
    v = g.normal(size=(H, W, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    away = g.uniform(size=(H, W)) < 1.0 / 3.0
    away[1, 4:6] = False
    v[..., 2] = np.where(away, -1.0, 1.0) * np.maximum(np.abs(v[..., 2]), 0.05)
    v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    mask = np.ones((H, W), dtype=bool)
    v[0, 0] = 0.0
    v[0, 1] = (np.nan, 0.0, 1.0)
    v[0, 2] = (1.0, 0.0, 0.0)
    v[0, 3] = (0.0, 0.6, 0.8)
    mask[0, 3] = False
    v[0, 4] = np.float32(0.5) * v[1, 4]
    v[0, 5] = np.float32(2.0) * v[1, 5]
    return v, mask


def unit_normals(normals, mask=None):
    """(n [H, W, 3], drawn [H, W]): n = normal / |normal|; drawn where the mask is set, the normal is neither zero nor NaN nor infinite and
    n.z > 0; n is zero where the pixel is not drawn"""
    v = np.asarray(normals, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        len2 = np.sum(v * v, axis=-1)
        ok = (len2 > 0) & np.isfinite(len2)
        n = np.where(ok[..., None], v / np.sqrt(np.where(ok, len2, 1.0))[..., None], 0.0)
    drawn = ok & (n[..., 2] > 0)
    if mask is not None:
        drawn &= np.asarray(mask) != 0
    return np.where(drawn[..., None], n, 0.0), drawn


def shade(z, env, normals, mask, Q, Rot=None):
    """drm_render_normals for one row without light samples -> (image [3, H, W], drawn [H, W])"""
    n, drawn = unit_normals(normals, mask)
    return mr.sample_radiance(z, env, n, Q, Rot).transpose(2, 0, 1), drawn


def shade_lit(z, env, normals, mask, Q, M, Rot=None):
    """drm_render_normals for one row with M light samples (a map without light: the plain sum) -> (image [3, H, W], drawn [H, W])"""
    n, drawn = unit_normals(normals, mask)
    den = lr.Density(np.asarray(env, dtype=np.float64))
    lit = M > 0 and den.tot > 0
    rot = np.eye(3) if Rot is None else np.asarray(Rot, dtype=np.float64)
    out = np.zeros(n.shape)
    out[drawn] = lr._mis_rows(z, den, n[drawn].reshape(1, -1, 1, 3), Q, M if lit else 0, rot, lr.light_table(den, M) if lit else None)[:, 0].T
    return out.transpose(2, 0, 1), drawn


def texel_coordinates(n, R):
    """(ti, tj) of unit normals n [..., 3]: the inverse of n = (cos b sin a, sin b, cos b cos a), a = (2 px - 1) pi / 2,
    b = (1 - 2 py) pi / 2, with texel (i, j)'s centre at (py, px) = ((i + 1/2) / R, (j + 1/2) / R)"""
    a = np.arctan2(n[..., 0], n[..., 2])
    b = np.arcsin(np.clip(n[..., 1], -1.0, 1.0))
    return (0.5 - b / np.pi) * R - 0.5, (a / np.pi + 0.5) * R - 0.5


def lookup(refmap, refmask, normals, mask):
    """drm_image_from_refmap for one row: refmap [3, R, R], refmask [R, R] or None -> (image [3, H, W], alpha [H, W], marginal [H, W]).
    marginal: ti or tj lies within MARGIN of an integer, where an fp32 evaluation of the coordinates may take other taps."""
    v = np.asarray(refmap, dtype=np.float64)
    R = v.shape[-1]
    n, drawn = unit_normals(normals, mask)
    ti, tj = texel_coordinates(np.where(drawn[..., None], n, [0.0, 0.0, 1.0]), R)
    fi, fj = np.floor(ti), np.floor(tj)
    fy, fx = ti - fi, tj - fj
    i0, i1 = (np.clip(fi.astype(np.int64) + k, 0, R - 1) for k in (0, 1))
    j0, j1 = (np.clip(fj.astype(np.int64) + k, 0, R - 1) for k in (0, 1))
    top = (1 - fx) * v[:, i0, j0] + fx * v[:, i0, j1]
    bot = (1 - fx) * v[:, i1, j0] + fx * v[:, i1, j1]
    alpha = drawn.copy()
    if refmask is not None:
        m = np.asarray(refmask) != 0
        alpha &= m[i0, j0] & m[i0, j1] & m[i1, j0] & m[i1, j1]
    marginal = drawn & ((np.abs(ti - np.rint(ti)) < MARGIN) | (np.abs(tj - np.rint(tj)) < MARGIN))
    return np.where(alpha, (1 - fy) * top + fy * bot, 0.0), alpha, marginal

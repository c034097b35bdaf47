"""float64 numpy restatement of a mesh object image under a measured BRDF (drm_render_mesh_tables: mesh_table_shade_kernel in
csrc/mesh_table.hip), written from the contract in include/drmnet_hip.h and made of the restatements that already exist: shadow_ref.trace
gives mesh_ref's visibility and shading normals and, for the proxy row [0, 1, 1, 1, sqrt(alpha), 0.5], exactly the two sample sets of the
table render (the GGX visible normals of roughness alpha and the cosine-weighted directions) with their `open_*` / `marginal_*` masks and the
counts of traced, marginal and occluded rays; the lobe weights are then replaced by the table's balance-heuristic weights
f_table(n, v, l) (n.l) / (p_s + p_d) of merl_ref.sample_radiance, 0 where a sample is not used, and shadow_ref.shade gives `image`, `slack`
and `unsafe_pixel` unchanged.  Used by tests/test_mesh_merl_cpu.py and tests/test_gpu_mesh_merl.py; nothing here touches a GPU."""
import numpy as np

import merl_ref as mr
import render_ref as rr
import shadow_ref as sr

PI = np.pi


def proxy_row(alpha):
    """the principled row whose lobes are the table render's sample sets: a dielectric (so the cosine set exists) of GGX roughness alpha"""
    return [0.0, 1.0, 1.0, 1.0, float(np.sqrt(alpha)), 0.5]


def table_weights(table, alpha, n, l, used, mode="linear"):
    """f_table(n, v, l) (n.l) / (p_s(l) + p_d(l)) [M, Q^2, 3] for normals n [M, 3] (n.z > 0) and directions l [M, Q^2, 3], v = +z; 0 where
    not `used` [M, Q^2] or n.l <= 0.  p_s = G1(v) D(h) / (4 n.v) at h = normalize(v + l), p_d = n.l / pi (merl_ref.sample_radiance's)."""
    v = np.array([0.0, 0.0, 1.0])
    nn = np.asarray(n, dtype=np.float64)[:, None, :]
    cv = nn[..., 2]
    cl = np.sum(nn * l, axis=-1)
    h = l + v
    h = h / np.sqrt(np.sum(h * h, axis=-1))[..., None]
    use = used & (cl > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = rr.ggx_g1(alpha, cv, h[..., 2]) * rr.ggx_d(alpha, np.sum(nn * h, axis=-1)) / (4 * cv)
        f = mr.lookup(table, np.broadcast_to(nn, l.shape), np.broadcast_to(v, l.shape), np.where(use[..., None], l, v), mode)
        w = np.where(use, cl / (ps + cl / PI), 0.0)
    return f * w[..., None]


def trace(positions, normals, faces, table, alpha, Rot, H, W, S, Q, shadows=True, mode="linear"):
    """shadow_ref.trace of one row under `table` with proxy roughness alpha: everything that does not depend on the environment"""
    tr = sr.trace(positions, normals, faces, proxy_row(alpha), Rot, H, W, S, Q, shadows)
    n = tr["normal"][tr["lit"]]
    tr["w_spec"] = table_weights(table, alpha, n, tr["l_spec"], tr["traced_spec"], mode)
    tr["w_diff"] = table_weights(table, alpha, n, tr["l_diff"], np.ones(tr["traced_spec"].shape, dtype=bool), mode)
    return tr


def shade(tr, env):
    """shadow_ref.shade: image [3, H, W], slack [3, H, W], unsafe_pixel [H, W]"""
    return sr.shade(tr, env)


def render(positions, normals, faces, table, alpha, env, Rot, H, W, S, Q, shadows=True, mode="linear"):
    """drm_render_mesh_tables for one row: shade(trace(...)) with the trace added under "trace" """
    tr = trace(positions, normals, faces, table, alpha, Rot, H, W, S, Q, shadows, mode)
    out = shade(tr, env)
    out["trace"] = tr
    return out

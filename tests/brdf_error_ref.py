"""float64 numpy restatement of the BRDF-space error sums (drmnet_amd/csrc/brdf_error.hip, drmnet_amd/reflectance.py), written from their
definition on merl_ref.export.  It takes nothing from drmnet_amd.  Used by tests/test_brdf_error_cpu.py and tests/test_gpu_brdf_error.py;
nothing here touches a GPU.

A candidate row a and a target b (a table [3, 90, 90, 180], or a row) are compared on the nodes (i, j, k) of the MERL grid (or the sub-grid of
the index lists).  A node counts where both cosines n.wo and n.wi are strictly positive after the 1e-12 snap and no channel of the target
entry is negative.  The candidate's value is the table entry of the row as float32 (what the export stores), a principled target's the same;
ci = n.wi; the three channels are pooled and every counting node weighs one.  The nine sums, in order:
n, n_log (a > 0 and b > 0), sum d and sum d^2 of d = log10 a - log10 b over those, sum (log1p(a ci) - log1p(b ci))^2, sum ((a - b) ci)^2,
sum (a ci)^2, sum (a ci)(b ci), sum (b ci)^2."""
import numpy as np

import merl_ref as mr


def grid(i=None, j=None, k=None):
    """(ci, lit) of the (sub-)grid: n.wi with the snap applied, and where both cosines are strictly positive"""
    i, j, k = np.meshgrid(*(np.arange(full) if sub is None else np.asarray(sub) for sub, full in ((i, mr.NH), (j, mr.ND), (k, mr.NP))), indexing="ij")
    t = i / 90.0
    th, td, pd = t * t * (np.pi / 2), j * (np.pi / 180), k * (np.pi / 180)
    n = np.stack([-np.sin(th), np.zeros_like(th), np.cos(th)], axis=-1)
    wo = np.stack([np.sin(td) * np.cos(pd), np.sin(td) * np.sin(pd), np.cos(td)], axis=-1)
    wi = wo * np.array([-1.0, -1.0, 1.0])
    co, ci = np.sum(n * wo, -1), np.sum(n * wi, -1)
    co, ci = np.where(np.abs(co) < mr.SNAP, 0.0, co), np.where(np.abs(ci) < mr.SNAP, 0.0, ci)
    return ci, (co > 0) & (ci > 0)


def values(z, i=None, j=None, k=None):
    """the table of the canonical row z as the export stores it: float32 values, held as float64 [3, ...]; the row itself as float32 holds it"""
    row = np.asarray(z, dtype=np.float32).astype(np.float64)
    return mr.export(list(row), i, j, k).astype(np.float32).astype(np.float64)


def error_sums(a, b, i=None, j=None, k=None):
    """a: a canonical row [6] or its values(); b: a table [3, ...] on the same (sub-)grid, or a row -> float64 [9]"""
    a = values(a, i, j, k) if np.ndim(a) == 1 else np.asarray(a, dtype=np.float64)
    b = values(b, i, j, k) if np.ndim(b) == 1 else np.asarray(b, dtype=np.float64)
    ci, lit = grid(i, j, k)
    counts = lit & (b >= 0).all(axis=0)
    a, b, ci = a[:, counts], b[:, counts], ci[counts][None]
    both = (a > 0) & (b > 0)
    d = np.log10(a[both]) - np.log10(b[both])
    l = np.log1p(a * ci) - np.log1p(b * ci)
    return np.array([a.size, both.sum(), d.sum(), (d * d).sum(), (l * l).sum(), (((a - b) * ci) ** 2).sum(), ((a * ci) ** 2).sum(),
                     (a * ci * b * ci).sum(), ((b * ci) ** 2).sum()], dtype=np.float64)


def errors(s):
    """the figures from the sums [9]; a zero denominator gives 0"""
    s = np.asarray(s, dtype=np.float64)
    div = lambda x, y: x / y if y > 0 else 0.0
    mean = div(s[2], s[1])
    return {"n": int(s[0]), "n_log": int(s[1]), "rmse_log10": np.sqrt(div(s[3], s[1])), "mean_log10": mean,
            "rmse_log10_scaled": np.sqrt(max(div(s[3], s[1]) - mean * mean, 0.0)), "rmse_log1p": np.sqrt(div(s[4], s[0])),
            "rel_l2": np.sqrt(div(s[5], s[8])), "scale": div(s[7], s[6]),
            "rel_l2_scaled": np.sqrt(div(max(s[8] - div(s[7] * s[7], s[6]), 0.0), s[8]))}


def objective(z, b, name="log1p", i=None, j=None, k=None):
    """the fit's objective of the row z against the target b: rmse_log1p or rel_l2"""
    return float(errors(error_sums(z, b, i, j, k))[{"log1p": "rmse_log1p", "l2": "rel_l2"}[name]])

"""The true reflectance: how far a principled BRDF is from a target BRDF, and the principled row closest to a measured one.

``estimate`` answers with the six principled parameters ``zK``.  With the row a scene was synthesized with, or the measured table it was lit
under, ``brdf_errors`` says how far the estimate is from it, and ``fit_principled`` finds the best principled row for a table: the floor no
estimate can go below.  Both stand on csrc/brdf_error.hip (``drm_brdf_error_sums``), which scores up to 4096 candidate rows against one target
in one pass over the MERL grid (drmnet_amd/merl.py) and returns nine fp64 sums per row; the figures are formed from the sums on the host in
float64.  The search (``halton``, ``pattern_search``) is host numpy, deterministic, and knows nothing of BRDFs.

Conventions.  A node of the grid counts where the export stores a BRDF value (both cosines strictly positive) and the target has a
measurement there; every counting node weighs one -- the usual MERL-sample convention, no solid-angle weighting -- and the three channels are
pooled.  a is the candidate's value, b the target's, ci = n.wi.

Out of scope: table-against-table errors (the kernel's candidates are rows), anisotropic tables, gradient-based fitting.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple

import numpy as np

# the sums of drm_brdf_error_sums, in the order of include/drmnet_hip.h (DRM_BRDF_ERROR_*)
N, N_LOG, D, DD, LOG1P, L2, AA, AB, BB = range(9)
SUMS = 9
MAX_ROWS = 4096
OBJECTIVES = {"log1p": "rmse_log1p", "l2": "rel_l2"}
HALTON_BASES = (2, 3, 5, 7, 11, 13)


def _rows(rows) -> np.ndarray:
    """[C, 6] canonical rows as float32 (a PrincipledBSDF or one row gives C = 1), clipped to [0, 1] as get_bsdf clips"""
    row = getattr(rows, "row", rows)
    r = np.asarray(row, dtype=np.float64)
    if r.ndim == 1:
        r = r[None]
    if r.ndim != 2 or r.shape[1] != 6 or r.shape[0] < 1 or not np.isfinite(r).all():
        raise ValueError(f"rows must be finite canonical rows [C, 6] or a PrincipledBSDF, got shape {r.shape}")
    return np.ascontiguousarray(np.clip(r, 0.0, 1.0), dtype=np.float32)


def brdf_error_sums(rows, target) -> np.ndarray:
    """drm_brdf_error_sums: ``rows`` [C, 6] canonical (or a PrincipledBSDF) against ``target`` -- a merl.MeasuredBSDF, a [3, 90, 90, 180]
    array (load_merl's layout; negative = no measurement), or a PrincipledBSDF / canonical row [6] -> float64 [C, 9], the sums N, N_LOG, D,
    DD, LOG1P, L2, AA, AB, BB of this module.  More than 4096 rows go in several launches; a row's sums do not depend on its company."""
    import torch

    from . import _lib
    from .merl import SHAPE, MeasuredBSDF
    from .render import _device

    z = _rows(rows)
    dev = _device()
    table = zt = None
    if isinstance(target, MeasuredBSDF):
        table = target.device_table(dev)
    elif hasattr(target, "row") or np.ndim(target) == 1:
        t = _rows(target)
        if t.shape[0] != 1:
            raise ValueError("a principled target is one row")
        zt = torch.from_numpy(t).to(dev)
    elif np.shape(target) == SHAPE:
        table = MeasuredBSDF(target, alpha=1.0).device_table(dev)
    else:
        raise ValueError(f"target must be a MeasuredBSDF, a table {SHAPE}, a PrincipledBSDF or a row [6], got shape {np.shape(target)}")
    out = np.empty((z.shape[0], SUMS), dtype=np.float64)
    with torch.cuda.device(dev):
        for at in range(0, z.shape[0], MAX_ROWS):
            zc = torch.from_numpy(z[at:at + MAX_ROWS]).to(dev)
            C = int(zc.shape[0])
            nbytes = _lib.brdf_error_workspace_bytes(C)
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            sums = torch.empty((C, SUMS), dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().drm_brdf_error_sums(zc.data_ptr(), C, _lib.ptr(table), _lib.ptr(zt), ws.data_ptr(), nbytes, sums.data_ptr(),
                                                      _lib.stream_ptr(dev)))
            out[at:at + C] = sums.cpu().numpy()
    return out


def errors_from_sums(sums) -> Dict[str, float]:
    """One row of sums [9] -> the figures, named like relight.image_errors; a zero denominator gives 0.
      n, n_log           channel values counted; those with a > 0 and b > 0
      rmse_log10         root mean square of d = log10 a - log10 b over the n_log values
      mean_log10         mean of d: the log of the scale between the two
      rmse_log10_scaled  its spread about the mean: illumination and albedo share a scale ambiguity, so this is the fair figure for an estimate
      rmse_log1p         root mean square of log1p(a ci) - log1p(b ci) over all n
      rel_l2             |(a - b) ci| / |b ci|
      scale              <a ci, b ci> / <a ci, a ci>, the factor that brings a closest to b
      rel_l2_scaled      |scale a ci - b ci| / |b ci|"""
    s = np.asarray(sums, dtype=np.float64)
    if s.shape != (SUMS,):
        raise ValueError(f"sums must be [{SUMS}], got {s.shape}")

    def div(a, b):
        return float(a / b) if b > 0 else 0.0

    mean = div(s[D], s[N_LOG])
    return {"n": int(s[N]), "n_log": int(s[N_LOG]),
            "rmse_log10": float(np.sqrt(div(s[DD], s[N_LOG]))),
            "mean_log10": mean,
            "rmse_log10_scaled": float(np.sqrt(max(div(s[DD], s[N_LOG]) - mean * mean, 0.0))),
            "rmse_log1p": float(np.sqrt(div(s[LOG1P], s[N]))),
            "rel_l2": float(np.sqrt(div(s[L2], s[BB]))),
            "scale": div(s[AB], s[AA]),
            "rel_l2_scaled": float(np.sqrt(div(max(s[BB] - div(s[AB] * s[AB], s[AA]), 0.0), s[BB])))}


def brdf_errors(a, target) -> Dict[str, float]:
    """How far the principled BRDF ``a`` (a PrincipledBSDF or a canonical row [6]) is from ``target`` (as brdf_error_sums takes it): the
    figures of errors_from_sums, from one launch."""
    z = _rows(a)
    if z.shape[0] != 1:
        raise ValueError("brdf_errors compares one row; brdf_error_sums takes many")
    return errors_from_sums(brdf_error_sums(z, target)[0])


def halton(n: int, dims: int = 6) -> np.ndarray:
    """The first n points of the Halton sequence in ``dims`` <= 6 dimensions (bases 2, 3, 5, 7, 11, 13), index from 1 -> float64 [n, dims],
    every value in (0, 1)."""
    if not 1 <= dims <= len(HALTON_BASES) or n < 0:
        raise ValueError(f"halton: 1 <= dims <= {len(HALTON_BASES)} and n >= 0")
    out = np.zeros((n, dims), dtype=np.float64)
    for d, base in enumerate(HALTON_BASES[:dims]):
        idx = np.arange(1, n + 1, dtype=np.int64)
        f = 1.0
        while idx.any():
            f /= base
            out[:, d] += f * (idx % base)
            idx //= base
    return out


class SearchResult(NamedTuple):
    x: np.ndarray        # the best point [6]
    objective: float
    rounds: int          # search rounds (evaluate calls after the survey)
    evaluations: int     # candidates evaluated, survey included


def pattern_search(evaluate: Callable[[np.ndarray], np.ndarray], starts, *, keep: int = 8, step0: float = 1 / 8, step_min: float = 2 ** -12,
                   max_rounds: int = 400, survey_batch: int = 1024) -> SearchResult:
    """Minimise ``evaluate`` over the box [0, 1]^d by a compass search from the best of ``starts`` [S, d].  ``evaluate(candidates [M, d]) ->
    objective [M]``.  Deterministic: the same calls in the same order every time.
      survey   ``starts`` are evaluated in batches of at most ``survey_batch`` and the ``keep`` best kept (ties: the lower index).
      round    every kept point p that has not retired, with its own step h_p, offers its 2 d axis neighbours clip(p +- h_p e_i, 0, 1)
               (+ before -, i ascending) and then the pattern move clip(2 p - p_prev, 0, 1); all points' candidates go in ONE evaluate call.
               A point moves to its best candidate if that is strictly better than where it stands (ties: the lowest candidate index) and
               remembers where it came from; otherwise h_p halves and the pattern is forgotten.  A point whose h_p < step_min retires.
    The search ends when every point has retired or after ``max_rounds`` rounds; the best point (ties: the lower index) is returned."""
    starts = np.asarray(starts, dtype=np.float64)
    if starts.ndim != 2 or starts.shape[0] < 1:
        raise ValueError(f"starts must be [S >= 1, d], got {starts.shape}")
    d = starts.shape[1]
    vals = np.concatenate([np.asarray(evaluate(starts[at:at + survey_batch]), dtype=np.float64).reshape(-1)
                           for at in range(0, starts.shape[0], survey_batch)])
    if vals.shape != (starts.shape[0],):
        raise ValueError("evaluate must return one objective per candidate")
    evaluations = int(starts.shape[0])
    order = np.argsort(vals, kind="stable")[:max(1, int(keep))]
    pts, f = starts[order].copy(), vals[order].copy()
    prev = pts.copy()
    h = np.full(len(pts), float(step0))
    eye = np.eye(d)
    rounds = 0
    while rounds < max_rounds:
        live = np.flatnonzero(h >= step_min)
        if live.size == 0:
            break
        cands = []
        for q in live:
            for i in range(d):
                cands.append(np.clip(pts[q] + h[q] * eye[i], 0.0, 1.0))
                cands.append(np.clip(pts[q] - h[q] * eye[i], 0.0, 1.0))
            cands.append(np.clip(2.0 * pts[q] - prev[q], 0.0, 1.0))
        got = np.asarray(evaluate(np.stack(cands)), dtype=np.float64).reshape(len(live), 2 * d + 1)
        rounds += 1
        evaluations += got.size
        for row, q in enumerate(live):
            best = int(np.argmin(got[row]))  # (the first of equal minima)
            if got[row, best] < f[q]:
                prev[q] = pts[q]
                pts[q] = cands[row * (2 * d + 1) + best]
                f[q] = got[row, best]
            else:
                prev[q] = pts[q]
                h[q] *= 0.5
    best = int(np.argmin(f))
    return SearchResult(pts[best].copy(), float(f[best]), rounds, evaluations)


def fit_principled(target, *, objective: str = "log1p", starts: int = 4096, keep: int = 8, step0: float = 1 / 8, step_min: float = 2 ** -12,
                   max_rounds: int = 400) -> dict:
    """The principled row closest to ``target`` (a merl.MeasuredBSDF or a table [3, 90, 90, 180]; a principled target is allowed too):
    pattern_search over halton(starts) with every batch of candidates scored by one drm_brdf_error_sums launch ->
    {"z": the canonical row (six floats, as float32 holds them: what was scored), "errors": brdf_errors of it, "objective": its objective,
    "rounds", "evaluations"}.

    ``objective``: "log1p" (rmse_log1p, the default: relative where the BRDF is large, absolute where it is small) or "l2" (rel_l2, ruled by
    the peak).  Both count every valid entry.  rmse_log10 is deliberately not offered: it runs over the n_log entries where candidate and
    target are both positive, a set that varies with the candidate -- a row whose lobe is cut off to 0 almost everywhere would be scored on a
    handful of entries and win.

    The parameters are identified only up to what the BRDF depends on: ``specular`` is inert at metallic = 1 (and the base colour of a
    channel whose every term it scales by 0), so rows that differ there are the same answer."""
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {sorted(OBJECTIVES)}, got {objective!r}")
    from .merl import SHAPE, MeasuredBSDF

    if not isinstance(target, MeasuredBSDF) and np.shape(target) == SHAPE:
        target = MeasuredBSDF(target, alpha=1.0)  # (packed and uploaded once for the whole search)

    def evaluate(cands: np.ndarray) -> np.ndarray:
        s = brdf_error_sums(cands, target)
        with np.errstate(divide="ignore", invalid="ignore"):
            if objective == "log1p":
                v = np.sqrt(s[:, LOG1P] / s[:, N])
            else:
                v = np.sqrt(s[:, L2] / s[:, BB])
        return np.where(np.isfinite(v), v, 0.0)  # (a zero denominator gives 0, as errors_from_sums)

    res = pattern_search(evaluate, halton(int(starts)), keep=keep, step0=step0, step_min=step_min, max_rounds=max_rounds)
    z = [float(v) for v in np.asarray(res.x, dtype=np.float32)]
    errors = brdf_errors(z, target)
    return {"z": z, "errors": errors, "objective": errors[OBJECTIVES[objective]], "rounds": res.rounds, "evaluations": res.evaluations}

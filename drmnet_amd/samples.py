"""N draws of one image, judged: which explains the image best, which lies closest to all the others, and how far they spread.

``estimate.estimate_samples`` draws N (illumination, reflectance) pairs of one object image; this module ranks them.  Every comparison
runs on the batched image-error kernel (csrc/image_error.hip through ``relight.image_errors_batch``): ``rerender_errors`` is one warp, one
render and one launch of N pairs; ``pairwise_distances`` one launch of N^2 pairs (N <= 64).  ``sample_statistics`` is plumbing (torch ops).
``rank`` and ``write_samples`` are what ``estimate --num_samples N`` calls.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .estimate import MAX_SAMPLES  # N^2 pairs in one launch of at most 4096


@torch.no_grad()
def rerender_errors(DRMNet_model, Lr0: torch.Tensor, zK: torch.Tensor, input_img: torch.Tensor, input_normal: torch.Tensor, mask) -> List[Dict[str, float]]:
    """Every draw shaded back onto the input's normal map and compared with the input image on ``mask``: Lr0 [N, 3, S, S], zK [N, P],
    input_img / input_normal [H, W, 3], mask [H, W] -> N dicts of ``relight.image_errors_batch``.  One r0toenvmap over the batch, one
    render_normals call (one normal map shaded N ways), one image-error call (N channel-first renders against the one channel-last input)."""
    from .relight import image_errors_batch, render_normals

    envmaps = DRMNet_model.r0toenvmap(Lr0, (DRMNet_model.image_size, DRMNet_model.image_size * 2))
    images, _ = render_normals(input_normal, zK, DRMNet_model.brdf_param_names, envmaps, mask=mask)
    return image_errors_batch(images, input_img, mask)


@torch.no_grad()
def pairwise_distances(Lr0: torch.Tensor) -> np.ndarray:
    """D [N, N] float64, D[i, j] = ``rel_l2_scaled`` of draw i's mirror map against draw j's over every texel (i brought to j's scale: the
    draws share the scale ambiguity, so this is the distance between their shapes; not symmetric).  Lr0 [N, 3, S, S] on the GPU, N <= 64:
    one launch of N^2 pairs.  The diagonal is exactly 0."""
    from .relight import IMAGE_SUM_NAMES, image_error_sums

    if not isinstance(Lr0, torch.Tensor) or Lr0.dim() != 4 or Lr0.shape[1] != 3:
        raise ValueError(f"pairwise_distances: Lr0 must be [N, 3, S, S], got {tuple(getattr(Lr0, 'shape', ()))}")
    N = int(Lr0.shape[0])
    if not 1 <= N <= MAX_SAMPLES:
        raise ValueError(f"pairwise_distances: N = {N} draws in [1, {MAX_SAMPLES}] (N^2 pairs in one launch)")
    i, j = np.divmod(np.arange(N * N), N)
    sums = image_error_sums(Lr0, Lr0, torch.ones(Lr0.shape[2:], dtype=torch.uint8), pairs=np.stack([i, j, np.zeros_like(i)], axis=1))
    s = sums.cpu().numpy()
    nb, d = np.sqrt(s[:, IMAGE_SUM_NAMES.index("bb")]), np.sqrt(s[:, IMAGE_SUM_NAMES.index("l2_scaled")])
    with np.errstate(divide="ignore", invalid="ignore"):  # errors_from_image_sums' rel_l2_scaled, 4096 rows at once
        return np.where(nb > 0, d / nb, np.where(d == 0, 0.0, np.inf)).reshape(N, N)


def _candidates(who: str, N: int, finite) -> np.ndarray:
    """the draws a choice is made among: those ``finite`` marks (bool [N]; None: all), or all of them where it marks none"""
    if finite is None:
        return np.ones(N, dtype=bool)
    ok = np.asarray(finite, dtype=bool)
    if ok.shape != (N,):
        raise ValueError(f"{who}: finite must be [N = {N}] booleans, got {ok.shape}")
    return ok if ok.any() else np.ones(N, dtype=bool)


def medoid(D, finite=None) -> int:
    """the draw closest to all the others: the argmin of D's row sums; ties go to the lowest index, a row with a NaN counts as infinitely
    far.  ``finite`` (bool [N], ``finite_draws``) leaves the draws it does not mark out of the rows and of the sums."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError(f"medoid: D must be [N, N] with N >= 1, got {D.shape}")
    ok = _candidates("medoid", D.shape[0], finite)
    among = np.flatnonzero(ok)
    total = D[np.ix_(among, among)].sum(axis=1)
    return int(among[np.argmin(np.where(np.isnan(total), np.inf, total))])


def finite_draws(Lr0: torch.Tensor, zK: torch.Tensor) -> List[bool]:
    """which draws are estimates at all: every texel of the mirror map and every BRDF parameter finite.  A row of NaN parameters shades
    to a black image, whose ``rel_l2`` of exactly 1 would beat every draw that is merely far off."""
    return (torch.isfinite(Lr0).flatten(1).all(dim=1) & torch.isfinite(zK).flatten(1).all(dim=1)).cpu().tolist()


def select(kind: str, *, errors: Optional[Sequence[Dict[str, float]]] = None, distances=None, finite=None) -> int:
    """The index of the draw to keep.  "rerender": the lowest ``rel_l2`` of ``errors`` (``rerender_errors``): the re-render is to equal the
    input absolutely, there is no scale ambiguity in image space; ties go to the lowest index and a NaN is never chosen over a number.
    "medoid": ``medoid(distances, finite)``.  "first": the first candidate.  ``finite`` (bool [N], ``finite_draws``): a draw it does
    not mark is never chosen while it marks another."""
    if kind == "rerender":
        if not errors:
            raise ValueError("select('rerender') needs the draws' re-render errors")
        rel = np.array([e["rel_l2"] for e in errors], dtype=np.float64)
        among = np.flatnonzero(_candidates("select", len(rel), finite))
        return int(among[np.argmin(np.where(np.isnan(rel), np.inf, rel)[among])])
    if kind == "medoid":
        if distances is None:
            raise ValueError("select('medoid') needs the pairwise distances")
        return medoid(distances, finite)
    if kind == "first":
        return 0 if finite is None else int(np.argmax(_candidates("select", len(np.asarray(finite)), finite)))
    raise ValueError(f"select: kind must be 'rerender', 'medoid' or 'first', got {kind!r}")


@torch.no_grad()
def sample_statistics(Lr0: torch.Tensor, zK: torch.Tensor) -> Dict[str, torch.Tensor]:
    """per-texel mean and standard deviation of the mirror maps over the draws, and the same of the BRDF parameters (the divisor is N: one
    draw has the spread 0): Lr0 [N, 3, S, S], zK [N, P] -> {"Lr0_mean", "Lr0_std" [3, S, S], "zK_mean", "zK_std" [P]}"""
    return {"Lr0_mean": Lr0.mean(dim=0), "Lr0_std": Lr0.std(dim=0, unbiased=False), "zK_mean": zK.mean(dim=0), "zK_std": zK.std(dim=0, unbiased=False)}


def rank(DRMNet_model, Lr0, zK, K, input_img, input_normal, mask, kind: str) -> dict:
    """everything ``estimate --num_samples`` reports of the draws but the counts: the re-render errors, the pairwise matrix, which draws
    are finite (``finite_draws``), and among those the medoid and the draw ``kind`` selects"""
    errors = rerender_errors(DRMNet_model, Lr0, zK, input_img, input_normal, mask)
    D = pairwise_distances(Lr0)
    finite = finite_draws(Lr0, zK)
    return {"select": kind, "selected": select(kind, errors=errors, distances=D, finite=finite), "medoid": medoid(D, finite), "finite": finite,
            "zK": zK.cpu().tolist(), "K": K.cpu().tolist(), "rerender_errors": errors, "pairwise_rel_l2_scaled": D.tolist()}


def write_samples(output_dir: Path, DRMNet_model, Lr0: torch.Tensor, zK: torch.Tensor, report: dict) -> None:
    """What ``--num_samples N > 1`` adds: samples.json (num_samples, seed, select, selected, per-draw zK, K and re-render errors, the
    pairwise matrix, the medoid, which draws are finite, the mean and standard deviation of zK over those); samples_Lr0.npy [N, 3, S, S]; sample_mean_env.png, the mean mirror
    map through r0toenvmap and hdr2ldr; sample_std.exr, the per-texel standard deviation of the mirror maps [S, S, 3]."""
    from . import file_io
    from .transform import hdr2ldr

    output_dir = Path(output_dir)
    keep = torch.tensor(report["finite"], dtype=torch.bool, device=Lr0.device)
    keep = keep if bool(keep.any()) else ~keep  # the statistics run over the finite draws (report["finite"]), over all where there is none
    stats = sample_statistics(Lr0[keep], zK[keep])
    keys = ("num_samples", "seed", "select", "selected", "medoid", "finite", "zK", "K", "rerender_errors", "pairwise_rel_l2_scaled")
    out = dict({k: report[k] for k in keys}, zK_mean=stats["zK_mean"].cpu().tolist(), zK_std=stats["zK_std"].cpu().tolist())
    (output_dir / "samples.json").write_text(json.dumps(out, indent=1) + "\n")
    np.save(output_dir / "samples_Lr0.npy", Lr0.cpu().numpy())
    mean_env = DRMNet_model.r0toenvmap(stats["Lr0_mean"][None], (DRMNet_model.image_size, DRMNet_model.image_size * 2))[0]
    file_io.save_png(output_dir / "sample_mean_env.png", hdr2ldr(mean_env.cpu().numpy()))
    file_io.save_exr(output_dir / "sample_std.exr", stats["Lr0_std"].permute(1, 2, 0).contiguous())

"""Single-image inverse rendering, the reference's scripts/estimate.py on the MI355X path.

    python -m drmnet_amd.estimate --input_img data/sample/image.exr --input_normal data/sample/normal.npy \\
        --input_mask data/sample/mask.png [--obsnet_base_path configs/obsnet/eval_obsnet.yaml] [--drmnet_base_path ...]

`estimate()` keeps the reference's signature and statement order (scripts/estimate.py:29-107); every stage runs on the GPU:
mask erosion + refmap_mask_make (csrc/refmap.hip), ObsNet DDIM inpainting and the DRMNet reverse loop (device loops behind
the C ABI).  The keyword-only `hooks` let tests inject the random draws the reference takes from torch's global generator.
`main` writes the reference's two images (sample_env.png, and sample_brdf.png through visualize_bsdf on csrc/render.hip) and also saves
and prints the BRDF parameters.  With `--rerender` (off by default) it also shades the estimate back onto the input's normal map
(drmnet_amd/relight.py) and reports how far that image, and the image ObsNet's inpainted reflectance map stands for, are from the input:
sample_rerender.exr / .png, sample_refmap_image.exr, sample_errors.json.  With `--save_merl` (off by default) it also writes
sample_brdf.binary, the estimated BRDF as a MERL table (drmnet_amd/merl.py).  With `--gt_envmap E.exr --gt_view_from x y z` (a pair, off by
default: the `--envmap` and `--view_from` `synthesize` was given) it also judges the estimated illumination against the true one
(drmnet_amd/groundtruth.py): sample_gt_mirmap.exr, the mirror reflectance map Lr0 should equal; sample_gt_env.exr, the true map in the
camera frame the estimated map is in; sample_Lr0.exr; and sample_gt_errors.json.  With `--gt_z m R G B r s` (the `--z` `synthesize` rendered
with) or `--gt_merl M.binary` (the table `relight --merl` rendered under; the two exclude each other) it also judges the estimated BRDF in
BRDF space (drmnet_amd/reflectance.py): sample_gt_errors.json gains "brdf", and under a measured truth "brdf_fit", the best principled fit of
the table, the floor the estimate is to be read against.
DRMNet is stochastic: `estimate_samples` draws N estimates of one image in one batch (the reflectance-map gather once, one DDIM run and
one DRMNet loop at batch N), and with `--num_samples N` (1 ... 64, default 1: the path and the files above, unchanged) `--select
rerender|medoid|first` (default rerender) names the draw that becomes the estimate every other file is written from, `--seed S` fixes the
draws, and samples.json (per-draw zK, K and re-render errors, the pairwise matrix, the medoid), samples_Lr0.npy, sample_mean_env.png and
sample_std.exr are added (drmnet_amd/samples.py, on the batched image-error kernel csrc/image_error.hip).
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .img2refmap import erode_mask, refmap_mask_make


@torch.no_grad()
def estimate(DRMNet_model, ObsNet_model, input_img: torch.Tensor, input_normal: torch.Tensor, mask: torch.Tensor, tag: str = "sample",
             erode_kernel_size: int = 5, *, hooks: Optional[dict] = None):
    hooks = hooks or {}
    refmap_res = DRMNet_model.ds.size
    # edge removing (estimate.py:43-50)
    if erode_kernel_size > 0:
        mask = erode_mask(mask, erode_kernel_size)
    # Making refmap from object image (estimate.py:52-58)
    refmap_est, refmask = refmap_mask_make(input_img[mask], input_normal[mask], res=refmap_res, angle_threshold=np.pi / 128 / 2)  # (hard-coded in the reference too: scripts/estimate.py:57)
    # Inpainting refmap (estimate.py:63-81)
    batch = {"tag": [tag], "raw_refmap": refmap_est.permute(2, 0, 1)[None], "raw_refmask": refmask[None]}
    c, _, _ = ObsNet_model.get_cond_for_predict(batch, noise=hooks.get("cond_noise"))
    use_ddim = ObsNet_model.ddim_steps is not None
    extra = {k: hooks[k] for k in ("x_T", "noise") if k in hooks}
    with ObsNet_model.ema_scope("Plotting"):
        samples, _ = ObsNet_model.sample_log(cond=c, batch_size=len(batch["tag"]), ddim=use_ddim, ddim_steps=ObsNet_model.ddim_steps,
                                             eta=ObsNet_model.ddim_eta, **extra)
    inpaint_sample = ObsNet_model.ds.rescale(ObsNet_model.decode_first_stage(samples))[0]
    # Inverse Rendering (estimate.py:86-104)
    batch = {"tag": [tag], "LrK": inpaint_sample[None]}
    LrK, _, illnet_c, refnet_c, _ = DRMNet_model.get_input_for_predict(batch)
    loop_extra = {k: hooks[k] for k in ("noise0", "step_noise") if k in hooks}
    with DRMNet_model.ema_scope():
        samples, zK_est, _ = DRMNet_model.p_sample_loop(LrK, illnet_c, refnet_c, verbose=False, **loop_extra)
    Lr0_sample = DRMNet_model.ds.rescale(DRMNet_model.decode_first_stage(samples))[0].clip(0)
    zK_est = zK_est[0]
    if DRMNet_model.refmap_input_scaler is not None:
        Lr0_sample = Lr0_sample / DRMNet_model.normalizing_scale[0]
    if "stages" in hooks:  # tests look at the intermediate products
        hooks["stages"].update(mask=mask, refmap=refmap_est, refmask=refmask, cond=c, inpaint=inpaint_sample, LrK=LrK)
    return Lr0_sample, zK_est


@torch.no_grad()
def estimate_batch(DRMNet_model, ObsNet_model, input_imgs: torch.Tensor, input_normals: torch.Tensor, masks: torch.Tensor,
                   erode_kernel_size: int = 5, *, early_exit: bool = True, seed: Optional[int] = None, hooks: Optional[dict] = None):
    """`estimate` for B object images at once (BASELINE configs[4]: the chain batched the way the samplers like it):
    per-object erosion + refmap gather, then ONE ObsNet DDIM run and ONE DRMNet loop over the whole batch.
    input_imgs / input_normals [B, H, W, 3], masks [B, H, W] bool  ->  (Lr0 [B, 3, res, res], zK [B, z_dim], K [B]).
    `hooks` injects the random draws as in `estimate` (batched along dim 0 / dim 1 of the per-step tensors)."""
    hooks = hooks or {}
    refmap_res = DRMNet_model.ds.size
    refmaps, refmasks = [], []
    timer = _StageTimer(hooks)
    timer.mark("start")
    for img, nrm, mask in zip(input_imgs, input_normals, masks):
        if erode_kernel_size > 0:
            mask = erode_mask(mask, erode_kernel_size)
        rm, mk = refmap_mask_make(img[mask], nrm[mask], res=refmap_res, angle_threshold=np.pi / 128 / 2)  # (scripts/estimate.py:57)
        refmaps.append(rm.permute(2, 0, 1))
        refmasks.append(mk)
    timer.mark("refmap_gather")
    return _chain_rows(DRMNet_model, ObsNet_model, refmaps, refmasks, hooks.get("cond_noise"), early_exit, seed, hooks, timer)


class _StageTimer:
    """hooks["timing"]: per-stage device time (ms) of one call, measured with events on the current stream and added to what is there"""

    def __init__(self, hooks: dict):
        self.hooks, self.marks = hooks, []

    def mark(self, name: str) -> None:
        if "timing" in self.hooks:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    def finish(self) -> None:
        if self.marks:
            self.marks[-1][1].synchronize()
            for (_, e0), (name, e1) in zip(self.marks[:-1], self.marks[1:]):
                self.hooks["timing"][name] = self.hooks["timing"].get(name, 0.0) + e0.elapsed_time(e1)


def _chain_rows(DRMNet_model, ObsNet_model, refmaps, refmasks, cond_noise, early_exit: bool, seed: Optional[int], hooks: dict, timer: _StageTimer):
    """What ``estimate_batch`` and ``estimate_samples`` share once every row has its raw reflectance map [3, res, res] and mask: ONE ObsNet
    DDIM run and ONE DRMNet loop over the rows -> (Lr0 [B, 3, res, res], zK [B, z_dim], K [B]).  hooks["stages"], where given, receives
    the batched intermediate products (cond, inpaint, LrK)."""
    B = len(refmaps)
    batch = {"tag": [f"obj{i}" for i in range(B)], "raw_refmap": torch.stack(refmaps), "raw_refmask": torch.stack(refmasks)}
    c, _, _ = ObsNet_model.get_cond_for_predict(batch, noise=cond_noise)
    use_ddim = ObsNet_model.ddim_steps is not None
    extra = {} if seed is None else {"seed": seed}
    obs_extra = {k: hooks[k] for k in ("x_T", "noise") if k in hooks}
    with ObsNet_model.ema_scope("Plotting"):
        samples, _ = ObsNet_model.sample_log(cond=c, batch_size=B, ddim=use_ddim, ddim_steps=ObsNet_model.ddim_steps, eta=ObsNet_model.ddim_eta,
                                             **extra, **obs_extra)
    inpaint = ObsNet_model.ds.rescale(ObsNet_model.decode_first_stage(samples))
    timer.mark("obsnet_sampler")
    LrK, _, illnet_c, refnet_c, _ = DRMNet_model.get_input_for_predict({"tag": batch["tag"], "LrK": inpaint})
    loop_extra = {k: hooks[k] for k in ("noise0", "step_noise") if k in hooks}
    with DRMNet_model.ema_scope():
        samples, zK_est, K = DRMNet_model.p_sample_loop(LrK, illnet_c, refnet_c, verbose=False, early_exit=early_exit, **extra, **loop_extra)
    Lr0 = DRMNet_model.ds.rescale(DRMNet_model.decode_first_stage(samples)).clip(0)
    if DRMNet_model.refmap_input_scaler is not None:
        Lr0 = Lr0 / DRMNet_model.normalizing_scale[:, None, None, None]
    timer.mark("drmnet_loop")
    timer.finish()
    if "stages" in hooks:
        hooks["stages"].update(cond=c, inpaint=inpaint, LrK=LrK)
    return Lr0, zK_est, K


MAX_SAMPLES = 64  # one image's draws are ranked against each other by one launch of N^2 <= 4096 pairs (samples.pairwise_distances)
SELECT_KINDS = ("rerender", "medoid", "first")  # what samples.select chooses by


@torch.no_grad()
def estimate_samples(DRMNet_model, ObsNet_model, input_img: torch.Tensor, input_normal: torch.Tensor, mask: torch.Tensor, num_samples: int,
                     erode_kernel_size: int = 5, *, early_exit: bool = True, seed: Optional[int] = None, hooks: Optional[dict] = None):
    """N draws of ONE object image in one call: DRMNet is stochastic, and what it returns for an image is one of many plausible
    (illumination, reflectance) pairs.  The erosion and the reflectance-map gather run once; the same raw map and mask stand on N batch
    rows, and the rest is ``estimate_batch``'s statement order -- one ObsNet DDIM run and one DRMNet loop at batch N -- so the rows differ
    through the noise alone.  input_img / input_normal [H, W, 3], mask [H, W] bool, 1 <= num_samples <= 64
    -> (Lr0 [N, 3, res, res], zK [N, z_dim], K [N]).
    ``seed``: the samplers get it, and the padding noise of ``get_cond_for_predict`` is ops.randn under seed + 1 (the rule validation_step
    has for its second pass), so a seed fixes every draw; None leaves the draws to the samplers' and torch's generators.  ``hooks`` are
    ``estimate_batch``'s, batched over the N rows (hooks["cond_noise"] stands in for the seeded padding noise)."""
    hooks = hooks or {}
    if isinstance(num_samples, bool) or not 1 <= int(num_samples) <= MAX_SAMPLES:
        raise ValueError(f"estimate_samples: num_samples in [1, {MAX_SAMPLES}], got {num_samples!r}")
    N = int(num_samples)
    timer = _StageTimer(hooks)
    timer.mark("start")
    if erode_kernel_size > 0:
        mask = erode_mask(mask, erode_kernel_size)
    rm, mk = refmap_mask_make(input_img[mask], input_normal[mask], res=DRMNet_model.ds.size, angle_threshold=np.pi / 128 / 2)  # (scripts/estimate.py:57)
    timer.mark("refmap_gather")
    cond_noise = hooks.get("cond_noise")
    if cond_noise is None and seed is not None and ObsNet_model.padding_mode == "noise":
        from . import ops

        cond_noise = ops.randn((N, rm.shape[2], ObsNet_model.image_size, ObsNet_model.image_size), int(seed) + 1, device=rm.device)
    return _chain_rows(DRMNet_model, ObsNet_model, [rm.permute(2, 0, 1)] * N, [mk] * N, cond_noise, early_exit, seed, hooks, timer)


def save_brdf_png(path, zK, brdf_param_names) -> None:
    """scripts/estimate.py:146-148: the estimated BRDF's visualize_bsdf figure, tone-mapped (hdr2ldr), with its sphere mask as alpha."""
    from . import file_io
    from .render import get_bsdf, visualize_bsdf
    from .transform import hdr2ldr

    fig, mask = visualize_bsdf(get_bsdf(zK, brdf_param_names))
    file_io.save_png(path, hdr2ldr(fig), mask=mask)


def parser() -> argparse.ArgumentParser:
    # Provenance: this entry point deliberately mirrors the reference's command line (scripts/estimate.py:105-142: the same options, defaults, mask
    # rule and output files -- SURVEY 2 #20 keeps it as the user-facing surface); everything it calls is this package's own code over the HIP library.
    parser = argparse.ArgumentParser()
    parser.add_argument("--input_img", type=Path, help="The path of HDR image for an object (.exr)")
    parser.add_argument("--input_normal", type=Path, help="The path of normal map for an object (.npy)")
    parser.add_argument("--input_mask", type=Path, help="The path of mask for an object (.png)", default=None)
    parser.add_argument("--obsnet_base_path", type=Path, help="the config path for obsnet", default=Path("./configs/obsnet/eval_obsnet.yaml"))
    parser.add_argument("--drmnet_base_path", type=Path, help="the config path for drmnet", default=Path("./configs/drmnet/eval_drmnet.yaml"))
    parser.add_argument("--output_dir", type=Path, help="the output directory", default=Path("./outputs/"))
    parser.add_argument("--rerender", action="store_true",
                        help="also re-render the estimate on the input's normal map and report how far it is from the input image (default: off)")
    parser.add_argument("--save_merl", action="store_true",
                        help="also write sample_brdf.binary, the estimated BRDF as a MERL table (default: off)")
    parser.add_argument("--gt_envmap", type=Path, default=None,
                        help="the true lat-long environment map (.exr, world frame): also report the estimated illumination's error; needs --gt_view_from")
    parser.add_argument("--gt_view_from", type=float, nargs=3, default=None, metavar=("x", "y", "z"),
                        help="the viewer position the object image was taken from (off the +-y axis); needs --gt_envmap")
    parser.add_argument("--gt_z", type=float, nargs=6, default=None, metavar=("m", "R", "G", "B", "r", "s"),
                        help="the true principled row (metallic, base colour R G B, roughness, specular): also report the estimated BRDF's error")
    parser.add_argument("--gt_merl", type=Path, default=None,
                        help="the true measured BRDF (a MERL .binary): also report the estimated BRDF's error and the best principled fit of the table")
    parser.add_argument("--num_samples", type=int, default=1,
                        help=f"draw N estimates of the image in one batch, in [1, {MAX_SAMPLES}]; N > 1 keeps the draw --select names and adds "
                             "samples.json, samples_Lr0.npy, sample_mean_env.png and sample_std.exr (default: 1)")
    parser.add_argument("--select", choices=SELECT_KINDS, default=None,
                        help="which of the N draws becomes the estimate: the lowest re-render error against the input image, the draw closest to "
                             "all the others, or the first (default: rerender); needs --num_samples > 1")
    parser.add_argument("--seed", type=int, default=None, help="fix the N draws; needs --num_samples > 1")
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    """the command line, with the rules argparse cannot state: --gt_envmap and --gt_view_from come as a pair; --gt_z and --gt_merl exclude
    each other; --num_samples is in [1, 64]; --select and --seed are errors unless --num_samples > 1 (one draw has nothing to choose from, and
    without the flag the draws stay where the reference takes them), and with N > 1 --select defaults to rerender"""
    p = parser()
    args = p.parse_args(argv)
    if not 1 <= args.num_samples <= MAX_SAMPLES:
        p.error(f"--num_samples in [1, {MAX_SAMPLES}], got {args.num_samples}")
    if args.num_samples == 1 and (args.select is not None or args.seed is not None):
        p.error("--select and --seed need --num_samples > 1: a single draw is the reference's, taken as it takes it")
    if args.num_samples > 1 and args.select is None:
        args.select = "rerender"
    if (args.gt_envmap is None) != (args.gt_view_from is None):
        p.error("--gt_envmap and --gt_view_from come as a pair: the true map is in the world frame, the estimate in the camera's")
    if args.gt_z is not None and args.gt_merl is not None:
        p.error("--gt_z and --gt_merl exclude each other: the true reflectance is one principled row or one measured table")
    return args


def save_brdf_merl(path, zK, brdf_param_names) -> None:
    """the estimated BRDF exported as a MERL file (merl.bsdf_to_merl, merl.save_merl): what other tools and BRDF error metrics consume"""
    from .merl import MeasuredBSDF, save_merl
    from .render import get_bsdf

    save_merl(MeasuredBSDF.from_principled(get_bsdf(zK, brdf_param_names), alpha=1.0).table, path)


def write_rerender(output_dir: Path, drmnet_model, Lr0_sample, zK_est, inpaint, input_img, input_normal, mask) -> dict:
    """What ``--rerender`` adds: sample_rerender.exr / .png, the estimate shaded on the input's normal map (relight.rerender);
    sample_refmap_image.exr, ObsNet's inpainted reflectance map read at every pixel's normal (relight.image_from_refmap); and
    sample_errors.json, both against the input image on the un-eroded mask: "estimate" is the whole loop, "inpainted_refmap" what the
    reflectance-map model itself cannot explain (shadows, interreflection, a BRDF that varies), before any estimate is made."""
    import json

    from . import file_io
    from .relight import image_errors, image_from_refmap, rerender, save_image

    image, _ = rerender(drmnet_model, Lr0_sample, zK_est, input_normal, mask)
    save_image(output_dir / "sample_rerender", image[0], mask)
    lookup, _ = image_from_refmap(inpaint, input_normal, mask=mask)
    file_io.save_exr(output_dir / "sample_refmap_image.exr", lookup[0].permute(1, 2, 0))
    errors = {"estimate": image_errors(image[0].permute(1, 2, 0), input_img, mask),
              "inpainted_refmap": image_errors(lookup[0].permute(1, 2, 0), input_img, mask)}
    (output_dir / "sample_errors.json").write_text(json.dumps(errors, indent=1) + "\n")
    return errors


def write_groundtruth(output_dir: Path, Lr0_sample, envmap_est, envmap_gt, view_from) -> dict:
    """What ``--gt_envmap`` adds: sample_gt_mirmap.exr and sample_gt_env.exr, the true illumination as the mirror reflectance map and as
    the camera-frame environment map (groundtruth.gt_mirror_map / gt_camera_envmap); sample_Lr0.exr, the estimated mirror map they are
    compared with (the estimated environment map is sample_env.png's); and sample_gt_errors.json: "mirror_map" and "envmap", each the
    estimate against the truth over every texel (relight.image_errors: the scaled figures allow for the scale ambiguity)."""
    import json

    from . import file_io
    from .groundtruth import illumination_errors

    maps = {}
    errors = illumination_errors(Lr0_sample, envmap_est, envmap_gt, view_from, maps=maps)
    file_io.save_exr(output_dir / "sample_gt_mirmap.exr", maps["mirror_map"].permute(1, 2, 0))
    file_io.save_exr(output_dir / "sample_gt_env.exr", maps["envmap"])
    file_io.save_exr(output_dir / "sample_Lr0.exr", Lr0_sample.permute(1, 2, 0))
    (output_dir / "sample_gt_errors.json").write_text(json.dumps(errors, indent=1) + "\n")
    return errors


def write_groundtruth_brdf(output_dir: Path, zK_est, brdf_param_names, truth, errors: Optional[dict] = None, fit_options: Optional[dict] = None) -> dict:
    """What ``--gt_z`` / ``--gt_merl`` add to sample_gt_errors.json (created when ``--gt_envmap`` did not write it; ``errors`` is what it
    wrote): "brdf" = reflectance.brdf_errors(the estimated row, truth), the scaled figures allowing for the scale ambiguity; and, for a
    measured truth (a merl.MeasuredBSDF), "brdf_fit" = reflectance.fit_principled(truth) with its ``z``: the best any principled row can do,
    the floor the estimate is to be read against.  ``fit_options`` are fit_principled's keywords."""
    import json

    from .merl import MeasuredBSDF
    from .reflectance import brdf_errors, fit_principled
    from .render import get_bsdf

    errors = dict(errors or {})
    errors["brdf"] = brdf_errors(get_bsdf(zK_est, brdf_param_names), truth)
    if isinstance(truth, MeasuredBSDF):
        errors["brdf_fit"] = fit_principled(truth, **(fit_options or {}))
    (output_dir / "sample_gt_errors.json").write_text(json.dumps(errors, indent=1) + "\n")
    return errors


def main(argv=None, *, models=None, hooks: Optional[dict] = None):
    """``models`` = (DRMNet_model, ObsNet_model), already on the GPU with their ``ds``, stands in for the two configs, and ``hooks`` are
    ``estimate``'s: tests run the command line on small networks with injected draws.  hooks["fit"]: keywords for the fit of ``--gt_merl``."""
    from . import file_io
    from .config import instantiate_from_config, load_config
    from .transform import hdr2ldr

    args = parse_args(argv)
    if args.gt_view_from is not None:
        from .render import view_rotation

        view_rotation(args.gt_view_from)  # (a view along +-y is a ValueError here, before any work)

    if models is not None:
        drmnet_model, obsnet_model = models
    else:
        obsnet_base_config = load_config(args.obsnet_base_path)
        obsnet_model = instantiate_from_config(obsnet_base_config["model"]).cuda()
        obsnet_model.ds = instantiate_from_config(obsnet_base_config["data"]["params"]["predict"])
        drmnet_base_config = load_config(args.drmnet_base_path)
        drmnet_model = instantiate_from_config(drmnet_base_config["model"]).cuda()
        drmnet_model.ds = instantiate_from_config(drmnet_base_config["data"]["params"]["predict"])

    input_img = file_io.load_exr(args.input_img, as_torch=True).cuda()
    input_normal = torch.from_numpy(np.load(args.input_normal)).cuda()
    normal_mask = torch.linalg.norm(input_normal, dim=-1) > 0.5
    if args.input_mask is not None:
        input_mask = file_io.load_png(args.input_mask, as_torch=True).cuda()
        if input_mask.ndim == 3:
            input_mask = input_mask[:, :, 0]
        mask = torch.logical_and(input_mask, normal_mask)
    else:
        mask = normal_mask

    hooks = dict(hooks or {})
    if args.rerender:
        hooks.setdefault("stages", {})
    if args.num_samples > 1:
        from . import samples

        draws = estimate_samples(drmnet_model, obsnet_model, input_img, input_normal, mask, args.num_samples, seed=args.seed, hooks=hooks)
        report = samples.rank(drmnet_model, *draws, input_img, input_normal, mask, args.select)
        Lr0_sample, zK_est = draws[0][report["selected"]], draws[1][report["selected"]]
        if args.rerender:
            hooks["stages"]["inpaint"] = hooks["stages"]["inpaint"][report["selected"]]
    else:
        Lr0_sample, zK_est = estimate(drmnet_model, obsnet_model, input_img, input_normal, mask, hooks=hooks)
    envmap_est = drmnet_model.r0toenvmap(Lr0_sample[None], (drmnet_model.image_size, drmnet_model.image_size * 2))[0]  # [H, W, 3]
    args.output_dir.mkdir(exist_ok=True)
    if args.num_samples > 1:
        samples.write_samples(args.output_dir, drmnet_model, draws[0], draws[1], dict(report, num_samples=args.num_samples, seed=args.seed))
        print(f"kept draw {report['selected']} of {args.num_samples} (--select {args.select}; the medoid is draw {report['medoid']})")
    file_io.save_png(args.output_dir / "sample_env.png", hdr2ldr(envmap_est.cpu().numpy()))
    save_brdf_png(args.output_dir / "sample_brdf.png", zK_est, drmnet_model.brdf_param_names)
    np.save(args.output_dir / "sample_brdf.npy", zK_est.cpu().numpy())
    if args.save_merl:
        save_brdf_merl(args.output_dir / "sample_brdf.binary", zK_est, drmnet_model.brdf_param_names)
    print("estimated BRDF parameters", dict(zip(drmnet_model.brdf_param_names, zK_est.tolist())))
    if args.rerender:
        errors = write_rerender(args.output_dir, drmnet_model, Lr0_sample, zK_est, hooks["stages"]["inpaint"], input_img, input_normal, mask)
        print("re-rendered estimate against the input image", errors)
    gt_errors = None
    if args.gt_envmap is not None:
        envmap_gt = file_io.load_exr(args.gt_envmap, as_torch=True).cuda()
        gt_errors = write_groundtruth(args.output_dir, Lr0_sample, envmap_est, envmap_gt, args.gt_view_from)
        print("estimated illumination against the ground truth", gt_errors)
    if args.gt_z is not None or args.gt_merl is not None:
        from .merl import MeasuredBSDF

        truth = np.clip(args.gt_z, 0.0, 1.0) if args.gt_z is not None else MeasuredBSDF.from_file(args.gt_merl, alpha=1.0)
        gt_errors = write_groundtruth_brdf(args.output_dir, zK_est, drmnet_model.brdf_param_names, truth, gt_errors, hooks.get("fit"))
        print("estimated BRDF against the ground truth", {k: gt_errors[k] for k in ("brdf", "brdf_fit") if k in gt_errors})


if __name__ == "__main__":
    main()

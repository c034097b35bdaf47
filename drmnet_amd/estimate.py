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
    marks = []  # hooks["timing"]: per-stage device time (ms) of this call, measured with events on the current stream

    def mark(name):
        if "timing" in hooks:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

    mark("start")
    for img, nrm, mask in zip(input_imgs, input_normals, masks):
        if erode_kernel_size > 0:
            mask = erode_mask(mask, erode_kernel_size)
        rm, mk = refmap_mask_make(img[mask], nrm[mask], res=refmap_res, angle_threshold=np.pi / 128 / 2)  # (scripts/estimate.py:57)
        refmaps.append(rm.permute(2, 0, 1))
        refmasks.append(mk)
    B = len(refmaps)
    mark("refmap_gather")
    batch = {"tag": [f"obj{i}" for i in range(B)], "raw_refmap": torch.stack(refmaps), "raw_refmask": torch.stack(refmasks)}
    c, _, _ = ObsNet_model.get_cond_for_predict(batch, noise=hooks.get("cond_noise"))
    use_ddim = ObsNet_model.ddim_steps is not None
    extra = {} if seed is None else {"seed": seed}
    obs_extra = {k: hooks[k] for k in ("x_T", "noise") if k in hooks}
    with ObsNet_model.ema_scope("Plotting"):
        samples, _ = ObsNet_model.sample_log(cond=c, batch_size=B, ddim=use_ddim, ddim_steps=ObsNet_model.ddim_steps, eta=ObsNet_model.ddim_eta,
                                             **extra, **obs_extra)
    inpaint = ObsNet_model.ds.rescale(ObsNet_model.decode_first_stage(samples))
    mark("obsnet_sampler")
    LrK, _, illnet_c, refnet_c, _ = DRMNet_model.get_input_for_predict({"tag": batch["tag"], "LrK": inpaint})
    loop_extra = {k: hooks[k] for k in ("noise0", "step_noise") if k in hooks}
    with DRMNet_model.ema_scope():
        samples, zK_est, K = DRMNet_model.p_sample_loop(LrK, illnet_c, refnet_c, verbose=False, early_exit=early_exit, **extra, **loop_extra)
    Lr0 = DRMNet_model.ds.rescale(DRMNet_model.decode_first_stage(samples)).clip(0)
    if DRMNet_model.refmap_input_scaler is not None:
        Lr0 = Lr0 / DRMNet_model.normalizing_scale[:, None, None, None]
    mark("drmnet_loop")
    if marks:
        marks[-1][1].synchronize()
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            hooks["timing"][name] = hooks["timing"].get(name, 0.0) + e0.elapsed_time(e1)
    return Lr0, zK_est, K


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
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    """the command line, with the two rules argparse cannot state: --gt_envmap and --gt_view_from come as a pair, and --gt_z and --gt_merl
    exclude each other"""
    p = parser()
    args = p.parse_args(argv)
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
    Lr0_sample, zK_est = estimate(drmnet_model, obsnet_model, input_img, input_normal, mask, hooks=hooks)
    envmap_est = drmnet_model.r0toenvmap(Lr0_sample[None], (drmnet_model.image_size, drmnet_model.image_size * 2))[0]  # [H, W, 3]
    args.output_dir.mkdir(exist_ok=True)
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

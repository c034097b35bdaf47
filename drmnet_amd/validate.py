"""Validation of a DRMNet or ObsNetDiffusion checkpoint, the reference's ``python main.py --base <yaml>`` without ``-t`` (main.py:685, trainer.validate) on the
MI355X path.

    python -m drmnet_amd.validate --base configs/drmnet/eval_drmnet.yaml --data_root data/LavalIndoor+PolyHaven_2k [--split val]
        [--datalist envs_val.txt] [--batch_size 20] [--limit N] [--precision auto] [--seed 0] [--ckpt drmnet.ckpt]

Every batch goes through ``DRMNet.validation_step``: the forward process renders the reflectance maps of (zK, zk, zkm1) under the item's
environment map and view (csrc/render.hip), both networks run once on the live and once on the EMA weights, and the losses are reduced on
the device (csrc/losses.hip).  One JSON line is printed: the epoch means of ``val/loss_refmap``, ``val/loss_refcode``, ``val/loss`` and their
``_ema`` twins, weighted by batch size as Lightning's ``on_epoch`` reduction weights them, plus the item and batch counts.

The dataset is the ``data.params.validation`` node of the YAML when it has one (a copy of the reference's training YAML works unchanged);
otherwise it is a ParametricRefmapDataset built from the flags, with the transform of the YAML's ``predict`` node.

An ``ObsNetDiffusion`` model (configs/obsnet/train_obsnet.yaml of the reference: cond_stage_key ``masked_LrK``) goes through
``ObsNetDiffusion.validation_step`` instead: LrK rendered from zK, the dataset's ``dynamic_normalize`` transform under the item's sparse mask,
the forward process and the loss reduction on csrc/obs_forward.hip, the network once on the live and once on the EMA weights.  The means
are then those of ``val/loss_simple``, ``val/loss_vlb``, ``val/loss`` and their ``_ema`` twins.  Its items need masks: when the validation
node carries a non-null ``mask_root``, the node's params build a ``drmnet_amd.dataset.MaskedRefmapDataset`` -- the node's own target,
ParametricRefmapDataset, raises for ``mask_root`` (it stands for the OpenCV-reading class of the reference) -- and without a node
``--mask_root`` [``--mask_list``] do the same from the flags.  The maps come with the items (``return_envmap: true`` in the node; the flag path
sets it) or from the model's ``envmap_dir``.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Optional

import torch

QUADRATURE_NOTE = ("the reflectance maps are rendered with a fixed 32 x 32 quadrature per lobe without importance sampling or prefiltering of the "
                   "environment map: it is unvalidated for small, very bright lights in 1000 x 2000 maps")


def light_note(light_samples: int) -> str:
    """The caveat's replacement once the renders are light-sampled"""
    return (f"the reflectance maps are rendered with a 32 x 32 quadrature per lobe combined by multiple importance sampling with M = {light_samples} "
            "light samples drawn from each environment map (drm_shading's light_samples)")


def set_light_samples(model, light_samples: int) -> None:
    """--light_samples on the model's reflectance-map renderer (a DRMNet without a renderer_config gets its default renderer first)"""
    from .render import RefMapRenderer

    renderer = model._renderer() if hasattr(model, "_renderer") else getattr(model, "renderer", None)
    if not isinstance(renderer, RefMapRenderer):
        raise SystemExit("validate: --light_samples needs a model whose renderer is drmnet_amd.render.RefMapRenderer")
    renderer.light_samples = RefMapRenderer(1, light_samples=light_samples).light_samples  # (validated as the constructor validates it)


def collate(items):
    """torch's default_collate (main.py:366-371 without the mesh entry this dataset never has)."""
    from torch.utils.data import default_collate

    return default_collate(items)


@torch.no_grad()
def validate(model, dataset, batch_size: int, limit: Optional[int] = None, precision: Optional[str] = None, seed: int = 0) -> dict:
    """One validation epoch of ``model`` (on the GPU) over the first ``limit`` items of ``dataset`` in order, ``batch_size`` at a time.  The
    dataset is attached both ways as main.py does (``dataset.model``, ``model.ds``).  ``model``: a DRMNet or an ObsNetDiffusion -- the means are
    those of whatever keys its ``validation_step`` returns.  ``precision``: the model's set_precision mode, None leaves the model as it is.
    ``seed``: batch i keys its forward noise by seed + 2 i (live) and seed + 2 i + 1 (EMA).  Returns the batch-size-weighted epoch means as
    floats, plus "items", "batches" and the per-batch dicts under "per_batch" (each with its "batch_size")."""
    if precision is not None:
        model.set_precision(precision)
    dataset.model = model
    model.ds = dataset
    n = len(dataset) if limit is None else min(len(dataset), int(limit))
    per_batch = []
    for i, start in enumerate(range(0, n, batch_size)):
        batch = collate([dataset[j] for j in range(start, min(start + batch_size, n))])
        out = model.validation_step(batch, i, seed=seed + 2 * i)
        per_batch.append((model.batch_size, out))  # (device scalars: nothing waits for the GPU inside the loop)
    rows = [dict({k: float(v) for k, v in out.items()}, batch_size=bs) for bs, out in per_batch]
    result = {k: sum(r[k] * r["batch_size"] for r in rows) / n for k in rows[0] if k != "batch_size"} if rows else {}
    result.update(items=n, batches=len(rows), per_batch=rows)
    return result


def build_dataset(config: dict, args):
    """The YAML's data.params.validation node (as a MaskedRefmapDataset when it carries a mask_root); without one, a ParametricRefmapDataset
    from the flags (a MaskedRefmapDataset with --mask_root)."""
    from .config import get_obj_from_str, instantiate_from_config
    from .dataset import MaskedRefmapDataset, ParametricRefmapDataset

    params = (config.get("data") or {}).get("params") or {}
    if "validation" in params and args.data_root is None:
        node = params["validation"]
        node_params = dict(node.get("params") or {})
        if node_params.get("mask_root") is not None and get_obj_from_str(node["target"]) is ParametricRefmapDataset:
            return MaskedRefmapDataset(**dict(node_params, mask_list=node_params.get("mask_list", getattr(args, "mask_list", None))))
        return instantiate_from_config(node)
    if args.data_root is None:
        raise SystemExit("validate: the config has no data.params.validation node, so --data_root is needed")
    base = dict((params.get("predict") or {}).get("params") or {})
    model_params = config["model"]["params"]
    if "z0" in model_params:
        zdim = len(model_params["z0"])
    else:  # ObsNet has no z0: the BRDF code is as long as the renderer's parameter list
        zdim = len(((model_params.get("renderer_config") or {}).get("params") or {}).get("brdf_param_names") or [1.0])
    kw = dict(size=base.get("size", model_params.get("image_size", 128)), split=args.split, data_root=str(args.data_root), zdim=zdim,
              transform_func=base.get("transform_func", "log"), clamp_before_exp=base.get("clamp_before_exp", 0), return_envmap=True,
              datalist=args.datalist)
    if getattr(args, "mask_root", None) is not None:
        return MaskedRefmapDataset(mask_root=str(args.mask_root), mask_list=args.mask_list, **kw)
    return ParametricRefmapDataset(**kw)


def make_parser(light_samples: int = 0) -> argparse.ArgumentParser:
    note = light_note(light_samples) if light_samples > 0 else QUADRATURE_NOTE
    p = argparse.ArgumentParser(prog="python -m drmnet_amd.validate", description="Validation losses of a DRMNet or ObsNetDiffusion checkpoint on the GPU. Note: " + note + ".")
    p.add_argument("--base", type=Path, required=True, help="the model config (the reference's eval or training YAML)")
    p.add_argument("--data_root", type=Path, default=None, help="directory of the <name>.exr environment maps (overrides the YAML's validation node)")
    p.add_argument("--split", choices=["train", "val", "test"], default="val")
    p.add_argument("--datalist", type=str, default=None, help="text file naming one <name>.exr per line (default data/datalists/<data_root name>/envs_<split>.txt)")
    p.add_argument("--mask_root", type=Path, default=None, help="ObsNet: directory of the sparse masks (<mask_root>/<train|test>/<name of the list>)")
    p.add_argument("--mask_list", type=str, default=None,
                   help="text file naming one mask image per line (default data/datalists/<mask_root name>/sparsemaskannotations_<split>.txt)")
    p.add_argument("--batch_size", type=int, default=20)
    p.add_argument("--limit", type=int, default=None, help="validate the first N items only")
    p.add_argument("--precision", default="auto", help="conv arithmetic of the networks (DRMNet.set_precision / ObsNetDiffusion.set_precision)")
    p.add_argument("--seed", type=int, default=0, help="keys the forward noise (ObsNet: the steps t as well)")
    p.add_argument("--ckpt", type=Path, default=None, help="checkpoint to load instead of the YAML's ckpt_path")
    p.add_argument("--light_samples", type=int, default=0,
                   help="M > 0 (a power of two in [64, 65536]): render with M light samples per environment map, for maps with suns and lamps "
                        "(sets light_samples on the model's RefMapRenderer); 0 keeps the plain quadrature")
    return p


def main(argv=None) -> dict:
    from .config import instantiate_from_config, load_config

    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--light_samples", type=int, default=0)
    args = make_parser(pre.parse_known_args(argv)[0].light_samples).parse_args(argv)
    config = load_config(args.base)
    model_cfg = {"target": config["model"]["target"], "params": dict(config["model"].get("params") or {})}
    if args.ckpt is not None:
        model_cfg["params"]["ckpt_path"] = str(args.ckpt)
    model = instantiate_from_config(model_cfg).cuda()
    if args.light_samples:
        set_light_samples(model, args.light_samples)
    dataset = build_dataset(config, args)
    result = validate(model, dataset, args.batch_size, limit=args.limit, precision=args.precision, seed=args.seed)
    result.pop("per_batch")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()

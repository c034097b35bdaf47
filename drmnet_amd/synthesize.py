"""Make the input of ``python -m drmnet_amd.estimate`` from a mesh, a BRDF and an environment map -- the forward model, run forward.

    python -m drmnet_amd.synthesize --mesh M.obj --envmap E.exr (--z m R G B r s | --merl material.binary) --view_from x y z --image_size 128 --output_dir D

writes into D the three files ``estimate`` reads,

    image.exr    H x W x 3 radiance of the object (drmnet_amd.mesh.render_mesh: direct light, black background; with ``--shadows`` the
                 object shadows itself, and with ``--bounces 1`` on top of it the light one part reflects onto another is there (one
                 bounce); with ``--light_samples M`` a sun or a lamp a few texels wide is resolved, its cast shadow included)
    normal.npy   H x W x 3 float32 shading normals in the view frame (right, up, back)
    mask.png     |normal| > 0.5: the pixels more than half covered

and ``refmap.exr``: the reflectance map RefMapRenderer renders for the same (z, envmap, view), the ground truth the estimate should approach.
``--light_samples`` applies to both renders, so the image and the map it is judged against resolve the same lights.
``--z`` is the canonical row (metallic, base colour R G B, roughness, specular).  ``--merl material.binary`` takes its place (exactly one
of the two): the object is shaded under that measured BRDF (drmnet_amd.mesh.render_mesh_measured, read as ``--merl_lookup`` says;
``--shadows`` holds, ``--light_samples`` and ``--bounces`` are not built under a table) and ``refmap.exr`` is render.render_table's, so
``estimate --gt_merl material.binary`` on the written files judges the estimate against the material the image was made with.  The mesh (.obj, or a .pt dict) is scaled to radius 0.9
so that it fits the film from every view; without ``--envmap`` the environment is white.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

from .render import QUAD

# --z in the order of the canonical row, under names canonical_rows reads
NAMES = ("metallic", "base_color.value.R", "base_color.value.G", "base_color.value.B", "roughness", "specular")


def main(argv=None):
    from . import file_io
    from .mesh import check_bounces, load_mesh, normalize_mesh, render_mesh, render_mesh_measured
    from .render import render, render_table

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--mesh", type=Path, required=True, help="triangle mesh (.obj, or a .pt dict of vertex_positions / vertex_normals / faces)")
    parser.add_argument("--envmap", type=Path, default=None, help="lat-long environment map (.exr); default: white")
    parser.add_argument("--z", type=float, nargs=6, default=None, metavar=("m", "R", "G", "B", "r", "s"),
                        help="metallic, base colour R G B, roughness, specular (exactly one of --z and --merl)")
    parser.add_argument("--merl", type=Path, default=None, help="a measured BRDF (MERL .binary) as the material, in place of --z")
    parser.add_argument("--merl_lookup", choices=("linear", "nearest"), default="linear", help="how --merl's table is read (default: linear)")
    parser.add_argument("--view_from", type=float, nargs=3, default=[0.0, 0.0, 1.1], metavar=("x", "y", "z"), help="viewer position (off the +-y axis)")
    parser.add_argument("--image_size", type=int, default=128)
    parser.add_argument("--refmap_res", type=int, default=128, help="resolution of refmap.exr")
    parser.add_argument("--quad", type=int, default=QUAD)
    parser.add_argument("--shadows", action="store_true", help="trace shadow rays: parts of the mesh cut light off from other parts (default: off)")
    parser.add_argument("--bounces", type=int, default=0, help="1: one bounce of interreflection (needs --shadows; not with --light_samples); default 0")
    parser.add_argument("--bounce_quad", type=int, default=4, help="the bounce is estimated with bounce_quad^2 directions, 1 .. 16 (default 4)")
    parser.add_argument("--light_samples", type=int, default=0,
                        help="light samples drawn from the environment map, for image.exr and refmap.exr alike: a power of two in [64, 65536] "
                        "(default 0: the lobe quadrature alone)")
    parser.add_argument("--output_dir", type=Path, default=Path("./outputs/"))
    args = parser.parse_args(argv)
    if (args.z is None) == (args.merl is None):
        parser.error("exactly one of --z and --merl")
    if args.merl is not None and (args.light_samples or args.bounces):
        parser.error("--light_samples and --bounces under --merl are not built: a measured BRDF renders with the quadrature alone, with or without --shadows")
    check_bounces(args.bounces, args.bounce_quad, args.shadows, args.light_samples)

    if not torch.cuda.is_available():
        raise RuntimeError("synthesize renders on the GPU (drmnet_amd has no CPU path) and no GPU is visible")
    dev = torch.device("cuda", torch.cuda.current_device())
    obj = normalize_mesh(load_mesh(args.mesh))
    env = None if args.envmap is None else file_io.load_exr(args.envmap, as_torch=True).to(dev)[None]
    view = torch.tensor([args.view_from], dtype=torch.float32)
    if args.merl is not None:
        from .merl import MeasuredBSDF

        bsdf = MeasuredBSDF.from_file(args.merl)
        image, normal, _, _ = render_mesh_measured(obj, bsdf, env, image_size=args.image_size, view_from=view, quad=args.quad, shadows=args.shadows,
                                                  lookup=args.merl_lookup)
        refmap = render_table(bsdf, env, res=args.refmap_res, quad=args.quad, view_from=view, lookup=args.merl_lookup)
    else:
        z = torch.tensor([args.z], dtype=torch.float32, device=dev)
        image, normal, _, _ = render_mesh(obj, z, NAMES, env, image_size=args.image_size, view_from=view, quad=args.quad, shadows=args.shadows,
                                         light_samples=args.light_samples, bounces=args.bounces, bounce_quad=args.bounce_quad)
        refmap = render(z, NAMES, env, res=args.refmap_res, quad=args.quad, view_from=view, light_samples=args.light_samples)
    normal = normal[0].permute(1, 2, 0).cpu().numpy()
    mask = np.linalg.norm(normal, axis=-1) > 0.5
    args.output_dir.mkdir(parents=True, exist_ok=True)
    file_io.save_exr(args.output_dir / "image.exr", image[0].permute(1, 2, 0))
    np.save(args.output_dir / "normal.npy", normal)
    file_io.save_png(args.output_dir / "mask.png", np.repeat(mask[:, :, None].astype(np.float32), 3, axis=-1))
    file_io.save_exr(args.output_dir / "refmap.exr", refmap[0].permute(1, 2, 0))
    print(f"wrote image.exr, normal.npy, mask.png ({int(mask.sum())} of {mask.size} pixels) and refmap.exr to {args.output_dir}")


if __name__ == "__main__":
    main()

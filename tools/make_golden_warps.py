#!/usr/bin/env python3
"""Generate tests/golden/warps.npz by running the REFERENCE's own sphere / envmap warps (utils/transform.py: envmap2mirmap, rotate_envmap,
mirimg2envmap, refmap2refimg_torch) on the CPU, imported through tools/refharness.py as tools/make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_warps.py

Writes data only: seeded inputs, the reference's fp32 outputs, the case list (function, arguments, array names; a JSON string) and, for
every case whose source azimuth goes through the `% 2 pi` wrap, the recorded seam margin.  At the wrap an ulp of difference in the azimuth
moves a border-clamped sample from column 0 to column W - 1, so a fixture with a sample there would compare rounding, not warps: the margin
is the smallest distance (radians, float64, tests/warp_ref.py) of any sample's source azimuth from the wrap, and a case below MIN_MARGIN is
refused, not written.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refharness as rh  # noqa: E402
import warp_ref as wr  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MIN_MARGIN = 1e-4


def f32(v):
    """a direction as fp32-exact Python floats: what the reference, the package and the float64 restatement are all given"""
    return [float(x) for x in np.asarray(v, dtype=np.float32)]


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return f32(v / np.linalg.norm(v))


def azimuth_view(k):
    """view k of 64 on the horizontal circle"""
    a = 2 * np.pi * k / 64
    return f32([np.sin(a), 0.0, np.cos(a)])


TILTED = unit([0.6, 0.3, 0.742])  # off the horizontal circle: top is re-orthogonalised


def main():
    rh.install_stubs()
    from utils import transform as rt

    g = torch.Generator().manual_seed(20)
    arrays = {
        "env": torch.exp(0.5 * torch.randn((2, 3, 32, 64), generator=g)).numpy(),
        "ball": torch.exp(0.5 * torch.randn((1, 3, 32, 32), generator=g)).numpy(),
        "refmap": torch.exp(0.5 * torch.randn((2, 3, 16, 16), generator=g)).numpy(),
    }
    cases = []

    def add(fn, src, items, kwargs, margin=None, squeeze=False):
        """run the reference on arrays[src][items] and record the case"""
        x = torch.from_numpy(arrays[src][items])
        name = f"{fn}_{len(cases):02d}"
        if margin is not None and margin < MIN_MARGIN:
            raise SystemExit(f"{name} {kwargs}: a sample {margin:.2e} rad from the azimuth wrap (< {MIN_MARGIN}): pick another view")
        args = dict(kwargs)
        for k in ("output_shape", "out_shape"):
            if k in args:
                args[k] = tuple(args[k])
        out = getattr(rt, fn)(x[0] if squeeze else x, **args)
        case = {"fn": fn, "input": src, "items": [items.start, items.stop], "kwargs": kwargs, "out": name, "squeeze": squeeze}
        if isinstance(out, tuple):
            arrays[name + "_mask"] = out[1].numpy()
            out = out[0]
        arrays[name] = out.numpy()
        if margin is not None:
            case["seam_margin"] = margin
        cases.append(case)
        print(f"  {name}: {tuple(arrays[name].shape)}" + (f", seam margin {margin:.2e} rad" if margin is not None else ""), kwargs)

    def e2m(shape, items=slice(0, 2), **kw):
        geometry = {k: v for k, v in kw.items() if k != "log_scale_interpolation"}
        margin = wr.seam_margin(wr.envmap2mirmap_positions(32, 64, shape, **geometry)[2])
        add("envmap2mirmap", "env", items, dict(output_shape=list(shape), **kw), margin)

    # envmap2mirmap on white noise: every output shape from the default view, the other views at the pooled shapes, one flag per case
    for shape in ((16, 16), (10, 10), (8, 16), (48, 48)):
        e2m(shape)
    for view in (azimuth_view(5), azimuth_view(37), TILTED):
        for shape in ((16, 16), (10, 10)):
            e2m(shape, view_from=view)
    e2m((48, 48), items=slice(0, 1), view_from=TILTED)
    e2m((16, 16), mitigate_aliasing=False)
    e2m((16, 16), log_scale_interpolation=True)
    e2m((16, 16), flip_horizontal=True)
    e2m((16, 16), envmap_left_edge=[1.0, 0.0, 0.0])

    # rotate_envmap, one map at a time (all the reference handles)
    yaw = 0.7
    frames = {
        "identity": ([0.0, 1.0, 0.0], [0.0, 0.0, -1.0]),
        "yaw": ([0.0, 1.0, 0.0], f32([np.sin(yaw), 0.0, -np.cos(yaw)])),
    }
    up = np.asarray(wr.reorthogonalise(np.asarray(TILTED, np.float64), np.array([0.0, 1.0, 0.0])))
    frames["tilted"] = (f32(up), f32(-np.asarray(TILTED, np.float64)))
    for name, shape in (("identity", None), ("yaw", None), ("tilted", None), ("tilted", (16, 32))):
        zen, left = frames[name]
        kw = dict(src_envmap_zenith=[0.0, 1.0, 0.0], src_envmap_left_edge=[0.0, 0.0, -1.0], tgt_envmap_zenith=zen, tgt_envmap_left_edge=left)
        margin = wr.seam_margin(wr.rotate_envmap_positions(shape or (32, 64), kw["src_envmap_zenith"], kw["src_envmap_left_edge"], zen, left)[2])
        if shape is not None:
            kw["out_shape"] = list(shape)
        add("rotate_envmap", "env", slice(1, 2), kw, margin)

    # mirimg2envmap: 32 x 32 ball image -> (16, 32)
    for view in ([0.0, 0.0, 1.0], TILTED):
        for log in (False, True):
            add("mirimg2envmap", "ball", slice(0, 1), dict(output_shape=[16, 32], view_from=view, log_scale_interpolation=log))

    # refmap2refimg_torch: the default radius, a 3-D input with radius 12, and the mask
    add("refmap2refimg_torch", "refmap", slice(0, 2), {})
    add("refmap2refimg_torch", "refmap", slice(0, 1), dict(radius=12), squeeze=True)
    add("refmap2refimg_torch", "refmap", slice(0, 2), dict(return_mask=True))

    path = os.path.join(GOLD, "warps.npz")
    np.savez_compressed(path, cases=np.array(json.dumps(cases)), **arrays)
    print(f"wrote warps.npz ({os.path.getsize(path) / 1024:.0f} KiB, {len(cases)} cases)")


if __name__ == "__main__":
    main()

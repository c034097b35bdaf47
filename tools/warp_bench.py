#!/usr/bin/env python3
"""Time envmap2mirmap at its typical use, a batch of 1024 x 2048 environment maps pooled to 128 x 128 mirror maps, on csrc/sphere_warp.hip and
on torch's own kernels on the same GPU.

    python tools/warp_bench.py [--batch 32] [--reps 100] [--warmup 3] [--out result.json]

The baseline is what the reference runs, torch.nn.functional.grid_sample on the 1024 x 1024 sample grid followed by adaptive_avg_pool2d; its
uv grid is built once outside the timed window (the reference rebuilds it on every call), so the comparison is against torch's two kernels
alone.  The fused kernel builds the geometry per sample inside the launch and never stores the 1024 x 1024 intermediate.  Both are timed
with device events over `reps` calls, alternating, after `warmup` calls of each; the two outputs are compared first.  Prints one JSON line.
Not part of bench.py: there is no number for this on earlier revisions, which lack the warp.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_uv(H, W, OH, OW, B, dev):
    """the reference's sample grid for the default frame (view +x, top +y, zenith +y, left edge -z, reversed azimuth), in fp32 torch ops"""
    S = min(H, W) if OH < H else max(OH, OW)
    theta = (torch.arange(S, device=dev, dtype=torch.float32) + 0.5) * (torch.pi / S)
    phi = (torch.arange(S, device=dev, dtype=torch.float32) - (S - 1) / 2) * (torch.pi / S)
    theta, phi = torch.meshgrid(theta, phi, indexing="ij")
    top, view, binormal = (torch.tensor(v, device=dev) for v in ([0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]))
    n = torch.cos(theta)[..., None] * top + (torch.sin(theta) * torch.cos(phi))[..., None] * view + (torch.sin(theta) * torch.sin(phi))[..., None] * binormal
    r = torch.nn.functional.normalize(2 * (n @ view)[..., None] * n - view, dim=-1)
    zen, left, bi = (torch.tensor(v, device=dev) for v in ([0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]))
    t, p = torch.arccos(r @ zen), torch.arctan2(r @ bi, r @ left)
    uv = torch.stack([p % (2 * torch.pi) / torch.pi - 1, t * (2 / torch.pi) - 1], dim=-1)
    return uv[None].expand(B, -1, -1, -1).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--in_shape", type=int, nargs=2, default=(1024, 2048))
    ap.add_argument("--out_shape", type=int, nargs=2, default=(128, 128))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("warp_bench times GPU kernels and no GPU is visible")
    from drmnet_amd.transform import envmap2mirmap

    dev = torch.device("cuda", torch.cuda.current_device())
    (H, W), (OH, OW), B = a.in_shape, a.out_shape, a.batch
    env = torch.exp(0.5 * torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(0))).to(dev)
    uv = torch_uv(H, W, OH, OW, B, dev)

    def fused():
        return envmap2mirmap(env, (OH, OW))

    def baseline():
        return torch.nn.functional.adaptive_avg_pool2d(
            torch.nn.functional.grid_sample(env, uv, mode="bilinear", padding_mode="border", align_corners=False), (OH, OW))

    agree = float((fused() - baseline()).norm() / baseline().norm())
    for _ in range(a.warmup):
        fused(), baseline()
    times = {"fused": [], "baseline": []}
    for _ in range(a.reps):
        for name, fn in (("fused", fused), ("baseline", baseline)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    result = {"workload": f"envmap2mirmap {B}x3x{H}x{W} -> {OH}x{OW}", "fused_ms": med["fused"], "torch_grid_sample_pool_ms": med["baseline"],
              "fused_ms_min_max": [min(times["fused"]), max(times["fused"])], "torch_ms_min_max": [min(times["baseline"]), max(times["baseline"])],
              "speedup": med["baseline"] / med["fused"], "rel_l2_fused_vs_torch": agree, "reps": a.reps}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return result


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/mesh_light_sun.npz: the sun scene of the convergence test of light sampling on mesh object images, with what of its
float64 reference is too slow to trace in a test.

    python tools/make_golden_mesh_light.py

The scene: shadow_ref.two_spheres() seen from +z on a 12 x 12 film, S = 1, the ROUGH row (0, 0.8, 0.5, 0.2, 0.5, 0.5), under the 32 x 64 map
smooth_env(32, 64) with texel [11, 19] = (3e4, 2.5e4, 2e4).  The reference is mesh_light_ref.texel_sum: the integral of L V f cos as a sum
over the directions of the supersample-4 texel grid, each direction traced with the occlusion rule (float64, CPU only; about three minutes).
Stored: the map; `open4`, for every lit film sample the bit mask of the supersample-4 directions that are not cut off (it depends on the
scene and the view alone; tests/test_mesh_light_cpu.py re-traces a seeded subset of it and recomputes the sums); `truth4` / `plain4`, the
shadowed and unshadowed texel sums [3, 12, 12]; and, for the film rows ROWS8, `truth8`, the shadowed sum at supersample 8, kept to show
what the reference itself is good to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_light_ref as mlr  # noqa: E402
import render_ref as rr  # noqa: E402
import shadow_ref as sr  # noqa: E402

FILM, S, Q = 12, 1, 32
ROUGH = [0.0, 0.8, 0.5, 0.2, 0.5, 0.5]
SUN = (11, 19)
ROWS8 = (3, 4, 5)  # the film rows the ball's shadow crosses


def smooth_env(EH, EW):
    """the smooth environment of tests/test_gpu_render.py"""
    d, _ = rr.env_dirs(EH, EW)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([1 + 0.5 * x + 0.3 * y * y, 0.8 + 0.4 * z - 0.2 * x * y, 1.2 + 0.6 * y + 0.1 * x], -1)


def sun_scene():
    env = smooth_env(32, 64).astype(np.float32).astype(np.float64)
    env[SUN] = (3e4, 2.5e4, 2e4)
    return env


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


if __name__ == "__main__":
    env = sun_scene()
    p, n, f = sr.two_spheres()
    tr = mlr.trace(p, n, f, ROUGH, None, FILM, FILM, S, 4)  # (the lobes are not used here: a small Q)
    K = int(tr["lit"].sum())
    rad4, open4 = mlr.texel_sum(tr, env, 4, p, f)
    truth4 = mlr.film(tr, rad4)
    plain4 = mlr.film(tr, mlr.texel_sum(tr, env, 4, open_rays=np.ones_like(open4))[0])
    # the lit samples of the rows ROWS8, in the order of tr["lit"]
    row_of = np.nonzero(tr["lit"])[0] // S
    samples = [k for k in range(K) if row_of[k] in ROWS8]
    rad8, _ = mlr.texel_sum(tr, env, 8, p, f, samples=samples)
    truth8 = mlr.film(tr, rad8)[:, list(ROWS8)]
    print(f"{K} lit samples, {len(samples)} of them in the rows {ROWS8}; {1 - open4.mean():.3f} of the directions cut off")
    print(f"shadows move the truth by {rel_l2(plain4, truth4):.3f}; supersample 4 against 8 on the rows {ROWS8}: "
          f"rel-L2 {rel_l2(truth4[:, list(ROWS8)], truth8):.2e}")
    out = os.path.join(ROOT, "tests", "golden", "mesh_light_sun.npz")
    np.savez_compressed(out, env=env, z=np.array(ROUGH), film=FILM, S=S, open4=np.packbits(open4, axis=1), truth4=truth4, plain4=plain4,
                        rows8=np.array(ROWS8), truth8=truth8)
    print("wrote", out, os.path.getsize(out), "bytes")

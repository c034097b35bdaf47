#!/usr/bin/env python3
"""Writes tests/golden/render_light_sun.npz: the sun scene of the light-sampled render's accuracy tests and its float64 reference renders.

    python tools/make_golden_light.py

The scene is a 32 x 64 map, background (0.6, 0.8, 1.0), texel [9, 33] = (3e4, 2.5e4, 2e4) and texel [20, 40] = (500, 800, 300), rendered
at R = 8, S = 2 for two BSDF rows with roughness >= 0.5.  The references are tests/render_ref.py's texel sums (float64, CPU only; about a
minute): `texel4` at supersample 4, which tests/test_render_light_cpu.py recomputes, and `texel8` at supersample 8, kept to show what the
reference itself is good to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import render_ref as rr  # noqa: E402

R, S = 8, 2
Z = np.array([[0.0, 0.7, 0.5, 0.3, 0.5, 0.6], [0.4, 0.7, 0.5, 0.3, 1.0, 0.2]])


def sun_scene():
    env = np.tile(np.array([0.6, 0.8, 1.0]), (32, 64, 1))
    env[9, 33] = (3e4, 2.5e4, 2e4)
    env[20, 40] = (500.0, 800.0, 300.0)
    return env


if __name__ == "__main__":
    env = sun_scene()
    t4 = np.stack([rr.render_texel_sum(z, env, R, S, supersample=4) for z in Z])
    t8 = np.stack([rr.render_texel_sum(z, env, R, S, supersample=8) for z in Z])
    for k in range(len(Z)):
        print(f"z {Z[k].tolist()}: supersample 4 against 8: rel-L2 {np.linalg.norm(t4[k] - t8[k]) / np.linalg.norm(t8[k]):.2e}")
    out = os.path.join(ROOT, "tests", "golden", "render_light_sun.npz")
    np.savez(out, env=env, z=Z, texel4=t4, texel8=t8, R=R, S=S)
    print("wrote", out, os.path.getsize(out), "bytes")

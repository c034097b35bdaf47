"""The bytes the forward model's renders write: the sphere (drm_render_refmap_views / _lit), a normal map (drm_render_normals), both under
MERL tables (drm_brdf_to_merl, drm_render_refmap_table, drm_render_normals_table), the four mesh entries and drm_mirmap2envmap.

A case compares the SHA-256 of its output tensors' bytes with tests/golden/render_digests.json.  The digests were recorded by running this
file's cases (`python tests/test_gpu_render_pinned.py --record FILE`, DRM_LIB_PATH naming the library) against the library built from the
commit BEFORE the sample sets and the pixel kernels were stated once (csrc/render_shared.h), never from the code under test.  These kernels
have no atomics: every lane keeps its partial sums in a fixed order and the lanes meet in a fixed butterfly.  The recorder ran every case
twice and pins only a digest that reproduced (the JSON holds null otherwise).  All 37 reproduced (FELL_BACK below is empty), so this file has
no tolerance to fall back to: a null in the JSON fails its case.  The existing tests of each entry compare with the float64 restatements.

Inputs are built on the CPU from seeded generators.  Shapes, the smallest at which each shared piece can go wrong: B = 2 rows (one with both
lobes, one with metallic 1, where the diffuse lobe is skipped); Q = 9, 81 grid points over 64 lanes, so 17 lanes take two points and both
the stride loop and the lane order matter; maps 8 x 16 with one texel 1000 times brighter, and for the lit cases one map all zero, which
turns the light technique off for that row; M = 64 light samples; two views off the axes.  Sphere: R = 7, whose centre pixel at S = 1 sees
exactly +z, the frame's lensq == 0 branch.  Normal map: 6 x 6 with pixels exactly (0, 0, 1), zero, NaN, back-facing and masked off.
Mesh: shadow_ref.two_spheres() (400 faces), 8 x 8, S = 2, Q = 5.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_digests.json")
FELL_BACK = ()  # (every case reproduced on the recording run)
NAMES6 = ["metallic.value", "base_color.value.R", "base_color.value.G", "base_color.value.B", "roughness.value", "specular"]
ROWS = [[0.3, 0.8, 0.5, 0.2, 0.4, 0.5], [1.0, 0.9, 0.6, 0.3, 0.05, 0.5]]
ROWS2 = [[0.0, 0.2, 0.7, 0.9, 0.7, 1.0], [0.6, 0.5, 0.5, 0.5, 0.2, 0.0]]  # the second stack of the L = 2 case
VIEWS = [(0.6, 0.3, 1.0), (-1.0, 0.2, 0.4)]
Q, M, R = 9, 64, 7


def envs(lit=False):
    """[2, 8, 16, 3] positive maps with one texel 1000 times brighter; lit: map 1 is all zero (no light: lt.norm == 0)"""
    e = torch.rand((2, 8, 16, 3), generator=torch.Generator().manual_seed(3)) + 0.05
    e[0, 2, 5] *= 1000.0
    e[1, 6, 11] *= 1000.0
    if lit:
        e[1] = 0.0
    return e


def normal_maps(Bn):
    """[Bn, 6, 6, 3] front-facing normals of any length with the special pixels, and the mask [Bn, 6, 6]"""
    n = torch.randn((Bn, 6, 6, 3), generator=torch.Generator().manual_seed(5))
    n[..., 2] = n[..., 2].abs() + 0.1
    n[:, 0, 0] = torch.tensor([0.0, 0.0, 1.0])
    n[:, 0, 1] = 0.0
    n[:, 0, 2, 1] = float("nan")
    n[:, 0, 3] = torch.tensor([0.1, 0.2, -1.0])
    mask = torch.ones((Bn, 6, 6), dtype=torch.uint8)
    mask[:, 1, 1] = 0
    return n, mask


@functools.lru_cache(maxsize=None)
def tables():
    """the two rows exported by drm_brdf_to_merl, each with merl.proxy_alpha of its table"""
    from drmnet_amd.merl import MeasuredBSDF
    from drmnet_amd.render import get_bsdf

    return [MeasuredBSDF.from_principled(get_bsdf(row, NAMES6)) for row in ROWS]


def sphere(S=2, env="maps", view=False, flip=False, light=0, stacked=False):
    def run(dev):
        from drmnet_amd.render import render

        z = torch.tensor([ROWS, ROWS2] if stacked else ROWS)
        e = None if env is None else envs(lit=light > 0).to(dev)
        return [render(z.to(dev), NAMES6, e, res=R, quad=Q, subpixel=S, flip=flip, view_from=torch.tensor(VIEWS) if view else None, light_samples=light)]

    return run


def normals(Bn, env="maps", view=False, light=0):
    def run(dev):
        from drmnet_amd.relight import render_normals

        n, mask = normal_maps(Bn)
        e = None if env is None else envs(lit=light > 0).to(dev)
        return render_normals(n.to(dev), torch.tensor(ROWS).to(dev), NAMES6, e, mask=mask, view_from=torch.tensor(VIEWS) if view else None, quad=Q,
                              light_samples=light)

    return run


def the_tables():
    def run(dev):
        tables.cache_clear()  # (exported anew: the later cases share what this one built)
        return [t.device_table(dev) for t in tables()] + [torch.tensor([t.alpha for t in tables()], dtype=torch.float32)]

    return run


def sphere_table(lookup, env="maps", view=False):
    def run(dev):
        from drmnet_amd.render import render_table

        e = None if env is None else envs().to(dev)
        return [render_table(tables(), e, res=R, quad=Q, subpixel=2, view_from=torch.tensor(VIEWS) if view else None, lookup=lookup)]

    return run


def normals_table(lookup, view=False):
    def run(dev):
        from drmnet_amd.relight import render_normals_measured

        n, mask = normal_maps(2)
        return render_normals_measured(n.to(dev), tables(), envs().to(dev), mask=mask, view_from=torch.tensor(VIEWS) if view else None, quad=Q,
                                       lookup=lookup)

    return run


def mesh(view=False, shadows=False, light=0, bounces=0):
    def run(dev):
        import shadow_ref as sr
        from drmnet_amd.mesh import render_mesh

        p, n, f = sr.two_spheres()
        obj = {"vertex_positions": torch.tensor(np.asarray(p), dtype=torch.float32), "vertex_normals": torch.tensor(np.asarray(n), dtype=torch.float32),
               "faces": torch.tensor(np.asarray(f), dtype=torch.int32)}
        return render_mesh(obj, torch.tensor(ROWS).to(dev), NAMES6, envs(lit=light > 0).to(dev), image_size=8, view_from=torch.tensor(VIEWS) if view else None,
                           quad=5, subpixel=2, shadows=shadows, light_samples=light, bounces=bounces, bounce_quad=2)

    return run


def mirmap(log=False, basis=False, channels_last=False):
    def run(dev):
        from drmnet_amd import ops

        g = torch.Generator().manual_seed(7)
        mir = torch.rand((2, 3, 16, 16), generator=g) + 0.1
        b = torch.rand((3, 16, 16), generator=g) + 0.5
        return [ops.mirmap2envmap(mir.to(dev), (8, 16), basis=b.to(dev) if basis else None, log_scale_interpolation=log, channels_last=channels_last)]

    return run


CASES = {
    "sphere_plain": sphere(),
    "sphere_view": sphere(view=True),
    "sphere_flip": sphere(flip=True),
    "sphere_white": sphere(env=None),
    "sphere_lit": sphere(light=M),
    "sphere_lit_view": sphere(light=M, view=True),
    "sphere_stacked": sphere(stacked=True),
    "sphere_s1_centre_sees_z": sphere(S=1),
    "tables": the_tables(),
    "sphere_table_linear": sphere_table("linear"),
    "sphere_table_nearest": sphere_table("nearest"),
    "sphere_table_linear_view": sphere_table("linear", view=True),
    "sphere_table_nearest_view": sphere_table("nearest", view=True),
    "sphere_table_white": sphere_table("linear", env=None),
    "normals_table_linear": normals_table("linear"),
    "normals_table_linear_view": normals_table("linear", view=True),
    "normals_table_nearest": normals_table("nearest"),
    "mesh_plain": mesh(),
    "mesh_view": mesh(view=True),
    "mesh_shadowed_view": mesh(view=True, shadows=True),
    "mesh_lit": mesh(light=M),
    "mesh_lit_shadowed": mesh(light=M, shadows=True),
    "mesh_bounced_view": mesh(view=True, shadows=True, bounces=1),
    "mirmap2envmap_plain": mirmap(),
    "mirmap2envmap_log": mirmap(log=True),
    "mirmap2envmap_basis": mirmap(basis=True),
    "mirmap2envmap_channels_last": mirmap(channels_last=True),
}
for _bn in (1, 2):
    CASES.update({f"normals_plain_bn{_bn}": normals(_bn), f"normals_view_bn{_bn}": normals(_bn, view=True), f"normals_white_bn{_bn}": normals(_bn, env=None),
                  f"normals_lit_bn{_bn}": normals(_bn, light=M), f"normals_lit_view_bn{_bn}": normals(_bn, light=M, view=True)})


def digest(outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(name, dev):
    outs = CASES[name](dev)
    torch.cuda.synchronize()
    return outs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_render_bytes(dev, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert want is not None, f"{name} has no pinned digest: every case reproduced when the digests were recorded (FELL_BACK is empty)"
    got = digest(run_case(name, dev))
    print(f"{name}: sha256 {got}")
    assert got == want


if __name__ == "__main__":  # the recorder: every case twice; a digest that does not reproduce is stored as null
    assert sys.argv[1] == "--record"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    d = torch.device("cuda:0")
    rec = {}
    for nm in CASES:
        a, b = digest(run_case(nm, d)), digest(run_case(nm, d))
        rec[nm] = a if a == b else None
        print(nm, a, "reproduced" if a == b else f"DID NOT REPRODUCE ({b})", flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")

"""Self-shadowing on the GPU (drm_mesh_occluded, drm_render_mesh with shadows: csrc/bvh.h, csrc/bvh.hip, mesh_shade_kernel<VIEW, true> in
csrc/render.hip, through drmnet_amd.mesh and drmnet_amd.synthesize) against the float64 restatement in tests/shadow_ref.py.

The rule, restated (include/drmnet_hip.h): a ray (o, d) in object space, d of any length, is occluded iff some face g != exclude with its
vertex indices in [0, V) has, with e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1.pv, tv = o - p0, qv = tv x e1, U = tv.pv, V = d.qv,
T = e2.qv, s = sign(det): det != 0 and finite, s U >= 0, s V >= 0, s (U + V) <= |det|, s T > 0.  It is division-free: the exact cases (face
coordinates multiples of 1/64 up to 1, origins on the 1/32 grid up to 1, integer directions up to 4; the largest product, T, stays below
2^24 in units of 64^-3) are decided identically in float32 and float64 and are compared everywhere.  The BVH may never change an answer:
with and without it the query runs the same triangle routine, and the two are compared for every ray, no exceptions.

Shading is compared on the pixels that are not `unsafe_pixel` (mesh_ref: 1e-4 view units from every edge and depth tie), after taking off
`slack`, the absolute contributions of the pixel's marginal rays (shadow_ref: the plane crossing within 1e-4 of an edge, or within 1e-4 of
the origin, or |det| < 1e-9), at the 1e-5 rel-L2 bar the unshadowed mesh image and the sphere render hold.  The restatement alone puts, over
the nine (view, row) cases of SHADING, at most 1.58 % of the traced rays in the marginal set (view 0, METAL), at most 0.59 % of the film
samples in the unsafe set, and at most 1.65 % of the image sum into the slack under the smooth environment and 1.68 % under the white one
(view 0, METAL; ROUGH: 0.63 / 0.68 / 0.05 % for the three views); 1.5 % to 4.2 % of the traced rays are occluded, and the float64 shadowed
image differs from the unshadowed one by 3.7 % to 13.7 % rel-L2."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as mr
import shadow_ref as sr
from conftest import rel_l2
from test_gpu_mesh import DIFFUSE, ENV, METAL, ROUGH, as_obj, rotation
from test_render_cpu import NAMES6

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Q, S, FILM = 8, 2, 16
ROWS = [ROUGH, METAL, DIFFUSE]
VIEWS = [None, (0.6, 0.3, 1.0), (-1.0, 0.2, 0.4)]
CAP = 0.02  # marginal rays of the traced ones, slack of the image sum, unsafe film samples
SCENE = sr.two_spheres()
SOUP = sr.soup()


def bare(p, f):
    """a mesh dict for ray queries (the normals are not read)"""
    return as_obj(p, np.zeros_like(np.asarray(p, dtype=np.float64)), f)


def gpu_occluded(mesh, o, d, ex, bvh):
    from drmnet_amd.mesh import occluded

    o, d = (torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV) for a in (o, d))
    return occluded(mesh, o, d, None if ex is None else torch.tensor(np.asarray(ex), dtype=torch.int32, device=DEV), bvh=bvh).cpu().numpy()


def gpu_render(mesh, z_rows, envs, views, shadows, H=FILM, W=FILM, bvh=None):
    from drmnet_amd.mesh import render_mesh

    z = torch.tensor(z_rows, dtype=torch.float32, device=DEV)
    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    view = None if views is None else torch.tensor(views, dtype=torch.float32)
    return [t.cpu().numpy().astype(np.float64) for t in render_mesh(as_obj(*mesh), z, NAMES6, env, image_size=(H, W), view_from=view, quad=Q, subpixel=S,
                                                                  shadows=shadows, bvh=bvh)]


# ---------------------------------------------------------------------------------------------- 1. exact queries
def exact_case():
    """faces in 1/64, origins in 1/32, integer directions: (positions, faces, origins, dirs, exclude, want) with `want` the hand-derived answers of
    the named rays (the float64 rule is asserted to give them) followed by a grid of rays whose answers the float64 rule gives"""
    tris = np.array([
        [(0, -32, 16), (32, 0, 16), (0, 32, 16)],        # 0  A, in the plane z = 1/4
        [(0, -32, 16), (0, 32, 16), (-32, 0, 16)],       # 1  B, shares the edge x = 0 with A
        [(-64, -64, -32), (64, -64, -32), (0, 64, -32)],  # 2  C, a large face below
        [(-16, -48, 48), (48, -48, 48), (16, -16, 40)],  # 3  D, tilted, above
        [(-16, -48, 48), (48, -48, 48), (16, -16, 40)],  # 4  D again (a duplicate face)
        [(40, 40, -8), (40, 56, 24), (56, 40, 8)],       # 5  E, oblique
    ], dtype=np.float64) / 64.0
    p, f = tris.reshape(-1, 3), np.arange(18, dtype=np.int32).reshape(6, 3)
    named = [  # origin (1/32), direction, exclude, occluded?
        ((0, 0, 0), (0, 0, 1), -1, True),       # through the edge A and B share
        ((0, 0, 0), (0, 0, 1), 0, True),        # ... which B still covers without A
        ((0, 0, 0), (0, 0, 1), 1, True),        # ... and A without B
        ((0, -16, 0), (0, 0, 2), -1, True),     # through the vertex (0, -1/2, 1/4)
        ((16, 0, 0), (0, 0, 3), -1, True),      # through the vertex (1/2, 0, 1/4) of A alone
        ((16, 0, 0), (0, 0, 3), 0, False),      # ... excluded
        ((-32, 0, 8), (1, 0, 0), -1, False),    # in the plane of A and B: det = 0
        ((-32, 1, 8), (4, 0, 0), -1, False),
        ((8, 0, 8), (0, 0, 1), -1, False),      # the origin on A, upward: T = 0 on A, D is not above this point
        ((8, 0, 8), (0, 0, -1), -1, True),      # the origin on A, downward: C
        ((8, 0, 8), (0, 0, -1), 2, False),      # ... C excluded
        ((8, 0, 16), (0, 0, 1), -1, False),     # A behind the origin
        ((8, -16, 8), (0, 0, 1), -1, True),     # D and its duplicate above (x = 1/4, y = -1/2 is inside D)
        ((8, -16, 8), (0, 0, 1), 3, True),      # one of the pair excluded: the other still occludes
        ((8, -16, 8), (0, 0, 1), 4, True),
        ((8, -16, 30), (0, 0, 1), -1, False),   # above D
        ((32, 32, -16), (-1, -1, 0), -1, False),  # sliding in the plane of C
        ((24, 24, 0), (0, 0, 1), -1, True),     # through the hypotenuse of the oblique E (x + y = 3/2)
        ((24, 24, 0), (0, 0, 1), 5, False),
        ((25, 24, 0), (0, 0, 1), -1, False),    # one grid step outside it
    ]
    o = [np.array(a, dtype=np.float64) / 32.0 for a, _, _, _ in named]
    d = [np.array(b, dtype=np.float64) for _, b, _, _ in named]
    ex = [c for _, _, c, _ in named]
    want = [w for _, _, _, w in named]
    # a grid: every origin of a 5 x 5 x 3 lattice against 30 directions, zero components included, with a rotating exclusion
    dirs = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0), (1, 1, 0), (0, 1, -1), (-1, 0, 1), (1, 2, 3), (-3, 2, 1), (4, -4, 1), (1, -1, 4), (-2, -3, -4),
            (4, 4, 4), (0, 3, 4), (-4, 0, 3), (2, -1, 0), (1, 3, -2), (-1, -1, 2), (3, 0, -4), (0, -4, 1), (2, 2, -1), (-4, 1, 1), (1, -4, -2), (-2, 4, 3),
            (3, 3, 1), (-3, -1, 4), (0, 2, -3), (4, 1, 0), (-1, 4, -4), (2, 0, 1)]
    k = 0
    for x in (-24, -8, 0, 8, 24):
        for y in (-24, -16, 0, 8, 20):
            for zc in (-20, 0, 8):
                for dd in dirs:
                    o.append(np.array((x, y, zc), dtype=np.float64) / 32.0)
                    d.append(np.array(dd, dtype=np.float64))
                    ex.append(k % 7 - 1)
                    k += 1
    return p, f, np.array(o), np.array(d), np.array(ex), np.array(want)


def test_exact_queries_equal_the_float64_rule_everywhere():
    from drmnet_amd.mesh import build_bvh

    p, f, o, d, ex, want = exact_case()
    assert np.all(p * 64 == np.round(p * 64)) and np.abs(p).max() <= 1 and np.all(o * 32 == np.round(o * 32)) and np.abs(o).max() <= 1
    assert np.all(d == np.round(d)) and np.abs(d).max() <= 4 and (d == 0).any(axis=1).sum() >= 500
    ref = sr.occluded(p, f, o, d, ex)
    assert ref[:len(want)].tolist() == want.tolist()
    assert 0.1 <= ref.mean() <= 0.9
    mesh = bare(p, f)
    for bvh in (build_bvh(mesh), None):
        got = gpu_occluded(mesh, o, d, ex, bvh)
        assert np.array_equal(got, ref), (bvh is None, np.nonzero(got != ref)[0][:10])
    # no exclusion at all (a NULL exclude array)
    ref = sr.occluded(p, f, o, d)
    for bvh in ("auto", None):
        assert np.array_equal(gpu_occluded(mesh, o, d, None, bvh), ref)


# ---------------------------------------------------------------------------------------------- 2. the BVH changes nothing
def rays_for(p, f, blob, n=50000, seed=11):
    """seeded rays: random ones, axis-parallel directions, origins on and inside node boxes, origins on faces"""
    from drmnet_amd.mesh import decode_bvh

    rng = np.random.default_rng(seed)
    p32 = np.asarray(p, dtype=np.float32)
    t = decode_bvh(blob)
    part = n // 5
    o = [rng.uniform(-1.0, 1.0, (part, 3))]
    d = [rng.normal(size=(part, 3))]
    # axis-parallel and plane-parallel directions (one or two components exactly 0)
    dd = rng.normal(size=(part, 3))
    dd[np.arange(part), rng.integers(0, 3, part)] = 0.0
    half = part // 2
    dd[np.arange(half), (np.argmax(dd[:half] == 0, axis=1) + 1) % 3] = 0.0
    o.append(rng.uniform(-1.0, 1.0, (part, 3)))
    d.append(dd)
    # origins on node boxes: a random point of a random node's box moved onto one of its six planes (exactly: a float32 of the blob)
    node = rng.integers(0, len(t["skip"]), part)
    lo, hi = t["box_min"][node].astype(np.float64), t["box_max"][node].astype(np.float64)
    pt = lo + rng.uniform(0, 1, (part, 3)) * (hi - lo)
    axis, side = rng.integers(0, 3, part), rng.integers(0, 2, part)
    pt[np.arange(part), axis] = np.where(side[:, None] == 0, lo, hi)[np.arange(part), axis]
    ddd = rng.normal(size=(part, 3))
    ddd[::4, 0] = 0.0
    o.append(pt)
    d.append(ddd)
    # origins inside node boxes (their centres)
    node = rng.integers(0, len(t["skip"]), part)
    o.append(0.5 * (t["box_min"][node].astype(np.float64) + t["box_max"][node]))
    d.append(rng.normal(size=(part, 3)))
    # origins on faces: a vertex, an edge midpoint or an inner point of a kept face
    g = t["order"][rng.integers(0, len(t["order"]), part)]
    w = rng.dirichlet((1, 1, 1), part)
    w[::3] = (1.0, 0.0, 0.0)
    w[1::3] = (0.5, 0.5, 0.0)
    tri = p32[np.asarray(f)[g]].astype(np.float64)
    o.append(np.einsum("nk,nkc->nc", w, tri))
    d.append(rng.normal(size=(part, 3)))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32), np.concatenate([np.full(4 * part, -1), g]).astype(np.int32)


@pytest.mark.parametrize("name", ["soup", "two_spheres"])
def test_the_bvh_changes_no_answer(name):
    from drmnet_amd.mesh import build_bvh

    p, f = (SOUP[0], SOUP[1]) if name == "soup" else (SCENE[0], SCENE[2])
    mesh = bare(p, f)
    blob = build_bvh(mesh)
    o, d, ex = rays_for(p, f, blob)
    assert len(o) >= 50000 and (d == 0).any(axis=1).sum() >= 10000
    for exclude in (None, ex):
        with_bvh, brute = gpu_occluded(mesh, o, d, exclude, blob), gpu_occluded(mesh, o, d, exclude, None)
        print(f"{name}: {len(o)} rays, {with_bvh.mean():.3f} occluded with the BVH, {brute.mean():.3f} without")
        assert np.array_equal(with_bvh, brute), np.nonzero(with_bvh != brute)[0][:10]
        assert 0.1 <= brute.mean() <= 0.9
    # (an independent look at a subset: the float64 rule agrees wherever it is not marginal)
    sub = slice(0, len(o), 25)
    ref, marg = sr.occluded(np.asarray(p, dtype=np.float32), f, o[sub], d[sub], ex[sub], marginal=True)
    got = gpu_occluded(mesh, o, d, ex, blob)[sub]
    assert np.array_equal(got[~marg], ref[~marg]) and marg.mean() < 0.3


# ---------------------------------------------------------------------------------------------- 3. shading against the restatement
SHADING = [(v, r) for v in range(len(VIEWS)) for r in range(len(ROWS))]


def view_rot(v):
    return None if VIEWS[v] is None else rotation(VIEWS[v])


@functools.lru_cache(maxsize=None)
def scene_trace(v, r):
    """what the restatement of a (view, row) holds apart from the environment, computed once"""
    return sr.trace(*SCENE, ROWS[r], view_rot(v), FILM, FILM, S, Q)


@functools.lru_cache(maxsize=None)
def scene_ref(v, r, white):
    return sr.shade(scene_trace(v, r), None if white else ENV)


@functools.lru_cache(maxsize=None)
def scene_gpu(v, white, shadows=True):
    """the three BSDF rows of a view in one call"""
    views = None if VIEWS[v] is None else [VIEWS[v]] * 3
    return gpu_render(SCENE, ROWS, None if white else [ENV] * 3, views, shadows)[0]


@pytest.mark.parametrize("v,r", SHADING)
def test_shadowed_shading_matches_the_restatement(v, r):
    tr = scene_trace(v, r)
    # the comparison cannot empty itself: measured on the restatement alone
    marginal, unsafe, occl = tr["marginal"] / tr["traced"], tr["vis"]["unsafe"].mean(), tr["occluded"] / tr["traced"]
    assert marginal <= CAP and unsafe <= CAP and occl >= 0.01 and tr["traced"] >= 10000
    for white in (False, True):
        ref = scene_ref(v, r, white)
        share = ref["slack"].sum() / ref["image"].sum()
        safe = ~ref["unsafe_pixel"]
        gpu = scene_gpu(v, white)[r]
        over = np.maximum(np.abs(gpu - ref["image"]) - ref["slack"], 0.0)[:, safe]
        err = float(np.linalg.norm(over) / np.linalg.norm(ref["image"][:, safe]))
        print(f"view {v} row {r} white {white}: marginal rays {marginal:.4f}, unsafe samples {unsafe:.4f}, occluded {occl:.4f}, slack share {share:.4f}, "
              f"rel-L2 beyond the slack on safe pixels {err:.3g}")
        assert share <= CAP and safe.mean() >= 0.9 and (ref["image"][:, safe].sum(axis=0) > 0).sum() >= 50
        assert err <= 1e-5, (v, r, white, err)


@pytest.mark.parametrize("v", range(len(VIEWS)))
def test_the_shadow_is_there(v):
    for white in (False, True):
        lit, dark = scene_gpu(v, white, False), scene_gpu(v, white)
        for r in range(3):
            assert rel_l2(dark[r], lit[r]) > 1e-2, (v, r, white)
    if v == 0:
        # the ball casts a real shadow on the body: body samples that lose more than 10 % of their diffuse-lobe rays to the ball alone
        tr = scene_trace(0, 0)
        p, _, f = SCENE
        body = tr["face"] < 320
        lost = sr.occluded(p, f[320:], np.repeat(tr["origin"][body], Q * Q, axis=0), tr["l_diff"][body].reshape(-1, 3)).reshape(-1, Q * Q).mean(axis=1)
        assert (lost > 0.1).sum() >= 5


# ---------------------------------------------------------------------------------------------- 4. monotonic and neutral
@pytest.mark.parametrize("v", range(len(VIEWS)))
def test_shadowed_is_never_brighter(v):
    for white in (False, True):
        lit, dark = scene_gpu(v, white, False), scene_gpu(v, white)
        assert np.all(dark <= lit) and np.all(dark >= 0) and (dark < lit).sum() >= 100


def test_a_flat_shaded_convex_mesh_has_no_shadow():
    from test_shadow_cpu import flat_icosphere

    mesh = flat_icosphere()
    for view in (None, (0.6, 0.3, 1.0)):
        views = None if view is None else [view] * 3
        lit, dark = (gpu_render(mesh, ROWS, [ENV] * 3, views, s)[0] for s in (False, True))
        for r in range(3):
            slack = sr.render(*mesh, ROWS[r], ENV, None if view is None else rotation(view), FILM, FILM, S, Q)["slack"]
            diff = lit[r] - dark[r]
            assert np.all(diff >= 0) and np.all(diff <= slack * (1 + 1e-5) + 1e-7 * (slack > 0)) and np.all(diff[slack == 0] == 0), (view, r)
            assert (slack == 0).mean() > 0.5 and lit[r].max() > 0.1


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_shadowed_renders_are_reproducible_and_rows_are_independent():
    from drmnet_amd import _lib
    from drmnet_amd.mesh import render_mesh

    views = [(0.0, 0.0, 1.1), VIEWS[1], VIEWS[2]]
    envs = [ENV, 1.5 * ENV, ENV[:, ::-1].copy()]
    stacked = gpu_render(SCENE, ROWS, envs, views, True)
    again = gpu_render(SCENE, ROWS, envs, views, True)
    for a, b in zip(stacked, again):
        assert np.array_equal(a, b)
    for r in range(3):
        one = gpu_render(SCENE, ROWS[r:r + 1], envs[r:r + 1], views[r:r + 1], True)
        for a, b in zip(stacked, one):
            assert np.array_equal(a[r], b[0]), r
    assert not np.array_equal(stacked[0][0], stacked[0][1])
    # shadows=False is drm_render_mesh itself
    plain = gpu_render(SCENE, ROWS, envs, views, False)
    status, direct = raw_call(SCENE, shadowed=False, rows=ROWS, envs=envs, views=views)
    assert status == 0
    for a, b in zip(plain, direct):
        assert np.array_equal(a, b.astype(np.float64))
    assert not np.array_equal(plain[0], stacked[0])


# ---------------------------------------------------------------------------------------------- 6. arguments
def raw_call(mesh, shadowed=True, rows=(ROUGH,), envs=(ENV,), views=None, blob="build", blob_bytes=None, ws_bytes=None, H=FILM, W=FILM):
    """drm_render_mesh with shadows = 1 (or 0) through ctypes on sentinel-filled outputs: (status, outputs)"""
    import abi_call
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh
    from drmnet_amd.render import view_rotation

    lib = _lib.lib()
    obj = {k: t.to(DEV) for k, t in as_obj(*mesh).items()}
    B, V, F = len(rows), obj["vertex_positions"].shape[0], obj["faces"].shape[0]
    need = lib.drm_render_mesh_workspace_bytes(F, B, H, W, S)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    z = torch.tensor(rows, dtype=torch.float32, device=DEV)
    env = torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV).contiguous()
    view = None if views is None else view_rotation(torch.tensor(views, dtype=torch.float32)).to(DEV).contiguous()
    outs = [torch.full(s, -7.0, device=DEV) for s in ((B, 3, H, W), (B, 3, H, W), (B, 1, H, W), (B, H, W))]
    sh = abi_call.shading(B, z=z.data_ptr(), env=env.data_ptr(), EH=env.shape[1], EW=env.shape[2], view=_lib.ptr(view), quad=Q)
    dev_blob, nbytes = None, 0
    if shadowed:
        if isinstance(blob, str):
            blob = build_bvh(as_obj(*mesh))
        dev_blob = None if blob is None else blob.to(DEV)
        nbytes = (0 if blob is None else blob.numel()) if blob_bytes is None else blob_bytes
    m = abi_call.mesh_render(obj["vertex_positions"].data_ptr(), obj["vertex_normals"].data_ptr(), obj["faces"].data_ptr(), V, F,
                             [o.data_ptr() for o in outs], H, W, S, ws.data_ptr(), need if ws_bytes is None else ws_bytes, shadows=int(shadowed),
                             bvh=_lib.ptr(dev_blob), bvh_bytes=nbytes)
    status = abi_call.render_mesh(sh, m, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, [o.cpu().numpy() for o in outs]


def test_bad_shadow_arguments_launch_nothing():
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    ok, outs = raw_call(SCENE)
    assert ok == 0 and all(not np.any(o == -7.0) for o in outs)
    assert np.array_equal(outs[0][0].astype(np.float64), gpu_render(SCENE, [ROUGH], [ENV], None, True)[0][0])
    good = build_bvh(as_obj(*SCENE))
    other = build_bvh(as_obj(*mr.icosphere(1)))  # built for another F
    damaged = good.clone()
    damaged[0] ^= 0xFF  # the magic
    need = _lib.lib().drm_render_mesh_workspace_bytes(len(SCENE[2]), 1, FILM, FILM, S)
    INVALID, WORKSPACE = 1, 3
    for want, over in ((INVALID, dict(blob=None)), (INVALID, dict(blob=other)), (INVALID, dict(blob=damaged)),
                       (INVALID, dict(blob=good[:len(good) - 4].clone())),                      # truncated: shorter than its header says
                       (INVALID, dict(blob=good, blob_bytes=len(good) - 1)), (INVALID, dict(blob=good[:16].clone())),
                       (WORKSPACE, dict(ws_bytes=need - 1))):
        status, outs = raw_call(SCENE, **over)
        assert status == want, (want, status, {k: (v if not torch.is_tensor(v) else len(v)) for k, v in over.items()})
        assert all(np.all(o == -7.0) for o in outs)
    # the ray query checks its blob as well, and a bad one leaves the output alone
    lib = _lib.lib()
    obj = {k: t.to(DEV) for k, t in as_obj(*SCENE).items()}
    o = torch.zeros(8, 3, device=DEV)
    d = torch.ones(8, 3, device=DEV)
    out = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    for blob in (other, damaged):
        b = blob.to(DEV)
        status = lib.drm_mesh_occluded(obj["vertex_positions"].data_ptr(), obj["faces"].data_ptr(), obj["vertex_positions"].shape[0], len(SCENE[2]),
                                       b.data_ptr(), o.data_ptr(), d.data_ptr(), None, out.data_ptr(), 8, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert status == INVALID and bool((out == -7).all())
    with pytest.raises(RuntimeError):
        gpu_render(SCENE, [ROUGH], [ENV], None, True, bvh=other)


# ---------------------------------------------------------------------------------------------- 7. surface
def test_mesh_renderer_keeps_the_bvh_with_its_scene(monkeypatch):
    from drmnet_amd import mesh as mesh_mod
    from drmnet_amd.mesh import MeshRenderer, render_mesh

    builds = []
    real = mesh_mod.build_bvh
    monkeypatch.setattr(mesh_mod, "build_bvh", lambda obj: builds.append(1) or real(obj))
    obj = as_obj(*SCENE)
    env = torch.tensor(ENV, dtype=torch.float32)
    z = torch.tensor(ROUGH)
    view = (0.6, 0.3, 1.0)
    r = MeshRenderer(FILM, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q, shadows=True)
    first = r.rendering(z, NAMES6, env, obj=obj, channel_first=True)
    blob = r._bvh
    assert len(builds) == 1 and blob is not None and blob.is_cuda and torch.equal(blob.cpu(), real(obj))
    second = r.rendering(z, NAMES6, channel_first=True)
    assert len(builds) == 1 and r._bvh is blob and torch.equal(first, second)
    want = render_mesh(obj, z[None].to(DEV), NAMES6, env[None].to(DEV), image_size=FILM, view_from=torch.tensor([view]), quad=Q, shadows=True)[0][0]
    assert len(builds) == 2 and torch.equal(first, want)
    plain = MeshRenderer(FILM, init_view_from=view, brdf_param_names=list(NAMES6), quad=Q).rendering(z, NAMES6, env, obj=obj, channel_first=True)
    assert len(builds) == 2 and bool((first <= plain).all()) and not torch.equal(first, plain)
    # a new_scene mesh gets a BVH for that call only
    small = as_obj(*mr.icosphere(1))
    fresh = r.rendering(z, NAMES6, env, obj=small, new_scene=True, channel_first=True)
    assert len(builds) == 3 and r._bvh is blob
    assert torch.equal(fresh, render_mesh(small, z[None].to(DEV), NAMES6, env[None].to(DEV), image_size=FILM, view_from=torch.tensor([view]), quad=Q,
                                          shadows=True)[0][0])
    assert torch.equal(r.rendering(z, NAMES6, channel_first=True), first)


def test_synthesize_with_shadows(tmp_path):
    from drmnet_amd import file_io, synthesize

    torch.save(dict(as_obj(*SCENE)), tmp_path / "scene.pt")
    file_io.save_exr(tmp_path / "env.exr", ENV.astype(np.float32))
    images = {}
    for flag in ([], ["--shadows"]):
        out = tmp_path / ("out" + "".join(flag))
        synthesize.main(["--mesh", str(tmp_path / "scene.pt"), "--envmap", str(tmp_path / "env.exr"), "--z", *[str(x) for x in ROUGH], "--view_from", "0.6",
                         "0.3", "1.0", "--image_size", "24", "--refmap_res", "8", "--quad", str(Q), "--output_dir", str(out), *flag])
        assert all((out / n).exists() for n in ("image.exr", "normal.npy", "mask.png", "refmap.exr"))
        images[bool(flag)] = file_io.load_exr(out / "image.exr")
    assert images[True].shape == (24, 24, 3) and np.all(images[True] <= images[False]) and rel_l2(images[True], images[False]) > 1e-2

"""Measured BRDFs on the GPU (csrc/brdf_table.hip through drmnet_amd.merl, render.render_table, relight.render_normals_measured and the
command lines) against the float64 restatement tests/merl_ref.py.

Bars.  The export and the eval are held to drm_brdf_eval's rtol 1e-5 / atol 1e-6; a render to the 1e-5 rel-L2 of the sphere render
against its restatement (the kernel runs the same grids in fp32); convergence to the 2e-3 of the principled quadrature; the Lambertian
table to the CPU test's 2e-3.  The synthetic tables of the render tests are isotropic BRDFs: their dependence on phi_d vanishes where
theta_h or theta_d is 0, as any measured table's does (there phi_d turns a direction about the normal, or is undefined)."""
import functools

import numpy as np
import pytest
import torch

import merl_ref as mr
import relight_ref as rl
import render_ref as rr
from conftest import rel_l2
from drmnet_amd import merl
from test_gpu_render import eval_configs, smooth_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DIELECTRIC, METALLIC, MIXED = (0.0, 0.7, 0.5, 0.3, 0.5, 0.6), (1.0, 0.9, 0.6, 0.3, 0.3, 1.0), (0.3, 0.7, 0.5, 0.3, 0.8, 0.6)
VIEW = (0.6, 0.3, 1.0)
I, J, K = np.meshgrid(np.arange(90.0), np.arange(90.0), np.arange(180.0), indexing="ij")


def rotation(view_from):
    from drmnet_amd.render import view_rotation

    return view_rotation(torch.tensor([view_from], dtype=torch.float32))[0].double().numpy()


@functools.lru_cache(maxsize=None)
def exported(row):
    """the restatement's table of a row as the GPU is given it (float32), read-only"""
    t = mr.export(list(row)).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def smooth_table():
    """a synthetic smooth isotropic table: a broad lobe in theta_h, a falling term in theta_d, and an azimuthal term that vanishes at
    theta_h = 0 and theta_d = 0 and has period 180 in k (so the wrap 179 -> 0 is continuous)"""
    base = 0.25 + 0.6 * np.exp(-(I / 35.0) ** 2) + 0.15 * (J / 90.0) ** 2 + 0.1 * (I / 90.0) * (J / 90.0) * np.cos(2 * np.pi * K / 180.0)
    t = np.stack([base, 0.8 * base + 0.05, 0.6 * base + 0.02 * (J / 90.0)]).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def measured(name):
    from drmnet_amd.merl import MeasuredBSDF

    table = smooth_table() if name == "smooth" else exported({"dielectric": DIELECTRIC, "metallic": METALLIC, "mixed": MIXED}[name])
    return MeasuredBSDF(table, alpha=0.45 if name == "smooth" else None)


def affine_table():
    return np.stack([1.0 + c + 0.01 * I + 0.02 * J + 0.003 * K for c in range(3)]).astype(np.float32)


def index_table():
    flat = (I * 90 + J) * 180 + K
    return np.stack([flat + 0.25 * c for c in range(3)]).astype(np.float32)  # (exact in float32: below 2^22 in steps of 1/4)


def directions(n, seed):
    """n triples (normal, v, l) as float32, built on test_gpu_render.eval_configs: its first fifth grazing (v or l within ~0.6 degree of
    the horizon), the last third with l near reflect(v, n) (theta_h between 5e-4 and 5e-2), a twentieth left wherever it fell (mostly
    invalid: below the surface) and everything else turned into the normal's hemisphere"""
    _, nrm, v, l = (a.astype(np.float64) for a in eval_configs(n, seed))
    g = np.random.default_rng(seed + 100)
    free = slice(n // 5, n // 5 + n // 20)
    keep_v, keep_l = v[free].copy(), l[free].copy()
    v *= np.where(np.sum(nrm * v, 1, keepdims=True) < 0, -1.0, 1.0)
    k = n - n // 3
    refl = 2 * np.sum(nrm[k:] * v[k:], 1, keepdims=True) * nrm[k:] - v[k:]
    u = g.normal(size=(n - k, 3))
    l[k:] = refl + g.uniform(1e-3, 1e-1, size=(n - k, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    l *= np.where(np.sum(nrm * l, 1, keepdims=True) < 0, -1.0, 1.0)
    v[free], l[free] = keep_v, keep_l
    return [np.ascontiguousarray(a, dtype=np.float32) for a in (nrm, v, l)]


def from_coordinates(xh, xd, xp, seed):
    """(n, v, l) float32 whose table coordinates are (xh, xd, xp), each triple in a random frame"""
    g = np.random.default_rng(seed)
    th, td, pd = (xh / 90.0) ** 2 * (np.pi / 2), xd * (np.pi / 180), xp * (np.pi / 180)
    n = np.stack([-np.sin(th), np.zeros_like(th), np.cos(th)], -1)
    v = np.stack([np.sin(td) * np.cos(pd), np.sin(td) * np.sin(pd), np.cos(td)], -1)
    l = v * np.array([-1.0, -1.0, 1.0])
    q, _ = np.linalg.qr(g.normal(size=(len(xh), 3, 3)))
    q = q * np.sign(np.linalg.det(q))[:, None, None]
    return [np.ascontiguousarray(np.einsum("nij,nj->ni", q, a), dtype=np.float32) for a in (n, v, l)]


def upload(table):
    from drmnet_amd.merl import pack_table

    return torch.from_numpy(pack_table(table)).to(DEV)[None].contiguous()


def gpu_eval(tables, n, v, l, linear, table_of=None):
    """drm_merl_eval through ctypes: tables [NT, 90, 90, 180, 4] on the GPU -> [N, 3]"""
    from drmnet_amd import _lib

    t = [torch.from_numpy(a).to(DEV) for a in (n, v, l)]
    of = None if table_of is None else torch.tensor(table_of, dtype=torch.int32, device=DEV)
    out = torch.empty((len(n), 3), device=DEV)
    _lib.check(_lib.lib().drm_merl_eval(tables.data_ptr(), int(tables.shape[0]), _lib.ptr(of), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                        out.data_ptr(), len(n), int(linear), _lib.stream_ptr(DEV)))
    return out.cpu().numpy()


def f64(*arrays):
    return [a.astype(np.float64) for a in arrays]


# ---------------------------------------------------------------------------------------------- 1. export
def test_export_matches_the_restatement_on_the_whole_grid():
    from drmnet_amd import _lib

    rows = [DIELECTRIC, METALLIC, MIXED]
    z = torch.tensor(rows, dtype=torch.float32, device=DEV)
    out = torch.full((3, 90, 90, 180, 4), 7.0, device=DEV)
    _lib.check(_lib.lib().drm_brdf_to_merl(z.data_ptr(), 3, out.data_ptr(), _lib.stream_ptr(DEV)))
    got = out.cpu().numpy()
    assert not got[..., 3].any()
    for b, row in enumerate(rows):
        ref = mr.export(list(np.asarray(row, dtype=np.float32).astype(np.float64)))
        g = np.moveaxis(got[b, ..., :3], -1, 0)
        assert np.array_equal(g == -1, ref == -1) and np.array_equal((g == -1).any(0), (g == -1).all(0)), b
        print(f"row {b}: {int((ref[0] == -1).sum())} of {ref[0].size} entries below the horizon, peak {ref.max():.4g}")
        np.testing.assert_allclose(g, ref, rtol=1e-5, atol=1e-6)
        assert 0.05 < (ref[0] == -1).mean() < 0.5 and ref.max() > 0.3


# ---------------------------------------------------------------------------------------------- 2. eval
def test_linear_eval_is_exact_on_an_affine_table():
    T = affine_table()
    n, v, l = directions(100000, 11)
    got = gpu_eval(upload(T), n, v, l, True)
    n64, v64, l64 = f64(n, v, l)
    ref = mr.eval_table(T, n64, v64, l64, "linear")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    ok = (np.sum(n64 * v64, 1) > 0) & (np.sum(n64 * l64, 1) > 0)
    xh, xd, xp = mr.coordinates(n64[ok], v64[ok], l64[ok])
    inner = (xh < 89) & (xd < 89) & (xp < 179)
    want = np.stack([1.0 + c + 0.01 * xh + 0.02 * xd + 0.003 * xp for c in range(3)], -1) * np.sum(n64[ok] * l64[ok], 1)[:, None]
    np.testing.assert_allclose(got[ok][inner], want[inner], rtol=1e-5, atol=1e-6)
    print(f"{int(ok.sum())} valid of {len(n)}, {int(inner.sum())} away from the clamp and wrap cells, theta_h down to {np.degrees((xh.min() / 90) ** 2 * np.pi / 2):.3g} deg")
    assert 0.9 < ok.mean() < 0.99 and inner.mean() > 0.9 and not got[~ok].any() and xh.min() < 2.0


def test_nearest_eval_reads_the_bin_and_equals_the_restatement_exactly():
    T = index_table()
    tables = upload(T)
    # bin centres, the first and last bin of every axis among them
    ax = np.array([0, 1, 5, 45, 88, 89])
    i, j, k = (a.reshape(-1) for a in np.meshgrid(ax, ax, np.array([0, 1, 90, 178, 179]), indexing="ij"))
    n, v, l = from_coordinates(i + 0.5, j + 0.5, k + 0.5, 5)
    n64, v64, l64 = f64(n, v, l)
    ok = (np.sum(n64 * v64, 1) > 1e-3) & (np.sum(n64 * l64, 1) > 1e-3)
    # float32 cannot hold every corner of the grid: at theta_h = 0.003 degree and theta_d = 89.5 degrees its rounding of v and l turns the half
    # vector by more than a bin of phi_d.  Kept: the triples that, as float32, still sit within a quarter bin of their centre.
    with np.errstate(invalid="ignore"):
        x = np.stack(mr.coordinates(n64, v64, l64))
    ok &= (np.abs(x[0] - i - 0.5) < 0.25) & (np.abs(x[1] - j - 0.5) < 0.25) & (np.abs(x[2] - k - 0.5) < 0.25)
    assert ok.sum() >= 80
    for idx, last in ((i, 89), (j, 89), (k, 179)):
        assert {0, last} <= set(idx[ok])
    got = gpu_eval(tables, n[ok], v[ok], l[ok], False) / np.sum(n64[ok] * l64[ok], 1)[:, None]
    np.testing.assert_allclose(got, T[:, i[ok], j[ok], k[ok]].T, rtol=2e-6, atol=0)  # (the division by n.l in float64 of a float32 product)
    assert np.array_equal(np.rint(got[:, 0]), T[0, i[ok], j[ok], k[ok]])
    # random directions: no coordinate within 1e-9 of an integer, then equality with the restatement
    n, v, l = directions(100000, 12)
    n64, v64, l64 = f64(n, v, l)
    ok = (np.sum(n64 * v64, 1) > 0) & (np.sum(n64 * l64, 1) > 0)
    x = np.stack(mr.coordinates(n64[ok], v64[ok], l64[ok]))
    assert np.abs(x - np.rint(x)).min() > 1e-9
    got = gpu_eval(tables, n, v, l, False)
    ref = mr.eval_table(T, n64, v64, l64, "nearest").astype(np.float32)
    assert np.array_equal(got, ref)
    assert len(np.unique(got[:, 0])) > 50000


def test_negative_entries_read_zero_and_renormalise():
    T = affine_table()
    T[:, 20:30, 10:20, 50:70] = -1.0
    tables = upload(T)
    g = np.random.default_rng(13)
    xh, xd, xp = g.uniform(18, 32, 20000), g.uniform(8, 22, 20000), g.uniform(48, 72, 20000)
    n, v, l = from_coordinates(xh, xd, xp, 14)
    n64, v64, l64 = f64(n, v, l)
    cl = np.sum(n64 * l64, 1)
    assert (cl > 0.5).all() and (np.sum(n64 * v64, 1) > 0.5).all()
    ch, cd, cp = mr.coordinates(n64, v64, l64)
    inside = (ch >= 20) & (ch < 29) & (cd >= 10) & (cd < 19) & (cp >= 50) & (cp < 69)  # all eight corners in the block
    outside = (ch < 19) | (ch >= 30) | (cd < 9) | (cd >= 20) | (cp < 49) | (cp >= 70)  # none of them
    border = ~inside & ~outside
    assert inside.sum() > 500 and border.sum() > 2000 and outside.sum() > 2000
    for mode in ("nearest", "linear"):
        got = gpu_eval(tables, n, v, l, mode == "linear")
        np.testing.assert_allclose(got, mr.eval_table(T, n64, v64, l64, mode), rtol=1e-5, atol=1e-6)
        assert not got[inside].any() and (got[outside] > 0).all()
    lin = gpu_eval(tables, n, v, l, True)[border] / cl[border, None]
    # on the border the renormalised value is a mean of valid corners: within the affine table's range over them, never pulled toward 0 or -1
    lo = 1.0 + 0.01 * (np.floor(ch[border])) + 0.02 * np.floor(cd[border]) + 0.003 * np.floor(cp[border])
    assert (lin[:, 0] >= lo - 1e-5).all() and (lin[:, 0] <= lo + 0.033 + 1e-5).all()


def test_table_of_picks_the_table():
    a, b = affine_table(), index_table()
    tables = torch.cat([upload(a), upload(b)])
    n, v, l = directions(2000, 15)
    of = np.arange(2000) % 2
    got = gpu_eval(tables, n, v, l, False, of)
    assert np.array_equal(got[0::2], gpu_eval(upload(a), n[0::2], v[0::2], l[0::2], False))
    assert np.array_equal(got[1::2], gpu_eval(upload(b), n[1::2], v[1::2], l[1::2], False))


# ---------------------------------------------------------------------------------------------- 3. renders
R8 = 8
NAMES3 = ("dielectric", "metallic", "smooth")


@functools.lru_cache(maxsize=None)
def envs3():
    e = np.stack([smooth_env(16, 32, s) for s in range(3)])
    e[1] += 3.0 * (rr.env_dirs(16, 32)[0][..., 1:2] > 0.8)  # a sharp-edged light
    e = e.astype(np.float32)
    e.setflags(write=False)
    return e


def gpu_render(names, envs, res, **kw):
    from drmnet_amd.render import render_table

    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    return render_table([measured(n) for n in names], env, res=res, **kw).cpu().numpy()


@pytest.mark.parametrize("case", ["plain", "view", "flip"])
def test_render_matches_the_restatement(case):
    kw = {"plain": {}, "view": {"view_from": torch.tensor([VIEW] * 3)}, "flip": {"flip": True}}[case]
    out = gpu_render(NAMES3, envs3(), R8, **kw)
    assert out.shape == (3, 3, R8, R8)
    for b, name in enumerate(NAMES3):
        m = measured(name)
        ref = mr.render_table(m.table, m.alpha, envs3()[b].astype(np.float64), R8, Q=32, S=2, flip=case == "flip", rot=rotation(VIEW) if case == "view" else None)
        err = rel_l2(out[b], ref)
        print(f"{case} {name} (alpha {m.alpha:.3f}): rel-L2 {err:.3g}")
        assert err <= 1e-5, (name, err)
    if case != "plain":
        plain = gpu_render(NAMES3, envs3(), R8)
        assert rel_l2(out[2], plain[2]) > 1e-2 and rel_l2(out[0], plain[0]) > 1e-2


def test_render_converges():
    names = ("dielectric", "metallic", "mixed")
    env = [smooth_env(16, 32)] * 3
    a, b = gpu_render(names, env, 16), gpu_render(names, env, 16, quad=128)
    for k, name in enumerate(names):
        err = rel_l2(a[k], b[k])
        print(f"{name} (alpha {measured(name).alpha:.3f}): Q = 32 against Q = 128 rel-L2 {err:.3g}")
        assert err <= 2e-3, (name, err)


def test_render_invariants():
    from drmnet_amd.merl import MeasuredBSDF

    rho = 0.6
    lam = MeasuredBSDF(np.full((3, 90, 90, 180), rho / np.pi, dtype=np.float32))
    assert lam.alpha == 1.0
    from drmnet_amd.render import render_table

    img = render_table(lam, None, res=8).cpu().numpy()
    print(f"Lambertian table under a white map: max |pixel - rho| {np.abs(img - rho).max():.3g}")
    assert img.shape == (1, 3, 8, 8) and np.abs(img - rho).max() <= 2e-3
    views = torch.tensor([(0.0, 0.0, 1.1), VIEW, (-1.0, 0.2, 0.4)])
    a = gpu_render(NAMES3, envs3(), 16, view_from=views)
    assert np.array_equal(a, gpu_render(NAMES3, envs3(), 16, view_from=views))  # bitwise reproducible
    for r in range(3):
        one = gpu_render(NAMES3[r:r + 1], envs3()[r:r + 1], 16, view_from=views[r:r + 1])
        assert np.array_equal(a[r], one[0]), r  # a batch equals its rows rendered alone
    same = gpu_render(("metallic", "smooth", "metallic"), envs3()[[1, 0, 1]], 16)
    assert np.array_equal(same[0], same[2]) and not np.array_equal(same[0], same[1])
    # equal objects share one device table
    from drmnet_amd.merl import device_tables

    tables, table_of, alpha = device_tables([measured("metallic"), measured("smooth"), measured("metallic")], 3, DEV)
    assert tables.shape == (2, 90, 90, 180, 4) and table_of.tolist() == [0, 1, 0] and alpha.shape == (2,)
    assert measured("metallic").device_table(DEV) is measured("metallic").device_table(DEV)
    near = gpu_render(("metallic",), envs3()[:1], 16, lookup="nearest")
    assert 1e-4 < rel_l2(near[0], gpu_render(("metallic",), envs3()[:1], 16)[0]) < 0.1


# ---------------------------------------------------------------------------------------------- 4. normal maps
def test_normal_map_images_match_the_restatement():
    from drmnet_amd.relight import render_normals_measured
    from drmnet_amd.render import render_table

    normals, mask = rl.normal_map(5, H=12, W=10)
    mask[7, 3] = False  # a mask hole (row 0 already holds a zero normal, a NaN normal, n.z = 0 and a masked-out pixel)
    envs = torch.tensor(envs3(), device=DEV)
    for views in (None, torch.tensor([VIEW] * 3)):
        image, alpha = render_normals_measured(torch.tensor(normals, device=DEV), [measured(n) for n in NAMES3], envs, mask=torch.tensor(mask, device=DEV),
                                               view_from=views, quad=8)
        assert image.shape == (3, 3, 12, 10) and alpha.shape == (3, 12, 10)
        image, alpha = image.cpu().numpy(), alpha.cpu().numpy()
        _, drawn = rl.unit_normals(normals, mask)
        assert not drawn[7, 3] and not drawn[0, 0] and 40 <= drawn.sum() <= 100
        for b, name in enumerate(NAMES3):
            m = measured(name)
            ref, _ = mr.shade(m.table, m.alpha, envs3()[b].astype(np.float64), normals, mask, 8, None if views is None else rotation(VIEW))
            err = rel_l2(image[b][:, drawn], ref[:, drawn])
            print(f"view {views is not None} {name}: normal-map image rel-L2 {err:.3g}")
            assert err <= 1e-5, (name, err)
            assert np.array_equal(alpha[b], drawn.astype(np.float32)) and not image[b][:, ~drawn].any() and (image[b][:, drawn] > 0).all()
    # the centre pixel of an odd film sees n = (0, 0, 1) exactly: the sphere render at S = 1 and the normal map give the same bits
    one = torch.tensor([[[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]]], device=DEV)
    for name in ("metallic", "smooth"):
        sphere = render_table(measured(name), envs[:1], res=5, quad=16, subpixel=1)
        image, alpha = render_normals_measured(one, measured(name), envs[:1], quad=16)
        assert torch.equal(image[0, :, 0, 0], sphere[0, :, 2, 2]) and torch.equal(image[0, :, 0, 1], sphere[0, :, 2, 2]) and bool(alpha.all())
    # and every sphere normal, given as a float32 normal map, is the sphere render at S = 1 to rounding
    centres = torch.tensor(rr.sensor_normals(8, 1)[:, :, 0].astype(np.float32), device=DEV)
    sphere = render_table(measured("smooth"), envs[:1], res=8, quad=16, subpixel=1)
    image, _ = render_normals_measured(centres, measured("smooth"), envs[:1], quad=16)
    assert rel_l2(image.cpu(), sphere.cpu()) <= 1e-5


# ---------------------------------------------------------------------------------------------- 5. the Python surface
def test_python_surface(tmp_path):
    from drmnet_amd.render import PrincipledBSDF, eval_bsdf, visualize_bsdf

    m = measured("mixed")
    n, v, l = directions(3000, 16)
    for lookup in ("nearest", "linear"):
        got = eval_bsdf(m, n, l, v, lookup=lookup)  # (wo = light, wi = viewer)
        assert got.shape == (3000, 3) and np.isfinite(got).all() and got.max() > 0.1
        assert np.array_equal(got, gpu_eval(upload(m.table), n, v, l, lookup == "linear"))
    assert np.array_equal(eval_bsdf(m, n, l, v), eval_bsdf(m, n, l, v, lookup="nearest"))
    with pytest.raises(ValueError):
        eval_bsdf(m, n, l, v, lookup="cubic")
    fig, mask = visualize_bsdf(m, imsize=(64, 64))
    fig_p, mask_p = visualize_bsdf(PrincipledBSDF(MIXED), imsize=(64, 64))
    assert fig.shape == fig_p.shape == (64, 224, 3) and np.array_equal(mask, mask_p) and np.isfinite(fig).all()
    # both figures against the restatement on the layout's own vectors (one viewer vector broadcast over every pixel); the default lookup,
    # nearest, against the principled figure only: the figure's light angles put theta_d exactly on bin boundaries, where floor is rounding's
    from drmnet_amd.render import visualize_layout

    normal, light, _ = visualize_layout(30, (64, 64), 0)
    n64, l64 = normal[mask].astype(np.float64), light[mask].astype(np.float64)
    v64 = np.broadcast_to(np.array([0.0, 0.0, -1.0]), n64.shape)
    np.testing.assert_allclose(fig_p[mask], rr.eval_bsdf(list(MIXED), n64, v64, l64), rtol=1e-5, atol=1e-6)
    fig_l, _ = visualize_bsdf(m, imsize=(64, 64), lookup="linear")
    np.testing.assert_allclose(fig_l[mask], mr.eval_table(m.table, n64, v64, l64, "linear"), rtol=1e-5, atol=1e-6)
    lit = fig_p.sum(-1) > 1e-3
    print(f"figure of the exported table against the principled figure: rel-L2 {rel_l2(fig[lit], fig_p[lit]):.3g} (nearest), "
          f"{rel_l2(fig_l[lit], fig_p[lit]):.3g} (linear)")
    assert rel_l2(fig[lit], fig_p[lit]) < 0.1 and rel_l2(fig_l[lit], fig_p[lit]) < 0.01 and lit.mean() > 0.25
    # bsdf_to_merl keeps the reference's return shape; the file round trip
    t = merl.bsdf_to_merl(PrincipledBSDF(MIXED))
    assert t.shape == (90, 90, 180, 3) and t.dtype == np.float32
    np.testing.assert_allclose(np.moveaxis(t, -1, 0), exported(MIXED), rtol=1e-5, atol=1e-6)
    scaled = merl.bsdf_to_merl(PrincipledBSDF(MIXED), color_scale=True)
    valid = t[..., 0] >= 0
    np.testing.assert_allclose(scaled[valid] * merl.COLOR_SCALES, t[valid], rtol=1e-6)
    assert np.all(scaled[~valid] == -1)
    b = merl.MeasuredBSDF.from_principled(PrincipledBSDF(MIXED))
    merl.save_merl(b.table, tmp_path / "mixed.binary")
    back = merl.MeasuredBSDF.from_file(tmp_path / "mixed.binary")
    np.testing.assert_allclose(back.table, b.table, rtol=2e-7, atol=0)
    assert abs(back.alpha - b.alpha) < 1e-6 and 0.8 <= b.alpha / 0.64 <= 1.25


def test_the_command_lines_write_their_files(tmp_path):
    import os

    from conftest import GOLD
    from drmnet_amd import file_io, relight

    merl.main(["--z", *[str(x) for x in METALLIC], "--output", str(tmp_path / "est.binary"), "--figure", str(tmp_path / "est.png")])
    table = merl.load_merl(tmp_path / "est.binary")
    np.testing.assert_allclose(table, exported(METALLIC), rtol=1e-5, atol=1e-6)
    merl.main(["--input", str(tmp_path / "est.binary"), "--figure", str(tmp_path / "a.png")])
    from PIL import Image

    for name in ("est.png", "a.png"):
        img = Image.open(tmp_path / name)
        assert img.mode == "RGBA" and img.size == (1792, 512)
    a, b = (np.asarray(Image.open(tmp_path / name)).astype(np.int32) for name in ("est.png", "a.png"))
    assert np.abs(a - b).max() <= 1 and a[..., :3].max() > 100  # (the file holds the table to float32 rounding: at most one 8-bit level)
    # relight --merl on the sample's normal map
    normal = os.path.join(GOLD, "sample", "normal.npy")
    relight.main(["--input_normal", normal, "--merl", str(tmp_path / "est.binary"), "--quad", "8", "--output_dir", str(tmp_path / "out")])
    image = file_io.load_exr(tmp_path / "out" / "image.exr")
    nrm = torch.from_numpy(np.load(normal)).to(DEV)
    mask = torch.linalg.norm(nrm, dim=-1) > 0.5
    want, _ = relight.render_normals_measured(nrm.float(), merl.MeasuredBSDF.from_file(tmp_path / "est.binary"), None, mask=mask, quad=8)
    assert np.array_equal(image, want[0].permute(1, 2, 0).cpu().numpy()) and image.max() > 0.1 and (tmp_path / "out" / "image.png").exists()


def test_estimate_save_merl_writes_a_loadable_table(tmp_path):
    from drmnet_amd import estimate
    from test_render_cpu import NAMES6

    estimate.save_brdf_merl(tmp_path / "sample_brdf.binary", torch.tensor(DIELECTRIC, device=DEV), NAMES6)
    np.testing.assert_allclose(merl.load_merl(tmp_path / "sample_brdf.binary"), exported(DIELECTRIC), rtol=1e-5, atol=1e-6)
    # the command line on the tiny networks of test_gpu_estimate.py with the recorded draws: the flag adds one file, the table of sample_brdf.npy
    import os

    from conftest import GOLD, gold
    from test_gpu_estimate import tiny_models

    g = gold("estimate_chain")
    models = tiny_models(g, DEV)
    for m in models:
        m.set_precision("fp32")
    d = os.path.join(GOLD, "sample")
    hooks = {k: torch.from_numpy(g[s]).to(DEV) for k, s in (("cond_noise", "cond"), ("x_T", "x_T"), ("noise", "noise"), ("noise0", "noise0"),
                                                            ("step_noise", "step_noise"))}
    estimate.main(["--input_img", os.path.join(d, "image.exr"), "--input_normal", os.path.join(d, "normal.npy"), "--input_mask", os.path.join(d, "mask.png"),
                   "--output_dir", str(tmp_path / "out"), "--save_merl"], models=models, hooks=hooks)
    zK = np.load(tmp_path / "out" / "sample_brdf.npy")
    from drmnet_amd.render import get_bsdf

    row = get_bsdf(torch.tensor(zK), models[0].brdf_param_names).row
    np.testing.assert_allclose(merl.load_merl(tmp_path / "out" / "sample_brdf.binary"), mr.export(row), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------- 6. arguments
def raw_render(entry, tables="ok", NT=2, table_of=(0, 1, 0), alpha=(0.3, 0.5), quad=8, subpixel=1, EH=16, EW=32, out="ok"):
    """drm_render_refmap / drm_render_normals under tables through ctypes on sentinel-filled outputs: (status, message, outputs)"""
    import abi_call
    from drmnet_amd import _lib

    lib = _lib.lib()
    t = torch.cat([upload(affine_table()), upload(smooth_table())])
    of = None if table_of is None else torch.tensor(table_of, dtype=torch.int32, device=DEV)
    al = None if alpha is None else torch.tensor(alpha, dtype=torch.float32, device=DEV)
    env = torch.tensor(envs3(), device=DEV)
    tp = {"ok": t.data_ptr(), None: None, "misaligned": t.data_ptr() + 4}[tables]
    sh = abi_call.shading(3, tables=tp, NT=NT, table_of=_lib.ptr(of), alpha=_lib.ptr(al), linear=1, env=env.data_ptr(), EH=EH, EW=EW, quad=quad)
    if entry == "refmap":
        outs = [torch.full((3, 3, 8, 8), -7.0, device=DEV)]
        status = abi_call.render_refmap(sh, 1, 8, subpixel, 0, outs[0].data_ptr() if out else None, _lib.stream_ptr(DEV))
    else:
        nrm = torch.tensor(rl.normal_map(5)[0], device=DEV)
        outs = [torch.full((3, 3, 12, 12), -7.0, device=DEV), torch.full((3, 12, 12), -7.0, device=DEV)]
        status = abi_call.render_normals(sh, nrm.data_ptr(), None, 1, 12, 12, outs[0].data_ptr() if out else None, outs[1].data_ptr(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, (lib.drm_last_error() or b"").decode(), [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("entry", ["refmap", "normals"])
def test_bad_arguments_launch_nothing(entry):
    for over in (dict(), dict(table_of=None), dict(NT=1, table_of=(0, 0, 0), alpha=(1.0,))):
        status, _, outs = raw_render(entry, **over)
        assert status == 0 and all(not np.any(o == -7.0) for o in outs), over
    cases = [(dict(table_of=(0, 2, 0)), "table_of"), (dict(table_of=(0, -1, 0)), "table_of"), (dict(alpha=(0.3, 0.001)), "alpha"),
             (dict(alpha=(2.0, 0.5)), "alpha"), (dict(alpha=(0.3, float("nan"))), "alpha"), (dict(alpha=(float("inf"), 0.5)), "alpha"),
             (dict(alpha=None), "alpha"), (dict(tables=None), "tables"), (dict(tables="misaligned"), "tables"), (dict(NT=0), "NT"), (dict(quad=0), "quad"),
             (dict(quad=1025), "quad"), (dict(EH=0), "envmap")]
    if entry == "refmap":
        cases += [(dict(subpixel=0), "subpixel"), (dict(subpixel=17), "subpixel")]
    for over, word in cases:
        status, message, outs = raw_render(entry, **over)
        assert status != 0 and word in message, (over, status, message)
        assert all(np.all(o == -7.0) for o in outs), over


def test_bad_eval_and_export_arguments_launch_nothing():
    from drmnet_amd import _lib

    lib = _lib.lib()
    t = upload(affine_table())
    n, v, l = (torch.from_numpy(a).to(DEV) for a in directions(64, 17))
    out = torch.full((64, 3), -7.0, device=DEV)
    s = _lib.stream_ptr(DEV)
    bad_of = torch.full((64,), 1, dtype=torch.int32, device=DEV)
    for args, word in (((None, 1, None, n.data_ptr(), v.data_ptr(), l.data_ptr(), out.data_ptr(), 64, 1, s), "tables"),
                       ((t.data_ptr(), 1, bad_of.data_ptr(), n.data_ptr(), v.data_ptr(), l.data_ptr(), out.data_ptr(), 64, 1, s), "table_of"),
                       ((t.data_ptr(), 1, None, None, v.data_ptr(), l.data_ptr(), out.data_ptr(), 64, 1, s), "null"),
                       ((t.data_ptr(), 1, None, n.data_ptr(), v.data_ptr(), l.data_ptr(), out.data_ptr(), -1, 1, s), "N")):
        status = lib.drm_merl_eval(*args)
        torch.cuda.synchronize()
        assert status != 0 and word in lib.drm_last_error().decode(), (word, lib.drm_last_error())
        assert bool((out == -7.0).all())
    assert lib.drm_merl_eval(t.data_ptr(), 1, None, None, None, None, None, 0, 1, s) == 0  # no elements: nothing is read
    z = torch.tensor([DIELECTRIC], device=DEV)
    for args, word in (((None, 1, t.data_ptr(), s), "null"), ((z.data_ptr(), 0, t.data_ptr(), s), "rows"), ((z.data_ptr(), 1, None, s), "null")):
        assert lib.drm_brdf_to_merl(*args) != 0 and word in lib.drm_last_error().decode()

"""The reflectance-map forward model on the GPU (csrc/render.hip through drmnet_amd.render and DRMNet) against the float64
restatement in tests/render_ref.py: the BSDF value, the quadrature, its convergence, the conventions (mirror round trip) and the
DRMNet surface built on it (basis_r0, reconstruct, the BRDF figure)."""

import numpy as np
import pytest
import torch

import render_ref as rr
from conftest import rel_l2
from test_render_cpu import MIRROR, NAMES6, ROUND_TRIP_BAR, _smooth_refmap, round_trip_error

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def smooth_env(EH, EW, seed=0):
    d, _ = rr.env_dirs(EH, EW)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k = 0.1 * seed
    return np.stack([1 + 0.5 * x + 0.3 * y * y + k, 0.8 + 0.4 * z - 0.2 * x * y, 1.2 + 0.6 * y + 0.1 * x + k * z], -1)


def eval_configs(n, seed):
    """random (z, n, v, l) with a fifth of the rows grazing (v or l within ~0.6 degree of the horizon) and a third near-mirror"""
    g = np.random.default_rng(seed)

    def unit(k):
        a = g.normal(size=(k, 3))
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    nrm, v, l = unit(n), unit(n), unit(n)
    for w, sl in ((v, slice(0, n // 10)), (l, slice(n // 10, n // 5))):
        t = unit(n)[sl]
        t -= (t * nrm[sl]).sum(1, keepdims=True) * nrm[sl]
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        c = g.uniform(1e-4, 1e-2, size=(t.shape[0], 1))
        w[sl] = c * nrm[sl] + np.sqrt(1 - c * c) * t
    z = g.uniform(-0.1, 1.1, size=(n, 6))
    z[: n // 3, 4] = g.uniform(0, 0.1, size=n // 3)
    return [np.ascontiguousarray(a, dtype=np.float32) for a in (z, nrm, v, l)]


def test_brdf_eval_matches_the_restatement():
    from drmnet_amd import _lib

    z, n, v, l = eval_configs(100000, 7)
    t = [torch.from_numpy(a).to(DEV) for a in (z, n, v, l)]
    out = torch.empty((len(z), 3), device=DEV)
    _lib.check(_lib.lib().drm_brdf_eval(t[0].data_ptr(), len(z), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), out.data_ptr(), len(z),
                                        _lib.stream_ptr(DEV)))
    ref = rr.eval_bsdf(*(a.astype(np.float64) for a in (z, n, v, l)))
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)
    # eval_bsdf's argument order (wo = light, wi = viewer) and broadcasting of one BSDF over many directions
    from drmnet_amd.render import eval_bsdf, get_bsdf

    b = get_bsdf(torch.tensor([0.3, 0.9, 0.5, 0.1, 0.4, 0.6]), NAMES6)
    got = eval_bsdf(b, n[:1000], l[:1000], v[:1000])
    np.testing.assert_allclose(got, rr.eval_bsdf(np.array(b.row), n[:1000].astype(np.float64), v[:1000].astype(np.float64), l[:1000].astype(np.float64)),
                               rtol=1e-5, atol=1e-6)


def test_render_matches_the_restatement():
    from drmnet_amd.render import render

    g = np.random.default_rng(3)
    z = np.array([[0.0, 0.8, 0.5, 0.2, 0.3, 0.5], [1.0, 0.9, 0.6, 0.3, 0.05, 1.0], [0.4, 0.2, 0.7, 0.9, 0.8, 0.2], [1.0, 1.0, 1.0, 1.0, 0.0, 1.0]])
    envs = np.stack([smooth_env(32, 64, s) * g.uniform(0.5, 2.0) for s in range(4)])
    envs[1] += 3.0 * (rr.env_dirs(32, 64)[0][..., 1:2] > 0.8)  # a sharp-edged light
    out = render(torch.tensor(z, dtype=torch.float32), NAMES6, torch.tensor(envs, dtype=torch.float32), res=32).cpu().numpy()
    for b in range(4):
        assert rel_l2(out[b], rr.render_quadrature(z[b], envs[b], 32)) <= 1e-5, b
    # white environment at R = 128 (a few pixel rows of the restatement), and the flipped sensor
    white = render(torch.tensor([[0.2, 0.9, 0.4, 0.6, 0.35, 0.8]]), NAMES6, None, res=128).cpu().numpy()[0]
    rows = [0, 1, 50, 64, 127]
    n = rr.sensor_normals(128, 2)[rows]
    ref = rr._quadrature([0.2, 0.9, 0.4, 0.6, 0.35, 0.8], None, n, 32)
    assert rel_l2(white[:, rows], ref) <= 1e-5
    flip = render(torch.tensor(z[2:3], dtype=torch.float32), NAMES6, torch.tensor(envs[2:3], dtype=torch.float32), res=32, flip=True).cpu().numpy()[0]
    assert rel_l2(flip, rr.render_quadrature(z[2], envs[2], 32, flip=True)) <= 1e-5
    assert rel_l2(flip, out[2]) > 1e-2


@pytest.mark.parametrize("m", [0.0, 1.0])
def test_quadrature_converges(m):
    """default (Q, S) = (32, 2) against Q = 128 on a smooth map, and for r >= 0.3 against a texel-sum integral of the same pixels"""
    from drmnet_amd.render import render

    env = smooth_env(16, 32)
    rs = [0.0, 0.05, 0.2, 0.5, 1.0]
    z = torch.tensor([[m, 0.7, 0.5, 0.3, r, 0.6] for r in rs])
    envs = torch.tensor(env, dtype=torch.float32)[None].expand(len(rs), -1, -1, -1)
    a = render(z, NAMES6, envs, res=16).cpu().numpy()
    b = render(z, NAMES6, envs, res=16, quad=128).cpu().numpy()
    for k, r in enumerate(rs):
        assert rel_l2(a[k], b[k]) <= 2e-3, (r, rel_l2(a[k], b[k]))
        if r >= 0.3:
            rows = list(range(0, 16, 2))
            ts = rr.render_texel_sum(z[k].numpy().astype(np.float64), env, 16, rows=rows)
            assert rel_l2(a[k][:, rows], ts) <= 2e-3, (r, rel_l2(a[k][:, rows], ts))


def tiny_drmnet(image_size, **kw):
    from drmnet_amd.drmnet import DRMNet
    from oracle import unet as ou

    unet_t = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(ou.TINY_UNET_CFG)}
    enc_t = {"target": "ldm.modules.diffusionmodules.openaimodel.EncoderUNetModel", "params": dict(ou.TINY_ENC_CFG)}
    kw = dict(dict(z0=MIRROR, brdf_param_names=NAMES6), **kw)
    return DRMNet(illnet_config=unet_t, refnet_config=enc_t, max_timesteps=4, image_size=image_size, concat_mode=True, use_ema=False, **kw).to(DEV)


def test_mirror_round_trip_through_reconstruct():
    from drmnet_amd.dataset import BaseDataset

    m = tiny_drmnet(128)
    m.ds = BaseDataset(size=128, transform_func="log", clamp_before_exp=20)
    r = _smooth_refmap(128)
    err = []
    for img in (r, r[:, :, ::-1].copy()):
        Lr0 = m.ds.transform(torch.tensor(img, dtype=torch.float32, device=DEV)[None])
        rec = m.reconstruct(Lr0, torch.tensor([MIRROR], dtype=torch.float32, device=DEV))
        assert rec.shape == (1, 3, 128, 128)
        err.append(round_trip_error(rec[0].cpu().double().numpy(), r))
    assert err[0] <= ROUND_TRIP_BAR and err[1] >= 10 * ROUND_TRIP_BAR, err


def test_drmnet_basis_and_brdf_figures(tmp_path):
    from drmnet_amd.estimate import save_brdf_png

    assert torch.equal(tiny_drmnet(32).basis_r0, torch.ones(3, 32, 32, device=DEV))  # the default stays exactly ones
    m = tiny_drmnet(64, basis_r0="render")
    env = m.r0toenvmap(torch.ones(1, 3, 64, 64, device=DEV))  # first GPU use renders the basis
    assert not m._basis_pending and env.shape == (1, 64, 128, 3)
    cv = rr.sensor_normals(64, 1)[:, :, 0, 2]
    assert np.abs(m.basis_r0.cpu().numpy()[:, cv >= 0.2] - 1).max() <= 5e-3
    z0 = [0.3, 0.9, 0.6, 0.2, 0.6, 0.5]  # tinted, rough, half metallic
    m2 = tiny_drmnet(32, basis_r0="render", z0=z0)
    assert rel_l2(m2.render_basis_r0().cpu(), rr.render_quadrature(z0, None, 32)) <= 1e-5
    grid = m2.get_visualized_brdf_grid(torch.tensor([z0, MIRROR], dtype=torch.float32))
    assert grid.shape == (256, 448, 3) and np.isfinite(grid).all()
    save_brdf_png(tmp_path / "sample_brdf.png", torch.tensor(z0, device=DEV), NAMES6)
    from PIL import Image
    from drmnet_amd.render import visualize_layout

    img = Image.open(tmp_path / "sample_brdf.png")
    assert img.mode == "RGBA" and img.size == (1792, 512)
    alpha = np.asarray(img)[..., 3]
    assert np.array_equal(alpha == 255, visualize_layout()[2]) and set(np.unique(alpha)) <= {0, 255}


def test_renders_are_bitwise_reproducible():
    from drmnet_amd.render import RefMapRenderer

    r = RefMapRenderer(64, brdf_param_names=NAMES6)
    env = torch.tensor(smooth_env(32, 64), dtype=torch.float32, device=DEV)
    z = torch.tensor([0.5, 0.8, 0.3, 0.6, 0.4, 0.7], device=DEV)
    a = r.rendering(z, NAMES6, env)
    b = r.rendering(z, NAMES6)  # envmap=None: the scene keeps the last map
    assert a.shape == (64, 64, 3) and torch.equal(a, b)
    c = r.render(torch.stack([z, z]), NAMES6, torch.stack([env, env]))
    assert torch.equal(c[0], c[1]) and torch.equal(c[0], a.permute(2, 0, 1))

"""CPU checks of the reflectance-map forward model: the host parameter mapping, the YAML wiring of the renderer, and the float64
restatement (tests/render_ref.py) the GPU tests compare the kernels against -- its physics and its sensor / envmap conventions."""
import os

import numpy as np
import pytest
import torch

import render_ref as rr
from conftest import ROOT

NAMES6 = ["metallic.value", "base_color.value.R", "base_color.value.G", "base_color.value.B", "roughness.value", "specular"]
MIRROR = [1, 1, 1, 1, 0, 1]  # the shipped z0


def test_parameter_names_map_to_the_canonical_row():
    from drmnet_amd.render import canonical_rows, get_bsdf

    z = torch.tensor([[0.3, 0.2, 0.5, 0.9, 0.4, 0.7], [1.5, -0.2, 0.5, 2.0, 0.1, -1.0]])
    assert torch.equal(canonical_rows(z, NAMES6), z.clip(0, 1))
    assert canonical_rows(torch.tensor([0.25]), ["specular"]).tolist() == [0, 0, 0, 0, 0, 0.25]  # the package default: black dielectric
    row = canonical_rows(torch.tensor([0.6, 0.3, 0.8]), ["roughness", "base_color.value", "metallic"]).tolist()
    assert row == pytest.approx([0.8, 0.3, 0.3, 0.3, 0.6, 1.0])
    assert canonical_rows(torch.tensor([0.5, 0.5]), ["roughness.value", "metallic.value"]).tolist() == [0.5, 0, 0, 0, 0.5, 1.0]
    assert get_bsdf(torch.tensor(MIRROR, dtype=torch.float32), NAMES6).row == [1.0, 1.0, 1.0, 1.0, 0.0, 1.0]
    for bad in ("spec_tint", "sheen", "clearcoat", "anisotropic", "spec_trans", "flatness", "eta"):
        with pytest.raises(NotImplementedError):
            canonical_rows(torch.zeros(2), ["metallic", bad])
    with pytest.raises(NotImplementedError):
        canonical_rows(torch.zeros(2), ["base_color.value.R", "base_color.value.G"])
    with pytest.raises(ValueError):
        canonical_rows(torch.zeros(3), ["metallic"])


def test_shipped_config_builds_the_renderer_without_a_gpu():
    from drmnet_amd.config import instantiate_from_config, load_config
    from drmnet_amd.drmnet import DRMNet
    from drmnet_amd.render import RefMapRenderer
    from oracle import unet as ou

    params = dict(load_config(os.path.join(ROOT, "configs/drmnet/eval_drmnet.yaml"))["model"]["params"])
    r = instantiate_from_config(params["renderer_config"])
    assert isinstance(r, RefMapRenderer)
    assert r.image_size == (128, 128) and r.refmap_res == 128 and r.spp == 256 and r.envmap_size == (1000, 2000)
    params.update(illnet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(ou.TINY_UNET_CFG)},
                  refnet_config={"target": "ldm.modules.diffusionmodules.openaimodel.EncoderUNetModel", "params": dict(ou.TINY_ENC_CFG)},
                  use_ema=False, ckpt_path=None)
    m = DRMNet(**params)
    assert isinstance(m.renderer, RefMapRenderer)
    assert torch.equal(m.basis_r0, torch.ones(3, 128, 128))
    m2 = DRMNet(**dict(params, basis_r0="render"))  # rendered on first GPU use, not here
    assert m2._basis_pending and not torch.cuda.is_initialized()
    with pytest.raises(ValueError):
        DRMNet(**dict(params, basis_r0="mitsuba"))
    with pytest.raises(NotImplementedError):
        RefMapRenderer(64, return_normal=True)
    with pytest.raises(NotImplementedError):
        RefMapRenderer(64, init_view_from=[1, 0, 0])


def _random_pairs(n, seed):
    g = np.random.default_rng(seed)

    def unit(k):
        a = g.normal(size=(k, 3))
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    nrm, v, l = unit(n), unit(n), unit(n)
    v = np.where((v * nrm).sum(1, keepdims=True) < 0, -v, v)
    l = np.where((l * nrm).sum(1, keepdims=True) < 0, -l, l)
    z = g.uniform(size=(n, 6))
    return z, nrm, v, l


def test_restatement_is_reciprocal():
    z, nrm, v, l = _random_pairs(20000, 1)
    cv, cl = (nrm * v).sum(1, keepdims=True), (nrm * l).sum(1, keepdims=True)
    np.testing.assert_allclose(rr.eval_bsdf(z, nrm, v, l) / cl, rr.eval_bsdf(z, nrm, l, v) / cv, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("r", [0.0, 0.05, 0.2, 0.5, 1.0])
def test_white_furnace(r):
    """m = 1, c = 1 (F = 1): the reflected fraction of a white environment never exceeds 1, and is ~1 for the mirror away from the rim."""
    P = rr.render_quadrature([1, 1, 1, 1, r, 0.5], None, 16)
    assert P.max() <= 1.0 + 1e-9
    if r == 0.0:
        cv = rr.sensor_normals(16, 1)[:, :, 0, 2]
        assert P[:, cv >= 0.2].min() >= 0.995


def test_diffuse_closed_form():
    """m = 0, s = 0 (eta = 1: no specular), r = 0, white environment, at n = v: the albedo of the Disney diffuse is c (1 - 1/42)."""
    c = np.array([0.8, 0.5, 0.2])
    z = [0, *c, 0, 0]
    P = rr._quadrature(z, None, np.array([0.0, 0.0, 1.0]).reshape(1, 1, 1, 3), 256)[:, 0, 0]
    np.testing.assert_allclose(P, 41 / 42 * c, rtol=1e-4)  # (the midpoint rule in u1 meets a square root at the horizon)
    # the same integral straight from eval_bsdf on a fine (theta, phi) grid
    th = (np.arange(4000) + 0.5) * (np.pi / 2) / 4000
    l = np.stack([np.sin(th), np.zeros_like(th), np.cos(th)], -1)
    f = rr.eval_bsdf(z, np.array([0, 0, 1.0]), np.array([0, 0, 1.0]), l)
    np.testing.assert_allclose((f * (np.sin(th) * (np.pi / 2) / 4000 * 2 * np.pi)[:, None]).sum(0), 41 / 42 * c, rtol=1e-6)


@pytest.mark.parametrize("imsize,step,start", [((512, 512), 30, 0), ((128, 128), 30, 0), ((64, 48), 45, 10)])
def test_visualize_layout(imsize, step, start):
    from drmnet_amd.render import visualize_layout

    normal, wo, mask = visualize_layout(step, imsize, start)
    w, h = imsize
    k = len(range(start, 180, step))
    assert mask.shape == (h, (w * (k + 1)) // 2) and normal.shape == wo.shape == mask.shape + (3,)
    # a pixel is in the figure when it lies on one of the k discs of radius w / 2 centred half a width apart
    y = 2.0 * (np.arange(h)[:, None] + 0.5) / w - 1.0
    cols = np.arange(mask.shape[1])[None, :]
    inside = np.zeros_like(mask)
    for i in range(k):
        x = 2.0 * (cols - (i * w) // 2 + 0.5) / w - 1.0
        inside |= (x >= -1) & (x <= 1) & (x * x + y * y <= 1.0)
    assert int(mask.sum()) == int(inside.sum()) and np.array_equal(mask, inside)
    assert np.allclose(np.linalg.norm(normal[mask], axis=-1), 1, atol=1e-5) and (normal[mask][:, 2] <= 0).all()
    if imsize == (512, 512):
        assert mask.shape == (512, 1792)


def _smooth_refmap(R):
    p = (np.arange(R) + 0.5) / R
    Y, X = np.meshgrid(p, p, indexing="ij")
    return np.stack([1 + 0.6 * X + 0.2 * Y * Y, 0.7 + 0.5 * X * Y + 0.3 * Y, 1.3 - 0.4 * X * X + 0.2 * Y], 0)


ROUND_TRIP_BAR = 2e-3  # rel-L2 over the pixels with n.v >= 0.3


def round_trip_error(rendered, r):
    cv = rr.sensor_normals(r.shape[-1], 1)[:, :, 0, 2]
    sel = cv >= 0.3
    return float(np.linalg.norm((rendered - r)[:, sel]) / np.linalg.norm(r[:, sel]))


def test_mirror_round_trip_pins_the_conventions():
    """The mirror z0 renders mirmap2envmap(r) back to r: the sensor and the envmap share mirmap2envmap's geometry.  r mirrored
    left-right must miss by far more."""
    from oracle import transforms as ot

    R = 32
    r = _smooth_refmap(R)
    err = []
    for img in (r, r[:, :, ::-1].copy()):
        env = ot.mirmap2envmap(torch.from_numpy(img)[None].float(), (R, 2 * R), channels_last=True)[0].double().numpy()
        err.append(round_trip_error(rr.render_quadrature(MIRROR, env, R), r))
    assert err[0] <= ROUND_TRIP_BAR and err[1] >= 10 * ROUND_TRIP_BAR, err

"""The light-sampled render on the GPU (drm_render_refmap with light samples through drmnet_amd.render, DRMNet and validate) against its float64
restatement tests/light_ref.py and, on the sun scene of tests/golden/render_light_sun.npz, against the texel-sum integral.

Not yet run on an MI355X: the bar against the restatement is the 1e-5 the plain render is held to; each test prints its
figures before it asserts.  The render's per-lane sum compiled for the host meets the restatement at 5e-8 ... 1.8e-6 on these kinds of rows."""
import os

import numpy as np
import pytest
import torch

import light_ref as lr
from conftest import rel_l2
from test_forward_cpu import ENC_T, NAMES6, UNET_T
from test_render_light_cpu import random_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The plain render meets its restatement at 1e-5 (test_render_matches_the_restatement); the lit render starts from the same bar.
RESTATEMENT_BAR = 1e-5
Z4 = np.array([[0.0, 0.8, 0.5, 0.2, 0.3, 0.5], [1.0, 0.9, 0.6, 0.3, 0.05, 1.0], [0.4, 0.2, 0.7, 0.9, 0.8, 0.2], [1.0, 1.0, 1.0, 1.0, 0.0, 1.0]])


def t32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32)


def f32(a):
    """what the GPU is given, as float64 for the restatement"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def hot_envs():
    """random-valued 32 x 64 maps with two hot texels each, so no CDF boundary lands on a dyadic sample"""
    spots = [[(9, 33, 3e4), (20, 40, 600.0)], [(14, 5, 8e3), (3, 60, 2e3)], [(25, 17, 1e4), (16, 63, 900.0)], [(11, 48, 2e4), (12, 50, 5e3)]]
    return f32(np.stack([random_env(32, 64, 10 + b, spots[b]) for b in range(4)]))


def raw_lit(z, L, env, view, B, R, M, ws=None, ws_bytes=None, out=None, quad=32, flip=0):
    """drm_render_refmap itself with light_samples = M: (status, out).  ws = False: no light workspace at all (NULL, 0 bytes)"""
    import abi_call
    from drmnet_amd import _lib

    lib = _lib.lib()
    EH, EW = (int(env.shape[1]), int(env.shape[2])) if env is not None else (0, 0)
    if ws is False:
        ws_bytes = 0
    elif ws is None:
        n = int(lib.drm_render_light_workspace_bytes(B, EH, EW, M))
        ws = torch.empty((max(n, 8) // 8,), dtype=torch.float64, device=DEV)
        ws_bytes = n if ws_bytes is None else ws_bytes
    out = torch.empty((L * B, 3, R, R), device=DEV) if out is None else out
    sh = abi_call.shading(B, z=z.data_ptr(), env=_lib.ptr(env), EH=EH, EW=EW, view=_lib.ptr(view), quad=quad, light_samples=M,
                          lws=None if ws is False else ws.data_ptr(), lws_bytes=ws_bytes)
    st = abi_call.render_refmap(sh, L, R, 2, flip, out.data_ptr(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return st, out


def test_lit_render_matches_the_restatement():
    """four z (the mirror among them) from +z, two of them through a view, one flipped"""
    from drmnet_amd.render import render, view_rotation

    envs, R = hot_envs(), 12
    z = f32(Z4)
    out = render(t32(z), NAMES6, t32(envs), res=R, light_samples=1024).cpu().numpy()
    errs = [rel_l2(out[b], lr.render_mis(z[b], envs[b], R, M=1024)) for b in range(4)]
    view_from = f32([[0.7, 0.3, 0.9], [-1.0, -0.4, 0.2]])
    rots = view_rotation(torch.tensor(view_from)).double().numpy()
    seen = render(t32(z[[0, 2]]), NAMES6, t32(envs[[0, 2]]), res=R, light_samples=256, view_from=t32(view_from)).cpu().numpy()
    errs += [rel_l2(seen[k], lr.render_mis(z[b], envs[b], R, M=256, rot=rots[k])) for k, b in enumerate((0, 2))]
    flipped = render(t32(z[2:3]), NAMES6, t32(envs[2:3]), res=R, light_samples=256, flip=True).cpu().numpy()[0]
    errs.append(rel_l2(flipped, lr.render_mis(z[2], envs[2], R, M=256, flip=True)))
    print("lit render against the restatement (z0 z1 z2 mirror | view z0 z2 | flipped z2):", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= RESTATEMENT_BAR, errs
    assert rel_l2(seen[0], out[0]) > 1e-2 and rel_l2(flipped, out[2]) > 1e-2


def test_lit_render_meets_the_texel_sum_where_the_quadrature_does_not():
    from drmnet_amd.render import render

    sun = np.load(os.path.join(GOLD, "render_light_sun.npz"))
    z, R = t32(sun["z"]), int(sun["R"])
    envs = t32(sun["env"])[None].expand(len(z), -1, -1, -1)
    lit = render(z, NAMES6, envs, res=R, light_samples=1024).cpu().numpy()
    plain = render(z, NAMES6, envs, res=R, light_samples=0).cpu().numpy()
    for k in range(len(z)):
        assert float(z[k, 4]) >= 0.5
        e_lit, e_plain = rel_l2(lit[k], sun["texel4"][k]), rel_l2(plain[k], sun["texel4"][k])
        print(f"z {z[k].tolist()}: light_samples 1024 {e_lit:.3e}  light_samples 0 {e_plain:.3e}")
        assert e_lit <= 2e-3 and e_plain > 5e-2, (k, e_lit, e_plain)


def test_without_light_samples_it_is_the_old_path_bit_for_bit():
    from drmnet_amd import _lib
    from drmnet_amd.render import canonical_rows, render, view_rotation

    envs = t32(hot_envs()[:2])
    z = t32(np.stack([Z4[:2], Z4[2:]]))  # [L = 2, B = 2, 6]
    view_from = t32([[0.7, 0.3, 0.9], [0.0, 0.0, 1.0]])
    rows = canonical_rows(z, NAMES6).reshape(-1, 6).contiguous().to(DEV)
    env_d, view_d = envs.to(DEV), view_rotation(view_from).to(DEV)
    old = torch.empty((4, 3, 8, 8), device=DEV)
    for view in (None, view_d):
        assert raw_lit(rows, 2, env_d, view, 2, 8, 0, ws=False, out=old)[0] == 0  # the plain render: no light samples, no workspace
        got = render(z, NAMES6, envs, res=8, light_samples=0, view_from=None if view is None else view_from)
        assert torch.equal(got.reshape(4, 3, 8, 8), old)
        st, raw = raw_lit(rows, 2, env_d, view, 2, 8, 0, ws=torch.empty(1, dtype=torch.float64, device=DEV), ws_bytes=0)
        assert st == 0 and torch.equal(raw, old)
    # no map: the white environment, whatever light_samples says (no workspace is asked for)
    assert raw_lit(rows, 2, None, None, 2, 8, 0, ws=False, out=old)[0] == 0
    assert torch.equal(render(z, NAMES6, None, res=8, light_samples=1024).reshape(4, 3, 8, 8), old)
    st, raw = raw_lit(rows, 2, None, None, 2, 8, 1024, ws=torch.empty(1, dtype=torch.float64, device=DEV), ws_bytes=0)
    assert st == 0 and torch.equal(raw, old)


def test_lit_renders_are_reproducible_and_stack_row_by_row():
    from drmnet_amd.render import render

    envs = t32(hot_envs()[:2])
    z = t32(np.stack([Z4[[0, 1]], Z4[[2, 3]], Z4[[1, 0]]]))  # [L = 3, B = 2, 6]
    view_from = t32([[0.7, 0.3, 0.9], [-1.0, -0.4, 0.2]])
    a = render(z, NAMES6, envs, res=10, light_samples=256, view_from=view_from)
    b = render(z, NAMES6, envs, res=10, light_samples=256, view_from=view_from)
    assert a.shape == (3, 2, 3, 10, 10) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    for l in range(3):
        assert torch.equal(render(z[l], NAMES6, envs, res=10, light_samples=256, view_from=view_from), a[l])
    assert torch.equal(render(z[0, 1:], NAMES6, envs[1:], res=10, light_samples=256, view_from=view_from[1:])[0], a[0, 1])
    # two identical rows of a batch give identical maps
    twin = render(z[0, :1].expand(2, -1), NAMES6, envs[:1].expand(2, -1, -1, -1), res=10, light_samples=256)
    assert torch.equal(twin[0], twin[1])


def test_polar_lights():
    """a hot texel in the first and one in the last texel row: the half cells at the poles"""
    from drmnet_amd.render import render

    env = f32(random_env(16, 32, 5, [(0, 7, 5e3), (15, 20, 2e4)]))
    z = f32(Z4[[0, 2]])
    view_from = f32([[0.1, 0.9, 0.4], [0.2, -0.8, 0.5]])  # looking down from near the poles: the lights are on the film
    from drmnet_amd.render import view_rotation

    rots = view_rotation(torch.tensor(view_from)).double().numpy()
    out = render(t32(z), NAMES6, t32(env)[None].expand(2, -1, -1, -1), res=8, light_samples=512, view_from=t32(view_from)).cpu().numpy()
    assert np.isfinite(out).all()
    errs = [rel_l2(out[k], lr.render_mis(z[k], env, 8, M=512, rot=rots[k])) for k in range(2)]
    print("polar lights against the restatement:", errs)
    assert max(errs) <= RESTATEMENT_BAR, errs


def test_a_black_map_in_the_batch_renders_as_the_plain_quadrature():
    from drmnet_amd.render import render

    envs = hot_envs()[:3].copy()
    envs[1] = 0.0
    envs[2] = -envs[2]  # all non-positive: no light technique either
    z = t32(Z4[:3])
    lit = render(z, NAMES6, t32(envs), res=8, light_samples=256)
    plain = render(z, NAMES6, t32(envs), res=8, light_samples=0)
    assert bool(torch.isfinite(lit).all())
    assert bool((lit[1] == 0).all()) and float((lit[1] - plain[1]).abs().max()) <= 1e-6
    assert rel_l2(lit[2], plain[2]) <= 1e-6
    assert rel_l2(lit[0], plain[0]) > 1e-3  # the lit map of the batch did get its light samples


def test_argument_checks_launch_nothing():
    from drmnet_amd import _lib
    from drmnet_amd.render import render

    lib = _lib.lib()
    env = t32(hot_envs()[:1]).to(DEV)
    z = t32(Z4[:1]).to(DEV)
    need = int(lib.drm_render_light_workspace_bytes(1, 32, 64, 64))
    assert need >= 64 * 28 + 8 * 33 and int(lib.drm_render_light_workspace_bytes(2, 32, 64, 64)) == 2 * need
    ws = torch.empty((need // 8 + 1,), dtype=torch.float64, device=DEV)
    for M, nbytes in ((100, need), (32, need), (1 << 17, need), (-64, need), (64, need - 8), (64, 0)):
        assert M == 64 or int(lib.drm_render_light_workspace_bytes(1, 32, 64, M)) == 0
        out = torch.full((1, 3, 4, 4), -7.0, device=DEV)
        st, _ = raw_lit(z, 1, env, None, 1, 4, M, ws=ws, ws_bytes=nbytes, out=out)
        assert st != 0 and lib.drm_last_error() and bool((out == -7.0).all()), (M, nbytes)
    st, out = raw_lit(z, 1, env, None, 1, 4, 64, ws=ws, ws_bytes=need)
    assert st == 0 and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        render(z, NAMES6, env, res=4, light_samples=100)


def test_validation_step_inherits_light_samples_from_the_renderer_config():
    from drmnet_amd.dataset import BaseDataset
    from drmnet_amd.drmnet import DRMNet
    from drmnet_amd.render import RefMapRenderer

    cfg = {"target": "drmnet_amd.render.RefMapRenderer", "params": {"refmap_res": 16, "brdf_param_names": NAMES6, "light_samples": 256}}
    m = DRMNet(illnet_config=UNET_T, refnet_config=ENC_T, renderer_config=cfg, concat_mode=True, gamma=0.9, epsilon=1e-3, z0=[1, 1, 1, 1, 0, 1],
               brdf_param_names=NAMES6, image_size=16, max_timesteps=6, use_ema=False, sigma=0.02, refmap_input_scaler=0.12, loss_type="l2",
               l_refmap_weight=10.0, l_refcode_weight=0.1)
    assert isinstance(m.renderer, RefMapRenderer) and m.renderer.light_samples == 256
    m.ds = BaseDataset(16, "log", clamp_before_exp=20)
    m = m.to(DEV).set_precision("f16x3")
    gen = torch.Generator().manual_seed(3)
    zK = torch.tensor([[0.0, 0.7, 0.5, 0.3, 0.5, 0.6], [0.4, 0.7, 0.5, 0.3, 1.0, 0.2]])
    K, k, zk, zkm1 = m.get_schedule(zK, z0=m._z0, normalized_k=torch.rand((2,), generator=gen), return_zkm1=True)
    sun = t32(np.load(os.path.join(GOLD, "render_light_sun.npz"))["env"])
    batch = {"zK": zK, "K": K, "k": k, "zk": zk, "zkm1": zkm1, "envmap_name": ["sun0", "sun1"], "view_from": t32([[0.0, 0.0, 1.0], [0.5, 0.0, 0.8]]),
             "envmap": torch.stack([sun, sun.flip(1)])}
    lit = m.validation_step(batch, 0, seed=11)
    m.renderer.light_samples = 0
    plain = m.validation_step(batch, 0, seed=11)
    assert sorted(lit) == sorted(plain) and all(bool(torch.isfinite(v)) for v in lit.values())
    assert not torch.equal(lit["val/loss_refmap"], plain["val/loss_refmap"]) and not torch.equal(lit["val/loss"], plain["val/loss"])

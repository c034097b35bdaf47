"""What the sphere / envmap warps promise without a GPU: the float64 restatement tests/warp_ref.py agrees with the reference's own outputs
(tests/golden/warps.npz), no golden case sits on the azimuth seam, the frame vectors a batched call hands the kernel are those of the
per-item calls, the four entries are declared, and the command line pairs --gt_envmap with --gt_view_from."""
import os
import re

import numpy as np
import pytest
import torch

import warp_ref as wr
from conftest import ROOT, gold, rel_l2

# the project's stated tolerance for this arithmetic chain (trig, then grid_sample, on white noise): tests/test_gpu_transforms.py
WARP_TOL = 1e-5
NEW_SYMBOLS = ("drm_envmap2mirmap", "drm_rotate_envmap", "drm_mirimg2envmap", "drm_refmap2refimg")


@pytest.fixture(scope="module")
def cases():
    return wr.golden_cases(gold("warps"))


def test_the_restatement_matches_the_reference(cases):
    """the reference runs in fp32 and this in float64: 0.4e-6 to 2.4e-6 rel-L2 where measured, asserted at WARP_TOL"""
    seen = set()
    for case, x, kw, want, mask in cases:
        fn = case["fn"]
        seen.add(fn)
        if fn == "refmap2refimg_torch":
            got, disc = wr.refmap2refimg(x if x.ndim == 4 else x[None], kw.get("radius"))
            got = got if x.ndim == 4 else got[0]
            assert mask is None or np.array_equal(disc, mask)
            assert np.all(got[..., ~disc] == 0) and np.all(want[..., ~disc] == 0)
        else:
            got = getattr(wr, fn)(x, **kw)
        err = rel_l2(got, want)
        print(f"{case['out']}: rel-L2 {err:.2e}")
        assert got.shape == want.shape and err < WARP_TOL, (case, err)
    assert seen == {"envmap2mirmap", "rotate_envmap", "mirimg2envmap", "refmap2refimg_torch"}


def test_no_golden_case_sits_on_the_azimuth_seam(cases):
    wrapped = [c for c, *_ in cases if c["fn"] in ("envmap2mirmap", "rotate_envmap")]
    assert len(wrapped) >= 15 and all("seam_margin" in c for c in wrapped)
    for c in wrapped:
        assert c["seam_margin"] >= 1e-4, c
    # the stored figure is what the restatement measures
    c = wrapped[0]
    kw = {k: v for k, v in c["kwargs"].items() if k != "log_scale_interpolation"}
    assert wr.seam_margin(wr.envmap2mirmap_positions(32, 64, **kw)[2]) == pytest.approx(c["seam_margin"], rel=1e-9)


def test_pool_windows_are_torchs():
    x = torch.randn((3, 32, 32), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for shape in ((16, 16), (10, 10), (8, 16), (32, 32), (5, 7)):
        assert np.allclose(wr.adaptive_avg_pool(x.numpy(), shape), torch.nn.functional.adaptive_avg_pool2d(x, shape).numpy(), rtol=0, atol=1e-14)


def test_batched_frames_are_the_per_item_frames():
    from drmnet_amd import transform as t

    v = torch.nn.functional.normalize(torch.randn((6, 3), generator=torch.Generator().manual_seed(2)), dim=-1)
    v[0] = torch.tensor([1.0, 0.0, 0.0])  # dot(view, top) == 0: top is kept as given for this item alone
    for build in (t.envmap2mirmap_frames, t.mirimg2envmap_frames):
        batched = build(6, view_from=v)
        assert torch.equal(batched, torch.cat([build(1, view_from=v[i]) for i in range(6)]))
        assert torch.equal(batched[0], build(1, view_from=[1, 0, 0])[0])
    e = t.envmap2mirmap_frames(1)[0]  # top, view, top x view; zenith, left edge, -(zenith x left edge)
    assert e.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, -1], [0, 1, 0], [0, 0, -1], [1, 0, 0]]
    assert t.envmap2mirmap_frames(1, flip_horizontal=True)[0, 2].tolist() == [0, 0, 1]
    r = t.rotate_envmap_frames(2, [0, 1, 0], [0, 0, -1], v[:2], v[2:4])
    assert torch.equal(r[1], t.rotate_envmap_frames(1, [0, 1, 0], [0, 0, -1], v[1], v[3])[0]) and r.shape == (2, 6, 3)
    with pytest.raises(ValueError):
        t.envmap2mirmap_frames(2, view_from=v[:3])
    with pytest.raises(ValueError):
        t.rotate_envmap(torch.zeros(1, 3, 4, 8))  # no target frame


def test_the_entries_are_declared_and_the_abi_version_stays():
    from drmnet_amd import _lib

    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 4 and re.search(r"#define DRM_ABI_VERSION 4\b", header)
    assert "sphere_warp.hip" in __import__("drmnet_amd.build", fromlist=["SOURCES"]).SOURCES


def test_gt_envmap_and_gt_view_from_come_as_a_pair(capsys):
    from drmnet_amd import estimate

    base = ["--input_img", "i.exr", "--input_normal", "n.npy"]
    for argv in (["--gt_envmap", "e.exr"], ["--gt_view_from", "0", "0", "1"]):
        with pytest.raises(SystemExit) as e:
            estimate.parse_args(base + argv)
        assert e.value.code == 2 and "--gt_envmap" in capsys.readouterr().err
    a = estimate.parse_args(base + ["--gt_envmap", "e.exr", "--gt_view_from", "0.6", "0.3", "1"])
    assert str(a.gt_envmap) == "e.exr" and a.gt_view_from == [0.6, 0.3, 1.0]
    a = estimate.parse_args(base)
    assert a.gt_envmap is None and a.gt_view_from is None

"""What the normal-map images (drmnet_amd.relight: drm_render_normals, drm_image_from_refmap) promise without a GPU: the two entries are
declared and exported, the restated lookup coordinates invert the sensor, image_errors reduces as documented, and every argument error of the
two functions and of both command lines is raised before a GPU is touched."""
import os

import numpy as np
import pytest
import torch

import relight_ref as rl
import render_ref as rr
from conftest import ROOT
from drmnet_amd import _lib, relight
from test_render_cpu import NAMES6

ROUGH = [0.0, 0.8, 0.5, 0.2, 0.5, 0.5]


def test_both_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    L = _lib.lib()
    for name in ("drm_render_normals", "drm_image_from_refmap"):
        assert name + "(" in header and name in _lib.SYMBOLS and hasattr(L, name)
    assert L.drm_render_normals.argtypes[0]._type_ is _lib.Shading and len(L.drm_image_from_refmap.argtypes) == 13
    assert L.drm_abi_version() == 4


@pytest.mark.parametrize("R", [1, 7, 16, 128])
def test_the_lookup_coordinates_invert_the_sensor(R):
    n = rr.sensor_normals(R, 1, False)[:, :, 0]
    ti, tj = rl.texel_coordinates(n, R)
    I, J = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    assert np.abs(ti - I).max() <= 1e-12 and np.abs(tj - J).max() <= 1e-12
    # and the restated lookup at the texel centres is the map
    v = np.random.default_rng(R).uniform(0.1, 2.0, size=(3, R, R))
    image, alpha, _ = rl.lookup(v, None, n, None)
    assert alpha.all() and np.abs(image - v).max() <= 1e-11


def test_the_restatement_skips_what_the_header_says():
    nrm = np.array([[[0, 0, 0], [np.nan, 0, 1], [1, 0, 0], [0, 0, 2]], [[0, 0, -1], [np.inf, 0, 1], [0.3, 0.4, 0.5], [0, 3, 4]]], dtype=np.float64)
    mask = np.ones((2, 4), dtype=bool)
    mask[1, 3] = False
    n, drawn = rl.unit_normals(nrm, mask)
    assert drawn.tolist() == [[False, False, False, True], [False, False, True, False]]
    assert np.array_equal(n[0, 3], [0, 0, 1]) and abs(np.linalg.norm(n[1, 2]) - 1) < 1e-15 and not n[~drawn].any()
    image, d2 = rl.shade(ROUGH, None, nrm, mask, 4)
    assert np.array_equal(d2, drawn) and (image[:, drawn] > 0).all() and not image[:, ~drawn].any()


def test_image_errors_on_hand_made_images():
    b = np.random.default_rng(0).uniform(0.5, 2.0, size=(4, 5, 3))
    mask = np.zeros((4, 5), dtype=bool)
    mask[1:3, 1:4] = True
    same = relight.image_errors(b, b, mask)
    assert same == {"n": 6, "rel_l2": 0.0, "scale": 1.0, "rel_l2_scaled": 0.0, "rmse_log10": 0.0, "n_log": 18}
    twice = relight.image_errors(torch.tensor(2 * b), b, torch.tensor(mask))  # tensors are brought over
    assert twice["rel_l2"] == pytest.approx(1.0, abs=1e-15) and twice["scale"] == pytest.approx(0.5, abs=1e-15)
    assert twice["rel_l2_scaled"] <= 1e-15 and twice["rmse_log10"] == pytest.approx(np.log10(2.0), abs=1e-15) and twice["n_log"] == 18
    black = relight.image_errors(np.zeros_like(b), b, mask)
    assert black["rel_l2"] == 1.0 and black["scale"] == 0.0 and black["rel_l2_scaled"] == 1.0 and black["n_log"] == 0 and black["rmse_log10"] == 0.0
    # what lies outside the mask does not count; a partly black image counts its positive entries only in the log figure
    a = b.copy()
    a[0, 0] = 1e6
    a[1, 1, 0] = 0.0
    part = relight.image_errors(a, b, mask)
    assert part["n"] == 6 and part["n_log"] == 17 and part["rel_l2"] == pytest.approx(b[1, 1, 0] / np.linalg.norm(b[mask]), rel=1e-12)
    empty = relight.image_errors(b, b, np.zeros((4, 5), dtype=bool))
    assert empty == {"n": 0, "rel_l2": 0.0, "scale": 0.0, "rel_l2_scaled": 0.0, "rmse_log10": 0.0, "n_log": 0}
    with pytest.raises(ValueError):
        relight.image_errors(b, b[:3], mask)
    with pytest.raises(ValueError):
        relight.image_errors(b.transpose(2, 0, 1), b.transpose(2, 0, 1), mask)


def test_render_normals_argument_errors_come_before_the_gpu():
    nrm, z = torch.zeros(4, 5, 3), torch.tensor([ROUGH, ROUGH])
    bad = [dict(normals=torch.zeros(4, 5)), dict(normals=torch.zeros(4, 5, 4)), dict(normals=torch.zeros(3, 4, 5, 3)),  # Bn = 3, B = 2
           dict(normals=torch.zeros(0, 5, 3)), dict(normals=np.zeros((4, 5, 3))), dict(z=torch.tensor(ROUGH)), dict(z=torch.zeros(2, 5)),
           dict(mask=torch.ones(5, 4)), dict(mask=torch.ones(2, 4, 5)), dict(normals=torch.zeros(2, 4, 5, 3), mask=torch.ones(4, 5)),
           dict(light_samples=100), dict(light_samples=32), dict(light_samples=-64), dict(light_samples=1 << 17), dict(quad=0), dict(quad=1025),
           dict(envmaps=torch.zeros(1, 8, 16, 3)), dict(envmaps=torch.zeros(2, 8, 16)), dict(view_from=[[0.0, 1.0, 0.0]] * 2),
           dict(view_from=[[0.0, 0.0, 1.0]])]
    for over in bad:
        a = dict(normals=nrm, z=z, mask=None, envmaps=None, view_from=None, quad=8, light_samples=0)
        a.update(over)
        with pytest.raises(ValueError):
            relight.render_normals(a["normals"], a["z"], NAMES6, a["envmaps"], mask=a["mask"], view_from=a["view_from"], quad=a["quad"],
                                   light_samples=a["light_samples"])
    # well-formed CPU tensors: there is no CPU path
    for over in (dict(), dict(envmaps=torch.zeros(2, 8, 16, 3)), dict(normals=torch.zeros(2, 4, 5, 3), mask=torch.ones(2, 4, 5), light_samples=64)):
        a = dict(normals=nrm, z=z, mask=None, envmaps=None, light_samples=0)
        a.update(over)
        with pytest.raises(RuntimeError, match="GPU only"):
            relight.render_normals(a["normals"], a["z"], NAMES6, a["envmaps"], mask=a["mask"], light_samples=a["light_samples"])


def test_image_from_refmap_argument_errors_come_before_the_gpu():
    ref, nrm = torch.zeros(3, 8, 8), torch.zeros(4, 5, 3)
    bad = [dict(refmap=torch.zeros(8, 8)), dict(refmap=torch.zeros(3, 8, 9)), dict(refmap=torch.zeros(8, 8, 3)), dict(refmap=np.zeros((3, 8, 8))),
           dict(refmap=torch.zeros(2, 3, 8, 8), normals=torch.zeros(3, 4, 5, 3)),  # Br = 2, Bn = 3
           dict(refmask=torch.ones(8, 9)), dict(refmask=torch.ones(2, 8, 8)), dict(refmap=torch.zeros(2, 3, 8, 8), refmask=torch.ones(8, 8)),
           dict(normals=torch.zeros(4, 5)), dict(mask=torch.ones(5, 4))]
    for over in bad:
        a = dict(refmap=ref, normals=nrm, mask=None, refmask=None)
        a.update(over)
        with pytest.raises(ValueError):
            relight.image_from_refmap(a["refmap"], a["normals"], mask=a["mask"], refmask=a["refmask"])
    for over in (dict(), dict(refmap=torch.zeros(2, 3, 8, 8), refmask=torch.ones(2, 8, 8)), dict(normals=torch.zeros(2, 4, 5, 3), mask=torch.ones(2, 4, 5))):
        a = dict(refmap=ref, normals=nrm, mask=None, refmask=None)
        a.update(over)
        with pytest.raises(RuntimeError, match="GPU only"):
            relight.image_from_refmap(a["refmap"], a["normals"], mask=a["mask"], refmask=a["refmask"])


def test_command_line_argument_errors_come_before_the_gpu(tmp_path, monkeypatch):
    from drmnet_amd import file_io

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (reaching the render would be a RuntimeError here, not a ValueError)
    np.save(tmp_path / "n.npy", np.zeros((4, 5, 3), dtype=np.float32))
    np.save(tmp_path / "flat.npy", np.zeros((4, 5), dtype=np.float32))
    file_io.save_png(tmp_path / "m.png", np.ones((5, 4, 3), dtype=np.float32))
    file_io.save_exr(tmp_path / "i.exr", np.ones((4, 6, 3), dtype=np.float32))
    base = ["--input_normal", str(tmp_path / "n.npy"), "--z", *[str(v) for v in ROUGH], "--output_dir", str(tmp_path / "out")]
    for extra in (["--light_samples", "100"], ["--light_samples", "-64"], ["--quad", "0"], ["--view_from", "0", "1", "0"],
                  ["--input_mask", str(tmp_path / "m.png")], ["--input_img", str(tmp_path / "i.exr")]):
        with pytest.raises(ValueError):
            relight.main(base + extra)
    with pytest.raises(ValueError):
        relight.main(["--input_normal", str(tmp_path / "flat.npy")] + base[2:])
    for argv in (base[2:], base[:2] + base[8:], base[:8], base + ["--z", "1", "2"]):  # a required option is missing; --z takes six values
        with pytest.raises(SystemExit):
            relight.main(argv)
    with pytest.raises(RuntimeError, match="no GPU is visible"):
        relight.main(base)
    assert not (tmp_path / "out").exists()


def test_estimate_keeps_its_command_line():
    from pathlib import Path

    from drmnet_amd import estimate

    old = estimate.parser().parse_args(["--input_img", "a.exr", "--input_normal", "n.npy", "--input_mask", "m.png", "--obsnet_base_path", "o.yaml",
                                        "--drmnet_base_path", "d.yaml", "--output_dir", "out"])
    assert (old.input_img, old.input_normal, old.input_mask, old.obsnet_base_path, old.drmnet_base_path, old.output_dir) == tuple(
        Path(p) for p in ("a.exr", "n.npy", "m.png", "o.yaml", "d.yaml", "out"))
    assert old.rerender is False
    none = estimate.parser().parse_args([])
    assert none.input_mask is None and none.output_dir == Path("./outputs/") and none.obsnet_base_path == Path("./configs/obsnet/eval_obsnet.yaml")
    assert none.drmnet_base_path == Path("./configs/drmnet/eval_drmnet.yaml") and none.rerender is False
    assert estimate.parser().parse_args(["--rerender"]).rerender is True
    with pytest.raises(SystemExit):
        estimate.parser().parse_args(["--rerender", "yes"])

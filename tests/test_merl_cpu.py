"""CPU-only checks of the measured-BRDF path (drmnet_amd/merl.py, csrc/brdf_table.hip): the MERL file format, the packed device layout,
the proxy roughness, and -- on the float64 restatement tests/merl_ref.py alone -- the conventions of the table render: an exported
principled row rendered under its table against the principled render of that row, and the Lambertian known answer.  Nothing here needs a GPU.

Bars and the figures the restatement gives: alpha / r^2 in [0.8, 1.25] (measured 0.883 .. 1.051 over the ten rows); the table render of an
exported row within rel-L2 5e-3 of the principled quadrature (measured 2.1e-3 and 1.4e-3: the table's discretisation; a wrong azimuth
convention or a lost cosine is above 5e-2); the Lambertian table within 2e-3 of rho (measured 5.1e-4)."""
import functools
import os
import struct

import numpy as np
import pytest

import merl_ref as mr
import render_ref as rr
from conftest import ROOT, rel_l2
from drmnet_amd import merl  # (the product module under test: every check here is about it or about the rule it implements)

ROW_A, ROW_B = [0.0, 0.7, 0.5, 0.3, 0.5, 0.6], [0.3, 0.7, 0.5, 0.3, 0.8, 0.6]


def smooth_env(EH=16, EW=32):
    d, _ = rr.env_dirs(EH, EW)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([1 + 0.5 * x + 0.3 * y * y, 0.8 + 0.4 * z - 0.2 * x * y, 1.2 + 0.6 * y + 0.1 * x], -1)


@functools.lru_cache(maxsize=None)
def exported(row):
    t = mr.export(list(row))
    t.setflags(write=False)
    return t


def merl_bytes():
    """a MERL file whose doubles are a known function of the flat index: value(q) = q / 7 - 1000"""
    n = 3 * mr.NH * mr.ND * mr.NP
    vals = np.arange(n, dtype=np.float64) / 7.0 - 1000.0
    return struct.pack("<iii", 90, 90, 180) + struct.pack(f"<{n}d", *vals), vals


def test_file_format_round_trips(tmp_path):
    raw, vals = merl_bytes()
    (tmp_path / "a.binary").write_bytes(raw)
    t = merl.load_merl(tmp_path / "a.binary")
    assert t.shape == (3, 90, 90, 180) and t.dtype == np.float32
    want = (vals.reshape(3, 90, 90, 180).astype(np.float32) * mr.SCALES.astype(np.float32).reshape(3, 1, 1, 1))
    assert np.array_equal(t, want)
    # a value sits where (colour, theta_h, theta_d, phi_d) says: flat index ((c 90 + i) 90 + j) 180 + k
    for c, i, j, k in ((0, 0, 0, 0), (1, 2, 3, 4), (2, 89, 89, 179), (1, 0, 89, 0)):
        q = ((c * 90 + i) * 90 + j) * 180 + k
        assert t[c, i, j, k] == np.float32(np.float32(vals[q]) * np.float32(mr.SCALES[c]))
    # save_merl of what the file holds reproduces the bytes (from the unrounded values: float32 has rounded t)
    merl.save_merl(vals.reshape(3, 90, 90, 180) * mr.SCALES.reshape(3, 1, 1, 1), tmp_path / "b.binary")
    back = (tmp_path / "b.binary").read_bytes()
    assert back[:12] == raw[:12] and len(back) == len(raw)
    np.testing.assert_allclose(np.frombuffer(back[12:], dtype="<f8"), vals, rtol=1e-15, atol=0)
    # load(save(x)) is x to float32 rounding
    merl.save_merl(t, tmp_path / "c.binary")
    np.testing.assert_allclose(merl.load_merl(tmp_path / "c.binary"), t, rtol=2e-7, atol=0)
    for header in ((90, 90, 179), (90, 90, 360), (0, 0, 0)):
        (tmp_path / "bad.binary").write_bytes(struct.pack("<iii", *header) + raw[12:])
        with pytest.raises(ValueError, match="invalid BRDF file"):
            merl.load_merl(tmp_path / "bad.binary")
    with pytest.raises(ValueError):
        merl.save_merl(np.zeros((3, 90, 90)), tmp_path / "d.binary")


def test_packed_layout_round_trips():
    g = np.random.default_rng(0)
    t = g.uniform(0.0, 2.0, size=(3, 90, 90, 180)).astype(np.float32)
    t[:, 80:, 70:, :] = -1.0
    t[1, 3, 4, 5] = -0.5  # one negative channel marks the whole entry
    p = merl.pack_table(t)
    assert p.shape == (90, 90, 180, 4) and p.dtype == np.float32 and p.flags["C_CONTIGUOUS"] and not p[..., 3].any()
    assert np.array_equal(p[7, 8, 9, :3], t[:, 7, 8, 9]) and np.array_equal(p[3, 4, 5], [-1, -1, -1, 0]) and np.array_equal(p[85, 75, 11], [-1, -1, -1, 0])
    back = merl.unpack_table(p)
    valid = (t >= 0).all(axis=0)
    assert np.array_equal(back[:, valid], t[:, valid]) and np.all(back[:, ~valid] == -1)
    b = merl.MeasuredBSDF(t, alpha=0.3)
    assert b.alpha == 0.3 and b.table.shape == (3, 90, 90, 180) and "0.3" in repr(b)
    with pytest.raises(ValueError):
        merl.MeasuredBSDF(t[:, :10])
    with pytest.raises(ValueError):
        merl.MeasuredBSDF(t, alpha=0.0)


def test_coordinates_return_the_grid_at_its_nodes():
    """the grid bsdf_to_merl samples is the set of integer coordinates, in any frame: node directions, rotated, come back as (i, j, k)"""
    g = np.random.default_rng(1)
    i, j, k = g.integers(1, 90, 400), g.integers(1, 89, 400), g.integers(0, 180, 400)
    th, td, pd = (i / 90.0) ** 2 * (np.pi / 2), j * (np.pi / 180), k * (np.pi / 180)
    n = np.stack([-np.sin(th), np.zeros_like(th), np.cos(th)], -1)
    v = np.stack([np.sin(td) * np.cos(pd), np.sin(td) * np.sin(pd), np.cos(td)], -1)
    l = v * np.array([-1.0, -1.0, 1.0])
    rot, _ = np.linalg.qr(g.normal(size=(3, 3)))
    rot *= np.sign(np.linalg.det(rot))
    xh, xd, xp = mr.coordinates(n @ rot.T, v @ rot.T, l @ rot.T)
    assert np.abs(xh - i).max() < 1e-8 and np.abs(xd - j).max() < 1e-8
    assert np.abs(np.mod(xp - k + 90, 180) - 90).max() < 1e-8
    # and so linear returns an exported table's own entries there
    T = exported(tuple(ROW_B))
    keep = (T[0, i, j, k] >= 0) & (xp > 0.5) & (xp < 179.5)
    got = mr.lookup(T, (n @ rot.T)[keep], (v @ rot.T)[keep], (l @ rot.T)[keep], "linear")
    ok = (np.sum((n @ rot.T)[keep] * (v @ rot.T)[keep], -1) > 0) & (np.sum((n @ rot.T)[keep] * (l @ rot.T)[keep], -1) > 0)
    np.testing.assert_allclose(got[ok], T[:, i[keep], j[keep], k[keep]].T[ok], rtol=1e-6, atol=1e-9)
    assert ok.sum() > 100


def test_proxy_alpha_tracks_the_roughness():
    for m in (0.0, 1.0):
        for r in (0.2, 0.3, 0.5, 0.8, 1.0):
            T = np.zeros((3, 90, 90, 180))
            T[:, :, :1, :1] = mr.export([m, 0.7, 0.5, 0.3, r, 0.6], j=[0], k=[0])
            a = mr.proxy_alpha(T)
            print(f"m {m} r {r}: alpha {a:.4f}, alpha / r^2 {a / (r * r):.3f}")
            assert 0.8 <= a / (r * r) <= 1.25, (m, r, a)
            assert merl.proxy_alpha(T) == a  # the product's rule is the restatement's
    flat = np.full((3, 90, 90, 180), 0.3)
    assert mr.proxy_alpha(flat) == 1.0 and merl.proxy_alpha(flat) == 1.0
    assert merl.MeasuredBSDF(flat.astype(np.float32)).alpha == 1.0


@pytest.mark.parametrize("row", [ROW_A, ROW_B])
def test_table_render_of_an_exported_row_is_the_principled_render(row):
    """conventions, on the restatement alone: the azimuth, the cosine and the balance weights"""
    T = exported(tuple(row))
    env = smooth_env()
    img = mr.render_table(T, mr.proxy_alpha(T), env, 8, Q=32, S=2)
    err = rel_l2(img, rr.render_quadrature(row, env, 8, Q=32, S=2))
    print(f"row {row}: table render against the principled quadrature: rel-L2 {err:.3g}")
    assert err <= 5e-3, err


def test_lambertian_table_reflects_its_albedo():
    rho = 0.6
    img = mr.render_table(np.full((3, 90, 90, 180), rho / np.pi), 1.0, None, 8, Q=32, S=2)
    print(f"Lambertian table under a white map: max |pixel - rho| {np.abs(img - rho).max():.3g}")
    assert np.abs(img - rho).max() <= 2e-3


def test_symbols_are_declared_listed_and_typed():
    from drmnet_amd import _lib

    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    L = _lib.lib()
    for name in ("drm_brdf_to_merl", "drm_merl_eval", "drm_render_refmap", "drm_render_normals"):
        assert name + "(" in header and name in _lib.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None, name
    assert {"tables", "NT", "table_of", "table_alpha", "table_linear"} <= {n for n, _ in _lib.Shading._fields_}
    assert L.drm_abi_version() == 4 and "packed table" in header
    from drmnet_amd import build

    assert "brdf_table.hip" in build.SOURCES and "render_shared.h" in build.HEADERS


def test_command_lines_reject_what_is_not_built(tmp_path, capsys):
    from drmnet_amd import estimate, relight

    np.save(tmp_path / "n.npy", np.zeros((4, 5, 3), dtype=np.float32))
    base = ["--input_normal", str(tmp_path / "n.npy"), "--output_dir", str(tmp_path / "out")]
    z = ["--z", "0", "0.7", "0.5", "0.3", "0.5", "0.6"]
    with pytest.raises(SystemExit):
        relight.main(base + z + ["--merl", str(tmp_path / "a.binary")])  # exactly one of --z / --merl
    with pytest.raises(SystemExit):
        relight.main(base)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        relight.main(base + ["--merl", str(tmp_path / "a.binary"), "--light_samples", "64"])
    assert "light samples under a table are not built" in capsys.readouterr().err
    assert relight.parser().parse_args(base + ["--merl", "a.binary"]).z is None
    assert estimate.parser().parse_args(["--save_merl"]).save_merl is True and estimate.parser().parse_args([]).save_merl is False
    for argv in ([], z, ["--input", "a.binary"], z + ["--input", "a.binary", "--output", "b.binary"]):
        with pytest.raises(SystemExit):
            merl.main(argv)
    assert not (tmp_path / "out").exists()

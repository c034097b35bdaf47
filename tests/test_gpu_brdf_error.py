"""BRDF-space errors and the principled fit on the GPU (csrc/brdf_error.hip through drmnet_amd.reflectance and the command lines) against the
float64 restatement tests/brdf_error_ref.py.

Bars.  The counts are integers and are held exactly.  The other sums are held to rtol 1e-5, the bar drm_brdf_to_merl itself is held to against
the same restatement: the sums are built from its entries, and the float32 rounding of the entries is the same on both sides.  A row against
its own exported table scores exactly 0, because the export and the error kernel form a row's value with one device function (merl_grid.h);
the bound that two float32 roundings of one float64 value would allow (|d log10| <= 2 * 2^-24 / ln 10 = 5.2e-8 per value, 1e-7 on an RMS) is
asserted as well.  The fit is held to a bar derived from its target alone: the largest objective of the twelve rows z* +- e_i / 256, by the
restatement on the 1/3 sub-grid (54 000 nodes; the twelve are means over the grid and range over 3.8e-5 ... 1.06e-3 for MIXED, a sub-grid
moves them in the third digit)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import brdf_error_ref as er
from drmnet_amd import merl
from drmnet_amd import reflectance as rf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DIELECTRIC, METALLIC, MIXED = (0.0, 0.7, 0.5, 0.3, 0.5, 0.6), (1.0, 0.9, 0.6, 0.3, 0.3, 1.0), (0.3, 0.7, 0.5, 0.3, 0.8, 0.6)
GLOSSY, MIRROR = (0.2, 0.2, 0.6, 0.8, 0.25, 0.5), (1.0, 1.0, 1.0, 1.0, 0.03, 1.0)
ROWS = (DIELECTRIC, METALLIC, MIXED, GLOSSY, MIRROR)
I, J, K = np.meshgrid(np.arange(90.0), np.arange(90.0), np.arange(180.0), indexing="ij")
SUB = (np.arange(0, 90, 3), np.arange(0, 90, 3), np.arange(0, 180, 3))
QUICK_FIT = dict(starts=64, step_min=2.0 ** -6)  # what the command-line tests pass to the fit: a survey of 64 rows and four halvings of the step


@functools.lru_cache(maxsize=None)
def smooth_table():
    """the smooth synthetic isotropic table of test_gpu_merl.py, restated: a broad lobe in theta_h, a falling term in theta_d, an azimuthal
    term that vanishes at theta_h = 0 and theta_d = 0"""
    base = 0.25 + 0.6 * np.exp(-(I / 35.0) ** 2) + 0.15 * (J / 90.0) ** 2 + 0.1 * (I / 90.0) * (J / 90.0) * np.cos(2 * np.pi * K / 180.0)
    t = np.stack([base, 0.8 * base + 0.05, 0.6 * base + 0.02 * (J / 90.0)]).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def ref_values(row):
    """the restatement's table of a row as the export stores it (float32 values as float64), read-only"""
    t = er.values(row)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def exported(row):
    """the table drm_brdf_to_merl exports for a row, as a MeasuredBSDF"""
    from drmnet_amd.render import PrincipledBSDF

    return merl.MeasuredBSDF.from_principled(PrincipledBSDF(row), alpha=1.0)


def ref_sums(target):
    return np.stack([er.error_sums(ref_values(r), target) for r in ROWS])


def check_against(got, ref, what):
    """counts exactly, the other sums to rtol 1e-5"""
    for c in range(len(got)):
        print(f"{what} row {c}: n {int(got[c, 0])}, n_log {int(got[c, 1])} (restatement {int(ref[c, 1])}), "
              f"largest relative difference of the sums {np.max(np.abs(got[c, 2:] - ref[c, 2:]) / np.maximum(np.abs(ref[c, 2:]), 1e-300)):.3g}")
    assert np.array_equal(got[:, 0], ref[:, 0]), what
    # the a > 0 decisions: the same on both sides on every row, the near-mirror row included (its D (n.h) stays far above the 1e-20 cut-off
    # over the whole grid), so equality is asserted
    assert np.array_equal(got[:, 1], ref[:, 1]), what
    np.testing.assert_allclose(got[:, 2:], ref[:, 2:], rtol=1e-5, atol=0, err_msg=what)


# ---------------------------------------------------------------------------------------------- 1. the sums
@pytest.mark.parametrize("target", ["table", "row"])
def test_sums_match_the_restatement(target):
    if target == "table":
        got, ref = rf.brdf_error_sums(ROWS, smooth_table()), ref_sums(smooth_table().astype(np.float64))
    else:
        got, ref = rf.brdf_error_sums(ROWS, MIXED), ref_sums(ref_values(MIXED))
        assert not got[2, 2:6].any() and got[2, 6] == got[2, 7] == got[2, 8]  # MIXED against itself
    assert got.shape == (5, 9) and got.dtype == np.float64
    check_against(got, ref, target)
    assert got[0, 0] == 3 * er.grid()[1].sum() and (got[:, 0] == got[0, 0]).all() and (got[:, 8] == got[0, 8]).all()
    # the other target forms agree: a MeasuredBSDF, and a PrincipledBSDF
    from drmnet_amd.render import PrincipledBSDF

    if target == "table":
        assert np.array_equal(got, rf.brdf_error_sums(np.asarray(ROWS), merl.MeasuredBSDF(smooth_table(), alpha=1.0)))
    else:
        assert np.array_equal(got[3:4], rf.brdf_error_sums(PrincipledBSDF(GLOSSY), PrincipledBSDF(MIXED)))


# ---------------------------------------------------------------------------------------------- 2. sharp zero
@pytest.mark.parametrize("row", ROWS, ids=["dielectric", "metallic", "mixed", "glossy", "mirror"])
def test_a_row_against_its_own_export_scores_zero(row):
    e = rf.brdf_errors(row, exported(row))
    print(row, e)
    assert e["rmse_log10"] <= 1e-7 and e["rmse_log1p"] <= 1e-7
    # one device function forms the value on both sides: the result is exactly 0, not a rounding of it
    assert e["rmse_log10"] == 0.0 and e["rmse_log1p"] == 0.0 and e["mean_log10"] == 0.0 and e["rel_l2"] == 0.0 and e["scale"] == 1.0
    assert e["n"] == 3 * er.grid()[1].sum()
    if row in (DIELECTRIC, METALLIC, MIXED):
        assert e["n_log"] == e["n"]
    assert e["n_log"] > 0.9 * e["n"]
    # and it is a sharp zero: the neighbour one float32 step down the red base colour is not
    near = list(row)
    near[1] = float(np.nextafter(np.float32(row[1]), np.float32(0.0)))
    assert rf.brdf_errors(near, exported(row))["rmse_log1p"] > 0.0


# ---------------------------------------------------------------------------------------------- 3. batches
def test_a_row_does_not_depend_on_its_batch_and_calls_repeat():
    table = merl.MeasuredBSDF(smooth_table(), alpha=1.0)
    five = rf.brdf_error_sums(ROWS, table)
    assert np.array_equal(five, rf.brdf_error_sums(ROWS, table))
    assert np.array_equal(five[3], rf.brdf_error_sums([ROWS[3]], table)[0])
    assert np.array_equal(five[3], rf.brdf_error_sums([ROWS[3], ROWS[0], ROWS[1]], table)[0])
    # in another block's candidate lanes (a block scores 16 rows) and in a last block that is not full: row 3 as row 22 of 37
    many = rf.brdf_error_sums([ROWS[c % 5] for c in range(17)] + [ROWS[(c + 3) % 5] for c in range(20)], table)
    assert np.array_equal(many[22], five[3]) and np.array_equal(many[16], five[1]) and np.array_equal(many[36], five[2])
    assert np.isfinite(five).all() and len({tuple(r) for r in five[:, 2:6]}) == 5  # (the rows differ)


# ---------------------------------------------------------------------------------------------- 4. invalid entries
def test_target_entries_without_a_measurement_do_not_count():
    t = smooth_table().copy()
    t[:, 10:20] = -1.0
    got = rf.brdf_error_sums(ROWS, t)
    lit = er.grid()[1]
    plain = rf.brdf_error_sums(ROWS[:1], smooth_table())
    assert lit[10:20].sum() > 100000 and got[0, 0] == plain[0, 0] - 3 * lit[10:20].sum()
    check_against(got, ref_sums(t.astype(np.float64)), "holed table")


# ---------------------------------------------------------------------------------------------- 5. rejections
def test_bad_arguments_are_rejected_and_the_process_goes_on():
    from drmnet_amd import _lib

    lib = _lib.lib()
    s = _lib.stream_ptr(DEV)
    z = torch.tensor(ROWS, dtype=torch.float32, device=DEV)
    zt = torch.tensor([MIXED], dtype=torch.float32, device=DEV)
    big = torch.zeros((4097, 6), device=DEV)
    table = torch.from_numpy(merl.pack_table(smooth_table())).to(DEV)
    shifted = torch.zeros(table.numel() + 4, device=DEV)
    nbytes = _lib.brdf_error_workspace_bytes(4097)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    sums = torch.full((4097, 9), -7.0, dtype=torch.float64, device=DEV)
    w5 = _lib.brdf_error_workspace_bytes(5)
    assert w5 == 5 * 128 * 9 * 8
    cases = [((z.data_ptr(), 5, table.data_ptr(), zt.data_ptr(), ws.data_ptr(), nbytes, sums.data_ptr(), s), "exactly one"),
             ((z.data_ptr(), 5, None, None, ws.data_ptr(), nbytes, sums.data_ptr(), s), "exactly one"),
             ((z.data_ptr(), 0, table.data_ptr(), None, ws.data_ptr(), nbytes, sums.data_ptr(), s), "C in [1, 4096]"),
             ((big.data_ptr(), 4097, table.data_ptr(), None, ws.data_ptr(), nbytes, sums.data_ptr(), s), "C in [1, 4096]"),
             ((z.data_ptr(), 5, shifted.data_ptr() + 4, None, ws.data_ptr(), nbytes, sums.data_ptr(), s), "16-byte aligned"),
             ((z.data_ptr(), 5, table.data_ptr(), None, ws.data_ptr(), w5 - 8, sums.data_ptr(), s), "workspace"),
             ((None, 5, table.data_ptr(), None, ws.data_ptr(), nbytes, sums.data_ptr(), s), "null"),
             ((z.data_ptr(), 5, table.data_ptr(), None, ws.data_ptr(), nbytes, None, s), "null")]
    for args, word in cases:
        status = lib.drm_brdf_error_sums(*args)
        torch.cuda.synchronize()
        message = (lib.drm_last_error() or b"").decode()
        assert status != 0 and "brdf_error_sums" in message and word in message, (word, status, message)
        assert bool((sums == -7.0).all()), word
    assert lib.drm_brdf_error_sums(z.data_ptr(), 5, table.data_ptr(), None, ws.data_ptr(), w5, sums.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(sums[:5].cpu().numpy(), rf.brdf_error_sums(ROWS, smooth_table())) and bool((sums[5:] == -7.0).all())
    with pytest.raises(ValueError):
        rf.brdf_error_sums(ROWS, np.zeros((3, 90, 90, 90)))
    with pytest.raises(ValueError):
        rf.brdf_errors(ROWS, smooth_table())


# ---------------------------------------------------------------------------------------------- 6. the fit recovers a principled table
def twelve(row, name="log1p"):
    """the objectives of row +- e_i / 256 against the row's own table, by the restatement on the 1/3 sub-grid"""
    target = er.values(row, *SUB)
    out = []
    for i in range(6):
        for sign in (1.0, -1.0):
            z = np.array(row, dtype=np.float64)
            z[i] = np.clip(z[i] + sign / 256.0, 0.0, 1.0)
            out.append(er.objective(z, target, name, *SUB))
    return out


@pytest.mark.parametrize("row", [MIXED, GLOSSY], ids=["mixed", "glossy"])
def test_fit_recovers_a_principled_table(row):
    fit = rf.fit_principled(exported(row))
    again = rf.fit_principled(exported(row))
    bar = twelve(row)
    print(f"fit of {row}: z {[round(v, 5) for v in fit['z']]}, objective {fit['objective']:.3g}, {fit['rounds']} rounds, {fit['evaluations']} evaluations; "
          f"the twelve: {[float(f'{v:.3g}') for v in bar]}")
    assert fit["objective"] <= max(bar)
    assert fit["z"] == again["z"] and fit["objective"] == again["objective"] and fit["evaluations"] == again["evaluations"]
    assert len(fit["z"]) == 6 and fit["rounds"] > 0 and 4096 + 13 * fit["rounds"] <= fit["evaluations"] <= 4096 + 104 * fit["rounds"]
    assert fit["objective"] == fit["errors"]["rmse_log1p"] == rf.brdf_errors(fit["z"], exported(row))["rmse_log1p"]


# ---------------------------------------------------------------------------------------------- 7. a table no row equals
def test_fit_of_a_non_principled_table_is_no_worse_than_its_seed():
    factor = 1.0 + 0.2 * np.cos(2 * np.pi * K / 180.0) * (I / 90.0) * (J / 90.0)  # (vanishes where phi_d is undefined)
    base = exported(MIXED).table
    table = np.where(base < 0, base, base * factor.astype(np.float32)[None]).astype(np.float32)
    seed = er.objective(ref_values(MIXED), table.astype(np.float64))
    fit = rf.fit_principled(table)
    print(f"fit of the modulated table: z {[round(v, 5) for v in fit['z']]}, objective {fit['objective']:.4g}; the seed row's {seed:.4g}; "
          f"{fit['rounds']} rounds, {fit['evaluations']} evaluations")
    assert fit["objective"] <= seed and seed > 1e-3


# ---------------------------------------------------------------------------------------------- 8. estimate --gt_z / --gt_merl
def test_estimate_reports_the_brdf_errors(tmp_path):
    from conftest import GOLD, gold
    from drmnet_amd import estimate, file_io
    from drmnet_amd.render import get_bsdf
    from test_gpu_estimate import tiny_models

    g = gold("estimate_chain")
    models = tiny_models(g, DEV)
    for m in models:
        m.set_precision("fp32")
    d = os.path.join(GOLD, "sample")
    hooks = {k: torch.from_numpy(g[s]).to(DEV) for k, s in (("cond_noise", "cond"), ("x_T", "x_T"), ("noise", "noise"), ("noise0", "noise0"),
                                                            ("step_noise", "step_noise"))}
    hooks["fit"] = QUICK_FIT
    base = ["--input_img", os.path.join(d, "image.exr"), "--input_normal", os.path.join(d, "normal.npy"), "--input_mask", os.path.join(d, "mask.png")]
    merl.save_merl(exported(GLOSSY).table, tmp_path / "truth.binary")
    env = np.random.default_rng(3).uniform(0.1, 2.0, size=(16, 32, 3)).astype(np.float32)
    file_io.save_exr(tmp_path / "env.exr", torch.from_numpy(env))

    def run(name, extra):
        estimate.main(base + ["--output_dir", str(tmp_path / name)] + extra, models=models, hooks=hooks)
        row = get_bsdf(torch.tensor(np.load(tmp_path / name / "sample_brdf.npy")), models[0].brdf_param_names)
        path = tmp_path / name / "sample_gt_errors.json"
        return row, (json.loads(path.read_text()) if path.exists() else None)

    # without the new options the file holds what it held
    _, old = run("env", ["--gt_envmap", str(tmp_path / "env.exr"), "--gt_view_from", "0.6", "0.3", "1"])
    assert sorted(old) == ["envmap", "mirror_map"]
    row, both = run("env_z", ["--gt_envmap", str(tmp_path / "env.exr"), "--gt_view_from", "0.6", "0.3", "1", "--gt_z", *[str(v) for v in MIXED]])
    assert sorted(both) == ["brdf", "envmap", "mirror_map"] and both["envmap"] == old["envmap"] and both["mirror_map"] == old["mirror_map"]
    assert both["brdf"] == rf.brdf_errors(row, MIXED) and both["brdf"]["n"] == 3 * er.grid()[1].sum() and both["brdf"]["rmse_log1p"] > 0
    row, table = run("merl", ["--gt_merl", str(tmp_path / "truth.binary")])
    truth = merl.MeasuredBSDF.from_file(tmp_path / "truth.binary", alpha=1.0)
    assert sorted(table) == ["brdf", "brdf_fit"] and table["brdf"] == rf.brdf_errors(row, truth)
    fit = table["brdf_fit"]
    assert len(fit["z"]) == 6 and fit == rf.fit_principled(truth, **QUICK_FIT) and fit["errors"]["n"] == table["brdf"]["n"]


# ---------------------------------------------------------------------------------------------- 9. merl --fit / --compare
def test_merl_command_lines_print_the_library_figures(tmp_path, capsys):
    from drmnet_amd.render import CANONICAL

    merl.save_merl(exported(GLOSSY).table, tmp_path / "g.binary")
    truth = merl.MeasuredBSDF.from_file(tmp_path / "g.binary", alpha=1.0)
    capsys.readouterr()
    merl.main(["--input", str(tmp_path / "g.binary"), "--compare", "--z", *[str(v) for v in MIXED]])
    out = json.loads(capsys.readouterr().out)
    assert out == rf.brdf_errors(MIXED, truth) and out["rmse_log1p"] > 0.01
    merl.main(["--compare", "--z", *[str(v) for v in MIXED], "--against", str(tmp_path / "g.binary")])
    assert json.loads(capsys.readouterr().out) == out
    for objective in ("log1p", "l2"):
        merl.main(["--input", str(tmp_path / "g.binary"), "--fit", "--objective", objective, "--output", str(tmp_path / "fit.binary")], fit_options=QUICK_FIT)
        line = capsys.readouterr().out.splitlines()[0]
        got = json.loads(line)
        want = rf.fit_principled(truth, objective=objective, **QUICK_FIT)
        assert list(got["z"]) == list(CANONICAL) and list(got["z"].values()) == want["z"]
        assert got["errors"] == want["errors"] and got["objective"] == want["objective"] and got["rounds"] == want["rounds"]
        assert got["evaluations"] == want["evaluations"] > 64
        np.testing.assert_allclose(merl.load_merl(tmp_path / "fit.binary"), exported(tuple(want["z"])).table, rtol=2e-7, atol=0)

"""CPU-only checks of the BRDF-space errors and the fit (drmnet_amd/reflectance.py): the Halton points, the pattern search on functions with a
known minimum, the figures from hand-made sums, the float64 restatement (tests/brdf_error_ref.py) against itself, and the argument rules of
both command lines.  Nothing here touches a GPU."""
import numpy as np
import pytest

import brdf_error_ref as er
from drmnet_amd import reflectance as rf

MIXED = (0.3, 0.7, 0.5, 0.3, 0.8, 0.6)
SUB = (np.arange(0, 90, 3), np.arange(0, 90, 3), np.arange(0, 180, 3))  # a 1/3 sub-grid: 54 000 nodes


def test_halton_first_values_shape_and_range():
    h = rf.halton(9)
    assert h.shape == (9, 6) and h.dtype == np.float64
    np.testing.assert_allclose(h[:7, 0], [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8], rtol=0, atol=1e-15)
    np.testing.assert_allclose(h[:5, 1], [1 / 3, 2 / 3, 1 / 9, 4 / 9, 7 / 9], rtol=0, atol=1e-15)
    np.testing.assert_allclose(h[:6, 2], [1 / 5, 2 / 5, 3 / 5, 4 / 5, 1 / 25, 6 / 25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(h[:2, 5], [1 / 13, 2 / 13], rtol=0, atol=1e-15)
    big = rf.halton(4096)
    assert big.shape == (4096, 6) and (big > 0).all() and (big < 1).all()
    assert np.array_equal(big[:9], h) and rf.halton(5, dims=2).shape == (5, 2) and rf.halton(0).shape == (0, 6)
    assert len(np.unique(big[:, 0])) == 4096  # (no point repeats)
    with pytest.raises(ValueError):
        rf.halton(4, dims=7)


QUAD_MIN = np.array([0.375, 0.625, 0.25, 0.8125, 0.5, 0.09375])  # interior, dyadic
QUAD_W = np.array([1.0, 3.0, 0.5, 2.0, 7.0, 1.5])


def quadratic(x):
    return np.sum(QUAD_W * (x - QUAD_MIN) ** 2, axis=1)


VALLEY_REST = np.array([0.25, 0.75, 0.375, 0.5])


def valley(x):
    """a curved valley x1 = x0^2 / 2 that falls toward x0 = 1.25: over the box its minimum lies on the face x0 = 1, at x1 = 1 / 2"""
    return (x[:, 0] - 1.25) ** 2 + 4.0 * (x[:, 1] - 0.5 * x[:, 0] ** 2) ** 2 + np.sum((x[:, 2:] - VALLEY_REST) ** 2, axis=1)


VALLEY_MIN = np.concatenate([[1.0, 0.5], VALLEY_REST])


@pytest.mark.parametrize("fn,minimum", [(quadratic, QUAD_MIN), (valley, VALLEY_MIN)], ids=["quadratic", "valley_on_a_face"])
def test_pattern_search_finds_the_minimum_and_repeats(fn, minimum):
    starts = rf.halton(256)
    a = rf.pattern_search(fn, starts)
    b = rf.pattern_search(fn, starts)
    print(f"{fn.__name__}: |x - x*|_inf {np.abs(a.x - minimum).max():.3g}, objective {a.objective:.3g} (at x* {fn(minimum[None])[0]:.3g}), "
          f"{a.rounds} rounds, {a.evaluations} evaluations")
    assert np.abs(a.x - minimum).max() <= 2.0 ** -12
    if fn is valley:
        assert a.x[0] == 1.0  # on the face, not near it
    assert np.array_equal(a.x, b.x) and a.objective == b.objective and a.rounds == b.rounds and a.evaluations == b.evaluations
    assert a.objective == fn(a.x[None])[0] and 0 < a.rounds < 400


def test_pattern_search_ties_rounds_and_calls():
    starts = rf.halton(2500)
    calls = []

    def constant(x):
        calls.append(len(x))
        assert x.shape[1] == 6 and (x >= 0).all() and (x <= 1).all()
        return np.full(len(x), 3.0)

    r = rf.pattern_search(constant, starts)
    # no candidate is ever strictly better: the first start stands, and every step halves from 2^-3 until it is below 2^-12: ten rounds
    assert np.array_equal(r.x, starts[0]) and r.objective == 3.0 and r.rounds == 10
    # the survey in batches of at most 1024, then ONE call per round with the 13 candidates of each of the 8 points
    assert calls == [1024, 1024, 452] + [8 * 13] * 10 and r.evaluations == sum(calls)
    calls.clear()
    r = rf.pattern_search(quadratic_counted(calls), starts[:100], keep=3, max_rounds=5)
    assert r.rounds == 5 and calls == [100] + [3 * 13] * 5
    # ties in the survey go to the lower index
    r = rf.pattern_search(lambda x: np.zeros(len(x)), np.array([[0.5] * 6, [0.25] * 6]), keep=1)
    assert np.array_equal(r.x, [0.5] * 6)


def quadratic_counted(calls):
    def fn(x):
        calls.append(len(x))
        return quadratic(x)

    return fn


def test_errors_from_hand_made_sums():
    #            n   n_log  d     dd    log1p  l2    aa    ab    bb
    s = np.array([12.0, 8.0, -4.0, 10.0, 3.0, 2.0, 4.0, 6.0, 16.0])
    e = rf.errors_from_sums(s)
    assert e["n"] == 12 and e["n_log"] == 8 and isinstance(e["n"], int)
    assert e["rmse_log10"] == np.sqrt(10.0 / 8.0) and e["mean_log10"] == -0.5
    assert e["rmse_log10_scaled"] == np.sqrt(10.0 / 8.0 - 0.25)
    assert e["rmse_log1p"] == 0.5 and e["rel_l2"] == np.sqrt(2.0 / 16.0) and e["scale"] == 1.5
    assert e["rel_l2_scaled"] == np.sqrt((16.0 - 36.0 / 4.0) / 16.0)
    assert e == {k: v for k, v in er.errors(s).items()}
    # zero denominators give 0, and a rounding below zero under a root is 0
    z = rf.errors_from_sums(np.zeros(9))
    assert z == {"n": 0, "n_log": 0, "rmse_log10": 0.0, "mean_log10": 0.0, "rmse_log10_scaled": 0.0, "rmse_log1p": 0.0, "rel_l2": 0.0, "scale": 0.0,
                 "rel_l2_scaled": 0.0}
    no_log = rf.errors_from_sums(np.array([6.0, 0.0, 0.0, 0.0, 6.0, 1.0, 0.0, 0.0, 4.0]))  # a candidate that is 0 everywhere
    assert no_log["rmse_log10"] == 0.0 and no_log["scale"] == 0.0 and no_log["rel_l2_scaled"] == 1.0 and no_log["rmse_log1p"] == 1.0
    tight = rf.errors_from_sums(np.array([3.0, 3.0, 3.0, 3.0 - 1e-16, 0.0, 0.0, 1.0, 1.0, 1.0 - 1e-16]))
    assert tight["rmse_log10_scaled"] == 0.0 and tight["rel_l2_scaled"] == 0.0
    with pytest.raises(ValueError):
        rf.errors_from_sums(np.zeros(8))
    with pytest.raises(ValueError):
        rf.fit_principled(np.zeros((3, 90, 90, 180), dtype=np.float32), objective="log10")


def test_the_restatement_against_itself():
    table = er.values(MIXED, *SUB)
    ci, lit = er.grid(*SUB)
    s = er.error_sums(MIXED, table, *SUB)
    assert s[0] == 3 * lit.sum() and s[1] == s[0] and 0.6 < lit.mean() < 0.9
    assert not s[2:6].any() and s[6] == s[7] == s[8] > 0
    e = er.errors(s)
    assert all(e[k] == 0.0 for k in ("rmse_log10", "mean_log10", "rmse_log10_scaled", "rmse_log1p", "rel_l2", "rel_l2_scaled")) and e["scale"] == 1.0
    # a target twice the row (below the horizon it stays -1)
    e = er.errors(er.error_sums(MIXED, np.where(table < 0, table, 2.0 * table), *SUB))
    assert abs(e["mean_log10"] + np.log10(2.0)) <= 1e-12 and abs(e["rmse_log10"] - np.log10(2.0)) <= 1e-12
    assert e["rmse_log10_scaled"] <= 1e-12 and abs(e["scale"] - 2.0) <= 1e-12 and e["rel_l2_scaled"] <= 1e-12 and abs(e["rel_l2"] - 0.5) <= 1e-12
    assert e["n"] == e["n_log"] == 3 * lit.sum()
    # entries without a measurement leave the count
    holed = table.copy()
    holed[:, 4:7] = -1.0
    assert er.error_sums(MIXED, holed, *SUB)[0] == 3 * lit.sum() - 3 * lit[4:7].sum() and lit[4:7].sum() > 0
    # a row target is its table
    other = (0.2, 0.2, 0.6, 0.8, 0.25, 0.5)
    assert np.array_equal(er.error_sums(other, MIXED, *SUB), er.error_sums(other, table, *SUB))
    assert er.objective(other, table, "log1p", *SUB) > 0.01 and er.objective(other, table, "l2", *SUB) > 0.01


def test_argument_rules_of_both_command_lines(capsys):
    from drmnet_amd import estimate, merl

    base = ["--input_img", "i.exr", "--input_normal", "n.npy"]
    z = ["0.3", "0.7", "0.5", "0.3", "0.8", "0.6"]
    with pytest.raises(SystemExit) as e:
        estimate.parse_args(base + ["--gt_z", *z, "--gt_merl", "m.binary"])
    assert e.value.code == 2 and "--gt_z and --gt_merl exclude each other" in capsys.readouterr().err
    a = estimate.parse_args(base + ["--gt_z", *z])
    assert a.gt_z == [float(v) for v in z] and a.gt_merl is None
    a = estimate.parse_args(base + ["--gt_merl", "m.binary"])
    assert a.gt_z is None and str(a.gt_merl) == "m.binary"
    a = estimate.parse_args(base)
    assert a.gt_z is None and a.gt_merl is None
    for argv, word in ((["--fit"], "--fit needs --input"), (["--fit", "--z", *z, "--output", "o.binary"], "--fit needs --input"),
                       (["--compare", "--input", "a.binary", "--against", "b.binary"], "table-versus-table"),
                       (["--compare", "--z", *z], "exactly one table"), (["--compare", "--z", *z, "--input", "a.binary", "--against", "b.binary"], "exactly one table"),
                       (["--fit", "--compare", "--input", "a.binary"], "exclude each other"), (["--input", "a.binary", "--against", "b.binary", "--figure", "f.png"], "--compare")):
        with pytest.raises(SystemExit) as e:
            merl.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    a = merl.parse_args(["--input", "a.binary", "--fit", "--objective", "l2"])
    assert a.fit and a.objective == "l2" and merl.parse_args(["--input", "a.binary", "--fit"]).objective == "log1p"
    a = merl.parse_args(["--compare", "--z", *z, "--against", "b.binary"])
    assert a.compare and str(a.against) == "b.binary" and a.input is None

"""Premises of tests/test_gpu_transform_sharp.py, shown without a GPU (tests/transform_ref.py; DESIGN.md "Transform-kernel checks"):
the restatements agree with the installed torch and with oracle/transforms.py, the identity resize is the identity, correct fp32 arithmetic
(the oracle, or the kernel's order with torch's CPU libm) stays inside every bound, every mutant fails its named case, and the poison
expectations are what the oracle returns."""
import numpy as np
import pytest
import torch

import transform_ref as R
from oracle import transforms as ot

F = np.float32
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def outside(out, ref, bound, by=1.0):
    """a check of `out` against (ref, bound) fails: another class somewhere, or more than `by` bounds away"""
    try:
        return R.ratio(out, ref, bound) > by
    except AssertionError:
        return True


def test_op_code_table_is_the_packages():
    from drmnet_amd import ops

    assert R.MAP_CODES == ops.MAP_CODES and R.MAX_CHAIN == ops.MAX_CHAIN
    assert sorted(R.ALGEBRAIC + R.LIBM) == sorted(R.MAP_CODES)


def test_libm_figures():
    """torch's CPU fp32 functions against float64 over the sweeps: the figures DESIGN.md quotes; a figure of 4 or more would mean a broken sweep"""
    ulps = R.libm_ulps()
    print({k: round(v, 3) for k, v in ulps.items()})
    assert set(ulps) == {"log10f", "powf", "logf", "expf", "sinf", "cosf", "atan2f", "acosf"}
    for k, v in ulps.items():
        assert 0.0 < v < 4.0 and R.K(k) == v + 2.0, (k, v)


# ------------------------------------------------------------------------------------------------ maps

def test_algebraic_restatement_is_torchs():
    """map32 against the oracle's torch expressions, bit for bit, on the whole sweep"""
    x = R.algebraic_sweep()
    t = T(x)
    lo, hi, sc = F(-2.5), F(1.75), F(0.37)
    want = {"lowerbound": t.clip(0.5), "unit_to_signed": t * 2 - 1, "signed_to_unit": (t + 1) / 2, "denorm_log": t * (T(hi) - T(lo)) + T(lo),
            "img_mul": t * T(sc), "img_div": t / T(sc), "clip0": t.clip(0)}
    for name in R.ALGEBRAIC:
        got = R.map32(name, 0.5, x, lo, hi, sc)
        ok = R.bits_equal(got, want[name].numpy())
        if name in ("lowerbound", "clip0"):  # torch.clip may return either zero for -0 against 0; the kernel keeps -0 (v < 0 is false)
            ok |= (got == 0) & (want[name].numpy() == 0)
        assert ok.all(), (name, x[~ok], got[~ok])
    assert np.isnan(R.map32("lowerbound", 0.5, F(np.nan))) and np.isnan(R.map32("clip0", 0.0, F(np.nan)))


@pytest.mark.parametrize("name", list(R.CHAINS) + ["chain8", "chain9"])
def test_host_fp32_chain_is_inside_the_bound(name):
    steps = R.CHAINS.get(name) or (R.CHAIN8 if name == "chain8" else R.CHAIN9)
    x, lo, hi, sc = R.chain_inputs(name, 3, 1025)
    ref, bound = R.chain64(steps, x, lo, hi, sc)
    r = R.ratio(R.chain32_host(steps, x, lo, hi, sc), ref, bound)
    print(name, "host fp32 / bound", round(r, 3))
    assert r <= 1.0
    if name in R.CHAINS:  # and the oracle's own composition agrees with the float64 chain
        p = (T(lo).view(-1, 1), T(hi).view(-1, 1))
        if name == "log_fwd":
            o = ot.transform(T(x), "log")[0]
        elif name == "obs_fwd":
            o = ot.transform(T(x), "0p1tom1p1_normalizedLogarithmic_lowerbound1e-6", params=p)[0]
        elif name in ("log_inv", "log_inv_nocap"):
            o = ot.rescale(T(x), "log", R.CAP if name == "log_inv" else 0.0)
        elif name == "obs_inv":
            o = ot.rescale(T(x), "0p1tom1p1_normalizedLogarithmic", R.CAP, p)
        else:
            return
        assert R.ratio(o.numpy(), ref, bound) <= 1.0


def test_norm_log_with_equal_bounds():
    x = np.array([[1.0, 10.0, 0.1, 0.0]], dtype=F)
    lo = hi = np.array([0.0], dtype=F)
    ref, bound = R.chain64([("norm_log", 0.0)], x, lo, hi)
    assert np.isnan(ref[0, 0]) and ref[0, 1] == np.inf and ref[0, 2] == -np.inf and ref[0, 3] == -np.inf
    assert R.ratio(R.chain32_host([("norm_log", 0.0)], x, lo, hi), ref, bound) == 0.0
    o = ot.transform(T(x), "normalizedLogarithmic", params=(T(lo), T(hi)))[0].numpy()
    assert R.ratio(o, ref, bound) == 0.0


def test_chain_mutants_fail_their_cases():
    # reversed: the obs forward chain
    x, lo, hi, sc = R.chain_inputs("obs_fwd", 3, 63)
    good = R.chain32_host(R.CHAINS["obs_fwd"], x, lo, hi, sc)
    ref, bound = R.chain64(R.CHAINS["obs_fwd"], x, lo, hi, sc, reverse=True)
    assert outside(good, ref, bound, 1e3)
    # the clamp after the exponential: exp_m1 clamps the exponent at 20, the mutant the power at 20
    x, lo, hi, sc = R.chain_inputs("log_inv", 3, 63)
    good = R.chain32_host(R.CHAINS["log_inv"], x, lo, hi, sc)
    ref, bound = R.chain64(R.CHAINS["log_inv"], x, lo, hi, sc, clamp_after=True)
    assert R.ratio(good, ref, bound) > 1e3
    # image 0's lo / hi / scale for every image: the ragged cases (B = 3, distinct vectors)
    for name in ("obs_inv", "est_mul_log"):
        for per in R.RAGGED:
            x, lo, hi, sc = R.chain_inputs(name, 3, per)
            good = R.chain32_host(R.CHAINS[name], x, lo, hi, sc)
            ref, bound = R.chain64(R.CHAINS[name], x, lo, hi, sc, image0=True)
            assert R.ratio(good[:1], ref[:1], bound[:1]) <= 1.0 and outside(good[1:], ref[1:], bound[1:], 1e3)


# ------------------------------------------------------------------------------------------------ ranges, scale, tone map

@pytest.mark.parametrize("name", R.RANGE_CASES)
def test_range_reference_is_the_oracles(name):
    x, m = R.range_case(name)
    lo, hi, blo, bhi = R.range64(x, m)
    _, (olo, ohi) = ot.transform(T(x), "normalizedLogarithmic", mask=T(m))
    assert R.ratio(olo.reshape(-1).numpy(), lo, blo) <= 1.0 and R.ratio(ohi.reshape(-1).numpy(), hi, bhi) <= 1.0
    if name == "empty_mask":
        assert lo[0] == -np.inf and hi[0] == -np.inf
    if name == "batch3":
        assert len(set(lo.tolist())) == 3 and len(set(hi.tolist())) == 3


def test_range_mutants_fail_their_cases():
    for mutant, case, kw in (("mask_not_broadcast", "channel2_only", dict(broadcast=False)), ("min_without_substitute", "masked_out_max", dict(substitute=False)),
                             ("range_image0", "batch3", dict(image0=True))):
        assert R.MUTANT_CASES[mutant] == "range:" + case
        x, m = R.range_case(case)
        lo, hi, blo, bhi = R.range64(x, m)
        mlo, mhi, _, _ = R.range64(x, m, **kw)
        with np.errstate(all="ignore"):
            far = max(np.nanmax(np.abs(np.nan_to_num(mlo - lo, nan=np.inf, posinf=np.inf, neginf=np.inf))),
                      np.nanmax(np.abs(np.nan_to_num(mhi - hi, nan=np.inf, posinf=np.inf, neginf=np.inf))))
        assert far > 0.5, (mutant, far)  # half a decade: the bound is a few ulps


@pytest.mark.parametrize("name", R.LUM_CASES)
def test_luminance_scale_reference(name):
    x = R.lum_case(name)
    s, rel = R.lumscale64(x, 0.12)
    h = R.lumscale32_host(x, 0.12)
    o = ot.luminance_scale(T(x), 0.12).numpy()
    if name == "nothing_lit":
        assert np.isnan(s).all() and np.isnan(h).all() and np.isnan(o).all()
        return
    r = R.ratio(h, s, np.abs(s) * rel)
    print(name, "host fp32 / bound", round(r, 3))
    assert r <= 1.0
    assert np.allclose(o, s, rtol=2e-6)  # (the oracle adds in fp32: not the kernel's arithmetic, so only close)


def test_luminance_mutants_fail_their_cases():
    for mutant, case, kw in (("unlit_counted", "unlit_and_dim", dict(count_unlit=True)), ("clip_missing", "unlit_and_dim", dict(clip=False)),
                             ("scale_image0", "batch3", dict(image0=True))):
        assert R.MUTANT_CASES[mutant] == "lum:" + case
        x = R.lum_case(case)
        s, rel = R.lumscale64(x, 0.12)
        ms, _ = R.lumscale64(x, 0.12, **kw)
        assert np.max(np.abs(ms - s) / (np.abs(s) * rel)) > 1e3, mutant


@pytest.mark.parametrize("name", R.TONE_CASES)
def test_tonemap_reference(name):
    x, m, alpha, gamma = R.tone_case(name)
    ref, bound = R.tonemap64(x, m, alpha, gamma)
    h = R.tonemap32_host(x, m, alpha, gamma)
    with np.errstate(all="ignore"):
        o = ot.hdr2ldr(x, None if m is None else m.astype(bool), alpha, gamma).reshape(-1, 3)
    if name == "nothing_lit":
        assert np.isnan(ref).all() and np.isnan(h).all() and np.isnan(o).all()
        return
    r = R.ratio(h, ref, bound)
    print(name, "host fp32 / bound", round(r, 3))
    assert r <= 1.0
    assert np.abs(o - ref).max() < 2e-6


def test_threshold_pixels_sit_on_the_threshold():
    p = R.threshold_pixels()
    L = R.lum32(p[:, 0], p[:, 1], p[:, 2])
    assert L[0] == R.C5E5 and L[1] == np.nextafter(R.C5E5, F(0)) and L[2] == np.nextafter(R.C5E5, F(1))
    assert (L > R.C5E5).tolist() == [False, False, True]


def test_tonemap_mutants_fail_their_cases():
    for mutant, case, kw in (("threshold_missing", "threshold", dict(threshold=False)), ("mask_ignored", "mask_brightest", dict(use_mask=False)),
                             ("gamma_not_inverted", "alpha_gamma", dict(invert_gamma=False))):
        assert R.MUTANT_CASES[mutant] == "tone:" + case
        x, m, alpha, gamma = R.tone_case(case)
        ref, bound = R.tonemap64(x, m, alpha, gamma)
        mref, _ = R.tonemap64(x, m, alpha, gamma, **kw)
        assert np.max(np.abs(mref - ref) / bound) > 1e2, mutant


# ------------------------------------------------------------------------------------------------ poison

def test_poison_expectations_are_the_oracles():
    for case in ("range_nan_in_mask", "range_inf_outside_mask"):
        x, m = R.poison_case(case)
        lo, hi, _, _ = R.range64(x, m)
        _, (olo, ohi) = ot.transform(T(x), "normalizedLogarithmic", mask=T(m))
        olo, ohi = olo.reshape(-1).numpy(), ohi.reshape(-1).numpy()
        assert np.isnan(lo[1]) and np.isnan(hi[1]) and np.isnan(olo[1]) and np.isnan(ohi[1])
        assert np.isfinite(lo[[0, 2]]).all() and np.isfinite(olo[[0, 2]]).all() and np.isfinite(ohi[[0, 2]]).all()
    (x,) = R.poison_case("lum_nan")
    s, _ = R.lumscale64(x, 0.12)
    o = ot.luminance_scale(T(x), 0.12).numpy()
    assert np.isnan(s).tolist() == [False, True, False] == np.isnan(o).tolist()
    for case in ("tone_nan", "tone_inf_outside_mask"):
        x, m, a, g = R.poison_case(case)
        ref, _ = R.tonemap64(x, m, a, g)
        with np.errstate(all="ignore"):
            o = ot.hdr2ldr(x, m.astype(bool), a, g)
        assert np.isnan(ref).all() and np.isnan(o).all(), case
        assert np.isnan(R.tonemap32_host(x, m, a, g)).all(), case  # the kernel's rule, restated
    # a lit +Inf pixel: the coefficient is 0, that pixel Inf * 0 = NaN, every other one 0 -- with a defined (zero-width) bound
    x, m, a, g = R.tone_case("hw1025")
    x = x.copy()
    x[0, 3, 1] = np.inf
    ref, bound = R.tonemap64(x, m, a, g)
    with np.errstate(all="ignore"):
        o = ot.hdr2ldr(x, None, a, g).reshape(-1, 3)
    h = R.tonemap32_host(x, m, a, g)
    assert np.isfinite(bound[~np.isnan(ref)]).all() and np.isnan(ref).sum() == 1 and np.isnan(ref[3, 1])
    for got in (o, h):
        assert np.isnan(got[3, 1]) and (np.delete(got.reshape(-1), 10) == 0).all()
    (x,) = R.poison_case("lum_nan")
    assert np.isnan(R.lumscale32_host(x, 0.12)).tolist() == [False, True, False]


def test_reverting_a_poison_fix_fails_the_poison_case():
    """the rules before the fixes, stated on purpose (np.fmax, keep_poison=False): fmaxf / fminf drop a NaN, `L > 0` and `L > 5e-5` skip one,
    fmaxf(NaN, 0) is 0 -- each returns a finite answer where the reference has NaN (DESIGN.md lists the pairs of fix and test)"""
    for case in ("range_nan_in_mask", "range_inf_outside_mask"):
        x, m = R.poison_case(case)
        with np.errstate(all="ignore"):
            xm = (x * m)[1]
            old_hi = np.log10(np.fmax.reduce(xm.reshape(-1)))
        assert np.isfinite(old_hi) and np.isnan(R.range64(x, m)[1][1])
    (x,) = R.poison_case("lum_nan")
    assert np.isfinite(R.lumscale32_host(x, 0.12, keep_poison=False)).all() and np.isnan(R.lumscale64(x, 0.12)[0][1])
    for case in ("tone_nan", "tone_inf_outside_mask"):
        x, m, a, g = R.poison_case(case)
        assert np.isfinite(R.tonemap32_host(x, m, a, g, keep_poison=False)).all() and np.isnan(R.tonemap64(x, m, a, g)[0]).all()


# ------------------------------------------------------------------------------------------------ resize

def _interp(x, size, mode):
    t = T(x)[:, None]
    if mode == "nearest":
        return torch.nn.functional.interpolate(t, size=size)[:, 0].numpy()
    return torch.nn.functional.interpolate(t, size=size, mode=mode, align_corners=False, antialias=True)[:, 0].numpy()


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_restatement_agrees_with_torch(shape, mode):
    (ih, iw), size = shape
    for x in (R.one_hots(ih, iw), R.dense_image(3, ih, iw)):
        got = R.resize32(x, size, mode)
        want = _interp(x, size, mode)
        if mode == "nearest":
            assert np.array_equal(got, want)
        else:
            assert R.ratio(got, want, R.resize_bound(x, size, mode) + 1e-45) <= 1.0
        # and with the oracle's weight matrices
        assert np.allclose(got, ot.resize(T(x), size, mode).numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
@pytest.mark.parametrize("shape", [((4, 4), (2, 2)), ((20, 20), (17, 19))], ids=["plane_loop_shape", "two_blocks_shape"])
def test_resize_restatement_agrees_with_torch_on_the_other_shapes(shape, mode):
    (ih, iw), size = shape
    x = R.dense_image(5, ih, iw)
    got, want = R.resize32(x, size, mode), _interp(x, size, mode)
    if mode == "nearest":
        assert np.array_equal(got, want)
    else:
        assert R.ratio(got, want, R.resize_bound(x, size, mode)) <= 1.0


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
def test_identity_resize_is_the_identity(mode):
    x = R.dense_image(2, 8, 8)
    assert R.first_bits_mismatch(R.resize32(x, (8, 8), mode), x) is None


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_constant_image_stays_within_two_ulps(mode):
    """on the four listed shapes, in the kernel's order; (20, 20) -> (17, 19) bicubic leaves by 3 ulps (ATen's own passes by 4), so the GPU
    test does not ask it of that shape"""
    u = float(np.spacing(F(0.7)))
    dev = lambda shape, size: np.abs(R.resize32(np.full((1,) + shape, 0.7, dtype=F), size, mode).astype(np.float64) - float(F(0.7))).max() / u
    assert max(dev(shape, size) for shape, size in R.RESIZE_SHAPES) <= 2.0
    if mode == "bicubic":
        assert dev((20, 20), (17, 19)) == 3.0


def test_max_downscale_lengths():
    assert R.max_downscale("bilinear") == (94, 95) and R.max_downscale("bicubic") == (47, 48)
    for mode, n in (("bilinear", 94), ("bicubic", 47)):
        counts = [len(R.aa_taps32(mode, i, n, 2)[1]) for i in range(2)]
        assert max(counts) < R.RESIZE_MAX_TAPS and min(counts) > n // 2  # every tap present: the cap is not reached under the guard
        got = R.resize32(R.one_hots(2, n), (2, 2), mode)
        assert R.ratio(got, _interp(R.one_hots(2, n), (2, 2), mode), R.resize_bound(R.one_hots(2, n), (2, 2), mode) + 1e-45) <= 1.0


def test_resize_mutants_fail_their_cases():
    for mutant, case in R.RESIZE_MUTANTS.items():
        assert R.MUTANT_CASES[mutant] == "resize:" + case
        killed = []
        for (ih, iw), size in R.RESIZE_SHAPES:
            x = R.one_hots(ih, iw) if case == "onehot" else R.dense_image(3, ih, iw)
            for mode in (["nearest"] if mutant == "nearest_round" else ["bilinear", "bicubic"]):
                if R.first_bits_mismatch(R.resize32(x, size, mode, mutant), R.resize32(x, size, mode)) is not None:
                    killed.append((ih, iw, size, mode))
        assert killed, mutant
        print(mutant, "fails", len(killed), "cases")


# ------------------------------------------------------------------------------------------------ warp

def _pixels(grid, h, w):
    u, v = grid[..., 0].double().numpy(), grid[..., 1].double().numpy()
    return ((u + 1) * w - 1) / 2, ((v + 1) * h - 1) / 2


@pytest.mark.parametrize("env", R.ENVMAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mir", R.MIRRORS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_positions_are_inside_the_position_bound(mir, env):
    (h, w), (oh, ow) = mir, env
    pos = R.warp_positions(oh, ow, h, w)
    px, py = _pixels(ot.envmap_grid(oh, ow), h, w)
    rx, ry = R.ratio(px, pos["raw_x"], pos["ex"]), R.ratio(py, pos["raw_y"], pos["ey"])
    print(mir, env, "oracle fp32 position / bound", round(rx, 3), round(ry, 3), "largest finite bound (pixels)",
          float(np.max(pos["ex"][np.isfinite(pos["ex"])])), "infinite at", int(np.isinf(pos["ex"]).sum()), "texels")
    assert rx <= 1.0 and ry <= 1.0
    assert np.isinf(pos["ex"]).sum() <= 2  # only the singular direction may be free, and only where a texel centre sits on it


@pytest.mark.parametrize("env", R.ENVMAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tap_restatement_agrees_with_the_oracle(env):
    """tap_weights32 at the oracle's fp32 positions, applied to a random mirror, against the oracle's grid_sample"""
    h, w = 8, 8
    oh, ow = env
    g = ot.envmap_grid(oh, ow)
    wt = R.tap_weights32(g[..., 0].numpy(), g[..., 1].numpy(), h, w)
    assert ((wt != 0).sum((2, 3)) <= 4).all() and np.allclose(wt.sum((2, 3)), 1.0, atol=4 * R.U)
    mirror = R.dense_image(3, h, w, seed=4)
    got = np.einsum("ijyx,cyx->cij", wt.astype(np.float64), mirror.astype(np.float64))
    want = ot.mirmap2envmap(T(mirror)[None], env)[0].numpy()
    bound = 8 * R.U * np.einsum("ijyx,cyx->cij", np.abs(wt).astype(np.float64), np.abs(mirror).astype(np.float64))
    assert R.ratio(want, got, bound) <= 1.0


@pytest.mark.parametrize("env", R.ENVMAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_share_of_undetermined_texels(env):
    pos = R.warp_positions(env[0], env[1], 8, 8)
    det = R.determinate(pos, 8, 8)
    share = 1.0 - det.mean()
    print(env, "texels whose taps the float64 position does not decide:", int((~det).sum()), "of", det.size)
    assert share < 0.05
    # where it decides, the restatement at the rounded float64 position has the float64 position's texel
    x0, y0, *_ = R.taps32(pos["u"].astype(F), pos["v"].astype(F), 8, 8)
    assert (x0[det] == np.floor(pos["ix"][det])).all() and (y0[det] == np.floor(pos["iy"][det])).all()


def _ramp_expected(pos):
    return np.stack([np.ones_like(pos["ix"]), pos["ix"], pos["iy"]])


def test_warp_mutants_fail_their_cases():
    """the oracle's output on the ramp / one-hot / basis inputs is correct fp32 arithmetic: inside the bound of the reference, outside the
    bound of every mutant's expectation on at least one shape"""
    killed = {m: 0 for m in R.WARP_MUTANTS}
    for (h, w) in R.MIRRORS:
        for (oh, ow) in R.ENVMAPS:
            ramp = R.ramp_maps(h, w)
            out = ot.mirmap2envmap(T(ramp), (oh, ow))[0].double().numpy()
            pos = R.warp_positions(oh, ow, h, w)
            bx, by = R.ramp_eval_bound(h, w)
            bound = np.stack([np.full_like(pos["ex"], 4 * R.U), pos["ex"] + bx, pos["ey"] + by])
            assert R.ratio(out, _ramp_expected(pos), bound) <= 1.0
            for mutant, kw in (("align_corners", dict(align_corners=True)), ("no_border_clamp", dict(clamp=False)),
                               ("azimuth_not_reversed", dict(reverse_azimuth=False))):
                mp = R.warp_positions(oh, ow, h, w, **kw)
                with np.errstate(all="ignore"):
                    bad = np.abs(out - _ramp_expected(mp)) > np.stack([np.full_like(mp["ex"], 4 * R.U), mp["ex"] + bx, mp["ey"] + by])
                killed[mutant] += int(bad.any())
            # basis: ramp * basis warped with the division is the ramp's warp; without it, it is not
            basis = R.power2_basis(3, h, w)
            skipped = ot.mirmap2envmap(T(ramp * basis[None]), (oh, ow))[0].double().numpy()
            divided = ot.mirmap2envmap(T(ramp * basis[None]), (oh, ow), basis=T(basis))[0].double().numpy()
            assert R.ratio(divided, _ramp_expected(pos), bound) <= 1.0
            killed["basis_skipped"] += int((np.abs(skipped - _ramp_expected(pos)) > bound).any())
            if (h, w) == (8, 8):
                g = ot.envmap_grid(oh, ow)
                good = R.tap_weights32(g[..., 0].numpy(), g[..., 1].numpy(), h, w)
                swapped = R.tap_weights32(g[..., 0].numpy(), g[..., 1].numpy(), h, w, "taps_swapped")
                tol = (pos["ex"] + pos["ey"] + 4 * R.U)[..., None, None]
                killed["taps_swapped"] += int((np.abs(good.astype(np.float64) - swapped) > tol).any())
    assert R.MUTANT_CASES["taps_swapped"] == "warp:onehot" and R.MUTANT_CASES["basis_skipped"] == "warp:basis"
    assert all(v > 0 for v in killed.values()), killed


def test_every_mutant_has_a_case():
    want = {"chain_reversed", "clamp_after_exp", "image0_vectors", "mask_not_broadcast", "min_without_substitute", "range_image0", "unlit_counted",
            "clip_missing", "scale_image0", "threshold_missing", "mask_ignored", "gamma_not_inverted"} | set(R.RESIZE_MUTANTS) | set(R.WARP_MUTANTS)
    assert set(R.MUTANT_CASES) == want

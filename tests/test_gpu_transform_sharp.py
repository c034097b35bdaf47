"""The six kernels of csrc/transform.hip (drm_map_chain, drm_masked_log_range, drm_luminance_scale, drm_mirmap2envmap, drm_hdr2ldr, drm_resize)
through drmnet_amd.ops / drmnet_amd.dataset / drmnet_amd.transform, against tests/transform_ref.py: bit equality with the order-faithful fp32
restatements where the arithmetic is algebraic, float64 references with bounds counted from the kernel's arithmetic where the device's libm is
involved.  tests/test_transform_ref_cpu.py shows on the CPU that the premises hold and that every mutant of R.MUTANT_CASES fails its case here;
DESIGN.md "Transform-kernel checks" has the rules, the bounds and the figures.

Every bounded test prints `RATIO <case> <worst error / bound>` (run with -s).  Measured on the MI355X (131 cases in about a second), worst
error / bound of every bounded case; a libm call is charged torch's CPU figure plus 2 ulps (2.52 ... 2.89):

  test_libm_op_bound      log_p1 0.833, log10 0.625, norm_log 0.561, exp_m1 0.616 (clamp 20) / 0.616 (none), exp10 0.336 / 0.339
                          device ulp distance from float64 of the call alone: log10f 1.636, powf 1.210 (torch's CPU: 0.520, 0.577)
  test_project_chain      log_fwd 0.651, log_inv 0.373, log_inv_nocap 0.373, obs_fwd 0.558, obs_inv 0.564, est_div_clip0 0.998 (one correctly
                          rounded division against a bound of one rounding), est_mul_log 0.644
  test_chain_of_eight_..  chain8 0.356, chain9 0.358
  test_ragged_per_image   per_image 1, 3, 4, 5, 63, 1025: obs_inv 0.228, 0.368, 0.261, 0.368, 0.428, 0.564;
                          est_mul_log 0.317, 0.451, 0.366, 0.451, 0.562, 0.644
  test_masked_log_range   tiny_3x5 0.415, 513 0.415, channel2_only 0.009, masked_out_max 0.052, empty_mask 0 (-Inf, -Inf), batch3 0.381
  test_luminance_scale    hw1 0.101, hw511 0.019, hw513 0.106, unlit_and_dim 0.109, batch3 0.079; nothing_lit NaN
  test_warp_ramp          mirror 8 x 8, envmaps 4 x 8 / 10 x 28 / 7 x 5: plain 0.096 / 0.250 / 0.106, basis the same, log 0.218 each
                          mirror 5 x 9: plain 0.104 / 0.500 / 0.094, basis the same, log 0.218 each (0.250 and 0.500 are the constant channel
                          one ulp from 1 against its 2 ulps); no texel had an infinite bound
  test_warp_onehot        envmaps 4 x 8, 10 x 28, 7 x 5: 0.082, 0.149, 0.098; texels left out of the tap-block check: 0 of 32, 280, 35
  test_warp_batch_loop    0.016
  test_warp_channels_last C = 1, 3, 5: 0.002, 0.004, 0.003, and bit-equal to the NCHW output
  test_tonemap            hw1 0.105, hw1023 0.232, hw1025 0.202, threshold 0.140, mask_brightest 0.188, alpha_gamma 0.136; nothing_lit NaN
The other tests compare bits or classes (NaN, Inf) and have no ratio.
"""
import math

import numpy as np
import pytest
import torch

import transform_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def G(a, dev, dtype=F):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def report(case, r):
    print(f"RATIO {case} {r:.3f}")
    return r


def assert_bits(out, ref, what=""):
    bad = R.first_bits_mismatch(out, ref)
    assert bad is None, f"{what}: {bad}"


def run_chain(dev, steps, x, lo=None, hi=None, sc=None, **kw):
    from drmnet_amd import ops

    b = x.shape[0]
    v = lambda t: None if t is None else G(t, dev)
    return N(ops.map_chain(G(x, dev).reshape(b, 1, 1, -1), steps, lo=v(lo), hi=v(hi), scale=v(sc), **kw)).reshape(b, -1)


# ------------------------------------------------------------------------------------------------ map chain

@pytest.mark.parametrize("name", R.ALGEBRAIC)
def test_algebraic_op_bits(dev, name):
    """0, -0, denormals, +-Inf, NaN, both sides of every threshold; three images with their own lo / hi / scale"""
    sweep = R.algebraic_sweep()
    x = np.stack([sweep, sweep[::-1], np.roll(sweep, 7)])
    lo, hi, sc = np.array([-2.5, -1.0, 0.25], F), np.array([1.75, 3.0, 0.5], F), np.array([0.37, 3.0, 1e-3], F)
    got = run_chain(dev, [(name, 0.5)], x, lo, hi, sc)
    assert_bits(got, R.map32(name, 0.5, x, lo[:, None], hi[:, None], sc[:, None]), name)


@pytest.mark.parametrize("name", R.LIBM)
def test_libm_op_bound(dev, name):
    if name in ("exp_m1", "exp10"):
        x = np.concatenate([np.linspace(-30.0, 30.0, 3001), [19.99, 20.0, 20.01, 21.0, 25.0, np.inf, -np.inf, np.nan]]).astype(F)[None]
    else:
        x = np.concatenate([np.geomspace(1e-7, 1e5, 3001), np.linspace(0.5, 2.0, 1001), [0.0, -0.0, -1.0, -1e-3, np.inf, np.nan]]).astype(F)[None]
    lo, hi = np.array([-3.0], F), np.array([2.25], F)
    for arg in ((R.CAP, math.inf) if name in ("exp_m1", "exp10") else (0.0,)):
        got = run_chain(dev, [(name, arg)], x, lo, hi)
        ref, bound = R.chain64([(name, arg)], x, lo, hi)
        assert report(f"libm:{name}:{arg}", R.ratio(got, ref, bound)) <= 1.0
        if name == "log10":
            assert got[0, -6] == -np.inf and got[0, -5] == -np.inf and np.isnan(got[0, -4]) and np.isnan(got[0, -3])  # log10(+-0), log10(< 0)
        if name in ("log10", "exp10"):  # the call alone: the device's ulp distance from float64
            fin = np.isfinite(ref[0]) & (np.abs(ref[0]) > 1e-37) & (np.abs(ref[0]) < 3e38)
            print(f"ULP device {'log10f' if name == 'log10' else 'powf'} {R._ulp_dist(got[0][fin], ref[0][fin]):.3f}")


@pytest.mark.parametrize("name", list(R.CHAINS))
def test_project_chain(dev, name):
    """every chain the project compiles, through BaseDataset where a config compiles it and through ops.map_chain for estimate's two"""
    from drmnet_amd.dataset import BaseDataset

    x, lo, hi, sc = R.chain_inputs(name, 3, 1025)
    ref, bound = R.chain64(R.CHAINS[name], x, lo, hi, sc)
    if name.startswith("est"):
        got = run_chain(dev, R.CHAINS[name], x, sc=sc)
    else:
        func = "log" if name.startswith("log") else "0p1tom1p1_normalizedLogarithmic_lowerbound1e-6"
        ds = BaseDataset(25, func, clamp_before_exp=0.0 if name.endswith("nocap") else R.CAP)
        assert (ds._inverse if "inv" in name else ds._forward[0]) == R.CHAINS[name]
        ds.Logarithmic_params = [G(lo, dev).view(-1, 1, 1, 1), G(hi, dev).view(-1, 1, 1, 1)]
        t = G(x, dev).reshape(3, 1, 25, 41)
        got = N(ds.rescale(t) if "inv" in name else ds.transform(t)).reshape(3, -1)
    assert report(f"chain:{name}", R.ratio(got, ref, bound)) <= 1.0


def test_norm_log_with_equal_bounds(dev):
    x = np.array([[1.0, 10.0, 0.1, 0.0, 3.0]], dtype=F)
    lo = hi = np.array([0.0], dtype=F)
    ref, bound = R.chain64([("norm_log", 0.0)], x, lo, hi)
    got = run_chain(dev, [("norm_log", 0.0)], x, lo, hi)
    assert R.ratio(got, ref, bound) == 0.0 and np.isnan(got[0, 0]) and got[0, 1] == np.inf and got[0, 2] == -np.inf


ALG9 = [("img_mul", 0.0), ("unit_to_signed", 0.0), ("lowerbound", -0.75), ("denorm_log", 0.0), ("signed_to_unit", 0.0), ("img_div", 0.0), ("clip0", 0.0),
        ("unit_to_signed", 0.0), ("img_mul", 0.0)]


def alg_chain32(steps, x, lo, hi, sc):
    v = x
    for name, arg in steps:
        v = R.map32(name, arg, v, lo[:, None], hi[:, None], sc[:, None])
    return v


@pytest.mark.parametrize("per", R.RAGGED)
def test_ragged_per_image(dev, per):
    """B = 3: odd images start off a quad boundary; lo / hi / scale distinct per image.  An algebraic chain bit for bit, two libm chains bounded."""
    x, lo, hi, sc = R.chain_inputs("est_mul_log", 3, per)
    assert_bits(run_chain(dev, ALG9[:5], x, lo, hi, sc), alg_chain32(ALG9[:5], x, lo, hi, sc), f"per_image {per}")
    for name in ("obs_inv", "est_mul_log"):
        x, lo, hi, sc = R.chain_inputs(name, 3, per)
        ref, bound = R.chain64(R.CHAINS[name], x, lo, hi, sc)
        assert report(f"ragged:{name}:{per}", R.ratio(run_chain(dev, R.CHAINS[name], x, lo, hi, sc), ref, bound)) <= 1.0


def test_chain_of_eight_and_of_nine(dev):
    """8 ops are one pass; 9 take two, the second in place"""
    x, lo, hi, sc = R.chain_inputs("est_mul_log", 3, 1025)
    for name, steps in (("chain8", R.CHAIN8), ("chain9", R.CHAIN9)):
        ref, bound = R.chain64(steps, x, lo, hi, sc)
        assert report(name, R.ratio(run_chain(dev, steps, x, lo, hi, sc), ref, bound)) <= 1.0
    assert len(ALG9) == 9
    assert_bits(run_chain(dev, ALG9[:8], x, lo, hi, sc), alg_chain32(ALG9[:8], x, lo, hi, sc), "8 algebraic ops")
    assert_bits(run_chain(dev, ALG9, x, lo, hi, sc), alg_chain32(ALG9, x, lo, hi, sc), "9 algebraic ops")


def test_in_place(dev):
    from drmnet_amd import ops

    x, lo, hi, sc = R.chain_inputs("est_mul_log", 3, 1025)
    for steps in (R.CHAIN9, ALG9, R.CHAINS["log_fwd"]):
        t = G(x, dev).reshape(3, 1, 25, 41)
        want = N(ops.map_chain(t, steps, lo=G(lo, dev), hi=G(hi, dev), scale=G(sc, dev)))
        assert_bits(N(t).reshape(3, -1), x, "the input of an out-of-place call")
        res = ops.map_chain(t, steps, lo=G(lo, dev), hi=G(hi, dev), scale=G(sc, dev), out=t)
        assert res.data_ptr() == t.data_ptr()
        assert_bits(N(t), want, "out = x")


@pytest.mark.parametrize("per", [256, 343])
@pytest.mark.parametrize("off_x,off_out", [(o, 0) for o in (1, 2, 3)] + [(0, o) for o in (1, 2, 3)] + [(1, 1), (2, 3), (3, 1)])
def test_views_off_the_16_byte_boundary(dev, off_x, off_out, per):
    """contiguous views at a storage offset of 1, 2 or 3 elements (4-byte but not 16-byte aligned), for x, for out and for both: bit-equal to the
    aligned run.  per = 256 would take the float4 path for every quad from the element index alone."""
    from drmnet_amd import ops

    x, lo, hi, sc = R.chain_inputs("est_mul_log", 3, per)
    kw = dict(lo=G(lo, dev), hi=G(hi, dev), scale=G(sc, dev))
    steps = ALG9[:6] + [("log_p1", 0.0)]
    aligned = G(x, dev).reshape(3, 1, 1, per)
    assert aligned.data_ptr() % 16 == 0
    want = N(ops.map_chain(aligned, steps, **kw))
    n = 3 * per
    xbuf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    obuf = torch.full((n + 8,), 7.0, dtype=torch.float32, device=dev)
    xv = xbuf[off_x:off_x + n].view(3, 1, 1, per)
    xv.copy_(aligned)
    ov = obuf[off_out:off_out + n].view(3, 1, 1, per)
    assert xv.is_contiguous() and ov.is_contiguous() and xv.data_ptr() % 16 == 4 * off_x and ov.data_ptr() % 16 == 4 * off_out
    res = ops.map_chain(xv, steps, out=ov, **kw)
    assert res.data_ptr() == ov.data_ptr()
    assert_bits(N(ov), want, f"offsets {off_x}, {off_out}")
    rest = N(obuf)
    assert (rest[:off_out] == 7.0).all() and (rest[off_out + n:] == 7.0).all()  # nothing written outside the view


def test_out_is_checked(dev):
    from drmnet_amd import ops

    x = torch.ones((2, 3, 4, 4), dtype=torch.float32, device=dev)
    steps = [("clip0", 0.0)]
    for bad in (torch.empty((2, 3, 4, 5), dtype=torch.float32, device=dev), torch.empty((2, 3, 4, 4), dtype=torch.float64, device=dev),
                torch.empty((2, 3, 4, 4), dtype=torch.float32), torch.empty((2, 3, 4, 8), dtype=torch.float32, device=dev)[..., ::2],
                torch.empty((2, 4, 4, 3), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)):
        with pytest.raises(RuntimeError):
            ops.map_chain(x, steps, out=bad)
    with pytest.raises(RuntimeError):
        ops.map_chain(x, [], out=torch.empty((2, 3, 4, 5), dtype=torch.float32, device=dev))


# ------------------------------------------------------------------------------------------------ ranges and scale

@pytest.mark.parametrize("name", R.RANGE_CASES)
def test_masked_log_range(dev, name):
    from drmnet_amd import ops

    x, m = R.range_case(name)
    lo, hi, blo, bhi = R.range64(x, m)
    glo, ghi = ops.masked_log_range(G(x, dev), G(m, dev))
    assert report(f"range:{name}", max(R.ratio(N(glo), lo, blo), R.ratio(N(ghi), hi, bhi))) <= 1.0
    if name == "empty_mask":
        assert N(glo)[0] == -np.inf and N(ghi)[0] == -np.inf


@pytest.mark.parametrize("name", R.LUM_CASES)
def test_luminance_scale(dev, name):
    from drmnet_amd import ops

    x = R.lum_case(name)
    s, rel = R.lumscale64(x, 0.12)
    got = N(ops.luminance_scale(G(x, dev), 0.12))
    if name == "nothing_lit":
        assert np.isnan(s).all() and np.isnan(got).all()
        return
    assert report(f"lum:{name}", R.ratio(got, s, np.abs(s) * rel)) <= 1.0


@pytest.mark.parametrize("name", R.POISON_CASES)
def test_poison_survives(dev, name):
    """a bad value reaches the output as in the reference, and only the image that holds it"""
    from drmnet_amd import ops

    if name.startswith("range"):
        x, m = R.poison_case(name)
        lo, hi, blo, bhi = R.range64(x, m)
        assert np.isnan(lo[1]) and np.isnan(hi[1])
        glo, ghi = ops.masked_log_range(G(x, dev), G(m, dev))
        assert np.isnan(N(glo)[1]) and np.isnan(N(ghi)[1])
        assert R.ratio(N(glo), lo, blo) <= 1.0 and R.ratio(N(ghi), hi, bhi) <= 1.0
    elif name == "lum_nan":
        (x,) = R.poison_case(name)
        s, rel = R.lumscale64(x, 0.12)
        got = N(ops.luminance_scale(G(x, dev), 0.12))
        assert np.isnan(got).tolist() == [False, True, False] and R.ratio(got, s, np.abs(s) * rel) <= 1.0
    else:
        x, m, a, g = R.poison_case(name)
        ref, _ = R.tonemap64(x, m, a, g)
        assert np.isnan(ref).all()
        assert np.isnan(N(ops.hdr2ldr(G(x, dev), G(m, dev, np.uint8), a, g))).all()


def test_tonemap_lit_inf_pixel(dev):
    """a lit +Inf pixel: the coefficient is alpha / Inf = 0, the element itself Inf * 0 = NaN, every other element exactly 0"""
    from drmnet_amd import ops

    x, m, a, g = R.tone_case("hw1025")
    x = x.copy()
    x[0, 3, 1] = np.inf
    ref, bound = R.tonemap64(x, m, a, g)
    assert np.isnan(ref).sum() == 1 and np.isnan(ref[3, 1]) and (np.delete(ref.reshape(-1), 10) == 0).all() and np.isfinite(np.delete(bound.reshape(-1), 10)).all()
    got = N(ops.hdr2ldr(G(x, dev), None, a, g)).reshape(-1)
    assert np.isnan(got[10]) and (np.delete(got, 10) == 0).all()


# ------------------------------------------------------------------------------------------------ resize

SHAPE_IDS = [f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in R.RESIZE_SHAPES]


def run_resize(dev, x, size, mode):
    from drmnet_amd import ops

    return N(ops.resize(G(x, dev), size, mode))


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=SHAPE_IDS)
def test_resize_onehot_bits(dev, shape, mode):
    """planes = IH * IW one-hot images: the whole weight tensor wy (x) wx of every output pixel"""
    (ih, iw), size = shape
    x = R.one_hots(ih, iw)
    assert_bits(run_resize(dev, x, size, mode), R.resize32(x, size, mode), "resize:onehot")


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
@pytest.mark.parametrize("shape", R.RESIZE_SHAPES + [((20, 20), (17, 19))], ids=SHAPE_IDS + ["20x20to17x19"])
def test_resize_dense_bits(dev, shape, mode):
    """a dense random image (the loop order shows only here); 17 x 19 = 323 outputs: two blocks, the second ragged"""
    (ih, iw), size = shape
    x = R.dense_image(3, ih, iw)
    assert_bits(run_resize(dev, x, size, mode), R.resize32(x, size, mode), "resize:dense")
    if shape not in R.RESIZE_SHAPES:
        # the extra shape is here for its ragged second block.  Its bicubic weights sum to 1.3 in magnitude over six taps an axis: the
        # restatement (to which the device is bit-equal above) leaves the constant by 3 ulps and ATen's own passes by 4, on the CPU
        return
    c = np.full((1, ih, iw), 0.7, dtype=F)
    got = run_resize(dev, c, size, mode)
    assert np.abs(got.astype(np.float64) - float(F(0.7))).max() <= 2 * float(np.spacing(F(0.7))), "a constant image stays constant within 2 ulps"


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_resize_largest_downscale(dev, mode, axis):
    """the largest down-scaling the host guard 2 half smax + 2 <= 96 admits, one axis at a time (the other has length 2): bit-equal with every
    tap present; the next length is refused"""
    ok, refused = R.max_downscale(mode)
    shape = (ok, 2) if axis == 0 else (2, ok)
    x = R.one_hots(*shape)
    want = R.resize32(x, (2, 2), mode)
    assert (want != 0).reshape(2 * ok, -1).any(1).all(), "a tap is missing from the restatement"
    assert_bits(run_resize(dev, x, (2, 2), mode), want, "resize:onehot at the largest down-scaling")
    bad = R.dense_image(1, *((refused, 2) if axis == 0 else (2, refused)))
    with pytest.raises(RuntimeError):
        run_resize(dev, bad, (2, 2), mode)


@pytest.mark.parametrize("mode", R.RESIZE_MODES)
def test_resize_plane_loop(dev, mode):
    """4097 planes: past the 4096 rows of the grid, so plane 4096 is the second trip of a block's plane loop; every plane distinct"""
    x = R.dense_image(4097, 4, 4)
    assert len({p.tobytes() for p in x}) == 4097
    assert_bits(run_resize(dev, x, (2, 2), mode), R.resize32(x, (2, 2), mode), "plane loop")


# ------------------------------------------------------------------------------------------------ mirror-ball warp

PAIRS = [(m, e) for m in R.MIRRORS for e in R.ENVMAPS]
PAIR_IDS = [f"mir{m[0]}x{m[1]}env{e[0]}x{e[1]}" for m, e in PAIRS]


@pytest.mark.parametrize("variant", ["plain", "log", "basis"])
@pytest.mark.parametrize("mir,env", PAIRS, ids=PAIR_IDS)
def test_warp_ramp(dev, mir, env, variant):
    """the maps 1, x, y: bilinear sampling of an affine map returns the clamped sample position itself, so the output is (1, ix, iy) at EVERY
    texel, within the position bound (which grows towards the singular direction instead of leaving a texel out)"""
    from drmnet_amd import ops

    (h, w), (oh, ow) = mir, env
    pos = R.warp_positions(oh, ow, h, w)
    ramp = R.ramp_maps(h, w)
    bx, by = R.ramp_eval_bound(h, w)
    want = np.stack([np.ones_like(pos["ix"]), pos["ix"], pos["iy"]])
    bound = np.stack([np.full_like(pos["ex"], 2 * 2.0 ** -23), pos["ex"] + bx, pos["ey"] + by])
    if variant == "plain":
        got = N(ops.mirmap2envmap(G(ramp, dev), env))[0]
    elif variant == "basis":
        basis = R.power2_basis(3, h, w)
        got = N(ops.mirmap2envmap(G(ramp * basis[None], dev), env, basis=G(basis, dev)))[0]
    else:
        # exp(ramp), interpolated in log scale: each tap's logf sees the rounded exp (u) and adds K ulps of the coordinate; expf on top
        got = N(ops.mirmap2envmap(G(np.exp(ramp.astype(np.float64)), dev), env, log_scale_interpolation=True))[0]
        e_acc = bound + (R.K("logf") * 2 + 1) * R.U * np.maximum(want, 1.0)
        want = np.exp(want)
        bound = want * (np.expm1(e_acc) + R.K("expf") * 2 * R.U)
    r = [R.ratio(got[c], want[c], bound[c]) for c in range(3)]
    assert report(f"warp:{variant}:{h}x{w}:{oh}x{ow}", max(r)) <= 1.0, r


@pytest.mark.parametrize("env", R.ENVMAPS, ids=[f"{e[0]}x{e[1]}" for e in R.ENVMAPS])
def test_warp_onehot(dev, env):
    """B = 64 one-hots of an 8 x 8 mirror: every texel's taps.  At most four, in one 2 x 2 block clipped at the border; the weights are the
    restatement's at the rounded float64 position, within the position bound (bilinear weights are continuous, so at every texel); the block is
    the float64 position's wherever that position decides it (R.determinate)."""
    from drmnet_amd import ops

    h = w = 8
    oh, ow = env
    pos = R.warp_positions(oh, ow, h, w)
    got = N(ops.mirmap2envmap(G(R.one_hots(h, w)[:, None], dev), env))[:, 0].reshape(h, w, oh, ow).transpose(2, 3, 0, 1)  # [oh, ow, y, x]
    want = R.tap_weights32(pos["u"].astype(F), pos["v"].astype(F), h, w)
    tol = (pos["ex"] + pos["ey"] + 4 * R.U)[..., None, None]
    assert report(f"warp:onehot:{oh}x{ow}", R.ratio(got, want, np.broadcast_to(tol, got.shape))) <= 1.0
    nz = got != 0
    assert (nz.sum((2, 3)) <= 4).all()
    ys, xs = nz.any(3), nz.any(2)
    span = lambda a: np.where(a.any(2), a.shape[2] - 1 - np.argmax(a[..., ::-1], 2) - np.argmax(a, 2), 0)
    assert (span(ys) <= 1).all() and (span(xs) <= 1).all(), "the taps are not one 2 x 2 block"
    det = R.determinate(pos, h, w)
    share = 1.0 - det.mean()
    print(f"SHARE warp:onehot:{oh}x{ow} left out {int((~det).sum())} of {det.size}")
    assert share < 0.05
    x0, y0 = np.floor(pos["ix"]).astype(int), np.floor(pos["iy"]).astype(int)
    yy, xx = np.arange(h)[None, None, :, None], np.arange(w)[None, None, None, :]
    block = (yy >= y0[..., None, None]) & (yy <= y0[..., None, None] + 1) & (xx >= x0[..., None, None]) & (xx <= x0[..., None, None] + 1)
    assert not (nz & ~block)[det].any(), "a tap outside the float64 position's block"
    main_got, main_want = got[det][np.arange(det.sum()), y0[det], x0[det]], want[det][np.arange(det.sum()), y0[det], x0[det]]
    assert (main_got > 0)[main_want > tol[det][:, 0, 0]].all(), "the block's first tap is missing"


def test_warp_batch_loop(dev):
    """B = 1025 of 4 x 4 -> 2 x 4: image 1024 is the second trip of the batch loop.  Every image against the float64 weights; images 0, 1023 and
    1024 bit-equal to a launch of their own."""
    from drmnet_amd import ops

    mir = R.dense_image(1025, 4, 4, seed=2)[:, None]
    got = N(ops.mirmap2envmap(G(mir, dev), (2, 4)))
    pos = R.warp_positions(2, 4, 4, 4)
    wt = R.tap_weights32(pos["u"].astype(F), pos["v"].astype(F), 4, 4).astype(np.float64)
    want = np.einsum("ijyx,byx->bij", wt, mir[:, 0].astype(np.float64))
    bound = (pos["ex"] + pos["ey"] + 8 * R.U)[None] * np.abs(mir[:, 0]).sum((1, 2))[:, None, None]
    assert report("warp:batch_loop", R.ratio(got[:, 0], want, bound)) <= 1.0
    for b in (0, 1023, 1024):
        assert_bits(N(ops.mirmap2envmap(G(mir[b:b + 1], dev), (2, 4)))[0], got[b], f"image {b}")


@pytest.mark.parametrize("c", [1, 3, 5])
def test_warp_channels_last(dev, c):
    from drmnet_amd import ops

    mir = np.abs(R.dense_image(2 * c, 5, 9, seed=c)).reshape(2, c, 5, 9) + F(0.1)
    basis = R.power2_basis(c, 5, 9)
    for kw in (dict(), dict(basis=G(basis, dev)), dict(log_scale_interpolation=True)):
        a = N(ops.mirmap2envmap(G(mir, dev), (7, 5), **kw))
        b = N(ops.mirmap2envmap(G(mir, dev), (7, 5), channels_last=True, **kw))
        assert b.shape == (2, 7, 5, c)
        assert_bits(b.transpose(0, 3, 1, 2), a, f"channels_last, C = {c}")
    pos = R.warp_positions(7, 5, 5, 9)
    wt = R.tap_weights32(pos["u"].astype(F), pos["v"].astype(F), 5, 9).astype(np.float64)
    a = N(ops.mirmap2envmap(G(mir, dev), (7, 5)))
    want = np.einsum("ijyx,bcyx->bcij", wt, mir.astype(np.float64))
    bound = (pos["ex"] + pos["ey"] + 8 * R.U)[None, None] * np.abs(mir).sum((2, 3))[:, :, None, None]
    assert report(f"warp:channels:{c}", R.ratio(a, want, bound)) <= 1.0


# ------------------------------------------------------------------------------------------------ tone map

@pytest.mark.parametrize("name", R.TONE_CASES)
def test_tonemap(dev, name):
    from drmnet_amd.transform import hdr2ldr

    x, m, alpha, gamma = R.tone_case(name)
    ref, bound = R.tonemap64(x, m, alpha, gamma)
    got = hdr2ldr(x, m, alpha, gamma).reshape(-1, 3)
    if name == "nothing_lit":
        assert np.isnan(ref).all() and np.isnan(got).all()
        return
    assert report(f"tone:{name}", R.ratio(got, ref, bound)) <= 1.0

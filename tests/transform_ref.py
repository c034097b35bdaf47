"""CPU helpers of the sharp checks of the six kernels of csrc/transform.hip (tests/test_transform_ref_cpu.py, tests/test_gpu_transform_sharp.py;
DESIGN.md "Transform-kernel checks").  numpy / torch on the CPU only; from the package it reads nothing but the op-code table ops.MAP_CODES.

(a) Order-faithful fp32 restatements.  The library is built with -ffp-contract=off and fp32 + - * / and floorf are correctly rounded on the
    device, so the algebraic maps (map32), the Rec.709 luminance (lum32), the resize in all three modes (resize32: index rule, filter
    polynomial, normalisation, loop order) and the taps of grid_sample_taps at an fp32 position (taps32) are restated in np.float32 in the
    kernel's own order of operations and compared bit for bit (bits_equal: NaN matches NaN, -0 does not match 0).

(b) Float64 references where the device's libm is involved (log_p1, log10, norm_log, exp_m1, exp10, the range statistics, the luminance scale,
    the tone map, the warp's sample position), each with a bound counted from the kernel's arithmetic, u = 2^-24:
      a correctly rounded op on a value r            u |r|
      a libm call returning r                        K[f] ulp(r), ulp(r) <= 2 u |r|
      an earlier absolute error d through f          |f'| d, e.g. d / (|t| ln 10) through log10, ln 10 * d (relative) through 10^x
    The fp32 constants of the kernel (0.1f, 1e-5f, 5e-5f, 1e-7f, the fp32 pi, 2.0f / pi, the luminance weights) are the reference's constants.
    K[f] is not fixed in advance: libm_ulps() measures the worst ulp distance of torch's CPU fp32 function from float64 over a fixed sweep of
    the argument range the kernels use, and K[f] = that + 2, the "ulp or two" between two libms that tests/test_gpu_transforms.py states.

(c) The warp's conditioning.  n = normalize(d + view): nz = 1 - sin(theta) cos(phi) cancels and len = |d + view| falls to zero at the middle
    row of the envmap's left and right edges, where the half vector's direction is undetermined.  warp_positions carries the component errors
    through the division (1 / len) and through atan2 / acos (1 / r, r the horizontal length of the unit half vector), both taken at their
    guarded lower ends (len - e_len, r - e_r); where the guard reaches zero the bound is infinite: every position passes there, no texel is
    left out.

(d) Mutants: each reference wrong in one way a kernel could be wrong, and the named case that fails for it (MUTANT_CASES).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
F = np.float32
C01, C1E5, C5E5, C1E7 = F(1e-1), F(1e-5), F(5e-5), F(1e-7)
LW = (F(0.212671), F(0.715160), F(0.072169))
PI32 = F(3.14159265358979323846)
TWO_OVER_PI = F(2.0) / PI32
LN10 = math.log(10.0)

MAP_CODES = {"log_p1": 0, "log10": 1, "lowerbound": 2, "unit_to_signed": 3, "norm_log": 4, "exp_m1": 5, "exp10": 6, "signed_to_unit": 7,
             "denorm_log": 8, "img_mul": 9, "img_div": 10, "clip0": 11}  # ops.MAP_CODES (the CPU test asserts that they are the same table)
ALGEBRAIC = ["lowerbound", "unit_to_signed", "signed_to_unit", "denorm_log", "img_mul", "img_div", "clip0"]
LIBM = ["log_p1", "log10", "norm_log", "exp_m1", "exp10"]
MAX_CHAIN = 8


def _gen(*key):
    return np.random.default_rng([int(k) for k in key])


def bits_equal(a, b):
    """elementwise: the same fp32 bits, or both NaN (a NaN's payload is not part of any rule)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def first_bits_mismatch(out, ref):
    ok = bits_equal(out, ref)
    if ok.all():
        return None
    i = tuple(int(v) for v in np.argwhere(~ok)[0])
    return f"{int((~ok).sum())} of {ok.size} differ; first at {i}: got {np.asarray(out)[i]!r}, want {np.asarray(ref)[i]!r}"


def ulp32(r):
    """the spacing of fp32 at |r| (float64 in, float64 out), never below the smallest denormal"""
    return np.spacing(np.abs(np.asarray(r, dtype=np.float64)).astype(F)).astype(np.float64)


def ratio(out, ref, bound):
    """worst |out - ref| / bound over the finite part, after asserting that the rest has the reference's class: NaN where it has NaN, the same
    infinity where it has one.  An infinite bound passes anything."""
    out = np.asarray(out, dtype=np.float64)
    ref, bound = np.broadcast_to(np.asarray(ref, dtype=np.float64), out.shape), np.broadcast_to(np.asarray(bound, dtype=np.float64), out.shape)
    free = np.isinf(bound)
    special = ~np.isfinite(ref) & ~free
    same = np.where(np.isnan(ref), np.isnan(out), out == ref)
    assert same[special].all(), f"class differs at {np.argwhere(special & ~same)[:4].tolist()}: got {out[special & ~same][:4]}, want {ref[special & ~same][:4]}"
    live = ~special & ~free
    if not live.any():
        return 0.0
    assert np.isfinite(out[live]).all(), f"not finite where the reference is: {np.argwhere(live & ~np.isfinite(out))[:4].tolist()}"
    err = np.abs(out[live] - ref[live])
    b = bound[live]
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))


# ------------------------------------------------------------------------------------------------ libm: measured ulp figures

def _ulp_dist(got32, want64):
    return float(np.max(np.abs(got32.astype(np.float64) - want64) / ulp32(want64)))


_LIBM = {}


def libm_ulps():
    """{function: worst ulp distance of torch's CPU fp32 function from float64} over fixed sweeps of the argument ranges the kernels use"""
    if _LIBM:
        return _LIBM
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F))
    geo = np.concatenate([np.geomspace(1e-7, 1e5, 120001), np.linspace(0.5, 2.0, 60001)]).astype(F)  # arguments of log10f / logf
    g64 = geo.astype(np.float64)
    _LIBM["log10f"] = _ulp_dist(torch.log10(t(geo)).numpy(), np.log10(g64))
    _LIBM["logf"] = _ulp_dist(torch.log(t(geo)).numpy(), np.log(g64))
    e = np.linspace(-37.0, 37.0, 148001).astype(F)  # exponents of 10^x
    _LIBM["powf"] = max(_ulp_dist(torch.pow(10.0, t(e)).numpy(), np.power(10.0, e.astype(np.float64))),
                        # and the tone map's t^(1 / gamma), t in (0, 1]
                        max(_ulp_dist(torch.pow(t(b), float(F(p))).numpy(), np.power(b.astype(np.float64), float(F(p))))
                            for p in (1 / 2.2, 1 / 1.8, 0.5) for b in [np.geomspace(1e-6, 1.0, 60001).astype(F)]))
    x = np.linspace(-16.0, 12.0, 112001).astype(F)
    _LIBM["expf"] = _ulp_dist(torch.exp(t(x)).numpy(), np.exp(x.astype(np.float64)))
    th = np.linspace(0.0, math.pi, 100001).astype(F)
    ph = np.linspace(-2 * math.pi, 0.0, 200001).astype(F)
    ang = np.concatenate([th, ph])
    a64 = ang.astype(np.float64)
    # sin / cos near a zero of theirs: the distance is in ulps of the float64 value, which is what the bound charges
    _LIBM["sinf"] = _ulp_dist(torch.sin(t(ang)).numpy(), np.sin(a64))
    _LIBM["cosf"] = _ulp_dist(torch.cos(t(ang)).numpy(), np.cos(a64))
    c = np.linspace(-1.0, 1.0, 200001).astype(F)
    _LIBM["acosf"] = _ulp_dist(torch.acos(t(c)).numpy(), np.arccos(c.astype(np.float64)))
    w = np.linspace(-math.pi, math.pi, 100001)
    ys = np.concatenate([np.sin(w) * s for s in (1.0, 0.37, 1e-3)]).astype(F)
    xs = np.concatenate([np.cos(w) * s for s in (1.0, 0.37, 1e-3)]).astype(F)
    _LIBM["atan2f"] = _ulp_dist(torch.atan2(t(ys), t(xs)).numpy(), np.arctan2(ys.astype(np.float64), xs.astype(np.float64)))
    return _LIBM


def K(name):
    """ulps charged for one call of the device's `name`: the CPU figure plus 2"""
    return libm_ulps()[name] + 2.0


# ------------------------------------------------------------------------------------------------ (a) algebraic maps, luminance

def map32(name, arg, v, lo=None, hi=None, sc=None):
    """apply_map of csrc/transform.hip for the algebraic ops, in np.float32; lo / hi / sc broadcast against v"""
    v = np.asarray(v, dtype=F)
    arg = F(arg)
    with np.errstate(all="ignore"):
        if name == "lowerbound":
            return np.where(v < arg, arg, v)
        if name == "unit_to_signed":
            return v * F(2) - F(1)
        if name == "signed_to_unit":
            return (v + F(1)) / F(2)
        if name == "denorm_log":
            return v * (hi - lo) + lo
        if name == "img_mul":
            return v * sc
        if name == "img_div":
            return v / sc
        if name == "clip0":
            return np.where(v < F(0), F(0), v)
    raise KeyError(name)


def algebraic_sweep(arg=0.5):
    """0, -0, denormals, +-Inf, NaN, both sides of every threshold (0, arg, -1, 0.5, 1), large and small normals, plus a random fill"""
    nx = lambda a, d: np.nextafter(F(a), F(d))
    pts = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754944e-38, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1e-30, -1e-30]
    for c in (0.0, arg, -1.0, 0.5, 1.0, 2.0):
        pts += [c, nx(c, np.inf), nx(c, -np.inf)]
    g = _gen(11)
    rnd = np.concatenate([g.standard_normal(200), np.exp(g.standard_normal(200) * 8), -np.exp(g.standard_normal(100) * 8)])
    return np.concatenate([np.array(pts, dtype=F), rnd.astype(F)])


def lum32(r, g, b):
    return (LW[0] * np.asarray(r, dtype=F) + LW[1] * np.asarray(g, dtype=F)) + LW[2] * np.asarray(b, dtype=F)


# ------------------------------------------------------------------------------------------------ (b) map chains in float64, with bounds

def _d(a):
    return np.asarray(a, dtype=np.float64)


def step64(name, arg, v, e, lo, hi, sc, clamp_after=False):
    """one map on the float64 value v that the fp32 value matches within e -> (value, bound).  lo / hi / sc: float64 views of the fp32 vectors."""
    arg = float(F(arg)) if np.isfinite(arg) else arg
    with np.errstate(all="ignore"):
        if name in ("lowerbound", "clip0"):
            return np.where(v < (arg if name == "lowerbound" else 0.0), arg if name == "lowerbound" else 0.0, v), e
        if name == "unit_to_signed":
            r = v * 2 - 1
            return r, 2 * e + U * np.abs(r)
        if name == "signed_to_unit":
            t = v + 1
            return t / 2, (e + U * np.abs(t)) / 2
        if name == "denorm_log":
            den = hi - lo
            p = v * den
            r = p + lo
            return r, e * np.abs(den) + 2 * U * np.abs(p) + U * np.abs(r)  # (den's rounding, the product's, the sum's)
        if name == "img_mul":
            r = v * sc
            return r, e * np.abs(sc) + U * np.abs(r)
        if name == "img_div":
            r = v / sc
            return r, e / np.abs(sc) + U * np.abs(r)
        if name in ("log_p1", "log10", "norm_log"):
            t, et = (v + float(C01), e + U * np.abs(v + float(C01))) if name == "log_p1" else (v, e)
            y = np.log10(t)
            ey = et / (np.maximum(np.abs(t) - et, 0.0) * LN10) + K("log10f") * ulp32(y)
            ey = np.where(np.isfinite(y), ey, 0.0)  # log10(0) = -Inf and log10(negative) = NaN are classes, not numbers
            if name == "log10":
                return y, ey
            if name == "log_p1":
                return y + 1, ey + U * np.abs(y + 1)
            d, den = y - lo, hi - lo
            ed = ey + U * np.abs(d)
            q = d / den
            return q, np.where(den == 0, 0.0, ed / np.abs(den) + 2 * U * np.abs(q))
        if name in ("exp_m1", "exp10"):
            c, ec = (v - 1, e + U * np.abs(v - 1)) if name == "exp_m1" else (v, e)
            if not clamp_after:
                c = np.minimum(c, arg)
            p = np.power(10.0, c)
            if clamp_after:
                p = np.minimum(p, arg)
            ep = p * (np.expm1(LN10 * ec) + K("powf") * 2 * U)  # 10^(c +- ec): exact, not first order
            ep = np.where(np.isfinite(p), np.maximum(ep, K("powf") * ulp32(p)), 0.0)
            if name == "exp10":
                return p, ep
            r = p - float(C01)
            return r, ep + U * np.abs(r)
    raise KeyError(name)


def chain64(steps, x, lo=None, hi=None, sc=None, reverse=False, clamp_after=False, image0=False):
    """steps on x [B, per] fp32 -> (float64 value, bound) [B, per]; the keyword arguments make the mutants"""
    v = _d(x)
    e = np.zeros_like(v)
    col = lambda t: None if t is None else _d(t).reshape(-1, 1)[[0] * v.shape[0] if image0 else slice(None)]
    lo, hi, sc = col(lo), col(hi), col(sc)
    for name, arg in (list(steps)[::-1] if reverse else steps):
        v, e = step64(name, arg, v, e, lo, hi, sc, clamp_after)
    return v, e


def chain32_host(steps, x, lo=None, hi=None, sc=None):
    """the same chain in fp32 with torch's CPU libm: what correct arithmetic with another libm gives (must stay inside chain64's bound)"""
    v = np.asarray(x, dtype=F)
    col = lambda t: None if t is None else np.asarray(t, dtype=F).reshape(-1, 1)
    lo, hi, sc = col(lo), col(hi), col(sc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F))
    with np.errstate(all="ignore"):
        for name, arg in steps:
            if name in ALGEBRAIC:
                v = map32(name, arg, v, lo, hi, sc)
            elif name == "log_p1":
                v = torch.log10(t(v + C01)).numpy() + F(1)
            elif name == "log10":
                v = torch.log10(t(v)).numpy()
            elif name == "norm_log":
                v = (torch.log10(t(v)).numpy() - lo) / (hi - lo)
            elif name == "exp_m1":
                v = torch.pow(10.0, t(np.minimum(v - F(1), F(arg)))).numpy() - C01
            elif name == "exp10":
                v = torch.pow(10.0, t(np.where(v > F(arg), F(arg), v))).numpy()
            else:
                raise KeyError(name)
    return v


CAP = 20.0  # clamp_before_exp of both configs
# every chain the project compiles: configs/drmnet ("log"), configs/obsnet ("resize_0p1tom1p1_normalizedLogarithmic_lowerbound1e-6"; the resize
# is no map), and estimate's two
CHAINS = {
    "log_fwd": [("log_p1", 0.0)],
    "log_inv": [("exp_m1", CAP)],
    "log_inv_nocap": [("exp_m1", math.inf)],
    "obs_fwd": [("lowerbound", 1e-6), ("norm_log", 0.0), ("unit_to_signed", 0.0)],
    "obs_inv": [("signed_to_unit", 0.0), ("denorm_log", 0.0), ("exp10", CAP)],
    "est_div_clip0": [("img_div", 0.0), ("clip0", 0.0)],
    "est_mul_log": [("img_mul", 0.0), ("log_p1", 0.0)],
}
CHAIN8 = [("img_mul", 0.0), ("lowerbound", 1e-6), ("log_p1", 0.0), ("unit_to_signed", 0.0), ("signed_to_unit", 0.0), ("exp_m1", CAP), ("img_div", 0.0),
          ("clip0", 0.0)]
CHAIN9 = CHAIN8 + [("log_p1", 0.0)]
RAGGED = [1, 3, 4, 5, 63, 1025]


def chain_inputs(name, b, per, seed=0):
    """(x [b, per], lo, hi, sc [b]) fp32: linear values from 1e-6 to 1e4 for the forward chains, the forward chain's own outputs (and a few
    values beyond the clamp) for the inverse ones; lo / hi / sc distinct per image"""
    g = _gen(b, per, seed, len(name))
    lin = np.exp(g.uniform(math.log(1e-6), math.log(1e4), (b, per))).astype(F)
    lin.reshape(-1)[:2] = (1e-6, 1e4)[:min(2, lin.size)]
    lo = (-3.0 - 0.5 * np.arange(b)).astype(F)
    hi = (2.0 + 0.25 * np.arange(b)).astype(F)
    sc = (0.3 * 1.7 ** np.arange(b)).astype(F)
    if name in ("log_inv", "log_inv_nocap"):
        x = (np.log10(_d(lin) + 0.1) + 1).astype(F)
        if name == "log_inv":
            x.reshape(-1)[-1] = 30.0  # beyond the clamp: 10^20
    elif name == "obs_inv":
        x = (2 * (np.log10(_d(lin)) - _d(lo)[:, None]) / _d(hi - lo)[:, None] - 1).astype(F)
        x.reshape(-1)[-1] = 9.0
    else:
        x = lin
    return x, lo, hi, sc


# ------------------------------------------------------------------------------------------------ ranges and scale

def range64(x, mask, broadcast=True, substitute=True, image0=False):
    """(lo, hi, bound_lo, bound_hi) [B] of x [B, C, H, W] fp32 under mask [B, 1, H, W] (0 / 1), as torch computes them (a NaN, or Inf * 0,
    poisons both); products with a 0 / 1 mask are exact, so only log10f is charged"""
    xt, m = torch.from_numpy(_d(x)), torch.from_numpy(_d(mask))
    if not broadcast:  # the mask reaches channel 0 only
        m = torch.cat([m, torch.ones_like(xt[:, 1:])], dim=1) if xt.shape[1] > 1 else m
    top = (xt * m).amax(dim=(1, 2, 3), keepdim=True)
    low = (xt * m + (1 - m) * top).amin(dim=(1, 2, 3)) if substitute else (xt * m).amin(dim=(1, 2, 3))
    with np.errstate(all="ignore"):
        lo, hi = np.log10(low.numpy()), np.log10(top.reshape(-1).numpy())
    if image0:
        lo, hi = np.full_like(lo, lo[0]), np.full_like(hi, hi[0])
    b = lambda r: np.where(np.isfinite(r), K("log10f") * ulp32(r), 0.0)
    return lo, hi, b(lo), b(hi)


def range_case(name):
    """(x [B, C, H, W], mask [B, 1, H, W]) of the named case: candidate extremes lie decades apart, so a wrong pick leaves the ulp bound"""
    g = _gen(len(name), 5)

    def img(c, h, w):
        return np.exp(g.uniform(math.log(0.5), math.log(2.0), (c, h, w))).astype(F)

    if name == "tiny_3x5":  # C * HW = 45, below the 512 threads
        x, m = img(3, 3, 5)[None], np.ones((1, 1, 3, 5), F)
        m[0, 0, 1, 2] = 0
        x[0, 1, 0, 3], x[0, 2, 2, 1], x[0, 0, 1, 2] = 1e3, 1e-3, 1e6
    elif name == "513":  # 512 k + 1 elements, the extremes in the first and the last one
        x, m = img(1, 1, 1025)[None], np.ones((1, 1, 1, 1025), F)
        x[0, 0, 0, 0], x[0, 0, 0, -1] = 1e-3, 1e3
    elif name == "channel2_only":
        x, m = img(3, 7, 9)[None], np.ones((1, 1, 7, 9), F)
        m[0, 0, :2] = 0
        x[0, 2, 4, 4], x[0, 2, 6, 8] = 1e4, 1e-4
        x[0, :, 0, 0] = (1e7, 1e-7, 1e7)  # the global extremes, masked out
    elif name == "masked_out_max":
        x, m = img(3, 6, 6)[None], np.ones((1, 1, 6, 6), F)
        m[0, 0, 3, 3] = 0
        x[0, 1, 3, 3] = 1e5
        x[0, 0, 3, 3] = 1e-5
    elif name == "empty_mask":
        x, m = img(3, 4, 4)[None], np.zeros((1, 1, 4, 4), F)
    elif name == "batch3":  # different answers per image; image 1 has the extremes in the first and last element
        x, m = np.stack([img(3, 5, 7) for _ in range(3)]), np.ones((3, 1, 5, 7), F)
        m[0, 0, 0, :3], m[2, 0, 4, :] = 0, 0
        x[0, 2, 2, 2], x[0, 1, 3, 3], x[0, 0, 0, 1] = 1e2, 1e-2, 1e9
        x[1, 0, 0, 0], x[1, 2, 4, 6] = 1e4, 1e-4
        x[2, 1, 1, 1], x[2, 0, 2, 5], x[2, 2, 4, 0] = 1e1, 1e-6, 1e-9
    else:
        raise KeyError(name)
    return x, m


RANGE_CASES = ["tiny_3x5", "513", "channel2_only", "masked_out_max", "empty_mask", "batch3"]


def lumscale64(x, scaler, count_unlit=False, clip=True, image0=False):
    """(scale [B], relative bound [B]) of x [B, 3, H, W] fp32: L in the kernel's fp32 order, then float64.  logf of every lit pixel is charged
    K ulps of its own value, the double sum is exact at these sizes, the mean is rounded once, expf and the division once each."""
    x = np.asarray(x, dtype=F)
    L = _d(lum32(x[:, 0], x[:, 1], x[:, 2])).reshape(x.shape[0], -1)
    with np.errstate(all="ignore"):
        lg = np.log(np.maximum(L, float(C1E5))) if clip else np.log(L)
        lit = np.ones_like(L, dtype=bool) if count_unlit else L > 0
        lg = np.where(np.isnan(L), np.nan, np.where(lit, lg, 0.0))  # NaN * 0 stays NaN
        cnt = lit.sum(1)
        m = lg.sum(1) / cnt
        s = float(F(scaler)) / np.exp(m)
        em = K("logf") * np.where(lit, ulp32(lg), 0.0).sum(1) / np.maximum(cnt, 1) + U * np.abs(m)
        rel = np.expm1(em) + K("expf") * 2 * U + U
    if image0:
        s, rel = np.full_like(s, s[0]), np.full_like(rel, rel[0])
    return s, rel


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F))


def lumscale32_host(x, scaler, keep_poison=True):
    """the kernel's arithmetic with torch's CPU libm: fp32 L and logf, a double sum, the mean rounded to fp32, expf, the division.
    keep_poison=False is the rule before the poison fix: a NaN luminance fails `L > 0` and is skipped."""
    x = np.asarray(x, dtype=F)
    L = lum32(x[:, 0], x[:, 1], x[:, 2]).reshape(x.shape[0], -1)
    with np.errstate(all="ignore"):
        lg = _d(torch.log(_t32(np.maximum(L, C1E5))).numpy())
        lit = L > 0
        s = np.where(lit, lg, 0.0).sum(1)
        if keep_poison:
            s = s + np.where(np.isnan(L), np.nan, 0.0).sum(1)
        m = (s / lit.sum(1)).astype(F)
        return F(scaler) / torch.exp(_t32(m)).numpy()


def tonemap32_host(x, mask=None, alpha=0.18, gamma=2.2, keep_poison=True):
    """hdr2ldr_kernel's arithmetic with torch's CPU libm.  keep_poison=False is the rule before the poison fix: an unlit NaN or +Inf luminance
    is skipped in the mean and the clip is fminf(fmaxf(t, 0), 1), which turns a NaN product into 0."""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    L = lum32(x[:, 0], x[:, 1], x[:, 2])
    lit = L > C5E5
    if mask is not None:
        lit = lit & (np.asarray(mask).reshape(-1) != 0)
    with np.errstate(all="ignore"):
        lg = _d(torch.log(_t32(np.maximum(L, F(0)) + C1E7)).numpy())
        s = np.where(lit, lg, 0.0).sum()
        if keep_poison and (~lit & (np.isnan(L) | (L == np.inf))).any():
            s = np.nan
        m = F(s / lit.sum())
        coeff = F(alpha) / torch.exp(_t32(np.array([m]))).numpy()[0]
        t = x * coeff
        if keep_poison:
            t = np.where(t <= 0, F(0), np.where(t > 1, F(1), t))
        else:
            t = np.fmin(np.fmax(t, F(0)), F(1))
        return torch.pow(_t32(t), float(F(1.0) / F(gamma))).numpy()


def lum_case(name):
    g = _gen(len(name), 9)

    def img(hw, n=1):
        return np.exp(g.standard_normal((n, 3, 1, hw)) * 1.5).astype(F)

    if name in ("hw1", "hw511", "hw513"):
        return img(int(name[2:]))
    if name == "unlit_and_dim":  # pixels with L <= 0, pixels with 0 < L < 1e-5
        x = img(300)
        x[0, :, 0, 10:60] = 0.0
        x[0, :, 0, 60:90] = -1.0
        x[0, :, 0, 90:140] *= 1e-7
        return x
    if name == "nothing_lit":
        return -img(40)
    if name == "batch3":
        x = img(129, 3)
        x[1] *= 30.0
        x[2, :, 0, :50] = 0.0
        return x
    raise KeyError(name)


LUM_CASES = ["hw1", "hw511", "hw513", "unlit_and_dim", "nothing_lit", "batch3"]


# ------------------------------------------------------------------------------------------------ tone map

def tonemap64(x, mask=None, alpha=0.18, gamma=2.2, threshold=True, use_mask=True, invert_gamma=True):
    """(out [HW, 3] float64, bound) of x [HW, 3] fp32: L and the lit test in the kernel's fp32 order; logf, expf and powf charged K ulps each"""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    L32 = lum32(x[:, 0], x[:, 1], x[:, 2])
    lit = (L32 > C5E5) if threshold else np.ones(L32.shape, dtype=bool)
    if mask is not None and use_mask:
        lit = lit & (np.asarray(mask).reshape(-1) != 0)
    with np.errstate(all="ignore"):
        arg = _d(np.maximum(L32, F(0)) + C1E7)  # the fp32 sum is the logf's argument
        lg = np.log(arg)
        poison = np.isnan(L32) | (~lit & (L32 == np.inf))
        cnt = lit.sum()
        m = (np.nan if poison.any() else 0.0) + np.where(lit, lg, 0.0).sum() / cnt
        em = K("logf") * np.where(lit, ulp32(lg), 0.0).sum() / max(cnt, 1) + U * abs(m)
        if not np.isfinite(m):
            em = 0.0  # a lit +Inf: the coefficient is alpha / Inf = 0 exactly, every output is exactly 0 or NaN (m NaN: all NaN)
        coeff = float(F(alpha)) / np.exp(m)
        rc = np.expm1(em) + K("expf") * 2 * U + U
        p = float(F(1.0) / F(gamma)) if invert_gamma else float(F(gamma))
        t = _d(x) * coeff
        tc = np.where(t <= 0, 0.0, np.where(t > 1, 1.0, t))  # NaN stays
        out = np.power(tc, p)
        bound = out * (np.expm1(p * np.log1p(rc + U)) + K("powf") * 2 * U) + 1e-45
    return out, bound


def tone_case(name):
    """(x [H, W, 3] fp32, mask [H, W] uint8 or None, alpha, gamma)"""
    g = _gen(len(name), 13)

    def img(hw):
        return (np.exp(g.standard_normal((1, hw, 3)) * 1.5) * 0.3).astype(F)

    if name in ("hw1", "hw1023", "hw1025"):
        return img(int(name[2:])), None, 0.18, 2.2
    if name == "threshold":  # L exactly 5e-5f, one fp32 step below, one above (threshold_pixels), among ordinary pixels
        x = img(37)
        x[0, :3] = threshold_pixels()
        return x, None, 0.18, 2.2
    if name == "mask_brightest":
        x = img(200)
        x[0, 5:25] *= 1e4
        m = np.ones((1, 200), np.uint8)
        m[0, 5:25] = 0
        return x, m, 0.18, 2.2
    if name == "alpha_gamma":
        return img(77), None, 0.3, 1.8
    if name == "nothing_lit":
        return img(30) * F(1e-6), None, 0.18, 2.2
    raise KeyError(name)


TONE_CASES = ["hw1", "hw1023", "hw1025", "threshold", "mask_brightest", "alpha_gamma", "nothing_lit"]


def threshold_pixels():
    """three grey pixels [3, 3] whose fp32 luminance is exactly 5e-5f, the fp32 number below it and the one above"""
    want = [C5E5, np.nextafter(C5E5, F(0)), np.nextafter(C5E5, F(1))]
    c = F(5e-5)
    cand = [c]
    for _ in range(64):
        cand = [np.nextafter(cand[0], F(0))] + cand + [np.nextafter(cand[-1], F(1))]
    cand = np.array(cand, dtype=F)
    res = []
    for wv in want:
        hit = [(r, gg, b) for r in cand[48:81] for gg in cand[48:81] for b in (cand[64],) if lum32(r, gg, b) == wv]
        assert hit, f"no pixel with luminance {wv!r}"
        res.append(hit[0])
    return np.array(res, dtype=F)


# ------------------------------------------------------------------------------------------------ (a) resize

RESIZE_MODES = ["nearest", "bilinear", "bicubic"]
RESIZE_SHAPES = [((12, 10), (5, 7)), ((5, 7), (12, 10)), ((8, 8), (8, 8)), ((9, 4), (4, 9))]
RESIZE_MAX_TAPS = 96


def _filter32(mode, x):
    x = F(abs(x))
    if mode == "bilinear":
        return F(1) - x if x < F(1) else F(0)
    a = F(-0.5)
    if x < F(1):
        return ((a + F(2)) * x - (a + F(3))) * x * x + F(1)
    if x < F(2):
        return (((x - F(5)) * x + F(8)) * x - F(4)) * a
    return F(0)


def aa_taps32(mode, i, in_len, out_len, mutant=None):
    """(first, weights fp32 [count]) of output index i along an axis: aa_taps of csrc/transform.hip"""
    scale = F(in_len) / F(out_len)
    half = F(1.0 if mode == "bilinear" else 2.0)
    shrink = scale >= F(1) and mutant != "support_not_scaled"
    support = half * scale if shrink else half
    inv = F(1) / scale if shrink else F(1)
    centre = scale * (F(i) + (F(0) if mutant == "no_half_pixel" else F(0.5)))
    first = max(int(centre - support + F(0.5)), 0)
    count = min(int(centre + support + F(0.5)), in_len) - first
    count = min(count, RESIZE_MAX_TAPS)
    if mutant == "last_tap_lost":
        count -= 1
    w = np.zeros(max(count, 0), dtype=F)
    total = F(0)
    for j in range(count):
        w[j] = _filter32(mode, (F(j + first) - centre + F(0.5)) * inv)
        total = total + w[j]
    if total != 0 and mutant != "not_normalised":
        for j in range(count):
            w[j] = w[j] / total
    return first, w


def resize32(x, size, mode, mutant=None):
    """resize_kernel on x [planes, IH, IW] fp32 -> [planes, OH, OW]: per output pixel and per row the horizontal sum in tap order, then the
    vertical sum in tap order (mutant "h_before_w": the other way round), all in fp32"""
    x = np.asarray(x, dtype=F)
    p, ih, iw = x.shape
    oh, ow = size
    out = np.zeros((p, oh, ow), dtype=F)
    if mode == "nearest":
        sh, sw = F(ih) / F(oh), F(iw) / F(ow)
        rule = (lambda v: int(np.floor(v + F(0.5)))) if mutant == "nearest_round" else (lambda v: int(np.floor(v)))
        for oy in range(oh):
            for ox in range(ow):
                out[:, oy, ox] = x[:, min(rule(F(oy) * sh), ih - 1), min(rule(F(ox) * sw), iw - 1)]
        return out
    tx = [aa_taps32(mode, ox, iw, ow, mutant) for ox in range(ow)]
    ty = [aa_taps32(mode, oy, ih, oh, mutant) for oy in range(oh)]
    with np.errstate(all="ignore"):
        for oy in range(oh):
            y0, wy = ty[oy]
            for ox in range(ow):
                x0, wx = tx[ox]
                if len(wx) == 0 or len(wy) == 0:
                    continue
                if mutant == "h_before_w":
                    acc = None
                    for k in range(len(wx)):
                        v = x[:, y0, x0 + k] * wy[0]
                        for j in range(1, len(wy)):
                            v = v + x[:, y0 + j, x0 + k] * wy[j]
                        acc = v * wx[0] if k == 0 else acc + v * wx[k]
                else:
                    acc = None
                    for j in range(len(wy)):
                        h = x[:, y0 + j, x0] * wx[0]
                        for k in range(1, len(wx)):
                            h = h + x[:, y0 + j, x0 + k] * wx[k]
                        acc = h * wy[0] if j == 0 else acc + h * wy[j]
                out[:, oy, ox] = acc
    return out


def resize_bound(x, size, mode):
    """what another correct fp32 evaluation (ATen's own passes, in an order of theirs) may differ by.  A weight: the filter polynomial's
    intermediates reach 4 in magnitude and it takes five operations, so 16 u absolute (near a zero of the cubic nothing relative holds), and
    count + 2 relative roundings of the normalisation; a tap: a product and an add per pass -> with E = 16 u on the support,
    sum (|wy| + E) (|wx| + E) |x| - sum |wy| |wx| |x| + (2 (nx + ny) + 16) u sum |wy| |wx| |x|"""
    x = _d(x)
    p, ih, iw = x.shape
    oh, ow = size
    wy, wx, ey, ex = np.zeros((oh, ih)), np.zeros((ow, iw)), np.zeros((oh, ih)), np.zeros((ow, iw))
    for i in range(oh):
        f, w = aa_taps32(mode, i, ih, oh)
        wy[i, f:f + len(w)], ey[i, f:f + len(w)] = np.abs(w), 16 * U
    for i in range(ow):
        f, w = aa_taps32(mode, i, iw, ow)
        wx[i, f:f + len(w)], ex[i, f:f + len(w)] = np.abs(w), 16 * U
    n = (ey != 0).sum(1).max() + (ex != 0).sum(1).max()
    s = lambda a, b: np.einsum("ai,pij,bj->pab", a, np.abs(x), b)
    return s(wy + ey, wx + ex) - s(wy, wx) + (2 * n + 16) * U * s(wy, wx)


def one_hots(ih, iw):
    return np.eye(ih * iw, dtype=F).reshape(ih * iw, ih, iw)


def dense_image(planes, ih, iw, seed=0):
    return _gen(planes, ih, iw, seed).standard_normal((planes, ih, iw)).astype(F)


def max_downscale(mode):
    """(largest admitted input length, first refused one) onto 2 outputs under the host guard 2 half smax + 2 <= 96"""
    half = 2.0 if mode == "bicubic" else 1.0
    n = 2
    while 2.0 * half * max((n + 1) / 2.0, 1.0) + 2.0 <= RESIZE_MAX_TAPS:
        n += 1
    return n, n + 1


RESIZE_MUTANTS = {"no_half_pixel": "onehot", "support_not_scaled": "onehot", "not_normalised": "onehot", "last_tap_lost": "onehot", "h_before_w": "dense",
                  "nearest_round": "onehot"}


# ------------------------------------------------------------------------------------------------ (a), (c) mirror-ball warp

def taps32(u, v, h, w, mutant=None):
    """grid_sample_taps (csrc/grid_sample.h) at fp32 positions u, v (arrays) -> (x0, y0, has_x1, has_y1, w00, w01, w10, w11)"""
    u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
    if mutant == "align_corners":
        ix, iy = (u + F(1)) / F(2) * F(w - 1), (v + F(1)) / F(2) * F(h - 1)
    else:
        ix, iy = ((u + F(1)) * F(w) - F(1)) / F(2), ((v + F(1)) * F(h) - F(1)) / F(2)
    ix = np.minimum(F(w - 1), np.maximum(ix, F(0)))
    iy = np.minimum(F(h - 1), np.maximum(iy, F(0)))
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    wx1, wy1 = ix - fx, iy - fy
    wx0, wy0 = F(1) - wx1, F(1) - wy1
    return x0, y0, x0 + 1 < w, y0 + 1 < h, wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1


def tap_weights32(u, v, h, w, mutant=None):
    """dense [..., h, w] fp32 weights of the (at most four) taps of every position: what a one-hot mirror set reads out"""
    x0, y0, hx, hy, w00, w01, w10, w11 = taps32(u, v, h, w, mutant)
    if mutant == "taps_swapped":
        w01, w10 = w10, w01
    out = np.zeros(u.shape + (h, w), dtype=F)
    idx = np.indices(u.shape)
    out[(*idx, y0, x0)] = w00
    m = hx
    out[(*[i[m] for i in idx], y0[m], x0[m] + 1)] = w01[m]
    m = hy
    out[(*[i[m] for i in idx], y0[m] + 1, x0[m])] = w10[m]
    m = hx & hy
    out[(*[i[m] for i in idx], y0[m] + 1, x0[m] + 1)] = w11[m]
    return out


def warp_positions(oh, ow, h, w, reverse_azimuth=True, align_corners=False, clamp=True):
    """float64 sample position of every envmap texel, in mirror pixels, with its bound -> dict(u, v, ix, iy, raw_x, raw_y, ex, ey, len)
    ix / iy are clamped to the border, raw_x / raw_y are not; ex / ey bound |fp32 position - float64 position| in pixels (section (c))."""
    pi = float(PI32)
    i, j = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    theta = (i + 0.5) * float(PI32 / F(oh))
    phi = (j + 0.5) * float(PI32 * F(2) / F(ow)) * (-1.0 if reverse_azimuth else 1.0)
    dth, dph = U * np.abs(theta), U * np.abs(phi)  # one rounding each: the step is the reference's own fp32 constant
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    e_st = np.abs(ct) * dth + K("sinf") * ulp32(st)
    e_sp = np.abs(cp) * dph + K("sinf") * ulp32(sp)
    e_cp = np.abs(sp) * dph + K("cosf") * ulp32(cp)
    nx, ny, nz = -st * sp, ct, -st * cp + 1.0
    e_nx = np.abs(sp) * e_st + np.abs(st) * e_sp + U * np.abs(nx)
    e_ny = np.abs(st) * dth + K("cosf") * ulp32(ny)
    e_nz = np.abs(cp) * e_st + np.abs(st) * e_cp + U * np.abs(st * cp) + U * np.abs(nz)
    ln = np.sqrt(nx * nx + ny * ny + nz * nz)
    # len: the components' errors, three squares and two adds inside the root (each at most u len^2, halved by the root), the root itself
    e_ln = (np.abs(nx) * e_nx + np.abs(ny) * e_ny + np.abs(nz) * e_nz) / np.maximum(ln, 1e-300) + 3.5 * U * ln
    lo_ln = ln - e_ln
    with np.errstate(all="ignore"):
        ok = lo_ln > 0
        inv = np.where(ok, 1.0 / np.where(ok, lo_ln, 1.0), np.inf)
        ux, uy, uz = nx / ln, ny / ln, nz / ln
        comp = lambda c, e: e * inv + np.abs(c) * e_ln * inv + U * np.abs(c)
        e_ux, e_uy, e_uz = comp(ux, e_nx), comp(uy, e_ny), comp(uz, e_nz)
        r = np.sqrt(ux * ux + uz * uz)
        lo_r = r - (e_ux + e_uz)
        okr = ok & (lo_r > 0)
        invr = np.where(okr, 1.0 / np.where(okr, lo_r, 1.0), np.inf)
        at, ac = np.arctan2(ux, uz), np.arccos(np.clip(uy, -1, 1))
        e_at = (e_ux + e_uz) * invr + K("atan2f") * ulp32(at)
        e_ac = e_uy * invr + K("acosf") * ulp32(ac)
        c2 = float(TWO_OVER_PI)
        u = at * c2
        e_u = e_at * c2 + U * np.abs(u)
        v0 = ac * c2
        v = v0 - 1.0
        e_v = e_ac * c2 + U * np.abs(v0) + U * np.abs(v)

        def unnorm(t, e, n):
            if align_corners:
                return (t + 1) / 2 * (n - 1), e * n
            a = (t + 1) * n
            return (a - 1) / 2, ((e + U * np.abs(t + 1)) * n + U * np.abs(a) + U * np.abs(a - 1)) / 2

        raw_x, ex = unnorm(u, e_u, w)
        raw_y, ey = unnorm(v, e_v, h)
    ix, iy = (np.clip(raw_x, 0, w - 1), np.clip(raw_y, 0, h - 1)) if clamp else (raw_x, raw_y)
    return dict(u=u, v=v, ix=ix, iy=iy, raw_x=raw_x, raw_y=raw_y, ex=ex, ey=ey, len=ln)


def ramp_maps(h, w):
    """[1, 3, h, w] fp32: the maps 1, x, y in pixel units.  Bilinear sampling of an affine map returns the clamped sample position itself."""
    y, x = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    return np.stack([np.ones((h, w), F), x, y])[None]


def ramp_eval_bound(h, w):
    """evaluating sum w_k c_k on integer coordinates c_k <= n - 1: the weights' two roundings, the product and three adds on partial sums of at
    most n - 1 -> 8 u (n - 1) at most for either coordinate channel (2 ulps of 1 for the constant one)"""
    return 8 * U * max(w - 1, 1), 8 * U * max(h - 1, 1)


def power2_basis(c, h, w):
    """[c, h, w] fp32, not constant, every entry a power of two: ramp * basis and its division are exact"""
    ch, y, x = np.meshgrid(np.arange(c), np.arange(h), np.arange(w), indexing="ij")
    return (2.0 ** ((x + 2 * y + ch) % 5 - 2)).astype(F)


def determinate(pos, h, w):
    """texels whose taps are decided by the float64 position alone: the unclamped position lies further than its bound from every texel
    boundary it could cross (an integer inside [0, n - 1]); a position clamped beyond its bound sits on the border texel with weight one"""
    def axis(raw, e, n):
        inside = (raw > 0) & (raw < n - 1)
        near = np.abs(raw - np.round(raw)) <= e
        return np.where(inside, ~near, (raw < -e) | (raw > n - 1 + e)) & np.isfinite(e)

    return axis(pos["raw_x"], pos["ex"], w) & axis(pos["raw_y"], pos["ey"], h)


POISON_CASES = ["range_nan_in_mask", "range_inf_outside_mask", "lum_nan", "tone_nan", "tone_inf_outside_mask"]


def poison_case(name):
    """inputs of the poison cases: clean images with one bad value"""
    if name.startswith("range"):
        x, m = range_case("batch3")
        x, m = x.copy(), m.copy()
        if name == "range_nan_in_mask":
            x[1, 1, 2, 2] = np.nan
        else:
            x[1, 0, 3, 3], m[1, 0, 3, 3] = np.inf, 0
        return x, m
    if name == "lum_nan":
        x = lum_case("batch3").copy()
        x[1, 2, 0, 77] = np.nan
        return (x,)
    x, m, a, g = tone_case("mask_brightest")
    x = x.copy()
    if name == "tone_nan":
        x[0, 100, 1] = np.nan
    else:
        x[0, 10, 1] = np.inf  # one of the masked-out pixels: log(Inf) * 0 is NaN in the reference
        assert m[0, 10] == 0
    return x, m, a, g


MIRRORS = [(8, 8), (5, 9)]
ENVMAPS = [(4, 8), (10, 28), (7, 5)]
WARP_MUTANTS = ["align_corners", "no_border_clamp", "azimuth_not_reversed", "taps_swapped", "basis_skipped"]

# mutant -> the named case (shared by the CPU and the GPU tests) that fails for it
MUTANT_CASES = {
    "chain_reversed": "chain:obs_fwd", "clamp_after_exp": "chain:log_inv", "image0_vectors": "ragged_per_image",
    "mask_not_broadcast": "range:channel2_only", "min_without_substitute": "range:masked_out_max", "range_image0": "range:batch3",
    "unlit_counted": "lum:unlit_and_dim", "clip_missing": "lum:unlit_and_dim", "scale_image0": "lum:batch3",
    "threshold_missing": "tone:threshold", "mask_ignored": "tone:mask_brightest", "gamma_not_inverted": "tone:alpha_gamma",
    "no_half_pixel": "resize:onehot", "support_not_scaled": "resize:onehot", "not_normalised": "resize:onehot", "last_tap_lost": "resize:onehot",
    "h_before_w": "resize:dense", "nearest_round": "resize:onehot",
    "align_corners": "warp:ramp", "no_border_clamp": "warp:ramp", "azimuth_not_reversed": "warp:ramp", "taps_swapped": "warp:onehot",
    "basis_skipped": "warp:basis",
}

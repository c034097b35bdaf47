"""CPU helpers of the sharp checks of three kernels every forward runs but no per-module test reached (tests/test_boundary_ref_cpu.py,
tests/test_gpu_boundary.py; DESIGN.md "Boundary-kernel checks"): the stem (csrc/stemhead.hip stem_conv_kernel), the 2x2 average pool with its
fused statistics (csrc/misc.hip avgpool2_kernel) and RefNet's pooled head (csrc/misc.hip encoder_head_kernel).  No GPU code; every reference is
plain fp64 torch.

(a) Exact family (stem, pooling outputs).  x, cond in {k/8 : |k| <= 16}, w in {k/32 : |k| <= 16}, bias in {k/8 : |k| <= 16}: all fp16 numbers, so
    the split form's lo halves are zero; the weight pre-scale and the per-tile guard are powers of two; all 9 Cin products and every partial sum
    of them, in any order, are multiples of 2^-8 below 2^6 (quant_ref.exact_bits: 14 bits).  The fp64 reference cast to fp32 is what a correct
    kernel returns, bit for bit.  Pooling: a sum of four such values times 0.25 is exact as well.

(b) Narrow family (tables).  x in {k/2 : |k| <= 2}, w in {k/4 : |k| <= 2}, bias in {k/8 : |k| <= 8}: a subset of (a).  An output is a multiple
    of 1/8 with |v| <= 54 * 1 * 1/2 + 1 = 28, its square a multiple of 1/64 below 784; about any pivot p of the same set |v - p| <= 56 and the
    square stays below 3136.  A thread that adds `per` of them holds at most per * 3136 * 64 units of 1/64: 2^23.6 for per = 64 (the pooling
    kernel's longest walk; the stem's lane adds 32), inside fp32's 24 bits, so the fp64 table is exactly the fp64 sums whatever the order and
    with or without a pivot (narrow_bits asserts this; with w up to |k| = 2 and x up to |k| = 4 the pivot form would need 2^25.6 and the
    premise would be false).  Pooling the narrow x gives multiples of 1/8 up to 1: far inside.

(c) Offset family (tables).  gn_ref.offset_means: per-channel offsets of 2^3 and 2^6 on unit noise -- through the bias for the stem, in the input
    for the pool.  Criterion: GroupNorm32 of the tensor the kernel returned, computed from the table the kernel returned (gn_ref._from_tables,
    fp64), against gn_ref.group_norm64 of the same tensor, elementwise within gn_ref.bound(..., "fp32", ...): a table may cost no more than the
    seven fp32 roundings the table form is allowed anyway.  lane_tables / pivot_lane_tables emulate a thread's fp32 arithmetic on the CPU.
    offset_means alternates the sign inside a group, so at the stem's four channels per group a group's mean is about zero and its variance
    about the offset's square: statistics that forgive an error of the size of the noise.  The same-sign variant (|offset_means|: a group
    whose channels share their offset, what one channel per group is in gn_ref's probes) has group variance 1 on a mean of 2^6 and is the
    case that raw fp32 moments fail; both run, against the same bound.

(d) Encoder head: out[n][o] = b[o] + sum_c w[o][c] P[n][c], P = mean_hw(silu(t)), t = x * scale + shift.  head_bound charges, with u = 2^-24:
      t        a product and an add (the library is built without contraction): u (|x scale| + |t|), passed through SiLU's slope <= 1.1
      silu     gn_ref.silu_eval_bound(a) = u (4 |a| + 2) for v / (1 + __expf(-v))
      pooling  four fp32 chains of ceil(HW / 4) adds, then three adds: every add rounds a partial sum that is at most sum |a|, so
               (ceil(HW / 4) + 3) u sum_p |a| / HW; the division: u |P|
      dot      a lane multiplies and adds ceil(C / 64) terms (two roundings each, the partial sum at most the lane's sum |w P|), then a six-level
               shuffle tree: (2 ceil(C / 64) + 6) u sum_c |w P|; the bias add: u |out|
    and the pooled errors enter the output through |w|.  Nothing in it is fitted to a result.

(e) Mutants: each reference wrong in one way the kernel could be wrong.
"""
import math

import torch
import torch.nn.functional as F

import gn_ref as G
from quant_ref import dyadic, exact_bits

U = 2.0 ** -24
STEM_TH, STEM_TW, STEM_COUT = 8, 16, 128  # csrc/stemhead.hip: the tile and the only Cout
STEM_CH = [(3, 3), (1, 3), (3, 1)]  # (Cx, Cc): CIN = 6, and CIN = 4 with the x | cond boundary inside a lane half either way

EXACT = dict(x_step=1 / 8, x_k=16, w_step=1 / 32, w_k=16, b_step=1 / 8, b_k=16)
NARROW = dict(x_step=1 / 2, x_k=2, w_step=1 / 4, w_k=2, b_step=1 / 8, b_k=8)

# name -> (N, H, W): the fixed shapes of the stem's equality tests
STEM_SHAPES = {"one_tile": (1, 8, 16), "small_map": (2, 4, 4), "ragged": (3, 12, 20), "one_live_row_col": (1, 9, 17)}
PERSISTENT_HW = (24, 48)  # nine tiles per image
ROWS_B, ROWS = 7, [4, 0, 4, 6, 1]  # five rows gathered from seven: a repeat and a permutation
OFFSET_SHAPE = (2, 16, 32)
POOL_SHAPES = [(1, 128, 8, 8), (2, 192, 12, 20), (3, 256, 4, 4), (1, 1024, 8, 16), (9, 64, 32, 32)]
# beyond the listed shapes: a thread adds more than one pixel only where the sparse-launch rule leaves long pixel blocks -- eight pixels per
# thread at (1, 32, 128, 128), the full 64 at the smallest launch with 256 workgroups of 256 pixels x 64 channel quads
POOL_LONG = [(1, 32, 128, 128), (4, 256, 256, 256)]
HEAD_SHAPES = [(1, 128, 1, 6), (3, 256, 6, 6), (2, 1024, 16, 6), (2, 132, 7, 5)]  # (N, C, HW, O)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(v) for i, v in enumerate(key)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------ (a), (b) families and their premises

def stem_inputs(fam, n, cx, cc, h, w, seed=0):
    """(x [n, cx, h, w], cond [n, cc, h, w], weight [128, cx + cc, 3, 3], bias [128]) fp32 of a dyadic family"""
    g = _gen(n, cx, cc, h, w, seed, fam["x_k"])
    x = dyadic((n, cx, h, w), fam["x_step"], fam["x_k"], g)
    cond = dyadic((n, cc, h, w), fam["x_step"], fam["x_k"], g)
    wt = dyadic((STEM_COUT, cx + cc, 3, 3), fam["w_step"], fam["w_k"], g)
    b = dyadic((STEM_COUT,), fam["b_step"], fam["b_k"], g)
    return x, cond, wt, b


def guard_case(cx, cc):
    """(x, cond, w, reference): one row of four tiles scaled by 2^-40, 0, 0, 2^40 -- a zero tile between the scales, since an output may not mix
    them (its 3 x 3 window would need more than 24 bits) and a tile's guard follows the largest value of its halo; no bias for the same reason"""
    x, cond, wt, _ = stem_inputs(EXACT, 1, cx, cc, 8, 64, seed=3)
    s = torch.zeros(64)
    s[:16], s[48:] = 2.0 ** -40, 2.0 ** 40
    x, cond = x * s, cond * s
    return x, cond, wt, stem_ref64(x, cond, wt, None)


def family_bits(fam, cin):
    """bits of the widest intermediate of a stem output of the family (asserted <= 24 by exact_bits), and that its operands are fp16 numbers"""
    xm, wm, bm = fam["x_step"] * fam["x_k"], fam["w_step"] * fam["w_k"], fam["b_step"] * fam["b_k"]
    for step, k in ((fam["x_step"], fam["x_k"]), (fam["w_step"], fam["w_k"])):
        assert math.frexp(step)[0] == 0.5 and k < 2 ** 11 and step * k <= 65504.0 and step >= 2.0 ** -14, "operand is no fp16 number"
    return exact_bits(9 * cin, fam["x_step"], xm, fam["w_step"], wm, adds=[(fam["b_step"], bm)])


def narrow_bits(per, cin=6, pooled=False):
    """bits a thread's fp32 sum of `per` squares of narrow-family values needs, about the worst pivot of the family: asserted <= 24.  pooled:
    the values are 2x2 means of the narrow x instead of stem outputs."""
    f = NARROW
    xm = f["x_step"] * f["x_k"]
    if pooled:
        unit, vmax = f["x_step"] / 4, xm
    else:
        unit = min(f["x_step"] * f["w_step"], f["b_step"])
        vmax = 9 * cin * xm * f["w_step"] * f["w_k"] + f["b_step"] * f["b_k"]
    dmax = 2 * vmax  # |v - p| for a pivot p of the same set; p = 0 is the plain sum, which needs less
    assert math.log2(vmax / unit + 1) <= 24 and math.log2(per * dmax / unit + 1) <= 24
    bits = math.log2(per * dmax * dmax / (unit * unit) + 1)
    assert bits <= 24, f"{per} squares about a pivot need {bits:.1f} bits"
    return bits


def pool_inputs(fam, n, c, h, w, seed=0):
    return dyadic((n, c, h, w), fam["x_step"], fam["x_k"], _gen(n, c, h, w, seed, fam["x_k"], 77))


# ------------------------------------------------------------------------------------------------ references

def stem_ref64(x, cond, wt, b, rows=None):
    xin = torch.cat([x, cond], 1).double()
    if rows is not None:
        xin = xin[torch.as_tensor(rows, dtype=torch.long)]
    return F.conv2d(xin, wt.double(), None if b is None else b.double(), padding=1)


def tables64(out):
    """[n, c, 2] fp64 (sum, sum of squares) over the pixels of out [n, c, h, w]"""
    o = out.double()
    return torch.stack([o.sum((2, 3)), (o * o).sum((2, 3))], dim=2)


def pool_ref64(x):
    return F.avg_pool2d(x.double(), 2)


def pool_out_bound(x):
    """three fp32 roundings of (a + b + c + d) / 4, each on a partial sum of at most |a| + |b| + |c| + |d| (the factor 0.25 is exact)"""
    return 3.0 * U * F.avg_pool2d(x.double().abs(), 2)


def stem_tiles(h, w):
    return ((h + STEM_TH - 1) // STEM_TH) * ((w + STEM_TW - 1) // STEM_TW)


def stem_ranges(n, h, w, cus):
    """[(t0, t1)] of every workgroup of the stem's persistent launch: grid = min(tiles, 2 CUs), t0 = total b / grid (launch_stem_conv)"""
    total = n * stem_tiles(h, w)
    grid = min(total, 2 * cus)
    return [(total * b // grid, total * (b + 1) // grid) for b in range(grid)]


def persistent_n(cus, h=PERSISTENT_HW[0], w=PERSISTENT_HW[1]):
    """the smallest batch at which the ranges hold about one and a half tiles each: some workgroups own two tiles of one image, some cross an
    image boundary (range_kinds says which; the tests assert both)"""
    return -(-3 * cus // stem_tiles(h, w))


def range_kinds(ranges, tiles_img):
    """(workgroups with two tiles of one image, workgroups whose range crosses an image boundary)"""
    same = sum(1 for a, b in ranges if any(t // tiles_img == (t + 1) // tiles_img for t in range(a, b - 1)))
    cross = sum(1 for a, b in ranges if b > a and a // tiles_img != (b - 1) // tiles_img)
    return same, cross


def avgpool2_launch(n, c, h, w):
    """(QL, px_per_block, passes, pixels per thread at most) of launch_avgpool2's rule (csrc/misc.hip)"""
    q4, hwo = c // 4, (h // 2) * (w // 2)
    ql = 64 if q4 >= 64 else 32 if q4 >= 32 else 16 if q4 >= 16 else 8 if q4 >= 8 else 4
    ppb = 256
    blocks = lambda: n * (-(-hwo // ppb)) * (-(-q4 // ql))
    while blocks() < 256 and ql > 8:
        ql >>= 1
    while blocks() < 256 and -(-hwo // ppb) < 16 and ppb > 256 // ql:
        ppb >>= 1
    return ql, ppb, -(-q4 // ql), -(-min(ppb, hwo) // (256 // ql))


# ------------------------------------------------------------------------------------------------ (c) the table criterion and its emulations

def table_criterion(out, stat, seed=0):
    """(error, bound) [n, c, h, w]: GroupNorm32 of `out` from the table `stat` [n, c, 2] = (sum, sum of squares) against group_norm64(out)"""
    n, c, h, w = out.shape
    gamma, beta = G.affine(c, seed)
    gn = G.group_norm64(out, gamma, beta)
    t = stat.double() / float(h * w)
    y = G._from_tables(out, t[:, :, 0], t[:, :, 1], gamma, beta)
    return (y - gn.y).abs(), G.bound(out, gn.sc, gn.sh, gn.y, "fp32", beta)


def _lanes(x, per):
    """[n, c, lanes, per] fp32 values and their live mask: a thread's `per` values, the tail of the map padded"""
    n, c, h, w = x.shape
    hw = h * w
    v = x.float().reshape(n, c, hw)
    live = torch.ones(hw, dtype=torch.bool)
    pad = (-hw) % per
    if pad:
        v = torch.cat([v, torch.zeros((n, c, pad))], dim=2)
        live = torch.cat([live, torch.zeros(pad, dtype=torch.bool)])
    return v.reshape(n, c, -1, per), live.reshape(-1, per)


def lane_tables(x, per):
    """the raw-moment arithmetic: a thread adds `per` values and their squares in fp32, the thread totals meet in double -> [n, c, 2] sums"""
    v, _ = _lanes(x, per)  # (gn_ref.fp32_lane_tables, as sums: the padding adds zeros)
    s = torch.zeros(v.shape[:3])
    q = torch.zeros(v.shape[:3])
    for e in range(per):
        s = s + v[..., e]
        q = q + v[..., e] * v[..., e]
    return torch.stack([s.double().sum(2), q.double().sum(2)], dim=2)


def pivot_lane_tables(x, per):
    """the same sums about the thread's first live value p, restored in double (csrc/conv_epilogue.h stat_unpivot) -> [n, c, 2] sums"""
    v, live = _lanes(x, per)
    p = v[..., 0]  # (a lane's first slot is live whenever the lane holds anything)
    s = torch.zeros(v.shape[:3])
    q = torch.zeros(v.shape[:3])
    for e in range(per):
        d = torch.where(live[:, e], v[..., e] - p, torch.zeros(()))
        s = s + d
        q = q + d * d
    cnt = live.sum(1).double()
    pd, sd = p.double(), s.double()
    S = sd + cnt * pd
    Q = q.double() + pd * (2.0 * sd + cnt * pd)
    return torch.stack([S.sum(2), Q.sum(2)], dim=2)


def offset_stem_inputs(n, cx, cc, h, w, seed=0, same_sign=False):
    """unit-variance outputs on the offset family's means: plain inputs, weights of variance 1 / (9 Cin), bias = gn_ref.offset_means(128), or
    its absolute value (same_sign)"""
    g = _gen(n, cx, cc, h, w, seed, 5)
    x = torch.randn((n, cx, h, w), generator=g)
    cond = torch.randn((n, cc, h, w), generator=g)
    wt = torch.randn((STEM_COUT, cx + cc, 3, 3), generator=g) / math.sqrt(9.0 * (cx + cc))
    b = G.offset_means(STEM_COUT).float()
    return x, cond, wt, b.abs() if same_sign else b


def offset_pool_input(n, c, h, w, seed=0, same_sign=False):
    if n * c * h * w > 1 << 22:
        # a large map: one 64 x 64 image of the family, repeated over the map and the batch (per-channel statistics as in the small cases)
        return offset_pool_input(1, c, 64, 64, seed, same_sign).repeat(n, 1, h // 64, w // 64)
    x = G.batch(n, c, h, w, seed=seed, family="offset")[0]
    if same_sign:  # (exact: noise on the 2^-10 grid, offsets 2^3 and 2^6)
        m = G.offset_means(c).float()[None, :, None, None]
        x = (x - m) + m.abs()
    return x


# ------------------------------------------------------------------------------------------------ (d) encoder head

def head_inputs(n, c, hw, o, offset, seed=0):
    """(x [n, c, hw, 1], scale, shift [n, c], w [o, c], b [o]) fp32: scale / shift normalise each channel of x as a GroupNorm table would"""
    g = _gen(n, c, hw, o, int(offset), seed)
    x = torch.randn((n, c, hw, 1), generator=g, dtype=torch.float64) * 1.5 + 0.3
    if offset:
        x = x + (8.0 * (1.0 - 2.0 * (torch.arange(c) % 2)) * (1.0 + 7.0 * (torch.arange(c) // 2 % 2))).double()[None, :, None, None]
    x = x.float()
    gamma = 1.0 + 0.5 * torch.randn((c,), generator=g, dtype=torch.float64)
    beta = torch.randn((c,), generator=g, dtype=torch.float64)
    mean, var = x.double().mean((2, 3)), x.double().var((2, 3), unbiased=False)
    sc = gamma[None] / torch.sqrt(var + 0.25)
    sh = beta[None] - mean * sc
    wt = torch.randn((o, c), generator=g) / math.sqrt(c)
    b = torch.randn((o,), generator=g)
    return x, sc.float(), sh.float(), wt, b


def head_ref64(x, sc, sh, wt, b, hw_div=None, drop_last_quad=False, image0=False):
    """fp64 reference; the keyword arguments make the mutants"""
    n, c = x.shape[:2]
    x = x.double().reshape(n, c, -1)
    sc, sh = sc.double(), sh.double()
    if image0:
        sc = sc[:1].expand_as(sc)
    t = x * sc[:, :, None] + sh[:, :, None]
    a = G.silu(t)
    hw = x.shape[2]
    p = a.sum(2) / float(hw if hw_div is None else hw_div)
    if drop_last_quad:
        p = torch.cat([p[:, :-4], torch.zeros((n, 4), dtype=torch.float64)], 1)
    return p @ wt.double().t() + b.double()[None]


def head_bound(x, sc, sh, wt, b):
    """elementwise |error| allowed for out [n, o]: the count of (d)"""
    n, c = x.shape[:2]
    x = x.double().reshape(n, c, -1)
    hw = x.shape[2]
    xs = x * sc.double()[:, :, None]
    t = xs + sh.double()[:, :, None]
    a = G.silu(t)
    p = a.mean(2)
    e_in = (G.SILU_SLOPE * U * (xs.abs() + t.abs()) + G.silu_eval_bound(a)).mean(2)
    e_pool = e_in + (math.ceil(hw / 4) + 3) * U * a.abs().mean(2) + U * p.abs()
    aw = wt.double().abs()
    out = p @ wt.double().t() + b.double()[None]
    return e_pool @ aw.t() + (2 * math.ceil(c / 64) + 6) * U * (p.abs() @ aw.t()) + U * out.abs()


def head_emulate32(x, sc, sh, wt, b):
    """the kernel's arithmetic in fp32 on the CPU, in its order: product then add, v / (1 + exp(-v)), four chains over every fourth pixel, the fixed
    ((p0 + p1) + p2) + p3, the division, 64 lanes over every 64th channel (product then add), the xor shuffle tree 32 .. 1, + bias"""
    n, c = x.shape[:2]
    x = x.float().reshape(n, c, -1)
    hw = x.shape[2]
    t = x * sc.float()[:, :, None] + sh.float()[:, :, None]
    a = t / (1.0 + torch.exp(-t))
    part = []
    for pl in range(4):
        s = torch.zeros((n, c))
        for p in range(pl, hw, 4):
            s = s + a[:, :, p]
        part.append(s)
    pooled = (((part[0] + part[1]) + part[2]) + part[3]) / float(hw)
    out = torch.zeros((n, wt.shape[0]))
    idx = torch.arange(64)
    for o in range(wt.shape[0]):
        acc = torch.zeros((n, 64))
        for c0 in range(0, c, 64):
            k = min(64, c - c0)
            acc[:, :k] = acc[:, :k] + wt[o, c0:c0 + k].float()[None] * pooled[:, c0:c0 + k]
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, idx ^ off]
        out[:, o] = acc[:, 0] + b[o].float()
    return out


HEAD_MUTANTS = {
    "divide_by_hw_minus_1": lambda x, sc, sh, wt, b: head_ref64(x, sc, sh, wt, b, hw_div=x.shape[2] * x.shape[3] - 1),
    "last_channel_quad_dropped": lambda x, sc, sh, wt, b: head_ref64(x, sc, sh, wt, b, drop_last_quad=True),
    "image0_scale": lambda x, sc, sh, wt, b: head_ref64(x, sc, sh, wt, b, image0=True),
}


# ------------------------------------------------------------------------------------------------ (e) mutants of the stem and the pool

def m_tap_transposed(x, cond, wt, b, rows=None):
    return stem_ref64(x, cond, wt.transpose(2, 3), b, rows)


def m_gather_x_only(x, cond, wt, b, rows):
    """cond read from the output's own batch row: the gather reaches one source only"""
    r = torch.as_tensor(rows, dtype=torch.long)
    return stem_ref64(x[r], cond[:len(rows)], wt, b)


def m_clamped_padding(x, cond, wt, b, rows=None):
    xin = F.pad(torch.cat([x, cond], 1).double(), (1, 1, 1, 1), mode="replicate")
    return F.conv2d(xin, wt.double(), b.double())


def m_ragged_pixels_counted(x, cond, wt, b):
    """tables over whole tiles: the conv of the zero-extended map at the pixels of the last tiles that lie outside the image enter as well"""
    h, w = x.shape[2:]
    hp, wp = -(-h // STEM_TH) * STEM_TH, -(-w // STEM_TW) * STEM_TW
    ext = lambda t: F.pad(t, (0, wp - w, 0, hp - h))
    return tables64(stem_ref64(ext(x), ext(cond), wt, b))


def tile_tables(out):
    """[n, tiles, c, 2] fp64: the (sum, sum of squares) of each 8 x 16 tile of out, tiles row-major as the kernel numbers them"""
    n, c, h, w = out.shape
    res = []
    for y0 in range(0, h, STEM_TH):
        for x0 in range(0, w, STEM_TW):
            res.append(tables64(out[:, :, y0:y0 + STEM_TH, x0:x0 + STEM_TW]))
    return torch.stack(res, dim=1)


def m_table_to_previous_image(out, cus):
    """a workgroup whose range crosses into image n keeps crediting the image it started in"""
    n, c, h, w = out.shape
    tt = tile_tables(out)
    ti = tt.shape[1]
    res = torch.zeros((n, c, 2), dtype=torch.float64)
    for a, b in stem_ranges(n, h, w, cus):
        for t in range(a, b):
            res[a // ti] += tt[t // ti, t % ti]
    return res


def m_pool_shifted(x):
    """the window starts one column late (the last one wraps)"""
    return pool_ref64(torch.roll(x, -1, dims=3))

"""CPU helpers of the sharp GroupNorm32 checks (tests/test_gn_ref_cpu.py, tests/test_gpu_groupnorm.py; DESIGN.md "GroupNorm checks").  No GPU code.

(a) group_norm64: GroupNorm32 (32 groups, eps 1e-5, biased variance) on NCHW in fp64, two-pass, with the per-(image, channel) tables
    sc = rstd * gamma, sh = beta - mean * rstd * gamma the library applies.

(b) bound: the elementwise absolute error the table form y = x * sc + sh may carry when the statistics are right.  The library rounds seven
    times in fp32 (csrc/gn_fold.h gn_finalize_image, then the conv loader):

        1 m  = (float) mean          4 t  = m * sc        6 p = x * sc
        2 r  = (float) rstd          5 sh = beta - t      7 y = p + sh
        3 sc = r * gamma

    x * sc carries roundings 2 3 6, mean * sc carries 1 2 3 4 5, beta carries 5, y carries 7: to first order
    |err| <= 2^-24 (3 |x sc| + 5 |mean sc| + |beta| + |y|).  No term is hit by more than five of the seven; the bound charges every term with all
    seven and one more for what the count leaves out (second-order products, the fp64 statistics, the reference's own rounding):

        K = 8,    bound = K 2^-24 (|x sc| + |mean sc| + |beta| + |y|)

    A reduced mode adds the rounding of y into the conv operand: 2^-22 |y| (f16x3: fp16 hi + lo, 22 bits), 2^-11 |y| (f16), 2^-8 |y| (bf16).
    The bound grows with |mean| / std: inherent to the scale / shift form (torch's fp32 GroupNorm has it too), and what keeps it honest on
    offset data.  beta of every input here has |beta| >= 1/4, so K 2^-24 |beta| >= 2^-23 also covers the absolute floor 2^-25 of an fp16
    subnormal (a y next to zero in f16, the lo half of a small y in f16x3), which a purely relative staging term would miss.

(c) Input families, all seeded; all but `plain` hold multiples of 2^-10 (times powers of two) and are exact in fp32.  batch() puts a different
    family into each image, cycling, so a table read from the wrong image fails as well.

(d) MUTANTS: group norms that are each wrong in one way the real code could be wrong, as plain fp64 functions.
"""
import collections

import torch
import torch.nn.functional as F

from quant_ref import quantise

GROUPS = 32
EPS = 1e-5
K = 8
U = 2.0 ** -24
STAGE = {"fp32": 0.0, "f16x3": 2.0 ** -22, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
MODES = list(STAGE)

GN = collections.namedtuple("GN", "y sc sh mean rstd")  # y [n, c, h, w]; the rest [n, c] (a group's value on each of its channels)


# ------------------------------------------------------------------------------------------------ (a) the reference

def _expand(g, c):
    """[n, 32] per group -> [n, c] per channel"""
    return g.repeat_interleave(c // GROUPS, dim=1)


def _apply(x, mean, rstd, gamma, beta):
    """mean, rstd [n, c] -> GN; y in the centred form (the table form's cancellation is the library's business, not the reference's)"""
    sc = rstd * gamma.double()[None]
    sh = beta.double()[None] - mean * sc
    y = (x - mean[:, :, None, None]) * sc[:, :, None, None] + beta.double()[None, :, None, None]
    return GN(y, sc, sh, mean, rstd)


def group_stats64(x):
    """two-pass (mean, biased variance) per (image, group): [n, 32] each"""
    n = x.shape[0]
    xg = x.double().reshape(n, GROUPS, -1)
    gm = xg.mean(2)
    return gm, ((xg - gm[:, :, None]) ** 2).mean(2)


def group_norm64(x, gamma, beta):
    x = x.double()
    c = x.shape[1]
    assert c % GROUPS == 0
    gm, gv = group_stats64(x)
    return _apply(x, _expand(gm, c), _expand(1.0 / torch.sqrt(gv + EPS), c), gamma, beta)


def upsample(x0):
    return F.interpolate(x0.double(), scale_factor=2, mode="nearest")


def concat_norm64(x0, x1, gamma, beta):
    """GroupNorm32 of cat(nearest_x2(x0), x1): x0 is STORED at quarter resolution"""
    return group_norm64(torch.cat([upsample(x0), x1.double()], dim=1), gamma, beta)


# ------------------------------------------------------------------------------------------------ (b) the bound

def bound(x, sc, sh, y, mode, beta):
    """elementwise |error| allowed for y = x * sc + sh in `mode`; x, y [n, c, h, w] fp64, sc, sh [n, c] fp64, beta [c].  mean * sc = beta - sh."""
    b = beta.double()[None]
    core = (x.double() * sc[:, :, None, None]).abs() + ((b - sh).abs() + b.abs())[:, :, None, None] + y.abs()
    return K * U * core + STAGE[mode] * y.abs()


def table_form32(x, gn, gamma, beta):
    """the library's arithmetic on exact statistics: the seven fp32 roundings of (b), as fp32"""
    m, r = gn.mean.float(), gn.rstd.float()
    sc = r * gamma.float()[None]
    sh = beta.float()[None] - m * sc
    return x.float() * sc[:, :, None, None] + sh[:, :, None, None]


def stage(y32, mode):
    """the conv operand a mode makes of an fp32 activation, as fp64: fp16 hi + lo (f16x3), real fp16 with its subnormals (f16), bf16"""
    if mode == "fp32":
        return y32.double()
    if mode == "f16x3":
        hi = y32.half()
        return hi.double() + (y32 - hi.float()).half().double()
    if mode == "f16":
        return y32.half().double()
    return quantise(y32, mode, "act")


def first_outside(err, bnd):
    """for an assertion message: None when err <= bnd everywhere, else (count, index, error, bound) of the first element outside"""
    bad = ~(err <= bnd)  # (a NaN is outside)
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return int(bad.sum()), idx, float(err[idx]), float(bnd[idx])


def worst_ratio(err, bnd):
    return float((err / bnd.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ (c) inputs

FAMILIES = ["offset", "scales", "const", "zero", "per_image", "plain"]  # "const" and "zero" are the constant family: zero kills the rest of an image


def _noise(shape, gen):
    """unit-variance noise on the 2^-10 grid"""
    return torch.round(torch.randn(shape, generator=gen, dtype=torch.float64) * 1024.0) / 1024.0


def offset_means(c):
    """per-channel means of the offset family: 2^3 in even groups, 2^6 in odd ones; the sign alternates inside a group and flips every second
    group, so the one-channel groups of c = 32 see both signs of both magnitudes"""
    ch = torch.arange(c)
    g, k = ch // (c // GROUPS), ch % (c // GROUPS)
    mag = torch.where(g % 2 == 0, 8.0, 64.0).double()
    return mag * (1.0 - 2.0 * ((k + g // 2) % 2).double())


def scale_exponents(c):
    """the scales family: channel ch is scaled by 2^((ch % 13) - 6), so neighbours inside a group differ and one-channel groups span 2^-6 .. 2^6"""
    return (torch.arange(c) % 13 - 6).double()


def image(family, c, h, w, index, gen):
    """one image [c, h, w] fp32 of a family; index = its position in the batch (per_image: scaled by 4^(index % 5), shifted by index % 5)"""
    cpg = c // GROUPS
    if family == "zero":
        return torch.zeros((c, h, w))
    if family == "plain":
        return torch.randn((c, h, w), generator=gen) * 1.5 + 0.3
    x = _noise((c, h, w), gen)
    if family == "offset":
        x = x + offset_means(c)[:, None, None]
    elif family == "scales":
        x = x * torch.exp2(scale_exponents(c))[:, None, None]
    elif family == "const":
        x[2 * cpg - 1] = 0.75  # the last channel of group 1
        x[3 * cpg:4 * cpg] = 2.0  # all of group 3
    elif family == "per_image":
        x = x * 4.0 ** (index % 5) + index % 5
    else:
        raise ValueError(family)
    x32 = x.float()
    assert bool((x32.double() == x).all())  # exact in fp32
    return x32


def batch(n, c, h, w, start=0, seed=0, family=None):
    """[n, c, h, w] fp32: image i of FAMILIES[(start + i) % 6], or every image of `family`"""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * c + h * w + start)
    fams = [family or FAMILIES[(start + i) % len(FAMILIES)] for i in range(n)]
    return torch.stack([image(f, c, h, w, i, gen) for i, f in enumerate(fams)]), fams


def starts(n):
    """batch starts that put every family into some image"""
    return list(range(0, len(FAMILIES), n))


def affine(c, seed=0):
    """(gamma, beta) fp32: gamma of both signs and exactly 0 on every eleventh channel; 1/4 <= |beta| <= 1 of both signs"""
    gen = torch.Generator().manual_seed(104729 * seed + c)
    gamma = 1.0 + 0.5 * torch.randn((c,), generator=gen)
    gamma[torch.arange(c) % 3 == 1] *= -1.0
    gamma[torch.arange(c) % 11 == 5] = 0.0
    beta = 0.25 + 0.75 * torch.rand((c,), generator=gen)
    beta[torch.arange(c) % 2 == 1] *= -1.0
    return gamma, beta


# the shapes of Probe A (tests/test_gpu_groupnorm.py says what each covers)
PROBE_A = [(3, 32, 4, 4), (2, 64, 6, 10), (5, 192, 8, 8), (2, 384, 10, 20), (1, 1408, 4, 8), (1, 1600, 4, 4)]
# the concat of the decoder cases of Probe B: x0 [n, 64] stored at quarter resolution, x1 [n, 32]; 96 channels, 3 per group: group 21 holds
# channel 63 of x0 and channels 0, 1 of x1
CONCAT = (2, 64, 32, 8, 8)


def concat_inputs(n, c0, c1, h, w, seed=0):
    """(x0 stored [n, c0, h/2, w/2], x1 [n, c1, h, w]) with different offsets and scales, on the 2^-10 grid"""
    gen = torch.Generator().manual_seed(15485863 * seed + c0 + c1 + h * w + n)
    x0 = _noise((n, c0, h // 2, w // 2), gen) * 4.0 + 3.0
    x1 = _noise((n, c1, h, w), gen) * 0.5 - 2.0
    return x0.float(), x1.float()


# ------------------------------------------------------------------------------------------------ (d) mutants

def chan_tables(x):
    """per-(image, channel) (mean, mean of squares) [n, c]: what the library keeps"""
    x = x.double()
    return x.mean((2, 3)), (x * x).mean((2, 3))


def _from_tables(x, m, q, gamma, beta, keep=None, divisor=None):
    """group norm of x from per-channel tables, E[x^2] - E[x]^2 clamped at 0 as gn_finalize_image does; keep [c]: 0 / 1 weights of the channels
    that enter the sums; divisor: what the sums are divided by (default: channels per group)"""
    n, c = m.shape
    cpg = c // GROUPS
    k = torch.ones(c, dtype=torch.float64) if keep is None else keep.double()
    d = float(cpg) if divisor is None else divisor
    gm = (m * k).reshape(n, GROUPS, cpg).sum(2) / d
    gq = (q * k).reshape(n, GROUPS, cpg).sum(2) / d
    gv = (gq - gm * gm).clamp_min(0.0)
    return _apply(x.double(), _expand(gm, c), _expand(1.0 / torch.sqrt(gv + EPS), c), gamma, beta).y


def _with_stats(x, gamma, beta, rstd_of, gidx=None, image0=False):
    x = x.double()
    c = x.shape[1]
    gm, gv = group_stats64(x)
    gr = rstd_of(gv, x[0].numel() // GROUPS)
    if image0:
        gm, gr = gm[:1].expand_as(gm), gr[:1].expand_as(gr)
    if gidx is None:
        gidx = torch.arange(c) // (c // GROUPS)
    return _apply(x, gm[:, gidx], gr[:, gidx], gamma, beta).y


_RSTD = lambda gv, cnt: 1.0 / torch.sqrt(gv + EPS)


def m_unbiased(x, gamma, beta):
    return _with_stats(x, gamma, beta, lambda gv, cnt: 1.0 / torch.sqrt(gv * cnt / (cnt - 1) + EPS))


def m_eps_1e6(x, gamma, beta):
    return _with_stats(x, gamma, beta, lambda gv, cnt: 1.0 / torch.sqrt(gv + 1e-6))


def m_eps_after_sqrt(x, gamma, beta):
    return _with_stats(x, gamma, beta, lambda gv, cnt: 1.0 / (torch.sqrt(gv) + EPS))


def m_group_off_by_one(x, gamma, beta):
    c = x.shape[1]
    cpg = c // GROUPS
    ch = torch.arange(c)
    gidx = ch // cpg
    gidx = torch.where((ch % cpg == 0) & (gidx > 0), gidx - 1, gidx)
    return _with_stats(x, gamma, beta, _RSTD, gidx=gidx)


def m_image0_table(x, gamma, beta):
    return _with_stats(x, gamma, beta, _RSTD, image0=True)


def m_last_channel_left_out(x, gamma, beta):
    """the eight-lane stride bug: a group's last channel never enters the sums, which are still divided by cpg"""
    c = x.shape[1]
    m, q = chan_tables(x)
    return _from_tables(x, m, q, gamma, beta, keep=(torch.arange(c) % (c // GROUPS) != c // GROUPS - 1))


def _cat(x0, x1):
    m0, q0 = chan_tables(x0)  # (on the stored map: replication leaves per-channel means unchanged)
    m1, q1 = chan_tables(x1)
    return torch.cat([upsample(x0), x1.double()], dim=1), m0, q0, m1, q1


def m_concat_same_count(x0, x1, gamma, beta):
    """raw sums of both sources divided by the full-resolution pixel count: the quarter-resolution source's means come out quartered"""
    x, m0, q0, m1, q1 = _cat(x0, x1)
    return _from_tables(x, torch.cat([m0 / 4, m1], 1), torch.cat([q0 / 4, q1], 1), gamma, beta)


def m_concat_boundary_source0(x0, x1, gamma, beta):
    """a group that straddles the boundary is built from its source-0 channels alone"""
    x, m0, q0, m1, q1 = _cat(x0, x1)
    c0, c = m0.shape[1], m0.shape[1] + m1.shape[1]
    cpg = c // GROUPS
    assert c0 % cpg != 0, "no group straddles the boundary"
    gb = c0 // cpg
    y = _from_tables(x, torch.cat([m0, m1], 1), torch.cat([q0, q1], 1), gamma, beta).clone()
    keep = (torch.arange(c) < c0)
    part = _from_tables(x, torch.cat([m0, m1], 1), torch.cat([q0, q1], 1), gamma, beta, keep=keep, divisor=float(c0 - gb * cpg))
    y[:, gb * cpg:(gb + 1) * cpg] = part[:, gb * cpg:(gb + 1) * cpg]
    return y


def fp32_lane_tables(x, per=8):
    """the fused conv epilogue's arithmetic (csrc/conv_split2.hip): a lane adds `per` values and their squares in fp32, one rounding per
    operation, and only the lane totals are added in double.  -> (mean, mean of squares) [n, c] fp64"""
    n, c, h, w = x.shape
    hw = h * w
    v = x.float().reshape(n, c, hw)
    pad = (-hw) % per
    if pad:
        v = torch.cat([v, torch.zeros((n, c, pad))], dim=2)
    v = v.reshape(n, c, -1, per)
    s = torch.zeros(v.shape[:3])
    q = torch.zeros(v.shape[:3])
    for e in range(per):
        s = s + v[..., e]
        q = q + v[..., e] * v[..., e]
    return s.double().sum(2) / hw, q.double().sum(2) / hw


def m_fp32_squares(x, gamma, beta):
    m, q = fp32_lane_tables(x)
    return _from_tables(x, m, q, gamma, beta)


# name -> (kind, function): "single" takes (x, gamma, beta), "concat" takes (x0 stored, x1, gamma, beta); each returns y fp64
MUTANTS = collections.OrderedDict([
    ("unbiased_variance", ("single", m_unbiased)),
    ("eps_1e-6", ("single", m_eps_1e6)),
    ("eps_after_sqrt", ("single", m_eps_after_sqrt)),
    ("group_off_by_one", ("single", m_group_off_by_one)),
    ("image0_table", ("single", m_image0_table)),
    ("last_channel_left_out", ("single", m_last_channel_left_out)),
    ("concat_same_count", ("concat", m_concat_same_count)),
    ("concat_boundary_source0", ("concat", m_concat_boundary_source0)),
    ("fp32_squares", ("single", m_fp32_squares)),
])
MEASURED_ONLY = "fp32_squares"  # not asserted: its error / bound ratio is the prediction of what the fused epilogue costs


# ------------------------------------------------------------------------------------------------ Probe B: a ResBlock whose output shows GN2

SILU_SLOPE = 1.1  # max |d silu / dx| = 1.0998 at x = 2.4


def silu(x):
    return x * torch.sigmoid(x)


def silu_eval_bound(a):
    """|error| of v * rcp(1 + __expf(-v)) in fp32 against silu(v) = a (csrc/conv_split2.hip silu2): the exponent's argument scaling (|v| 2^-24
    relative in e^-v) and v_exp_f32 (2^-23) weigh on the result by e^-v / (1 + e^-v); the add, the reciprocal (1 ulp) and the product add
    2^-24 + 2^-23 + 2^-24.  |silu(v)| (|v| + 2) (1 - sigmoid(v)) < 1.5 for every v, so |error| <= 2^-24 (4 |a| + 1.5); the constant is rounded
    up to 2, which also covers the 2^-25 floor of an fp16 subnormal lo half in f16x3."""
    return U * (4.0 * a.abs() + 2.0)


def identity3x3(c):
    w = torch.zeros((c, c, 3, 3))
    w[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    return w


def selection3x3(cout, cin):
    """centre-tap selection of all cin input channels into the first cin outputs"""
    w = torch.zeros((cout, cin, 3, 3))
    w[torch.arange(cin), torch.arange(cin), 1, 1] = 1.0
    return w


# name -> (n, c0, c1, cout, h, w, up0, modes): the smallest shape of each form (tests/test_gpu_conv_forms.py)
PROBE_B = collections.OrderedDict([
    ("prologue_128x32", (1, 32, 0, 32, 16, 16, False, ("fp32", "f16x3"))),
    ("ragged", (2, 64, 0, 64, 6, 10, False, ("fp32", "f16x3"))),
    ("split_in_launch", (1, 256, 0, 256, 16, 16, False, ("fp32", "f16x3"))),
    ("split_reduce", (32, 128, 0, 128, 4, 8, False, ("fp32", "f16x3"))),
    ("deferred_fold_256", (16, 32, 0, 64, 64, 64, False, ("fp32",))),
    ("parity", (11, 64, 32, 128, 64, 64, True, ("fp32", "f16x3"))),
    ("parity_prologue", (2, 64, 32, 128, 64, 64, True, ("fp32", "f16x3"))),
])
_BLOCKS = {}


def block_params(name):
    """(P, x0, x1, emb): the block's state dict (names of test_gpu_upconv.res_manifest, in that order) and inputs, fp32 on the CPU.
    out_layers conv = centre-tap identity, zero bias; in_layers.2.bias and emb_layers.1.bias = the offset family's means (half each, so h1
    carries them once); skip_connection, where there is one, zero.  Concat cases: in_layers conv = centre-tap selection."""
    from drmnet_amd import synth
    from test_gpu_upconv import res_manifest

    n, c0, c1, cout, h, w, up0, _ = PROBE_B[name]
    cin = c0 + c1
    P = synth.synth_state_dict(res_manifest(cin, cout), 5)
    g1, b1 = affine(cin, 1)
    g2, b2 = affine(cout, 2)
    P["in_layers.0.weight"], P["in_layers.0.bias"] = g1, b1
    P["out_layers.0.weight"], P["out_layers.0.bias"] = g2, b2
    means = offset_means(cout).float()
    P["in_layers.2.bias"] = means / 2
    P["emb_layers.1.bias"] = means / 2
    P["out_layers.3.weight"], P["out_layers.3.bias"] = identity3x3(cout), torch.zeros(cout)
    if cin != cout:
        P["skip_connection.weight"], P["skip_connection.bias"] = torch.zeros((cout, cin, 1, 1)), torch.zeros(cout)
    gen = torch.Generator().manual_seed(sum(ord(ch) for ch in name))
    emb = torch.randn((n, 512), generator=gen)
    if c1:
        P["in_layers.2.weight"] = selection3x3(cout, cin)
        x0, x1 = concat_inputs(n, c0, c1, h, w, seed=3)
    else:
        x0, x1 = batch(n, c0, h, w, seed=11, family="plain")[0], None  # (GN1 is Probe A's business: h1's offsets come from the biases)
    return P, x0, x1, emb


def _block(P, x0, x1, emb, dt, gn1=None):
    """(h1, block input) in dtype dt: torch's own arithmetic of the first stage; gn1 (fp64 only): a group norm to put in GN1's place, called as
    gn1(x, gamma, beta) or, on a concat, gn1(x0 stored, x1, gamma, beta)"""
    D = {k: v.to(dt) for k, v in P.items()}
    x = x0.to(dt) if x1 is None else torch.cat([F.interpolate(x0.to(dt), scale_factor=2, mode="nearest"), x1.to(dt)], dim=1)
    if gn1 is None:
        y1 = F.group_norm(x, GROUPS, D["in_layers.0.weight"], D["in_layers.0.bias"], EPS)
    else:
        y1 = gn1(x0, P["in_layers.0.weight"], P["in_layers.0.bias"]) if x1 is None else gn1(x0, x1, P["in_layers.0.weight"], P["in_layers.0.bias"])
    a = silu(y1)
    if x1 is None:
        h = F.conv2d(a, D["in_layers.2.weight"], D["in_layers.2.bias"], padding=1)
    else:  # the selection conv, without the multiplications by 0 and 1
        cin, cout = x.shape[1], D["in_layers.2.bias"].shape[0]
        h = torch.cat([a, torch.zeros((x.shape[0], cout - cin) + tuple(x.shape[2:]), dtype=dt)], dim=1) + D["in_layers.2.bias"][None, :, None, None]
    e = F.linear(silu(emb.to(dt)), D["emb_layers.1.weight"], D["emb_layers.1.bias"])
    return h + e[:, :, None, None], x


def _block_base(name):
    if name not in _BLOCKS:
        P, x0, x1, emb = block_params(name)
        h64, x64 = _block(P, x0, x1, emb, torch.float64)
        h32, _ = _block(P, x0, x1, emb, torch.float32)
        u = float((h32.double() - h64).abs().max())
        gn2 = group_norm64(h64, P["out_layers.0.weight"], P["out_layers.0.bias"])
        a2 = silu(gn2.y)
        ref = a2 + x64 if x64.shape[1] == a2.shape[1] else a2
        _BLOCKS[name] = (P, x0, x1, emb, h64, u, gn2, a2, ref)
    return _BLOCKS[name]


def block_forward64(name, gn1=None, gn2=None):
    """the block's output in fp64 with a mutant in GN1's or GN2's place (tests/test_gn_ref_cpu.py)"""
    P, x0, x1, emb, h64, _, _, _, _ = _block_base(name)
    h, x = (h64, None) if gn1 is None else _block(P, x0, x1, emb, torch.float64, gn1)
    if x is None:
        x = x0.double() if x1 is None else torch.cat([upsample(x0), x1.double()], dim=1)
    y2 = (gn2 or (lambda t, g, b: group_norm64(t, g, b).y))(h, P["out_layers.0.weight"], P["out_layers.0.bias"])
    a2 = silu(y2)
    return a2 + x if x.shape[1] == a2.shape[1] else a2


def block_case(name, mode):
    """(P, x0, x1, emb, reference fp64 of the block's output, its elementwise bound in `mode`): computed once per (name, mode), never modified.

    out = skip + SiLU(GN2(h1)); skip = x where cin == cout, else 0.  The bound:
        SILU_SLOPE (bound(GN2) + 2 |sc2| u)     u = max |h1 of torch's CPU fp32 - h1 fp64|: the error h1 carries when GN2 reads it, measured on
                                                the reference arithmetic; the factor 2 for a different accumulation order
      + silu_eval_bound + STAGE[mode] |a2|      evaluating SiLU in fp32 and rounding it into the conv operand
      + 2^-24 |out|                             the epilogue's residual add
    For the concat cases h1 is itself SiLU(GN1(cat)) selected through the in_layers conv: u is measured on that whole first stage, the same rule."""
    key = (name, mode)
    if key not in _BLOCKS:
        P, x0, x1, emb, h64, u, gn2, a2, ref = _block_base(name)
        b = SILU_SLOPE * (bound(h64, gn2.sc, gn2.sh, gn2.y, "fp32", P["out_layers.0.bias"]) + 2.0 * u * gn2.sc.abs()[:, :, None, None])
        b = b + silu_eval_bound(a2) + STAGE[mode] * a2.abs() + U * ref.abs()
        _BLOCKS[key] = (P, x0, x1, emb, ref, b)
    return _BLOCKS[key]

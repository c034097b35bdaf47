"""CPU helpers of the sharp conv checks (tests/test_quant_ref_cpu.py, tests/test_gpu_conv_exact.py, tests/test_gpu_conv_modes.py).  No GPU code.

Two ideas (DESIGN.md "Exact and emulated conv checks"):

(a) Dyadic inputs.  x in {k/8 : |k| <= 16}, w in {k/32 : |k| <= 16}: every product is a multiple of 2^-8 with |p| <= 1, a sum of K < 2^14 of them has
    at most 22 significant bits, so fp32 accumulation is exact in any order (split-K slabs included), the operands are fp16 / bf16 numbers (the fp16
    `lo` halves and the e4m3 cross terms are zero), the weight pre-scale and the range guard are powers of two, and the epilogue adds dyadic terms.
    Every mode must EQUAL the fp64 reference: exact_bits states the budget of a case, first_mismatch names the element.

(b) Reduced-precision modes (f16, bf16) round their conv operands; quantise restates that rounding, res_block64 restates the ResBlock in fp64 with
    a hook on every conv operand, and classes cuts the output into the places where an addressing bug would sit (border ring, tile edges, images,
    32-channel blocks, parities, pixel tiles).  Operand rounding is spatially homogeneous: the relative error of every class stays within a few per
    cent of the whole tensor's (measured [0.93, 1.08] on the CPU), so a class outside [0.8, 1.25] is a bug that whole-tensor rel-L2 dilutes.
"""
import collections
import math

import torch
import torch.nn.functional as F

from conftest import rel_l2
from drmnet_amd import ops, synth
from oracle import unet as ou
from test_gpu_upconv import res_manifest  # (a helper: the state-dict names of one ResBlock)

# pixel-tile families of the conv pipeline, larger first (csrc/conv_forms.h DRM_PIXEL_TILES), and those with masked-edge instantiations
PIXEL_TILES = [(16, 16), (8, 16), (8, 8), (4, 8), (4, 4)]
RAGGED_TILES = [(8, 16), (8, 8), (4, 4)]
TERMS = {"fp32": 0, "f16": 1, "f16mx": 2, "f16x3": 3, "bf16": 4}  # the TERMS template argument of conv_split2_kernel per mode (f16mx: its mx sites)
MIN_CLASS = 512
RATIO = (0.8, 1.25)


# ------------------------------------------------------------------------------------------------ (a) dyadic inputs

def dyadic(shape, step, kmax, gen):
    """random multiples of `step` with |k| <= kmax, as fp32"""
    k = torch.randint(-kmax, kmax + 1, tuple(shape), generator=gen)
    return (k.double() * step).float()


def exact_bits(K, x_step, x_max, w_step, w_max, adds=()):
    """Significant bits the widest intermediate of  sum_K x w (+ each of `adds` = [(step, max), ...] in turn)  can need: every partial sum is a
    multiple of the smallest step and bounded by K x_max w_max + sum of the maxima.  fp32 holds 24: asserted."""
    steps = [x_step * w_step] + [s for s, _ in adds]
    for s in steps:
        assert s > 0 and math.frexp(s)[0] == 0.5, f"step {s} is no power of two"
    unit = min(steps)
    bound = K * x_max * w_max + sum(m for _, m in adds)
    bits = math.ceil(math.log2(bound / unit + 1))
    assert bits <= 24, f"K = {K}: {bits} bits do not fit fp32's 24"
    return bits


X_STEP, X_KMAX, W_STEP, W_KMAX = 1 / 8, 16, 1 / 32, 16
ADD_STEP, ADD_KMAX = 1 / 8, 16  # bias, emb and residual of the epilogue cases

# name -> (n, cin, cout, h, w, k, extras): every conv case of tests/test_gpu_conv_exact.py.  extras: "epi" = bias, emb and residual live;
# "guard" = image n scaled by 2^GUARD_J[n].
GUARD_J = (20, -20, 5, 0, -9)
EXACT_CASES = {}


def _case(name, n, cin, cout, h, w, k, extras=""):
    EXACT_CASES[name] = (n, cin, cout, h, w, k, extras)


# every GEMM tile through the op (the shapes of tests/test_gpu_conv_forms.py, which records why they cannot be smaller)
_case("tile_128x32", 1, 32, 32, 16, 16, 3)
_case("tile_128x64_1x1", 32, 32, 64, 32, 32, 1)
_case("tile_256x64", 16, 32, 64, 64, 64, 3)
_case("tile_256x128", 11, 32, 128, 64, 64, 3)
_case("tile_256x192_1x1", 2, 32, 192, 256, 256, 1)
_case("tile_256x256_1x1", 2, 32, 256, 256, 256, 1)
_case("tile_ragged", 1, 32, 64, 6, 10, 3)
# ragged and odd maps
for _h, _w in [(6, 10), (12, 20), (7, 9), (5, 5), (2, 2), (1, 1), (4, 36)]:
    for _k in (1, 3):
        _case(f"map_{_h}x{_w}_k{_k}", 2, 32, 32, _h, _w, _k)
# multi-image tiles that are not filled
_case("images_5_on_4x8", 5, 32, 32, 4, 8, 3)
_case("images_3_on_8x8", 3, 32, 64, 8, 8, 3)
_case("images_9_on_4x4_768", 9, 768, 768, 4, 4, 3)
# channel edges: padded input channels (kc = 8 path for 3x3, whole-chunk padding for 1x1), masked output channels, the longest 1x1 reduction
for _k in (1, 3):
    _case(f"cin_6_k{_k}", 2, 6, 32, 8, 8, _k)
    _case(f"cin_40_k{_k}", 2, 40, 64, 8, 8, _k)
    _case(f"cout_3_k{_k}", 2, 32, 3, 8, 8, _k)
    _case(f"cout_40_k{_k}", 2, 32, 40, 8, 8, _k)
_case("cin_1536_1x1", 2, 1536, 64, 8, 8, 1)
# every epilogue term live: plain, ragged, multi-image
_case("epi_plain", 2, 32, 64, 16, 16, 3, "epi")
_case("epi_ragged", 2, 32, 64, 6, 10, 3, "epi")
_case("epi_images_5_on_4x8", 5, 64, 32, 4, 8, 1, "epi")
# range guard: per-image powers of two
_case("guard_k3", 5, 32, 32, 8, 8, 3, "guard")
_case("guard_k1", 5, 32, 64, 8, 8, 1, "guard")

# ops.linear without SiLU, on the shapes of test_gpu_ops.test_linear_variants: (n, in, out) -> the kernel launch_linear (csrc/misc.hip) picks
LINEAR_CASES = [(3, 6, 64, "linear_kernel"), (5, 64, 64, "linear_mfma_kernel"), (2, 128, 512, "linear_rows_kernel"), (32, 512, 512, "linear_mfma_kernel"),
                (4, 512, 14976, "linear_rows_kernel"), (1, 100, 7, "linear_kernel")]


def exact_case_bits(name):
    n, cin, cout, h, w, k, extras = EXACT_CASES[name]
    adds = [(ADD_STEP, ADD_STEP * ADD_KMAX)] * 3 if "epi" in extras else []
    return exact_bits(cin * k * k, X_STEP, X_STEP * X_KMAX, W_STEP, W_STEP * W_KMAX, adds)


def igemm_expected(name, mode):
    """plan_conv's rule (csrc/conv_plan.hip): the pipeline kernel takes whole 32-chunks of (padded) input channels, exact fp32 only on maps that
    are whole 4x4 tiles; conv_igemm_kernel takes the rest.  The op pads Cin to 32 for 1x1 and to 8 for 3x3 (csrc/abi.hip)."""
    n, cin, cout, h, w, k, _ = EXACT_CASES[name]
    cinp = (cin + 31) // 32 * 32 if k == 1 else (cin + 7) // 8 * 8
    return cinp % 32 != 0 or (mode == "fp32" and (h % 4 != 0 or w % 4 != 0))


_EXACT = {}


def exact_case(name):
    """(x, wt, bias, emb, res, ref fp64) of a conv case: computed once, shared by the modes, never modified.  For a "guard" case x is already
    scaled per image and ref is the scaled reference."""
    if name not in _EXACT:
        n, cin, cout, h, w, k, extras = EXACT_CASES[name]
        exact_case_bits(name)
        gen = torch.Generator().manual_seed(sum(ord(ch) for ch in name))
        x = dyadic((n, cin, h, w), X_STEP, X_KMAX, gen)
        wt = dyadic((cout, cin, k, k), W_STEP, W_KMAX, gen)
        bias = emb = res = None
        if "epi" in extras:
            bias = dyadic((cout,), ADD_STEP, ADD_KMAX, gen)
            emb = dyadic((n, cout), ADD_STEP, ADD_KMAX, gen)
            res = dyadic((n, cout, h, w), ADD_STEP, ADD_KMAX, gen)
        ref = F.conv2d(x.double(), wt.double(), None if bias is None else bias.double(), padding=k // 2)
        if emb is not None:
            ref = ref + emb.double()[:, :, None, None] + res.double()
        if "guard" in extras:
            s = torch.tensor([2.0 ** j for j in GUARD_J[:n]], dtype=torch.float64)[:, None, None, None]
            x, ref = (x.double() * s).float(), ref * s
        _EXACT[name] = (x, wt, bias, emb, res, ref)
    return _EXACT[name]


_LINEAR = {}


def linear_case(n, i, o):
    if (n, i, o) not in _LINEAR:
        exact_bits(i, X_STEP, X_STEP * X_KMAX, W_STEP, W_STEP * W_KMAX, [(ADD_STEP, ADD_STEP * ADD_KMAX)])
        gen = torch.Generator().manual_seed(n + i + o)
        x, wt, b = dyadic((n, i), X_STEP, X_KMAX, gen), dyadic((o, i), W_STEP, W_KMAX, gen), dyadic((o,), ADD_STEP, ADD_KMAX, gen)
        _LINEAR[(n, i, o)] = (x, wt, b, F.linear(x.double(), wt.double(), b.double()))
    return _LINEAR[(n, i, o)]


class Mismatch(collections.namedtuple("Mismatch", "index got want count total classes")):
    """index = (n, c, y, x) of the first element that differs, its two values, how many differ, and the classes they fall in"""

    def __str__(self):
        return (f"{self.count} of {self.total} elements differ; first at (n, c, y, x) = {self.index}: got {self.got!r}, want {self.want!r}"
                + (f"; classes hit: {self.classes}" if self.classes is not None else ""))


def first_mismatch(out, ref, cls=None):
    """for an assertion message: the Mismatch of `out` [N, C, H, W] against `ref`, or None where they are equal"""
    out, ref = out.detach().cpu(), ref.detach().cpu().to(out.dtype)
    bad = out != ref
    if out.dtype.is_floating_point:
        bad |= torch.isnan(out)
    count = int(bad.sum())
    if count == 0:
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    where = None if cls is None else [nm for nm, m in cls.items() if bool((bad & m).any())]
    return Mismatch(idx, out[idx].item(), ref[idx].item(), count, out.numel(), where)


# ------------------------------------------------------------------------------------------------ (b) operand rounding of the reduced modes

def quantise(t, mode, kind):
    """The conv operand the kernel multiplies in `mode`, as fp64.  kind "act": a staged activation (GroupNorm-fed, or a raw input behind its
    per-image power-of-two range guard); kind "w": a weight tensor (pre-scaled as csrc/conv_split.hip split_scale_kernel does).
      bf16        round to nearest even (activations and weights alike; its exponent range is fp32's)
      f16, act    round to 11 significant bits, range-free (the guard moves a raw input into range; normalised values are O(1))
      f16, w      half(w 2^k) / 2^k, k = 14 - e with max|w| = f 2^e, clamped to +-30
    Every other mode keeps at least 22 bits: identity."""
    t32 = t.float()  # (what the kernel reads is an fp32 number)
    if mode == "bf16":
        return t32.bfloat16().double()
    if mode != "f16":
        return t.double()
    if kind == "w":
        m = float(t32.abs().max())
        k = 0
        if 0.0 < m < math.inf:
            k = max(-30, min(30, 14 - math.frexp(m)[1]))
        return (t32 * 2.0 ** k).half().double() / 2.0 ** k
    mant, e = torch.frexp(t32.double())
    return torch.ldexp(torch.round(mant * 2048.0) / 2048.0, e)


def identity(t, kind, site):
    return t.double()


def mode_hook(mode):
    return lambda t, kind, site: quantise(t, mode, kind)


def _gn_silu(x, w, b):
    return ou.silu(F.group_norm(x, ou.GN_GROUPS, w, b, ou.GN_EPS))


def res_block64(P, x0, emb, x1=None, up0=False, hook=identity, two_launch=False):
    """ResBlock._forward in fp64 on cat(nearest_x2(x0) if up0, x1), with hook(tensor, kind, site) on every conv operand (kind "act" / "w"; site
    "in", "in_a", "in_b", "out", "skip").  P: the block's state dict (fp32, names of test_gpu_upconv.res_manifest).  The emb linear is fp32 in
    every mode of the library (launch_linear takes no precision): not hooked.  two_launch: the in_layers conv as the 4-tap parity form on the
    stored x0 (weights folded by ops.fold_upconv_weight, THEN hooked) plus the 3x3 conv on x1."""
    D = {k: v.double() for k, v in P.items()}
    c0 = x0.shape[1]
    xs = [F.interpolate(x0.double(), scale_factor=2, mode="nearest") if up0 else x0.double()] + ([x1.double()] if x1 is not None else [])
    x = torch.cat(xs, dim=1)
    cin, cout = x.shape[1], D["in_layers.2.weight"].shape[0]
    a = _gn_silu(x, D["in_layers.0.weight"], D["in_layers.0.bias"])
    w1 = D["in_layers.2.weight"]
    if two_launch:
        assert up0 and x1 is not None
        wa, wb = ops.fold_upconv_weight(w1, c0)
        a0 = F.pad(hook(a[:, :c0, ::2, ::2], "act", "in_a"), (1, 1, 1, 1))  # (per element, GroupNorm + SiLU commute with the replication)
        wa = hook(wa, "w", "in_a")
        hs, ws = x0.shape[2], x0.shape[3]
        h = F.conv2d(hook(a[:, c0:], "act", "in_b"), hook(wb, "w", "in_b"), D["in_layers.2.bias"], padding=1)
        for pa in (0, 1):
            for pb in (0, 1):
                p = 2 * pa + pb
                h[:, :, pa::2, pb::2] += F.conv2d(a0[:, :, pa:pa + hs + 1, pb:pb + ws + 1], wa[p * cout:(p + 1) * cout])
    else:
        h = F.conv2d(hook(a, "act", "in"), hook(w1, "w", "in"), D["in_layers.2.bias"], padding=1)
    e = F.linear(ou.silu(emb.double()), D["emb_layers.1.weight"], D["emb_layers.1.bias"])
    h = h + e[:, :, None, None]
    a2 = _gn_silu(h, D["out_layers.0.weight"], D["out_layers.0.bias"])
    h = F.conv2d(hook(a2, "act", "out"), hook(D["out_layers.3.weight"], "w", "out"), D["out_layers.3.bias"], padding=1)
    if cin != cout:
        x = F.conv2d(hook(x, "act", "skip"), hook(D["skip_connection.weight"], "w", "skip"), D["skip_connection.bias"])
    return x + h


# ------------------------------------------------------------------------------------------------ where an error sits

def tile_family(h, w):
    """the pixel-tile family plan_conv picks for an H x W map: the largest that divides it, else the masked-edge family wasting the fewest rows"""
    for th, tw in PIXEL_TILES:
        if h % th == 0 and w % tw == 0:
            return th, tw
    area = lambda f: -(-h // f[0]) * f[0] * (-(-w // f[1]) * f[1])
    best = None
    for f in RAGGED_TILES:
        if best is None or area(f) < area(best):
            best = f
    return best


def _merged(group, min_count):
    """[(name, mask), ...] in order; a class with fewer than min_count elements is merged into its neighbour (the next one; the last into the
    previous)"""
    out = []
    carry = None
    for nm, m in group:
        if carry is not None:
            nm, m = carry[0] + "+" + nm, carry[1] | m
            carry = None
        if int(m.sum()) < min_count:
            carry = (nm, m)
        else:
            out.append((nm, m))
    if carry is not None:
        if out:
            out[-1] = (out[-1][0] + "+" + carry[0], out[-1][1] | carry[1])
        elif int(carry[1].sum()) > 0:
            out.append(carry)
    return out


def classes(n, c, h, w, min_count=MIN_CLASS):
    """{name: boolean mask [n, c, h, w]}: border ring / interior, the tile-edge pixels of each pixel-tile family, each image, each 32-channel
    block, each output parity, and each (image, pixel tile) of the map's family.  Depends on the shape alone."""
    ys, xs = torch.arange(h)[:, None].expand(h, w), torch.arange(w)[None, :].expand(h, w)
    full = lambda m2: m2[None, None].expand(n, c, h, w).clone()
    groups = []
    ring = (ys == 0) | (ys == h - 1) | (xs == 0) | (xs == w - 1)
    groups.append([("ring", full(ring)), ("interior", full(~ring))])
    for th, tw in PIXEL_TILES:
        if th <= h and tw <= w:
            edge = (ys % th == 0) | (ys % th == th - 1) | (xs % tw == 0) | (xs % tw == tw - 1)
            groups.append([(f"edge_{th}x{tw}", full(edge))])
    img = []
    for i in range(n):
        m = torch.zeros((n, c, h, w), dtype=torch.bool)
        m[i] = True
        img.append((f"image_{i}", m))
    groups.append(img)
    blk = []
    for j in range(0, c, 32):
        m = torch.zeros((n, c, h, w), dtype=torch.bool)
        m[:, j:j + 32] = True
        blk.append((f"channels_{j}", m))
    groups.append(blk)
    groups.append([(f"parity_{a}{b}", full((ys % 2 == a) & (xs % 2 == b))) for a in (0, 1) for b in (0, 1)])
    th, tw = tile_family(h, w)
    tiles = []
    for i in range(n):
        for ty in range(0, h, th):
            for tx in range(0, w, tw):
                m = torch.zeros((n, c, h, w), dtype=torch.bool)
                m[i, :, ty:ty + th, tx:tx + tw] = True
                tiles.append((f"tile_{i}_{ty}_{tx}", m))
    groups.append(tiles)
    out = {}
    for g in groups:
        for nm, m in _merged(g, min_count):
            out[nm] = m
    return out


def class_ratios(out, ref, cls):
    """{class: (relative error of `out` against `ref` inside the class) / (the whole tensor's)}"""
    d2, r2 = (out.double() - ref.double()) ** 2, ref.double() ** 2
    whole = math.sqrt(float(d2.sum()) / float(r2.sum()))
    return {nm: math.sqrt(float(d2[m].sum()) / max(float(r2[m].sum()), 1e-300)) / max(whole, 1e-300) for nm, m in cls.items()}


def check_accurate(out, ref, cls, bar):
    """4.2: -> (failures, rel_l2).  Whole tensor below `bar`, and no class above twice the whole tensor's figure (rounding error per output grows
    with the number of taps no faster than the signal: border classes can only sit lower, so only the upper bound is asserted)."""
    e = rel_l2(out, ref)
    fails = [] if e < bar else [f"rel_l2 {e:.3e} >= {bar:.1e}"]
    if not torch.isfinite(out).all():
        fails.append("not finite")
    fails += [f"class {nm}: {r:.3f} x the whole tensor's error" for nm, r in class_ratios(out, ref, cls).items() if not r <= 2.0]
    return fails, e


def check_reduced(out, exact, emul, cls):
    """4.3: -> (failures, (E, rel_l2(out, exact), rel_l2(out, emul))), E = rel_l2(emul, exact).  The error is the operand rounding the emulation
    restates: as large as E, explained by the emulation, and homogeneous over the classes."""
    E, e_exact, e_emul = rel_l2(emul, exact), rel_l2(out, exact), rel_l2(out, emul)
    fails = []
    if not torch.isfinite(out).all():
        fails.append("not finite")
    if not RATIO[0] * E <= e_exact <= RATIO[1] * E:
        fails.append(f"rel_l2 vs exact {e_exact:.3e} outside [{RATIO[0]}, {RATIO[1]}] x E = {E:.3e}")
    if not e_emul <= E / 2:
        fails.append(f"rel_l2 vs emulation {e_emul:.3e} > E / 2 = {E / 2:.3e}")
    fails += [f"class {nm}: ratio {r:.3f} outside {list(RATIO)}" for nm, r in class_ratios(out, exact, cls).items() if not RATIO[0] <= r <= RATIO[1]]
    return fails, (E, e_exact, e_emul)


# ------------------------------------------------------------------------------------------------ the ResBlock cases of test_gpu_conv_modes.py

# form -> (n, c0, c1, cout, h, w, up0): the smallest shapes for which the engine plans each form (tests/test_gpu_conv_forms.py, test_gpu_upconv.py)
BLOCK_CASES = {
    "split_in_launch": (1, 256, 0, 256, 16, 16, False),
    "split_reduce": (32, 128, 0, 128, 4, 8, False),
    "four_tap_32x32": (5, 64, 32, 128, 32, 32, True),
    "four_tap_8x16": (5, 96, 32, 64, 8, 16, True),
    "single_launch_12x20": (6, 64, 32, 128, 12, 20, True),
}
FOUR_TAP = ("four_tap_32x32", "four_tap_8x16")  # the two-launch form runs here (ops.set_upconv_split(2)); 12x20 is ragged: the single launch stays
REDUCED = ("f16", "bf16")
_BLOCK = {}
_BLOCK_EMUL = {}


def block_case(name):
    """(x0, x1, emb, P, exact fp64 reference, classes) of a ResBlock case: computed once, shared, never modified"""
    if name not in _BLOCK:
        n, c0, c1, cout, h, w, up0 = BLOCK_CASES[name]
        gen = torch.Generator().manual_seed(1000 * h + w + c0 + n)
        x0 = torch.randn((n, c0, h >> up0, w >> up0), generator=gen) * 1.5 - 0.5  # (different offset and scale on the two sources)
        x1 = torch.randn((n, c1, h, w), generator=gen) * 2 + 1 if c1 else None
        emb = torch.randn((n, 512), generator=gen)
        P = synth.synth_state_dict(res_manifest(c0 + c1, cout), 5)
        ref = res_block64(P, x0, emb, x1, up0)
        _BLOCK[name] = (x0, x1, emb, P, ref, classes(n, cout, h, w))
    return _BLOCK[name]


def block_emulation(name, mode, two_launch):
    """the fp64 block with the operands rounded as `mode` rounds them (two_launch: as the 4-tap form rounds them)"""
    key = (name, mode, bool(two_launch))
    if key not in _BLOCK_EMUL:
        x0, x1, emb, P, _, _ = block_case(name)
        _BLOCK_EMUL[key] = res_block64(P, x0, emb, x1, BLOCK_CASES[name][6], mode_hook(mode), two_launch)
    return _BLOCK_EMUL[key]


# ------------------------------------------------------------------------------------------------ corruptions (tests/test_quant_ref_cpu.py)

def corruptions(out, a, wt, tile):
    """{name: corrupted copy of `out`}: what five addressing bugs of the conv that produced `out` from the operands (a, wt [Cout, Cin, 3, 3]) would
    leave.  `out` may carry further terms (bias, residual): the corruptions change the conv's contribution alone.  tile = (th, tw)."""
    n, cout, h, w = out.shape
    th, tw = tile
    cin = a.shape[1]
    assert w > tw and n >= 2 and cin >= 32 and cout >= 18
    a, wt = a.double(), wt.double()
    res = {}
    # one tap column (the left halo column) dropped on the right-hand edge tiles of one image
    x0 = (w - 1) // tw * tw
    wcol = torch.zeros_like(wt)
    wcol[:, :, :, 0] = wt[:, :, :, 0]
    c = out.clone()
    c[1, :, :, x0] -= F.conv2d(a[1:2], wcol, padding=1)[0, :, :, x0].to(out.dtype)
    res["tap_column_dropped"] = c
    # two channels swapped inside one 32-block
    c = out.clone()
    c[:, [3, 17]] = out[:, [17, 3]]
    res["channels_swapped"] = c
    # the last image (of a half-filled multi-image tile) zeroed
    c = out.clone()
    c[n - 1] = 0
    res["last_image_zeroed"] = c
    # one K chunk of 32 channels dropped for one pixel tile
    c = out.clone()
    c[0, :, :th, :tw] -= F.conv2d(a[0:1, cin - 32:], wt[:, cin - 32:], padding=1)[0, :, :th, :tw].to(out.dtype)
    res["k_chunk_dropped"] = c
    # one output parity shifted by one stored pixel
    c = out.clone()
    c[:, :, 0::2, 1::2] = torch.roll(out[:, :, 0::2, 1::2], 1, dims=3)
    res["parity_shifted"] = c
    return res

"""The in_layers conv of a decoder ResBlock over cat(nearest_x2(x0), x1) as two launches (engine.hip plan_upconv_split):

    conv3x3(cat(up(a0), a1)) = PS(conv2x2'(a0)) + conv3x3(a1),        a = SiLU(GroupNorm(x)) with the block's tables

launch A = conv_split2_kernel<4, ...> on the STORED x0 (four parity 2x2 convs, pixel-shuffled into h1), launch B = the ordinary 3x3 conv on x1
with bias, emb, res = out = h1.  ops.set_upconv_split: 0 = never, 1 = by the measured rule, 2 = wherever the form applies.

Every case asserts through the library profiler which instantiation ran.  Tolerances are those of the tests of the single-launch form: OP_TOL
= 1e-5 against the CPU reference (tests/test_gpu_ops.py), 2e-5 for f16mx against the exact-fp32 run of the same op (tests/test_gpu_f16mx.py),
conftest.NET_TOL on a whole network.
"""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import NET_TOL, rel_l2
from drmnet_amd import synth
from oracle import unet as ou

OP_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def res_manifest(cin, cout):
    m = [("in_layers.0.weight", (cin,)), ("in_layers.0.bias", (cin,)), ("in_layers.2.weight", (cout, cin, 3, 3)), ("in_layers.2.bias", (cout,)),
         ("emb_layers.1.weight", (cout, 512)), ("emb_layers.1.bias", (cout,)), ("out_layers.0.weight", (cout,)), ("out_layers.0.bias", (cout,)),
         ("out_layers.3.weight", (cout, cout, 3, 3)), ("out_layers.3.bias", (cout,))]
    if cin != cout:
        m += [("skip_connection.weight", (cout, cin, 1, 1)), ("skip_connection.bias", (cout,))]
    return m


def profiled(fn):
    """fn() under the library's launch profiler -> (result, {instantiation name: launches})"""
    from drmnet_amd import _lib

    L = _lib.lib()
    L.drm_profile_reset()
    L.drm_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.drm_profile_enable(0)
    K = 5
    ms, fl, by, cnt = (C.c_double * K)(), (C.c_double * K)(), (C.c_double * K)(), (C.c_int64 * K)()
    L.drm_profile_collect(ms, fl, by, cnt)
    need = L.drm_profile_variants(None, 0)
    buf = C.create_string_buffer(int(need) + 16)
    L.drm_profile_variants(buf, len(buf))
    names = {}
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        names[f[0]] = int(f[2])
    L.drm_profile_reset()
    return out, names


def four_tap(names):
    """(TH, TW, BM, BN) of every conv_split2_kernel<4, ...> instantiation that ran"""
    tiles = set()
    for nm in names:
        m = re.match(r"void drm::conv_split2_kernel<4, (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), ", nm)
        if m:
            th, tw, wm, wn, mt, nt = (int(v) for v in m.groups())
            tiles.add((th, tw, wm * mt * 32, wn * nt * 32))
    return tiles


_CASES = {}


def case(n, c0, c1, cout, h, w):
    """inputs, parameters and the CPU reference of one shape (computed once, shared by the tests, never modified)"""
    key = (n, c0, c1, cout, h, w)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * h + w + c0 + n)
        x0 = torch.randn((n, c0, h // 2, w // 2), generator=gen) * 1.5 - 0.5  # (different offset and scale on the two sources)
        x1 = torch.randn((n, c1, h, w), generator=gen) * 2 + 1
        emb = torch.randn((n, 512), generator=gen)
        P = synth.synth_state_dict(res_manifest(c0 + c1, cout), 5)  # (random, asymmetric 3x3 kernels)
        xin = torch.cat([F.interpolate(x0, scale_factor=2, mode="nearest"), x1], dim=1)
        ref = ou.res_block({"rb." + k: v for k, v in P.items()}, ou.Res("rb", c0 + c1, cout), xin, emb)
        _CASES[key] = (x0, x1, emb, P, ref)
    return _CASES[key]


def run_op(dev, n, c0, c1, cout, h, w, precision, mode):
    from drmnet_amd import ops

    x0, x1, emb, P, _ = case(n, c0, c1, cout, h, w)
    Pd = [p.to(dev) for p in P.values()]
    try:
        ops.set_precision(precision)
        ops.set_upconv_split(mode)
        out, names = profiled(lambda: ops.resblock(Pd, x0.to(dev), emb.to(dev), x1.to(dev), up0=True).cpu())
    finally:
        ops.set_precision("fp32")
        ops.set_upconv_split(1)
    return out, names


# (n, C0, C1, Cout, full-resolution H, W) -> the (TH, TW, BM, BN) launch A must run on, per precision class.  Groups of 3 (96 channels) and 6
# (192 channels) straddle the concat boundary.  Batches are > 4: at N <= 4 the consumer finalises its GroupNorm tables itself and the single
# launch stays (the fallback test below).
SHAPES = [
    # 256x128 tiles on 16x16 pixels: A 11 * 1024 / 256 x 4 = 176 tiles, B 176: exactly the wide-tile threshold
    ((11, 64, 32, 128, 64, 64), {"fp32": (16, 16, 256, 128), "split": (16, 16, 256, 128)}),
    # 256x192 tiles in the split modes (512 workgroups each); exact fp32 has no 192-wide form: 256x128
    ((16, 64, 32, 384, 64, 64), {"fp32": (16, 16, 256, 128), "split": (16, 16, 256, 192)}),
    # narrow 128-row tiles (8x16 pixels x 32 channels), odd batch
    ((5, 64, 32, 128, 32, 32), {"fp32": (8, 16, 128, 32), "split": (8, 16, 128, 32)}),
    # non-square 8x32 stored map (Cout != C0 + C1: a ResBlock with equal channel counts has an identity skip, which the op does not take on a
    # concatenated input)
    ((6, 128, 64, 256, 16, 64), {"fp32": (8, 16, 128, 32), "split": (8, 16, 128, 32)}),
    # 4x8 family: four images per tile, odd batch (the last tile is half empty)
    ((5, 96, 32, 64, 8, 16), {"fp32": (4, 8, 128, 32), "split": (4, 8, 128, 32)}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("shape,tiles", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_two_launch_form_vs_cpu_reference(dev, shape, tiles, precision):
    out, names = run_op(dev, *shape, precision, 2)
    ref = case(*shape)[4]
    e = rel_l2(out, ref)
    ran = four_tap(names)
    print(f"upconv split {shape} {precision}: rel_l2 {e:.2e}, 4-tap tiles {sorted(ran)}")
    assert ran == {tiles["fp32" if precision == "fp32" else "split"]}, names
    assert e < OP_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape,tiles", SHAPES[:2], ids=[str(s[0]) for s in SHAPES[:2]])
def test_two_launch_form_f16mx_vs_exact_fp32(dev, shape, tiles):
    ref, names32 = run_op(dev, *shape, "fp32", 2)
    out, names = run_op(dev, *shape, "f16mx", 2)
    e = rel_l2(out, ref)
    ran = four_tap(names)
    print(f"upconv split {shape} f16mx vs fp32: {e:.2e}, 4-tap tiles {sorted(ran)}")
    assert four_tap(names32) and ran == {tiles["split"]}, names
    assert any(re.match(r"void drm::conv_split2_kernel<4, (\d+, ){8}2, ", nm) for nm in names), names  # (TERMS = 2: the block-scaled form)
    assert torch.isfinite(out).all() and e < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode,why", [
    ((2, 64, 32, 128, 64, 64), 2, "N <= 4: the consumer finalises the GroupNorm tables in its prologue"),
    ((6, 64, 32, 128, 12, 20), 2, "ragged map"),
    ((3, 768, 640, 768, 8, 8), 2, "split-K"),
    ((11, 64, 32, 128, 64, 64), 0, "mode 0"),
], ids=["gn_fold", "ragged", "split_k", "mode0"])
def test_fallback_to_the_single_launch(dev, shape, mode, why):
    out, names = run_op(dev, *shape, "f16x3", mode)
    e = rel_l2(out, case(*shape)[4])
    print(f"single launch ({why}) {shape}: rel_l2 {e:.2e}")
    assert not four_tap(names), names
    assert any(nm.startswith("void drm::conv_split2_kernel<9, ") for nm in names), names
    assert e < OP_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "f16mx"])
def test_illnet_forward_both_forms_agree(dev, precision):
    """Both forms approximate the same function: a wiring error (tables, weight slices, parity order) shows as O(1)."""
    from drmnet_amd import ops
    from drmnet_amd.unet import UNetModel

    n, h, w = 6, 32, 64
    m = UNetModel(**ou.ILLNET_CFG)
    synth.load_synth(m, 11)
    m = m.to(dev).set_precision(precision)
    x = synth.synth_refmaps(n, h, w, synth.SEED_INPUT)
    gen = torch.Generator().manual_seed(synth.SEED_INPUT + 1)
    xc = torch.cat([x + 0.025 * torch.randn(x.shape, generator=gen), x], dim=1).contiguous().to(dev)
    t_emb = torch.randn((n, 128), generator=gen).to(dev)
    try:
        ops.set_upconv_split(0)
        ref, names0 = profiled(lambda: m(xc, t_emb=t_emb).cpu())
        ops.set_upconv_split(2)
        out, names2 = profiled(lambda: m(xc, t_emb=t_emb).cpu())
    finally:
        ops.set_upconv_split(1)
    e = rel_l2(out, ref)
    print(f"IllNet {n}x{h}x{w} {precision}: two-launch form vs single launch {e:.2e}; 4-tap tiles {sorted(four_tap(names2))}")
    assert not four_tap(names0) and four_tap(names2), (names0, names2)
    assert torch.isfinite(out).all() and e < NET_TOL[precision]
    del m
    torch.cuda.empty_cache()


def test_weight_fold_table_on_the_cpu():
    """parity -> tap groups (ops.UPCONV_TAP_GROUPS, the table csrc/conv_split.hip fold_upconv_weight_kernel implements): the folded 2x2 kernels on
    the stored map, pixel-shuffled, plus the 3x3 conv on the skip slice equal conv2d(cat(nearest_x2(x0), x1)) in fp64"""
    from drmnet_amd import ops

    gen = torch.Generator().manual_seed(3)
    n, c0, c1, cout, h, w = 3, 8, 4, 6, 6, 10  # (stored map 3 x 5: odd sizes)
    x0 = torch.randn((n, c0, h // 2, w // 2), generator=gen, dtype=torch.float64)
    x1 = torch.randn((n, c1, h, w), generator=gen, dtype=torch.float64)
    wt = torch.randn((cout, c0 + c1, 3, 3), generator=gen, dtype=torch.float64)
    ref = F.conv2d(torch.cat([F.interpolate(x0, scale_factor=2, mode="nearest"), x1], dim=1), wt, padding=1)
    wa, wb = ops.fold_upconv_weight(wt, c0)
    assert tuple(wa.shape) == (4 * cout, c0, 2, 2) and tuple(wb.shape) == (cout, c1, 3, 3)
    out = F.conv2d(x1, wb, padding=1)
    xp = F.pad(x0, (1, 1, 1, 1))
    for a in (0, 1):
        for b in (0, 1):
            p = 2 * a + b
            # out[2i + a, 2j + b] = sum W'[dy, dx] x0[i + a - 1 + dy, j + b - 1 + dx]: a valid 2x2 correlation of the padded map from (a, b) on
            y = F.conv2d(xp[:, :, a:a + h // 2 + 1, b:b + w // 2 + 1], wa[p * cout:(p + 1) * cout])
            out[:, :, a::2, b::2] += y
    assert rel_l2(out, ref) < 1e-14
    # the table itself: every 3x3 tap lands in exactly one window position per parity
    for a in (0, 1):
        assert sorted(ops.UPCONV_TAP_GROUPS[a][0] + ops.UPCONV_TAP_GROUPS[a][1]) == [0, 1, 2]
    assert ops.UPCONV_TAP_GROUPS[0][0] == (0,) and ops.UPCONV_TAP_GROUPS[1][1] == (2,)

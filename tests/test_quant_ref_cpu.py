"""The references and criteria of tests/test_gpu_conv_exact.py and tests/test_gpu_conv_modes.py, checked on the CPU alone (tests/quant_ref.py):

* the fp64 restatement of the ResBlock equals oracle.unet.res_block, in its single-launch and in its two-launch (4-tap) form;
* every exact case keeps its bit budget, and an fp32 conv of it equals the fp64 one bit for bit -- the reference itself meets the exactness premise;
* in every reduced-mode block case the emulation's error against the exact reference is spatially homogeneous: every class ratio inside [0.8, 1.25]
  (measured [0.93, 1.08] on GroupNorm + SiLU + 3x3 conv at five shapes; the margin covers classes down to 512 elements);
* the criteria see what they are for: five addressing bugs, applied to a reference output, are rejected by the exact and by the emulated check.
"""
import pytest
import torch
import torch.nn.functional as F

import quant_ref as q
from conftest import rel_l2
from oracle import unet as ou


@pytest.mark.parametrize("name", ["split_reduce", "four_tap_8x16"])
def test_restated_block_equals_the_oracle(name):
    n, c0, c1, cout, h, w, up0 = q.BLOCK_CASES[name]
    x0, x1, emb, P, ref, _ = q.block_case(name)
    xin = torch.cat([F.interpolate(x0, scale_factor=2, mode="nearest") if up0 else x0] + ([x1] if x1 is not None else []), dim=1)
    with ou.working_dtype(torch.float64):
        want = ou.res_block({"rb." + k: v.double() for k, v in P.items()}, ou.Res("rb", c0 + c1, cout), xin.double(), emb.double())
    assert ref.dtype == torch.float64 and rel_l2(ref, want) < 1e-12
    if up0:  # the two-launch form states the same function
        assert rel_l2(q.res_block64(P, x0, emb, x1, up0, q.identity, two_launch=True), want) < 1e-12


@pytest.mark.parametrize("name", list(q.EXACT_CASES))
def test_exact_case_reference_is_exact_in_fp32(name):
    n, cin, cout, h, w, k, extras = q.EXACT_CASES[name]
    assert q.exact_case_bits(name) <= 24
    x, wt, bias, emb, res, ref = q.exact_case(name)
    assert torch.equal(ref.float().double(), ref), "the fp64 reference is no fp32 number"
    out = F.conv2d(x, wt, None, padding=k // 2)
    if bias is not None:  # the epilogue's order (csrc/conv_epilogue.h epi_value)
        out = out + bias[None, :, None, None] + emb[:, :, None, None] + res
    assert out.dtype == torch.float32 and torch.equal(out, ref.float()), q.first_mismatch(out, ref)


@pytest.mark.parametrize("i,o,n", [(i, o, n) for n, i, o, _ in q.LINEAR_CASES])
def test_exact_linear_reference_is_exact_in_fp32(i, o, n):
    x, wt, b, ref = q.linear_case(n, i, o)
    assert torch.equal(F.linear(x, wt, b), ref.float()) and torch.equal(ref.float().double(), ref)


def test_quantise_matches_the_number_formats():
    gen = torch.Generator().manual_seed(7)
    t = torch.randn((4096,), generator=gen) * 3
    assert torch.equal(q.quantise(t, "f16", "act"), t.half().double())  # (in fp16's normal range the range-free rounding IS the cast)
    big = t * 2.0 ** 20  # beyond fp16: the guard's power of two moves it into range first
    assert torch.equal(q.quantise(big, "f16", "act"), t.half().double() * 2.0 ** 20)
    w = t * 0.01
    k = 2.0 ** (14 - torch.frexp(w.abs().max())[1].item())
    assert 8192 <= float(w.abs().max()) * k < 16384 and torch.equal(q.quantise(w, "f16", "w"), (w * k).half().double() / k)
    assert torch.equal(q.quantise(t, "bf16", "w"), t.bfloat16().double()) and torch.equal(q.quantise(t, "f16x3", "act"), t.double())
    d = q.dyadic((1000,), q.X_STEP, q.X_KMAX, gen)
    for mode in ("f16", "bf16"):  # dyadic operands are fp16 and bf16 numbers
        assert torch.equal(q.quantise(d, mode, "act"), d.double()) and torch.equal(q.quantise(d * q.W_STEP / q.X_STEP, mode, "w"), d.double() / 4)


def test_classes_are_fixed_by_the_shape_and_large_enough():
    for n, c0, c1, cout, h, w, up0 in q.BLOCK_CASES.values():
        cls = q.classes(n, cout, h, w)
        assert {"ring", "image_0", "channels_0", "parity_00"} <= {nm.split("+")[0] for nm in cls}
        assert all(int(m.sum()) >= q.MIN_CLASS for m in cls.values()), {nm: int(m.sum()) for nm, m in cls.items()}
    small = q.classes(1, 32, 2, 4)  # 256 elements: everything merges into classes that exist
    assert small and all(int(m.sum()) > 0 for m in small.values())
    assert q.tile_family(12, 20) == (4, 4) and q.tile_family(32, 32) == (16, 16) and q.tile_family(4, 8) == (4, 8) and q.tile_family(6, 10) == (4, 4)


@pytest.mark.parametrize("mode", q.REDUCED)
@pytest.mark.parametrize("name", list(q.BLOCK_CASES))
def test_emulation_error_is_homogeneous_over_the_classes(name, mode):
    x0, x1, emb, P, ref, cls = q.block_case(name)
    emul = q.block_emulation(name, mode, name in q.FOUR_TAP)
    ratios = q.class_ratios(emul, ref, cls)
    lo, hi = min(ratios, key=ratios.get), max(ratios, key=ratios.get)
    print(f"{name} {mode}: E = {rel_l2(emul, ref):.3e}, {len(cls)} classes, ratios {ratios[lo]:.3f} ({lo}) .. {ratios[hi]:.3f} ({hi})")
    assert all(q.RATIO[0] <= r <= q.RATIO[1] for r in ratios.values()), {nm: round(r, 3) for nm, r in ratios.items() if not q.RATIO[0] <= r <= q.RATIO[1]}
    # the emulation itself, as fp32, passes the reduced-mode criteria
    fails, _ = q.check_reduced(emul.float(), ref, emul, cls)
    assert not fails, fails


CORRUPTIONS = ["tap_column_dropped", "channels_swapped", "last_image_zeroed", "k_chunk_dropped", "parity_shifted"]


@pytest.mark.parametrize("what", CORRUPTIONS)
def test_exact_criterion_rejects(what):
    name = "map_12x20_k3"
    n, cin, cout, h, w, k, _ = q.EXACT_CASES[name]
    x, wt, _, _, _, ref = q.exact_case(name)
    good = ref.float()
    bad = q.corruptions(good, x, wt, q.tile_family(h, w))[what]
    assert torch.equal(good, ref.float()) and not torch.equal(bad, ref.float())
    assert q.first_mismatch(good, ref) is None
    mm = q.first_mismatch(bad, ref, q.classes(n, cout, h, w))
    print(what, "->", mm)
    assert mm.count > 0 and mm.classes and bad[mm.index].item() == mm.got != mm.want == good[mm.index].item()


@pytest.fixture(scope="module")
def out_conv_operands():
    """the out_layers conv's operands of one block case, as each mode's emulation multiplies them"""
    name = "four_tap_32x32"
    x0, x1, emb, P, ref, cls = q.block_case(name)
    got = {}
    for mode in ("fp32",) + q.REDUCED:
        rec = {}

        def hook(t, kind, site, mode=mode, rec=rec):
            v = q.quantise(t, mode, kind)
            if site == "out":
                rec[kind] = v
            return v
        out = q.res_block64(P, x0, emb, x1, True, hook, two_launch=True)
        got[mode] = (out, rec["act"], rec["w"])
    return name, ref, cls, got


@pytest.mark.parametrize("what", CORRUPTIONS)
def test_mode_criteria_reject(out_conv_operands, what):
    name, ref, cls, got = out_conv_operands
    n, c0, c1, cout, h, w, up0 = q.BLOCK_CASES[name]
    tile = q.tile_family(h, w)
    # accurate modes: an fp32 copy of the exact output passes, its corruption does not
    out, a, wt = got["fp32"]
    assert rel_l2(out, ref) < 1e-12
    fails, e = q.check_accurate(out.float(), ref, cls, 1e-5)
    assert not fails, fails
    fails, e = q.check_accurate(q.corruptions(out.float(), a, wt, tile)[what], ref, cls, 1e-5)
    print(f"{what} accurate: rel_l2 {e:.2e}: {fails[:3]}")
    assert fails
    # reduced modes: the emulation stands in for the GPU's output
    for mode in q.REDUCED:
        out, a, wt = got[mode]
        fails, _ = q.check_reduced(out.float(), ref, out, cls)
        assert not fails, fails
        fails, figs = q.check_reduced(q.corruptions(out.float(), a, wt, tile)[what], ref, out, cls)
        print(f"{what} {mode}: E {figs[0]:.2e}, vs exact {figs[1]:.2e}, vs emulation {figs[2]:.2e}: {fails[:3]}")
        assert fails

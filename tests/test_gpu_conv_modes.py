"""The engine-only forms of the conv pipeline against a reference in EVERY mode, with a statement of where the error sits (tests/quant_ref.py (b),
DESIGN.md "Exact and emulated conv checks"): split-K finished in the launch, split-K with the second-launch reduce on 128x128 tiles, the 4-tap parity
form and its single-launch fallback through ops.resblock, and the pooled epilogue through a two-level network.

Per case and mode:
  * the conv_split2_kernel instantiations that ran carry the form's flags and the mode's TERMS (library profiler);
  * fp32, f16x3, f16mx: rel-L2 against the fp64 block below the bar of tests/test_gpu_upconv.py (1e-5, f16mx 2e-5), and no class of the output
    (border ring, tile edges, images, 32-channel blocks, parities, pixel tiles) above twice the whole tensor's relative error;
  * f16, bf16: with E = rel_l2(emulation, exact), the fp64 block with its conv operands rounded as the mode rounds them (computed on the CPU):
    rel_l2(GPU, exact) in [0.8, 1.25] E, rel_l2(GPU, emulation) <= E / 2 (the emulation explains the error; the CPU measurement leaves a factor 10
    for bf16 and 3.5 for fp16), and every class ratio of (GPU - exact) in [0.8, 1.25] (tests/test_quant_ref_cpu.py: the emulation's own ratios are).
References, emulations and classes are computed once per case on the CPU and shared by the modes.
"""
import pytest
import torch

import quant_ref as q
from conftest import NET_TOL, rel_l2
from drmnet_amd import synth
from oracle import unet as ou
from test_gpu_upconv import profiled

MODES = ["fp32", "f16x3", "f16mx", "f16", "bf16"]
PREFIX = "void drm::conv_split2_kernel<"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def instantiations(names):
    """(TAPS, TH, TW, WM, WN, MT, NT, ring, taps per step, TERMS, ragged, in-launch split-K, pooled) of every conv_split2_kernel that ran"""
    out = []
    for nm in names:
        if nm.startswith(PREFIX):
            f = nm[len(PREFIX):].rstrip(">").split(", ")
            out.append(tuple(int(v) for v in f[:10]) + tuple(v == "true" for v in f[10:13]))
    return out


def terms_of(mode, taps):
    """the 3x3 convs of a ResBlock (and the 4-tap form) are the f16mx sites; its 1x1 skip conv runs f16x3 there"""
    return 3 if (mode == "f16mx" and taps == 1) else q.TERMS[mode]


# form -> what the instantiations of its 3x3 / 4-tap launches must show
def _split_in_launch(ins):
    return any(i[0] == 9 and i[1:7] == (8, 16, 4, 1, 1, 1) and i[10:] == (False, True, False) for i in ins)  # 128x32 tiles, SK


def _split_reduce(ins):
    return any(i[0] == 9 and i[1:7] == (4, 8, 2, 2, 2, 2) and i[10:] == (False, False, False) for i in ins)  # 128x128 tiles on 4x8 pixels


def _four_tap(ins):
    return any(i[0] == 4 and i[10:] == (False, False, False) for i in ins) and any(i[0] == 9 for i in ins)


def _single_launch(ins):
    return not any(i[0] == 4 for i in ins) and any(i[0] == 9 and i[10:] == (False, False, False) for i in ins)


FORM = {"split_in_launch": _split_in_launch, "split_reduce": _split_reduce, "four_tap_32x32": _four_tap, "four_tap_8x16": _four_tap,
        "single_launch_12x20": _single_launch}


def run_block(dev, name, mode):
    from drmnet_amd import ops

    x0, x1, emb, P, _, _ = q.block_case(name)
    Pd = [p.to(dev) for p in P.values()]
    try:
        ops.set_precision(mode)
        ops.set_upconv_split(2)  # (wherever the form applies: the 12x20 case keeps the single launch by itself, its stored map is ragged)
        out, names = profiled(lambda: ops.resblock(Pd, x0.to(dev), emb.to(dev), None if x1 is None else x1.to(dev), up0=q.BLOCK_CASES[name][6]).cpu())
    finally:
        ops.set_precision("fp32")
        ops.set_upconv_split(1)
    return out, names


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(q.BLOCK_CASES))
def test_block_forms_in_every_mode(dev, name, mode):
    x0, x1, emb, P, ref, cls = q.block_case(name)  # (the classes are fixed here, before the GPU runs)
    out, names = run_block(dev, name, mode)
    ins = instantiations(names)
    # 4.1 the form's flags and the mode's TERMS
    assert FORM[name](ins), names
    assert ins and all(i[9] == terms_of(mode, i[0]) for i in ins), names
    two_launch = any(i[0] == 4 for i in ins)
    assert two_launch == (name in q.FOUR_TAP)
    if mode in q.REDUCED:
        # 4.3 the error is the operand rounding the emulation restates, everywhere
        emul = q.block_emulation(name, mode, two_launch)
        fails, (E, e_exact, e_emul) = q.check_reduced(out, ref, emul, cls)
        ratios = q.class_ratios(out, ref, cls)
        print(f"{name} {mode}: E = {E:.3e}, GPU vs exact {e_exact:.3e} ({e_exact / E:.3f} E), GPU vs emulation {e_emul:.3e} (E / {E / e_emul:.1f}), "
              f"class ratios {min(ratios.values()):.3f} .. {max(ratios.values()):.3f}")
    else:
        # 4.2 the bar of tests/test_gpu_upconv.py, and no class above twice the whole tensor
        fails, e = q.check_accurate(out, ref, cls, 2e-5 if mode == "f16mx" else 1e-5)
        ratios = q.class_ratios(out, ref, cls)
        print(f"{name} {mode}: rel_l2 {e:.3e}, largest class ratio {max(ratios.values()):.3f} ({max(ratios, key=ratios.get)})")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 4.4 the pooled epilogue

POOL_CFG = dict(image_size=64, in_channels=6, out_channels=3, model_channels=128, attention_resolutions=[], num_res_blocks=1, dropout=0.0,
                channel_mult=[1, 2], num_heads=1, resblock_updown=False, conv_resample=False)
POOL_SHAPE = (11, 64, 64)  # the one case that cannot shrink: the pooled form needs 176 workgroups of 256x128 (tests/test_gpu_conv_forms.py)


@pytest.fixture(scope="module")
def pooled_case(dev):
    """the two-level network of tests/test_gpu_conv_forms.py, its inputs and its fp64 oracle output: built once, shared by the modes"""
    from drmnet_amd.unet import UNetModel

    n, h, w = POOL_SHAPE
    gen = torch.Generator().manual_seed(n + h + w)
    x, t_emb = torch.randn((n, 6, h, w), generator=gen), torch.randn((n, 128), generator=gen)
    P = synth.synth_state_dict(ou.param_manifest(POOL_CFG, "unet"), 11)
    with ou.working_dtype(torch.float64):
        ref = ou.unet_forward({k: v.double() for k, v in P.items()}, ou.build_topology(POOL_CFG, "unet"), x.double(), t_emb=t_emb.double())
    m = UNetModel(**POOL_CFG)
    synth.load_synth(m, 11)
    m = m.to(dev)
    yield m, x.to(dev), t_emb.to(dev), ref
    del m
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16mx", "f16", "bf16"])  # (the pooled form is a split-mode form: s2_form, terms != 0)
def test_pooled_epilogue_in_every_mode(dev, pooled_case, mode):
    m, x, t_emb, ref = pooled_case
    m.set_precision(mode)
    out, names = profiled(lambda: m(x, t_emb=t_emb).cpu())
    pooled = [i for i in instantiations(names) if i[12]]
    e = rel_l2(out, ref)
    print(f"pooled {POOL_SHAPE} {mode}: rel_l2 vs the fp64 oracle {e:.3e}; pooled instantiations {pooled}")
    assert pooled == [(9, 16, 16, 4, 2, 2, 2, 2, 3, q.TERMS[mode], False, False, True)], names
    assert torch.isfinite(out).all() and e < NET_TOL[mode]

"""AttentionBlock with proj_out folded into the v rows of the qkv projection (csrc/conv_split.hip fold_attn_params_kernel) and the residual add +
output statistics in the last kernel of the attention core (csrc/attn.hip, attn_flash.hip): out = x + sum_s P[t,s] ((Wp Wv) xn_s + Wp bv + bp).

The fold is exact in real arithmetic (every softmax row sums to one), so the block is held to what the unfolded one was held to: the CPU oracle's
attention_block / the reference goldens at the tolerances the existing attention tests use per arithmetic mode -- 1e-5 on single ops in fp32 and
f16x3 (test_gpu_ops.OP_TOL, test_gpu_split.OP_TOL), 2e-5 for f16x3 on the long-sequence 384 @ 32x32 block and for f16mx, 5e-3 for f16, 3e-2 for
bf16 (test_gpu_attn_flash.TOL); whole networks at conftest.NET_TOL."""
import pytest
import torch

from conftest import NET_TOL, gold, rel_l2
from drmnet_amd import _lib, ops, synth
from oracle import unet as ou
from test_gpu_nets import build
from test_gpu_ops import OP_TOL, attn_manifest, block_inputs

pytestmark = pytest.mark.gpu
MODES = ["fp32", "f16x3", "f16mx", "f16", "bf16"]
BLOCKS = [(512, 16, 16), (384, 32, 32), (768, 4, 8)]


def op_tol(mode, ch, h, w):
    if mode == "fp32":
        return OP_TOL
    if mode == "f16x3":
        return 2e-5 if (ch, h * w) == (384, 1024) else OP_TOL  # (the long-sequence block: test_gpu_attn_flash.TOL)
    return {"f16mx": 2e-5, "f16": 5e-3, "bf16": 3e-2}[mode]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def run(P, x, mode, dev):
    try:
        ops.set_precision(mode)
        return ops.attention_block([p.to(dev) for p in P.values()], x.to(dev)).cpu()
    finally:
        ops.set_precision("fp32")


def oracle(P, ch, x):
    return ou.attention_block({"ab." + k: v for k, v in P.items()}, ou.Attn("ab", ch), x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ch,h,w", BLOCKS)
def test_folded_block_vs_reference_golden(dev, ch, h, w, mode):
    gd = gold(f"attnblock_{ch}_{h}x{w}")
    x, _ = block_inputs(ch, ch, h, w, int(gd["n"]))
    P = synth.synth_state_dict(attn_manifest(ch), int(gd["seed"]))
    err = rel_l2(run(P, x, mode, dev), gd["out"])
    print(f"folded attention {ch}@{h}x{w} ({mode}): rel-L2 vs the reference {err:.2e}")
    assert err < op_tol(mode, ch, h, w)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ch,h,w", BLOCKS)
def test_large_biases(dev, ch, h, w, mode):
    """qkv.bias and proj_out.bias x 30: the q . bk term that a softmax over keys drops and the folded Wp bv + bp then dominate (the attention
    branch is several times the norm of x)."""
    gd = gold(f"attnblock_{ch}_{h}x{w}")
    x, _ = block_inputs(ch, ch, h, w, int(gd["n"]))
    P = synth.synth_state_dict(attn_manifest(ch), int(gd["seed"]))
    P["qkv.bias"] = P["qkv.bias"] * 30
    P["proj_out.bias"] = P["proj_out.bias"] * 30
    ref = oracle(P, ch, x)
    out = run(P, x, mode, dev)
    err = rel_l2(out, ref)
    print(f"folded attention {ch}@{h}x{w} ({mode}), biases x 30: rel-L2 vs the oracle {err:.2e}, |branch| / |x| = {float((ref - x).norm() / x.norm()):.2f}")
    assert torch.isfinite(out).all() and err < op_tol(mode, ch, h, w)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ch,h,w,n", [(64, 4, 4, 3), (128, 8, 4, 5), (256, 16, 32, 3), (384, 32, 32, 3)])
def test_distinct_rows_and_bounds_sizes(dev, ch, h, w, n, mode):
    """N > 1 with rows of different scale and offset (per-image factors, per-image residual and statistics rows); T = 16 is below the 32-wide key
    chunk of the short-sequence P v kernel (exact-fp32 P v in the split modes), T = 32 is exactly one; 16x32 x 3 runs on the conv pipeline."""
    gen = torch.Generator().manual_seed(17 * ch + h + n)
    x = torch.randn((n, ch, h, w), generator=gen)
    x[0] = x[0] * 3.0 + 0.5
    x[n - 1] = x[n - 1] * 0.25 - 1.0
    P = synth.synth_state_dict(attn_manifest(ch), 31)
    ref = oracle(P, ch, x)
    out = run(P, x, mode, dev)
    err = rel_l2(out, ref)
    print(f"folded attention {ch}@{h}x{w} N={n} ({mode}): rel-L2 vs the oracle {err:.2e}")
    assert torch.isfinite(out).all() and err < op_tol(mode, ch, h, w)
    # a row of the batch is that image alone: no cross-image state (a leak would be an O(1) error).  N = 1 may take another core (16x32: the
    # short-sequence form below N * T = 1024) and another tile family in the qkv conv, so the two agree to the mode's own accuracy, not bit for bit.
    one = run(P, x[1:2].contiguous(), mode, dev)
    assert rel_l2(one[0], out[1]) < op_tol(mode, ch, h, w)


# a U-Net whose attention blocks are each followed by a ResBlock that normalises their output: 16x32 (T = 512, conv-pipeline core at N * T > 1024),
# 8x16 (T = 128, short-sequence core)
ATTN_RES_CFG = dict(image_size=32, in_channels=6, out_channels=3, model_channels=128, attention_resolutions=[1, 2], num_res_blocks=1,
                    channel_mult=[1, 2], num_heads=1, resblock_updown=False, conv_resample=False)


def net_case(cfg, seed, n, h, w):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 6, h, w), generator=gen)
    t = torch.randint(0, 1000, (n,), generator=gen)
    P = synth.synth_state_dict(ou.param_manifest(cfg, "unet"), seed)
    return x, t, P, ou.unet_forward(P, ou.build_topology(cfg, "unet"), x, timesteps=t)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg,n,h,w", [(ATTN_RES_CFG, 3, 16, 32), (ATTN_RES_CFG, 1, 16, 32), (ou.TINY_UNET_CFG, 2, 16, 16)])
def test_attention_then_resblock_vs_oracle(dev, cfg, n, h, w, mode):
    """The moments the core's epilogue accumulates are what the next GroupNorm reads."""
    x, t, _, ref = net_case(cfg, 41, n, h, w)
    m = build(cfg, "unet", 41, dev).set_precision(mode)
    out = m(x.to(dev), timesteps=t.to(dev)).cpu()
    err = rel_l2(out, ref)
    print(f"attention -> resblock net mc={cfg['model_channels']} {n}x{h}x{w} ({mode}): rel-L2 vs the oracle {err:.2e}")
    assert torch.isfinite(out).all() and err < NET_TOL[mode]


@pytest.mark.parametrize("mode", ["fp32", "f16mx"])
def test_two_weight_sets_fold_separately(dev, mode):
    """Live and EMA weights are folded and packed per set: switching back and forth gives each set's own oracle result."""
    cfg = ATTN_RES_CFG
    x, t, _, ref_live = net_case(cfg, 43, 2, 16, 32)
    m = build(cfg, "unet", 43, dev).set_precision(mode)
    P_ema = synth.synth_state_dict(ou.param_manifest(cfg, "unet"), 44)
    ref_ema = ou.unet_forward(P_ema, ou.build_topology(cfg, "unet"), x, timesteps=t)
    assert rel_l2(ref_ema, ref_live) > 1e-2  # (the two sets are different networks)
    ema = [P_ema[k].to(dev) for k in m._keys]
    xd, td = x.to(dev), t.to(dev)
    for which, ref in (("live", ref_live), ("ema", ref_ema), ("live", ref_live), ("ema", ref_ema)):
        m.use_weights(which, ema if which == "ema" else None)
        err = rel_l2(m(xd, timesteps=td).cpu(), ref)
        print(f"weight set {which} ({mode}): rel-L2 vs its own oracle {err:.2e}")
        assert err < NET_TOL[mode]
    m.use_weights("live")


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f16mx"])
def test_sizing_equals_use(dev, mode):
    """A workspace of exactly drm_unet_workspace_bytes runs the forward."""
    cfg = ATTN_RES_CFG
    n, h, w = 3, 16, 32
    x, t, _, ref = net_case(cfg, 47, n, h, w)
    m = build(cfg, "unet", 47, dev).set_precision(mode)
    m.sync_weights()
    L = _lib.lib()
    need = int(L.drm_unet_workspace_bytes(m._h, n, h, w))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    xd, td = x.to(dev), t.to(dev)
    out = torch.empty((n, 3, h, w), device=dev)
    rc = L.drm_unet_forward(m._h, xd.data_ptr(), 6, None, 0, None, None, td.data_ptr(), None, out.data_ptr(), n, h, w, ws.data_ptr(), need,
                            _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0, L.drm_last_error()
    err = rel_l2(out.cpu(), ref)
    print(f"forward in exactly {need} bytes ({mode}): rel-L2 vs the oracle {err:.2e}")
    assert err < NET_TOL[mode]

"""The bytes the conv epilogues write, per form of conv_split2_kernel: value rule (scale, + bias, + emb, + residual in that order, csrc/conv_epilogue.h),
NCHW and NHWC quad stores, statistics into the next GroupNorm, split-K finishes, the parity form and the pooled tail.

A pinned case compares the SHA-256 of the output tensor's bytes with tests/golden/conv_epilogue_digests.json.  The digests were recorded by running
this file's cases (`python tests/test_gpu_conv_epilogue.py --record FILE`) against the library built from the commit BEFORE the epilogue rules were
stated once, never from the code under test.  Shapes: the smallest for which plan_conv picks each form (tests/test_gpu_conv_forms.py), with bias,
emb and residual live where the op takes them.

The block and network cases pass through fp64 atomics whose order is not fixed; the recorder ran every case twice and pinned only those whose digest
reproduced (the JSON holds null otherwise).  An unpinned case is compared with the fp64 torch reference instead, at the tolerance of the existing test
of its form (tests/test_gpu_upconv.py: 1e-5 per block, 2e-5 for f16mx; conftest.NET_TOL for the network).  Cases that fell back when the digests were
recorded: none -- all eight reproduced (FELL_BACK below).

The four block and network digests were recorded again, by the same recorder, when the epilogue's output statistics changed their arithmetic on
purpose (sums about a per-lane pivot instead of fp32 sums of x and x * x: DESIGN.md "GroupNorm checks"): the next GroupNorm's tables move in their
last bits, and with them every byte behind it.  The four conv cases, whose output no statistics feed, kept their digests from the earlier commit;
what the new statistics are held to is tests/test_gpu_groupnorm.py's elementwise bound against fp64.

pooled_net was recorded once more, the same way, when the stem's statistics took the same pivot form (DESIGN.md "Boundary-kernel checks": its
first GroupNorm reads the stem's table).  The library with the stem as it was reproduced the old digest in the same session; old and new outputs
differ by 6.6e-7 in rel-L2 and stand at 9.83e-7 and 9.80e-7 from the fp64 reference, against this case's bar of 2e-5.
"""
import hashlib
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_epilogue_digests.json")
FELL_BACK = ()  # (every case reproduced on the recording run)
NET_CFG = dict(image_size=64, in_channels=6, out_channels=3, model_channels=128, attention_resolutions=[], num_res_blocks=1, dropout=0.0,
               channel_mult=[1, 2], num_heads=1, resblock_updown=False, conv_resample=False)


def conv_inputs(n, cin, cout, h, w, k, full):
    """(x, weight, bias, emb, residual) on the CPU; `full`: every term of the value rule live"""
    gen = torch.Generator().manual_seed(n + cin + cout + h + w)
    x = torch.randn((n, cin, h, w), generator=gen)
    wt = torch.randn((cout, cin, k, k), generator=gen) * 0.05
    if not full:
        return x, wt, None, None, None
    return x, wt, torch.randn((cout,), generator=gen), torch.randn((n, cout), generator=gen), torch.randn((n, cout, h, w), generator=gen)


def conv(precision, n, cin, cout, h, w, k, full=False):
    def run(dev):
        from drmnet_amd import ops

        x, wt, b, e, r = (None if t is None else t.to(dev) for t in conv_inputs(n, cin, cout, h, w, k, full))
        ops.set_precision(precision)
        return ops.norm_act_conv(x, wt, bias=b, emb=e, residual=r)

    def ref():
        x, wt, b, e, r = (None if t is None else t.double() for t in conv_inputs(n, cin, cout, h, w, k, full))
        out = F.conv2d(x, wt, b, padding=k // 2)
        return out + e[:, :, None, None] + r if full else out

    return run, ref, {"f16x3": 1e-5, "fp32": 1e-5, "bf16": 3e-2}[precision]


def block_inputs(n, c0, c1, cout, h, w, up0):
    from drmnet_amd import synth
    from test_gpu_upconv import res_manifest

    gen = torch.Generator().manual_seed(n + c0 + cout + h + w)
    x0 = torch.randn((n, c0, h >> up0, w >> up0), generator=gen)
    x1 = torch.randn((n, c1, h, w), generator=gen) if c1 else None
    emb = torch.randn((n, 512), generator=gen)
    return x0, x1, emb, synth.synth_state_dict(res_manifest(c0 + c1, cout), 5)


def resblock(precision, n, c0, c1, cout, h, w, up0=False):
    def run(dev):
        from drmnet_amd import ops

        x0, x1, emb, P = block_inputs(n, c0, c1, cout, h, w, up0)
        ops.set_precision(precision)
        return ops.resblock([p.to(dev) for p in P.values()], x0.to(dev), emb.to(dev), None if x1 is None else x1.to(dev), up0=up0)

    def ref():
        from oracle import unet as ou

        x0, x1, emb, P = block_inputs(n, c0, c1, cout, h, w, up0)
        xin = F.interpolate(x0, scale_factor=2, mode="nearest") if up0 else x0
        if x1 is not None:
            xin = torch.cat([xin, x1], dim=1)
        with ou.working_dtype(torch.float64):
            return ou.res_block({"rb." + k: v.double() for k, v in P.items()}, ou.Res("rb", c0 + c1, cout), xin.double(), emb.double())

    return run, ref, 2e-5 if precision == "f16mx" else 1e-5


def two_level_net(precision, n, h, w):
    def inputs():
        gen = torch.Generator().manual_seed(n + h + w)
        return torch.randn((n, 6, h, w), generator=gen), torch.randn((n, 128), generator=gen)

    def model():
        from drmnet_amd import synth
        from drmnet_amd.unet import UNetModel

        m = UNetModel(**NET_CFG)
        synth.load_synth(m, 11)
        return m

    def run(dev):
        x, t = inputs()
        return model().to(dev).set_precision(precision)(x.to(dev), t_emb=t.to(dev))

    def ref():
        from oracle import unet as ou

        x, t = inputs()
        P = {k: v.double() for k, v in model().state_dict().items()}
        with ou.working_dtype(torch.float64):
            return ou.unet_forward(P, ou.build_topology(NET_CFG, "unet"), x.double(), t_emb=t.double())

    from conftest import NET_TOL
    return run, ref, NET_TOL[precision]


CASES = {
    # through ops.norm_act_conv: the NCHW store, deterministic by construction
    "plain_f16x3_full": conv("f16x3", 1, 32, 32, 16, 16, 3, full=True),
    "ragged_f16x3_full": conv("f16x3", 1, 32, 64, 6, 10, 3, full=True),
    "fp32_256x64": conv("fp32", 16, 32, 64, 64, 64, 3),
    "bf16_1x1": conv("bf16", 32, 32, 64, 32, 32, 1),
    # through ops.resblock: the NHWC quad store, statistics into the next GroupNorm, split-K
    "split_in_launch": resblock("f16x3", 1, 256, 0, 256, 16, 16),
    "split_reduce_f16mx": resblock("f16mx", 32, 128, 0, 128, 4, 8),
    "parity_and_residual": resblock("f16x3", 11, 64, 32, 128, 64, 64, up0=True),
    # the two-level network of test_gpu_conv_forms.py: the pooled tail and the pooled statistics
    "pooled_net": two_level_net("f16x3", 11, 64, 64),
}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(name, dev):
    from drmnet_amd import ops

    try:
        out = CASES[name][0](dev)
        torch.cuda.synchronize()
    finally:
        ops.set_precision("fp32")
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_epilogue_bytes(dev, name):
    from conftest import rel_l2

    with open(GOLDEN) as f:
        want = json.load(f)[name]
    out = run_case(name, dev)
    assert torch.isfinite(out).all()
    if want is not None:
        got = digest(out)
        print(f"{name}: sha256 {got}")
        assert got == want
    else:
        e = rel_l2(out.cpu(), CASES[name][1]())
        print(f"{name}: not pinned (its digest did not reproduce on the recording run); rel_l2 vs fp64 reference {e:.2e}")
        assert e < CASES[name][2]


if __name__ == "__main__":  # the recorder: every case twice; a digest that does not reproduce is stored as null
    assert sys.argv[1] == "--record"
    d = torch.device("cuda:0")
    rec = {}
    for nm in CASES:
        a, b = digest(run_case(nm, d)), digest(run_case(nm, d))
        rec[nm] = a if a == b else None
        print(nm, a, "reproduced" if a == b else f"DID NOT REPRODUCE ({b})", flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")

"""Which conv_split2_kernel instantiation a launch runs, per form: one case per GEMM tile, and one each for a ragged map, the in-launch split-K finish,
the pooled epilogue, the 4-tap parity form, an exact-fp32 unit and the f16mx unit -- the smallest shapes for which plan_conv (csrc/conv_plan.hip) picks
each.  The dispatch is derived from the forms csrc/conv_forms.h states; the names below are literals so that a change of either shows here.

The expected names were recorded from a run of this test's body against the library built from the commit BEFORE the forms were stated once (hand-written
dispatch), never from the code under test.  Plain and ragged forms run through the per-module conv op; split-K, 4-tap and pooled forms through the
resblock op or a two-level network, since only the engine plans them.
"""
import pytest
import torch

from drmnet_amd import synth
from test_gpu_upconv import profiled, res_manifest

PREFIX = "void drm::conv_split2_kernel"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def conv(precision, n, cin, cout, h, w, k):
    def run(dev):
        from drmnet_amd import ops

        gen = torch.Generator(device=dev).manual_seed(n + cin + cout + h + w)
        x = torch.randn((n, cin, h, w), generator=gen, device=dev)
        wt = torch.randn((cout, cin, k, k), generator=gen, device=dev) * 0.05
        ops.set_precision(precision)
        return ops.norm_act_conv(x, wt)
    return run


def resblock(precision, n, c0, c1, cout, h, w, up0=False):
    def run(dev):
        from drmnet_amd import ops

        gen = torch.Generator(device=dev).manual_seed(n + c0 + cout + h + w)
        x0 = torch.randn((n, c0, h >> up0, w >> up0), generator=gen, device=dev)
        x1 = torch.randn((n, c1, h, w), generator=gen, device=dev) if c1 else None
        emb = torch.randn((n, 512), generator=gen, device=dev)
        P = [p.to(dev) for p in synth.synth_state_dict(res_manifest(c0 + c1, cout), 5).values()]
        ops.set_precision(precision)
        return ops.resblock(P, x0, emb, x1, up0=up0)
    return run


def two_level_net(precision, n, h, w):
    def run(dev):
        from drmnet_amd.unet import UNetModel

        m = UNetModel(image_size=h, in_channels=6, out_channels=3, model_channels=128, attention_resolutions=[], num_res_blocks=1, dropout=0.0,
                      channel_mult=[1, 2], num_heads=1, resblock_updown=False, conv_resample=False)
        synth.load_synth(m, 11)
        m = m.to(dev).set_precision(precision)
        gen = torch.Generator(device=dev).manual_seed(n + h + w)
        return m(torch.randn((n, 6, h, w), generator=gen, device=dev), t_emb=torch.randn((n, 128), generator=gen, device=dev))
    return run


# case -> (what to run, every conv_split2_kernel instantiation that must have run: template arguments
# <TAPS, TH, TW, WM, WN, MT, NT, ring, taps per step, TERMS, ragged, in-launch split-K, pooled>)
CASES = {
    # 128x32 tiles on a sparse grid: 1 image of 16x16 (2 tiles of 8x16 pixels)
    "tile_128x32": (conv("f16x3", 1, 32, 32, 16, 16, 3), {"<9, 8, 16, 4, 1, 1, 1, 2, 3, 3, false, false, false>"}),
    # 128x64: 256 workgroups of 128 rows, 128 of 256 rows; 1x1, bf16
    "tile_128x64_1x1_bf16": (conv("bf16", 32, 32, 64, 32, 32, 1), {"<1, 8, 16, 2, 2, 2, 1, 4, 1, 4, false, false, false>"}),
    # 256x64: 256 workgroups of 256 rows; exact fp32
    "tile_256x64_fp32": (conv("fp32", 16, 32, 64, 64, 64, 3), {"<9, 16, 16, 4, 2, 2, 1, 2, 3, 0, false, false, false>"}),
    # 256x128: 11 * 4096 / 256 = 176 workgroups, the wide-tile threshold; plain fp16
    "tile_256x128_f16": (conv("f16", 11, 32, 128, 64, 64, 3), {"<9, 16, 16, 4, 2, 2, 2, 2, 3, 1, false, false, false>"}),
    # 256x192 and 256x256 (1x1): 512 workgroups
    "tile_256x192_1x1": (conv("f16x3", 2, 32, 192, 256, 256, 1), {"<1, 16, 16, 4, 2, 2, 3, 3, 1, 3, false, false, false>"}),
    "tile_256x256_1x1": (conv("f16x3", 2, 32, 256, 256, 256, 1), {"<1, 16, 16, 4, 2, 2, 4, 2, 1, 3, false, false, false>"}),
    # a 6x10 map is no whole number of tiles: masked 4x4 pixel tiles, 64 channels wide
    "ragged": (conv("f16x3", 1, 32, 64, 6, 10, 3), {"<9, 4, 4, 2, 2, 2, 1, 2, 3, 3, true, false, false>"}),
    # 128x128 tiles exist for 3x3 on 4-row pixel tiles: 32 images of 4x8, split over K with the second-launch finish; f16mx (TERMS = 2)
    "tile_128x128_split_reduce_f16mx": (resblock("f16mx", 32, 128, 0, 128, 4, 8), {"<9, 4, 8, 2, 2, 2, 2, 3, 1, 2, false, false, false>"}),
    # 1 image of 16x16, 256 channels: 128x32 tiles split over K, finished inside the launch
    "split_in_launch": (resblock("f16x3", 1, 256, 0, 256, 16, 16), {"<9, 8, 16, 4, 1, 1, 1, 2, 3, 3, false, true, false>"}),
    # cat(nearest_x2(x0), x1) at 176 workgroups for both launches: the 4-tap parity form and the 3x3 conv on x1
    "four_tap": (resblock("f16x3", 11, 64, 32, 128, 64, 64, up0=True), {
        "<1, 16, 16, 4, 2, 2, 2, 4, 1, 3, false, false, false>",
        "<4, 16, 16, 4, 2, 2, 2, 2, 2, 3, false, false, false>",
        "<9, 16, 16, 4, 2, 2, 2, 2, 3, 3, false, false, false>",
    }),
    # the Downsample behind the first level's block, from its out_layers conv's epilogue (176 workgroups of 256x128)
    "pooled": (two_level_net("f16x3", 11, 64, 64), {
        "<1, 16, 16, 4, 2, 2, 2, 4, 1, 3, false, false, false>",
        "<1, 8, 16, 2, 2, 2, 1, 4, 1, 3, false, false, false>",
        "<4, 16, 16, 4, 2, 2, 2, 2, 2, 3, false, false, false>",
        "<9, 16, 16, 4, 2, 2, 2, 2, 3, 3, false, false, false>",
        "<9, 16, 16, 4, 2, 2, 2, 2, 3, 3, false, false, true>",
        "<9, 8, 16, 2, 2, 2, 1, 2, 3, 3, false, false, false>",
        "<9, 8, 16, 4, 1, 1, 1, 2, 3, 3, false, false, false>",
    }),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_instantiation_that_runs(dev, name):
    from drmnet_amd import ops

    run, want = CASES[name]
    try:
        out, names = profiled(lambda: run(dev))
    finally:
        ops.set_precision("fp32")
    got = {nm[len(PREFIX):] for nm in names if nm.startswith(PREFIX)}
    print(f"{name}: {sorted(got)}")
    assert torch.isfinite(out).all()
    assert got == want

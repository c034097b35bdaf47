"""CPU-only checks of the C-ABI library: it loads, exports every symbol include/drmnet_hip.h declares,
and its parameter table equals the reference state_dict() layout (no compute calls)."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from conftest import GOLD, ROOT
from drmnet_amd import _lib
from oracle import unet as ou

HEADER = os.path.join(ROOT, "include", "drmnet_hip.h")


def header_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(drm_[a-z0-9_]+)\s*\(", txt)))


def test_library_loads_and_exports_every_declared_symbol():
    L = _lib.lib()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/drmnet_hip.h but not exported"
    assert sorted(_lib.SYMBOLS) == syms
    assert L.drm_abi_version() == _lib.ABI_VERSION == 4


def table(cfg, kind):
    from drmnet_amd.unet import EncoderUNetModel, UNetModel

    cls = UNetModel if kind == "unet" else EncoderUNetModel
    m = cls(**cfg)
    return m, [[k, list(v.shape)] for k, v in m.state_dict().items()]


@pytest.mark.parametrize(
    "name,cfg,kind",
    [("illnet", ou.ILLNET_CFG, "unet"), ("refnet", ou.REFNET_CFG, "encoder"), ("obsnet", ou.OBSNET_CFG, "unet"),
     ("tiny_unet", ou.TINY_UNET_CFG, "unet"), ("tiny_enc", ou.TINY_ENC_CFG, "encoder")],
)
def test_engine_param_table_matches_reference_state_dict(manifests, name, cfg, kind):
    m, tab = table(cfg, kind)
    assert tab == manifests[name]
    assert m.workspace_bytes(2, 128, 128) > 0 if name in ("illnet", "refnet", "obsnet") else m.workspace_bytes(2, 16, 16) > 0


def test_unsupported_configs_are_rejected_loudly():
    from drmnet_amd.unet import UNetModel

    base = dict(ou.TINY_UNET_CFG)
    for bad in (dict(use_spatial_transformer=True, context_dim=8), dict(resblock_updown=True), dict(conv_resample=True),
                dict(use_scale_shift_norm=True), dict(num_heads=2), dict(use_fp16=True), dict(dims=3)):
        cfg = dict(base)
        cfg.update(bad)
        with pytest.raises(NotImplementedError):
            UNetModel(**cfg)


def test_errors_do_not_cross_the_abi_as_exceptions():
    L = _lib.lib()
    d = _lib.UNetDesc()
    d.kind = 7
    h = C.c_void_p()
    assert L.drm_unet_create(C.byref(d), C.byref(h)) != 0
    assert b"kind" in L.drm_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(1)


def test_cpu_tensors_fail_loudly():
    from drmnet_amd.unet import UNetModel

    m = UNetModel(**ou.TINY_UNET_CFG)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 6, 16, 16), timesteps=torch.zeros(1, dtype=torch.long))


def test_workspace_query_rejects_bad_shapes():
    from drmnet_amd.unet import UNetModel

    m = UNetModel(**ou.TINY_UNET_CFG)
    assert m.workspace_bytes(1, 10, 10) == 0  # 10x10 is not divisible down to a 4x4 map


# the dry sizing pass makes every conv's split-K, ticket-table and attention-workspace decision on the CPU: its answers are pinned to the recorded
# table (tests/golden/workspace_bytes.json) so a change of any of those decisions shows without a GPU
WS_NETS = [("illnet", ou.ILLNET_CFG, "unet"), ("refnet", ou.REFNET_CFG, "encoder"), ("obsnet", ou.OBSNET_CFG, "unet"), ("tiny_unet", ou.TINY_UNET_CFG, "unet")]
WS_SIZES = [(1, 128, 128), (32, 128, 256), (128, 128, 256), (2, 96, 160)]
WS_TINY_SIZES = [(3, 4, 4), (2, 12, 20), (1, 44, 20), (5, 24, 40), (2, 36, 68)]  # (test_gpu_sizes.py)


def workspace_table():
    from drmnet_amd.unet import EncoderUNetModel, UNetModel

    out = {}
    for name, cfg, kind in WS_NETS:
        m = (UNetModel if kind == "unet" else EncoderUNetModel)(**cfg)
        for prec in m.PRECISIONS:
            m.set_precision(prec)
            for n, h, w in WS_TINY_SIZES if name == "tiny_unet" else WS_SIZES:
                out[f"{name} {prec} {n}x{h}x{w}"] = m.workspace_bytes(n, h, w)
    return out


def test_workspace_bytes_match_the_recorded_sizing():
    with open(os.path.join(GOLD, "workspace_bytes.json")) as f:
        assert workspace_table() == json.load(f)


# the chains' workspace on top of the network's: recorded from the two hand-written chain drivers before they became one (ObsNet and the tiny U-Net,
# the networks the chains run on), so the shared driver's allocations and the chain's sizing walk are pinned without a GPU
def sampler_workspace_table():
    from drmnet_amd.unet import UNetModel

    out = {}
    for name, cfg, sizes in (("obsnet", ou.OBSNET_CFG, WS_SIZES), ("tiny_unet", ou.TINY_UNET_CFG, WS_TINY_SIZES)):
        m = UNetModel(**cfg)
        for prec in m.PRECISIONS:
            m.set_precision(prec)
            for n, h, w in sizes:
                out[f"{name} {prec} {n}x{h}x{w}"] = int(_lib.lib().drm_sampler_workspace_bytes(m._h, n, h, w))
    return out


def test_sampler_workspace_bytes_match_the_recorded_sizing():
    with open(os.path.join(GOLD, "sampler_workspace_bytes.json")) as f:
        assert sampler_workspace_table() == json.load(f)


# every branch of the attention plan (attn.hip plan_attention: single-kernel, conv-pipeline and short-sequence forms, guarded or not) at the
# smallest shape that reaches it, sized through a two-level U-Net whose only attention blocks run at C channels on the H x W map; the recorded
# answers (tests/golden/attn_workspace_bytes.json) are those of the code before the plan existed
ATTN_WS_CASES = [(384, 32, 32, (1, 3), ["f16x3", "f16mx", "f16", "bf16"]), (384, 32, 32, (2,), ["fp32"]), (512, 16, 16, (5,), ["f16x3", "bf16", "fp32"]),
                 (512, 16, 16, (2,), ["f16x3", "f16", "bf16"]), (64, 4, 4, (3,), ["f16x3"]), (32, 8, 4, (1,), ["fp32"]), (640, 8, 8, (2,), ["fp32"]),
                 (768, 4, 8, (2,), ["f16x3", "f16mx"])]


def test_attention_workspace_bytes_match_the_recorded_sizing():
    from drmnet_amd.unet import UNetModel

    nets, out = {}, {}
    for c, h, w, ns, modes in ATTN_WS_CASES:
        if c not in nets:
            nets[c] = UNetModel(image_size=16, in_channels=6, model_channels=min(c, 128), out_channels=3, num_res_blocks=1, attention_resolutions=[2],
                                channel_mult=[1, max(1, c // 128)], num_heads=1, resblock_updown=False, conv_resample=False)
        for mode in modes:
            nets[c].set_precision(mode)
            for n in ns:
                out[f"{c} {mode} {n}x{h}x{w}"] = nets[c].workspace_bytes(n, 2 * h, 2 * w)
    with open(os.path.join(GOLD, "attn_workspace_bytes.json")) as f:
        assert out == json.load(f)

"""GroupNorm32 against the fp64 reference, elementwise, with the statistics coming from every producer (tests/gn_ref.py holds the reference, the
rounding-model bound, the input families and the mutants; tests/test_gn_ref_cpu.py shows on the CPU that the bound holds for correct arithmetic
and that every mutant leaves it on a case below; DESIGN.md "GroupNorm checks").

Probe A  ops.norm_act_conv(x, identity 1x1, gamma, beta) returns GN(x) itself (multiplying by 1.0 and adding zeros is exact in the fp32 MFMA
         chain): the stand-alone moments (csrc/gn.hip chan_moments_*) and gn_finalize_kernel, in every mode, on offset, scaled, constant, zero,
         per-image and plain images.
Probe B  ops.resblock with out_layers = centre-tap identity: out = skip + SiLU(GN2(h1)), h1 carrying per-channel offsets of 2^3 and 2^6 from
         in_layers.2.bias + emb_layers.1.bias.  GN2's statistics come from the conv epilogue that wrote h1 (csrc/conv_split2.hip stat_out, in
         each of its forms; csrc/conv.hip for the second-launch split-K finish); the tables are finalised by gn_finalize_kernel or, for N <= 4,
         in the prologue of the out_layers conv.  The decoder cases put a GroupNorm over a concat boundary in front (GN1).
Probe C  a two-level network with attention and conv biases scaled by 2^4, against the fp64 oracle: the pooled epilogue's statistics and the
         attention core's are reachable only there.  Whole-tensor rel-L2: coarser than A and B.
"""
import ctypes as C

import pytest
import torch

import gn_ref as G
from conftest import NET_TOL, rel_l2

PREFIX = "void drm::conv_split2_kernel"
TERMS = {"fp32": 0, "f16x3": 3}
PROF_GNSTATS = 3  # csrc/profiler.h ProfKind: launches of the stand-alone moments


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def outside(out, ref, bnd):
    """None, or the message naming the first (n, c, y, x) whose error is outside the bound"""
    err = (out.detach().cpu().double() - ref).abs()
    bad = G.first_outside(err, bnd)
    if bad is None:
        return None
    count, idx, e, b = bad
    return (f"{count} of {err.numel()} elements outside the bound; first at (n, c, y, x) = {idx}: got {float(out[idx])!r}, want {float(ref[idx])!r}, "
            f"error {e:.3e} > bound {b:.3e}; worst error / bound {G.worst_ratio(err, bnd):.2f}")


# ------------------------------------------------------------------------------------------------ Probe A

# (n, C, H, W) -> what the shape covers (csrc/gn.hip, csrc/gn_fold.h)
PROBE_A = {
    (3, 32, 4, 4): "cpg = 1: seven of a group's eight lanes idle",
    (2, 64, 6, 10): "ragged map; HW = 60: splits = 1",
    (5, 192, 8, 8): "cpg = 6, five images",
    (2, 384, 10, 20): "cpg = 12: a second trip for 4 of 8 lanes; HW = 200: 3 uneven splits (66 / 67 / 67); 96 channel quads: a masked second qb block",
    (1, 1408, 4, 8): "cpg = 44, as in the decoder",
    (1, 1600, 4, 4): "C > 6 * 256: the non-preload path of gn_finalize_image",
}
assert list(PROBE_A) == G.PROBE_A
_A = {}


def probe_a_case(shape):
    """[(x, families, reference GN, gamma, beta), ...], one per batch start: computed once, shared by the modes, never modified"""
    if shape not in _A:
        n, c, h, w = shape
        gamma, beta = G.affine(c)
        _A[shape] = []
        for start in G.starts(n):
            x, fams = G.batch(n, c, h, w, start)
            _A[shape].append((x, fams, G.group_norm64(x, gamma, beta), gamma, beta))
    return _A[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", G.MODES)
@pytest.mark.parametrize("shape", list(PROBE_A), ids=lambda s: "x".join(str(v) for v in s))
def test_probe_a_moments_and_finalize(dev, shape, mode):
    from drmnet_amd import ops

    c = shape[1]
    wt = torch.eye(c)[:, :, None, None].contiguous().to(dev)
    fails, worst = [], 0.0
    try:
        ops.set_precision(mode)
        for x, fams, gn, gamma, beta in probe_a_case(shape):
            out = ops.norm_act_conv(x.to(dev), wt, None, gamma.to(dev), beta.to(dev), silu=False).cpu()
            bnd = G.bound(x, gn.sc, gn.sh, gn.y, mode, beta)
            worst = max(worst, G.worst_ratio((out.double() - gn.y).abs(), bnd))
            msg = outside(out, gn.y, bnd)
            if msg:
                fails.append(f"{fams}: {msg}")
    finally:
        ops.set_precision("fp32")
    print(f"probe A {shape} {mode}: worst error / bound {worst:.3f}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ Probe B

def profiled(fn):
    """fn() under the library's launch profiler -> (result, instantiations of conv_split2_kernel that ran, launches per ProfKind)"""
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
    buf = C.create_string_buffer(int(L.drm_profile_variants(None, 0)) + 16)
    L.drm_profile_variants(buf, len(buf))
    L.drm_profile_reset()
    names = [ln.split("\t")[0] for ln in buf.value.decode().splitlines()]
    return out, [nm[len(PREFIX):] for nm in names if nm.startswith(PREFIX)], list(cnt)


FIELDS = "taps th tw wm wn mt nt ring tps terms rag sk pool".split()


def forms(insts):
    """template arguments of each instantiation as a dict, with bm / bn = GEMM rows / channels of the tile"""
    out = []
    for s in insts:
        v = [t.strip() for t in s.strip("<>").split(",")]
        assert len(v) == len(FIELDS), s
        d = {k: (t == "true" if t in ("true", "false") else int(t)) for k, t in zip(FIELDS, v)}
        d["bm"], d["bn"] = d["wm"] * d["mt"] * 32, d["wn"] * d["nt"] * 32
        out.append(d)
    return out


def has(fs, **want):
    return any(all(f[k] == v for k, v in want.items()) for f in fs)


# case -> (what the instantiations must show, stand-alone moment launches: one per block input where h1's statistics come fused).  The tile
# shapes are those tests/test_gpu_conv_forms.py pins for these shapes; exact fp32 (TERMS = 0) has no pipeline form on a map that is not whole
# 4x4 tiles (csrc/conv_plan.hip): the fp32 run of the ragged case is conv_igemm_kernel and h1's statistics are the stand-alone moments.
def expect(name, mode, fs, moments):
    t = TERMS[mode]
    if name == "prologue_128x32":  # N <= 4: both GroupNorms are finalised in the prologue of their conv (ConvPlan::gn_fold)
        return has(fs, taps=9, bm=128, bn=32, terms=t, rag=False, sk=False, pool=False) and moments == 1
    if name == "ragged":
        return (not fs and moments == 2) if mode == "fp32" else (has(fs, taps=9, th=4, tw=4, terms=t, rag=True) and moments == 1)
    if name == "split_in_launch":
        return has(fs, taps=9, bm=128, bn=32, terms=t, sk=True) and moments == 1
    if name == "split_reduce":  # 128x128 tiles on 4x8 pixel tiles exist only for the split-K form with the second-launch finish
        return has(fs, taps=9, th=4, tw=8, bm=128, bn=128, terms=t, sk=False) and moments == 1
    if name == "deferred_fold_256":  # 16 tiles of 256 rows per image: a workgroup keeps its LDS statistics across tiles of one image
        return has(fs, taps=9, bm=256, bn=64, terms=0, rag=False, sk=False) and moments == 1
    if name == "parity":  # launch A = the 4-tap form, launch B = 3x3 on x1 with res == out and the statistics of the sum
        return has(fs, taps=4, bm=256, bn=128, terms=t) and has(fs, taps=9, bm=256, bn=128, terms=t) and moments == 2
    if name == "parity_prologue":  # N <= 4: no parity form, one launch over the concat, tables finalised in its prologue
        return not has(fs, taps=4) and has(fs, taps=9, bm=128, bn=32, terms=t) and moments == 2
    raise KeyError(name)


PROBE_B = [(name, mode) for name, case in G.PROBE_B.items() for mode in case[7]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", PROBE_B, ids=[f"{n}-{m}" for n, m in PROBE_B])
def test_probe_b_fused_statistics(dev, name, mode):
    from drmnet_amd import ops

    P, x0, x1, emb, ref, bnd = G.block_case(name, mode)
    up0 = G.PROBE_B[name][6]
    Pd = [p.to(dev) for p in P.values()]
    try:
        ops.set_precision(mode)
        out, insts, cnt = profiled(lambda: ops.resblock(Pd, x0.to(dev), emb.to(dev), None if x1 is None else x1.to(dev), up0=up0).cpu())
    finally:
        ops.set_precision("fp32")
    err = (out.double() - ref).abs()
    print(f"probe B {name} {mode}: worst error / bound {G.worst_ratio(err, bnd):.3f}; stand-alone moment launches {cnt[PROF_GNSTATS]}; ran {sorted(insts)}")
    assert expect(name, mode, forms(insts), cnt[PROF_GNSTATS]), (sorted(insts), cnt[PROF_GNSTATS])
    msg = outside(out, ref, bnd)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ Probe C

NET_CFG = dict(image_size=64, in_channels=6, out_channels=3, model_channels=128, attention_resolutions=[2], num_res_blocks=1, dropout=0.0,
               channel_mult=[1, 2], num_heads=1, resblock_updown=False, conv_resample=False)
NET_N = 11  # 176 workgroups of 256x128 on the first level: from there on the Downsample is the out_layers conv's pooled epilogue
_C = {}


def net_case():
    """(state dict with conv biases x 2^4, x, t_emb, fp64 oracle output, rel-L2 of the CPU fp32 oracle against it): computed once"""
    if not _C:
        from drmnet_amd import synth
        from drmnet_amd.unet import UNetModel
        from oracle import unet as ou

        m = UNetModel(**NET_CFG)
        synth.load_synth(m, 11)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        for k in sd:
            if k.endswith(".bias") and sd[k[:-4] + "weight"].dim() >= 3:  # a conv's bias: activations carry offsets
                sd[k] = sd[k] * 16.0
        gen = torch.Generator().manual_seed(NET_N + 64)
        x, t = torch.randn((NET_N, 6, 64, 64), generator=gen), torch.randn((NET_N, 128), generator=gen)
        topo = ou.build_topology(NET_CFG, "unet")
        with ou.working_dtype(torch.float64):
            ref = ou.unet_forward({k: v.double() for k, v in sd.items()}, topo, x.double(), t_emb=t.double())
        e32 = rel_l2(ou.unet_forward(sd, topo, x, t_emb=t), ref)
        _C["case"] = (sd, x, t, ref, e32)
    return _C["case"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_probe_c_pooled_and_attention_statistics(dev, mode):
    """Coarser than Probes A and B: one rel-L2 over a whole network output, where a wrong table of one GroupNorm is diluted by everything else.
    The bar is measured on the reference arithmetic: 4 x the rel-L2 of the CPU fp32 oracle on the same offset weights against the fp64 oracle,
    and never more than conftest.NET_TOL."""
    from drmnet_amd.unet import UNetModel

    sd, x, t, ref, e32 = net_case()
    m = UNetModel(**NET_CFG)
    m.load_state_dict(sd)
    m = m.to(dev).set_precision(mode)
    out, insts, cnt = profiled(lambda: m(x.to(dev), t_emb=t.to(dev)).cpu())
    e = rel_l2(out, ref)
    bar = min(4.0 * e32, NET_TOL[mode])
    print(f"probe C {mode}: rel_l2 {e:.3e}; CPU fp32 oracle {e32:.3e}; bar {bar:.3e}; stand-alone moment launches {cnt[PROF_GNSTATS]}")
    if mode != "fp32":  # (the pooled epilogue is a form of the split modes)
        assert has(forms(insts), taps=9, pool=True), sorted(insts)
    assert torch.isfinite(out).all()
    assert e <= bar

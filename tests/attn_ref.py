"""CPU helpers of the sharp attention checks (tests/test_attn_ref_cpu.py, tests/test_gpu_attn_sharp.py).  No GPU code.

The attention tests before these drew randn inputs and 1/sqrt(fan_in) weights: log2-logits of standard deviation 1.5, a largest probability of
0.017 at T = 1024, and not one rescale of the single-kernel form's running maximum after the first key tile (DESIGN.md "Sharp attention checks").
Here `gain` G multiplies the q rows and the k rows of qkv.weight / qkv.bias by sqrt(G) each: the logits grow by G while q and k stay the same
size as each other (the qkv conv packs its weight tensor with ONE power of two: the row groups stay inside its 2^-24 .. 1 window).

    block_case      inputs, parameters, fp64 log2-logits and folded v' of one block (computed once, shared, never modified)
    exact / ref32   the block in fp64 / fp32 (oracle.unet.attention_block); r64 = their distance on the branch out - x
    lazy_softmax    the single-kernel form's online softmax in fp64 (csrc/attn_flash.hip: 128-key tiles, the running maximum raised only when a
                    tile exceeds it by more than FA_TAU = 6 log2 units), with three mutants of its rescale
    classes         masks over the output where an attention bug would sit
    emulate         the fp64 block with the operand roundings of the f16 / bf16 modes
"""
import math
import types

import torch
import torch.nn.functional as F

from conftest import rel_l2
from drmnet_amd import synth
from oracle import unet as ou
from quant_ref import MIN_CLASS, TERMS, _merged, quantise
from test_oracle_golden import attn_manifest

LOG2E = 1.4426950408889634
TILE, TAU = 128, 6.0  # FA_KT, FA_TAU of csrc/attn_flash.hip
MUTANTS = ("o_not_rescaled", "l_not_rescaled", "lane0_factor")
BRANCH_BAR = 1e-4  # the branch bar of the accurate modes (tests/test_gpu_attn_flash.py)
REDUCED = ("f16", "bf16")
REDUCED_MAX_GAIN = 8  # beyond it the softmax is nearly one-hot and an operand rounding flips arg-maxes: chaos, not a kernel property
RATIO = (0.5, 2.0)  # class band of the reduced modes: twice quant_ref.RATIO (a logit perturbation d changes a probability by e^d - 1, not linearly)

# id -> form the plan must take in the split modes, C, H, W, N, gains, modes.  Exact fp32 is the three-launch short-sequence form at every shape.
CASES = {
    "flash_1024": dict(form="flash", C=384, H=32, W=32, N=1, gains=(4, 64), modes=("fp32", "f16x3", "f16", "bf16")),
    "flash_1152": dict(form="flash", C=384, H=24, W=48, N=3, gains=(8,), modes=("f16x3", "f16")),  # 27 workgroups: the unswizzled order
    "conv_512": dict(form="conv", C=128, H=16, W=32, N=3, gains=(8, 64), modes=("f16x3", "f16mx", "f16", "bf16")),
    "small_256": dict(form="small", C=128, H=16, W=16, N=2, gains=(8, 64), modes=("fp32", "f16x3", "f16mx", "f16", "bf16")),
    "small_32": dict(form="small", C=128, H=8, W=4, N=5, gains=(8, 64), modes=("fp32", "f16x3", "f16mx", "f16", "bf16")),
    "small_16": dict(form="small", C=64, H=4, W=4, N=3, gains=(8, 64), modes=("fp32", "f16x3", "f16mx", "f16", "bf16")),
}
# fp32 three-launch form: softmax_rows_reg_kernel<Q> for Q = 3, 5, 6, 7 (T = 256 Q) and the generic row kernel at T = 1088
SOFTMAX_Q = {"softmax_Q3": (24, 32), "softmax_Q5": (32, 40), "softmax_Q6": (32, 48), "softmax_Q7": (28, 64), "softmax_generic_1088": (32, 34)}
SOFTMAX_Q_C, SOFTMAX_Q_GAIN = 64, 8
# the image-group loop: 64 images at T = 2048 fill the 1 GiB score buffer, image 64 is a short last group
GROUPS = dict(C=128, H=32, W=64, N=65, gain=4, modes=("fp32", "f16x3"))
SEED = 5


def gpu_cases():
    """(id, gain, mode) of every block case of tests/test_gpu_attn_sharp.py; the reduced modes run gains up to REDUCED_MAX_GAIN"""
    return [(nm, g, m) for nm, c in CASES.items() for g in c["gains"] for m in c["modes"] if m not in REDUCED or g <= REDUCED_MAX_GAIN]


def variant(form, mode, C, T, passes=1):
    """the name launch_attention_core (csrc/attn.hip) gives the profiler: drm::attn_core<form, TERMS, split_qk, split_pv, passes>"""
    terms = 3 if mode == "f16mx" else TERMS[mode]  # (attention has no mx site)
    if terms == 0:
        form = "small"
    sq = int(form == "small" and terms != 0 and C % 32 == 0)
    sp = int(sq and T % 32 == 0)
    return f"drm::attn_core<{form}, {terms}, {sq}, {sp}, {passes}>"


# ------------------------------------------------------------------------------------------------ cases

_CASES = {}


def block_case(C, H, W, N, gain, seed=SEED):
    """x [N, C, H, W], P (the six parameters of attn_manifest(C), q and k rows times sqrt(gain)), logits [N, T, T] (fp64, log2 units, query x key)
    and v [N, T, C] (fp64, the folded v' = Wp (Wv xn + bv) + bp per key): branch = softmax(logits) v."""
    key = (C, H, W, N, gain, seed)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * seed + C + 3 * H + W + N)
        x = torch.randn((N, C, H, W), generator=gen)
        x[0] = x[0] * 0.5 + 0.25  # rows of different scale and offset: per-image factors, per-image residual
        if N > 1:
            x[N - 1] = x[N - 1] * 3.0 - 1.0
        P = synth.synth_state_dict(attn_manifest(C), 31)
        w, b = P["qkv.weight"].clone(), P["qkv.bias"].clone()
        w[:2 * C] *= math.sqrt(gain)
        b[:2 * C] *= math.sqrt(gain)
        P["qkv.weight"], P["qkv.bias"] = w, b
        D = {k: v.double() for k, v in P.items()}
        xn = F.group_norm(x.double().reshape(N, C, H * W), ou.GN_GROUPS, D["norm.weight"], D["norm.bias"], ou.GN_EPS)
        q, k, v = F.conv1d(xn, D["qkv.weight"], D["qkv.bias"]).split(C, dim=1)
        logits = torch.einsum("bct,bcs->bts", q, k) * (LOG2E / math.sqrt(C))
        vp = F.conv1d(v, D["proj_out.weight"], D["proj_out.bias"]).transpose(1, 2).contiguous()
        _CASES[key] = types.SimpleNamespace(C=C, H=H, W=W, N=N, T=H * W, gain=gain, x=x, P=P, logits=logits, v=vp, memo={})
    return _CASES[key]


def named_case(name, gain):
    c = CASES[name]
    return block_case(c["C"], c["H"], c["W"], c["N"], gain)


def _memo(case, key, fn):
    if key not in case.memo:
        case.memo[key] = fn()
    return case.memo[key]


def _oracle(case, dtype):
    with ou.working_dtype(dtype):
        return ou.attention_block({"ab." + k: v.to(dtype) for k, v in case.P.items()}, ou.Attn("ab", case.C), case.x.to(dtype))


def exact(case):
    """the block in fp64 [N, C, H, W]"""
    return _memo(case, "exact", lambda: _oracle(case, torch.float64))


def ref32(case):
    return _memo(case, "ref32", lambda: _oracle(case, torch.float32))


def branch(case, out):
    """out - x: the residual is added exactly and would dilute an error of the attention branch about five times"""
    return out.double() - case.x.double()


def r64(case):
    """the fp32 reference's own distance from fp64 on the branch"""
    return _memo(case, "r64", lambda: rel_l2(branch(case, ref32(case)), branch(case, exact(case))))


def accurate_bar(case):
    """fp32, f16x3, f16mx: the branch bar of the existing tests, or ten times the fp32 reference's own error where that is larger (the margin of
    test_stress_weights_vs_reference for noise-level comparisons)"""
    return max(BRANCH_BAR, 10.0 * r64(case))


def check_accurate(case, out, rows=None):
    """The accurate modes on a block output `out` [N, C, H, W] (rows: the rows of a larger batch that are the case's) -> (failures, branch rel-L2).
    Whole branch below accurate_bar; and per class the rule of quant_ref.check_accurate -- no class above twice the whole tensor's relative error --
    OR within ten times the fp32 oracle's own error IN THAT CLASS.  The second term is needed in the peaked regime: rounding noise is not
    homogeneous there (a logit's rounding moves a flat softmax row, not a one-hot one), and the fp32 oracle itself carries 7 .. 8 times its
    whole-tensor error on the queries whose largest probability is below 0.5 at G = 64 (test_attn_ref_cpu.test_fp32_oracle_is_not_homogeneous);
    ten is the project's margin for noise-level comparisons, as in accurate_bar."""
    from quant_ref import class_ratios
    cls, bar = classes(case), accurate_bar(case)
    got = branch(case, out if rows is None else out[rows])
    want, own = branch(case, exact(case)), branch(case, ref32(case))
    e = rel_l2(got, want)
    fails = [] if e < bar else [f"branch rel_l2 {e:.3e} >= {bar:.1e}"]
    if not torch.isfinite(got).all():
        fails.append("not finite")
    r_got, r_own = class_ratios(got, want, cls), class_ratios(own, want, cls)
    for nm, r in r_got.items():
        if not r * e <= max(2.0 * e, 10.0 * r_own[nm] * r64(case)):
            fails.append(f"class {nm}: {r * e:.3e} = {r:.2f} x the whole tensor's error; the fp32 oracle has {r_own[nm] * r64(case):.3e} there")
    return fails, e


def nchw(case, t):
    """[N, T, C] -> [N, C, H, W]"""
    return t.transpose(1, 2).reshape(case.N, case.C, case.H, case.W)


def pmax_argmax(case):
    return _memo(case, "pmax", lambda: tuple(torch.softmax(case.logits / LOG2E, dim=-1).max(dim=-1)))


# ------------------------------------------------------------------------------------------------ the online softmax of attn_flash_kernel

def lazy_softmax(logits, v, tile=TILE, tau=TAU, mutant=None, stage=None, trace=None):
    """softmax(logits) v by the single-kernel form's rule, in fp64: per `tile` keys, m_run is raised to the tile's maximum only where that exceeds it
    by more than `tau` (the first tile always raises), O and the row sum l are rescaled by 2^(m_old - m_new), p = 2^(s - m_run) <= 2^tau.
    stage: optional rounding of p as it enters P v (the row sum takes the unrounded p, as the kernel does).
    mutant: "o_not_rescaled" (O keeps its old scale), "l_not_rescaled" (the row sum does), "lane0_factor" (the 32 queries of a wave all take the
    factor of the first).  -> (out [.., Tq, C], raises [.., Tq] after the first tile, head-room [.., Tq]: the largest excess over m_run that did NOT
    raise it, in log2 units).  trace: optional list that receives the raise mask [.., Tq] of every tile."""
    assert mutant in (None,) + MUTANTS
    tq, tk = logits.shape[-2], logits.shape[-1]
    assert tk % tile == 0 and (mutant != "lane0_factor" or tq % 32 == 0)
    lead = logits.shape[:-1]
    m = torch.full(lead, -math.inf, dtype=torch.float64)
    l = torch.zeros(lead, dtype=torch.float64)
    O = torch.zeros(lead + (v.shape[-1],), dtype=torch.float64)
    raises = torch.zeros(lead, dtype=torch.long)
    room = torch.zeros(lead, dtype=torch.float64)
    for t0 in range(0, tk, tile):
        s = logits[..., t0:t0 + tile]
        mt = s.max(dim=-1).values
        up = mt > m + tau
        m_new = torch.where(up, mt, m)
        f = torch.exp2(m - m_new)  # (first tile: 2^-inf = 0)
        if trace is not None:
            trace.append(up)
        if t0:
            raises += up
            room = torch.maximum(room, torch.where(up, torch.zeros_like(mt), mt - m))
        fo = fl = f
        if mutant == "lane0_factor":
            fo = fl = f.reshape(lead[:-1] + (tq // 32, 32))[..., :1].expand(lead[:-1] + (tq // 32, 32)).reshape(lead)
        elif mutant == "o_not_rescaled" and t0:
            fo = torch.ones_like(f)
        elif mutant == "l_not_rescaled" and t0:
            fl = torch.ones_like(f)
        m = m_new
        p = torch.exp2(s - m[..., None])
        l = l * fl + p.sum(dim=-1)
        O = O * fo[..., None] + torch.matmul(p if stage is None else stage(p), v[..., t0:t0 + tile, :])
    return O / l[..., None], raises, room


def lazy_stats(case):
    """(raises, head-room) [N, T] of a long-sequence case"""
    return _memo(case, "lazy", lambda: lazy_softmax(case.logits, case.v)[1:])


# ------------------------------------------------------------------------------------------------ where an error sits

def classes(case, min_count=MIN_CLASS):
    """{name: boolean mask [N, C, H, W]}: each image, each 32-query wave and 128-query workgroup tile, each 32-channel block, the 128-key tile that
    holds the query's arg-max, queries with / without a raise of the running maximum after the first tile (T >= 1024), queries whose largest
    probability is above / below 0.5.  Classes below min_count elements are merged into their neighbour (quant_ref's rule)."""
    def make():
        N, C, T = case.N, case.C, case.T
        qidx = torch.arange(T)[None].expand(N, T)
        img = torch.arange(N)[:, None].expand(N, T)
        full = lambda mq: mq[:, None, :].expand(N, C, T).reshape(N, C, case.H, case.W).clone()  # (query t = y W + x)
        pm, am = pmax_argmax(case)
        groups = [[(f"image_{i}", full(img == i)) for i in range(N)]]
        for nm, sz in (("wave", 32), ("workgroup", 128)):
            if T > sz:
                groups.append([(f"{nm}_{i}_{t0}", full((img == i) & (qidx // sz == t0 // sz))) for i in range(N) for t0 in range(0, T, sz)])
        blk = []
        for j in range(0, C, 32):
            mk = torch.zeros((N, C, case.H, case.W), dtype=torch.bool)
            mk[:, j:j + 32] = True
            blk.append((f"channels_{j}", mk))
        groups.append(blk)
        if T % TILE == 0 and T >= 2 * TILE:
            groups.append([(f"argmax_tile_{t0}", full(am // TILE == t0 // TILE)) for t0 in range(0, T, TILE)])
        if T % TILE == 0 and T >= 1024:
            late = lazy_stats(case)[0] > 0
            groups.append([("late_raise", full(late)), ("no_late_raise", full(~late))])
        groups.append([("pmax_above_half", full(pm > 0.5)), ("pmax_below_half", full(pm <= 0.5))])
        out = {}
        for g in groups:
            for nm, mk in _merged(g, min_count):
                out[nm] = mk
        return out
    return _memo(case, ("classes", min_count), make)


# ------------------------------------------------------------------------------------------------ operand rounding of the reduced modes

def _round_pow2(t, mode):
    """q, k or v' [N, T, C] as the core stages it: times the image's power of two 2^k (attn_scales_kernel: bound = sqrt(max over channels of the
    sum of squares over the pixels), bound 2^k in [2^14, 2^15)), rounded to fp16, divided again; bf16 has fp32's range and rounds directly."""
    t32 = t.float()  # (the kernel reads the qkv conv's fp32 output)
    if mode == "bf16":
        return t32.bfloat16().double()
    out = torch.empty_like(t, dtype=torch.float64)
    for n in range(t.shape[0]):
        bound = math.sqrt(float((t32[n].double() ** 2).sum(dim=0).max()))
        k = max(-40, min(40, 15 - math.frexp(bound)[1])) if 0.0 < bound < math.inf else 0
        out[n] = (t32[n] * 2.0 ** k).clamp(-65504.0, 65504.0).half().double() / 2.0 ** k
    return out


def _stage(mode, factor):
    if mode == "bf16":
        return lambda p: p.float().bfloat16().double()
    return lambda p: (p.float() * factor).half().double() / factor


def emulate(case, mode, form):
    """The fp64 block [N, C, H, W] with the roundings of `mode` (f16 / bf16) in the core `form` ("flash", "conv", "small"):
      the qkv conv's operands (GroupNorm output; the folded [3C, C] weight, v rows = Wp Wv, one power of two) as quant_ref.quantise rounds a conv's;
      q, k and v' at their per-image power of two;
      the probabilities at the form's staging factor: 2^12 on the normalised row in attn.hip, 2^8 on 2^(s - m_run) with the lazy maximum in the
      single-kernel form.  T % 32 != 0 (the 4x4 level): P v stays exact fp32, neither p nor v' is rounded."""
    assert mode in REDUCED and form in ("flash", "conv", "small")

    def make():
        N, C, T = case.N, case.C, case.T
        D = {k: v.double() for k, v in case.P.items()}
        wq, wp = D["qkv.weight"][:, :, 0], D["proj_out.weight"][:, :, 0]
        wf = torch.cat([wq[:2 * C], wp @ wq[2 * C:]]).float()  # the fold: fp64 products, rounded once (conv_split.hip fold_attn_params_kernel)
        bf = torch.cat([D["qkv.bias"][:2 * C], wp @ D["qkv.bias"][2 * C:] + D["proj_out.bias"]]).float()
        xn = F.group_norm(case.x.double().reshape(N, C, T), ou.GN_GROUPS, D["norm.weight"], D["norm.bias"], ou.GN_EPS)
        qkv = F.conv1d(quantise(xn, mode, "act"), quantise(wf, mode, "w")[:, :, None], bf.double())
        q, k, v = (t.transpose(1, 2) for t in qkv.split(C, dim=1))  # [N, T, C]
        q, k = _round_pow2(q, mode), _round_pow2(k, mode)
        logits = torch.einsum("btc,bsc->bts", q, k) * (LOG2E / math.sqrt(C))
        if form == "flash":
            o = lazy_softmax(logits, _round_pow2(v, mode), stage=_stage(mode, 256.0))[0]
        elif T % 32 == 0:
            o = torch.matmul(_stage(mode, 4096.0)(torch.softmax(logits / LOG2E, dim=-1)), _round_pow2(v, mode))
        else:
            o = torch.matmul(torch.softmax(logits / LOG2E, dim=-1), v.float().double())
        return case.x.double() + nchw(case, o)
    return _memo(case, ("emulate", mode, form), make)


def class_band(r_emul, band=RATIO):
    """The band a class ratio of (GPU - exact) is held to, from the emulation's own ratio of that class: RATIO where the emulation is homogeneous
    (its ratio 1), moved out to the emulation's ratio where the rounding error itself is not (test_attn_ref_cpu.test_emulation_class_ratios)."""
    return band[0] * min(1.0, r_emul), band[1] * max(1.0, r_emul)


def class_ratios_in(ratios, band=RATIO):
    return [f"class {nm}: ratio {r:.3f} outside {list(band)}" for nm, r in ratios.items() if not band[0] <= r <= band[1]]


# ------------------------------------------------------------------------------------------------ the image-group case

def groups_batch(case, n):
    """x [n, C, H, W] of the image-group case from a 3-row case: rows 0, n - 2, n - 1 are the case's rows; rows 1 .. n - 3 are copies of rows 0 and
    n - 2 alternately.  -> (x, {row of the batch: row of the case})"""
    assert case.N == 3 and n >= 4
    src = {0: 0, n - 2: 1, n - 1: 2}
    for i in range(1, n - 2):
        src[i] = 0 if i % 2 == 0 else 1
    return torch.stack([case.x[src[i]] for i in range(n)]), src

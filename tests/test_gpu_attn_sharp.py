"""Sharp checks of the attention core (csrc/attn.hip: three forms; csrc/attn_flash.hip: the single-kernel online softmax) in the PEAKED regime that
randn inputs never reach (DESIGN.md "Sharp attention checks"; CPU side: tests/attn_ref.py, tests/test_attn_ref_cpu.py).  Every case runs
ops.attention_block with the q and k rows of the qkv projection times sqrt(G) (logits times G), is compared with the block in fp64 on the branch
out - x, and first asserts from the library profiler which core ran: drm::attn_core<form, TERMS, split_qk, split_pv, passes>.

Cases (attn_ref.CASES; tests/test_attn_ref_cpu.py shows with the library's own planner that each takes the form named here) and the dispatch
branches they are the first to reach:

  flash_1024   384 @ 32x32 x 1, G = 4 / 64      attn_flash_kernel at its own shape with 0.25 / 0.87 of the queries raising the running maximum after
                                                the first key tile (rescale of O^T and of the row sum, mixed waves under __any)
  flash_1152   384 @ 24x48 x 3, G = 8           27 workgroups: the UNSWIZZLED workgroup order, (total & 7) != 0 in attn_flash_kernel
  conv_512     128 @ 16x32 x 3, G = 8 / 64      the conv-pipeline form in the peaked regime (probabilities below fp16 at the 2^12 staging factor)
  small_256    128 @ 16x16 x 2                  qk_small / pv_small in the peaked regime
  small_32     128 @ 8x4 x 5                    ... T = one 32-key chunk
  small_16     64 @ 4x4 x 3                     split S with the exact-fp32 P v (bgemm64_kernel<false>)
  softmax_Q3 / Q5 / Q6 / Q7                     64 @ 24x32, 32x40, 32x48, 28x64 x 1, fp32: softmax_rows_reg_kernel<3>, <5>, <6>, <7>
  softmax_generic_1088                          64 @ 32x34 x 1, fp32: the generic softmax_rows_kernel at T > 256
  groups_65    128 @ 32x64 x 65, G = 4          the image-group loop of attention_conv (f16x3: plans qk[1] / pv[1], the per-group offsets into q_tab,
                                                k_inv, wk, wv, x, out_stat) and of attention_small (fp32: bgemm64 at n0 = 64): 64 images + a last group of 1
  every fp32 case                               the all-fp32 bgemm64 path in the peaked regime

Assertions: accurate modes (fp32, f16x3, f16mx): branch rel-L2 < max(1e-4, 10 r64), r64 = the fp32 oracle's own distance from fp64 on the case, and no
class (attn_ref.classes) above twice the whole tensor's error or ten times the fp32 oracle's own error in that class (attn_ref.check_accurate); at G = 64 the one-hot queries equal v'[arg-max] to 2^-20.  Reduced modes (f16, bf16;
G <= 8): GPU vs exact within [E / 2, 2 E], GPU vs emulation <= E (E = emulation vs exact), every class ratio within [0.5, 2] of the band around the
emulation's own ratio of that class.  A permutation of the pixels commutes with the block.  Measured figures: DESIGN.md.
"""
import pytest
import torch

import attn_ref as ar
from conftest import rel_l2
from drmnet_amd import ops
from quant_ref import class_ratios
from test_gpu_upconv import profiled

pytestmark = pytest.mark.gpu
ACCURATE = ("fp32", "f16x3", "f16mx")
ROW_BAR = 1e-6  # "a row equals its own single run" in the accurate modes (tests/test_gpu_attn_flash.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def run(P, x, mode, dev):
    """-> (out on the CPU, the attention cores the profiler saw)"""
    try:
        ops.set_precision(mode)
        params = [p.to(dev) for p in P.values()]
        xd = x.to(dev)
        out, names = profiled(lambda: ops.attention_block(params, xd))
        return out.cpu(), sorted(nm for nm in names if nm.startswith("drm::attn_core<"))
    finally:
        ops.set_precision("fp32")


def one_hot_error(case, b_gpu):
    """rel-L2 of the branch against v'[arg-max] over the queries whose fp64 largest probability exceeds 1 - 1e-6, and their count"""
    pm, am = ar.pmax_argmax(case)
    sel = pm > 1.0 - 1e-6
    want = torch.gather(case.v, 1, am[..., None].expand(-1, -1, case.C))
    got = b_gpu.reshape(case.N, case.C, case.T).transpose(1, 2)
    return rel_l2(got[sel], want[sel]), int(sel.sum())


def assert_accurate(label, case, out, mode, rows=None):
    fails, e = ar.check_accurate(case, out, rows)
    print(f"{label} ({mode}): branch rel-L2 vs fp64 {e:.2e} (bar {ar.accurate_bar(case):.1e}, r64 {ar.r64(case):.2e})")
    if case.gain == 64:
        e1, cnt = one_hot_error(case, ar.branch(case, out if rows is None else out[rows]))
        print(f"{label} ({mode}): {cnt} one-hot queries are {e1:.2e} from v'[arg-max] (bar 2^-20 = {2.0 ** -20:.2e})")
        if not (cnt > 0 and e1 < 2.0 ** -20):  # the 22-bit split of v' with two bits of margin for the fp32 epilogue
            fails.append(f"{cnt} one-hot queries: {e1:.3e} from v'[arg-max]")
    assert not fails, fails


@pytest.mark.parametrize("name,gain,mode", [c for c in ar.gpu_cases() if c[2] in ACCURATE])
def test_peaked_block_accurate_modes(dev, name, gain, mode):
    c, case = ar.CASES[name], ar.named_case(name, gain)
    out, cores = run(case.P, case.x, mode, dev)
    assert cores == [ar.variant(c["form"], mode, case.C, case.T)], cores
    assert_accurate(f"{name} G={gain}", case, out, mode)


@pytest.mark.parametrize("name,gain,mode", [c for c in ar.gpu_cases() if c[2] in ar.REDUCED])
def test_peaked_block_reduced_modes(dev, name, gain, mode):
    c, case = ar.CASES[name], ar.named_case(name, gain)
    out, cores = run(case.P, case.x, mode, dev)
    assert cores == [ar.variant(c["form"], mode, case.C, case.T)], cores
    b_gpu, b_ref, b_em = ar.branch(case, out), ar.branch(case, ar.exact(case)), ar.branch(case, ar.emulate(case, mode, c["form"]))
    E, e_exact, e_emul = rel_l2(b_em, b_ref), rel_l2(b_gpu, b_ref), rel_l2(b_gpu, b_em)
    cls = ar.classes(case)
    r_gpu, r_em = class_ratios(b_gpu, b_ref, cls), class_ratios(b_em, b_ref, cls)
    rel = {nm: r_gpu[nm] / max(r_em[nm], 1e-300) for nm in cls}
    print(f"{name} G={gain} ({mode}): E {E:.2e}, GPU vs exact {e_exact:.2e} = {e_exact / E:.2f} E, GPU vs emulation {e_emul:.2e} = {e_emul / E:.2f} E; class ratios "
          f"[{min(r_gpu.values()):.2f}, {max(r_gpu.values()):.2f}] (emulation [{min(r_em.values()):.2f}, {max(r_em.values()):.2f}]), GPU / emulation per class "
          f"[{min(rel.values()):.2f}, {max(rel.values()):.2f}]")
    assert torch.isfinite(out).all()
    assert E / 2 <= e_exact <= 2 * E
    assert e_emul <= E
    bad = [f"class {nm}: ratio {r:.3f} outside [{lo:.2f}, {hi:.2f}] (emulation {r_em[nm]:.3f})" for nm, r in r_gpu.items()
           for lo, hi in [ar.class_band(r_em[nm])] if not lo <= r <= hi]
    assert not bad, bad


@pytest.mark.parametrize("name", list(ar.SOFTMAX_Q))
def test_row_softmax_kernels_fp32(dev, name):
    """the fp32 three-launch form at T = 768, 1280, 1536, 1792 (the register row softmax, Q = 3, 5, 6, 7) and T = 1088 (the generic one)"""
    h, w = ar.SOFTMAX_Q[name]
    case = ar.block_case(ar.SOFTMAX_Q_C, h, w, 1, ar.SOFTMAX_Q_GAIN)
    out, cores = run(case.P, case.x, "fp32", dev)
    assert cores == ["drm::attn_core<small, 0, 0, 0, 1>"], cores
    assert_accurate(f"{name} T={case.T}", case, out, "fp32")


@pytest.mark.parametrize("mode", ar.GROUPS["modes"])
def test_image_groups_65(dev, mode):
    """64 images fill the 1 GiB score buffer at T = 2048, image 64 is a short last group.  Rows 0, 63, 64 against fp64; rows 1 .. 62 are copies of
    rows 0 and 63 alternately and must equal them at the row bar."""
    g = ar.GROUPS
    case = ar.block_case(g["C"], g["H"], g["W"], 3, g["gain"])
    x, src = ar.groups_batch(case, g["N"])
    out, cores = run(case.P, x, mode, dev)
    assert cores == [ar.variant("conv", mode, case.C, case.T, passes=2)], cores
    assert torch.isfinite(out).all()
    assert_accurate(f"groups_65 G={g['gain']}", case, out, mode, rows=[0, g["N"] - 2, g["N"] - 1])
    first = {0: 0, 1: g["N"] - 2}
    worst = max(rel_l2(out[i], out[first[s]]) for i, s in src.items() if i not in (0, g["N"] - 2, g["N"] - 1))
    print(f"groups_65 ({mode}): copies differ from their originals by at most {worst:.1e}")
    assert worst < ROW_BAR


@pytest.mark.parametrize("name,gain", [("flash_1024", 64), ("conv_512", 8), ("small_256", 8)])
def test_pixel_permutation_commutes(dev, name, gain):
    """GroupNorm, the 1x1 projections and attention commute with a permutation of the H W positions: block(x[..., perm]) == block(x)[..., perm].
    The permutation moves every query's arg-max key to another place and changes which key tiles raise the running maximum."""
    c, case = ar.CASES[name], ar.named_case(name, gain)
    perm = torch.randperm(case.T, generator=torch.Generator().manual_seed(3))
    am = ar.pmax_argmax(case)[1]
    inv = torch.argsort(perm)
    moved = float(((inv[am] // 32) != (am // 32)).double().mean())  # (the key's new position: where perm[j] = its old one)
    assert moved > 0.8, moved  # (a random place is another 32-key block with probability 1 - 32 / T >= 0.875)
    flat = lambda t: t.reshape(case.N, case.C, case.T)
    xp = flat(case.x)[:, :, perm].reshape(case.x.shape).contiguous()
    out, cores = run(case.P, case.x, "f16x3", dev)
    outp, coresp = run(case.P, xp, "f16x3", dev)
    assert cores == coresp == [ar.variant(c["form"], "f16x3", case.C, case.T)], (cores, coresp)
    e = rel_l2(flat(outp), flat(out)[:, :, perm])
    print(f"{name} G={gain}: block(x[perm]) vs block(x)[perm] {e:.1e}")
    assert e < ROW_BAR

"""Bit-exact conv and linear checks on dyadic inputs (tests/quant_ref.py (a), DESIGN.md "Exact and emulated conv checks").

x in {k/8 : |k| <= 16}, w in {k/32 : |k| <= 16}: every product and every partial sum is an fp32 number (quant_ref.exact_bits, at most 22 of 24 bits),
the operands are fp16 and bf16 numbers, the weight pre-scale and the per-image range guard are powers of two, the epilogue adds dyadic terms.  So
ops.norm_act_conv (no GroupNorm, no SiLU) must EQUAL the fp64 reference in fp32, f16x3, f16 and bf16, on conv_split2_kernel and on conv_igemm_kernel,
whatever the accumulation order: an addressing, masking, ring, halo, tile or padding error shows as a mismatch at a named element, in the reduced
modes as sharply as in fp32.  tests/test_quant_ref_cpu.py checks on the CPU that every case keeps the premise.

Each case asserts through the library profiler which kernel ran: the TERMS template argument of conv_split2_kernel (0 / 3 / 1 / 4), or -- where
plan_conv sends the shape to conv_igemm_kernel, the only other conv kernel -- that no conv_split2_kernel instantiation ran.
"""
import re

import pytest
import torch

import quant_ref as q
from test_gpu_upconv import profiled

MODES = ["fp32", "f16x3", "f16", "bf16"]
PREFIX = "void drm::conv_split2_kernel<"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def terms_that_ran(names):
    """the TERMS template argument (the 10th) of every conv_split2_kernel instantiation that ran"""
    return {int(re.match(r"(?:\w+, ){9}(\d+), ", nm[len(PREFIX):]).group(1)) for nm in names if nm.startswith(PREFIX)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(q.EXACT_CASES))
def test_conv_equals_the_fp64_reference(dev, name, mode):
    from drmnet_amd import ops

    n, cin, cout, h, w, k, extras = q.EXACT_CASES[name]
    x, wt, bias, emb, res, ref = q.exact_case(name)
    d = lambda t: None if t is None else t.to(dev)
    try:
        ops.set_precision(mode)
        out, names = profiled(lambda: ops.norm_act_conv(d(x), d(wt), d(bias), emb=d(emb), residual=d(res)))
    finally:
        ops.set_precision("fp32")
    ran = terms_that_ran(names)
    print(f"{name} {mode}: {q.exact_case_bits(name)} bits, conv_split2_kernel TERMS {sorted(ran)}")
    if q.igemm_expected(name, mode):
        assert not ran, names  # conv_igemm_kernel
    else:
        assert ran == {q.TERMS[mode]}, names
    want = ref.float().to(dev)
    assert out.shape == want.shape
    if not torch.equal(out, want):
        cls = q.classes(n, cout, h, w, 1) if out.numel() <= 1 << 21 else None  # (the masks of the largest maps would not fit)
        pytest.fail(f"{name} {mode}: {q.first_mismatch(out, ref, cls)}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,i,o,kernel", q.LINEAR_CASES, ids=[f"{n}x{i}x{o}" for n, i, o, _ in q.LINEAR_CASES])
def test_linear_equals_the_fp64_reference(dev, n, i, o, kernel):
    """launch_linear (csrc/misc.hip) picks `kernel` from (n, i): linear_rows_kernel for n <= 4 and i % 16 == 0, linear_mfma_kernel for other
    i % 16 == 0, linear_kernel for the rest (i = 6, 100).  All three accumulate fp32 products: exact here."""
    from drmnet_amd import ops

    x, wt, b, ref = q.linear_case(n, i, o)
    out = ops.linear(x.to(dev), wt.to(dev), b.to(dev)).cpu()
    assert torch.equal(out, ref.float()), f"{kernel} {n}x{i}->{o}: {q.first_mismatch(out[:, :, None, None], ref[:, :, None, None])}"

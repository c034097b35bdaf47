"""The stem, the 2x2 average pool and RefNet's pooled head against plain fp64 references, through their per-module entry points (ops.stem_conv,
ops.avgpool2, ops.encoder_head).  tests/boundary_ref.py holds the references, the input families, the bounds and the mutants;
tests/test_boundary_ref_cpu.py shows on the CPU that the premises hold, that correct arithmetic stays inside the bounds and that every mutant
fails a case below; DESIGN.md "Boundary-kernel checks" has the measured figures.

Stem     torch.equal against the fp64 reference on the exact family, in the exact fp32 form and the fp16 hi / lo split, for CIN = 6 and both
         CIN = 4 layouts: whole, small, ragged and barely-ragged maps, a persistent launch whose workgroups own two tiles of one image or cross
         an image boundary, the row gather, the per-tile range guard (2^-40 and 2^40 in one image), NaN / Inf poison.  Tables: exactly the fp64
         sums on the narrow family; the GroupNorm criterion on the offset families.
Pool     equality on the exact family, three roundings on the offset family, tables as for the stem; the launch variant of each shape printed.
Head     the elementwise bound derived from the kernel's arithmetic.
Every test asserts through the library profiler which kernel ran.

Measured on the MI355X (worst error / bound): with raw fp32 sums of v and v * v per lane / thread, as the two kernels had them, the one-sign
offset cases stood at 6.11 / 6.48 (stem, fp32 / f16x3), 1.22 (pool, 8 pixels per thread) and 12.76 (pool, 64 pixels per thread); about a pivot
they stand at 0.032, 0.008 and 0.004 at most.  The alternating-sign cases were at 0.04 before and are at 0.009 at most; the head is at 0.038.
"""
import pytest
import torch

import boundary_ref as R
import gn_ref as G
from quant_ref import first_mismatch
from test_gpu_upconv import profiled

FORMS = {"fp32": "true", "f16x3": "false"}  # op precision -> the EXACT template argument of stem_conv_kernel
CH = R.STEM_CH
CH_IDS = [f"cx{a}cc{b}" for a, b in CH]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no fallback)"
    return torch.device("cuda:0")


def run_stem(dev, mode, x, cond, wt, b, rows=None, stats=False):
    """ops.stem_conv in `mode` under the profiler; asserts that the instantiation of (Cx + Cc, mode) ran once -> out (, table) on the CPU"""
    from drmnet_amd import ops

    r = None if rows is None else torch.as_tensor(rows, dtype=torch.int32).to(dev)
    try:
        ops.set_precision(mode)
        res, names = profiled(lambda: ops.stem_conv(x.to(dev), cond.to(dev), wt.to(dev), None if b is None else b.to(dev), rows=r, want_stats=stats))
    finally:
        ops.set_precision("fp32")
    want = f"drm::stem_conv_kernel<{x.shape[1] + cond.shape[1]}, {FORMS[mode]}>"
    assert names.get(want) == 1 and sum(v for k, v in names.items() if "stem_conv_kernel" in k) == 1, names
    return (res[0].cpu(), res[1].cpu()) if stats else res.cpu()


def assert_equal(out, ref):
    bad = first_mismatch(out, ref.float())
    assert bad is None, str(bad)


def assert_tables_exact(stat, out):
    want = R.tables64(out)
    bad = (stat != want).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} of {stat.numel()} table entries differ from the fp64 sums of the returned output; first at (n, c, moment) = "
                              f"{tuple(int(v) for v in bad[0])}: got {float(stat[tuple(bad[0])])!r}, want {float(want[tuple(bad[0])])!r}")


# ------------------------------------------------------------------------------------------------ stem: equality

@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
@pytest.mark.parametrize("name", list(R.STEM_SHAPES))
def test_stem_equals_reference(dev, name, cx, cc, mode):
    n, h, w = R.STEM_SHAPES[name]
    args = R.stem_inputs(R.EXACT, n, cx, cc, h, w)
    assert_equal(run_stem(dev, mode, *args), R.stem_ref64(*args))


_PERSISTENT = {}


def persistent_case(fam, cx, cc, cus):
    """(inputs, reference fp64 cast to fp32, N): computed once per family and channel split, shared by the modes, never modified"""
    key = (id(fam), cx, cc, cus)
    if key not in _PERSISTENT:
        h, w = R.PERSISTENT_HW
        n = R.persistent_n(cus)
        ranges = R.stem_ranges(n, h, w, cus)
        same, cross = R.range_kinds(ranges, R.stem_tiles(h, w))
        assert len(ranges) == 2 * cus and same >= 1 and cross >= 1, (n, same, cross)  # the kernel's own range rule, on this device's CU count
        args = R.stem_inputs(fam, n, cx, cc, h, w)
        _PERSISTENT[key] = (args, R.stem_ref64(*args).float(), n)
    return _PERSISTENT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
def test_stem_persistent_ranges(dev, cx, cc, mode):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    args, ref, n = persistent_case(R.EXACT, cx, cc, cus)
    assert_equal(run_stem(dev, mode, *args), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
def test_stem_row_gather(dev, cx, cc, mode):
    _, h, w = R.STEM_SHAPES["ragged"]
    x, cond, wt, b = R.stem_inputs(R.NARROW, R.ROWS_B, cx, cc, h, w)
    out, stat = run_stem(dev, mode, x, cond, wt, b, rows=R.ROWS, stats=True)
    assert_equal(out, R.stem_ref64(x, cond, wt, b, rows=R.ROWS))
    dense, dstat = run_stem(dev, mode, x[R.ROWS], cond[R.ROWS], wt, b, stats=True)
    assert torch.equal(out, dense) and torch.equal(stat, dstat)
    assert_tables_exact(stat, out)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
def test_stem_guard_is_per_tile(dev, cx, cc, mode):
    x, cond, wt, ref = R.guard_case(cx, cc)
    out = run_stem(dev, mode, x, cond, wt, None)
    assert_equal(out, ref)
    assert bool((out[:, :, :, 17:47] == 0).all()) and bool((out[:, :, :, :16] != 0).any())  # the zero tiles, and the 2^-40 tile's bits kept


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
def test_stem_poison_stays_in_its_window(dev, cx, cc, poison, mode):
    n, h, w = R.STEM_SHAPES["ragged"]
    x, cond, wt, b = R.stem_inputs(R.NARROW, n, cx, cc, h, w)
    ref = R.stem_ref64(x, cond, wt, b).float()
    py, px = 7, 16  # the window rows 6 .. 8, columns 15 .. 17 lies in four tiles
    x, cond = x.clone(), cond.clone()
    if poison != poison:
        x[1, 0, py, px] = poison
    else:
        cond[1, cc - 1, py, px] = poison
    out, stat = run_stem(dev, mode, x, cond, wt, b, stats=True)
    hit = torch.zeros_like(out, dtype=torch.bool)
    hit[1, :, py - 1:py + 2, px - 1:px + 2] = True
    assert not bool(torch.isfinite(out[hit]).any()), "a poisoned window produced a finite output"
    bad = first_mismatch(torch.where(hit, ref, out), ref)
    assert bad is None, str(bad)
    assert_tables_exact(stat[[0, 2]], out[[0, 2]])
    assert not bool(torch.isfinite(stat[1]).any())


# ------------------------------------------------------------------------------------------------ stem: tables

@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
@pytest.mark.parametrize("rows", [False, True], ids=["dense", "rows"])
@pytest.mark.parametrize("case", ["ragged", "persistent"])
def test_stem_tables_are_exact_on_the_narrow_family(dev, case, rows, cx, cc, mode):
    if case == "ragged":
        n, h, w = R.STEM_SHAPES["ragged"]
        args = R.stem_inputs(R.NARROW, n + 2 if rows else n, cx, cc, h, w)
    else:
        args, _, n = persistent_case(R.NARROW, cx, cc, torch.cuda.get_device_properties(0).multi_processor_count)
    r = None
    if rows:  # a permutation with repeats of the B rows, N long
        b_rows = args[0].shape[0]
        r = [int(v) for v in torch.randint(0, b_rows, (n,), generator=torch.Generator().manual_seed(n + cx))]
    out, stat = run_stem(dev, mode, *args, rows=r, stats=True)
    if case == "ragged":
        assert_equal(out, R.stem_ref64(*args, rows=r))
    assert_tables_exact(stat, out)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FORMS))
@pytest.mark.parametrize("same_sign", [False, True], ids=["alternating", "one_sign"])
@pytest.mark.parametrize("cx,cc", CH, ids=CH_IDS)
def test_stem_tables_offset_family(dev, cx, cc, same_sign, mode):
    n, h, w = R.OFFSET_SHAPE
    args = R.offset_stem_inputs(n, cx, cc, h, w, same_sign=same_sign)
    out, stat = run_stem(dev, mode, *args, stats=True)
    # the outputs themselves are the equality tests' business; here: 9 Cin + 2 fp32 roundings and the split's dropped lo x lo terms, on sum |x w| + |b|
    lim = ((9 * (cx + cc) + 2) * R.U + 2.0 ** -21) * R.stem_ref64(*[t.abs() for t in args])
    assert G.first_outside((out.double() - R.stem_ref64(*args)).abs(), lim) is None
    err, bnd = R.table_criterion(out, stat)
    print(f"stem tables {'one sign' if same_sign else 'alternating'} cx{cx} cc{cc} {mode}: worst error / bound {G.worst_ratio(err, bnd):.3f}")
    bad = G.first_outside(err, bnd)
    assert bad is None, f"{bad[0]} of {err.numel()} elements outside the bound; first at {bad[1]}: error {bad[2]:.3e} > bound {bad[3]:.3e}; worst error / bound {G.worst_ratio(err, bnd):.2f}"


# ------------------------------------------------------------------------------------------------ pooling

def run_pool(dev, x, stats):
    from drmnet_amd import ops

    res, names = profiled(lambda: ops.avgpool2(x.to(dev), want_stats=stats))
    assert names.get("drm::avgpool2_kernel") == 1, names
    return (res[0].cpu(), res[1].cpu()) if stats else (res.cpu(), None)


def check_criterion(what, out, stat):
    err, bnd = R.table_criterion(out, stat)
    print(f"{what}: worst error / bound {G.worst_ratio(err, bnd):.3f}")
    bad = G.first_outside(err, bnd)
    assert bad is None, f"{what}: {bad[0]} of {err.numel()} elements outside the bound; first at {bad[1]}: error {bad[2]:.3e} > bound {bad[3]:.3e}; worst error / bound {G.worst_ratio(err, bnd):.2f}"


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "table"])
@pytest.mark.parametrize("shape", R.POOL_SHAPES + R.POOL_LONG[:1], ids=lambda s: "x".join(str(v) for v in s))
def test_pool(dev, shape, stats):
    print(f"avgpool2 {shape}: (QL, px_per_block, passes, pixels per thread) = {R.avgpool2_launch(*shape)}")
    x = R.pool_inputs(R.EXACT, *shape)
    out, _ = run_pool(dev, x, stats)
    assert_equal(out, R.pool_ref64(x))
    if stats:
        x = R.pool_inputs(R.NARROW, *shape)
        out, stat = run_pool(dev, x, True)
        assert_equal(out, R.pool_ref64(x))
        assert_tables_exact(stat, out)
    for same in (False, True):
        x = R.offset_pool_input(*shape, same_sign=same)
        out, stat = run_pool(dev, x, stats)
        bad = G.first_outside((out.double() - R.pool_ref64(x)).abs(), R.pool_out_bound(x))
        assert bad is None, f"{bad[0]} outputs outside three roundings; first at {bad[1]}: error {bad[2]:.3e} > bound {bad[3]:.3e}"
        if stats:
            check_criterion(f"pool tables {shape} {'one sign' if same else 'alternating'}", out, stat)


@pytest.mark.gpu
def test_pool_full_launch_tables(dev):
    """the smallest launch at which no sparse rule fires: 256 workgroups, a thread adds 64 pixels (what the 128 x 256 maps of the networks run)"""
    shape = R.POOL_LONG[1]
    assert R.avgpool2_launch(*shape) == (64, 256, 1, 64)
    x = R.offset_pool_input(*shape, same_sign=True)
    out, stat = run_pool(dev, x, True)
    assert torch.equal(out, torch.nn.functional.avg_pool2d(x, 2))  # (values on the 2^-10 grid: the fp32 pool is exact, as the small cases show)
    check_criterion(f"pool tables {shape} one sign", out, stat)


# ------------------------------------------------------------------------------------------------ encoder head

@pytest.mark.gpu
@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_encoder_head(dev, shape, offset):
    from drmnet_amd import ops

    args = R.head_inputs(*shape, offset)
    out, names = profiled(lambda: ops.encoder_head(*[t.to(dev) for t in args]).cpu())
    assert names.get("drm::encoder_head_kernel") == 1, names
    ref, bnd = R.head_ref64(*args), R.head_bound(*args)
    err = (out.double() - ref).abs()
    print(f"head {shape} {'offset' if offset else 'plain'}: worst error / bound {G.worst_ratio(err, bnd):.3f}")
    bad = G.first_outside(err, bnd)
    assert bad is None, f"{bad[0]} of {err.numel()} outputs outside the bound; first at (n, o) = {bad[1]}: error {bad[2]:.3e} > bound {bad[3]:.3e}"

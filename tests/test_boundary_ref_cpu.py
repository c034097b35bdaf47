"""What tests/test_gpu_boundary.py rests on, shown without a GPU (tests/boundary_ref.py): the premises of the exact and the narrow family for every
case the GPU tests run, the bounds on emulated correct arithmetic, every mutant leaving its check on a named case, and the prediction of what raw
fp32 moments cost the stem's and the pool's tables against the GroupNorm bound."""
import ctypes as C

import pytest
import torch

import boundary_ref as R
import gn_ref as G

CUS = 256  # the device shape the persistent case is sized for on the CPU (the GPU test reads the device's own count)


def exact32(t):
    return bool((t.float().double() == t).all())


# ------------------------------------------------------------------------------------------------ premises

def test_family_premises():
    for cx, cc in R.STEM_CH:
        assert R.family_bits(R.EXACT, cx + cc) <= 14 and R.family_bits(R.NARROW, cx + cc) <= 9
        assert R.narrow_bits(32, cx + cc) <= 24  # a stem lane: two 16-value accumulator blocks of one channel
        assert R.narrow_bits(64, cx + cc) <= 24  # (and twice that)
    assert R.narrow_bits(64, pooled=True) <= 24  # a pooling thread: 256-pixel blocks on 4 pixel lanes
    # the limits were chosen, not assumed: x up to |k| = 4 with w up to |k| = 2 needs 26 bits about a pivot
    wide = dict(R.NARROW, x_k=4)
    vmax = 54 * wide["x_step"] * wide["x_k"] * wide["w_step"] * wide["w_k"] + 1.0
    assert 32 * (2 * vmax) ** 2 * 64 > 2 ** 24


@pytest.mark.parametrize("cx,cc", R.STEM_CH)
@pytest.mark.parametrize("name", list(R.STEM_SHAPES))
def test_exact_family_references_are_fp32_numbers(name, cx, cc):
    n, h, w = R.STEM_SHAPES[name]
    ref = R.stem_ref64(*R.stem_inputs(R.EXACT, n, cx, cc, h, w))
    assert exact32(ref) and float(ref.abs().max()) <= 56.0


def test_guard_case_reference_is_exact_in_fp32():
    x, cond, wt, ref = R.guard_case(3, 3)
    assert exact32(ref) and float(ref[ref != 0].abs().min()) < 2.0 ** -40 and float(ref.abs().max()) > 2.0 ** 40


def narrow_table_cases():
    h, w = R.PERSISTENT_HW
    yield "ragged", R.STEM_SHAPES["ragged"], None
    yield "persistent", (R.persistent_n(CUS) // 8, h, w), None  # (the arithmetic per lane is the same at any batch)
    yield "rows", (R.ROWS_B,) + R.STEM_SHAPES["ragged"][1:], R.ROWS


@pytest.mark.parametrize("cx,cc", R.STEM_CH)
def test_narrow_family_tables_are_exact_in_any_order(cx, cc):
    for name, (n, h, w), rows in narrow_table_cases():
        out = R.stem_ref64(*R.stem_inputs(R.NARROW, n, cx, cc, h, w), rows=rows)
        assert exact32(out) and float(out.abs().max()) <= 28.0
        want = R.tables64(out)
        for per in (16, 32):
            assert torch.equal(R.lane_tables(out, per), want), (name, per)
            assert torch.equal(R.pivot_lane_tables(out, per), want), (name, per)
    for shape in R.POOL_SHAPES + R.POOL_LONG[:1]:
        out = R.pool_ref64(R.pool_inputs(R.NARROW, *shape))
        assert exact32(out)
        for per in (1, 8, 64):
            assert torch.equal(R.lane_tables(out, per), R.tables64(out)) and torch.equal(R.pivot_lane_tables(out, per), R.tables64(out)), (shape, per)


def test_pool_exact_family_is_exact():
    for shape in R.POOL_SHAPES:
        x = R.pool_inputs(R.EXACT, *shape)
        assert exact32(R.pool_ref64(x))
        assert torch.equal(torch.nn.functional.avg_pool2d(x, 2).double(), R.pool_ref64(x))  # fp32 arithmetic gets it exactly


def test_persistent_ranges_hold_both_kinds():
    h, w = R.PERSISTENT_HW
    n = R.persistent_n(CUS)
    assert n == 86 and R.stem_tiles(h, w) == 9
    ranges = R.stem_ranges(n, h, w, CUS)
    same, cross = R.range_kinds(ranges, 9)
    assert len(ranges) == 2 * CUS and same >= 1 and cross >= 1, (same, cross)
    assert ranges[0][0] == 0 and ranges[-1][1] == n * 9 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_pool_launch_rule_covers_the_variants():
    got = {s: R.avgpool2_launch(*s) for s in R.POOL_SHAPES + R.POOL_LONG}
    for s, v in got.items():
        print(f"avgpool2 {s}: (QL, px_per_block, passes, pixels per thread) = {v}")
    assert got[(2, 192, 12, 20)] == (8, 32, 6, 1) and got[(1, 1024, 8, 16)] == (8, 32, 32, 1)  # lanes narrowed, blocks shortened
    assert got[(1, 32, 128, 128)] == (8, 256, 1, 8) and got[(4, 256, 256, 256)] == (64, 256, 1, 64)  # long walks; the last: no sparse rule fires
    # no listed shape lets a thread add more than one pixel: the fp32 sums of the issue show only at POOL_LONG
    assert all(got[s][3] == 1 for s in R.POOL_SHAPES)


# ------------------------------------------------------------------------------------------------ the table criterion: prediction and the pivot

def _ratio(out, stat):
    err, bnd = R.table_criterion(out, stat)
    return G.worst_ratio(err, bnd)


def test_offset_tables_prediction_and_pivot():
    n, h, w = R.OFFSET_SHAPE
    raws = {}
    for same in (False, True):
        out = R.stem_ref64(*R.offset_stem_inputs(n, 3, 3, h, w, same_sign=same)).float()  # what a correct kernel returns, to a rounding
        pooled = R.pool_ref64(R.offset_pool_input(2, 64, 64, 64, same_sign=same)).float()
        for name, t, per in (("stem, 32 per lane", out, 32), ("pool, 1 pixel per thread", pooled, 1), ("pool, 8 pixels per thread", pooled, 8),
                             ("pool, 64 pixels per thread", pooled, 64)):
            exact = _ratio(t, R.tables64(t))
            raws[name, same] = raw = _ratio(t, R.lane_tables(t, per))
            piv = _ratio(t, R.pivot_lane_tables(t, per))
            print(f"predicted worst error / bound, offsets of {'one sign' if same else 'alternating sign'}, {name}: raw fp32 moments {raw:.2f}, "
                  f"about a pivot {piv:.3f}, exact tables {exact:.3f}")
            assert exact < 0.01 and piv <= 0.1, (name, same, exact, piv)
    # (what the raw form costs is the prediction, printed and not asserted; that the family matters is: same-sign groups are the sharp case)
    assert raws["stem, 32 per lane", True] > 10 * raws["stem, 32 per lane", False]


# ------------------------------------------------------------------------------------------------ encoder head

@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_head_emulation_stays_inside_the_bound(shape, offset):
    args = R.head_inputs(*shape, offset)
    ref, bnd = R.head_ref64(*args), R.head_bound(*args)
    err = (R.head_emulate32(*args).double() - ref).abs()
    print(f"head {shape} offset={offset}: emulated worst error / bound {G.worst_ratio(err, bnd):.3f}")
    assert G.first_outside(err, bnd) is None
    assert float((bnd / ref.abs().clamp_min(1e-3)).max()) < 1e-2  # (the bound is no licence: far below the mutants' errors)


HEAD_MUTANT_CASE = {"divide_by_hw_minus_1": (3, 256, 6, 6), "last_channel_quad_dropped": (2, 132, 7, 5), "image0_scale": (2, 1024, 16, 6)}


@pytest.mark.parametrize("name", list(R.HEAD_MUTANTS))
def test_head_mutants_leave_the_bound(name):
    for offset in (False, True):
        args = R.head_inputs(*HEAD_MUTANT_CASE[name], offset)
        err = (R.HEAD_MUTANTS[name](*args) - R.head_ref64(*args)).abs()
        assert G.first_outside(err, R.head_bound(*args)) is not None, (name, offset)


# ------------------------------------------------------------------------------------------------ mutants of the stem and the pool

@pytest.mark.parametrize("cx,cc", R.STEM_CH)
def test_stem_output_mutants_fail_a_named_case(cx, cc):
    n, h, w = R.STEM_SHAPES["ragged"]
    args = R.stem_inputs(R.EXACT, n, cx, cc, h, w)
    ref = R.stem_ref64(*args)
    assert not torch.equal(R.m_tap_transposed(*args), ref)
    assert not torch.equal(R.m_clamped_padding(*args), ref)
    assert torch.equal(R.m_clamped_padding(*args)[:, :, 1:-1, 1:-1], ref[:, :, 1:-1, 1:-1])  # (wrong at the border only)
    rargs = R.stem_inputs(R.EXACT, R.ROWS_B, cx, cc, h, w)
    assert not torch.equal(R.m_gather_x_only(*rargs, R.ROWS), R.stem_ref64(*rargs, rows=R.ROWS))


def test_stem_table_mutants_fail_a_named_case():
    n, h, w = R.STEM_SHAPES["ragged"]
    args = R.stem_inputs(R.NARROW, n, 3, 3, h, w)
    assert not torch.equal(R.m_ragged_pixels_counted(*args), R.tables64(R.stem_ref64(*args)))
    for name in ("one_tile",):  # (whole tiles: nothing to miscount)
        a = R.stem_inputs(R.NARROW, *((R.STEM_SHAPES[name][0], 3, 3) + R.STEM_SHAPES[name][1:]))
        assert torch.equal(R.m_ragged_pixels_counted(*a), R.tables64(R.stem_ref64(*a)))
    hp, wp = R.PERSISTENT_HW
    out = R.stem_ref64(*R.stem_inputs(R.NARROW, 5, 3, 3, hp, wp))
    assert R.range_kinds(R.stem_ranges(5, hp, wp, 7), 9)[1] >= 1  # 45 tiles on 14 workgroups: ranges cross images
    assert not torch.equal(R.m_table_to_previous_image(out, 7), R.tables64(out))
    assert torch.equal(R.m_table_to_previous_image(out, 1000), R.tables64(out))  # one tile per workgroup: nothing to miscredit


def test_pool_mutant_fails_every_shape():
    for shape in R.POOL_SHAPES:
        x = R.pool_inputs(R.EXACT, *shape)
        assert not torch.equal(R.m_pool_shifted(x), R.pool_ref64(x))
        xo = R.offset_pool_input(*shape)
        assert G.first_outside((R.m_pool_shifted(xo) - R.pool_ref64(xo)).abs(), R.pool_out_bound(xo)) is not None


# ------------------------------------------------------------------------------------------------ the entry points reject by name

def test_entry_points_name_the_bad_argument():
    from drmnet_amd import _lib

    L = _lib.lib()
    buf = C.create_string_buffer(64)  # (never read: the arguments are rejected first)
    p = C.addressof(buf)
    assert L.drm_op_stem_conv(p, 3, p, 2, None, p, None, p, None, 1, 128, 8, 16, None) != 0
    assert b"Cx + Cc" in L.drm_last_error()
    assert L.drm_op_stem_conv(p, 3, p, 3, None, p, None, p, None, 1, 64, 8, 16, None) != 0
    assert b"Cout" in L.drm_last_error()
    assert L.drm_op_avgpool2(p, p, None, 1, 8, 6, 5, None) != 0
    assert b"H and W" in L.drm_last_error()
    assert L.drm_op_avgpool2(p, p, None, 1, 6, 4, 4, None) != 0
    assert b"C must be" in L.drm_last_error()
    assert L.drm_op_encoder_head(p, p, p, p, p, p, 1, 130, 2, 2, 6, None) != 0
    assert b"C must be" in L.drm_last_error()

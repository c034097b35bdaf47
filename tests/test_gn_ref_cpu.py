"""The yardstick of tests/test_gpu_groupnorm.py, checked on the CPU (tests/gn_ref.py; DESIGN.md "GroupNorm checks"):

  * the fp64 reference equals torch's float64 group_norm;
  * the bound is not too tight: an fp32 emulation of the table form with EXACT statistics stays inside it on every batch Probe A runs, in
    every mode, and torch's own CPU fp32 block stays inside the Probe B bound;
  * the bound is not too loose: every mutant group norm but the last leaves it on the case named for it in CATCHES -- the GPU tests would
    fail on that mistake;
  * the last mutant (sums and squares in fp32 per lane, the fused conv epilogue's arithmetic) is measured, not asserted: its error / bound
    ratio per family is the prediction DESIGN.md sets next to the measured fused-path value.
"""
import pytest
import torch
import torch.nn.functional as F

import gn_ref as G


@pytest.mark.parametrize("shape", G.PROBE_A)
def test_reference_equals_torch_float64(shape):
    n, c, h, w = shape
    gamma, beta = G.affine(c)
    for start in G.starts(n):
        x, fams = G.batch(n, c, h, w, start)
        gn = G.group_norm64(x, gamma, beta)
        want = F.group_norm(x.double(), G.GROUPS, gamma.double(), beta.double(), G.EPS)
        scale = 1.0 + (x.double() * gn.sc[:, :, None, None]).abs()  # (torch's fp64 error scales with the cancelled terms, as every GroupNorm's does)
        assert float(((gn.y - want).abs() / scale).max()) < 1e-12, fams
        # the tables restate y
        tab = x.double() * gn.sc[:, :, None, None] + gn.sh[:, :, None, None]
        assert float(((gn.y - tab).abs() / scale).max()) < 1e-12, fams
        # and the table route of the mutants, unmutated, is the reference
        m, q = G.chan_tables(x)
        assert float(((G._from_tables(x, m, q, gamma, beta) - gn.y).abs() / scale).max()) < 1e-9, fams


def test_concat_reference_equals_torch_float64():
    n, c0, c1, h, w = G.CONCAT
    x0, x1 = G.concat_inputs(n, c0, c1, h, w)
    gamma, beta = G.affine(c0 + c1)
    want = F.group_norm(torch.cat([G.upsample(x0), x1.double()], 1), G.GROUPS, gamma.double(), beta.double(), G.EPS)
    assert float((G.concat_norm64(x0, x1, gamma, beta).y - want).abs().max()) < 1e-12


def test_families_are_what_they_say():
    c, h, w = 64, 8, 8
    for fam in ("offset", "scales", "const", "per_image"):
        x, _ = G.batch(3, c, h, w, family=fam)
        assert bool((x.double() * 2.0 ** 16 == torch.round(x.double() * 2.0 ** 16)).all()), fam  # dyadic: exact in fp32
    x, _ = G.batch(1, c, h, w, family="offset")
    mean = x.double().mean((2, 3))[0]
    assert float((mean - G.offset_means(c)).abs().max()) < 0.5 and set(G.offset_means(c).abs().tolist()) == {8.0, 64.0}
    assert set(G.offset_means(32).tolist()) == {8.0, -8.0, 64.0, -64.0}  # one-channel groups see both signs of both magnitudes
    x, _ = G.batch(1, c, h, w, family="const")
    gm, gv = G.group_stats64(x)
    assert float(gv[0, 3]) == 0.0 and float(gm[0, 3]) == 2.0 and float(x[0, 3].std()) == 0.0
    x, fams = G.batch(6, c, h, w)
    assert fams == G.FAMILIES and float(x[3].abs().max()) == 0.0
    gamma, beta = G.affine(c)
    assert bool((gamma == 0).any()) and bool((gamma > 0).any()) and bool((gamma < 0).any())
    assert float(beta.abs().min()) >= 0.25 and bool((beta > 0).any()) and bool((beta < 0).any())
    assert sorted({f for n in (1, 2, 3, 5) for s in G.starts(n) for f in G.batch(n, 32, 4, 4, s)[1]}) == sorted(G.FAMILIES)


@pytest.mark.parametrize("shape", G.PROBE_A)
def test_fp32_table_form_with_exact_statistics_is_inside_the_bound(shape):
    n, c, h, w = shape
    gamma, beta = G.affine(c)
    for start in G.starts(n):
        x, fams = G.batch(n, c, h, w, start)
        gn = G.group_norm64(x, gamma, beta)
        y32 = G.table_form32(x, gn, gamma, beta)
        for mode in G.MODES:
            err, bnd = (G.stage(y32, mode) - gn.y).abs(), G.bound(x, gn.sc, gn.sh, gn.y, mode, beta)
            print(f"{shape} start {start} {mode}: worst error / bound {G.worst_ratio(err, bnd):.3f}")
            assert G.first_outside(err, bnd) is None, (fams, mode, G.first_outside(err, bnd))


SMALL_BLOCKS = ["prologue_128x32", "ragged", "split_in_launch", "split_reduce", "parity_prologue"]  # (the 64x64 multi-image ones cost seconds here)


@pytest.mark.parametrize("name", SMALL_BLOCKS)
def test_torch_fp32_block_is_inside_the_probe_b_bound(name):
    """the reference arithmetic in fp32 (torch's GroupNorm, conv and SiLU on the CPU) against the fp64 composition: inside the Probe B bound"""
    P, x0, x1, emb, ref, bnd = G.block_case(name, "fp32")
    h32, x32 = G._block(P, x0, x1, emb, torch.float32)
    a2 = G.silu(F.group_norm(h32, G.GROUPS, P["out_layers.0.weight"], P["out_layers.0.bias"], G.EPS))
    out = a2 + x32 if x32.shape[1] == a2.shape[1] else a2
    err = (out.double() - ref).abs()
    print(f"{name}: worst error / bound {G.worst_ratio(err, bnd):.3f}")
    assert G.first_outside(err, bnd) is None, G.first_outside(err, bnd)


# mutant -> the GPU case meant to catch it: ("A", shape, start of the batch) of Probe A, or ("B", block case, which GroupNorm) of Probe B
CATCHES = {
    "unbiased_variance": ("A", (3, 32, 4, 4), 3),  # 16 values per group: the variance is off by 1/15 (images: zero, per_image, plain)
    "eps_1e-6": ("A", (3, 32, 4, 4), 0),  # the scales image: one-channel groups with variance 2^-12, where eps weighs 4 %
    "eps_after_sqrt": ("A", (3, 32, 4, 4), 0),  # the same groups: std 2^-6, where eps after the root weighs 6e-4
    "group_off_by_one": ("A", (5, 192, 8, 8), 0),  # offset: neighbouring groups of magnitude 2^3 and 2^6
    "image0_table": ("A", (5, 192, 8, 8), 0),
    "last_channel_left_out": ("A", (2, 384, 10, 20), 0),  # cpg = 12: the lanes' second trip
    "concat_same_count": ("B", "parity_prologue", 1),
    "concat_boundary_source0": ("B", "parity_prologue", 1),
}


def test_every_mutant_has_a_case():
    assert set(CATCHES) == set(G.MUTANTS) - {G.MEASURED_ONLY}
    assert all(c[1] in G.PROBE_A for c in CATCHES.values() if c[0] == "A")
    assert all(c[1] in G.PROBE_B for c in CATCHES.values() if c[0] == "B")


@pytest.mark.parametrize("name", list(CATCHES))
def test_mutant_leaves_the_bound_on_its_case(name):
    probe, case, arg = CATCHES[name]
    kind, fn = G.MUTANTS[name]
    if probe == "A":
        assert kind == "single"
        n, c, h, w = case
        assert arg in G.starts(n)
        gamma, beta = G.affine(c)
        x, fams = G.batch(n, c, h, w, arg)
        gn = G.group_norm64(x, gamma, beta)
        err = (fn(x, gamma, beta) - gn.y).abs()
        for mode in G.MODES:  # the widest bound (bf16) is the hardest to leave
            bnd = G.bound(x, gn.sc, gn.sh, gn.y, mode, beta)
            print(f"{name} on {case} {fams} {mode}: worst error / bound {G.worst_ratio(err, bnd):.1f}")
            assert G.first_outside(err, bnd) is not None, (name, mode)
    else:
        assert kind == "concat" and arg == 1
        for mode in G.PROBE_B[case][7]:
            _, _, _, _, ref, bnd = G.block_case(case, mode)
            err = (G.block_forward64(case, gn1=fn) - ref).abs()
            print(f"{name} on {case} {mode}: worst error / bound {G.worst_ratio(err, bnd):.1f}")
            assert G.first_outside(err, bnd) is not None, (name, mode)


def test_fp32_squares_prediction():
    """Measured, not asserted (the assertion is the GPU test's): what sums and squares in fp32 per 8 values cost against the bound, per
    family on the Probe A shapes (as if their statistics came from the fused epilogue), and on the Probe B blocks, whose GN2 does read them."""
    kind, fn = G.MUTANTS[G.MEASURED_ONLY]
    worst = {}
    for n, c, h, w in G.PROBE_A:
        gamma, beta = G.affine(c)
        for fam in G.FAMILIES:
            x, _ = G.batch(n, c, h, w, family=fam)
            gn = G.group_norm64(x, gamma, beta)
            r = G.worst_ratio((fn(x, gamma, beta) - gn.y).abs(), G.bound(x, gn.sc, gn.sh, gn.y, "fp32", beta))
            worst[fam] = max(worst.get(fam, 0.0), r)
            print(f"fp32_squares, Probe A shape {(n, c, h, w)}, {fam}: worst error / bound {r:.3f}")
    for fam, r in worst.items():
        print(f"fp32_squares, {fam}: worst error / bound over the shapes {r:.3f}")
    for name in SMALL_BLOCKS:
        _, _, _, _, ref, bnd = G.block_case(name, "fp32")
        r = G.worst_ratio((G.block_forward64(name, gn2=fn) - ref).abs(), bnd)
        print(f"fp32_squares as GN2 of block {name}: worst error / bound {r:.3f}")
        assert r == r  # (finite)

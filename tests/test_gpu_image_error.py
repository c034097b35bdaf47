"""The batched image errors on the GPU (csrc/image_error.hip through drmnet_amd.relight) against the float64 restatement
tests/image_error_ref.py and the host path relight.image_errors, and what is built on them: the all-pairs distances, N draws of one image
(estimate.estimate_samples), their ranking (drmnet_amd/samples.py) and ``estimate --num_samples``.

The bar, |got - want| <= 1e-10 |want| + 1e-12 on every figure with the counts exact (image_error_ref.difference), is derived, not measured:
every term of a sum is a non-negative fp64 value rounded at most twice, so two orders of adding n <= 3 * 97 * 131 terms differ by at most about
2 (n + 2) 2^-53 = 8.5e-12 relative, which the square root halves; d = log10 a - log10 b carries a few ulps of |log10| <= 4, about 4e-15
absolute.  The inputs keep rel_l2_scaled and rmse_log10_scaled >= 1e-3 (checked on the restatement), so no figure is a cancelled remainder."""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import image_error_ref as ir
from conftest import GOLD, gold
from drmnet_amd import relight, samples

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(1, 1), (7, 5), (64, 64), (97, 131)]  # HW = 1, 35, 4096 (parts x threads exactly) and 12707 (every part loops; a multiple of nothing)
LAYOUTS = [("first_padded", "last"), ("last_padded", "first"), ("first", "first"), ("last", "last")]
PAIRS = list(itertools.product(range(3), repeat=3)) + [(2, 2, 2), (0, 0, 0), (1, 2, 0), (2, 1, 2), (0, 2, 2), (1, 1, 0)]  # every triple, and six again: P = 33
assert len(PAIRS) == 33


@functools.lru_cache(maxsize=None)
def reference(H, W):
    """three images a side and three masks (full, empty, scattered) on an H x W film, and for every pair of PAIRS the figures of the
    restatement and of the host path: computed once, shared by every layout"""
    holes = 0 if H * W == 1 else 3
    a, b, m = ir.images(11, 3, H, W, holes), ir.images(12, 3, H, W, holes), ir.masks(13 + H, H, W)
    want = [ir.errors(ir.error_sums(a[i], b[j], m[k])) for i, j, k in PAIRS]
    host = [relight.image_errors(a[i], b[j], m[k]) for i, j, k in PAIRS]
    for w, h in zip(want, host):
        ir.difference(w, h, keys=tuple(h))  # the yardstick agrees with the path it replaces
        assert w["n"] == 0 or (w["rel_l2_scaled"] >= 1e-3 and w["rmse_log10_scaled"] >= 1e-3 and w["n_log"] >= 3), w
    assert any(w["n"] == H * W for w in want) and any(w["n"] == 0 for w in want)
    assert H * W == 1 or any(0 < w["n"] < H * W and w["n_log"] < 3 * w["n"] for w in want)
    return a, b, m, want, host


def stack(x: np.ndarray, layout: str) -> torch.Tensor:
    """x [B, H, W, 3] on the device in ``layout``: channel-last as it is, channel-first [B, 3, H, W]; _padded: rows of a larger buffer
    (a batch stride larger than the image), the padding NaN so that a read outside the image shows"""
    t = torch.from_numpy(x).to(DEV)
    if layout.startswith("first"):
        t = t.permute(0, 3, 1, 2).contiguous()
    if layout.endswith("_padded"):
        buf = torch.full((t.shape[0], t[0].numel() + 5), float("nan"), device=DEV)
        view = buf[:, : t[0].numel()].unflatten(1, tuple(t.shape[1:]))
        view.copy_(t)
        assert view.stride(0) == t[0].numel() + 5 and view.data_ptr() == buf.data_ptr()
        return view
    return t


@pytest.mark.parametrize("layouts", LAYOUTS, ids=lambda l: "-".join(l))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_thirty_three_pairs_against_the_restatement_and_the_host_path(shape, layouts):
    a, b, m, want, host = reference(*shape)
    got = relight.image_errors_batch(stack(a, layouts[0]), stack(b, layouts[1]), torch.from_numpy(m).to(DEV), pairs=PAIRS)
    assert len(got) == 33 and all(list(g) == list(ir.FIGURES) for g in got)
    worst = max(ir.difference(g, w) for g, w in zip(got, want))
    worst_host = max(ir.difference(g, h, keys=tuple(h)) for g, h in zip(got, host))
    print(f"image_errors_batch {shape} {layouts}: largest difference {worst:.3e} (restatement), {worst_host:.3e} (host image_errors), relative")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_pair_single_images_and_shared_rows(shape):
    a, b, m, want, _ = reference(*shape)
    first = torch.from_numpy(a[1]).to(DEV).permute(2, 0, 1).contiguous()  # [3, H, W]
    last = torch.from_numpy(b[2]).to(DEV)  # [H, W, 3]
    sums = relight.image_error_sums(first, last, torch.from_numpy(m[2]).to(DEV))
    assert sums.shape == (1, 10) and sums.dtype == torch.float64 and sums.device == DEV
    ir.difference(relight.errors_from_image_sums(sums[0].cpu().numpy()), want[PAIRS.index((1, 2, 2))])
    # without pairs: row i against row i, a stack of one shared by all (three renders against one input on one mask)
    got = relight.image_errors_batch(stack(a, "first"), last, m[0])
    assert len(got) == 3
    for i in range(3):
        ir.difference(got[i], want[PAIRS.index((i, 2, 0))])


@pytest.mark.parametrize("shape", [(7, 5), (97, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_pair_gives_the_same_bits_alone_anywhere_and_twice(shape):
    a, b, m, _, _ = reference(*shape)
    A, B, M = stack(a, "first_padded"), stack(b, "last"), torch.from_numpy(m).to(DEV)
    pair = (1, 2, 2)
    alone = relight.image_error_sums(A, B, M, pairs=[pair])
    assert bool(torch.isfinite(alone).all()) and float(alone[0, 0]) > 0
    others = [p for p in PAIRS if p != pair]
    for at in (0, 17, 32):
        listed = others[:32]
        listed.insert(at, pair)
        many = relight.image_error_sums(A, B, M, pairs=listed)
        assert many.shape == (33, 10) and torch.equal(many[at], alone[0]), at
        assert torch.equal(many, relight.image_error_sums(A, B, M, pairs=listed))  # two calls
    # the same pair as single images in the other layouts: the order of a pair's pixels does not depend on how they lie in memory
    single = relight.image_error_sums(torch.from_numpy(a[1]).to(DEV), torch.from_numpy(b[2]).to(DEV).permute(2, 0, 1).contiguous(), M[2])
    assert torch.equal(single[0], alone[0])


def test_non_finite_values_propagate_as_in_numpy():
    H, W = 7, 5
    a, b, m, _, _ = (np.copy(x) if isinstance(x, np.ndarray) else x for x in reference(H, W))
    on = np.argwhere(m[2] != 0)
    off = np.argwhere(m[2] == 0)
    a[0][tuple(on[0])] = [np.nan, 1.0, 2.0]
    a[1][tuple(on[1])] = [np.inf, 1.0, 2.0]
    a[2][tuple(off[0])] = [np.nan, np.inf, -np.inf]  # not on the scattered mask: never read
    pairs = [(0, 0, 2), (1, 0, 2), (2, 0, 2), (0, 1, 1)]
    got = relight.image_error_sums(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), torch.from_numpy(m).to(DEV), pairs=pairs).cpu().numpy()
    with np.errstate(all="ignore"):
        want = np.stack([ir.error_sums(a[i], b[j], m[k]) for i, j, k in pairs])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    finite = np.isfinite(want)
    assert np.all(np.abs(got[finite] - want[finite]) <= ir.RTOL * np.abs(want[finite]) + ir.ATOL)
    assert np.isnan(want[0]).any() and np.isinf(want[1]).any() and np.isfinite(want[2]).all() and not want[3].any()


def test_pairwise_distances_of_five_maps():
    maps = ir.images(21, 5, 16, 16)
    maps[4] = 2.0 * maps[1]  # one draw is another at twice the scale (exact in fp32, and in every sum): their distance is exactly 0 both ways
    D = samples.pairwise_distances(torch.from_numpy(maps).to(DEV).permute(0, 3, 1, 2).contiguous())
    assert D.shape == (5, 5) and D.dtype == np.float64
    ones = np.ones((16, 16))
    worst = 0.0
    for i in range(5):
        for j in range(5):
            want = relight.image_errors(maps[i], maps[j], ones)["rel_l2_scaled"]
            worst = max(worst, ir.difference({"rel_l2_scaled": D[i, j]}, {"rel_l2_scaled": want}, keys=("rel_l2_scaled",)))
            assert want >= 1e-3 or i == j or {i, j} == {1, 4}
    assert np.array_equal(np.diag(D), np.zeros(5)) and D[1, 4] == 0.0 and D[4, 1] == 0.0
    assert samples.medoid(D) == int(np.argmin(D.sum(axis=1)))
    print(f"pairwise_distances 5 x 16 x 16: largest difference {worst:.3e} relative")


# ---------------------------------------------------------------------------------------------- N draws of one image on the tiny networks

N = 3


@pytest.fixture(scope="module")
def chain():
    from types import SimpleNamespace

    from drmnet_amd import file_io
    from drmnet_amd.estimate import estimate_samples
    from test_gpu_estimate import tiny_models

    g = gold("estimate_chain")
    drm, obs = tiny_models(g, DEV)
    drm.set_precision("fp32")
    obs.set_precision("fp32")
    d = os.path.join(GOLD, "sample")
    img = file_io.load_exr(os.path.join(d, "image.exr"), as_torch=True).to(DEV)
    nrm = torch.from_numpy(np.load(os.path.join(d, "normal.npy"))).to(DEV)
    mask = torch.logical_and(file_io.load_png(os.path.join(d, "mask.png"), as_torch=True).to(DEV) > 0, torch.linalg.norm(nrm, dim=-1) > 0.5)
    gen = torch.Generator().manual_seed(3)

    def rows(name, dim):
        """the recorded draw on row 0, and behind it along ``dim`` two unit-variance draws near it (0.995 x + 0.1 e: the tiny synthetic
        networks are not trained, and far from the recorded draw their BRDF head can leave the numbers)"""
        x = torch.from_numpy(g[name])
        near = [float(np.sqrt(1.0 - 0.01)) * x + 0.1 * torch.randn(x.shape, generator=gen) for _ in range(N - 1)]
        return torch.cat([x] + near, dim=dim).to(DEV)

    hooks = {"cond_noise": rows("cond", 0), "x_T": rows("x_T", 0), "noise": rows("noise", 1), "noise0": rows("noise0", 0), "step_noise": rows("step_noise", 1)}
    Lr0, zK, K = estimate_samples(drm, obs, img, nrm, mask, N, hooks=dict(hooks))
    argv = ["--input_img", os.path.join(d, "image.exr"), "--input_normal", os.path.join(d, "normal.npy"), "--input_mask", os.path.join(d, "mask.png")]
    return SimpleNamespace(g=g, drm=drm, obs=obs, img=img, nrm=nrm, mask=mask, hooks=hooks, Lr0=Lr0, zK=zK, K=K, argv=argv)


def same_bits(x, y) -> bool:
    """bit for bit, a NaN equal to the same NaN"""
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def differ_pairwise(x) -> bool:
    return all(not torch.equal(x[i], x[j]) for i in range(len(x)) for j in range(i))


def test_samples_are_the_batch_on_replicated_inputs_bit_for_bit(chain):
    from drmnet_amd.estimate import estimate_batch

    c = chain
    assert c.Lr0.shape == (N, 3, 16, 16) and c.zK.shape == (N, 6) and c.K.shape == (N,)
    Lr0, zK, K = estimate_batch(c.drm, c.obs, c.img[None].expand(N, -1, -1, -1), c.nrm[None].expand(N, -1, -1, -1), c.mask[None].expand(N, -1, -1),
                                hooks=dict(c.hooks))
    assert same_bits(Lr0, c.Lr0) and same_bits(zK, c.zK) and same_bits(K.to(torch.int32), c.K.to(torch.int32))
    assert bool(torch.isfinite(c.Lr0).all()) and differ_pairwise(c.Lr0)  # the rows differ through the noise alone


def test_a_seed_fixes_the_draws(chain):
    from drmnet_amd.estimate import estimate_samples

    c = chain
    one = estimate_samples(c.drm, c.obs, c.img, c.nrm, c.mask, N, seed=7)
    two = estimate_samples(c.drm, c.obs, c.img, c.nrm, c.mask, N, seed=7)
    other = estimate_samples(c.drm, c.obs, c.img, c.nrm, c.mask, N, seed=8)
    assert all(same_bits(x.to(torch.float32), y.to(torch.float32)) for x, y in zip(one, two))
    assert not same_bits(one[0], other[0])
    assert differ_pairwise(one[0]) and differ_pairwise(other[0])


def test_rerender_errors_are_the_errors_of_each_rerender_alone(chain):
    c = chain
    got = samples.rerender_errors(c.drm, c.Lr0, c.zK, c.img, c.nrm, c.mask)
    assert len(got) == N
    alone = []
    for i in range(N):
        image, _ = relight.rerender(c.drm, c.Lr0[i], c.zK[i], c.nrm, c.mask)
        alone.append(relight.image_errors(image[0].permute(1, 2, 0), c.img, c.mask))
        worst = ir.difference(got[i], alone[i], keys=tuple(alone[i]))
        print(f"draw {i}: rel_l2 {got[i]['rel_l2']:.6f}, rel_l2_scaled {got[i]['rel_l2_scaled']:.6f}, largest difference {worst:.3e} relative")
    assert got[0]["n"] == int(c.mask.sum()) > 0
    rel = np.array([e["rel_l2"] for e in alone])
    assert samples.select("rerender", errors=got) == int(np.argmin(np.where(np.isnan(rel), np.inf, rel))) and np.isfinite(rel).any()
    report = samples.rank(c.drm, c.Lr0, c.zK, c.K, c.img, c.nrm, c.mask, "medoid")
    assert report["finite"] == samples.finite_draws(c.Lr0, c.zK) == [bool(torch.isfinite(c.zK[i]).all() and torch.isfinite(c.Lr0[i]).all()) for i in range(N)]
    assert report["selected"] == report["medoid"] == samples.medoid(samples.pairwise_distances(c.Lr0), report["finite"])
    assert json.dumps(report["rerender_errors"]) == json.dumps(got)


def golden_hooks(g):
    return {k: torch.from_numpy(g[s]).to(DEV) for k, s in (("cond_noise", "cond"), ("x_T", "x_T"), ("noise", "noise"), ("noise0", "noise0"),
                                                          ("step_noise", "step_noise"))}


def test_num_samples_1_writes_the_files_of_a_run_without_the_flag(chain, tmp_path):
    from drmnet_amd import estimate

    c = chain
    for name, flags in (("plain", []), ("one", ["--num_samples", "1"])):
        estimate.main(c.argv + ["--rerender", "--output_dir", str(tmp_path / name)] + flags, models=(c.drm, c.obs), hooks=golden_hooks(c.g))
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "one")) and not any(f.startswith("samples") or f in ("sample_mean_env.png", "sample_std.exr") for f in files)
    assert {"sample_env.png", "sample_brdf.png", "sample_brdf.npy", "sample_rerender.exr", "sample_errors.json"} <= set(files)
    for f in files:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "one" / f).read_bytes(), f


def test_num_samples_3_keeps_the_best_draw_and_adds_its_files(chain, tmp_path):
    from drmnet_amd import estimate, file_io

    c = chain
    estimate.main(c.argv + ["--rerender", "--num_samples", "3", "--seed", "7", "--output_dir", str(tmp_path)], models=(c.drm, c.obs))
    report = json.loads((tmp_path / "samples.json").read_text())
    assert report["num_samples"] == 3 and report["seed"] == 7 and report["select"] == "rerender"
    assert len(report["zK"]) == len(report["K"]) == len(report["rerender_errors"]) == 3 and np.array(report["pairwise_rel_l2_scaled"]).shape == (3, 3)
    sel = report["selected"]
    draws = np.load(tmp_path / "samples_Lr0.npy")
    assert draws.shape == (3, 3, 16, 16) and draws.dtype == np.float32
    # which draws are estimates at all is listed, and is what the listed values say: the tiny synthetic networks are untrained, and a draw
    # can end with a BRDF of NaNs, which shades to a black image of rel_l2 exactly 1
    finite = np.array(report["finite"])
    assert finite.tolist() == [bool(np.isfinite(report["zK"][i]).all() and np.isfinite(draws[i]).all()) for i in range(3)] and finite.any()
    # selected is the argmin of the run's own listed errors, over the draws it lists as finite
    listed = np.array([e["rel_l2"] for e in report["rerender_errors"]])
    assert sel == int(np.flatnonzero(finite)[np.argmin(listed[finite])]) and finite[sel] and np.isfinite(listed[sel])
    assert report["medoid"] == samples.medoid(np.array(report["pairwise_rel_l2_scaled"]), report["finite"]) and finite[report["medoid"]]
    assert np.array_equal(np.load(tmp_path / "sample_brdf.npy"), np.array(report["zK"][sel], dtype=np.float32))
    std = file_io.load_exr(tmp_path / "sample_std.exr")
    assert std.shape == (16, 16, 3) and np.allclose(std, draws[finite].std(axis=0).transpose(1, 2, 0), rtol=1e-5, atol=1e-7)
    assert tuple(file_io.load_png(tmp_path / "sample_mean_env.png").shape[:2]) == (16, 32)
    # everything after the selection is written from the selected draw: the re-render's own error is the listed one
    rerender = json.loads((tmp_path / "sample_errors.json").read_text())["estimate"]
    ir.difference(report["rerender_errors"][sel], rerender, keys=tuple(rerender))
    # and the seed makes the run repeat
    estimate.main(c.argv + ["--num_samples", "3", "--seed", "7", "--output_dir", str(tmp_path / "again")], models=(c.drm, c.obs))
    assert (tmp_path / "again" / "samples.json").read_bytes() == (tmp_path / "samples.json").read_bytes()
    assert (tmp_path / "again" / "samples_Lr0.npy").read_bytes() == (tmp_path / "samples_Lr0.npy").read_bytes()

"""CPU-only checks of the batched image errors and of the sampling surface built on them: the float64 restatement
(tests/image_error_ref.py) against relight.image_errors on hand-made images, the declaration of drm_image_error_sums in the header, the
binding and the built library, every refusal of the entry (host buffers stand in for device memory: the checks dereference nothing), the
wrapper's checks, the argument rules of ``estimate``'s command line, and medoid / select on hand-made matrices.  Nothing here touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import image_error_ref as ir
from conftest import ROOT
from drmnet_amd import _lib, relight, samples

INVALID = 1


def hand_made():
    """(name, a, b, mask) on a 3 x 4 film"""
    rng = np.random.default_rng(5)
    a = (10.0 ** rng.uniform(-2, 1, size=(3, 4, 3))).astype(np.float32)
    b = (a * rng.uniform(0.5, 2.0, size=a.shape)).astype(np.float32)
    full, part, empty = np.ones((3, 4), dtype=np.uint8), (np.arange(12).reshape(3, 4) % 3 != 1).astype(np.uint8) * 200, np.zeros((3, 4), dtype=np.uint8)
    holed_a, holed_b = a.copy(), b.copy()
    holed_a[0, 0, 0], holed_a[1, 2, 1], holed_b[2, 3, 2], holed_b[0, 0, 0] = 0.0, -0.5, -2.0, 0.0
    return [("full", a, b, full), ("partial", a, b, part), ("empty", a, b, empty), ("zero_a", np.zeros_like(a), b, full),
            ("zero_b", a, np.zeros_like(b), full), ("both_zero", np.zeros_like(a), np.zeros_like(b), part), ("not_positive", holed_a, holed_b, part),
            ("twice", a, 2.0 * a, full)]


@pytest.mark.parametrize("case", hand_made(), ids=lambda c: c[0])
def test_the_restatement_equals_image_errors(case):
    name, a, b, mask = case
    s = ir.error_sums(a, b, mask)
    want = relight.image_errors(torch.from_numpy(a), torch.from_numpy(b), mask)
    got = ir.errors(s)
    assert set(got) == set(want) | {"rmse_log10_scaled"}
    ir.difference(got, want, keys=tuple(want))
    assert got == relight.errors_from_image_sums(s)  # the product's figures from the same sums
    assert s[0] == (mask != 0).sum() and s[5] == ((a > 0) & (b > 0))[mask != 0].sum()
    if name == "empty" or name == "both_zero":
        assert all(got[k] == 0 for k in ir.FIGURES if k != "n") and got["n"] == (0 if name == "empty" else 8)
    if name == "zero_a":
        assert got["scale"] == 0.0 and got["rel_l2"] == 1.0 and got["rel_l2_scaled"] == 1.0 and got["n_log"] == 0 and got["rmse_log10"] == 0.0
    if name == "zero_b":
        assert got["rel_l2"] == float("inf") and got["rel_l2_scaled"] == 0.0 and got["scale"] == 0.0  # (scale 0 brings a onto the zero image)
    if name == "not_positive":
        assert got["n_log"] == 3 * got["n"] - 3  # four values <= 0 in three entries (a and b share one), all on the mask
    if name == "twice":
        assert abs(got["scale"] - 2.0) <= 1e-12 and got["rel_l2_scaled"] <= 1e-12 and abs(got["rmse_log10"] - np.log10(2.0)) <= 1e-12
        assert got["rmse_log10_scaled"] <= 1e-12 and abs(got["rel_l2"] - 0.5) <= 1e-12


def test_two_passes_where_one_pass_cancels():
    """the reason for the second pass: two draws 1e-7 apart on 97 x 131 pixels.  rel_l2_scaled^2 is about 5e-15 of BB, and the one-pass
    identity BB - AB^2 / AA forms it as the difference of two numbers each rounded to 1e-16 of BB: percents are lost where two passes lose
    nothing"""
    a = ir.images(3, 1, 97, 131, holes=0)[0].astype(np.float64)
    b = a * (1.0 + 1e-7 * np.sin(np.arange(a.size).reshape(a.shape)))
    s = ir.error_sums(a, b, np.ones(a.shape[:2]))
    two_pass = np.sqrt(s[8] / s[2])
    one_pass = np.sqrt(max(s[2] - s[3] * s[3] / s[1], 0.0) / s[2])
    la, lb = a.astype(np.longdouble), b.astype(np.longdouble)
    exact = float(np.sqrt(np.sum((np.sum(la * lb) / np.sum(la * la) * la - lb) ** 2) / np.sum(lb * lb)))
    print(f"rel_l2_scaled: extended precision {exact:.6e}, two passes {two_pass:.6e}, one pass {one_pass:.6e}")
    assert 1e-8 < exact < 1e-7 and abs(two_pass - exact) <= 1e-8 * exact
    assert abs(one_pass - exact) > 1e-4 * exact


def test_the_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "drmnet_hip.h")).read()
    assert "int drm_image_error_sums(const drm_image_error* args, void* stream);" in header
    assert "} drm_image_error;" in header and "#define DRM_IMAGE_ERROR_WORKSPACE_BYTES(P)" in header
    assert "drm_image_error_sums" in _lib.SYMBOLS and hasattr(_lib.lib(), "drm_image_error_sums")
    assert int(re.search(r"#define DRM_IMAGE_ERROR_SUMS (\d+)", header).group(1)) == _lib.IMAGE_ERROR_SUMS == len(ir.SUMS) == len(relight.IMAGE_SUM_NAMES) == 10
    assert int(re.search(r"#define DRM_IMAGE_ERROR_PARTS (\d+)", header).group(1)) == _lib.IMAGE_ERROR_PARTS
    assert _lib.image_error_workspace_bytes(33) == 33 * _lib.IMAGE_ERROR_PARTS * 10 * 8
    assert relight.IMAGE_SUM_NAMES == ir.SUMS
    for i, name in enumerate(("N", "AA", "BB", "AB", "L2", "N_LOG", "D", "DD", "L2_SCALED", "DD_CENTRED")):
        assert f"#define DRM_IMAGE_ERROR_{name} {i}\n" in header
    # the members of the struct, in order, as the binding mirrors them
    body = re.search(r"typedef struct drm_image_error \{(.*?)\} drm_image_error;", header, flags=re.S).group(1)
    members = [m for decl in body.split(";") for m in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert members == [f for f, _ in _lib.ImageError._fields_]
    assert _lib.lib().drm_abi_version() == 4


class Args:
    """valid arguments of drm_image_error_sums on host memory: 2 channel-first images against 1 channel-last on 2 masks of 5 x 7, 3 pairs"""

    def __init__(self):
        self.a, self.b = np.ones((2, 3, 5, 7), dtype=np.float32), np.ones((1, 5, 7, 3), dtype=np.float32)
        self.mask, self.pairs = np.ones((2, 35), dtype=np.uint8), np.array([[0, 0, 0], [1, 0, 1], [0, 0, 1]], dtype=np.int32)
        self.need = _lib.image_error_workspace_bytes(3)
        self.ws, self.sums = np.zeros(self.need // 8 + 1, dtype=np.float64), np.full((3, 10), -7.0)

    def struct(self, **over):
        a = dict(a=self.a.ctypes.data, a_count=2, a_batch_stride=105, a_pixel_stride=1, a_channel_stride=35, b=self.b.ctypes.data, b_count=1,
                 b_batch_stride=105, b_pixel_stride=3, b_channel_stride=1, mask=self.mask.ctypes.data, mask_count=2, HW=35, pairs=self.pairs.ctypes.data,
                 P=3, workspace=self.ws.ctypes.data, workspace_bytes=self.need, sums=self.sums.ctypes.data)
        a.update(over)
        return _lib.sized(_lib.ImageError, **a)


def test_every_refusal_names_what_is_wrong_before_any_launch():
    lib, g = _lib.lib(), Args()

    def refused(s, word):
        status = lib.drm_image_error_sums(C.byref(s), None)
        message = (lib.drm_last_error() or b"").decode()
        assert status == INVALID and "image_error" in message and word in message, (word, status, message)
        assert np.all(g.sums == -7.0) and not g.ws.any()

    for name in ("a", "b", "mask", "pairs", "workspace", "sums"):
        refused(g.struct(**{name: None}), "null pointer")
    for P in (0, -1, 4097):
        refused(g.struct(P=P, workspace_bytes=_lib.image_error_workspace_bytes(4097)), "P in [1, 4096]")
    for HW in (0, -35):
        refused(g.struct(HW=HW), "HW >= 1")
    for name in ("a_count", "b_count", "mask_count"):
        for n in (0, -2):
            refused(g.struct(**{name: n}), "must be >= 1")
    refused(g.struct(workspace_bytes=g.need - 1), "DRM_IMAGE_ERROR_WORKSPACE_BYTES")
    refused(g.struct(workspace_bytes=0), "DRM_IMAGE_ERROR_WORKSPACE_BYTES")
    refused(g.struct(workspace=g.ws.ctypes.data + 4), "8-byte aligned")
    refused(g.struct(sums=g.sums.ctypes.data + 4), "8-byte aligned")
    wrong = g.struct()
    wrong.struct_bytes += 8
    refused(wrong, "struct_bytes")
    assert lib.drm_image_error_sums(None, None) == INVALID and b"args is null" in lib.drm_last_error()


def test_the_wrapper_checks_shapes_and_pairs_on_the_host():
    a, b, mask = torch.ones(2, 3, 5, 7), torch.ones(1, 5, 7, 3), torch.ones(2, 5, 7, dtype=torch.uint8)
    for pairs, word in (([[2, 0, 0]], "ia"), ([[0, 1, 0]], "ib"), ([[0, 0, 2]], "im"), ([[0, 0, 0], [-1, 0, 0]], "ia"), ([[0, 0]], "[P, 3]"),
                        ([[0.0, 0.0, 0.0]], "integers"), (np.zeros((0, 3), dtype=np.int64), "P = 0"), (np.zeros((4097, 3), dtype=np.int64), "P = 4097")):
        with pytest.raises(ValueError, match=re.escape(word)):
            relight.image_error_sums(a, b, mask, pairs=pairs)
    with pytest.raises(ValueError, match="1 or P"):
        relight.image_error_sums(torch.ones(3, 3, 5, 7), b, mask)  # 3 rows against 2 masks, no pairs
    for bad_a in (torch.ones(2, 3, 5, 6), torch.ones(2, 4, 5, 7), torch.ones(5, 7), np.ones((2, 3, 5, 7), dtype=np.float32)):
        with pytest.raises(ValueError, match="a must be"):
            relight.image_error_sums(bad_a, b, mask)
    with pytest.raises(ValueError, match="mask must be"):
        relight.image_error_sums(a, b, torch.ones(35))
    # good arguments on the CPU are refused like every GPU-only entry of relight: a RuntimeError, after the argument checks
    with pytest.raises(RuntimeError, match="GPU only"):
        relight.image_error_sums(a, b, mask, pairs=[[1, 0, 1]])
    with pytest.raises(RuntimeError, match="GPU only"):
        relight.image_errors_batch(a[:1], b, mask[0])
    with pytest.raises(RuntimeError, match="GPU only"):
        samples.pairwise_distances(torch.ones(2, 3, 4, 4))
    with pytest.raises(ValueError, match="in \\[1, 64\\]"):
        samples.pairwise_distances(torch.ones(65, 3, 2, 2))
    # the layouts and strides the entry is given
    t, count, strides = relight._image_stack("t", "a", torch.ones(4, 3, 5, 7)[::2], 5, 7)
    assert count == 2 and strides == (210, 1, 35) and t.data_ptr() == t.untyped_storage().data_ptr()  # a strided batch, not copied
    assert relight._image_stack("t", "a", torch.ones(5, 7, 3), 5, 7)[1:] == (1, (105, 3, 1))
    assert relight._image_stack("t", "a", torch.ones(2, 3, 5, 14)[..., ::2], 5, 7)[2] == (210, 2, 70)  # every other column: still one pixel stride
    assert relight._image_stack("t", "a", torch.ones(2, 3, 10, 7)[:, :, ::2], 5, 7)[2] == (105, 1, 35)  # every other row: copied


def test_argument_rules_of_the_command_line(capsys):
    from drmnet_amd import estimate

    base = ["--input_img", "i.exr", "--input_normal", "n.npy"]
    for argv, word in ((["--num_samples", "0"], "--num_samples in [1, 64]"), (["--num_samples", "65"], "--num_samples in [1, 64]"),
                       (["--seed", "7"], "need --num_samples > 1"), (["--select", "medoid"], "need --num_samples > 1"),
                       (["--num_samples", "1", "--seed", "7"], "need --num_samples > 1"), (["--num_samples", "1", "--select", "first"], "need --num_samples > 1"),
                       (["--num_samples", "3", "--select", "best"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            estimate.parse_args(base + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    a = estimate.parse_args(base)
    assert a.num_samples == 1 and a.select is None and a.seed is None
    a = estimate.parse_args(base + ["--num_samples", "64"])
    assert a.num_samples == 64 and a.select == "rerender" and a.seed is None
    a = estimate.parse_args(base + ["--num_samples", "3", "--select", "medoid", "--seed", "7"])
    assert (a.num_samples, a.select, a.seed) == (3, "medoid", 7)
    with pytest.raises(ValueError, match="num_samples in"):
        estimate.estimate_samples(None, None, None, None, None, 65)
    with pytest.raises(ValueError, match="num_samples in"):
        estimate.estimate_samples(None, None, None, None, None, 0)


def test_medoid_and_select_on_hand_made_matrices():
    D = np.array([[0.0, 1.0, 4.0], [1.0, 0.0, 2.0], [4.0, 2.0, 0.0]])
    assert samples.medoid(D) == 1 and samples.medoid([[0.0]]) == 0
    assert samples.medoid(np.array([[0.0, 3.0, 3.0], [1.0, 0.0, 5.0], [2.0, 4.0, 0.0]])) == 0  # row sums 6, 6, 6: the lowest index
    assert samples.medoid(np.array([[0.0, 2.0, 2.0], [3.0, 0.0, 0.5], [0.5, 3.0, 0.0]])) == 1  # 4, 3.5, 3.5
    assert samples.medoid(np.array([[0.0, np.nan], [5.0, 0.0]])) == 1  # a NaN row is infinitely far
    assert samples.medoid(np.array([[0.0, 1.0, 1.0], [0.2, 0.0, 0.1], [9.0, 9.0, 0.0]])) == 1  # not symmetric: the rows count
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((0, 0))):
        with pytest.raises(ValueError):
            samples.medoid(bad)
    errors = [{"rel_l2": 0.5, "rel_l2_scaled": 0.01}, {"rel_l2": 0.25, "rel_l2_scaled": 0.2}, {"rel_l2": 0.25, "rel_l2_scaled": 0.1}, {"rel_l2": float("nan")}]
    assert samples.select("rerender", errors=errors) == 1  # rel_l2, not the scaled figure; the tie goes to the lowest index; NaN never wins
    assert samples.select("rerender", errors=[{"rel_l2": float("nan")}, {"rel_l2": float("inf")}]) == 0
    assert samples.select("medoid", distances=D) == 1 and samples.select("first") == 0 and samples.select("first", errors=errors, distances=D) == 0
    for kind, kw in (("rerender", {}), ("medoid", {}), ("best", {"errors": errors}), ("rerender", {"errors": []})):
        with pytest.raises(ValueError):
            samples.select(kind, **kw)
    # a draw that is not finite (a BRDF of NaNs shades to a black image of rel_l2 exactly 1) is never chosen while another is
    black = [{"rel_l2": 3.0}, {"rel_l2": 1.0}, {"rel_l2": 2.0}]
    assert samples.select("rerender", errors=black) == 1 and samples.select("rerender", errors=black, finite=[True, False, True]) == 2
    assert samples.select("rerender", errors=black, finite=[False, False, False]) == 1  # none is: all stand
    assert samples.select("first", finite=[False, True, True]) == 1 and samples.select("first", finite=[False, False]) == 0
    assert samples.select("rerender", errors=[{"rel_l2": float("inf")}] * 3, finite=[False, True, True]) == 1
    assert samples.medoid(D, [True, False, True]) == 0 and samples.select("medoid", distances=D, finite=[False, True, True]) == 1
    assert samples.medoid(D, [False, False, True]) == 2 and samples.medoid(D, [False, False, False]) == 1
    with pytest.raises(ValueError):
        samples.medoid(D, [True, False])
    assert samples.finite_draws(torch.tensor([1.0, float("nan"), 1.0, 1.0]).reshape(4, 1, 1, 1).expand(4, 3, 2, 2),
                                torch.tensor([[0.0], [0.0], [float("inf")], [1.0]])) == [True, False, False, True]
    stats = samples.sample_statistics(torch.tensor([1.0, 3.0]).reshape(2, 1, 1, 1).expand(2, 3, 2, 2), torch.tensor([[0.0, 1.0], [1.0, 1.0]]))
    assert torch.equal(stats["Lr0_mean"], torch.full((3, 2, 2), 2.0)) and torch.equal(stats["Lr0_std"], torch.ones(3, 2, 2))
    assert stats["zK_mean"].tolist() == [0.5, 1.0] and stats["zK_std"].tolist() == [0.5, 0.0]

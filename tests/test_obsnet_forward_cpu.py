"""CPU checks of ObsNet's validation pass: the float64 restatement of the forward process and the losses (tests/obsnet_forward_ref.py) against
the reference's recorded scalars (tests/golden/obsnet_forward.npz, tools/make_golden_obsnet_forward.py), the lvlb_weights / logvar tables, the
sparse-mask dataset, and the host surface around them."""
import inspect
import os

import numpy as np
import pytest
import torch

import obsnet_forward_ref as ofr
from conftest import ROOT, gold
from test_forward_cpu import NAMES6, UNET_T, tiny_drmnet, write_datalist

TRANSFORM = "0p1tom1p1_normalizedLogarithmic_lowerbound1e-6"
RENDERER_T = {"target": "utils.mitsuba3_utils.MitsubaRefMapRenderer", "params": {"refmap_res": 16, "spp": 256, "denoise": "simple", "brdf_param_names": NAMES6}}


def tiny_obsnet(g=None, **kw):
    """the tiny ObsNet of the fixture's reference run (constants from the fixture when it is given)"""
    from drmnet_amd.obsnet import ObsNetDiffusion

    f = lambda key, default: float(g[key]) if g is not None else default
    base = dict(unet_config=UNET_T, linear_start=f("linear_start", 1e-4), linear_end=f("linear_end", 0.09), timesteps=1000, first_stage_key="LrK",
                cond_stage_key="masked_LrK", padding_mode="noise", noisy_observe=f("noisy_observe", 0.04), l_simple_weight=f("l_simple_weight", 2.0),
                original_elbo_weight=f("original_elbo_weight", 0.5), logvar_init=f("logvar_init", 0.3), image_size=16, channels=3, concat_mode=True,
                clip_denoised=False, loss_type="l2", masked_loss=False, use_ema=False, renderer_config=RENDERER_T)
    return ObsNetDiffusion(**dict(base, **kw))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_restatement_reproduces_the_reference_losses(loss_type, masked):
    g = gold("obsnet_forward")
    assert ((g["mask"] == 0) | (g["mask"] == 1)).all() and all(0 < m.sum() < m.size for m in g["mask"])
    got = ofr.diffusion_losses(g["model_out"], g["e_q"], g["t"], g["logvar"], g["lvlb_weights"], loss_type, float(g["l_simple_weight"]),
                               float(g["original_elbo_weight"]), invmask=1 - g["out_mask"] if masked else None)
    want = g[f"loss_{loss_type}_{'masked' if masked else 'plain'}"]
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-5)  # (the reference summed in fp32)
    assert not np.allclose(got, g[f"loss_{loss_type}_{'plain' if masked else 'masked'}"], rtol=1e-3)


def test_restatement_reproduces_the_reference_forward_process_and_figures():
    g = gold("obsnet_forward")
    cond, x_noisy, noise, _, _ = ofr.forward_process(g["out_LrK_z"], g["out_mask"], g["t"], g["sqrt_alphas_cumprod"], g["sqrt_one_minus_alphas_cumprod"],
                                                     float(g["noisy_observe"]), "noise", g["e_observe"], g["e_padding"], g["e_q"])
    np.testing.assert_allclose(cond, g["out_c"], rtol=1e-6, atol=1e-6)  # (a handful of fp32 operations there)
    np.testing.assert_allclose(x_noisy, g["x_noisy"], rtol=1e-6, atol=1e-6)
    assert np.array_equal(noise, g["e_q"].astype(np.float64))
    assert sorted(g["t"].tolist())[0] == 0 and sorted(g["t"].tolist())[-1] == 999
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))
    inv = 1 - g["out_mask"]
    assert rms(g["model_out"]) == pytest.approx(float(g["rms_model_out"]), rel=1e-12)
    assert rms(g["model_out"] - g["e_q"]) == pytest.approx(float(g["rms_residual"]), rel=1e-6)
    assert ofr.masked_rms(g["model_out"], inv) == pytest.approx(float(g["rms_model_out_masked"]), rel=1e-12)
    assert ofr.masked_rms(g["model_out"] - g["e_q"], inv) == pytest.approx(float(g["rms_residual_masked"]), rel=1e-6)
    assert float(g["max_lvlb_t"]) == float(g["lvlb_weights"][g["t"]].max()) and float(g["exp_neg_logvar_init"]) == pytest.approx(np.exp(-0.3), rel=1e-7)


def test_restatement_edges():
    r = np.random.default_rng(0)
    B = 4
    out, tgt = (r.normal(size=(B, 3, 4, 4)).astype(np.float32) for _ in range(2))
    t = np.array([0, 3, 5, 9])
    logvar, lvlb = np.full(10, 0.3, dtype=np.float32), r.uniform(0.1, 2.0, size=10).astype(np.float32)
    mask = (r.uniform(size=(B, 1, 4, 4)) > 0.5).astype(np.float32)
    mask[2] = 1.0  # nothing unobserved in row 2
    masked = ofr.diffusion_losses(out, tgt, t, logvar, lvlb, "l2", 2.0, 0.5, invmask=1 - mask)
    assert np.isnan(masked).all() and np.isnan(ofr.per_row_loss(out, tgt, "l2", 1 - mask)).tolist() == [False, False, True, False]
    assert np.isfinite(ofr.diffusion_losses(out, tgt, t, logvar, lvlb, "l2", 2.0, 0.5)).all()
    with pytest.raises(NotImplementedError):
        ofr.diffusion_losses(out, tgt, t, logvar, lvlb, "huber", 1.0, 0.0)
    # by hand on one row: mean |d|, lvlb[t] L, w (L / e^lv + lv) + w' vlb
    one = ofr.diffusion_losses(out[:1], tgt[:1], t[1:2], logvar, lvlb, "l1", 2.0, 0.5)
    L = np.abs(out[:1].astype(np.float64) - tgt[:1]).mean()
    np.testing.assert_allclose(one, [L, lvlb[3] * L, 2.0 * (L / np.exp(np.float64(logvar[3])) + logvar[3]) + 0.5 * lvlb[3] * L], rtol=1e-14)
    # dropped terms of the forward process drop exactly
    x, e = r.normal(size=(B, 3, 4, 4)), [r.normal(size=(B, 3, 4, 4)) for _ in range(3)]
    sa, s1 = np.linspace(1, 0.1, 10), np.linspace(0.1, 1, 10)
    assert np.array_equal(ofr.forward_process(x, mask, t, sa, s1, 0.0, "zeros", *e)[0], mask * x)
    with pytest.raises(ValueError):
        ofr.forward_process(x, mask[..., :2], t, sa, s1, 0.0, "zeros", *e)


# ------------------------------------------------------------------------------------------------ tables
def test_lvlb_weights_and_logvar_equal_the_reference_tables():
    g = gold("obsnet_forward")
    m = tiny_obsnet(g)
    assert m.lvlb_weights.dtype == torch.float32 and np.array_equal(m.lvlb_weights.numpy(), g["lvlb_weights"])
    assert m.logvar.dtype == torch.float32 and np.array_equal(m.logvar.numpy(), g["logvar"]) and (g["logvar"] == np.float32(0.3)).all()
    assert m.lvlb_weights[0] == m.lvlb_weights[1] and torch.isfinite(m.lvlb_weights).all()
    assert np.array_equal(m.sqrt_alphas_cumprod.numpy(), g["sqrt_alphas_cumprod"])
    assert "lvlb_weights" not in m.state_dict() and "logvar" not in m.state_dict()


# ------------------------------------------------------------------------------------------------ the sparse masks
def write_masks(root, arrays, split_dir="train", mode="L"):
    from PIL import Image

    (root / split_dir).mkdir(parents=True, exist_ok=True)
    names = []
    for i, a in enumerate(arrays):
        names.append(f"m{i:02d}.png")
        Image.fromarray(np.asarray(a, dtype=np.uint8), mode=mode).save(root / split_dir / names[-1])
    (root / "list.txt").write_text("\n".join(names) + "\n")
    return str(root / "list.txt")


def blob(h, w, k, value=255):
    """mask k of a family that one pixel tells apart: a filled rectangle plus a marker at (0, k)"""
    a = np.zeros((h, w), dtype=np.uint8)
    a[h // 4: h // 2 + 2, 1: w - 2] = value
    a[0, k] = value
    return a


def test_masked_dataset_follows_the_parents_mask_draw(tmp_path):
    from drmnet_amd.dataset import MaskedRefmapDataset, ParametricRefmapDataset

    g = gold("forward_dataset")
    n_masks = 7
    mask_list = write_masks(tmp_path / "masks", [blob(16, 16, k) for k in range(n_masks)])
    datalist = write_datalist(tmp_path / "envs.txt", 32)
    ds = MaskedRefmapDataset(16, "val", str(tmp_path / "maps"), 6, mask_root=str(tmp_path / "masks"), mask_list=mask_list, datalist=datalist)
    parent = ParametricRefmapDataset(16, "val", str(tmp_path / "maps"), 6, datalist=datalist)
    assert isinstance(ds, ParametricRefmapDataset) and ds.with_mask and ds.mask_len == n_masks and ds.t == "train"
    ds.model = parent.model = tiny_drmnet(gamma=float(g["gamma"]), epsilon=float(g["epsilon"]), z0=g["z0"].tolist())
    picked = set()
    for i in range(32):
        item, base = ds[i], parent[i]
        assert sorted(set(item) - set(base)) == ["mask"]
        for key in ("zK", "normalized_k", "view_from", "K", "k", "zk"):  # the subclass changes nothing else, draw for draw
            assert torch.equal(torch.as_tensor(item[key]), torch.as_tensor(base[key])), key
        assert np.array_equal(item["zK"].numpy(), g["val_zK"][i])
        # the fifth draw of the item's generator: after zK, normalized_k, the azimuth and the unused theta
        ds.set_generator(i)
        torch.rand((6,), generator=ds.generator)
        for _ in range(3):
            torch.rand((), generator=ds.generator)
        u = torch.rand((), generator=ds.generator).item()
        want = int(u * n_masks)
        picked.add(want)
        mask = item["mask"]
        assert mask.shape == (16, 16) and mask.dtype == np.float64 and set(np.unique(mask)) == {0.0, 1.0}
        assert np.array_equal(mask, blob(16, 16, want) / 255)
    assert len(picked) > 3
    test_ds = MaskedRefmapDataset(16, "test", str(tmp_path / "maps"), 6, mask_root=str(tmp_path / "masks"),
                                  mask_list=write_masks(tmp_path / "masks", [blob(16, 16, 0)], split_dir="test"), datalist=datalist)
    assert test_ds.t == "test" and np.array_equal(test_ds[0]["mask"], blob(16, 16, 0) / 255)


def test_masked_dataset_skips_small_masks_and_wraps(tmp_path):
    from drmnet_amd.dataset import MaskedRefmapDataset

    small = np.zeros((16, 16), dtype=np.uint8)
    small[3, 3] = 255  # 1 pixel of 256: below a rate of 0.01 (2.56 pixels)
    datalist = write_datalist(tmp_path / "envs.txt", 16)
    kw = dict(mask_root=str(tmp_path / "masks"), mask_area_min_rate=0.01, datalist=datalist)
    # [big, small, small]: a draw of index 1 steps to 2, then wraps to 0
    mask_list = write_masks(tmp_path / "masks", [blob(16, 16, 5), small, small])
    ds = MaskedRefmapDataset(16, "val", str(tmp_path / "maps"), 6, mask_list=mask_list, **kw)
    seen = set()
    for i in range(16):
        ds.set_generator(i)
        torch.rand((6,), generator=ds.generator)
        for _ in range(3):
            torch.rand((), generator=ds.generator)
        seen.add(int(torch.rand((), generator=ds.generator).item() * 3))
        assert np.array_equal(ds[i]["mask"], blob(16, 16, 5) / 255), i
    assert seen == {0, 1, 2}
    # with the rate of the small mask's own area it is taken
    ds = MaskedRefmapDataset(16, "val", str(tmp_path / "maps"), 6, mask_list=write_masks(tmp_path / "masks", [small]), **dict(kw, mask_area_min_rate=1 / 256))
    assert ds[0]["mask"].sum() == 1.0
    with pytest.raises(ValueError):  # no mask is large enough: an error, not the reference's endless loop
        MaskedRefmapDataset(16, "val", str(tmp_path / "maps"), 6, mask_list=write_masks(tmp_path / "masks", [small, small]), **kw)[0]


def test_masked_dataset_resizes_by_the_nearest_rule_and_rejects_other_images(tmp_path):
    from drmnet_amd.dataset import MaskedRefmapDataset, ParametricRefmapDataset

    datalist = write_datalist(tmp_path / "envs.txt", 2)
    kw = dict(mask_root=str(tmp_path / "masks"), mask_area_min_rate=0.0, datalist=datalist)
    r = np.random.default_rng(3)
    a = (r.uniform(size=(7, 5)) > 0.5).astype(np.uint8) * 255  # 7 rows x 5 columns -> 4 x 4: rows floor(i 7/4) = 0 1 3 5, columns floor(j 5/4) = 0 1 2 3
    ds = MaskedRefmapDataset(4, "val", str(tmp_path / "maps"), 6, mask_list=write_masks(tmp_path / "masks", [a]), **kw)
    hand = np.array([[a[i, j] for j in (0, 1, 2, 3)] for i in (0, 1, 3, 5)]) / 255
    assert np.array_equal(ds[0]["mask"], hand) and set(np.unique(ds[0]["mask"])) <= {0.0, 1.0}
    b = (r.uniform(size=(3, 3)) > 0.5).astype(np.uint8) * 255  # 3 -> 8: floor(i 3/8) = 0 0 0 1 1 1 2 2
    ds = MaskedRefmapDataset(8, "val", str(tmp_path / "maps"), 6, mask_list=write_masks(tmp_path / "masks", [b]), **kw)
    idx = (0, 0, 0, 1, 1, 1, 2, 2)
    assert np.array_equal(ds[1]["mask"], np.array([[b[i, j] for j in idx] for i in idx]) / 255)
    assert ofr.nearest_indices(7, 4).tolist() == [0, 1, 3, 5] and ofr.nearest_indices(3, 8).tolist() == list(idx)
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)
    ds = MaskedRefmapDataset(4, "val", str(tmp_path / "maps"), 6, mask_list=write_masks(tmp_path / "masks", [rgb], mode="RGB"), **kw)
    with pytest.raises(ValueError, match="single-channel"):
        ds[0]
    with pytest.raises(NotImplementedError, match="OpenCV"):  # the parent keeps refusing
        ParametricRefmapDataset(16, "val", str(tmp_path), 6, mask_root=str(tmp_path / "masks"), datalist=datalist)


# ------------------------------------------------------------------------------------------------ host surface
def test_constructor_keeps_the_validation_parameters():
    from drmnet_amd.obsnet import DDPM, LatentDiffusion, ObsNetDiffusion

    m = tiny_obsnet(loss_type="l1", masked_loss=True, envmap_dir="data/maps", cache_data=True, refmap_cache_root="data/cache")
    assert m.validation_params == {"loss_type": "l1", "l_simple_weight": 2.0, "original_elbo_weight": 0.5, "logvar_init": 0.3, "masked_loss": True,
                                   "first_stage_key": "LrK", "envmap_dir": "data/maps"}
    bare = ObsNetDiffusion(unet_config=UNET_T, use_ema=False, image_size=16)
    assert bare.validation_params == {"loss_type": "l2", "l_simple_weight": 1.0, "original_elbo_weight": 0.0, "logvar_init": 0.0, "masked_loss": True,
                                      "first_stage_key": "image", "envmap_dir": None}
    for key in m.validation_params:
        assert not hasattr(m, key), key
    assert not torch.cuda.is_initialized()
    want = {"get_input": ["self", "batch", "k", "return_first_stage_outputs", "force_c_encode", "cond_key", "return_original_cond", "bs"],
            "forward": ["self", "x", "c", "mask"], "p_losses": ["self", "x_start", "cond", "mask", "t", "noise"], "shared_step": ["self", "batch"],
            "validation_step": ["self", "batch", "batch_idx"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(ObsNetDiffusion, name))
        positional = [p.name for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert positional == params, (name, positional)
    assert inspect.signature(ObsNetDiffusion.p_losses).parameters["seed"].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(DDPM.get_loss).parameters) == ["self", "pred", "target", "mean"] and issubclass(LatentDiffusion, DDPM)
    a, b = torch.tensor([1.0, 2.0, 4.0]), torch.tensor([0.0, 4.0, 4.0])
    assert float(m.get_loss(a, b)) == pytest.approx(1.0) and float(bare.get_loss(a, b)) == pytest.approx(5.0 / 3)
    assert bare.get_loss(a, b, mean=False).tolist() == [1.0, 4.0, 0.0]
    with pytest.raises(NotImplementedError):
        tiny_obsnet(loss_type="huber").get_loss(a, b)
    with pytest.raises(NotImplementedError):
        tiny_obsnet(learn_logvar=True)
    with pytest.raises(NotImplementedError):
        tiny_obsnet(parameterization="x0")


def test_p_losses_and_get_input_raise_where_there_is_no_path():
    m = tiny_obsnet()
    x, mask, t = torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16), torch.zeros(2, dtype=torch.long)
    m.train()
    with pytest.raises(NotImplementedError):
        m.p_losses(x, x, mask, t)
    m.eval()
    with pytest.raises(RuntimeError):  # eval mode: the tensors must live on the GPU (no CPU path)
        m.p_losses(x, x, mask, t)
    batch = {"zK": torch.zeros(2, 6), "envmap_name": ["a", "b"], "view_from": torch.tensor([[0.0, 0.0, 1.0]] * 2), "LrK": torch.ones(2, 3, 16, 16),
             "mask": torch.ones(2, 16, 16)}
    with pytest.raises(NotImplementedError, match="373"):
        m.get_input(batch, "LrK", cond_key="raw_refmap")
    with pytest.raises(NotImplementedError):
        tiny_obsnet(cond_stage_key="raw_refmap").get_input(batch, "LrK")
    with pytest.raises(RuntimeError):  # the model is on the CPU
        m.get_input(batch, "LrK")


def test_validate_parser_and_masked_validation_node(tmp_path):
    import yaml

    from drmnet_amd import validate as V
    from drmnet_amd.config import load_config
    from drmnet_amd.dataset import MaskedRefmapDataset, ParametricRefmapDataset

    mask_list = write_masks(tmp_path / "masks", [blob(16, 16, k) for k in range(3)])
    datalist = write_datalist(tmp_path / "envs.txt", 3)
    a = V.make_parser().parse_args(["--base", "x.yaml"])
    assert a.mask_root is None and a.mask_list is None
    model = {"target": "models.obsnet.ObsNetDiffusion", "params": {"unet_config": UNET_T, "image_size": 16, "renderer_config": RENDERER_T}}
    node = {"target": "dataset.parametricrefmap.ParametricRefmapDataset",
            "params": {"size": 16, "split": "val", "return_envmap": True, "data_root": str(tmp_path / "maps"), "mask_root": str(tmp_path / "masks"),
                       "transform_func": TRANSFORM, "zdim": 6, "epoch_cycle": 1000, "refmap_cache_root": "./data/cache/refmap", "datalist": datalist,
                       "mask_list": mask_list}}
    cfg = {"model": model, "data": {"target": "main.DataModuleFromConfig", "params": {"batch_size": 2, "validation": node}}}
    path = tmp_path / "obs.yaml"
    path.write_text(yaml.safe_dump(cfg))
    ds = V.build_dataset(load_config(str(path)), V.make_parser().parse_args(["--base", str(path)]))
    assert type(ds) is MaskedRefmapDataset and (ds.split, ds.return_envmap, len(ds), ds.mask_len, ds.transform_func_str) == ("val", True, 3, 3, TRANSFORM)
    # the list may come from the flag when the node does not name it
    del node["params"]["mask_list"]
    path.write_text(yaml.safe_dump(cfg))
    ds = V.build_dataset(load_config(str(path)), V.make_parser().parse_args(["--base", str(path), "--mask_list", mask_list]))
    assert type(ds) is MaskedRefmapDataset and ds.mask_len == 3
    # a null mask_root leaves the node's own class
    node["params"]["mask_root"] = None
    path.write_text(yaml.safe_dump(cfg))
    assert type(V.build_dataset(load_config(str(path)), V.make_parser().parse_args(["--base", str(path)]))) is ParametricRefmapDataset
    # without a node: the flags, with the maps returned
    a = V.make_parser().parse_args(["--base", "x.yaml", "--data_root", str(tmp_path / "maps"), "--datalist", datalist, "--mask_root", str(tmp_path / "masks"),
                                    "--mask_list", mask_list, "--split", "test"])
    (tmp_path / "masks" / "test").mkdir()
    ds = V.build_dataset({"model": model}, a)
    assert type(ds) is MaskedRefmapDataset and (ds.split, ds.t, ds.zdim, ds.size, ds.return_envmap, ds.mask_len) == ("test", "test", 6, 16, True, 3)
    shipped = load_config(os.path.join(ROOT, "configs/drmnet/eval_drmnet.yaml"))
    a = V.make_parser().parse_args(["--base", "x.yaml", "--data_root", str(tmp_path / "maps"), "--datalist", datalist])
    assert type(V.build_dataset(shipped, a)) is ParametricRefmapDataset  # DRMNet's path is unchanged

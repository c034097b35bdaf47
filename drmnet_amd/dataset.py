"""``BaseDataset`` -- the HDR <-> network-space maps either side of both samplers, on the HIP map kernels.

Operator surface of ``dataset.basedataset.BaseDataset`` (reference dataset/basedataset.py:10-112): ``size``, ``transform(x,
dynamic_normalize=False, mask=None)``, ``rescale(x)`` and the ``transform_func`` string -- ``_``-separated map names read like
function composition (``f_g`` = f(g(x))), so ``transform`` runs them right to left and ``rescale`` runs the inverses left to
right.  Here the string is compiled once into two op lists for ``drm_map_chain`` (csrc/transform.hip): a whole chain is ONE pass
over the tensor; the only data-dependent piece, the per-image masked (log10 min, log10 max) of ``normalizedLogarithmic``
(:63-69), is one reduction launch in front of the pass that needs it, and -- like the reference (:69) -- is remembered on the
dataset object for the matching ``rescale``.  GPU tensors only: there is no torch fallback.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import List, Optional, Tuple

import torch

from . import ops

# map name -> (forward step, inverse steps); None = identity.  "@" marks the clamp_before_exp argument, "b" the lowerbound value.
_TABLE = {
    "log": (("log_p1", 0.0), (("exp_m1", "@"),)),
    "log10": (("log10", 0.0), (("exp10", "@"),)),
    "0p1tom1p1": (("unit_to_signed", 0.0), (("signed_to_unit", 0.0),)),
    "normalizedLogarithmic": (("norm_log", 0.0), (("denorm_log", 0.0), ("exp10", "@"))),
}


def _require_gpu(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("BaseDataset maps run on the GPU (drmnet_amd has no CPU path); got a CPU tensor")
    return x.float().contiguous()


class BaseDataset(torch.utils.data.Dataset):
    def __init__(self, size: int, transform_func: str = "log", clamp_before_exp: float = 0.0):
        self.size = size
        self.transform_func_str = transform_func
        # basedataset.py:25: a literal False selects 10; any other value is used as given, and a falsy one means "no clamp" (:88,:94)
        self.clamp_before_exp = 10 if clamp_before_exp is False else clamp_before_exp
        self.Logarithmic_params = None  # [log10min, log10max], each [B, 1, 1, 1] (or [1, 1, 1] for a 3-D input), set by transform(dynamic_normalize=True)
        names = transform_func.split("_")
        # forward program: elementwise segments (one drm_map_chain pass each) cut at every resize, which keeps its position in the
        # chain as in the reference (:29-35: log(resize(x)) is not resize(log(x)), and normalizedLogarithmic's statistics are taken at
        # the resolution its input has at that point)
        self._forward: List = [[]]
        for name in reversed(names):
            if name.startswith("resize"):
                self._forward.append("bilinear" if name == "resize" else name[len("resize"):].replace("-", "_").lower())
                self._forward.append([])
            else:
                self._forward[-1].extend(self._compile(name, inverse=False))
        self._inverse: List[Tuple[str, float]] = []
        for name in names:
            self._inverse.extend(self._compile(name, inverse=True))

    # ------------------------------------------------------------------ compilation of the name string
    def _compile(self, name: str, inverse: bool) -> List[Tuple[str, float]]:
        if not name or "_" in name:
            raise NotImplementedError(name)
        cap = float(self.clamp_before_exp) if self.clamp_before_exp else math.inf
        if name.startswith("resize"):
            return []  # shape change, not an elementwise map: handled in transform(); rescale leaves the size alone (:86-87)
        if name.startswith("lowerbound"):
            return [] if inverse else [("lowerbound", float(name[len("lowerbound"):]))]
        if name not in _TABLE:
            raise NotImplementedError(name)
        fwd, inv = _TABLE[name]
        return [(n, cap if a == "@" else a) for n, a in inv] if inverse else [fwd]

    # kept for callers that ask for a single named map (same (sic) spelling as the reference, :42 / :82)
    def get_tranfrom_func(self, func_name: str):
        steps = self._compile(func_name, inverse=False)
        return lambda x, **kw: self._run(x, steps, **kw)

    def get_rescale_func(self, func_name: str):
        steps = self._compile(func_name, inverse=True)
        return lambda x, **kw: self._run(x, steps)

    # ------------------------------------------------------------------ execution
    def _run(self, x: torch.Tensor, steps, dynamic_normalize: bool = False, mask: Optional[torch.Tensor] = None):
        if not x.is_cuda:
            raise RuntimeError("BaseDataset maps run on the GPU (drmnet_amd has no CPU path); got a CPU tensor")
        x = x.float().contiguous()
        names = [n for n, _ in steps]
        lo = hi = None
        if "norm_log" in names and dynamic_normalize:
            if mask is None:
                raise AssertionError("dynamic_normalize needs a mask")
            cut = names.index("norm_log")
            if cut:  # the statistics are taken on the output of the maps in front (e.g. lowerbound1e-6)
                x = ops.map_chain(x, steps[:cut])
                steps = steps[cut:]
            lo, hi = ops.masked_log_range(x, mask)
            keep = (-1,) + (1,) * 3 if x.ndim >= 4 else (1, 1, 1)
            self.Logarithmic_params = [lo.view(keep), hi.view(keep)]
        if any(n in ("norm_log", "denorm_log") for n, _ in steps):
            if self.Logarithmic_params is None:
                raise RuntimeError("normalizedLogarithmic: call transform(..., dynamic_normalize=True, mask=...) first")
            lo, hi = (p.to(x.device) for p in self.Logarithmic_params)
            if lo.ndim != x.ndim:
                raise AssertionError(f"{x.ndim}, {lo.ndim}, {hi.ndim}")
        return ops.map_chain(x, steps, lo=lo, hi=hi) if steps else x

    def transform(self, x: torch.Tensor, dynamic_normalize: bool = False, mask: torch.Tensor = None):
        assert x.size(-1) >= self.size
        y = x
        for seg in self._forward:
            if isinstance(seg, list):
                if seg:
                    y = self._run(y, seg, dynamic_normalize=dynamic_normalize, mask=mask)
            elif y.shape[-1] != self.size or y.shape[-2] != self.size:
                # (the shipped path never gets here: refmaps are produced at `size`) torchvision's resize(..., antialias=True), :44-50
                y = ops.resize(_require_gpu(y), (self.size, self.size), seg)
        if not y.is_cuda:
            raise RuntimeError("BaseDataset maps run on the GPU (drmnet_amd has no CPU path); got a CPU tensor")
        return y.float().contiguous()

    def rescale(self, x: torch.Tensor):
        return self._run(x, self._inverse)


class ParametricRefmapDataset(BaseDataset):
    """The reference's synthetic validation / test (and training) items (dataset/parametricrefmap.py:16-220): item ``idx`` is environment map
    ``envs[idx]`` with a BRDF code, a point of the schedule and a view drawn from a generator seeded per index -- ``val`` and ``test`` items
    are the same in every epoch, ``train`` items move with ``set_current_epoch``.  The draws keep the reference's order (zK, normalized_k,
    the azimuth out of 64, the unused theta draw, the mask draw) so that an index names the same item as there; ``view_from`` lies on the
    horizontal circle.  With a model attached (``ds.model = drmnet``) whose ``_z0`` exists, ``K, k, zk, zkm1`` come from its
    ``get_schedule`` (``zkm1`` is NaN where K == 0).  ``return_envmap`` adds the map, read with file_io.load_exr.

    ``datalist``: the text file naming one ``<name>.exr`` per line; default the reference's ``data/datalists/<data_root name>/envs_<split>.txt``
    (relative to the working directory).  ``refmap_cache_root`` / ``return_cache`` are accepted and unused: no .pt refmap cache is read, every
    map is rendered by DRMNet.get_input.  ``mask_root`` (the sparse masks of ObsNet's data, read through OpenCV) is not implemented here:
    MaskedRefmapDataset below restates it without OpenCV."""

    def __init__(self, size: int, split: str, data_root: str, zdim: int, transform_func: str = "log", clamp_before_exp: float = 0,
                 return_envmap: bool = False, mask_root: Optional[str] = None, mask_area_min_rate: float = 0.002, epoch_bias: int = 0,
                 epoch_cycle: int = 1000, preload_envmap: bool = False, return_cache: bool = False, refmap_cache_root: Optional[str] = None,
                 datalist: Optional[str] = None):
        super().__init__(size, transform_func=transform_func, clamp_before_exp=clamp_before_exp)
        assert split in ["train", "val", "test"]
        if mask_root is not None:
            raise NotImplementedError("mask_root: the sparse masks belong to ObsNet's training data and need OpenCV")
        self.split = split
        self.root = Path(data_root)
        self.data_name = self.root.name
        with open(datalist if datalist is not None else f"data/datalists/{self.data_name}/envs_{split}.txt", "r") as f:
            self.envs = f.read().splitlines()
        self.with_mask = False
        self.zdim = zdim
        self.return_envmap = return_envmap
        self.generator = torch.Generator()
        self.current_epoch = 0
        self.model = None
        self.return_cache = return_cache
        self.refmap_cache_root = refmap_cache_root
        self.epoch_bias = epoch_bias
        self.epoch_cycle = epoch_cycle
        self.preload_envmap = preload_envmap
        if self.return_envmap and preload_envmap:
            self.envmaps = {env[:-4]: self._load(env[:-4]) for env in self.envs}

    def _load(self, env_name: str) -> torch.Tensor:
        from . import file_io

        return file_io.load_exr(self.root / f"{env_name}.exr", as_torch=True)

    def __len__(self):
        return len(self.envs)

    def set_current_epoch(self, epoch):
        self.current_epoch = epoch

    def set_generator(self, idx: int, epoch: Optional[int] = None):
        """parametricrefmap.py:84-99: train items are keyed by (epoch, idx); val and test items by idx alone, through one and two draws of
        a generator seeded with idx (so the two splits differ on the same index)."""
        draw = lambda: torch.empty((), dtype=torch.int64).random_(generator=self.generator).item()
        if self.split == "train":
            epoch = (epoch or self.current_epoch) + self.epoch_bias
            if epoch >= self.epoch_cycle:
                epoch = epoch % self.epoch_cycle
            self.generator.manual_seed(epoch * len(self) + idx)
        elif self.split == "val":
            self.generator.manual_seed(idx)
            self.generator.manual_seed(draw())
        else:
            self.generator.manual_seed(idx)
            draw()
            self.generator.manual_seed(draw())

    @torch.no_grad()
    def __getitem__(self, idx: int):
        env_name = self.envs[idx][:-4]
        self.set_generator(idx)
        rand = lambda *shape: torch.rand(shape, generator=self.generator)
        zK = rand(self.zdim)
        normalized_k = rand()
        phi = (rand() * 64).int() / 64 * torch.pi * 2 - torch.pi
        theta = (rand() * 0 + 0.5) * torch.pi  # (the reference draws and discards it: every view is on the horizontal circle)
        mask_draw = rand().item()
        # thetaphi2xyz(normal = +y, tangent = +z): cos(theta) y + sin(theta) cos(phi) z + sin(theta) sin(phi) x, summed in that order
        y, z, x = torch.tensor([0.0, 1.0, 0.0]), torch.tensor([0.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 0.0])
        view_from = torch.cos(theta) * y
        view_from += torch.sin(theta) * torch.cos(phi) * z
        view_from += torch.sin(theta) * torch.sin(phi) * x
        data = {"zK": zK, "envmap_name": env_name, "normalized_k": normalized_k, "view_from": view_from}
        z0 = getattr(self.model, "_z0", None) if self.model is not None else None
        if z0 is not None:
            K, k, zk, zkm1 = self.model.get_schedule(zK, z0=z0, normalized_k=normalized_k, return_zkm1=True)
            data.update(K=K, k=k, zk=zk, zkm1=zkm1 if K > 0 else torch.full_like(zkm1, torch.nan))
        if self.return_envmap:
            data["envmap"] = self.envmaps[env_name] if self.preload_envmap else self._load(env_name)
        self._add_mask(data, mask_draw)
        data["tag"] = env_name
        return data

    def _add_mask(self, data: dict, mask_draw: float) -> None:
        """what the item's fifth draw selects (parametricrefmap.py:119-131); nothing without masks"""


def _nearest_indices(src: int, dst: int) -> torch.Tensor:
    """OpenCV's INTER_NEAREST source index of every destination index: min(floor(dst_index * src / dst), src - 1), the scale src / dst taken in
    double precision as cv::resize takes it."""
    scale = float(src) / float(dst)
    return torch.tensor([min(int(math.floor(i * scale)), src - 1) for i in range(dst)], dtype=torch.long)


class MaskedRefmapDataset(ParametricRefmapDataset):
    """ParametricRefmapDataset with the sparse observation masks of ObsNet's data (dataset/parametricrefmap.py:45-52, :119-131), the items
    ObsNetDiffusion.get_input reads for cond_key "masked_LrK".  The parent's fifth draw u picks mask ``int(u * mask_len)`` of the list; a mask
    with fewer than ``H W mask_area_min_rate`` non-zero pixels is passed over for the next index (modulo ``mask_len``); the mask is resized to
    ``size x size`` by the nearest rule and stored under "mask" as ``mask / 255`` (float64, as numpy divides a uint8 array).  Every other
    entry of an item is the parent's, draw for draw.

    ``mask_list``: the text file naming one mask image per line, relative to ``mask_root/<train|test>`` (``val`` items read the ``train``
    directory, as in the reference); default ``data/datalists/<mask_root name>/sparsemaskannotations_<split>.txt``.

    The reference reads and resizes through OpenCV (cv2.imread(..., -1), cv2.resize(..., INTER_NEAREST)), which this project does not depend
    on.  Here Pillow reads the file -- single-channel 8-bit images only, anything else is an error rather than a guess at what imread would
    return -- and the resize is OpenCV's documented nearest rule, source index = min(floor(dst_index * src / dst), src - 1) per axis.  That
    rule is restated from OpenCV's documentation and source, NOT checked against a run of OpenCV: it is not installed where this was written."""

    def __init__(self, size: int, split: str, data_root: str, zdim: int, mask_root: str, mask_area_min_rate: float = 0.002,
                 mask_list: Optional[str] = None, **kwargs):
        super().__init__(size, split, data_root, zdim, mask_root=None, mask_area_min_rate=mask_area_min_rate, **kwargs)
        if mask_root is None:
            raise ValueError("MaskedRefmapDataset needs mask_root")
        self.with_mask = True
        self.mask_root = Path(mask_root)
        self.mask_name = self.mask_root.name
        self.t = "train" if split in ("train", "val") else "test"
        with open(mask_list if mask_list is not None else f"data/datalists/{self.mask_name}/sparsemaskannotations_{split}.txt", "r") as f:
            self.mask_annotations = f.read().splitlines()
        self.mask_len = len(self.mask_annotations)
        if self.mask_len == 0:
            raise ValueError("MaskedRefmapDataset: the mask list is empty")
        self.mask_area_min_rate = mask_area_min_rate

    def _read_mask(self, idx: int):
        import numpy as np
        from PIL import Image

        path = self.mask_root / self.t / self.mask_annotations[idx]
        with Image.open(path) as im:
            if im.mode != "L":
                raise ValueError(f"{path}: a mask must be a single-channel 8-bit image (Pillow mode 'L'), got mode {im.mode!r}")
            return np.array(im, dtype=np.uint8)

    def _add_mask(self, data: dict, mask_draw: float) -> None:
        mask_idx = int(mask_draw * self.mask_len)
        for _ in range(self.mask_len):
            mask = self._read_mask(mask_idx)
            height, width = mask.shape[:2]
            if mask.astype(bool).sum() >= height * width * self.mask_area_min_rate:  # don't use the masks with too small region
                break
            mask_idx = (mask_idx + 1) % self.mask_len
        else:
            raise ValueError(f"no mask of {self.mask_root / self.t} covers {self.mask_area_min_rate} of its image")  # (the reference loops forever)
        rows, cols = _nearest_indices(height, self.size).numpy(), _nearest_indices(width, self.size).numpy()
        data["mask"] = mask[rows][:, cols] / 255

"""Measured BRDFs (MERL tables) on csrc/brdf_table.hip: the file format, the export of an estimated BRDF, and the table as a material.

    python -m drmnet_amd.merl --z m R G B r s --output est.binary        # a principled row exported as a MERL file
    python -m drmnet_amd.merl --input a.binary --figure a.png            # the visualize_bsdf figure of a measured BRDF
    python -m drmnet_amd.merl --input a.binary --fit [--objective log1p|l2] [--output fitted.binary] [--figure f.png]
                                                                         # the closest principled row, as one JSON line
    python -m drmnet_amd.merl --input a.binary --compare --z m R G B r s # the BRDF-space errors of a row against a table, as JSON
    python -m drmnet_amd.merl --compare --z m R G B r s --against a.binary   # the same

Operator surface of the reference: ``load_merl`` / ``save_merl`` (utils/file_io.py:59-103) and ``bsdf_to_merl``
(utils/mitsuba3_utils.py:602-638) keep their names, shapes and file format.  ``MeasuredBSDF`` is the measured counterpart of
``render.PrincipledBSDF``: ``render.eval_bsdf`` / ``render.visualize_bsdf`` take either, ``render.render_table`` renders the sphere,
``relight.render_normals_measured`` an object image from a normal map and ``mesh.render_mesh_measured`` an object image of a triangle
mesh, with or without shadow rays (csrc/mesh_table.hip; ``synthesize --merl``), under it.  The file format and the packing are host numpy;
export, evaluation and rendering run on the GPU (no CPU path).  Fitting principled parameters to a table and the BRDF-space error metrics are
drmnet_amd/reflectance.py (csrc/brdf_error.hip); ``--fit`` and ``--compare`` are its command lines.

Out of scope: light samples and bounces under a table (on the sphere, a normal map or a mesh), anisotropic tables, and
table-against-table errors.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Optional

import numpy as np

RES_THETA_H, RES_THETA_D, RES_PHI_D = 90, 90, 180
SHAPE = (3, RES_THETA_H, RES_THETA_D, RES_PHI_D)
ENTRIES = RES_THETA_H * RES_THETA_D * RES_PHI_D
COLOR_SCALES = np.array([1.0 / 1500.0, 1.15 / 1500.0, 1.66 / 1500.0])
ALPHA_MIN, ALPHA_MAX = 0.005, 1.0


def load_merl(path) -> np.ndarray:
    """utils/file_io.py:82-103: a MERL ``.binary`` file -> float32 [3, 90, 90, 180] = (colour, theta_h, theta_d, phi_d), the colour scales
    applied.  The file is three int32 (90, 90, 180) and 3 * 1458000 float64, colour-major; another dimension product is a ValueError."""
    raw = np.fromfile(str(path), dtype=np.uint8)
    if raw.size < 12:
        raise ValueError("invalid BRDF file")
    dims = raw[:12].view("<i4")
    if int(dims[0]) * int(dims[1]) * int(dims[2]) != ENTRIES or raw.size < 12 + 3 * ENTRIES * 8:
        raise ValueError("invalid BRDF file")
    data = raw[12:12 + 3 * ENTRIES * 8].view("<f8").astype(np.float32).reshape(SHAPE)
    data *= COLOR_SCALES.astype(np.float32).reshape(3, 1, 1, 1)
    return data


def save_merl(data, path) -> None:
    """utils/file_io.py:67-79: data [3, 90, 90, 180] (as load_merl returns it) -> a MERL ``.binary`` file: divided by the colour scales,
    written as float64 in one piece."""
    d = np.asarray(data, dtype=np.float64)
    if d.shape != SHAPE:
        raise ValueError(f"save_merl: data must be {SHAPE}, got {d.shape}")
    d = (d.reshape(3, -1) / COLOR_SCALES.reshape(3, 1)).astype("<f8")
    with open(path, "wb") as f:
        f.write(np.array([RES_THETA_H, RES_THETA_D, RES_PHI_D], dtype="<i4").tobytes())
        f.write(d.tobytes())


def pack_table(table) -> np.ndarray:
    """[3, 90, 90, 180] -> the device layout [90, 90, 180, 4] float32: entry (r, g, b, 0); an entry with a negative channel (no
    measurement / below the horizon) becomes (-1, -1, -1, 0)."""
    t = np.asarray(table, dtype=np.float32)
    if t.shape != SHAPE:
        raise ValueError(f"a table is {SHAPE}, got {t.shape}")
    out = np.zeros((RES_THETA_H, RES_THETA_D, RES_PHI_D, 4), dtype=np.float32)
    out[..., :3] = np.moveaxis(t, 0, -1)
    out[..., :3][(t < 0).any(axis=0) | ~np.isfinite(t).all(axis=0)] = -1.0
    return out


def unpack_table(packed) -> np.ndarray:
    """the inverse of pack_table: [90, 90, 180, 4] -> [3, 90, 90, 180]"""
    p = np.asarray(packed, dtype=np.float32).reshape(RES_THETA_H, RES_THETA_D, RES_PHI_D, 4)
    return np.ascontiguousarray(np.moveaxis(p[..., :3], -1, 0))


def proxy_alpha(table) -> float:
    """The GGX roughness the renders place their specular samples with (they are consistent for any value; it only decides where the accuracy
    goes): the Rec. 709 luminance of the entries (i, 0, 0) is read as a GGX D, whose half maximum lies at tan^2 theta = alpha^2 (sqrt 2 - 1).
    floor = its minimum over valid entries, peak = lum[0] - floor; a peak not above 1e-6 floor is a diffuse table, alpha = 1.  Otherwise x =
    the first index at or below floor + peak / 2, interpolated linearly in index space, theta = (x / 90)^2 pi / 2 and
    alpha = clip(tan theta / sqrt(sqrt 2 - 1), 0.005, 1)."""
    t = np.asarray(table, dtype=np.float64)
    prof = t[:, :, 0, 0]
    lum = 0.2126 * prof[0] + 0.7152 * prof[1] + 0.0722 * prof[2]
    valid = (prof >= 0).all(axis=0)
    if not valid[0]:
        return ALPHA_MAX
    floor = float(lum[valid].min())
    peak = float(lum[0]) - floor
    if not peak > 1e-6 * floor:
        return ALPHA_MAX
    half = floor + 0.5 * peak
    x = float(RES_THETA_H - 1)
    for i in range(1, RES_THETA_H):
        if not valid[i] or lum[i] <= half:
            x = float(i) if (not valid[i] or lum[i - 1] == lum[i]) else (i - 1) + (lum[i - 1] - half) / (lum[i - 1] - lum[i])
            break
    theta = (x / 90.0) ** 2 * (np.pi / 2)
    return float(np.clip(np.tan(theta) / np.sqrt(np.sqrt(2.0) - 1.0), ALPHA_MIN, ALPHA_MAX))


class MeasuredBSDF:
    """One measured BRDF: ``table`` float32 [3, 90, 90, 180] on the host (load_merl's layout; a negative entry marks "no measurement / below
    the horizon") and ``alpha``, the proxy roughness of the renders (proxy_alpha(table) unless given).  Constructing one does not touch
    the GPU; ``device_table(dev)`` packs and uploads it once per device."""

    def __init__(self, table, alpha: Optional[float] = None):
        t = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
        if t.shape != SHAPE:
            raise ValueError(f"a table is {SHAPE}, got {t.shape}")
        self.table = t
        self.alpha = proxy_alpha(t) if alpha is None else float(alpha)
        if not (ALPHA_MIN <= self.alpha <= ALPHA_MAX):
            raise ValueError(f"alpha must be in [{ALPHA_MIN}, {ALPHA_MAX}], got {alpha}")
        self._device = {}

    @classmethod
    def from_file(cls, path, alpha: Optional[float] = None) -> "MeasuredBSDF":
        return cls(load_merl(path), alpha)

    @classmethod
    def from_principled(cls, bsdf, alpha: Optional[float] = None) -> "MeasuredBSDF":
        """the table drm_brdf_to_merl exports for a render.PrincipledBSDF"""
        return cls(np.moveaxis(bsdf_to_merl(bsdf), -1, 0), alpha)

    def device_table(self, dev):
        """the packed table [90, 90, 180, 4] as a tensor on ``dev`` (cached per device)"""
        import torch

        dev = torch.device(dev)
        if dev not in self._device:
            self._device[dev] = torch.from_numpy(pack_table(self.table)).to(dev)
        return self._device[dev]

    def __repr__(self):
        return f"MeasuredBSDF(alpha={self.alpha:g})"


def device_tables(bsdfs, B: int, dev):
    """``bsdfs``: one MeasuredBSDF (shared by all B rows) or a sequence of B -> (tables [NT, 90, 90, 180, 4], table_of int32 [B],
    alpha float32 [NT]) on ``dev``.  Equal objects share one device table."""
    import torch

    if isinstance(bsdfs, MeasuredBSDF):
        bsdfs = [bsdfs] * B
    bsdfs = list(bsdfs)
    if len(bsdfs) != B or not all(isinstance(b, MeasuredBSDF) for b in bsdfs):
        raise ValueError(f"bsdfs must be one MeasuredBSDF or a list of B = {B} of them")
    unique, table_of = [], []
    for b in bsdfs:
        hit = [k for k, u in enumerate(unique) if u is b]
        if not hit:
            unique.append(b)
        table_of.append(hit[0] if hit else len(unique) - 1)
    tables = unique[0].device_table(dev)[None] if len(unique) == 1 else torch.stack([u.device_table(dev) for u in unique])
    return (tables.contiguous(), torch.tensor(table_of, dtype=torch.int32, device=dev),
            torch.tensor([u.alpha for u in unique], dtype=torch.float32, device=dev))


def lookup_mode(lookup: str) -> int:
    """"nearest" -> 0, "linear" -> 1 (the ``linear`` argument of the C entries)"""
    if lookup not in ("nearest", "linear"):
        raise ValueError(f"lookup must be 'nearest' or 'linear', got {lookup!r}")
    return int(lookup == "linear")


def bsdf_to_merl(bsdf, color_scale: bool = False) -> np.ndarray:
    """utils/mitsuba3_utils.py:602-638 through drm_brdf_to_merl: a render.PrincipledBSDF sampled on the MERL grid -> [90, 90, 180, 3] float32
    (the reference's return shape), -1 below the horizon.  ``color_scale`` divides the valid entries' channels by the colour scales, as the
    reference does before it marks the invalid ones."""
    import torch

    from . import _lib
    from .render import _device

    dev = _device()
    z = torch.tensor(bsdf.row, dtype=torch.float32, device=dev).reshape(1, 6)
    out = torch.empty((1, RES_THETA_H, RES_THETA_D, RES_PHI_D, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().drm_brdf_to_merl(z.data_ptr(), 1, out.data_ptr(), _lib.stream_ptr(dev)))
    t = out[0, ..., :3].cpu().numpy()
    if color_scale:
        t = np.where(t < 0, t, t / COLOR_SCALES.astype(np.float32))
    return np.ascontiguousarray(t)


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="export a principled BRDF as a MERL file, or draw the figure of a MERL file")
    p.add_argument("--z", type=float, nargs=6, default=None, metavar=("m", "R", "G", "B", "r", "s"),
                   help="metallic, base colour R G B, roughness, specular: the BRDF to export")
    p.add_argument("--output", type=Path, default=None, help="the MERL file (.binary) --z is written to")
    p.add_argument("--input", type=Path, default=None, help="a MERL file (.binary) to draw")
    p.add_argument("--figure", type=Path, default=None, help="the visualize_bsdf figure (.png) of --input (or of the exported --z)")
    p.add_argument("--lookup", choices=("nearest", "linear"), default="nearest", help="how the figure reads the table (default: MERL's own reader rule)")
    p.add_argument("--fit", action="store_true", help="fit a principled row to --input and print it with its errors as one JSON line; "
                   "--output writes the fitted row's table, --figure draws it")
    p.add_argument("--objective", choices=("log1p", "l2"), default="log1p", help="what --fit minimises (default: rmse_log1p)")
    p.add_argument("--compare", action="store_true", help="print the BRDF-space errors of the row --z against the table --input (or --against) as JSON")
    p.add_argument("--against", type=Path, default=None, help="the MERL file (.binary) --compare holds --z against")
    return p


def parse_args(argv=None) -> argparse.Namespace:
    """the command line with the rules between its options"""
    ap = parser()
    args = ap.parse_args(argv)
    if args.fit and args.compare:
        ap.error("--fit and --compare exclude each other")
    if args.fit:
        if args.input is None:
            ap.error("--fit needs --input, the measured BRDF to fit")
        if args.z is not None or args.against is not None:
            ap.error("--fit takes --input alone (no --z, no --against)")
        return args
    if args.compare:
        if args.z is None:
            if args.input is not None and args.against is not None:
                ap.error("--compare: table-versus-table comparison is out of scope: the first BRDF must be a principled row, given as --z")
            ap.error("--compare needs the row --z and one table, --input or --against")
        if (args.input is None) == (args.against is None):
            ap.error("--compare needs exactly one table to hold --z against: --input or --against")
        return args
    if args.against is not None:
        ap.error("--against belongs to --compare")
    if (args.z is None) == (args.input is None):
        ap.error("exactly one of --z and --input")
    if args.z is not None and args.output is None:
        ap.error("--z needs --output")
    if args.input is not None and args.figure is None:
        ap.error("--input needs --figure")
    return args


def main(argv=None, *, fit_options: Optional[dict] = None):
    """``fit_options``: keywords for reflectance.fit_principled under ``--fit`` (tests pass a small ``starts``)"""
    import json

    args = parse_args(argv)
    from .render import CANONICAL, PrincipledBSDF, visualize_bsdf

    if args.compare:
        from .reflectance import brdf_errors

        target = MeasuredBSDF.from_file(args.input if args.input is not None else args.against, alpha=1.0)
        print(json.dumps(brdf_errors(np.clip(args.z, 0.0, 1.0), target)))
        return
    if args.fit:
        from .reflectance import fit_principled

        fit = fit_principled(MeasuredBSDF.from_file(args.input, alpha=1.0), objective=args.objective, **(fit_options or {}))
        print(json.dumps({"z": dict(zip(CANONICAL, fit["z"])), "objective": fit["objective"], "errors": fit["errors"], "rounds": fit["rounds"],
                          "evaluations": fit["evaluations"]}))
        if args.output is None and args.figure is None:
            return
        args.z, args.input = fit["z"], None  # (what follows exports and draws the fitted row)
    if args.z is not None and args.output is None:
        bsdf = MeasuredBSDF.from_principled(PrincipledBSDF(np.clip(args.z, 0.0, 1.0)))
    elif args.z is not None:
        bsdf = MeasuredBSDF.from_principled(PrincipledBSDF(np.clip(args.z, 0.0, 1.0)))
        save_merl(bsdf.table, args.output)
        print(f"wrote {args.output} (proxy alpha {bsdf.alpha:.4g})")
    else:
        bsdf = MeasuredBSDF.from_file(args.input)
    if args.figure is not None:
        from . import file_io
        from .transform import hdr2ldr

        fig, mask = visualize_bsdf(bsdf, lookup=args.lookup)
        file_io.save_png(args.figure, hdr2ldr(fig), mask=mask)  # (tone-mapped like estimate.save_brdf_png)
        print(f"wrote {args.figure}")


if __name__ == "__main__":
    main()

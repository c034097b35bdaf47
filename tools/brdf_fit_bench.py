#!/usr/bin/env python3
"""Time the BRDF-space error sums (csrc/brdf_error.hip) and the principled fit built on them.

    python tools/brdf_fit_bench.py [--reps 10] [--warmup 2] [--rows 1 104 1024] [--no-fit] [--out result.json]

For every C of --rows: one drm_brdf_error_sums launch of C candidate rows against one table, and next to it the first half of what it
replaces, drm_brdf_to_merl of the same C rows (in launches of at most 128 rows into one reused buffer: 23 MB per row); the other half,
reducing the C exported tables, is not timed, so the ratio understates the gain.  Also timed: the host route for ONE row -- export, copy to
the host, the nine sums in numpy float64 -- and one whole fit_principled at its defaults.  Device work is timed with events over `reps` calls
after `warmup` calls, the host route and the fit with the wall clock around a synchronised call.  The fused sums of one row are compared
with the host route's first.  Prints one JSON line.  Not part of bench.py: earlier revisions have no such kernel to compare with.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXED = (0.3, 0.7, 0.5, 0.3, 0.8, 0.6)
EXPORT_CHUNK = 128


def host_sums(a, b, ci, lit):
    """the nine sums of reflectance.brdf_error_sums for tables a, b [3, 90, 90, 180] in numpy float64"""
    counts = lit & (b >= 0).all(axis=0)
    a, b, ci = a[:, counts].astype(np.float64), b[:, counts].astype(np.float64), ci[counts][None]
    both = (a > 0) & (b > 0)
    d = np.log10(a[both]) - np.log10(b[both])
    l = np.log1p(a * ci) - np.log1p(b * ci)
    return np.array([a.size, both.sum(), d.sum(), (d * d).sum(), (l * l).sum(), (((a - b) * ci) ** 2).sum(), ((a * ci) ** 2).sum(),
                     (a * ci * b * ci).sum(), ((b * ci) ** 2).sum()])


def grid_cosines():
    i, j, k = np.meshgrid(np.arange(90.0), np.arange(90.0), np.arange(180.0), indexing="ij")
    th, td, pd = (i / 90.0) ** 2 * (np.pi / 2), j * (np.pi / 180), k * (np.pi / 180)
    co = -np.sin(th) * np.sin(td) * np.cos(pd) + np.cos(th) * np.cos(td)
    ci = np.sin(th) * np.sin(td) * np.cos(pd) + np.cos(th) * np.cos(td)
    co, ci = np.where(np.abs(co) < 1e-12, 0.0, co), np.where(np.abs(ci) < 1e-12, 0.0, ci)
    return ci, (co > 0) & (ci > 0)


def device_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [min(out), max(out)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=(1, 104, 1024))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-fit", action="store_true", help="skip the whole fit")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("brdf_fit_bench times GPU kernels and no GPU is visible")
    from drmnet_amd import _lib, merl
    from drmnet_amd import reflectance as rf
    from drmnet_amd.render import PrincipledBSDF

    dev = torch.device("cuda", torch.cuda.current_device())
    lib, stream = _lib.lib(), _lib.stream_ptr(dev)
    target = merl.MeasuredBSDF.from_principled(PrincipledBSDF(MIXED), alpha=1.0)
    table = target.device_table(dev)
    result = {"workload": "drm_brdf_error_sums of C rows against one table of 1458000 entries", "reps": a.reps, "rows": {}}
    cmax = max(a.rows)
    cands = torch.from_numpy(rf.halton(cmax).astype(np.float32)).to(dev)
    ws = torch.empty(_lib.brdf_error_workspace_bytes(cmax) // 8, dtype=torch.float64, device=dev)
    sums = torch.empty((cmax, rf.SUMS), dtype=torch.float64, device=dev)
    tables = torch.empty((min(cmax, EXPORT_CHUNK), 90, 90, 180, 4), dtype=torch.float32, device=dev)
    for C in a.rows:
        def fused():
            _lib.check(lib.drm_brdf_error_sums(cands.data_ptr(), C, table.data_ptr(), None, ws.data_ptr(), _lib.brdf_error_workspace_bytes(C),
                                               sums.data_ptr(), stream))

        def export():
            for at in range(0, C, EXPORT_CHUNK):
                n = min(EXPORT_CHUNK, C - at)
                _lib.check(lib.drm_brdf_to_merl(cands[at:].data_ptr(), n, tables.data_ptr(), stream))

        f_ms, f_range = device_ms(fused, a.reps, a.warmup)
        e_ms, e_range = device_ms(export, a.reps, a.warmup)
        result["rows"][str(C)] = {"error_sums_ms": f_ms, "error_sums_ms_min_max": f_range, "export_only_ms": e_ms, "export_only_ms_min_max": e_range,
                                  "export_over_fused": e_ms / f_ms}
    # the host route for one row, and its agreement with the kernel
    ci, lit = grid_cosines()
    row = cands[:1].cpu().numpy().astype(np.float64)[0]

    def host():
        t = np.moveaxis(merl.bsdf_to_merl(PrincipledBSDF(row)), -1, 0)
        return host_sums(t, target.table, ci, lit)

    ref = host()
    got = rf.brdf_error_sums(row, target)[0]
    result["fused_vs_host_max_rel"] = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        times.append((time.perf_counter() - t0) * 1e3)
    result["host_numpy_one_row_ms"] = float(np.median(times))
    if not a.no_fit:
        rf.brdf_error_sums(row, target)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = rf.fit_principled(target)
        result["fit"] = {"seconds": time.perf_counter() - t0, "objective": fit["objective"], "rounds": fit["rounds"], "evaluations": fit["evaluations"],
                         "z": fit["z"]}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return result


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timings behind DESIGN.md's forward-process paragraph (one MI355X).

    python tools/forward_bench.py render [--libs - drmnet_amd/csrc/_ab/libdrmnet_hip_copy.so]
        L x B stacked rows at R = 128 through one drm_render_refmap call (maps indexed per row) against the same L B rows as one set
        (L = 1) with the maps expanded L times, per library, alternating ("-" = the product library).
        --light_samples M also times the same stacked rows with light samples (the density and table launches included; under
        `rocprofv3 --kernel-trace --stats` the three light kernels and the render show on their own).
    python tools/forward_bench.py render --entries --libs - A.so B.so [--reps 10 --rounds 2] [--mesh_batch 4] [--match table normals]
        one call each of drm_render_refmap (plain, lit, under tables), drm_render_normals (plain, lit, under tables) and drm_render_mesh
        (plain, shadowed, lit, bounced) and drm_render_mesh_tables (plain, shadowed) at B rows, 128 x 128, maps 128 x 256, quad 32, subpixel 2, M = 1024, a mesh of 20 480 faces; device
        events, the libraries alternating in every round, and whether every library wrote the same bits.  The case labels are those of the
        logs recorded before the entries were merged (DESIGN.md maps them), so old and new logs line up.  Two copies of one library under
        two names give the spread that a difference between two libraries has to exceed.
    python tools/forward_bench.py step [--batch 20]
        one DRMNet.validation_step at full width (synthetic weights, 128 x 128, 128 x 256 maps) split into forward process (renders +
        transforms), networks and loss by device events.  Run it under `rocprofv3 --kernel-trace --stats -- python ...` for the kernel table.
    python tools/forward_bench.py obs_step [--batch 20]
        the same for one pass of ObsNetDiffusion's validation at full width (configs/obsnet/eval_obsnet.yaml's network with the validation
        keys of the reference's train_obsnet.yaml, synthetic weights, 128 x 128, 128 x 256 maps, random sparse masks): get_input (render,
        masked transform, conditioning half of drm_obs_forward_process), q_sample half + network, drm_diffusion_losses.
    python tools/forward_bench.py image_errors [--reps 10 --rounds 2]
        64 draws of one 128 x 128 object image ranked by re-render error (samples.rerender_errors end to end, the image-error call alone, its
        launches alone) against the same 64 comparisons through the host path relight.image_errors, and the 4096 pairs of
        samples.pairwise_distances at N = 64; device events around each call (the host work of a call ends inside its window).
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def bench_render(args):
    from drmnet_amd import _lib

    if args.entries:
        return bench_entries(args)
    dev = torch.device("cuda:0")
    L, B, R = args.stack, args.batch, 128
    libs = [(path, C.CDLL(_lib.LIB_PATH if path == "-" else os.path.join(ROOT, path))) for path in args.libs]
    g = torch.Generator().manual_seed(1)
    z = torch.rand((L, B, 6), generator=g).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = C.c_void_p
    for EH, EW in ((128, 256), (1000, 2000)):
        env = (torch.rand((B, EH, EW, 3), generator=g) + 0.05).to(dev)
        out = torch.empty((L, B, 3, R, R), device=dev)
        stacked_sh = _lib.sized(_lib.Shading, B=B, z=z.data_ptr(), envmap=env.data_ptr(), EH=EH, EW=EW, quad=32)

        def expanded(lib):
            e = env[None].expand(L, *env.shape).reshape(L * B, *env.shape[1:])  # (the copy is part of what is timed)
            sh = _lib.sized(_lib.Shading, B=L * B, z=z.data_ptr(), envmap=e.data_ptr(), EH=EH, EW=EW, quad=32)
            assert lib.drm_render_refmap(C.byref(sh), 1, R, 2, 0, vp(out.data_ptr()), stream) == 0

        def stacked(lib, sh=stacked_sh):
            assert lib.drm_render_refmap(C.byref(sh), L, R, 2, 0, vp(out.data_ptr()), stream) == 0

        results = {}
        for rep in range(args.rounds):
            for name, lib in libs:
                if args.light_samples:
                    lit_sh, _keep = _lib.make_shading(B, z=z, env=env, quad=32, light_samples=args.light_samples)
                    results.setdefault((name, f"drm_render_refmap_lit M={args.light_samples}"), []).extend(timed(lambda: stacked(lib, lit_sh), args.reps))
                results.setdefault((name, "expanded + drm_render_refmap"), []).extend(timed(lambda: expanded(lib), args.reps))
                results.setdefault((name, "drm_render_refmap_views"), []).extend(timed(lambda: stacked(lib), args.reps))
        # every form of every library renders the same bits
        ref = None
        for name, lib in libs:
            for form, call in (("expanded", expanded), ("stacked", stacked)):
                out.zero_()
                call(lib)
                torch.cuda.synchronize()
                ref = out.clone() if ref is None else ref
                print(f"maps {EH}x{EW}  [{name}] {form}: bitwise equal to the first form: {torch.equal(out, ref)}", flush=True)
        for (name, form), ms in results.items():
            ms = sorted(ms)
            print(f"maps {EH}x{EW} L={L} B={B} R={R}  [{name}] {form}: median {ms[len(ms) // 2]:.2f} ms  min {ms[0]:.2f}  max {ms[-1]:.2f}  (n={len(ms)})", flush=True)
        del env


def bench_entries(args):
    """render --entries: the table, normal-map and mesh entries (and the sphere's, plain and lit), per library, alternating in every round"""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_ref

    from drmnet_amd import _lib
    from drmnet_amd.merl import MeasuredBSDF, device_tables
    from drmnet_amd.mesh import build_bvh
    from drmnet_amd.render import get_bsdf, view_rotation

    dev = torch.device("cuda:0")
    B, Bm, R, EH, EW, Q, S, M = args.batch, args.mesh_batch or args.batch, 128, 128, 256, 32, 2, args.light_samples or 1024
    names = ["metallic.value", "base_color.value.R", "base_color.value.G", "base_color.value.B", "roughness.value", "specular"]
    libs = [(path, C.CDLL(_lib.LIB_PATH if path == "-" else os.path.join(ROOT, path))) for path in args.libs]
    g = torch.Generator().manual_seed(1)
    z = torch.rand((B, 6), generator=g).to(dev)
    env = (torch.rand((B, EH, EW, 3), generator=g) + 0.05).to(dev)
    phi = torch.rand((B,), generator=g) * 6.2831853
    view = view_rotation(torch.stack([torch.sin(phi), 0.3 * torch.ones(B), torch.cos(phi)], dim=-1)).to(dev)
    nrm = torch.randn((B, R, R, 3), generator=g)
    nrm[..., 2] = nrm[..., 2].abs() + 0.1
    nrm = nrm.to(dev)
    measured = [MeasuredBSDF.from_principled(get_bsdf(row, names)) for row in ([0.0, 0.7, 0.5, 0.3, 0.5, 0.6], [1.0, 0.7, 0.5, 0.3, 0.3, 0.6])]
    tables, table_of, alpha = device_tables([measured[b % 2] for b in range(B)], B, dev)
    # 20 480 faces that shadow and light one another: a body and three balls, icosphere(4) each (the scene of shadow_ref.two_spheres, finer)
    _, d, f = mesh_ref.icosphere(4)
    centres = [(0.0, 0.0, 0.0, 0.5), (0.40, 0.35, 0.30, 0.2), (-0.45, 0.30, 0.25, 0.2), (0.10, -0.50, 0.30, 0.2)]
    obj = {"vertex_positions": torch.tensor(np.concatenate([r * d + np.array([x, y, zc]) for x, y, zc, r in centres]), dtype=torch.float32),
           "vertex_normals": torch.tensor(np.concatenate([d] * 4), dtype=torch.float32),
           "faces": torch.tensor(np.concatenate([f + k * len(d) for k in range(4)]), dtype=torch.int32)}
    pos, vn, faces = (obj[k].to(dev).contiguous() for k in ("vertex_positions", "vertex_normals", "faces"))
    blob = build_bvh(obj).to(dev)
    V, F = int(pos.shape[0]), int(faces.shape[0])
    lbytes = int(_lib.lib().drm_render_light_workspace_bytes(B, EH, EW, M))
    mbytes = int(_lib.lib().drm_render_mesh_workspace_bytes(F, Bm, R, R, S))
    assert lbytes > 0 and mbytes > 0
    lws = torch.empty(((lbytes + 7) // 8,), dtype=torch.float64, device=dev)
    mws = torch.empty(((mbytes + 15) // 16, 2), dtype=torch.float64, device=dev)
    out = torch.empty((B, 3, R, R), device=dev)
    drawn = torch.empty((B, R, R), device=dev)
    mesh_out = [torch.empty((Bm, c, R, R), device=dev) for c in (3, 3, 1, 1)]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    # the shadings: B rows (Bm for the mesh) of principled rows or tables under the maps and views, plain or with M light samples
    def shading(rows, lit=False, measured=False):
        sh = _lib.sized(_lib.Shading, B=rows, envmap=env.data_ptr(), EH=EH, EW=EW, view=view.data_ptr(), quad=Q)
        if measured:
            sh.tables, sh.NT, sh.table_of, sh.table_alpha, sh.table_linear = tables.data_ptr(), int(tables.shape[0]), table_of.data_ptr(), alpha.data_ptr(), 1
        else:
            sh.z = z.data_ptr()
        if lit:
            sh.light_samples, sh.light_workspace, sh.light_workspace_bytes = M, lws.data_ptr(), lbytes
        return sh

    def mesh(**technique):
        return _lib.sized(_lib.MeshRender, vertex_positions=pos.data_ptr(), vertex_normals=vn.data_ptr(), faces=faces.data_ptr(), V=V, F=F, H=R, W=R,
                          subpixel=S, image=mesh_out[0].data_ptr(), normal=mesh_out[1].data_ptr(), depth=mesh_out[2].data_ptr(),
                          alpha=mesh_out[3].data_ptr(), workspace=mws.data_ptr(), workspace_bytes=mbytes, **technique)

    shadowed = dict(shadows=1, bvh=blob.data_ptr(), bvh_bytes=int(blob.numel()))

    def entries(lib):
        def refmap(sh):
            return [out], lambda: lib.drm_render_refmap(C.byref(sh), 1, R, S, 0, vp(out), stream)

        def normals(sh):
            return [out, drawn], lambda: lib.drm_render_normals(C.byref(sh), vp(nrm), None, B, R, R, vp(out), vp(drawn), stream)

        def meshes(sh, m):
            return mesh_out, lambda: lib.drm_render_mesh(C.byref(sh), C.byref(m), stream)

        def meshes_tables(sh, m):
            return mesh_out, lambda: lib.drm_render_mesh_tables(C.byref(sh), C.byref(m), stream)

        # (a library from before the entry existed is timed on the others)
        measured_mesh = {
            f"drm_render_mesh_tables B={Bm}": meshes_tables(shading(Bm, measured=True), mesh()),
            f"drm_render_mesh_tables_shadowed B={Bm}": meshes_tables(shading(Bm, measured=True), mesh(**shadowed)),
        } if hasattr(lib, "drm_render_mesh_tables") else {}
        return {
            "drm_render_refmap_views": refmap(shading(B)),
            f"drm_render_refmap_lit M={M}": refmap(shading(B, lit=True)),
            "drm_render_refmap_table": refmap(shading(B, measured=True)),
            "drm_render_normals": normals(shading(B)),
            f"drm_render_normals M={M}": normals(shading(B, lit=True)),
            "drm_render_normals_table": normals(shading(B, measured=True)),
            f"drm_render_mesh B={Bm}": meshes(shading(Bm), mesh()),
            f"drm_render_mesh_shadowed B={Bm}": meshes(shading(Bm), mesh(**shadowed)),
            f"drm_render_mesh_lit B={Bm} M={M}": meshes(shading(Bm, lit=True), mesh()),
            f"drm_render_mesh_bounced B={Bm}": meshes(shading(Bm), mesh(bounces=1, bounce_quad=4, **shadowed)),
            **measured_mesh,
        }

    results, bits = {}, {}
    for rep in range(args.rounds):
        for name, lib in libs:
            for entry, (outs, call) in entries(lib).items():
                if args.match and not any(m in entry for m in args.match):
                    continue

                def run():
                    assert call() == 0

                results.setdefault((entry, name), []).extend(timed(run, args.reps))
                torch.cuda.synchronize()
                bits.setdefault(entry, []).append((name, [t.clone() for t in outs]))
    for entry, seen in bits.items():
        same = all(torch.equal(a, b) for _, o in seen[1:] for a, b in zip(seen[0][1], o))
        print(f"{entry}: every library, every round, bitwise equal outputs: {same}", flush=True)
    for (entry, name), ms in results.items():
        ms = sorted(ms)
        print(f"B={B} {R}x{R} maps {EH}x{EW} Q={Q} S={S}  {entry}  [{name}]: median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}  (n={len(ms)})",
              flush=True)


def bench_step(args):
    from drmnet_amd import synth
    from drmnet_amd.config import load_config
    from drmnet_amd.dataset import BaseDataset
    from drmnet_amd.drmnet import DRMNet

    dev = torch.device("cuda:0")
    params = dict(load_config(os.path.join(ROOT, "configs/drmnet/eval_drmnet.yaml"))["model"]["params"], ckpt_path=None, use_ema=False)
    m = DRMNet(**params)
    synth.load_synth(m.illnet_model.diffusion_model, synth.SEED_ILLNET)
    synth.load_synth(m.refnet_model.diffusion_model, synth.SEED_REFNET)
    zman = [(k, tuple(v.shape)) for k, v in m.illnet_model.z_emb_layer.state_dict().items()]
    m.illnet_model.z_emb_layer.load_state_dict(synth.synth_state_dict(zman, synth.SEED_ZEMB))
    m.ds = BaseDataset(128, "log", clamp_before_exp=20)
    m = m.to(dev).set_precision(args.precision)
    B = args.batch
    g = torch.Generator().manual_seed(2)
    zK = torch.rand((B, 6), generator=g)
    K, k, zk, zkm1 = m.get_schedule(zK, z0=m._z0, normalized_k=torch.rand((B,), generator=g), return_zkm1=True)
    phi = torch.rand((B,), generator=g) * 6.2831853
    batch = {"zK": zK, "K": K, "k": k, "zk": zk, "zkm1": zkm1, "envmap_name": [f"e{i}" for i in range(B)],
             "view_from": torch.stack([torch.sin(phi), torch.zeros(B), torch.cos(phi)], dim=-1),
             "envmap": (torch.rand((B, 128, 256, 3), generator=g) + 0.05).to(dev)}
    parts = {}

    def step():
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        marks[0].record()
        K_, k_, Lr_K, Lr_k, Lr_km1, zK_, zk_, ic, rc = m.get_input(batch)
        marks[1].record()
        reversed_k = K_ - k_ - 1
        noised = Lr_k + 0.02 * torch.randn_like(Lr_k)
        model_out, z_out = m(noised, ic, rc, reversed_k.long())
        marks[2].record()
        from drmnet_amd import ops

        out = ops.validation_losses(model_out, noised, Lr_km1, K_, z_out, zk_, zK_, reversed_k, m.z0, m.gamma, "l2", 10.0, 0.1)
        marks[3].record()
        marks[3].synchronize()
        for name, i in (("forward process (renders + transforms)", 0), ("networks", 1), ("loss", 2)):
            parts.setdefault(name, []).append(marks[i].elapsed_time(marks[i + 1]))
        return out

    step()
    parts.clear()
    t0 = time.time()
    for _ in range(args.reps):
        out = step()
    wall = (time.time() - t0) / args.reps * 1e3
    for name, ms in parts.items():
        ms = sorted(ms)
        print(f"validation step B={B} {args.precision}: {name}: median {ms[len(ms) // 2]:.2f} ms (min {ms[0]:.2f}, max {ms[-1]:.2f}, n={len(ms)})")
    print(f"validation step B={B} {args.precision}: wall {wall:.1f} ms per pass of one weight set; losses {out.tolist()}", flush=True)


def bench_obs_step(args):
    from drmnet_amd import ops, synth
    from drmnet_amd.config import load_config
    from drmnet_amd.dataset import BaseDataset
    from drmnet_amd.obsnet import ObsNetDiffusion
    from drmnet_amd.render import RefMapRenderer

    dev = torch.device("cuda:0")
    params = dict(load_config(os.path.join(ROOT, "configs/obsnet/eval_obsnet.yaml"))["model"]["params"], ckpt_path=None, use_ema=False,
                  cond_stage_key="masked_LrK", noisy_observe=0.04, masked_loss=False)
    m = ObsNetDiffusion(**params)
    names = ["metallic.value", "base_color.value.R", "base_color.value.G", "base_color.value.B", "roughness.value", "specular"]
    m.renderer = RefMapRenderer(128, brdf_param_names=names)
    synth.load_synth(m.model.diffusion_model, synth.SEED_OBSNET)
    m.ds = BaseDataset(128, "0p1tom1p1_normalizedLogarithmic_lowerbound1e-6")
    m = m.to(dev).set_precision(args.precision)
    B = args.batch
    g = torch.Generator().manual_seed(2)
    phi = torch.rand((B,), generator=g) * 6.2831853
    batch = {"zK": torch.rand((B, 6), generator=g), "envmap_name": [f"e{i}" for i in range(B)],
             "view_from": torch.stack([torch.sin(phi), torch.zeros(B), torch.cos(phi)], dim=-1),
             "envmap": (torch.rand((B, 128, 256, 3), generator=g) + 0.05).to(dev), "mask": (torch.rand((B, 128, 128), generator=g) > 0.7).double()}
    t = torch.randint(0, m.num_timesteps, (B,), generator=g).to(dev)
    parts = {}

    def step():
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        marks[0].record()
        x, c, mask = m.get_input(batch, "LrK", seed=7)
        marks[1].record()
        _, x_noisy, noise = ops.obs_forward_process(x, None, t, m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, seed=7, want_cond=False)
        model_out = m.apply_model(x_noisy, t, c)
        marks[2].record()
        out = ops.diffusion_losses(model_out, noise, t, m.logvar, m.lvlb_weights, "l2", 1.0, 0.0)
        marks[3].record()
        marks[3].synchronize()
        for name, i in (("get_input (render + masked transform + conditioning)", 0), ("q_sample + network", 1), ("loss", 2)):
            parts.setdefault(name, []).append(marks[i].elapsed_time(marks[i + 1]))
        return out

    step()
    parts.clear()
    t0 = time.time()
    for _ in range(args.reps):
        out = step()
    wall = (time.time() - t0) / args.reps * 1e3
    for name, ms in parts.items():
        ms = sorted(ms)
        print(f"ObsNet validation step B={B} {args.precision}: {name}: median {ms[len(ms) // 2]:.2f} ms (min {ms[0]:.2f}, max {ms[-1]:.2f}, n={len(ms)})")
    print(f"ObsNet validation step B={B} {args.precision}: wall {wall:.1f} ms per pass of one weight set; losses {out.tolist()}", flush=True)


def bench_image_errors(args):
    """image_errors: N = 64 draws of one 128 x 128 object image ranked (samples.rerender_errors: warp, render, one image-error call of 64
    pairs), the image-error call alone, its three launches alone, the same 64 comparisons through the host path relight.image_errors, and
    samples.pairwise_distances at N = 64 (4096 pairs of 128 x 128 mirror maps) with its launches alone"""
    import numpy as np

    from drmnet_amd import _lib, ops, relight, samples
    from drmnet_amd.synthesize import NAMES

    class Model:  # what samples.rerender_errors asks of a DRMNet: the mirror-map warp (no basis division), the map size, the parameter names
        image_size, brdf_param_names = 128, NAMES

        @staticmethod
        def r0toenvmap(r0, shape):
            return ops.mirmap2envmap(r0, shape, channels_last=True)

    dev = torch.device("cuda:0")
    N, H, W = 64, 128, 128
    g = torch.Generator().manual_seed(4)
    Lr0 = (torch.rand((N, 3, 128, 128), generator=g) + 0.05).to(dev)
    zK = torch.rand((N, 6), generator=g).to(dev)
    y, x = torch.meshgrid(torch.linspace(1, -1, H), torch.linspace(-1, 1, W), indexing="ij")
    r2 = x * x + y * y
    normal = torch.stack([x, y, torch.sqrt((1 - r2).clamp_min(0))], dim=-1).to(dev)
    mask = (r2 < 0.98).to(dev)
    envs = Model.r0toenvmap(Lr0, (128, 256))
    images, _ = relight.render_normals(normal, zK, NAMES, envs, mask=mask)
    target = images[0].permute(1, 2, 0).contiguous() * 1.1 + 0.01

    def launches(a, b, m, pairs):
        """the entry alone on prepared arguments: what a caller that keeps its buffers pays"""
        ta, Ba, sa = relight._image_stack("bench", "a", a, *m.shape[-2:])
        tb, Bb, sb = relight._image_stack("bench", "b", b, *m.shape[-2:])
        m8 = (m != 0).to(torch.uint8).reshape(-1, m.shape[-2] * m.shape[-1]).contiguous()
        P = len(pairs)
        triples = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(dev)
        nbytes = _lib.image_error_workspace_bytes(P)
        ws, sums = torch.empty(nbytes // 8, dtype=torch.float64, device=dev), torch.empty((P, 10), dtype=torch.float64, device=dev)
        s = _lib.sized(_lib.ImageError, a=ta.data_ptr(), a_count=Ba, a_batch_stride=sa[0], a_pixel_stride=sa[1], a_channel_stride=sa[2], b=tb.data_ptr(),
                       b_count=Bb, b_batch_stride=sb[0], b_pixel_stride=sb[1], b_channel_stride=sb[2], mask=m8.data_ptr(), mask_count=int(m8.shape[0]),
                       HW=int(m8.shape[1]), pairs=triples.data_ptr(), P=P, workspace=ws.data_ptr(), workspace_bytes=nbytes, sums=sums.data_ptr())
        keep = (ta, tb, m8, triples, ws, sums)
        return lambda: (_lib.check(_lib.lib().drm_image_error_sums(s, _lib.stream_ptr(dev))), keep)[0]

    def host_loop():
        return [relight.image_errors(images[i].permute(1, 2, 0), target, mask) for i in range(N)]

    i, j = np.divmod(np.arange(N * N), N)
    cases = [("samples.rerender_errors N=64 (warp + render + errors, figures on the host)", lambda: samples.rerender_errors(Model, Lr0, zK, target, normal, mask)),
             ("relight.image_errors_batch 64 pairs (call + [64, 10] copy + figures)", lambda: relight.image_errors_batch(images, target, mask)),
             ("drm_image_error_sums 64 pairs, launches alone", launches(images, target, mask, [(k, 0, 0) for k in range(N)])),
             ("relight.image_errors x 64 (the host path: 2 x 64 copies + numpy)", host_loop),
             ("samples.pairwise_distances N=64 (4096 pairs, figures on the host)", lambda: samples.pairwise_distances(Lr0)),
             ("drm_image_error_sums 4096 pairs, launches alone", launches(Lr0, Lr0, torch.ones((128, 128), device=dev), np.stack([i, j, 0 * i], axis=1)))]
    results = {}
    for _ in range(args.rounds):
        for name, fn in cases:
            results.setdefault(name, []).extend(timed(fn, args.reps))
    batch, host = relight.image_errors_batch(images, target, mask), host_loop()
    worst = max(abs(b[k] - h[k]) / max(abs(h[k]), 1e-300) for b, h in zip(batch, host) for k in h if h[k] != 0)
    print(f"image errors, {N} renders of {H}x{W} against one input, {int(mask.sum())} masked pixels: batch against host path, largest relative difference {worst:.2e}")
    for name, ms in results.items():
        ms = sorted(ms)
        print(f"{name}: median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}  (n={len(ms)})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["render", "step", "obs_step", "image_errors"])
    ap.add_argument("--libs", nargs="*", default=["-"])
    ap.add_argument("--stack", type=int, default=4)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--precision", default="f16mx")
    ap.add_argument("--light_samples", type=int, default=0, help="render: also time the stacked render with this many light samples per map")
    ap.add_argument("--entries", action="store_true", help="render: time the sphere, table, normal-map and mesh entries per library instead")
    ap.add_argument("--mesh_batch", type=int, default=0, help="render --entries: rows of the mesh entries (default: --batch)")
    ap.add_argument("--match", nargs="*", default=[], help="render --entries: only the entries whose name contains one of these")
    a = ap.parse_args()
    {"render": bench_render, "step": bench_step, "obs_step": bench_obs_step, "image_errors": bench_image_errors}[a.what](a)

"""Mesh object images under measured BRDFs on the GPU (drm_render_mesh_tables: mesh_table_shade_kernel<VIEW, SHADOW> in csrc/mesh_table.hip,
through drmnet_amd.mesh.render_mesh_measured and synthesize --merl) against the float64 restatement tests/mesh_merl_ref.py.

The scene is shadow_ref.two_spheres() on a 16 x 16 film, Q = 8, S = 2, from the three views of test_gpu_shadow, under smooth_env(16, 32) and
white; the tables are test_gpu_merl's: `smooth` (alpha 0.45) and `dielectric` / `metallic`, exported rows with their proxy_alpha.

Bars.  Against the restatement: rel-L2 <= 1e-5 beyond the slack on safe pixels, the bar the principled shadowed mesh and the table renders
hold; the caps of test_gpu_shadow (CAP = 0.02 on marginal rays of the traced ones, unsafe samples and the slack's share of the image sum),
occluded share >= 0.01, traced >= 10 000, safe >= 0.9, >= 50 lit safe pixels, asserted on the restatement before anything is compared.  The
restatement alone, over the nine (view, table) cases and both environments: marginal <= 1.07 %, unsafe <= 0.59 %, slack share <= 1.71 %
(view 0, metallic, white), occluded 1.47 .. 3.46 %, traced 29 304 .. 33 872, 62 .. 75 lit safe pixels.  The shadow: rel-L2(shadowed, plain)
> 1e-2 (the restatement: 3.8 % .. 13.8 %).  An exported table against its own row under drm_render_mesh: above 1e-4 and at most 5e-2 (the
restatement: 0.85 % .. 2.2 % at Q = 8, the table's discretisation, not kernel error; the bar is a little over twice that)."""
import functools

import numpy as np
import pytest
import torch

import mesh_merl_ref as mm
import mesh_ref as mr
import shadow_ref as sr
from conftest import rel_l2
from test_gpu_merl import DIELECTRIC, METALLIC, measured
from test_gpu_mesh import ENV, as_obj, rotation
from test_gpu_shadow import CAP, FILM, Q, S, SCENE, VIEWS, view_rot
from test_render_cpu import NAMES6

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TABLES = ["smooth", "dielectric", "metallic"]
CASES = [(v, t) for v in range(len(VIEWS)) for t in range(len(TABLES))]
INVALID, WORKSPACE = 1, 3


def alpha_of(name):
    """the proxy roughness as the GPU is given it"""
    return float(np.float32(measured(name).alpha))


def gpu_render(mesh, names, envs, views, shadows, H=FILM, W=FILM, S=S, bvh=None, lookup="linear"):
    from drmnet_amd.mesh import render_mesh_measured

    env = None if envs is None else torch.tensor(np.asarray(envs), dtype=torch.float32, device=DEV)
    view = None if views is None else torch.tensor(views, dtype=torch.float32)
    bsdfs = [measured(n) for n in names]
    return [t.cpu().numpy().astype(np.float64) for t in render_mesh_measured(as_obj(*mesh), bsdfs, env, image_size=(H, W), view_from=view, quad=Q,
                                                                           subpixel=S, shadows=shadows, bvh=bvh, lookup=lookup)]


@functools.lru_cache(maxsize=None)
def scene_trace(v, t):
    """what the restatement of a (view, table) holds apart from the environment, computed once (shadowed, linear)"""
    name = TABLES[t]
    return mm.trace(*SCENE, measured(name).table.astype(np.float64), alpha_of(name), view_rot(v), FILM, FILM, S, Q)


def unshadowed(tr):
    """the same trace with every ray open: the plain render's (the sample sets and weights do not know about the shadow)"""
    out = dict(tr)
    for name in ("spec", "diff"):
        out["open_" + name] = np.ones_like(tr["open_" + name])
        out["marginal_" + name] = np.zeros_like(tr["marginal_" + name])
    return out


@functools.lru_cache(maxsize=None)
def scene_gpu(v, white, shadows=True):
    """the three tables of a view in one call"""
    views = None if VIEWS[v] is None else [VIEWS[v]] * 3
    return gpu_render(SCENE, TABLES, None if white else [ENV] * 3, views, shadows)[0]


def beyond_slack(gpu, ref):
    safe = ~ref["unsafe_pixel"]
    over = np.maximum(np.abs(gpu - ref["image"]) - ref["slack"], 0.0)[:, safe]
    return float(np.linalg.norm(over) / np.linalg.norm(ref["image"][:, safe])), safe


def restatement_caps(tr):
    """the comparison cannot empty itself: measured on the restatement alone"""
    marginal, unsafe, occl = tr["marginal"] / tr["traced"], tr["vis"]["unsafe"].mean(), tr["occluded"] / tr["traced"]
    assert marginal <= CAP and unsafe <= CAP and occl >= 0.01 and tr["traced"] >= 10000, (marginal, unsafe, occl, tr["traced"])
    return marginal, unsafe, occl


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("v,t", CASES)
def test_plain_and_shadowed_images_match_the_restatement(v, t):
    tr = scene_trace(v, t)
    marginal, unsafe, occl = restatement_caps(tr)
    for white in (False, True):
        env = None if white else ENV
        for shadows, trace in ((True, tr), (False, unshadowed(tr))):
            ref = mm.shade(trace, env)
            share = ref["slack"].sum() / ref["image"].sum()
            err, safe = beyond_slack(scene_gpu(v, white, shadows)[t], ref)
            lit_safe = int((ref["image"][:, safe].sum(axis=0) > 0).sum())
            print(f"view {v} {TABLES[t]} white {white} shadows {shadows}: marginal rays {marginal:.4f}, unsafe samples {unsafe:.4f}, occluded {occl:.4f}, "
                  f"traced {tr['traced']}, slack share {share:.4f}, lit safe pixels {lit_safe}, rel-L2 beyond the slack on safe pixels {err:.3g}")
            assert share <= CAP and safe.mean() >= 0.9 and lit_safe >= 50
            assert shadows or not ref["slack"].any()
            assert err <= 1e-5, (v, TABLES[t], white, shadows, err)


def test_the_nearest_lookup_matches_the_restatement():
    v, t = 1, 0
    tr = dict(scene_trace(v, t))
    restatement_caps(tr)
    table, n = measured(TABLES[t]).table.astype(np.float64), tr["normal"][tr["lit"]]
    tr["w_spec"] = mm.table_weights(table, alpha_of(TABLES[t]), n, tr["l_spec"], tr["traced_spec"], "nearest")
    tr["w_diff"] = mm.table_weights(table, alpha_of(TABLES[t]), n, tr["l_diff"], np.ones(tr["traced_spec"].shape, dtype=bool), "nearest")
    ref = mm.shade(tr, ENV)
    gpu = gpu_render(SCENE, [TABLES[t]], [ENV], [VIEWS[v]], True, lookup="nearest")[0][0]
    err, safe = beyond_slack(gpu, ref)
    share = ref["slack"].sum() / ref["image"].sum()
    linear = scene_gpu(v, False)[t]
    print(f"nearest, view {v} {TABLES[t]}: rel-L2 beyond the slack on safe pixels {err:.3g}; against the linear lookup {rel_l2(gpu, linear):.3g}")
    assert share <= CAP and safe.mean() >= 0.9 and not np.array_equal(gpu, linear)
    assert err <= 1e-5, err


# ---------------------------------------------------------------------------------------------- 2. the shadow
@pytest.mark.parametrize("v", range(len(VIEWS)))
def test_the_shadow_is_there_and_only_darkens(v):
    for white in (False, True):
        lit, dark = scene_gpu(v, white, False), scene_gpu(v, white)
        assert np.all(dark <= lit) and np.all(dark >= 0) and (dark < lit).sum() >= 100
        for t in range(3):
            rel = rel_l2(dark[t], lit[t])
            print(f"view {v} {TABLES[t]} white {white}: shadowed against plain rel-L2 {rel:.4f}")
            assert rel > 1e-2, (v, t, white)


def test_a_flat_shaded_convex_mesh_has_no_shadow_beyond_its_slack():
    from test_shadow_cpu import flat_icosphere

    mesh = flat_icosphere()
    for view in (None, (0.6, 0.3, 1.0)):
        views = None if view is None else [view] * 3
        lit, dark = (gpu_render(mesh, TABLES, [ENV] * 3, views, s)[0] for s in (False, True))
        for t, name in enumerate(TABLES):
            slack = mm.render(*mesh, measured(name).table.astype(np.float64), alpha_of(name), ENV, None if view is None else rotation(view), FILM, FILM, S,
                              Q)["slack"]
            diff = lit[t] - dark[t]
            assert np.all(diff >= 0) and np.all(diff <= slack * (1 + 1e-5) + 1e-7 * (slack > 0)) and np.all(diff[slack == 0] == 0), (view, name)
            assert (slack == 0).mean() > 0.5 and lit[t].max() > 0.1


# ---------------------------------------------------------------------------------------------- 3. one per-normal sum, and the table is read
def test_a_mesh_image_is_its_normal_map_shaded():
    from drmnet_amd.mesh import render_mesh_measured
    from drmnet_amd.relight import render_normals_measured

    bsdfs = [measured(n) for n in TABLES]
    env = torch.tensor(np.stack([ENV] * 3), dtype=torch.float32, device=DEV)
    for view in (None, torch.tensor([VIEWS[1]] * 3, dtype=torch.float32)):
        image, normal, _, alpha = render_mesh_measured(as_obj(*mr.icosphere(2)), bsdfs, env, image_size=16, view_from=view, quad=Q, subpixel=1)
        again, drawn = render_normals_measured(normal.permute(0, 2, 3, 1), bsdfs, env, mask=alpha > 0, view_from=view, quad=Q)
        err = rel_l2(again.cpu(), image.cpu())
        away = (alpha > 0) & (normal[:, 2] <= 0)
        print(f"view {view is not None}: mesh image under tables against its shaded normal map: rel-L2 {err:.3g}, bits equal: {torch.equal(again, image)}, "
              f"hits facing away {int(away.sum())}")
        assert torch.equal(drawn, alpha * (normal[:, 2] > 0)) and 100 <= int((alpha[0] > 0).sum()) <= 256
        assert not image.permute(0, 2, 3, 1)[away].any() and float(image.max()) > 0.1
        assert err <= 1e-5


@pytest.mark.parametrize("v", range(len(VIEWS)))
def test_the_table_is_really_read(v):
    from drmnet_amd.mesh import render_mesh

    views = None if VIEWS[v] is None else torch.tensor([VIEWS[v]] * 2, dtype=torch.float32)
    z = torch.tensor([DIELECTRIC, METALLIC], dtype=torch.float32, device=DEV)
    env = torch.tensor(np.stack([ENV] * 2), dtype=torch.float32, device=DEV)
    rows = render_mesh(as_obj(*SCENE), z, NAMES6, env, image_size=FILM, view_from=views, quad=Q, subpixel=S, shadows=True)[0].cpu().numpy().astype(np.float64)
    tabs = scene_gpu(v, False)[1:]
    for k, name in enumerate(("dielectric", "metallic")):
        rel = rel_l2(tabs[k], rows[k])
        print(f"view {v} {name}: the exported table against its row under drm_render_mesh, shadowed: rel-L2 {rel:.4f}")
        assert 1e-4 < rel <= 5e-2, (v, name, rel)


def test_rows_under_the_same_table_are_the_same_bits():
    out = gpu_render(SCENE, ["dielectric", "smooth", "dielectric"], [ENV] * 3, [VIEWS[1]] * 3, True)
    for a in out:
        assert np.array_equal(a[0], a[2])
    assert rel_l2(out[0][1], out[0][0]) > 1e-2


# ---------------------------------------------------------------------------------------------- 4. determinism
def test_renders_are_reproducible_rows_are_independent_and_a_given_bvh_is_the_built_one():
    from drmnet_amd.mesh import build_bvh

    views = [(0.0, 0.0, 1.1), VIEWS[1], VIEWS[2]]
    envs = [ENV, 1.5 * ENV, ENV[:, ::-1].copy()]
    for shadows in (True, False):
        stacked = gpu_render(SCENE, TABLES, envs, views, shadows)
        again = gpu_render(SCENE, TABLES, envs, views, shadows)
        for a, b in zip(stacked, again):
            assert np.array_equal(a, b)
        for r in range(3):
            one = gpu_render(SCENE, TABLES[r:r + 1], envs[r:r + 1], views[r:r + 1], shadows)
            for a, b in zip(stacked, one):
                assert np.array_equal(a[r], b[0]), (shadows, r)
        assert not np.array_equal(stacked[0][0], stacked[0][1])
    built, plain = gpu_render(SCENE, TABLES, envs, views, True), stacked
    given = gpu_render(SCENE, TABLES, envs, views, True, bvh=build_bvh(as_obj(*SCENE)))
    for a, b in zip(built, given):
        assert np.array_equal(a, b)
    assert not np.array_equal(built[0], plain[0])
    with pytest.raises(RuntimeError):
        gpu_render(SCENE, TABLES, envs, views, True, bvh=build_bvh(as_obj(*mr.icosphere(1))))


# ---------------------------------------------------------------------------------------------- 5. arguments
def raw_call(shadowed=True, material="tables", NT=2, table_of=(0, 1, 0), alpha=(0.45, 0.3), light_samples=0, bounces=0, blob="build", blob_bytes=None,
             ws="ok", ws_bytes=None, struct=None, quad=Q, tables="ok"):
    """drm_render_mesh_tables through ctypes on sentinel-filled outputs: (status, message, outputs)"""
    import abi_call
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    lib = _lib.lib()
    obj = {k: t.to(DEV) for k, t in as_obj(*SCENE).items()}
    B, V, F, H, W = 3, obj["vertex_positions"].shape[0], obj["faces"].shape[0], FILM, FILM
    need = lib.drm_render_mesh_workspace_bytes(F, B, H, W, S)
    wsbuf = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    t = torch.stack([measured("smooth").device_table(DEV), measured("dielectric").device_table(DEV)])
    of = None if table_of is None else torch.tensor(table_of, dtype=torch.int32, device=DEV)
    al = None if alpha is None else torch.tensor(alpha, dtype=torch.float32, device=DEV)
    z = torch.tensor([DIELECTRIC] * 3, dtype=torch.float32, device=DEV)
    env = torch.tensor(np.stack([ENV] * 3), dtype=torch.float32, device=DEV).contiguous()
    lws_bytes = int(lib.drm_render_light_workspace_bytes(B, env.shape[1], env.shape[2], 64))
    lws = torch.zeros(lws_bytes, dtype=torch.uint8, device=DEV)
    outs = [torch.full(s, -7.0, device=DEV) for s in ((B, 3, H, W), (B, 3, H, W), (B, 1, H, W), (B, H, W))]
    tp = {"ok": t.data_ptr(), None: None, "misaligned": t.data_ptr() + 4}[tables]
    mat = dict(tables=dict(tables=tp, NT=NT, table_of=_lib.ptr(of), alpha=_lib.ptr(al), linear=1), z=dict(z=z.data_ptr()),
               both=dict(z=z.data_ptr(), tables=tp, NT=NT, table_of=_lib.ptr(of), alpha=_lib.ptr(al), linear=1), none=dict())[material]
    sh = abi_call.shading(B, env=env.data_ptr(), EH=env.shape[1], EW=env.shape[2], quad=quad, light_samples=light_samples,
                          lws=lws.data_ptr() if light_samples else None, lws_bytes=lws_bytes if light_samples else 0, **mat)
    dev_blob, nbytes = None, 0
    if shadowed:
        if isinstance(blob, str):
            blob = build_bvh(as_obj(*SCENE))
        dev_blob = None if blob is None else blob.to(DEV)
        nbytes = (0 if blob is None else blob.numel()) if blob_bytes is None else blob_bytes
    ws_ptr = {"ok": wsbuf.data_ptr(), None: None, "misaligned": wsbuf.data_ptr() + 8}[ws]
    m = abi_call.mesh_render(obj["vertex_positions"].data_ptr(), obj["vertex_normals"].data_ptr(), obj["faces"].data_ptr(), V, F,
                             [o.data_ptr() for o in outs], H, W, S, ws_ptr, need if ws_bytes is None else ws_bytes, shadows=int(shadowed),
                             bvh=_lib.ptr(dev_blob), bvh_bytes=nbytes, bounces=bounces, bounce_quad=4 if bounces else 0)
    if struct == "shading":
        sh.struct_bytes += 4
    if struct == "mesh":
        m.struct_bytes += 4
    status = lib.drm_render_mesh_tables(sh, m, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return status, (lib.drm_last_error() or b"").decode(), [o.cpu().numpy() for o in outs]


def test_bad_arguments_launch_nothing():
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    for over in (dict(), dict(shadowed=False), dict(table_of=None), dict(NT=1, table_of=(0, 0, 0), alpha=(1.0,))):
        status, message, outs = raw_call(**over)
        assert status == 0 and all(not np.any(o == -7.0) for o in outs), (over, message)
    # the valid call is what the Python layer renders
    want = gpu_render(SCENE, ["smooth", "dielectric", "smooth"], [ENV] * 3, None, True)[0]
    assert measured("dielectric").alpha != 0.3  # (the raw call gives its own alphas: compare the row whose alpha is the table's)
    assert np.array_equal(raw_call()[2][0][0].astype(np.float64), want[0])
    good = build_bvh(as_obj(*SCENE))
    damaged = good.clone()
    damaged[0] ^= 0xFF  # the magic
    need = _lib.lib().drm_render_mesh_workspace_bytes(len(SCENE[2]), 3, FILM, FILM, S)
    cases = [(INVALID, dict(struct="shading"), "drm_shading"), (INVALID, dict(struct="mesh"), "drm_mesh_render"),
             (INVALID, dict(material="z"), "tables"), (INVALID, dict(material="both"), "material"), (INVALID, dict(material="none"), "material"),
             (INVALID, dict(light_samples=64), "light"), (INVALID, dict(bounces=1), "bounces"), (INVALID, dict(bounces=1, shadowed=False), "bounces"),
             (INVALID, dict(quad=0), "quad"),
             (INVALID, dict(tables=None), "material"), (INVALID, dict(tables="misaligned"), "tables"), (INVALID, dict(NT=0), "NT"),
             (INVALID, dict(table_of=(0, 2, 0)), "table_of"), (INVALID, dict(table_of=(0, -1, 0)), "table_of"),
             (INVALID, dict(alpha=(0.3, 0.001)), "alpha"), (INVALID, dict(alpha=(2.0, 0.5)), "alpha"), (INVALID, dict(alpha=(0.3, float("nan"))), "alpha"),
             (INVALID, dict(alpha=(float("inf"), 0.5)), "alpha"), (INVALID, dict(alpha=None), "alpha"),
             (INVALID, dict(blob=None), "bvh"), (INVALID, dict(blob=build_bvh(as_obj(*mr.icosphere(1)))), "bvh"), (INVALID, dict(blob=damaged), "bvh"),
             (INVALID, dict(blob=good[:len(good) - 4].clone()), "bvh"), (INVALID, dict(blob=good, blob_bytes=len(good) - 1), "bvh"),
             (INVALID, dict(blob=good[:16].clone()), "bvh"),
             (WORKSPACE, dict(ws=None), "workspace"), (WORKSPACE, dict(ws="misaligned"), "workspace"), (WORKSPACE, dict(ws_bytes=need - 1), "workspace")]
    for want_status, over, word in cases:
        status, message, outs = raw_call(**over)
        assert status == want_status and word in message, (over, status, message)
        assert all(np.all(o == -7.0) for o in outs), over


# ---------------------------------------------------------------------------------------------- 6. surface
def test_synthesize_with_a_measured_brdf(tmp_path):
    from drmnet_amd import file_io, merl, synthesize
    from drmnet_amd.render import render_table

    torch.save(dict(as_obj(*SCENE)), tmp_path / "scene.pt")
    file_io.save_exr(tmp_path / "env.exr", ENV.astype(np.float32))
    merl.save_merl(measured("dielectric").table, tmp_path / "material.binary")
    images = {}
    for flag in ([], ["--shadows"]):
        out = tmp_path / ("out" + "".join(flag))
        synthesize.main(["--mesh", str(tmp_path / "scene.pt"), "--envmap", str(tmp_path / "env.exr"), "--merl", str(tmp_path / "material.binary"),
                         "--view_from", "0.6", "0.3", "1.0", "--image_size", "24", "--refmap_res", "8", "--quad", str(Q), "--output_dir", str(out), *flag])
        assert all((out / n).exists() for n in ("image.exr", "normal.npy", "mask.png", "refmap.exr"))
        images[bool(flag)] = file_io.load_exr(out / "image.exr")
    assert images[True].shape == (24, 24, 3) and np.all(images[True] <= images[False]) and rel_l2(images[True], images[False]) > 1e-2
    assert images[False].max() > 0.1 and np.load(tmp_path / "out" / "normal.npy").shape == (24, 24, 3)
    env = torch.tensor(ENV.astype(np.float32), device=DEV)[None]
    want = render_table(merl.MeasuredBSDF.from_file(tmp_path / "material.binary"), env, res=8, quad=Q, view_from=torch.tensor([[0.6, 0.3, 1.0]]))
    assert np.array_equal(file_io.load_exr(tmp_path / "out" / "refmap.exr"), want[0].permute(1, 2, 0).cpu().numpy())

"""The four sphere / environment-map warps of drmnet_amd.transform restated in float64 numpy, as a test-side reference at sizes that have no
golden: envmap2mirmap (with its adaptive average pool), rotate_envmap, mirimg2envmap and refmap2refimg (utils/transform.py:170-363 of the
reference, whose fp32 outputs are in tests/golden/warps.npz; test_warps_cpu.py holds this file against them).

Everything is written per item and looped over the batch; a frame argument is [3] (shared) or [B, 3].  Vectors are used as given.  Each
``*_positions`` function returns the normalised sample positions (u, v) and the source azimuth before it is wrapped, so that a caller can
measure how close a sample comes to the azimuth seam, where border-clamped bilinear sampling is discontinuous.
"""
import numpy as np

PI = np.pi


def _vec(v, B):
    v = np.asarray(v, dtype=np.float64)
    assert v.shape in ((3,), (B, 3)), v.shape
    return np.broadcast_to(v.reshape(-1, 3), (B, 3))


def normalize(x, eps=1e-12):
    return x / np.clip(np.linalg.norm(x, axis=-1, keepdims=True), eps, None)


def reorthogonalise(view_from, top):
    """top <- normalize((view x top) x view) where view . top != 0"""
    if np.dot(view_from, top) != 0:
        return normalize(np.cross(np.cross(view_from, top), view_from))
    return top


def frame(normal, tangent, reverse_phi):
    b = np.cross(normal, tangent)
    return normal, tangent, (-b if reverse_phi else b)


def sphere_dir(theta, phi, fr):
    n, t, b = fr
    st = np.sin(theta)[..., None]
    return np.cos(theta)[..., None] * n + st * np.cos(phi)[..., None] * t + st * np.sin(phi)[..., None] * b


def dir_angles(d, fr):
    """(theta, phi) of directions d about a frame; the cosine is clipped to [-1, 1] (the reference leaves an overshoot to become NaN)"""
    n, t, b = fr
    return np.arccos(np.clip(d @ n, -1.0, 1.0)), np.arctan2(d @ b, d @ t)


def grid_sample(img, u, v):
    """torch.nn.functional.grid_sample(bilinear, padding_mode="border", align_corners=False): img [C, H, W], u / v [...] -> [C, ...]"""
    C, H, W = img.shape
    ix = np.clip(((u + 1) * W - 1) / 2, 0, W - 1)
    iy = np.clip(((v + 1) * H - 1) / 2, 0, H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx, wy = ix - x0, iy - y0
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)  # (their weights are 0 where they were clamped)
    return (img[:, y0, x0] * (1 - wx) * (1 - wy) + img[:, y0, x1] * wx * (1 - wy) + img[:, y1, x0] * (1 - wx) * wy + img[:, y1, x1] * wx * wy)


def adaptive_avg_pool(x, out_shape):
    """torch.nn.functional.adaptive_avg_pool2d: x [C, SH, SW] -> [C, OH, OW], windows [floor(i S / O), ceil((i + 1) S / O))"""
    C, SH, SW = x.shape
    OH, OW = out_shape
    out = np.empty((C, OH, OW), dtype=np.float64)
    for i in range(OH):
        y0, y1 = (i * SH) // OH, -((-(i + 1) * SH) // OH)
        for j in range(OW):
            x0, x1 = (j * SW) // OW, -((-(j + 1) * SW) // OW)
            out[:, i, j] = x[:, y0:y1, x0:x1].mean(axis=(1, 2))
    return out


def sample_grid_side(H, W, OH, OW):
    """the S of envmap2mirmap's S x S sample grid under mitigate_aliasing"""
    return min(H, W) if OH < H else max(OH, OW)


def envmap2mirmap_positions(H, W, output_shape, flip_horizontal=False, view_from=(1, 0, 0), top=(0, 1, 0), envmap_zenith=(0, 1, 0),
                            envmap_left_edge=(0, 0, -1), reverse_azimuth_envmap=True, mitigate_aliasing=True):
    """one item -> (u, v, azimuth), each [SH, SW]"""
    view_from, top = np.asarray(view_from, np.float64), np.asarray(top, np.float64)
    top = reorthogonalise(view_from, top)
    OH, OW = output_shape
    SH, SW = (sample_grid_side(H, W, OH, OW),) * 2 if mitigate_aliasing else (OH, OW)
    theta = (np.arange(SH) + 0.5) * (PI / SH)
    phi = (np.arange(SW) - (SW - 1) / 2) * (PI / SW)
    theta, phi = np.meshgrid(theta, phi, indexing="ij")
    n = sphere_dir(theta, phi, frame(top, view_from, flip_horizontal))
    r = normalize(2 * (n @ view_from)[..., None] * n - view_from)
    t, p = dir_angles(r, frame(np.asarray(envmap_zenith, np.float64), np.asarray(envmap_left_edge, np.float64), reverse_azimuth_envmap))
    return np.mod(p, 2 * PI) / PI - 1, t * (2 / PI) - 1, p


def envmap2mirmap(envmap, output_shape, flip_horizontal=False, view_from=(1, 0, 0), top=(0, 1, 0), envmap_zenith=(0, 1, 0),
                  envmap_left_edge=(0, 0, -1), reverse_azimuth_envmap=True, mitigate_aliasing=True, log_scale_interpolation=False):
    envmap = np.asarray(envmap, dtype=np.float64)
    B, C, H, W = envmap.shape
    vecs = [_vec(a, B) for a in (view_from, top, envmap_zenith, envmap_left_edge)]
    out = []
    for b in range(B):
        u, v, _ = envmap2mirmap_positions(H, W, output_shape, flip_horizontal, vecs[0][b], vecs[1][b], vecs[2][b], vecs[3][b], reverse_azimuth_envmap,
                                          mitigate_aliasing)
        img = np.log(np.clip(envmap[b], 1e-7, None)) if log_scale_interpolation else envmap[b]
        pooled = adaptive_avg_pool(grid_sample(img, u, v), output_shape)
        out.append(np.exp(pooled) if log_scale_interpolation else pooled)
    return np.stack(out)


def rotate_envmap_positions(out_shape, src_envmap_zenith, src_envmap_left_edge, tgt_envmap_zenith, tgt_envmap_left_edge):
    """one item -> (u, v, azimuth), each [OH, OW]"""
    OH, OW = out_shape
    hs, ws = PI / OH / 2, PI / OW
    theta, phi = np.meshgrid(np.linspace(hs, PI - hs, OH), np.linspace(ws, 2 * PI - ws, OW), indexing="ij")
    d = sphere_dir(theta, phi, frame(np.asarray(tgt_envmap_zenith, np.float64), np.asarray(tgt_envmap_left_edge, np.float64), True))
    t, p = dir_angles(d, frame(np.asarray(src_envmap_zenith, np.float64), np.asarray(src_envmap_left_edge, np.float64), True))
    return np.mod(p / PI, 2) - 1, t / (PI / 2) - 1, p


def rotate_envmap(envmap, src_envmap_zenith=(0, 1, 0), src_envmap_left_edge=(0, 0, -1), tgt_envmap_zenith=None, tgt_envmap_left_edge=None,
                  out_shape=None):
    envmap = np.asarray(envmap, dtype=np.float64)
    B, C, H, W = envmap.shape
    out_shape = (H, W) if out_shape is None else out_shape
    vecs = [_vec(a, B) for a in (src_envmap_zenith, src_envmap_left_edge, tgt_envmap_zenith, tgt_envmap_left_edge)]
    out = []
    for b in range(B):
        u, v, _ = rotate_envmap_positions(out_shape, *[a[b] for a in vecs])
        out.append(grid_sample(envmap[b], u, v))
    return np.stack(out)


def mirimg2envmap(refimg, output_shape, view_from=(0, 0, 1), top=(0, 1, 0), envmap_zenith=(0, 1, 0), envmap_left_edge=(0, 0, -1),
                  reverse_azimuth=True, log_scale_interpolation=False):
    refimg = np.asarray(refimg, dtype=np.float64)
    B = refimg.shape[0]
    OH, OW = output_shape
    vecs = [_vec(a, B) for a in (view_from, top, envmap_zenith, envmap_left_edge)]
    theta, phi = np.meshgrid((np.arange(OH) + 0.5) * (PI / OH), (np.arange(OW) + 0.5) * (2 * PI / OW), indexing="ij")
    out = []
    for b in range(B):
        view, tp = vecs[0][b], reorthogonalise(vecs[0][b], vecs[1][b])
        d = sphere_dir(theta, phi, frame(vecs[2][b], vecs[3][b], reverse_azimuth))
        t, p = dir_angles(normalize(d + view), frame(tp, np.cross(view, tp), False))
        t, p = t - PI / 2, p - PI / 2
        img = np.log(np.clip(refimg[b], 1e-7, None)) if log_scale_interpolation else refimg[b]
        s = grid_sample(img, np.cos(t) * np.sin(p), np.sin(t))
        out.append(np.exp(s) if log_scale_interpolation else s)
    return np.stack(out)


def sphere_disc(radius):
    """gen_sphere_normals_realcentering: (unit normals [2r, 2r, 3], zero outside; the disc [2r, 2r] bool)"""
    x = -radius + 0.5 + np.arange(2 * radius, dtype=np.float64)
    x, y = np.meshgrid(x, -x)
    zsq = radius**2 - (x**2 + y**2)
    mask = zsq >= 0
    n = np.stack([x, y, np.sqrt(np.where(mask, zsq, 0.0))], axis=-1) / radius
    return n * mask[..., None], mask


def refmap2refimg(refmap, radius=None):
    """refmap [B, C, H, W] -> (image [B, C, 2r, 2r], zero outside the disc; the disc)"""
    refmap = np.asarray(refmap, dtype=np.float64)
    B, C, H, W = refmap.shape
    radius = max(H, W) if radius is None else radius
    n, mask = sphere_disc(radius)
    t, p = dir_angles(n, frame(np.array([0.0, 1.0, 0.0]), np.array([-1.0, 0.0, 0.0]), False))
    out = np.stack([grid_sample(refmap[b], p * (2 / PI) - 1, t * (2 / PI) - 1) for b in range(B)])
    return out * mask, mask


def seam_margin(azimuth):
    """the smallest distance (radians) of any sample's source azimuth from the wrap of `% 2 pi`, which sits at azimuth 0"""
    a = np.abs(np.mod(np.asarray(azimuth) + PI, 2 * PI) - PI)
    return float(a.min())


def golden_cases(g):
    """the cases of tests/golden/warps.npz (tools/make_golden_warps.py), g = the loaded file -> a list of
    (case, input array, kwargs, the reference's output, its mask or None); tuples stand for the JSON lists of the shapes"""
    import json

    out = []
    for case in json.loads(str(g["cases"])):
        kw = {k: (tuple(v) if k in ("output_shape", "out_shape") else v) for k, v in case["kwargs"].items()}
        x = g[case["input"]][case["items"][0]:case["items"][1]]
        out.append((case, x[0] if case["squeeze"] else x, kw, g[case["out"]], g.get(case["out"] + "_mask")))
    return out

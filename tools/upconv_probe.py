#!/usr/bin/env python3
"""Times the first ResBlock of every finer IllNet decoder level -- in_layers over cat(nearest_x2(x0), x1) -- through the op-level ABI with the
single launch (ops.set_upconv_split(0)) and the two-launch form (2), interleaved in one process on one device (batch-32 step shapes).

    [DRM_PROF_DUMP=1] python tools/upconv_probe.py [precision] [rounds]

Per shape and round: the 3x3 family's time per block call in either mode (in_layers + out_layers; out_layers is the same launch in both, so
the difference is single - (A + B)) and launch A's own time (the only conv_split2_kernel<4, ...> launch).  With DRM_PROF_DUMP the library
prints the per-shape table of every collect to stderr: mode 0 gives the single launch (C0+C1 -> Cout) and out_layers (Cout -> Cout) apart.
"""
import ctypes as C, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drmnet_amd import _lib, ops, synth
prec = sys.argv[1] if len(sys.argv) > 1 else "f16mx"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
REPS = 4
ops.set_precision(prec)
L = _lib.lib(); dev = torch.device("cuda:0")
def man(cin, cout):
    return [("in_layers.0.weight", (cin,)), ("in_layers.0.bias", (cin,)), ("in_layers.2.weight", (cout, cin, 3, 3)), ("in_layers.2.bias", (cout,)),
            ("emb_layers.1.weight", (cout, 512)), ("emb_layers.1.bias", (cout,)), ("out_layers.0.weight", (cout,)), ("out_layers.0.bias", (cout,)),
            ("out_layers.3.weight", (cout, cout, 3, 3)), ("out_layers.3.bias", (cout,)), ("skip_connection.weight", (cout, cin, 1, 1)), ("skip_connection.bias", (cout,))]
# (n, C0, C1, Cout, H, W) of the full-resolution map
SHAPES = [(32, 256, 128, 128, 128, 256), (32, 384, 256, 256, 64, 128), (32, 512, 384, 384, 32, 64), (32, 640, 512, 512, 16, 32), (32, 768, 640, 640, 8, 16)]
if os.environ.get("UPCONV_SHAPES"):
    SHAPES = [tuple(int(v) for v in t.split(",")) for t in os.environ["UPCONV_SHAPES"].split(";")]
def variants():
    need = L.drm_profile_variants(None, 0)
    buf = C.create_string_buffer(int(need) + 16)
    L.drm_profile_variants(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        out[f[0]] = (int(f[2]), float(f[3]))
    return out
for (n, c0, c1, cout, h, w) in SHAPES:
    P = [p.to(dev) for p in synth.synth_state_dict(man(c0 + c1, cout), 1).values()]
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn((n, c0, h // 2, w // 2), generator=g).to(dev); x1 = torch.randn((n, c1, h, w), generator=g).to(dev)
    emb = torch.randn((n, 512), generator=g).to(dev)
    for mode in (0, 2):
        ops.set_upconv_split(mode); ops.resblock(P, x0, emb, x1, up0=True)
    torch.cuda.synchronize()
    for rnd in range(rounds):
        res = {}
        for mode in (0, 2):
            ops.set_upconv_split(mode)
            L.drm_profile_reset(); L.drm_profile_enable(1)
            for _ in range(REPS): ops.resblock(P, x0, emb, x1, up0=True)
            torch.cuda.synchronize(); L.drm_profile_enable(0)
            K = 5; ms, fl, by, cnt = (C.c_double*K)(), (C.c_double*K)(), (C.c_double*K)(), (C.c_int64*K)()
            print(f"-- {prec} N{n} {c0}+{c1}->{cout} @{h}x{w} round {rnd + 1} mode {mode}", file=sys.stderr, flush=True)
            L.drm_profile_collect(ms, fl, by, cnt)
            v4 = [(k, t) for k, t in variants().items() if k.startswith("void drm::conv_split2_kernel<4, ")]
            res[mode] = (ms[0] / REPS, cnt[0] // REPS, sum(t[1] for _, t in v4) / REPS, [k for k, _ in v4])
        d = res[0][0] - res[2][0]
        print(f"{prec} N{n} {c0}+{c1}->{cout} @{h}x{w} round {rnd + 1}: 3x3 family per block  mode 0 {res[0][0]:.4f} ms ({res[0][1]} launches)  "
              f"mode 2 {res[2][0]:.4f} ms ({res[2][1]} launches; A {res[2][2]:.4f} ms)  single - (A + B) = {d:+.4f} ms"
              + ("" if res[2][3] else "   [mode 2 ran the single launch: the form does not apply]"), flush=True)
    ops.set_upconv_split(1)
    del x0, x1, P; torch.cuda.empty_cache()

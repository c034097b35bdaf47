"""The argument structs of include/drmnet_hip.h without a GPU: every struct a caller fills starts with struct_bytes, which the library checks
before it reads anything else, and the combinations that one drm_shading / drm_mesh_render pair can spell but no render supports are
DRM_ERR_INVALID.  Host buffers stand in for device memory (as in tests/test_mesh_light_cpu.py, with its shapes: icosphere(0), B = 1, a 4 x 4
film, an 8 x 16 map, M = 64): every case returns from the checks, which dereference nothing, and leaves the outputs alone."""
import ctypes as C

import numpy as np
import pytest

import abi_call
import mesh_ref as mr
from drmnet_amd import _lib
from oracle import unet as ou
from test_shadow_cpu import ROUGH

INVALID, WORKSPACE = 1, 3
B, H, W, EH, EW, M, R = 1, 4, 4, 8, 16, 64, 4


class Scene:
    """valid arguments of the three renders on host memory; .shading(**over) / .mesh(**over) / the three calls"""

    def __init__(self):
        lib = _lib.lib()
        p, n, f = mr.icosphere(0)
        self.pos, self.nrm, self.faces = (np.ascontiguousarray(a, dtype=t) for a, t in ((p, np.float32), (n, np.float32), (f, np.int32)))
        self.z = np.array([ROUGH], dtype=np.float32)
        self.env = np.ones((B, EH, EW, 3), dtype=np.float32)
        self.tables = np.zeros(8, dtype=np.float64)  # (never read: every case that names it returns before check_tables)
        self.normals = np.zeros((1, H, W, 3), dtype=np.float32)
        self.need, self.light_need = int(lib.drm_render_mesh_workspace_bytes(len(self.faces), B, H, W, 2)), int(lib.drm_render_light_workspace_bytes(B, EH, EW, M))
        assert self.need > 0 and self.light_need > 0
        self.ws, self.lws, self.bvh = np.zeros(self.need // 8 + 2, dtype=np.float64), np.zeros(self.light_need // 8 + 2, dtype=np.float64), np.zeros(64, dtype=np.uint8)
        self.ws_ptr = (self.ws.ctypes.data + 15) & ~15
        self.mesh_outs = [np.full(s, -7.0, dtype=np.float32) for s in ((B, 3, H, W), (B, 3, H, W), (B, 1, H, W), (B, H, W))]
        self.sphere_out = np.full((2, B, 3, R, R), -7.0, dtype=np.float32)
        self.normals_outs = [np.full((B, 3, H, W), -7.0, dtype=np.float32), np.full((B, H, W), -7.0, dtype=np.float32)]

    def shading(self, lit=False, measured=False, **over):
        a = dict(z=self.z.ctypes.data, env=self.env.ctypes.data, EH=EH, EW=EW, quad=8)
        if lit:
            a.update(light_samples=M, lws=self.lws.ctypes.data, lws_bytes=self.light_need)
        if measured:
            a.update(z=None, tables=(self.tables.ctypes.data + 15) & ~15, NT=1, alpha=self.lws.ctypes.data)
        a.update(over)
        return abi_call.shading(B, **a)

    def mesh(self, **over):
        return abi_call.mesh_render(self.pos.ctypes.data, self.nrm.ctypes.data, self.faces.ctypes.data, len(self.pos), len(self.faces),
                                    [o.ctypes.data for o in self.mesh_outs], H, W, 2, self.ws_ptr, self.need, **over)

    def render_mesh(self, sh, m):
        return abi_call.render_mesh(sh, m), self.mesh_outs

    def render_refmap(self, sh, L=1):
        return abi_call.render_refmap(sh, L, R, 2, 0, self.sphere_out.ctypes.data), [self.sphere_out]

    def render_normals(self, sh):
        return abi_call.render_normals(sh, self.normals.ctypes.data, None, 1, H, W, *[o.ctypes.data for o in self.normals_outs]), self.normals_outs


@pytest.fixture(scope="module")
def scene():
    return Scene()


def refused(result, word=None):
    """the call returned DRM_ERR_INVALID with a message (holding `word`) and wrote nothing"""
    status, outs = result
    message = (_lib.lib().drm_last_error() or b"").decode()
    assert status == INVALID and message and (word is None or word in message), (status, message)
    assert all(np.all(o == -7.0) for o in outs)
    return message


def wrong_size(s):
    s.struct_bytes += 4
    return s


def test_render_structs_are_checked_by_size_first(scene):
    good = scene.mesh(shadows=1, bvh=scene.bvh.ctypes.data, bvh_bytes=16)  # would fail on its blob: the size check comes first
    for call in (lambda sh: scene.render_refmap(sh), lambda sh: scene.render_normals(sh), lambda sh: scene.render_mesh(sh, good)):
        message = refused(call(wrong_size(scene.shading())), "drm_shading")
        assert str(C.sizeof(_lib.Shading)) in message and str(C.sizeof(_lib.Shading) + 4) in message
        # the right size passes that check: a zeroed struct then fails on something else
        assert "struct_bytes" not in refused(call(_lib.sized(_lib.Shading)))
    message = refused(scene.render_mesh(scene.shading(), wrong_size(scene.mesh())), "drm_mesh_render")
    assert str(C.sizeof(_lib.MeshRender)) in message and str(C.sizeof(_lib.MeshRender) + 4) in message
    assert "struct_bytes" not in refused(scene.render_mesh(scene.shading(), _lib.sized(_lib.MeshRender)))
    # a struct from a smaller mirror (an older binding) is refused the same way
    small_shading, small_mesh = scene.shading(), scene.mesh()
    small_shading.struct_bytes -= 4
    small_mesh.struct_bytes -= 4
    refused(scene.render_refmap(small_shading), "drm_shading")
    refused(scene.render_mesh(scene.shading(), small_mesh), "drm_mesh_render")


def test_chain_structs_are_checked_by_size_first():
    from drmnet_amd.unet import UNetModel

    L = _lib.lib()
    net = UNetModel(**ou.TINY_UNET_CFG)
    n, hh, ww = 1, 16, 16
    x, cond = np.full((n, 3, hh, ww), -7.0, dtype=np.float32), np.zeros((n, 3, hh, ww), dtype=np.float32)
    ts, coef = np.zeros(4, dtype=np.int64), np.zeros((4, 5), dtype=np.float32)

    def ddim(opt=None, log=None, x_ptr=x.ctypes.data):
        return L.drm_ddim_sample(net._h, x_ptr, cond.ctypes.data, ts.ctypes.data_as(C.POINTER(C.c_int64)), coef.ctypes.data_as(C.POINTER(C.c_float)), 4, 0,
                                 None, 0, opt, log, n, hh, ww, None, 0, None)

    def ddpm(opt=None):
        return L.drm_ddpm_sample(net._h, x.ctypes.data, x.ctypes.data, cond.ctypes.data, coef.ctypes.data_as(C.POINTER(C.c_float)), 4, 0, None, 0, opt, n, hh,
                                 ww, None, 0, None)

    def message():
        return (L.drm_last_error() or b"").decode()

    for struct_type, name, calls in ((_lib.ChainLog, "drm_chain_log", [lambda s: ddim(log=C.byref(s))]),
                                     (_lib.SamplerOptions, "drm_sampler_options", [lambda s: ddim(opt=C.byref(s)), lambda s: ddpm(opt=C.byref(s))]),
                                     (_lib.MaskBlend, "drm_mask_blend", [lambda s: ddim(opt=C.byref(_lib.sized(_lib.SamplerOptions, blend=C.pointer(s)))),
                                                                         lambda s: ddpm(opt=C.byref(_lib.sized(_lib.SamplerOptions, blend=C.pointer(s))))])):
        for call in calls:
            assert call(wrong_size(_lib.sized(struct_type))) == INVALID
            assert name in message() and str(C.sizeof(struct_type)) in message() and str(C.sizeof(struct_type) + 4) in message()
            # the right size passes that check: a zeroed struct is no options / no log, and the call then fails on its missing workspace
            assert call(_lib.sized(struct_type)) == WORKSPACE and "struct_bytes" not in message()
    # ... or, for the log, on the missing x
    assert ddim(log=C.byref(_lib.sized(_lib.ChainLog)), x_ptr=None) == INVALID and "struct_bytes" not in message()
    # every_t > 0 without both buffers and a slot count stays an error; NULL options and a NULL log are none at all
    assert ddim(log=C.byref(_lib.sized(_lib.ChainLog, every_t=10, x=x.ctypes.data, slots=4))) == INVALID and "intermediates" in message()
    assert ddim() == WORKSPACE and ddpm() == WORKSPACE
    assert np.all(x == -7.0)


def test_combinations_the_old_entries_could_not_express_are_refused(scene):
    blob = dict(shadows=1, bvh=scene.bvh.ctypes.data, bvh_bytes=16)
    # bounces
    refused(scene.render_mesh(scene.shading(), scene.mesh(bounces=1, bounce_quad=4)), "bounces")                      # without shadows
    refused(scene.render_mesh(scene.shading(lit=True), scene.mesh(bounces=1, bounce_quad=4, **blob)), "bounces")      # with light samples under a map
    refused(scene.render_mesh(scene.shading(), scene.mesh(bounces=2, bounce_quad=4, **blob)), "bounces")
    # the material: both, none
    both, none = dict(tables=(scene.tables.ctypes.data + 15) & ~15, NT=1, alpha=scene.lws.ctypes.data), dict(z=None)
    for over in (both, none):
        refused(scene.render_refmap(scene.shading(**over)), "material")
        refused(scene.render_normals(scene.shading(**over)), "material")
        refused(scene.render_mesh(scene.shading(**over), scene.mesh()), "material")
    # tables: no stacks, no light samples under a map, no mesh
    refused(scene.render_refmap(scene.shading(measured=True), L=2), "tables")
    refused(scene.render_refmap(scene.shading(measured=True, lit=True)), "tables")
    refused(scene.render_normals(scene.shading(measured=True, lit=True)), "tables")
    refused(scene.render_mesh(scene.shading(measured=True), scene.mesh()), "tables")

"""Fields of drm_shading / drm_mesh_render that a render does not use are really unused: with shadows = 0, bounces = 0 and
light_samples = 0 the render is the plain one bit for bit while bvh and light_workspace point at valid, correctly sized device buffers
filled with 0xEE, and both buffers are all 0xEE afterwards.  shadow_ref.two_spheres(), an 8 x 8 film, S = 2, Q = 5, B = 2."""
import numpy as np
import pytest
import torch

import abi_call
import shadow_ref as sr
from test_gpu_mesh import ENV, METAL, ROUGH, as_obj

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILM, S, Q, B, M, R = 8, 2, 5, 2, 64, 8


def poisoned(nbytes):
    return torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=DEV)


def test_unused_fields_are_neither_read_nor_written():
    from drmnet_amd import _lib
    from drmnet_amd.mesh import build_bvh

    lib = _lib.lib()
    scene = sr.two_spheres()
    obj = {k: t.to(DEV) for k, t in as_obj(*scene).items()}
    V, F = obj["vertex_positions"].shape[0], obj["faces"].shape[0]
    z = torch.tensor([ROUGH, METAL], dtype=torch.float32, device=DEV)
    env = torch.tensor(np.stack([ENV, 1.5 * ENV]), dtype=torch.float32, device=DEV).contiguous()
    EH, EW = env.shape[1], env.shape[2]
    # the buffers a shadowed, light-sampled render of this very call would need, poisoned
    blob = poisoned(int(build_bvh(as_obj(*scene)).numel()))
    light_bytes = int(lib.drm_render_light_workspace_bytes(B, EH, EW, M))
    lws = poisoned(light_bytes)
    assert light_bytes > 0 and lws.data_ptr() % 8 == 0 and blob.data_ptr() % 16 == 0
    need = int(lib.drm_render_mesh_workspace_bytes(F, B, FILM, FILM, S))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def mesh(poison):
        outs = [torch.full(s, -7.0, device=DEV) for s in ((B, 3, FILM, FILM), (B, 3, FILM, FILM), (B, 1, FILM, FILM), (B, FILM, FILM))]
        extra = dict(lws=lws.data_ptr(), lws_bytes=light_bytes) if poison else {}
        sh = abi_call.shading(B, z=z.data_ptr(), env=env.data_ptr(), EH=EH, EW=EW, quad=Q, light_samples=0, **extra)
        m = abi_call.mesh_render(obj["vertex_positions"].data_ptr(), obj["vertex_normals"].data_ptr(), obj["faces"].data_ptr(), V, F,
                                 [o.data_ptr() for o in outs], FILM, FILM, S, ws.data_ptr(), need, shadows=0, bounces=0,
                                 **(dict(bvh=blob.data_ptr(), bvh_bytes=blob.numel(), bounce_quad=4) if poison else {}))
        _lib.check(abi_call.render_mesh(sh, m, _lib.stream_ptr(DEV)))
        torch.cuda.synchronize()
        return outs

    def sphere(poison):
        out = torch.full((B, 3, R, R), -7.0, device=DEV)
        extra = dict(lws=lws.data_ptr(), lws_bytes=light_bytes) if poison else {}
        sh = abi_call.shading(B, z=z.data_ptr(), env=env.data_ptr(), EH=EH, EW=EW, quad=Q, light_samples=0, **extra)
        _lib.check(abi_call.render_refmap(sh, 1, R, S, 0, out.data_ptr(), _lib.stream_ptr(DEV)))
        torch.cuda.synchronize()
        return [out]

    for render in (mesh, sphere):
        plain, same = render(False), render(True)
        for a, b in zip(plain, same):
            assert torch.equal(a, b) and not bool((a == -7.0).any())
        assert bool((blob == 0xEE).all()) and bool((lws == 0xEE).all())
    assert float(plain[0].abs().max()) > 0

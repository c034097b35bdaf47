"""Raw calls of the three render entries of include/drmnet_hip.h for the argument tests: every pointer is a plain address (an int, a
ctypes.c_void_p or None), host or device, and every struct member can be set to anything, so a test reaches states the Python layer refuses."""
from drmnet_amd import _lib


def shading(B, z=None, env=None, EH=0, EW=0, view=None, quad=8, light_samples=0, lws=None, lws_bytes=0, tables=None, NT=0, table_of=None, alpha=None,
            linear=0):
    """a drm_shading from addresses"""
    return _lib.sized(_lib.Shading, B=B, z=z, tables=tables, NT=NT, table_of=table_of, table_alpha=alpha, table_linear=linear, envmap=env, EH=EH, EW=EW,
                      view=view, quad=quad, light_samples=light_samples, light_workspace=lws, light_workspace_bytes=lws_bytes)


def render_refmap(sh, L, R, subpixel, flip, out, stream=None):
    return _lib.lib().drm_render_refmap(sh, L, R, subpixel, flip, out, stream)


def render_normals(sh, normals, mask, Bn, H, W, image, alpha, stream=None):
    return _lib.lib().drm_render_normals(sh, normals, mask, Bn, H, W, image, alpha, stream)


def mesh_render(pos, nrm, faces, V, F, outs, H, W, subpixel, ws, ws_bytes, shadows=0, bvh=None, bvh_bytes=0, bounces=0, bounce_quad=0):
    """a drm_mesh_render from addresses; outs = (image, normal, depth, alpha)"""
    image, normal, depth, alpha = outs
    return _lib.sized(_lib.MeshRender, vertex_positions=pos, vertex_normals=nrm, faces=faces, V=V, F=F, H=H, W=W, subpixel=subpixel, image=image,
                      normal=normal, depth=depth, alpha=alpha, workspace=ws, workspace_bytes=ws_bytes, shadows=shadows, bvh=bvh, bvh_bytes=bvh_bytes,
                      bounces=bounces, bounce_quad=bounce_quad)


def render_mesh(sh, m, stream=None):
    return _lib.lib().drm_render_mesh(sh, m, stream)

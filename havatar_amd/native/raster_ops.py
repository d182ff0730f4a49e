"""The rasteriser kernels (csrc/hav_raster.hip): the three orthographic condition renders of B tracked meshes, contiguous float32 HIP tensors.
  raster(verts, colors, tris, res, rots, bounds, cam_dist, outputs=OUTPUTS)   -> {name: tensor}; outputs and workspaces allocated here
  raster_into(out, keys, screen, verts, colors, tris, res, rots, bounds, cam_dist)
                                              the three launches on the caller's buffers: out = {name: tensor}, a missing name is not written;
                                              keys [B,3,res,res] int64 and screen [B,3,V,4] float32 are workspaces (workspaces(B, V, res, device))
  params()                                    (tile height, tile width, large-box threshold in pixels), read from the library
The depth test is a 64-bit integer atomic min: the same inputs give the same bits on every call, whatever the triangles' order of arrival.
No allocation inside the entry and no host read: the call can be captured into a hipGraph.  No fallback in here --
havatar_amd.conditions.render_conditions decides which tensors come this way and states the same definition on ATen for the others."""
import ctypes as C

import torch

from .. import _lib
from ..utils.util import get_box_warp_param
from .conv import _p, _stream

# name -> (shape after [B,3] given (H, W), dtype), in the order of hav_raster_ortho_f32's output pointers
OUTPUTS = {"face": (lambda H, W: (H, W), torch.int32), "z": (lambda H, W: (H, W), torch.float32),
           "normal": (lambda H, W: (H, W, 3), torch.float32), "render8": (lambda H, W: (H, W, 3), torch.uint8),
           "normal8": (lambda H, W: (H, W, 3), torch.uint8), "cond": (lambda H, W: (7, H, W), torch.float32)}


def params():
    L = _lib.lib()
    return int(L.hav_raster_param(0)), int(L.hav_raster_param(1)), int(L.hav_raster_param(2))


def _desc(t):
    return "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__


def _need(verts, colors, tris, res):
    for name, t, dt in (("verts", verts, torch.float32), ("colors", colors, torch.float32), ("tris", tris, torch.int32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise RuntimeError("raster_ops: %s is a contiguous %s HIP tensor (got %s); there is no fallback path" % (name, dt, _desc(t)))
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
        raise RuntimeError("raster_ops: verts is [B,V,3] (got %s)" % (tuple(verts.shape),))
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if tuple(colors.shape) not in ((B, V, 3), (V, 3)) or colors.device != verts.device:
        raise RuntimeError("raster_ops: colors is [B,V,3] or [V,3] = [%d,%d,3] on the vertices' device (got %s)" % (B, V, _desc(colors)))
    if tris.dim() != 2 or tris.shape[1] != 3 or tris.shape[0] < 1 or tris.device != verts.device:
        raise RuntimeError("raster_ops: tris is [F >= 1, 3] on the vertices' device (got %s)" % _desc(tris))
    res, F = int(res), int(tris.shape[0])
    if res < 1 or B * 3 * res * res >= 2 ** 31:
        raise RuntimeError("raster_ops: B 3 H W = %d x 3 x %d x %d must lie in [1, 2^31): the kernels' pixel indices are int32" % (B, res, res))
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise RuntimeError("raster_ops: V = %d and F = %d must be below 2^31" % (V, F))
    return B, V, F, res


def _view34(rots, bounds, cam_dist):
    cam_dist = float(cam_dist)
    if cam_dist != cam_dist or cam_dist in (float("inf"), float("-inf")):
        raise RuntimeError("raster_ops: cam_dist must be finite (got %r)" % cam_dist)
    scale, trans = get_box_warp_param(*bounds)
    vals = list(scale) + list(trans) + [float(v) for R in rots for row in R for v in row] + [cam_dist]
    if len(vals) != 34 or any(v != v or v in (float("inf"), float("-inf")) for v in vals):
        raise RuntimeError("raster_ops: rots holds three finite 3 x 3 matrices and bounds three finite (lo, hi) pairs")
    return (C.c_float * 34)(*vals)


def workspaces(B, V, res, device):
    return (torch.empty(B, 3, res, res, dtype=torch.int64, device=device), torch.empty(B, 3, V, 4, dtype=torch.float32, device=device))


def raster_into(out, keys, screen, verts, colors, tris, res, rots, bounds, cam_dist=10.0):
    B, V, F, res = _need(verts, colors, tris, res)
    view = _view34(rots, bounds, cam_dist)
    unknown = sorted(set(out) - set(OUTPUTS))
    if unknown or not any(out.get(k) is not None for k in OUTPUTS):
        raise RuntimeError("raster_ops: outputs are named %s and at least one is given (got %s)" % (", ".join(OUTPUTS), sorted(out)))
    for name, (tail, dt) in OUTPUTS.items():
        t = out.get(name)
        if t is not None and not (t.is_cuda and t.device == verts.device and t.dtype == dt and t.is_contiguous()
                                  and tuple(t.shape) == (B, 3) + tail(res, res)):
            raise RuntimeError("raster_ops: %s is a contiguous %s HIP tensor %s on the vertices' device (got %s)"
                               % (name, dt, (B, 3) + tail(res, res), _desc(t)))
    for name, t, dt, shape in (("keys", keys, torch.int64, (B, 3, res, res)), ("screen", screen, torch.float32, (B, 3, V, 4))):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == verts.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape
                and t.data_ptr() % 16 == 0):
            raise RuntimeError("raster_ops: the workspace %s is a contiguous, 16-byte aligned %s HIP tensor %s on the vertices' device (got %s)"
                               % (name, dt, shape, _desc(t)))
    with torch.cuda.device(verts.device):
        _lib.check(_lib.lib().hav_raster_ortho_f32(*[_p(out.get(k)) for k in OUTPUTS], _p(keys), _p(screen), _p(verts), _p(colors), _p(tris),
                                                   B, V, F, res, res, int(colors.dim() == 3), view, _stream(verts.device)),
                   "hav_raster_ortho_f32")
    return out


def raster(verts, colors, tris, res, rots, bounds, cam_dist=10.0, outputs=tuple(OUTPUTS)):
    B, V, F, res = _need(verts, colors, tris, res)
    out = {k: torch.empty((B, 3) + OUTPUTS[k][0](res, res), dtype=OUTPUTS[k][1], device=verts.device) for k in outputs}
    keys, screen = workspaces(B, V, res, verts.device)
    return raster_into(out, keys, screen, verts, colors, tris, res, rots, bounds, cam_dist)

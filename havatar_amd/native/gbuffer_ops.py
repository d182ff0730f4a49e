"""The G-buffer kernel (csrc/hav_gbuffer.hip): depth, normal and shade maps of rendered frames from the march's ray table and its depth and
accumulation maps, contiguous float32 HIP tensors.
  gbuffer(rays, depth, acc, H, W, acc_min, outputs=OUTPUTS)   -> {name: tensor}, one launch for all B frames, allocated here
  gbuffer_into(out, rays, depth, acc, H, W, acc_min)          the launch on the caller's buffers: out = {name: tensor}, a missing name is not written
  TILE_H, TILE_W                                              the pixel tile of a workgroup, read from the library (None until lib() loads)
No atomics: the same inputs give the same bits on every call.  No allocation inside the entry and no host read: the call can be captured into
a hipGraph.  No fallback in here -- havatar_amd.geometry.gbuffer decides which tensors come this way and states the same definition on ATen for
the others."""
import torch

from .. import _lib
from .conv import _p, _stream

# name -> (trailing shape, dtype), in the order of hav_gbuffer_f32's output pointers
OUTPUTS = {"z": ((), torch.float32), "normal": ((3,), torch.float32), "mask": ((), torch.uint8), "depth16": ((2,), torch.uint8),
           "normal8": ((3,), torch.uint8), "shade8": ((), torch.uint8), "choice": ((), torch.uint8)}


def tile():
    L = _lib.lib()
    return int(L.hav_gbuffer_tile(0)), int(L.hav_gbuffer_tile(1))


def __getattr__(name):          # TILE_H / TILE_W: read from the library on first use, so importing this module does not need the build
    if name in ("TILE_H", "TILE_W"):
        return tile()[0 if name == "TILE_H" else 1]
    raise AttributeError(name)


def _need(rays, depth, acc, H, W):
    for name, t in (("rays", rays), ("depth", depth), ("acc", acc)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("gbuffer_ops: %s is a contiguous float32 HIP tensor (got %s); there is no fallback path"
                               % (name, "%s %s %s" % (t.device, t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    H, W = int(H), int(W)
    if rays.dim() != 3 or H < 1 or W < 1 or rays.shape[1] != H * W or rays.shape[2] < 8 or rays.shape[0] < 1:
        raise RuntimeError("gbuffer_ops: rays is [B, H W, stride >= 8] with H, W >= 1 (got %s for %d x %d)" % (tuple(rays.shape), H, W))
    B = rays.shape[0]
    for name, t in (("depth", depth), ("acc", acc)):
        if t.numel() != B * H * W or t.shape[0] != B or t.device != rays.device:
            raise RuntimeError("gbuffer_ops: %s holds [B, H W] = [%d, %d] values on the rays' device (got %s on %s)"
                               % (name, B, H * W, tuple(t.shape), t.device))
    if rays.numel() >= 2 ** 31:
        raise RuntimeError("gbuffer_ops: B H W stride = %d does not fit the kernel's int32 indices" % rays.numel())
    return B, H, W


def gbuffer_into(out, rays, depth, acc, H, W, acc_min=0.5):
    B, H, W = _need(rays, depth, acc, H, W)
    acc_min = float(acc_min)
    if acc_min != acc_min or acc_min in (float("inf"), float("-inf")):
        raise RuntimeError("gbuffer_ops: acc_min must be finite (got %r)" % acc_min)
    unknown = sorted(set(out) - set(OUTPUTS))
    if unknown or not any(out.get(k) is not None for k in OUTPUTS):
        raise RuntimeError("gbuffer_ops: outputs are named %s and at least one is given (got %s)" % (", ".join(OUTPUTS), sorted(out)))
    for name, (tail, dt) in OUTPUTS.items():
        t = out.get(name)
        if t is not None and not (t.is_cuda and t.device == rays.device and t.dtype == dt and t.is_contiguous()
                                  and tuple(t.shape) == (B, H, W) + tail):
            raise RuntimeError("gbuffer_ops: %s is a contiguous %s HIP tensor %s on the rays' device (got %s %s on %s)"
                               % (name, dt, (B, H, W) + tail, t.dtype, tuple(t.shape), t.device))
    with torch.cuda.device(rays.device):
        _lib.check(_lib.lib().hav_gbuffer_f32(*[_p(out.get(k)) for k in OUTPUTS], _p(rays), _p(depth), _p(acc), B, H, W, int(rays.shape[2]),
                                              acc_min, _stream(rays.device)), "hav_gbuffer_f32")
    return out


def gbuffer(rays, depth, acc, H, W, acc_min=0.5, outputs=tuple(OUTPUTS)):
    B, H, W = _need(rays, depth, acc, H, W)
    out = {k: torch.empty((B, H, W) + OUTPUTS[k][0], dtype=OUTPUTS[k][1], device=rays.device) for k in outputs}
    return gbuffer_into(out, rays, depth, acc, H, W, acc_min)

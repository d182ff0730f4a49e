"""The image-metrics entries of libhavatar_hip.so (csrc/hav_metrics.hip): mean SSIM and mean squared error of an image pair in one pass.
  image_metrics_f32   a, b [B,C,H,W] float32 on a HIP device
  image_metrics_u8    a, b [B,H,W,3] uint8 on a HIP device (channels-last, what a PNG is), taken as 0..255 with L = 255
Both return (out [B,2] float32 = (mean SSIM, mse), map [B,C,H-10,W-10] float32 or None).  Inference metrics: no autograd.  No fallback in here --
havatar_amd.metrics decides which calls come this way (eligible()) and states the same definition on ATen for the others.

HAVATAR_METRICS (read at the call): 0 = the ATen statement throughout; unset / 1 = these entries for eligible HIP tensors (DESIGN.md 7.9 holds the
measurement that decided the default)."""
import torch

from .. import _lib, switches
from .conv import _p, _stream

DEFAULT = switches.default("HAVATAR_METRICS")
WIN = 11                       # window taps; the map is [H - WIN + 1, W - WIN + 1]
TILE_H, TILE_W = 32, 32        # map elements per workgroup (MET_TH, MET_TW of csrc/hav_metrics.hip)


def enabled():
    return switches.on("HAVATAR_METRICS")


def eligible(a, b):
    """a HIP pair the entries take: float32 [B,C,H,W] or uint8 [B,H,W,3], H, W >= 11, nothing that needs a gradient"""
    if not (a.is_cuda and b.is_cuda and a.device == b.device and a.dim() == 4 and a.shape == b.shape and a.dtype == b.dtype):
        return False
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        return False
    if a.dtype == torch.float32:
        return a.shape[2] >= WIN and a.shape[3] >= WIN
    return a.dtype == torch.uint8 and a.shape[3] == 3 and a.shape[1] >= WIN and a.shape[2] >= WIN


def _need(a, b, dtype):
    for t in (a, b):
        if not (t.is_cuda and t.dtype == dtype and t.dim() == 4):
            raise RuntimeError("metrics_ops: 4-d HIP %s tensors only (got %s %s %s); there is no fallback path"
                               % (dtype, t.device.type, t.dtype, tuple(t.shape)))
    if a.shape != b.shape:
        raise RuntimeError("metrics_ops: the pair differs in shape: %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise RuntimeError("metrics_ops: the pair is on two devices: %s and %s" % (a.device, b.device))


def _run(entry, name, a, b, B, C, H, W, want_map, extra):
    L = _lib.lib()
    n = int(L.hav_image_metrics_blocks(B, C, H, W))
    if n == 0:
        raise RuntimeError("%s: a pair of shape %s is not covered (H, W >= %d, at most 2^31 - 1 workgroups)" % (name, tuple(a.shape), WIN))
    a, b = a.detach().contiguous(), b.detach().contiguous()
    out = torch.empty(B, 2, dtype=torch.float32, device=a.device)
    partials = torch.empty(n, dtype=torch.float64, device=a.device)
    smap = torch.empty(B, C, H - WIN + 1, W - WIN + 1, dtype=torch.float32, device=a.device) if want_map else None
    with torch.cuda.device(a.device):
        _lib.check(entry(L)(_p(out), _p(partials), _p(smap), _p(a), _p(b), *extra, _stream(a.device)), name)
    return out, smap


def image_metrics_f32(a, b, data_range=1.0, want_map=False):
    _need(a, b, torch.float32)
    B, C, H, W = a.shape
    return _run(lambda L: L.hav_image_metrics_f32, "hav_image_metrics_f32", a, b, B, C, H, W, want_map, (B, C, H, W, float(data_range)))


def image_metrics_u8(a, b, want_map=False):
    _need(a, b, torch.uint8)
    B, H, W, C = a.shape
    if C != 3:
        raise RuntimeError("metrics_ops: uint8 pairs are [B,H,W,3] (got %s)" % (tuple(a.shape),))
    return _run(lambda L: L.hav_image_metrics_u8, "hav_image_metrics_u8", a, b, B, 3, H, W, want_map, (B, H, W))

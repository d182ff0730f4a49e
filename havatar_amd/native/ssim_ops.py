"""The autograd node of the SSIM training loss (csrc/hav_ssim_loss.hip): mean SSIM per sample of a float32 HIP pair with a gradient to the
first image.
  ssim_mean(pred, target, data_range)   pred, target [B,C,H,W] float32 on a HIP device -> ssim [B] float32
The forward is hav_image_metrics_f32 (native/metrics_ops.py) -- the bits of metrics.ssim(pred.detach(), target); the backward is
hav_ssim_loss_bwd_f32: two launches, float64 between the float32 loads and the one float32 store, no atomics.  The target is a
constant: it gets no gradient.  Once differentiable.  No fallback in here -- havatar_amd.metrics.ssim_loss decides which calls come this way and
states the same loss on ATen for the others."""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import metrics_ops
from .conv import _p, _stream

WIN = metrics_ops.WIN


def ssim_grad(gout, x, y, data_range=1.0, out=None):
    """d(sum_b gout[b] ssim_b) / dx for float32 HIP x, y [B,C,H,W] and gout [B]; every element of the result is written (out: a contiguous
    float32 buffer of x's shape to write into, whatever it holds)"""
    metrics_ops._need(x, y, torch.float32)
    if not (gout.is_cuda and gout.dtype == torch.float32 and gout.dim() == 1 and gout.shape[0] == x.shape[0] and gout.device == x.device):
        raise RuntimeError("ssim_ops: the output gradient is a float32 HIP [B] tensor on the pair's device (got %s %s %s); there is no fallback path"
                           % (gout.device, gout.dtype, tuple(gout.shape)))
    B, C, H, W = x.shape
    L = _lib.lib()
    if int(L.hav_ssim_grad_blocks(B, C, H, W)) == 0:
        raise RuntimeError("hav_ssim_loss_bwd_f32: a pair of shape %s is not covered (H, W >= %d, at most 2^31 - 1 workgroups)" % (tuple(x.shape), WIN))
    x, y, gout = x.detach().contiguous(), y.detach().contiguous(), gout.detach().contiguous()
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous() and out.device == x.device):
        raise RuntimeError("ssim_ops: out is a contiguous float32 HIP tensor of the pair's shape and device")
    grad = torch.empty_like(x) if out is None else out
    ws = torch.empty(3 * B * C * (H - WIN + 1) * (W - WIN + 1), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.hav_ssim_loss_bwd_f32(_p(grad), _p(ws), _p(x), _p(y), _p(gout), B, C, H, W, float(data_range), _stream(x.device)),
                   "hav_ssim_loss_bwd_f32")
    return grad


class SsimMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, data_range):
        pred, target = pred.contiguous(), target.contiguous()
        out, _ = metrics_ops.image_metrics_f32(pred, target, data_range, False)
        ctx.save_for_backward(pred, target)
        ctx.data_range = float(data_range)
        return out[:, 0].contiguous()

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError("SsimMean is once differentiable: backward under create_graph=True is not supported (nothing in the training "
                               "steps differentiates SSIM twice); set HAVATAR_METRICS=0 for the ATen statement")
        return SsimMean._backward(ctx, g)

    @staticmethod
    @once_differentiable
    def _backward(ctx, g):
        if ctx.needs_input_grad[1]:
            raise RuntimeError("SsimMean: the target is a constant (no gradient to the second image); set HAVATAR_METRICS=0 for the ATen statement")
        if not ctx.needs_input_grad[0]:
            return None, None, None
        pred, target = ctx.saved_tensors
        return ssim_grad(g.reshape(-1).to(torch.float32), pred, target, ctx.data_range), None, None


def ssim_mean(pred, target, data_range=1.0):
    """[B] mean SSIM per sample, differentiable in pred (made contiguous inside: the stage-one patch arrives as a permuted view)"""
    metrics_ops._need(pred, target, torch.float32)
    return SsimMean.apply(pred, target.detach(), float(data_range))

"""Autograd nodes of the LPIPS-VGG module (model/lpips.py) over libhavatar_hip.so (csrc/hav_lpips.hip, csrc/hav_conv.hip):
  ConvReluFrozen   relu(conv3x3(x, W) + bias) with FROZEN W, bias: forward on hav_conv3x3_split (bias and ReLU in its epilogue, slope 0), backward =
                   hav_relu_mask_bwd then the data gradient on hav_conv3x3_split with the hav_conv3x3_pack_t blob.  Saves y only: no weight
                   gradient is ever formed, so x is not kept.
  LpipsHead        one tap's  mean_{h,w} sum_c w[c] (a^ - b^)^2  (hav_lpips_head_fwd / _bwd).  THE ONE DELIBERATE DIFFERENCE to the PyTorch
                   statement: at a pixel whose features are all zero the gradient is finite (the term that carries 1 / n is dropped, its limit
                   is 0) where ATen's autograd, differentiating sqrt at 0, returns NaN.
Both are once differentiable (nothing in either training step differentiates LPIPS twice); under create_graph they raise.
HIP float32 tensors only; no fallback in here -- conv_relu_eligible() tells the module which layers stay on ATen.

HAVATAR_LPIPS (read at the call): 0 = the ATen statement throughout; 1 = the nodes; unset = DEFAULT below (DESIGN.md 7.8 holds the
measurement that decided it)."""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib, switches
from . import conv as nconv

DEFAULT = switches.default("HAVATAR_LPIPS")


def enabled():
    return switches.on("HAVATAR_LPIPS")


def _need_hip(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError("lpips_ops: HIP float32 tensors only (got %s %s); there is no fallback path" % (t.device.type, t.dtype))


def conv_relu_eligible(x, weight):
    """x [B,Cin,H,W] float32 on a HIP device, weight [Cout,Cin,3,3]: native.conv.eligible for the layer AND for its transposed layer (the data
    gradient: Cout inputs, Cin outputs, the same map), i.e. Cin % 64 == 0, Cout % 64 == 0 and
    (H % 4 == 0 and W % 32 == 0) or (H % 8 == 0 and W % 16 == 0)."""
    if not nconv.eligible(x, weight):
        return False
    Cout, Cin = weight.shape[:2]
    return Cin % 64 == 0 and Cout % 64 == 0


def relu_mask_bwd(g, y, want_bias=False):
    """gc = g * [y > 0] (hav_relu_mask_bwd); want_bias: also gbias [C] = sum over batch and pixels of gc -> (gc, gbias)"""
    _need_hip(g, y)
    g, y = g.contiguous(), y.contiguous()
    B, Cc = y.shape[:2]
    HW = y.numel() // (B * Cc)
    gc = torch.empty_like(y)
    gb = torch.empty(Cc, dtype=torch.float32, device=y.device) if want_bias else None
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().hav_relu_mask_bwd(nconv._p(gc), nconv._p(gb), nconv._p(g), nconv._p(y), B, Cc, HW, nconv._stream(y.device)),
                   "hav_relu_mask_bwd")
    return (gc, gb) if want_bias else gc


class ConvReluFrozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, pack, pack_t, Cout):
        _need_hip(x, bias)
        y = nconv.conv3x3(x, pack, Cout, bias=bias, slope=0.0, gain=1.0, act=True)          # (range control as every conv3x3 call: absmax of x)
        ctx.save_for_backward(y)
        ctx.pack_t, ctx.Cin = pack_t, x.shape[1]
        return y

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError("ConvReluFrozen is once differentiable: backward under create_graph=True is not supported (nothing in the "
                               "training steps differentiates LPIPS twice); set HAVATAR_LPIPS=0 for the ATen statement")
        return ConvReluFrozen._backward(ctx, g)

    @staticmethod
    @once_differentiable
    def _backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        y, = ctx.saved_tensors
        gc = relu_mask_bwd(g, y)
        gx = nconv.conv3x3(gc, ctx.pack_t, ctx.Cin, act=False, autoscale=True)          # gradients are ~1e-6: see hav_absmax
        return gx, None, None, None, None


def conv_relu_frozen(x, bias, pack, pack_t, Cout):
    """relu(conv3x3(x, W) + bias) for frozen W, bias: pack / pack_t = native.conv.pack(W) / pack_t(W); callers check conv_relu_eligible"""
    return ConvReluFrozen.apply(x.contiguous(), bias, pack, pack_t, Cout)


def head_fwd(f0, f1, w):
    """[B] = one tap's distance per sample; f0, f1 [B,C,H,W] contiguous, w [C]"""
    _need_hip(f0, f1, w)
    B, Cc, H, W = f0.shape
    if f1.shape != f0.shape or w.numel() != Cc:
        raise RuntimeError("lpips head: f0 %s, f1 %s, w %s" % (tuple(f0.shape), tuple(f1.shape), tuple(w.shape)))
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float32, device=f0.device)
    partials = torch.empty(int(L.hav_lpips_head_blocks(B, Cc, H, W)), dtype=torch.float64, device=f0.device)
    with torch.cuda.device(f0.device):
        _lib.check(L.hav_lpips_head_fwd(nconv._p(out), nconv._p(partials), nconv._p(f0), nconv._p(f1), nconv._p(w), B, Cc, H, W,
                                        nconv._stream(f0.device)), "hav_lpips_head_fwd")
    return out


def head_bwd(gout, f0, f1, w, want0=True, want1=True):
    """(d/df0, d/df1) of head_fwd given gout [B]; the one not wanted is None (and never computed)"""
    _need_hip(gout, f0, f1, w)
    if not (want0 or want1):
        return None, None
    B, Cc, H, W = f0.shape
    g0 = torch.empty_like(f0) if want0 else None
    g1 = torch.empty_like(f1) if want1 else None
    with torch.cuda.device(f0.device):
        _lib.check(_lib.lib().hav_lpips_head_bwd(nconv._p(g0), nconv._p(g1), nconv._p(gout), nconv._p(f0), nconv._p(f1), nconv._p(w), B, Cc, H, W,
                                                 nconv._stream(f0.device)), "hav_lpips_head_bwd")
    return g0, g1


class LpipsHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f0, f1, w):
        ctx.save_for_backward(f0, f1, w)
        return head_fwd(f0, f1, w).view(-1, 1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError("LpipsHead is once differentiable: backward under create_graph=True is not supported (nothing in the training "
                               "steps differentiates LPIPS twice); set HAVATAR_LPIPS=0 for the ATen statement")
        return LpipsHead._backward(ctx, g)

    @staticmethod
    @once_differentiable
    def _backward(ctx, g):
        f0, f1, w = ctx.saved_tensors
        g0, g1 = head_bwd(g.reshape(-1).contiguous(), f0, f1, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return g0, g1, None


def lpips_head(f0, f1, w):
    """f0, f1 [B,C,H,W]; w the tap's [1,C,1,1] weights -> [B,1,1,1]"""
    return LpipsHead.apply(f0.contiguous(), f1.contiguous(), w.reshape(-1).contiguous())

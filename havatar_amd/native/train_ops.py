"""Training-path field ops (hav_field_inputs_*, hav_composite_*): the HIP counterparts, under autograd, of what surrounds the
radiance MLP in predict_and_render_radiance -- skinning field + box warp + tri-plane gather + positional encoding on one side,
volume_render_radiance_field on the other.  HIP float32 tensors only; there is no fallback in here."""
import ctypes as C

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib, switches

# Under torch.autocast these nodes compute in fp32 like everywhere else: inputs are cast to fp32 and autocast is off inside forward AND backward
# (without this, torch.mm inside Conv3dSmall.forward would return bf16 under autocast while backward, which runs outside it, multiplies a
# bf16 gradient with the saved fp32 patch matrix: dtype mismatch; the kernels themselves refuse anything but fp32).
_fwd32 = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_bwd32 = torch.amp.custom_bwd(device_type="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_hip(name, *ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(name + ": HIP float32 tensors only")


def _field_params(pts, planes_cl, vol, boxes):
    P, B, H, W, Cc = planes_cl.shape
    if P != 2 or pts.ndim != 3 or pts.shape[0] != B or pts.shape[-1] != 3:
        raise RuntimeError("field_inputs: planes [2,B,H,W,C], pts [B,N,3]")
    if vol.ndim != 5 or vol.shape[0] != 1 or vol.shape[1] != 2 or not (vol.shape[2] == vol.shape[3] == vol.shape[4]):
        raise RuntimeError("field_inputs: skinning volume [1,2,D,D,D]")
    p = _lib.HavFieldParams()
    p.n, p.n_per_b, p.B, p.H, p.W, p.C, p.D = B * pts.shape[1], pts.shape[1], B, H, W, Cc, vol.shape[2]
    for name, v in zip(("nerf_scale", "nerf_trans", "skin_scale", "skin_trans"), boxes):
        setattr(p, name, (C.c_float * 3)(*[float(x) for x in v]))
    return p


def deterministic():
    """HAVATAR_DETERMINISTIC=1: the training-side scatters sum in 64-bit fixed point (bit-reproducible gradients; ~1 ms per step)."""
    return switches.off("HAVATAR_DETERMINISTIC")


class FieldInputs(Function):
    """X [B*N, 2C+48] = cat(triplane(boxwarp(p')), PE(p')),  p' = skinning_field(pts, inv_T, vol).  Gradients: planes_cl, vol."""

    @staticmethod
    @_fwd32
    def forward(ctx, pts, inv_T, vol, planes_cl, boxes, ray_rows=0):
        _need_hip("FieldInputs", pts, inv_T, vol, planes_cl)
        pts, inv_T, vol, planes_cl = pts.contiguous(), inv_T.contiguous(), vol.contiguous(), planes_cl.contiguous()
        p = _field_params(pts, planes_cl, vol, boxes)
        X = torch.empty(p.n, 2 * p.C + 48, device=pts.device, dtype=torch.float32)
        with torch.cuda.device(pts.device):
            rc = _lib.lib().hav_field_inputs_fwd(_p(X), C.byref(p), _p(pts), _p(inv_T), _p(vol), _p(planes_cl), _stream())
        _lib.check(rc, "hav_field_inputs_fwd")
        ctx.save_for_backward(pts, inv_T, vol, planes_cl)
        ctx.boxes, ctx.ray_rows = boxes, ray_rows
        return X

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, dX):
        pts, inv_T, vol, planes_cl = ctx.saved_tensors
        dvol, dpl = _field_backward(pts, inv_T, vol, planes_cl, ctx.boxes, dX, ctx.needs_input_grad[2], ctx.needs_input_grad[3],
                                    ctx.ray_rows)
        return None, None, dvol, dpl, None, None


def _field_backward(pts, inv_T, vol, planes_cl, boxes, dX, need_vol, need_planes, ray_rows=0):
    """(dvol, dplanes_cl) of the field inputs from dX [n, 2C+48] float32 (hav_field_inputs_bwd, or its fixed-point form).  ray_rows > 0 =
    the samples per ray of queries whose neighbouring rays are neighbouring pixels (hav_field_inputs_bwd_rows: the same sums, the scatter
    merges across 16 rays instead of along one)"""
    p = _field_params(pts, planes_cl, vol, boxes)
    det = deterministic() and p.C <= 64
    mk = torch.empty_like if det else torch.zeros_like          # (the fixed-point route writes every element itself)
    dvol = mk(vol) if need_vol else None
    dpl = mk(planes_cl) if need_planes else None
    if dvol is not None or dpl is not None:
        dX = dX.contiguous()
        L = _lib.lib()
        with torch.cuda.device(pts.device):
            if det:
                # HAVATAR_DETERMINISTIC=1: 64-bit fixed-point sums, integer atomics -- the same bits on every run (the float atomics of
                # the default route land in a different order every time)
                from .conv import absmax
                words = absmax(dX)
                scratch = torch.empty(int(L.hav_field_inputs_bwd_fixed_scratch_bytes(C.byref(p))), dtype=torch.uint8, device=pts.device)
                rc = L.hav_field_inputs_bwd_fixed(_p(dpl), _p(dvol), _p(dX), _p(words), _p(scratch), C.byref(p), _p(pts), _p(inv_T), _p(vol),
                                                  _p(planes_cl), _stream())
            elif ray_rows > 0:
                rc = L.hav_field_inputs_bwd_rows(_p(dpl), _p(dvol), _p(dX), C.byref(p), _p(pts), _p(inv_T), _p(vol), _p(planes_cl), int(ray_rows),
                                                 _stream())
            else:
                rc = L.hav_field_inputs_bwd(_p(dpl), _p(dvol), _p(dX), C.byref(p), _p(pts), _p(inv_T), _p(vol), _p(planes_cl), _stream())
        _lib.check(rc, "hav_field_inputs_bwd")
        from .conv import _trace
        _trace("FieldInputs.bwd dX,dvol,dplanes,vol", dX, dvol, dpl, vol)          # (development aid; a no-op unless HAVATAR_NAN_TRACE)
    return dvol, dpl


class FieldMlp(Function):
    """rf [B*N, 68] = radiance_mlp(field_inputs(pts)) as ONE autograd node: the rows X between the two kernels are bf16 (the MLP's bf16
    kernels round fp32 rows exactly so -- same rf, same gradients as FieldInputs -> FusedMlp), written once and read twice at half the
    bytes, and kept for the backward at half the memory.  Gradients: vol, planes_cl, the ten MLP tensors."""

    @staticmethod
    @_fwd32
    def forward(ctx, pts, inv_T, vol, planes_cl, boxes, ray_rows, *weights):
        from . import mlp_train
        _need_hip("FieldMlp", pts, inv_T, vol, planes_cl)
        pts, inv_T, vol, planes_cl = pts.contiguous(), inv_T.contiguous(), vol.contiguous(), planes_cl.contiguous()
        p = _field_params(pts, planes_cl, vol, boxes)
        X = torch.empty(p.n, 2 * p.C + 48, device=pts.device, dtype=torch.bfloat16)
        with torch.cuda.device(pts.device):
            rc = _lib.lib().hav_field_inputs_fwd_bf16(_p(X), C.byref(p), _p(pts), _p(inv_T), _p(vol), _p(planes_cl), _stream())
        _lib.check(rc, "hav_field_inputs_fwd_bf16")
        blob = mlp_train.pack(weights)
        ctx.save_for_backward(pts, inv_T, vol, planes_cl, X, blob)
        ctx.boxes, ctx.ray_rows = boxes, ray_rows
        ctx.shapes = [tuple(w.shape) for w in weights]
        return mlp_train.forward_only(X, blob)

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, d_rf):
        from . import mlp_train
        pts, inv_T, vol, planes_cl, X, blob = ctx.saved_tensors
        need_vol, need_pl = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dX, grads = mlp_train.backward_only(X, d_rf.contiguous(), blob, ctx.shapes, need_dx=need_vol or need_pl)
        dvol, dpl = _field_backward(pts, inv_T, vol, planes_cl, ctx.boxes, dX, need_vol, need_pl, ctx.ray_rows) if dX is not None else (None, None)
        return (None, None, dvol, dpl, None, None) + tuple(grads)


def field_mlp_eligible(planes_nchw, weights):
    """shapes FieldMlp takes: C = 64 channels per plane (2C + 48 = 176 input columns) and the radiance MLP the bf16 kernels are written for"""
    from . import mlp_train
    return planes_nchw.shape[2] == 64 and [tuple(w.shape) for w in weights] == mlp_train._SHAPES


def field_mlp(pts, inv_T, vol, planes_nchw, nerf_box, skin_box, weights, ray_rows=0):
    """as field_inputs() followed by mlp_train.fused_mlp(): pts [B,N,3] ... -> rf [B*N, 68]"""
    boxes = (tuple(nerf_box[0]), tuple(nerf_box[1]), tuple(skin_box[0]), tuple(skin_box[1]))
    return FieldMlp.apply(pts, inv_T, vol, planes_nchw.permute(0, 1, 3, 4, 2).contiguous(), boxes, int(ray_rows), *weights)


def field_inputs(pts, inv_T, vol, planes_nchw, nerf_box, skin_box, ray_rows=0):
    """pts [B,N,3], inv_T [B,4,3], vol [1,2,D,D,D], planes [2,B,C,H,W] (the Trainer's layout), boxes = (scale3, trans3) of the two
    UniformBoxWarp_new modules -> X [B*N, 2C+48].  The NCHW -> channels-last permutation is a differentiable ATen op.  ray_rows = S when
    pts is [B, rays, S] flattened and neighbouring rays are neighbouring pixels of an image row (the training patch): a hint for the backward."""
    boxes = (tuple(nerf_box[0]), tuple(nerf_box[1]), tuple(skin_box[0]), tuple(skin_box[1]))
    return FieldInputs.apply(pts, inv_T, vol, planes_nchw.permute(0, 1, 3, 4, 2).contiguous(), boxes, int(ray_rows))


class Composite(Function):
    """(rgb [n,CH], acc [n], weights [n,S], depth [n]) = volume_render_radiance_field(rf [n,S,CH+1], z, rd, noise, bg)."""

    @staticmethod
    @_fwd32
    def forward(ctx, rf, z, rd, noise, bg, n_sigmoid):
        _need_hip("Composite", rf, z, rd, noise, bg)
        rf, z, rd = rf.contiguous(), z.contiguous(), rd.contiguous()
        noise = noise.contiguous() if noise is not None else None
        bg = bg.contiguous() if bg is not None else None
        n, S, RW = rf.shape
        if z.shape != (n, S) or rd.shape != (n, 3) or (noise is not None and noise.shape != (n, S)) or (bg is not None and bg.shape != (n, 3)):
            raise RuntimeError("Composite: rf [n,S,CH+1], z [n,S], rd [n,3], noise [n,S], bg [n,3]")
        rgb = torch.empty(n, RW - 1, device=rf.device, dtype=torch.float32)
        acc, depth = torch.empty(n, device=rf.device), torch.empty(n, device=rf.device)
        w = torch.empty(n, S, device=rf.device)
        with torch.cuda.device(rf.device):
            rc = _lib.lib().hav_composite_fwd(_p(rgb), _p(acc), _p(w), _p(depth), _p(rf), _p(z), _p(rd), _p(noise), _p(bg), n, S, RW - 1,
                                              int(n_sigmoid), _stream())
        _lib.check(rc, "hav_composite_fwd")
        ctx.save_for_backward(rf, z, rd, noise, bg)
        ctx.n_sigmoid = int(n_sigmoid)
        return rgb, acc, w, depth

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, d_rgb, d_acc, d_w, d_depth):
        rf, z, rd, noise, bg = ctx.saved_tensors
        n, S, RW = rf.shape
        d_rf = torch.empty_like(rf)
        d_rgb = d_rgb.contiguous() if d_rgb is not None else torch.zeros(n, RW - 1, device=rf.device)
        d_acc, d_w, d_depth = [t.contiguous() if t is not None else None for t in (d_acc, d_w, d_depth)]
        with torch.cuda.device(rf.device):
            rc = _lib.lib().hav_composite_bwd(_p(d_rf), _p(d_rgb), _p(d_acc), _p(d_w), _p(d_depth), _p(rf), _p(z), _p(rd), _p(noise),
                                              _p(bg), n, S, RW - 1, ctx.n_sigmoid, _stream())
        _lib.check(rc, "hav_composite_bwd")
        from .conv import _trace
        _trace("Composite.bwd d_rf,d_rgb,rf", d_rf, d_rgb, rf)
        return d_rf, None, None, None, None, None


def composite(rf, z, rd, noise=None, bg=None, n_sigmoid=3):
    return Composite.apply(rf, z, rd, noise, bg, n_sigmoid)


class CompositeLong(Function):
    """Composite for 1 <= S <= 128 samples per ray (hav_composite_long_*: two adjacent samples per lane).  Same tensors, same maps; the
    transmittance product is associated as a tree, so results agree with Composite to rounding, not to the bit.  bwd_form names the
    backward's arrangement (0 = by shape; include/havatar.h::hav_composite_long_bwd_form) for the A/B tool and the tests."""

    @staticmethod
    @_fwd32
    def forward(ctx, rf, z, rd, noise, bg, n_sigmoid, bwd_form=0):
        _need_hip("CompositeLong", rf, z, rd, noise, bg)
        rf, z, rd = rf.contiguous(), z.contiguous(), rd.contiguous()
        noise = noise.contiguous() if noise is not None else None
        bg = bg.contiguous() if bg is not None else None
        n, S, RW = rf.shape
        if z.shape != (n, S) or rd.shape != (n, 3) or (noise is not None and noise.shape != (n, S)) or (bg is not None and bg.shape != (n, 3)):
            raise RuntimeError("CompositeLong: rf [n,S,CH+1], z [n,S], rd [n,3], noise [n,S], bg [n,3]")
        rgb = torch.empty(n, RW - 1, device=rf.device, dtype=torch.float32)
        acc, depth = torch.empty(n, device=rf.device), torch.empty(n, device=rf.device)
        w = torch.empty(n, S, device=rf.device)
        with torch.cuda.device(rf.device):
            rc = _lib.lib().hav_composite_long_fwd(_p(rgb), _p(acc), _p(w), _p(depth), _p(rf), _p(z), _p(rd), _p(noise), _p(bg), n, S, RW - 1,
                                                   int(n_sigmoid), _stream())
        _lib.check(rc, "hav_composite_long_fwd")
        ctx.save_for_backward(rf, z, rd, noise, bg)
        ctx.n_sigmoid, ctx.bwd_form = int(n_sigmoid), int(bwd_form)
        return rgb, acc, w, depth

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, d_rgb, d_acc, d_w, d_depth):
        rf, z, rd, noise, bg = ctx.saved_tensors
        n, S, RW = rf.shape
        d_rf = torch.empty_like(rf)
        d_rgb = d_rgb.contiguous() if d_rgb is not None else torch.zeros(n, RW - 1, device=rf.device)
        d_acc, d_w, d_depth = [t.contiguous() if t is not None else None for t in (d_acc, d_w, d_depth)]
        with torch.cuda.device(rf.device):
            rc = _lib.lib().hav_composite_long_bwd_form(_p(d_rf), _p(d_rgb), _p(d_acc), _p(d_w), _p(d_depth), _p(rf), _p(z), _p(rd), _p(noise),
                                                        _p(bg), n, S, RW - 1, ctx.n_sigmoid, ctx.bwd_form, _stream())
        _lib.check(rc, "hav_composite_long_bwd")
        from .conv import _trace
        _trace("CompositeLong.bwd d_rf,d_rgb,rf", d_rf, d_rgb, rf)
        return d_rf, None, None, None, None, None, None


def composite_long(rf, z, rd, noise=None, bg=None, n_sigmoid=3, bwd_form=0):
    """composite() for up to 128 samples per ray; raises RuntimeError where the library refuses (S > 128)."""
    return CompositeLong.apply(rf, z, rd, noise, bg, n_sigmoid, bwd_form)


def composite_long_eligible(S, rf_like):
    """what composite_long takes: a HIP float32 radiance field and at most 128 samples per ray"""
    return bool(rf_like.is_cuda and rf_like.dtype == torch.float32 and 1 <= int(S) <= 128)


def composite_long_enabled():
    """HAVATAR_COMPOSITE_LONG=1 (read at the call): a training step with 65-128 samples per pass stays on the native route"""
    return switches.off("HAVATAR_COMPOSITE_LONG")


def resample_depths(z, weights, num_fine, zeta=None, return_samples=False):
    """z2 [n, ceil(S_c/2)+num_fine] = sort(cat(z[:, ::2], sample_pdf(z_mid, weights[:, 1:-1], num_fine))) -- the statements of
    model/nerf_trainer.py:166-170 + utils/nerf_util.py:76-117 of the reference as one launch (hav_resample_depths).  z, weights
    [n, S_c] HIP float32; zeta [n, num_fine] = the raw torch.rand draw (the caller makes it, in the reference's order), None =
    det=True.  No gradient, like the reference's .detach()."""
    _need_hip("resample_depths", z, weights, zeta)
    z, weights = z.detach().contiguous(), weights.detach().contiguous()
    zeta = zeta.detach().contiguous() if zeta is not None else None
    n, S_c = z.shape
    num_fine = int(num_fine)
    if weights.shape != (n, S_c) or (zeta is not None and zeta.shape != (n, num_fine)):
        raise RuntimeError("resample_depths: z, weights [n,S_c], zeta [n,num_fine]")
    z2 = torch.empty(n, (S_c + 1) // 2 + num_fine, device=z.device, dtype=torch.float32)
    zs = torch.empty(n, num_fine, device=z.device, dtype=torch.float32) if return_samples else None
    with torch.cuda.device(z.device):
        rc = _lib.lib().hav_resample_depths(_p(z2), _p(zs), _p(z), _p(weights), _p(zeta), n, S_c, num_fine, _stream())
    _lib.check(rc, "hav_resample_depths")
    return (z2, zs) if return_samples else z2


class EqualLinearFn(Function):
    """y = F.linear(x, W * scale, bias * lr_mul) for x [B <= 8, in]: one launch forward, one backward (hav_equal_linear_*), instead of the
    3 + 6-7 ATen launches of the statement (model/styleUnet.py:128-162 of the reference) -- the modulation layer of every ModulatedConv2d
    and the discriminator's last layer.  Under create_graph=True the backward states the adjoints with differentiable ATen ops; inside
    conv2d_gradfix.no_weight_gradients() no weight gradient is formed."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, W, bias, scale, lr_mul):
        _need_hip("EqualLinearFn", x, W, bias)
        x, W = x.contiguous(), W.contiguous()
        bias = bias.contiguous() if bias is not None else None
        B, n_in = x.shape
        n_out = W.shape[0]
        if W.shape != (n_out, n_in) or (bias is not None and bias.shape != (n_out,)):
            raise RuntimeError("EqualLinearFn: x [B,in], W [out,in], bias [out]")
        y = torch.empty(B, n_out, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            rc = _lib.lib().hav_equal_linear_fwd(_p(y), _p(x), _p(W), _p(bias), float(scale), float(lr_mul), B, n_in, n_out, _stream())
        _lib.check(rc, "hav_equal_linear_fwd")
        ctx.save_for_backward(x, W)
        ctx.consts = (float(scale), float(lr_mul), bias is not None)
        return y

    @staticmethod
    @_bwd32
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        scale, lr_mul, has_bias = ctx.consts
        if torch.is_grad_enabled():
            # create_graph=True (R1 through the discriminator's last layer, path length through every modulation layer; reference
            # utils/styleUnet_util.py:74,92): the three adjoints as differentiable ATen statements, so that the second-order graph exists.
            # Inside conv2d_gradfix.no_weight_gradients() no weight gradient is formed, as in native/conv.py::_FusedConvBlock
            from ..model.op import conv2d_gradfix
            with torch.enable_grad():
                dx = torch.matmul(dy, W * scale) if ctx.needs_input_grad[0] else None
                dW = (torch.matmul(dy.t(), x) * scale if (ctx.needs_input_grad[1] and not conv2d_gradfix.weight_gradients_disabled)
                      else None)
                db = dy.sum(0) * lr_mul if (has_bias and ctx.needs_input_grad[2]) else None
            return dx, dW, db, None, None
        dy = dy.contiguous()
        B, n_in = x.shape
        n_out = W.shape[0]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(W) if ctx.needs_input_grad[1] else None
        db = torch.empty(n_out, device=x.device, dtype=torch.float32) if (has_bias and ctx.needs_input_grad[2]) else None
        with torch.cuda.device(x.device):
            rc = _lib.lib().hav_equal_linear_bwd(_p(dx), _p(dW), _p(db), _p(dy), _p(x), _p(W), scale, lr_mul, B, n_in, n_out, _stream())
        _lib.check(rc, "hav_equal_linear_bwd")
        return dx, dW, db, None, None


def equal_linear_eligible(x, W, bias):
    """training on HIP float32 tensors, a 2-D input of at most 8 rows (the style vectors of a batch), a shape the kernels take"""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and 1 <= x.shape[0] <= 8 and W.dtype == torch.float32 and W.dim() == 2
            and x.shape[1] == W.shape[1] and W.shape[1] <= 4096 and W.shape[0] * W.shape[1] <= (1 << 24)
            and (bias is None or bias.dtype == torch.float32) and torch.is_grad_enabled()
            and (x.requires_grad or W.requires_grad or (bias is not None and bias.requires_grad)))


def equal_linear(x, W, bias, scale, lr_mul):
    # (contiguous OUTSIDE the node: inside, where grad mode is off, a copy would be saved detached and cut the create_graph branch's graph)
    return EqualLinearFn.apply(x.contiguous(), W.contiguous(), bias, scale, lr_mul)


class Upsample3d2x(Function):
    """nn.Upsample(scale_factor=2, mode='trilinear', align_corners=False) on a float32 HIP tensor [N,C,D,H,W]: one launch forward,
    one backward (hav_upsample3d_2x_*), instead of the ~30 / ~60 ATen launches of the slice-and-lerp statement."""

    @staticmethod
    @_fwd32
    def forward(ctx, x):
        _need_hip("Upsample3d2x", x)
        x = x.contiguous()
        N, Cc, D, H, W = x.shape
        out = torch.empty(N, Cc, 2 * D, 2 * H, 2 * W, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().hav_upsample3d_2x_fwd(_p(out), _p(x), N * Cc, D, H, W, _stream()), "hav_upsample3d_2x_fwd")
        ctx.shape = (N, Cc, D, H, W)
        return out

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, g):
        N, Cc, D, H, W = ctx.shape
        g = g.contiguous()
        dx = torch.empty(N, Cc, D, H, W, device=g.device, dtype=torch.float32)
        with torch.cuda.device(g.device):
            _lib.check(_lib.lib().hav_upsample3d_2x_bwd(_p(dx), _p(g), N * Cc, D, H, W, _stream()), "hav_upsample3d_2x_bwd")
        return dx


def upsample3d_2x(x):
    return Upsample3d2x.apply(x)


class Conv3dSmall(Function):
    """nn.Conv3d(kernel 3, padding 1, stride 1) on a small cubic volume [1,C,R,R,R] (R <= 8: the first three layers of VolumeDecoder) as
    matrix products over an explicit patch matrix (hav_im2col3d / hav_col2im3d + three GEMMs): these layers are weight-bound (56 / 14 /
    3.5 MB of filters for 8 / 64 / 512 voxels) and MIOpen / CK take 350 / 200 / 115 us for their forward alone."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, w, b):
        _need_hip("Conv3dSmall", x, w)
        x, w = x.contiguous(), w.contiguous()
        _, Cc, R = x.shape[:3]
        Cout = w.shape[0]
        col = torch.empty(27 * Cc, R ** 3, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().hav_im2col3d(_p(col), _p(x), Cc, R, _stream()), "hav_im2col3d")
        w2 = w.view(Cout, 27 * Cc)
        y = torch.mm(w2, col) if b is None else torch.addmm(b.view(-1, 1), w2, col)
        ctx.save_for_backward(col, w)
        ctx.shape, ctx.has_bias = (Cc, R), b is not None
        return y.view(1, Cout, R, R, R)

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, g):
        col, w = ctx.saved_tensors
        Cc, R = ctx.shape
        Cout = w.shape[0]
        g2 = g.contiguous().view(Cout, R ** 3)
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dw = torch.mm(g2, col.t()).view_as(w)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g2.sum(1)
        if ctx.needs_input_grad[0]:
            dcol = torch.mm(w.view(Cout, 27 * Cc).t(), g2)
            dx = torch.empty(1, Cc, R, R, R, device=g.device, dtype=torch.float32)
            with torch.cuda.device(g.device):
                _lib.check(_lib.lib().hav_col2im3d(_p(dx), _p(dcol), Cc, R, _stream()), "hav_col2im3d")
        return dx, dw, db


def conv3d_small_eligible(x, conv):
    w, b = conv.weight, conv.bias
    if not (w.is_cuda and w.device == x.device and w.dtype == torch.float32 and (b is None or (b.dtype == torch.float32 and b.device == x.device))
            and getattr(conv, "padding_mode", "zeros") == "zeros"):
        return False          # anything else stays on nn.Conv3d (a non-fp32 weight made Conv3dSmall raise instead of falling back)
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.shape[0] == 1 and x.shape[2] == x.shape[3] == x.shape[4] and x.shape[2] <= 8
            and tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.padding) == (1, 1, 1) and tuple(conv.stride) == (1, 1, 1)
            and tuple(conv.dilation) == (1, 1, 1) and conv.groups == 1 and switches.on("HAVATAR_CONV3D_SMALL"))


def conv3d_small(x, conv):
    return Conv3dSmall.apply(x, conv.weight, conv.bias)


_K3_BLOBS = {}          # (weight data pointer, transposed, stream) -> (weak reference, key, blob)


def _conv3d_k3_blob(w, transposed):
    """The fragment blob of w [Cout,Cin,3,3,3] (hav_conv3d_k3_pack) or of its data gradient's filters (hav_conv3d_k3_pack_t), packed on the
    current stream.  Cached per weight tensor and stream, keyed by data pointer, `_version` and graph.weights_epoch(); never while a stream
    is capturing (the pack has to be part of a captured step: its weights change between replays).  The stream is part of the slot because a
    blob is only ordered behind its pack on the stream that packed it; entries whose weight tensor is gone are dropped at the next pack."""
    import weakref
    from ..graph import weights_epoch
    capturing = torch.cuda.is_current_stream_capturing()
    slot, key = (w.data_ptr(), transposed, torch.cuda.current_stream(w.device).cuda_stream), (w._version, weights_epoch(), w.device)
    hit = _K3_BLOBS.get(slot)
    if not capturing and hit is not None and hit[0]() is w and hit[1] == key:
        return hit[2]
    Cout, Cin = w.shape[:2]
    L = _lib.lib()
    n = int(L.hav_conv3d_k3_packed_bytes(Cin, Cout) if transposed else L.hav_conv3d_k3_packed_bytes(Cout, Cin))
    blob = torch.empty(n, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        fn, name = (L.hav_conv3d_k3_pack_t, "hav_conv3d_k3_pack_t") if transposed else (L.hav_conv3d_k3_pack, "hav_conv3d_k3_pack")
        _lib.check(fn(_p(blob), _p(w), Cout, Cin, 1.0, _stream()), name)
    if not capturing:
        for k in [k for k, v in _K3_BLOBS.items() if v[0]() is None]:
            del _K3_BLOBS[k]
        _K3_BLOBS[slot] = (weakref.ref(w), key, blob)
    return blob


def _conv3d_k3_run(y, x, blob, bias, amax, B, Cin, Cout, D, H, W):
    L = _lib.lib()
    n = int(L.hav_conv3d_k3_scratch_bytes(B, Cin, Cout, D, H, W))
    scratch = torch.empty(n, dtype=torch.uint8, device=x.device) if n else None
    _lib.check(L.hav_conv3d_k3_fwd(_p(y), _p(x), _p(blob), _p(bias), _p(amax), B, Cin, Cout, D, H, W, _p(scratch), _stream()), "hav_conv3d_k3_fwd")


class Conv3dK3(Function):
    """nn.Conv3d(kernel 3, padding 1, stride 1, zeros) on the split-fp16 matrix path (hav_conv3d_k3_*: csrc/hav_conv3d.hip), NCDHW float32
    with no layout transposes: the 16^3 - 64^3 layers of VolumeDecoder.  Both the activations and the gradient go through hav_absmax
    (power-of-two range control); every buffer comes from torch.empty and nothing synchronises, so the node can be captured."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, w, b):
        from .conv import absmax
        _need_hip("Conv3dK3", x, w, b)
        x = x.contiguous()
        wp = w if w.is_contiguous() else w.contiguous()
        B, Cin, D, H, W = x.shape
        Cout = w.shape[0]
        y = torch.empty(B, Cout, D, H, W, device=x.device, dtype=torch.float32)
        x_amax = absmax(x)
        blob = _conv3d_k3_blob(wp.detach() if wp is not w else w, False)
        with torch.cuda.device(x.device):
            _conv3d_k3_run(y, x, blob, b.contiguous() if b is not None else None, x_amax, B, Cin, Cout, D, H, W)
        ctx.save_for_backward(x, w, x_amax)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, g):
        from .conv import absmax
        x, w, x_amax = ctx.saved_tensors
        B, Cin, D, H, W = x.shape
        Cout = w.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = dw = db = None
        if not (need_x or need_w or need_b):
            return None, None, None
        g = g.contiguous()
        g_amax = absmax(g)
        L = _lib.lib()
        with torch.cuda.device(g.device):
            if need_x:
                dx = torch.empty_like(x)
                _conv3d_k3_run(dx, g, _conv3d_k3_blob(w if w.is_contiguous() else w.contiguous(), True), None, g_amax, B, Cout, Cin, D, H, W)
            if need_w or need_b:
                dw = torch.empty(Cout, Cin, 3, 3, 3, device=g.device, dtype=torch.float32) if need_w else None          # None: bias sums alone
                db = torch.empty(Cout, device=g.device, dtype=torch.float32) if need_b else None
                scratch = torch.empty(int(L.hav_conv3d_k3_wgrad_scratch_bytes(B, Cin, Cout, D, H, W)), dtype=torch.uint8, device=g.device)
                _lib.check(L.hav_conv3d_k3_wgrad(_p(dw), _p(db), _p(g), _p(x), _p(scratch), _p(g_amax), _p(x_amax), B, Cin, Cout, D, H, W,
                                                 _stream()), "hav_conv3d_k3_wgrad")
        return dx, dw, db


def conv3d_k3_eligible(x, conv):
    """The parameter checks of conv3d_small_eligible plus the shape constraints of hav_conv3d_k3_* (include/havatar.h): Cin, Cout in
    {16, 32, 64, 128}, W % 16 == 0, 32-bit offsets inside one sample."""
    w, b = conv.weight, conv.bias
    if not (w.is_cuda and w.device == x.device and w.dtype == torch.float32 and (b is None or (b.dtype == torch.float32 and b.device == x.device))
            and getattr(conv, "padding_mode", "zeros") == "zeros"):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and w.dim() == 5
            and tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.padding) == (1, 1, 1) and tuple(conv.stride) == (1, 1, 1)
            and tuple(conv.dilation) == (1, 1, 1) and conv.groups == 1):
        return False
    B, Cin, D, H, W = x.shape
    Cout = w.shape[0]
    return (w.shape[1] == Cin and Cin in (16, 32, 64, 128) and Cout in (16, 32, 64, 128) and W >= 16 and W % 16 == 0 and D >= 1 and H >= 1
            and 1 <= B <= 65535 and max(Cin, Cout) * D * H * W < 2 ** 31)


def conv3d_k3(x, conv):
    return Conv3dK3.apply(x, conv.weight, conv.bias)


class InormRelu3d(Function):
    """relu(nn.InstanceNorm3d(affine=False, track_running_stats=False)(y)) as one node (hav_inorm_relu_*: csrc/hav_decoder.hip): ordered fp32
    statistics (per-chunk mean and M2, merged by the parallel-variance formula), no float atomics, planes of the large layers cut over
    several workgroups.  Saves y and the per-plane mu, rstd; every buffer (scratch included) comes from torch.empty and nothing
    synchronises, so the node can be captured."""

    @staticmethod
    @_fwd32
    def forward(ctx, y, eps):
        _need_hip("InormRelu3d", y)
        y = y.contiguous()
        NC, V = y.shape[0] * y.shape[1], y.shape[2] * y.shape[3] * y.shape[4]
        z = torch.empty_like(y)
        stats = torch.empty(2, NC, device=y.device, dtype=torch.float32)
        L = _lib.lib()
        with torch.cuda.device(y.device):
            n = int(L.hav_inorm_relu_scratch_bytes(NC, V))
            scratch = torch.empty(n, dtype=torch.uint8, device=y.device) if n else None
            _lib.check(L.hav_inorm_relu_fwd(_p(z), _p(stats[0]), _p(stats[1]), _p(y), NC, V, float(eps), _p(scratch), _stream()), "hav_inorm_relu_fwd")
        ctx.save_for_backward(y, stats)
        return z

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, dz):
        y, stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        NC, V = y.shape[0] * y.shape[1], y.shape[2] * y.shape[3] * y.shape[4]
        dz = dz.contiguous()
        dy = torch.empty_like(y)
        L = _lib.lib()
        with torch.cuda.device(y.device):
            n = int(L.hav_inorm_relu_scratch_bytes(NC, V))
            scratch = torch.empty(n, dtype=torch.uint8, device=y.device) if n else None
            _lib.check(L.hav_inorm_relu_bwd(_p(dy), _p(dz), _p(y), _p(stats[0]), _p(stats[1]), NC, V, _p(scratch), _stream()), "hav_inorm_relu_bwd")
        return dy, None


def inorm_relu3d_eligible(y, norm):
    """A HIP float32 5-D tensor through an InstanceNorm3d without affine parameters and without running statistics, planes of at least
    two voxels (with one voxel PyTorch raises in training, and the fallback keeps doing so)."""
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 5):
        return False
    if not isinstance(norm, torch.nn.InstanceNorm3d) or norm.affine or norm.track_running_stats:
        return False
    if norm.weight is not None or norm.bias is not None or getattr(norm, "running_mean", None) is not None:
        return False
    NC, V = y.shape[0] * y.shape[1], y.shape[2] * y.shape[3] * y.shape[4]
    return 1 <= NC < 2 ** 31 and 2 <= V < 2 ** 31


def inorm_relu3d(y, eps=1e-5):
    """y [B,C,D,H,W] -> relu(instance_norm(y)), biased variance."""
    return InormRelu3d.apply(y, eps)


FINAL_CONV_MAX_CIN = 64          # FC_MAXC of csrc/hav_decoder.hip: the 27 Cin weights sit in LDS


class FinalConvSigmoid(Function):
    """cat([s, 1 - s], 1), s = sigmoid(nn.Conv3d(Cin, 1, 3, padding 1)(x)), as one node (hav_final_conv_sigmoid_*: csrc/hav_decoder.hip):
    direct fp32 arithmetic, NCDHW.  Saves x, w and the volume; dx, dw and db come from one call, each only if wanted.  Capturable like
    Conv3dK3."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, w, b):
        _need_hip("FinalConvSigmoid", x, w, b)
        x, w = x.contiguous(), w.contiguous()
        B, Cin, D, H, W = x.shape
        vol = torch.empty(B, 2, D, H, W, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().hav_final_conv_sigmoid_fwd(_p(vol), _p(x), _p(w), _p(b.contiguous() if b is not None else None), B, Cin, w.shape[0],
                                                             D, H, W, _stream()), "hav_final_conv_sigmoid_fwd")
        ctx.save_for_backward(x, w, vol)
        ctx.has_bias = b is not None
        return vol

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, dvol):
        x, w, vol = ctx.saved_tensors
        B, Cin, D, H, W = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None
        dvol = dvol.contiguous()
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty(1, device=x.device, dtype=torch.float32) if need_b else None
        L = _lib.lib()
        with torch.cuda.device(x.device):
            scratch = torch.empty(int(L.hav_final_conv_sigmoid_bwd_scratch_bytes(B, Cin, 1, D, H, W)), dtype=torch.uint8, device=x.device)
            _lib.check(L.hav_final_conv_sigmoid_bwd(_p(dx), _p(dw), _p(db), _p(dvol), _p(vol), _p(x), _p(w), _p(scratch), B, Cin, 1, D, H, W,
                                                    _stream()), "hav_final_conv_sigmoid_bwd")
        return dx, dw, db


def final_conv_sigmoid_eligible(x, conv):
    """The parameter checks of conv3d_k3_eligible with one output channel, Cin <= FINAL_CONV_MAX_CIN and 32-bit offsets inside one sample
    (any D, H, W >= 1)."""
    w, b = conv.weight, conv.bias
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5):
        return False
    if not (w.is_cuda and w.device == x.device and w.dtype == torch.float32 and (b is None or (b.dtype == torch.float32 and b.device == x.device))
            and getattr(conv, "padding_mode", "zeros") == "zeros"):
        return False
    if not (w.dim() == 5 and tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.padding) == (1, 1, 1) and tuple(conv.stride) == (1, 1, 1)
            and tuple(conv.dilation) == (1, 1, 1) and conv.groups == 1):
        return False
    B, Cin, D, H, W = x.shape
    return (w.shape[0] == 1 and w.shape[1] == Cin and 1 <= Cin <= FINAL_CONV_MAX_CIN and B >= 1 and D >= 1 and H >= 1 and W >= 1
            and max(Cin, 2, B) * D * H * W < 2 ** 31)


def final_conv_sigmoid(x, conv):
    """x [B,Cin,D,H,W] -> [B,2,D,H,W] = cat([s, 1 - s], 1), s = sigmoid(conv(x))."""
    return FinalConvSigmoid.apply(x, conv.weight, conv.bias)


class Demod(Function):
    """d [B,Cout] = rsqrt(sum_i s[b,i]^2 * scale^2 sum_k W[o,i,k]^2 + eps): the demodulation factors of a ModulatedConv2d
    (reference model/styleUnet.py:214-227, factored form) as one autograd node -- two launches each way (hav_demod_fwd / _bwd)
    instead of ~8 + ~14 ATen launches, three of which stream the whole weight tensor."""

    @staticmethod
    @_fwd32
    def forward(ctx, s, W, scale, eps):
        _need_hip("Demod", s, W)
        s, W = s.contiguous(), W.contiguous()
        B, Cin = s.shape
        Cout, KK = W.shape[0], W.shape[2] * W.shape[3]
        d = torch.empty(B, Cout, device=s.device, dtype=torch.float32)
        q = torch.empty(Cin, Cout, device=s.device, dtype=torch.float32)
        with torch.cuda.device(s.device):
            _lib.check(_lib.lib().hav_demod_fwd(_p(d), _p(q), _p(s), _p(W), float(scale), float(eps), B, Cin, Cout, KK, _stream()), "hav_demod_fwd")
        ctx.save_for_backward(s, W, d, q)
        ctx.scale, ctx.eps = float(scale), float(eps)
        return d

    @staticmethod
    @_bwd32
    def backward(ctx, gd):
        s, W, d, q = ctx.saved_tensors
        if torch.is_grad_enabled():
            # create_graph=True (path-length regulariser through the generator, reference utils/styleUnet_util.py:92): restate the node
            # with ATen under autograd so that the second-order graph exists
            with torch.enable_grad():
                wsq = (ctx.scale * W).pow(2).sum((2, 3)).t()
                dd = torch.rsqrt(torch.matmul(s * s, wsq) + ctx.eps)
                need = [t for t, n in zip((s, W), ctx.needs_input_grad[:2]) if n and t.requires_grad]
                got = iter(torch.autograd.grad(dd, need, gd, create_graph=True) if need else ())
            return tuple(next(got) if (n and t.requires_grad) else None for t, n in zip((s, W), ctx.needs_input_grad[:2])) + (None, None)
        B, Cin = s.shape
        Cout, KK = W.shape[0], W.shape[2] * W.shape[3]
        gs, gW, gq = torch.empty_like(s), torch.empty_like(W), torch.empty_like(q)
        with torch.cuda.device(s.device):
            _lib.check(_lib.lib().hav_demod_bwd(_p(gs), _p(gW), _p(gq), _p(gd.contiguous()), _p(s), _p(d), _p(q), _p(W), ctx.scale, B, Cin, Cout,
                                                KK, _stream()), "hav_demod_bwd")
        return gs, gW, None, None


def demod(s, W, scale, eps=1e-8):
    """s [B,Cin] (differentiable), W [Cout,Cin,k,k] raw parameter -> d [B,Cout]."""
    return Demod.apply(s, W, scale, eps)


# ------------------------------------------------------------------------------------------------------------------------------
# The wavelet nodes of stage two under autograd (HAVATAR_HAAR_TRAIN=1).  All four maps are linear, so each backward is the PARTNER node's
# forward, called through its apply(): the graph stays differentiable to any order with no ATen restatement.  Which bank the adjoint
# takes follows from the kernels' definitions (include/havatar.h; upfirdn2d applies its kernel flipped):
#   dwt_k   : out_band[y, x]    = sum_{i,j} in[2y + i, 2x + j] k_band[1 - i, 1 - j]
#   idwt_k  : out[2y + i, 2x + j] = sum_band in_band[y, x] k_band[i, j]
# so <dwt_k x, g> = sum in[2y+i, 2x+j] g_band[y, x] k_band[1-i, 1-j] = <x, idwt_flip(k) g>, and likewise idwt_k^T = dwt_flip(k), with
# flip = both axes of every 2x2 kernel reversed (for the Haar banks: flip(ll, lh, hl, hh) = (ll, -lh, -hl, hh), the other module's bank).
# The FIR stages: up_f (up 2, pad (2, 1)) has out[Y] = sum_y x[y] f[1 + Y - 2y] and down_f (down 2, pad (1, 1)) has out[y] = sum_Y
# x[Y] f[2 + 2y - Y] per axis, so up_f^T = down_flip(f) and down_f^T = up_flip(f).  Composed:
#   up2(ki, f, kd)^T          = down2(flip kd, flip f, flip ki, 1) = down2(flip kd, flip f / 4, flip ki, 4)
#   down2(ki, f, kd, s)^T     = up2(flip kd, s flip f, flip ki)
# (the / 4 and * 4 are exact; they keep the decimating FIR at Downsample's gain-free size, whatever order of differentiation).
# tests/test_haar_train_gpu.py asserts every one of these through <A x, y> = <x, A^T y> in fp64.
_FLIPS = {}


def _flipped(k, mul=1.0):
    """k [..., m, m] with the last two axes reversed, times mul; cached per tensor (banks are module buffers: a handful per network).  A
    miss while a stream is capturing is computed inside the capture and not kept (its memory belongs to the graph's pool); the warm-up
    that precedes a capture fills the cache, so a captured step reads the kept tensors"""
    slot = (k.data_ptr(), k._version, str(k.device), tuple(k.shape), tuple(k.stride()), float(mul))
    hit = _FLIPS.get(slot)
    if hit is not None:          # (same memory, same layout, same version: the same values, whichever tensor object names them)
        return hit[1]
    with torch.no_grad():
        out = k.flip(-2, -1)
        out = (out * mul if mul != 1.0 else out).contiguous()
    if not torch.cuda.is_current_stream_capturing():
        if len(_FLIPS) >= 256:
            _FLIPS.clear()
        _FLIPS[slot] = (k, out)          # (the source is kept alive: its memory cannot be handed to another tensor while the entry stands)
    return out


def haar_enabled():
    """HAVATAR_HAAR_TRAIN=1 (read at the call): the wavelet transforms of both stage-two networks run as one-launch autograd nodes"""
    return switches.off("HAVATAR_HAAR_TRAIN")


def _haar_tensor(x):
    """a 4-D HIP float32 tensor whose planes start on 16-byte boundaries once contiguous (the existing kernels' float4 accesses)"""
    return bool(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and (not x.is_contiguous() or x.data_ptr() % 16 == 0))


def haar_dwt_eligible(x):
    """[B,C,H,W] HIP float32 with H even and W % 8 == 0 (hav_haar_dwt; its adjoint hav_haar_idwt then sees W/2 % 4 == 0)"""
    return _haar_tensor(x) and x.shape[2] >= 2 and x.shape[2] % 2 == 0 and x.shape[3] >= 8 and x.shape[3] % 8 == 0 and x.shape[1] >= 1


def haar_idwt_eligible(x):
    """[B,4C,H,W] HIP float32 with W % 4 == 0 (hav_haar_idwt; its adjoint hav_haar_dwt then sees 2H even and 2W % 8 == 0)"""
    return _haar_tensor(x) and x.shape[1] >= 4 and x.shape[1] % 4 == 0 and x.shape[2] >= 1 and x.shape[3] >= 4 and x.shape[3] % 4 == 0


def haar_up2_eligible(x, fir):
    """[B,4C,H,W] HIP float32 with W even and a 4x4 FIR (hav_haar_up2; its adjoint hav_haar_down2 sees 2H, 2W: even)"""
    return (_haar_tensor(x) and x.shape[1] >= 4 and x.shape[1] % 4 == 0 and x.shape[2] >= 1 and x.shape[3] >= 2 and x.shape[3] % 2 == 0
            and tuple(fir.shape) == (4, 4))


def haar_down2_eligible(x, fir):
    """[B,4C,H,W] HIP float32 with H and W even and a 4x4 FIR (hav_haar_down2), and W % 4 == 0 so that its adjoint hav_haar_up2 sees an
    even width"""
    return (_haar_tensor(x) and x.shape[1] >= 4 and x.shape[1] % 4 == 0 and x.shape[2] >= 2 and x.shape[2] % 2 == 0 and x.shape[3] >= 4
            and x.shape[3] % 4 == 0 and tuple(fir.shape) == (4, 4))


def haar_down2_raw(x, ki4, fir, kd4, scale=1.0):
    """scale * dwt(upfirdn2d(iwt(x), fir, down 2, pad (1, 1))) as one launch (hav_haar_down2), no autograd: x [B,4C,H,W] -> [B,4C,H/2,W/2].
    Raises on anything but HIP float32 tensors; returns None where the library refuses the shape (odd H or W)."""
    _need_hip("haar_down2", x, ki4, fir, kd4)
    if x.dim() != 4 or x.shape[1] % 4 or x.shape[1] < 4 or tuple(fir.shape) != (4, 4) or ki4.numel() != 16 or kd4.numel() != 16:
        return None
    B, Cc, H, W = x.shape
    if H < 1 or W < 1 or H % 2 or W % 2:
        return None
    x, ki4, fir, kd4 = x.contiguous(), ki4.contiguous(), fir.contiguous(), kd4.contiguous()
    out = torch.empty(B, Cc, H // 2, W // 2, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        rc = _lib.lib().hav_haar_down2(_p(out), _p(x), _p(ki4), _p(fir), _p(kd4), float(scale), B, Cc // 4, H, W, _stream())
    if rc == -2:          # HAV_EUNSUP
        return None
    _lib.check(rc, "hav_haar_down2")
    return out


def _haar_call(name, x, k4, inverse):
    from . import fused
    out = fused.haar(x, k4, inverse=inverse)
    if out is None:
        raise RuntimeError(name + ": shape not taken (check *_eligible first)")
    return out


class HaarDwt(Function):
    """HaarTransform as one launch under autograd (hav_haar_dwt): x [B,C,H,W] -> [B,4C,H/2,W/2]; backward = HaarIdwt with the flipped bank."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, k4):
        _need_hip("HaarDwt", x, k4)
        ctx.save_for_backward(k4)
        return _haar_call("HaarDwt", x, k4, False)

    @staticmethod
    @_bwd32
    def backward(ctx, g):
        k4, = ctx.saved_tensors
        return (HaarIdwt.apply(g.contiguous(), _flipped(k4)) if ctx.needs_input_grad[0] else None), None


class HaarIdwt(Function):
    """InverseHaarTransform as one launch under autograd (hav_haar_idwt): x [B,4C,H,W] -> [B,C,2H,2W]; backward = HaarDwt with the flipped bank."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, k4):
        _need_hip("HaarIdwt", x, k4)
        ctx.save_for_backward(k4)
        return _haar_call("HaarIdwt", x, k4, True)

    @staticmethod
    @_bwd32
    def backward(ctx, g):
        k4, = ctx.saved_tensors
        return (HaarDwt.apply(g.contiguous(), _flipped(k4)) if ctx.needs_input_grad[0] else None), None


class HaarUp2(Function):
    """ToRGB's skip path dwt(upsample(iwt(x))) as one launch under autograd (hav_haar_up2): [B,4C,H,W] -> [B,4C,2H,2W]; backward =
    HaarDown2 with the flipped banks, FIR / 4 and scale 4."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, ki4, fir, kd4):
        from . import fused
        _need_hip("HaarUp2", x, ki4, fir, kd4)
        out = fused.haar_up2(x, ki4, fir, kd4)
        if out is None:
            raise RuntimeError("HaarUp2: shape not taken (check haar_up2_eligible first)")
        ctx.save_for_backward(ki4, fir, kd4)
        return out

    @staticmethod
    @_bwd32
    def backward(ctx, g):
        ki4, fir, kd4 = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return HaarDown2.apply(g.contiguous(), _flipped(kd4), _flipped(fir, 0.25), _flipped(ki4), 4.0), None, None, None


class HaarDown2(Function):
    """FromRGB's wavelet-domain down-sampling scale * dwt(downsample(iwt(x))) as one launch under autograd (hav_haar_down2): [B,4C,H,W] ->
    [B,4C,H/2,W/2]; backward = HaarUp2 with the flipped banks and scale * FIR."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, ki4, fir, kd4, scale):
        out = haar_down2_raw(x, ki4, fir, kd4, scale)
        if out is None:
            raise RuntimeError("HaarDown2: shape not taken (check haar_down2_eligible first)")
        ctx.save_for_backward(ki4, fir, kd4)
        ctx.scale = float(scale)
        return out

    @staticmethod
    @_bwd32
    def backward(ctx, g):
        ki4, fir, kd4 = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return HaarUp2.apply(g.contiguous(), _flipped(kd4), _flipped(fir, ctx.scale), _flipped(ki4)), None, None, None, None


def haar_dwt(x, k4):
    """HaarDwt where the shape is eligible, else None (the caller keeps its statement); anything but HIP float32 tensors raises"""
    _need_hip("haar_dwt", x, k4)
    return HaarDwt.apply(x.contiguous(), k4) if haar_dwt_eligible(x) else None


def haar_idwt(x, k4):
    _need_hip("haar_idwt", x, k4)
    return HaarIdwt.apply(x.contiguous(), k4) if haar_idwt_eligible(x) else None


def haar_up2(x, ki4, fir, kd4):
    _need_hip("haar_up2", x, ki4, fir, kd4)
    return HaarUp2.apply(x.contiguous(), ki4, fir, kd4) if haar_up2_eligible(x, fir) else None


def haar_down2(x, ki4, fir, kd4, scale=1.0):
    _need_hip("haar_down2", x, ki4, fir, kd4)
    return HaarDown2.apply(x.contiguous(), ki4, fir, kd4, float(scale)) if haar_down2_eligible(x, fir) else None


# ---------------------------------------------------------------------------------------------------------------------------------------
# The image-space losses of the stage-two joint step (hav_s2_image_loss_*: csrc/hav_s2_loss.hip; reference train_avatarHD.py:246-283)
# ---------------------------------------------------------------------------------------------------------------------------------------
def s2_loss_enabled():
    """harness/train_hd.py::joint_step takes Stage2ImageLoss for its image-space losses where the tensors are eligible (the default: the node is
    faster than the statement at both measured sizes); HAVATAR_S2_LOSS=0 selects the ATen statement.  Read at the call."""
    return switches.on("HAVATAR_S2_LOSS")


def stage2_image_loss_statement(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask, rgb_loss="mse"):
    """The reference's statements (train_avatarHD.py:246-247, :251, :268, :282-283) ->
    (rgb_loss, hr_l1, mask_bce, lr_mse.detach(), sr_mse.detach()); mask_bce is unweighted."""
    F = torch.nn.functional
    G = gt_lr_img.shape[-1]
    lr_img = F.interpolate(render[:, :3], size=(G, G), mode="bilinear", align_corners=True)
    rgb = (F.mse_loss if rgb_loss == "mse" else F.l1_loss)(lr_img, gt_lr_img)
    bce = F.binary_cross_entropy(mask.clip(1e-3, 1.0 - 1e-3), gt_lr_mask)
    hr_l1 = F.l1_loss(fake_img, gt_hr_img)
    return rgb, hr_l1, bce, F.mse_loss(lr_img, gt_lr_img).detach(), F.mse_loss(fake_img, gt_hr_img).detach()


def stage2_image_loss_eligible(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask):
    """Float32 HIP tensors, render [B,C>=3,r,r] (any strides), mask / gt_lr_mask [B,1,r,r], the three images [B,3,G,G], 2 <= r <= G,
    grad mode on.  (No cap on G / r: the backward's gather walks (2 (G - 1) / (r - 1) + 4)^2 pixels per low-resolution element, serially --
    measured at G / r = 4; see the cost note in csrc/hav_s2_loss.hip before using it at ratios far above that.)"""
    ts = (render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask)
    if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in ts):
        return False
    if not torch.is_grad_enabled():
        return False
    B, Cc, r, r2 = render.shape
    G = gt_lr_img.shape[-1]
    if Cc < 3 or r != r2 or not (2 <= r <= G) or B < 1:
        return False
    return (tuple(mask.shape) == tuple(gt_lr_mask.shape) == (B, 1, r, r)
            and tuple(gt_lr_img.shape) == tuple(fake_img.shape) == tuple(gt_hr_img.shape) == (B, 3, G, G))


class Stage2ImageLoss(Function):
    """(rgb3 [B,3,r,r] = render[:, :3] as a strided view, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask, rgb_mse) ->
    (rgb_loss, hr_l1, mask_bce, lr_mse, sr_mse): one pass and a one-workgroup reduction forward, one pass backward, no float atomics either
    way.  lr_img is never written.  First order only.  The narrow view keeps the other C - 3 channels out of the node: autograd's own slice
    backward pads them with exact zeros."""

    @staticmethod
    @_fwd32
    def forward(ctx, rgb3, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask, rgb_mse):
        _need_hip("Stage2ImageLoss", rgb3, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask)
        gt_lr_img, fake_img, gt_hr_img, gt_lr_mask = (t.contiguous() for t in (gt_lr_img, fake_img, gt_hr_img, gt_lr_mask))
        B, _, r, _ = rgb3.shape
        G = gt_lr_img.shape[-1]
        L = _lib.lib()
        out = torch.empty(5, device=rgb3.device, dtype=torch.float32)
        partials = torch.empty(5 * int(L.hav_s2_image_loss_blocks(B, G)), device=rgb3.device, dtype=torch.float64)
        rs, ms = rgb3.stride(), mask.stride()
        with torch.cuda.device(rgb3.device):
            _lib.check(L.hav_s2_image_loss_fwd(_p(out), _p(partials), _p(rgb3), rs[0], rs[1], rs[2], rs[3], _p(mask), ms[0], ms[2], ms[3],
                                               _p(gt_lr_img), _p(fake_img), _p(gt_hr_img), _p(gt_lr_mask), B, r, G, _stream()),
                       "hav_s2_image_loss_fwd")
        ctx.save_for_backward(rgb3, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask)
        ctx.rgb_mse = bool(rgb_mse)
        rgb, hr_l1, bce, lr_mse, sr_mse = out[1 if rgb_mse else 0], out[2], out[4], out[1], out[3]
        ctx.mark_non_differentiable(lr_mse, sr_mse)
        return rgb, hr_l1, bce, lr_mse, sr_mse

    @staticmethod
    @once_differentiable
    @_bwd32
    def backward(ctx, g_rgb, g_hr, g_bce, _g_lr_mse, _g_sr_mse):
        rgb3, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask = ctx.saved_tensors
        need_r, need_m, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if not (need_r or need_m or need_f):
            return (None,) * 7
        B, _, r, _ = rgb3.shape
        G = gt_lr_img.shape[-1]
        zero = rgb3.new_zeros(())
        gup = torch.stack([(g if g is not None else zero).reshape(()).float() for g in (g_rgb, g_hr, g_bce)])
        # grad_render in the layout the render arrives in ([B,r,r,3] permuted): the slice backward copies it into the C-channel gradient
        d_r = torch.empty(B, r, r, 3, device=rgb3.device, dtype=torch.float32).permute(0, 3, 1, 2) if need_r else None
        d_m = torch.empty(B, 1, r, r, device=rgb3.device, dtype=torch.float32) if need_m else None
        d_f = torch.empty_like(fake_img) if need_f else None
        rs, ms = rgb3.stride(), mask.stride()
        gs = d_r.stride() if need_r else (0, 0, 0, 0)
        with torch.cuda.device(rgb3.device):
            _lib.check(_lib.lib().hav_s2_image_loss_bwd(_p(d_f), _p(d_r), gs[0], gs[1], gs[2], gs[3], _p(d_m), _p(gup), _p(rgb3), rs[0], rs[1],
                                                        rs[2], rs[3], _p(mask), ms[0], ms[2], ms[3], _p(gt_lr_img), _p(fake_img), _p(gt_hr_img),
                                                        _p(gt_lr_mask), int(ctx.rgb_mse), B, r, G, _stream()), "hav_s2_image_loss_bwd")
        return d_r, d_m, None, d_f, None, None, None


def stage2_image_loss(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask, rgb_loss="mse", native=None):
    """The five image-space scalars of the joint step.  native=None: Stage2ImageLoss where the tensors are eligible unless HAVATAR_S2_LOSS=0,
    the ATen statement otherwise; native=True insists on the node (anything it does not take raises), native=False on the statement."""
    if native is None:
        native = s2_loss_enabled() and stage2_image_loss_eligible(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask)
    if not native:
        return stage2_image_loss_statement(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask, rgb_loss)
    _need_hip("stage2_image_loss", render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask)
    if not stage2_image_loss_eligible(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask):
        raise RuntimeError("stage2_image_loss: not eligible (float32 HIP tensors, 2 <= r <= G, grad mode on)")
    return Stage2ImageLoss.apply(render[:, :3], mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask, rgb_loss == "mse")

"""GPU: the skinning-volume decoder's InstanceNorm3d + ReLU node and its output layer (hav_inorm_relu_*, hav_final_conv_sigmoid_*:
csrc/hav_decoder.hip; native/train_ops.py::InormRelu3d, FinalConvSigmoid; opt-in wiring HAVATAR_DECODER=hip in
model/network/voxel_encoder.py), forward and backward.

Truth is the ATen statement in fp64 on the CPU with its autograd -- relu(F.instance_norm(y)) and cat([s, 1 - s], 1) with
s = sigmoid(F.conv3d(x, w, b, padding=1)); the yardstick ("floor") is the same statement in fp32 on the CPU; the bar is the project's
(tests/test_conv3d_gpu.py::_bar): err <= 3 floor + 2e-6 max|truth|.  Every figure goes through helpers.report before its assertion.
References are computed once per case and shared."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HAV_EINVAL, HAV_EUNSUP = -1, -2
EPS = 1e-5
IN_CAP = 4          # workgroups per CU of the norm's capped grids (include/havatar.h)
DECODER_NORM = [(512, 2), (256, 4), (128, 8), (64, 16), (32, 32), (16, 64)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lib():
    from havatar_amd import _lib as m
    return m.lib()


def _bar(tag, got, truth, floor32):
    assert got.shape == truth.shape and torch.isfinite(got).all(), tag
    scale = truth.abs().max().item()
    err = (got.double().cpu() - truth).abs().max().item()
    floor = (floor32.double() - truth).abs().max().item()
    report("decoder_native %s: err/scale %.3e floor/scale %.3e (scale %.3e)" % (tag, err / scale, floor / scale, scale))
    assert err <= 3.0 * floor + 2e-6 * scale, (tag, err / scale, floor / scale)


# ---------------------------------------------------------------------------------------------------------------- the norm
@functools.lru_cache(maxsize=None)
def _norm_case(shape, kind="randn"):
    """{"y", "g"} fp32 on the CPU and per dtype name ("f64" truth, "f32" floor) the tuple (z, dy).  kind: randn; shifted (mean -20,
    sigma 3); init (1e-3 randn + 1e-3: variance below eps); const0 (plane 0 is the constant 3); zerog0 (plane 0's upstream gradient is 0)"""
    gen = torch.Generator().manual_seed(sum(shape) * 7 + len(kind))
    y = torch.randn(*shape, generator=gen)
    g = torch.randn(*shape, generator=gen)
    if kind == "shifted":
        y = y * 3.0 - 20.0
    elif kind == "init":
        y = y * 1e-3 + 1e-3
    elif kind == "const0":
        y[0, 0] = 3.0
    elif kind == "zerog0":
        g[0, 0] = 0.0
    out = {"y": y, "g": g}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        yy = y.to(dt).requires_grad_(True)
        z = torch.relu(F.instance_norm(yy, eps=EPS))
        dy, = torch.autograd.grad(z, yy, g.to(dt))
        out[name] = (z.detach(), dy)
    return out


def _norm_run(case):
    from havatar_amd.native import train_ops
    y = case["y"].to(DEV).requires_grad_(True)
    assert train_ops.inorm_relu3d_eligible(y, torch.nn.InstanceNorm3d(y.shape[1]))
    z = train_ops.inorm_relu3d(y, EPS)
    dy, = torch.autograd.grad(z, y, case["g"].to(DEV))
    return z.detach(), dy


def _norm_check(tag, shape, kind="randn", first_plane=0):
    """z and dy of the case against the bar, over the planes [:, first_plane:] (the constant plane is left to its caller: fp32 ATen itself
    returns dy of the order of 1e3 there, which would make the floor meaningless for the others)"""
    case = _norm_case(shape, kind)
    z, dy = _norm_run(case)
    assert torch.isfinite(z).all() and torch.isfinite(dy).all(), tag
    cut = lambda t: t[:, first_plane:]
    _bar(tag + " z", cut(z), cut(case["f64"][0]), cut(case["f32"][0]))
    _bar(tag + " dy", cut(dy), cut(case["f64"][1]), cut(case["f32"][1]))
    return z, dy


@pytest.mark.parametrize("C_,R", DECODER_NORM)
def test_norm_decoder_shapes(C_, R):
    """The six planes-by-voxels shapes of VolumeDecoder(1024, 64): 512 planes of 8 voxels (one wave each) up to 16 planes of 64^3 (cut)."""
    _norm_check("norm %dx%d^3" % (C_, R), (1, C_, R, R, R))


@pytest.mark.parametrize("shape,kind", [((2, 5, 3, 5, 7), "randn"), ((1, 3, 1, 1, 5), "randn"), ((1, 4, 40, 33, 31), "shifted"),
                                        ((1, 16, 64, 64, 64), "init")])
def test_norm_odd_planes_shifted_data_and_the_initial_regime(shape, kind):
    """V = 105 (odd: planes are 4-byte aligned, the scalar path) with N = 2; V = 5; four planes of 40 x 33 x 31 voxels with mean -20 and
    sigma 3 (cut, with a ragged last piece: sum(y^2) - mean^2 would lose five digits here); 16 x 64^3 at 1e-3 randn + 1e-3, the decoder's
    regime at initialisation, variance below eps."""
    L = _lib()
    V = shape[2] * shape[3] * shape[4]
    if kind == "shifted":
        chunks = L.hav_inorm_relu_chunks(shape[0] * shape[1], V)
        assert chunks > 1 and V % 1024 != 0, chunks          # pieces are multiples of 1024 voxels: the last one is ragged
    _norm_check("norm %s %s" % ("x".join(map(str, shape)), kind), shape, kind)


@pytest.mark.parametrize("shape", [(1, 3, 4, 4, 4), (1, 2, 32, 32, 32)])
def test_norm_constant_plane_and_zero_upstream_gradient(shape):
    """Plane 0 is the constant 3 (its sums are exact in fp32, so mean = 3 and M2 = 0 exactly): z and dy of that plane are all zero and
    everything is finite.  Separately plane 0's upstream gradient is zero: its dy is zero.  In the single-owner and in the cut form."""
    z, dy = _norm_check("norm const plane %s" % "x".join(map(str, shape)), shape, "const0", first_plane=1)
    assert (z[0, 0] == 0).all() and (dy[0, 0] == 0).all()
    z, dy = _norm_check("norm zero gradient %s" % "x".join(map(str, shape)), shape, "zerog0")
    assert (dy[0, 0] == 0).all() and torch.isfinite(dy).all()


def test_norm_forms():
    """hav_inorm_relu_chunks: 16 planes of 64^3 are cut (and need scratch), 512 planes of 2^3 have a single owner (and need none)."""
    L = _lib()
    assert L.hav_inorm_relu_chunks(16, 64 ** 3) > 1 and L.hav_inorm_relu_scratch_bytes(16, 64 ** 3) > 0
    assert L.hav_inorm_relu_chunks(32, 32 ** 3) > 1
    assert L.hav_inorm_relu_chunks(512, 8) == 1 and L.hav_inorm_relu_scratch_bytes(512, 8) == 0
    assert L.hav_inorm_relu_chunks(64, 16 ** 3) == 1


@pytest.mark.parametrize("form", ["wave", "workgroup", "cut"])
def test_norm_second_grid_trip(form):
    """Every launch of the norm sizes its grid as min(work items, IN_CAP * CUs) and walks the items with a grid stride.  One shape per form,
    chosen from the CU count so that there are more items than workgroups: one-wave owners (4 planes per workgroup), workgroup owners,
    and the cut form (items = planes x pieces; the statistics, the apply pass and both backward passes share that grid)."""
    L = _lib()
    cap = IN_CAP * _cus()
    if form == "wave":
        shape = (1, 4 * cap + 3, 2, 2, 2)
        NC, V = shape[1], 8
        assert L.hav_inorm_relu_chunks(NC, V) == 1 and V <= 256 and (NC + 3) // 4 > cap
    elif form == "workgroup":
        shape = (1, cap + 5, 3, 10, 10)
        NC, V = shape[1], 300
        assert L.hav_inorm_relu_chunks(NC, V) == 1 and V > 256 and NC > cap
    else:
        shape = (1, 16, 64, 64, 64)
        chunks = L.hav_inorm_relu_chunks(16, 64 ** 3)
        assert chunks > 1 and 16 * chunks > cap, (chunks, cap)
    _norm_check("norm second trip %s" % form, shape)


# ---------------------------------------------------------------------------------------------------------------- the output layer
@functools.lru_cache(maxsize=None)
def _final_case(Cin, B, D, H, W, bias):
    """{"x","w","b","g"} fp32 on the CPU and per dtype name the tuple (vol, dx, dw, db or None)"""
    gen = torch.Generator().manual_seed(Cin * 100 + B * 10 + D + (1 if bias else 0))
    x = torch.randn(B, Cin, D, H, W, generator=gen)
    w = torch.randn(1, Cin, 3, 3, 3, generator=gen) / math.sqrt(27 * Cin)
    b = torch.randn(1, generator=gen) * 0.1 if bias else None
    g = torch.randn(B, 2, D, H, W, generator=gen)
    out = {"x": x, "w": w, "b": b, "g": g}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        ps = [t.to(dt).requires_grad_(True) for t in (x, w) + ((b,) if bias else ())]
        s = torch.sigmoid(F.conv3d(ps[0], ps[1], ps[2] if bias else None, padding=1))
        vol = torch.cat([s, 1 - s], 1)
        gr = torch.autograd.grad(vol, ps, g.to(dt))
        out[name] = (vol.detach(), gr[0], gr[1], gr[2] if bias else None)
    return out


def _final_conv(case):
    Cin = case["w"].shape[1]
    conv = torch.nn.Conv3d(Cin, 1, 3, padding=1, bias=case["b"] is not None).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(case["w"])
        if case["b"] is not None:
            conv.bias.copy_(case["b"])
    return conv


def _final_run(case):
    from havatar_amd.native import train_ops
    conv = _final_conv(case)
    x = case["x"].to(DEV).requires_grad_(True)
    assert train_ops.final_conv_sigmoid_eligible(x, conv)
    vol = train_ops.final_conv_sigmoid(x, conv)
    ps = (x, conv.weight) + ((conv.bias,) if conv.bias is not None else ())
    gr = torch.autograd.grad(vol, ps, case["g"].to(DEV))
    return vol.detach(), gr[0], gr[1], gr[2] if conv.bias is not None else None


FINAL_SHAPES = [(16, 1, 64, 64, 64), (32, 1, 32, 32, 32), (16, 1, 3, 5, 7), (16, 2, 3, 5, 7), (5, 1, 4, 4, 4)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("Cin,B,D,H,W", FINAL_SHAPES)
def test_output_layer_forward_and_gradients(Cin, B, D, H, W, bias):
    """vol, dx, dw, db against the bar: the decoder's two output layers (16 channels on 64^3, 32 on 32^3), an odd volume smaller than one
    tile in every direction (4-byte aligned rows, B = 1 and 2) and a channel count that is no multiple of the staging round."""
    case = _final_case(Cin, B, D, H, W, bias)
    t64, t32 = case["f64"], case["f32"]
    tag = "final Cin=%d B=%d %dx%dx%d%s" % (Cin, B, D, H, W, "" if bias else " (no bias)")
    vol, dx, dw, db = _final_run(case)
    _bar(tag + " vol", vol, t64[0], t32[0])
    _bar(tag + " dx", dx, t64[1], t32[1])
    _bar(tag + " dw", dw, t64[2], t32[2])
    if bias:
        _bar(tag + " db", db, t64[3], t32[3])


def test_output_layer_bias_gradient_alone():
    """Only the bias wants a gradient (dx, dw NULL through the C ABI): db has the same bits as in the full backward."""
    from havatar_amd.native import train_ops
    case = _final_case(16, 2, 3, 5, 7, True)
    _, _, _, db = _final_run(case)
    conv = _final_conv(case)
    conv.weight.requires_grad_(False)
    vol = train_ops.final_conv_sigmoid(case["x"].to(DEV), conv)
    db1, = torch.autograd.grad(vol, (conv.bias,), case["g"].to(DEV))
    assert torch.equal(db1, db)
    _bar("final bias alone db", db1, case["f64"][3], case["f32"][3])


def test_output_layer_weight_gradient_second_grid_trip():
    """The weight gradient deals the [4 x 4 x 32]-voxel tiles to ceil(2 CUs / rounds) workgroups per round of four channels; a workgroup walks
    its tiles with a grid stride and keeps the sums in registers.  16 channels on 64^3: 512 tiles, four rounds -- more tiles than
    workgroups."""
    Cin, B, D, H, W = FINAL_SHAPES[0]
    tiles, rounds = B * ((D + 3) // 4) * ((H + 3) // 4) * ((W + 31) // 32), (Cin + 3) // 4
    groups = min(tiles, (2 * _cus() + rounds - 1) // rounds)
    assert tiles > groups, (tiles, groups)
    case = _final_case(Cin, B, D, H, W, True)
    _, _, dw, db = _final_run(case)
    _bar("final second trip dw", dw, case["f64"][2], case["f32"][2])
    _bar("final second trip db", db, case["f64"][3], case["f32"][3])


# ---------------------------------------------------------------------------------------------------------------- both nodes
def test_both_nodes_are_bit_reproducible():
    """Forward and gradients of both nodes, twice from the same inputs: the same bits (no float atomics, every sum in a fixed order).  The
    norm in its three forms."""
    from havatar_amd.native import train_ops
    for shape in [(1, 512, 2, 2, 2), (1, 64, 16, 16, 16), (1, 32, 32, 32, 32)]:
        case = _norm_case(shape)
        a, b = _norm_run(case), _norm_run(case)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), shape
    case = _final_case(32, 1, 32, 32, 32, True)
    a, b = _final_run(case), _final_run(case)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_refusals_through_the_c_abi_leave_outputs_untouched():
    """NULL pointers and V < 2 return HAV_EINVAL, Cin over the bound and Cout != 1 return HAV_EUNSUP, before any launch: NaN-filled outputs
    stay NaN, and the size queries answer 0."""
    L = _lib()
    nan = lambda n: torch.full((n,), float("nan"), device=DEV)
    src = torch.randn(1 << 16, device=DEV)
    scratch = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    z, mu, rs, dy = nan(4096), nan(64), nan(64), nan(4096)
    st = _stream()
    assert L.hav_inorm_relu_fwd(None, _p(mu), _p(rs), _p(src), 4, 64, EPS, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_fwd(_p(z), None, _p(rs), _p(src), 4, 64, EPS, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_fwd(_p(z), _p(mu), _p(rs), None, 4, 64, EPS, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_fwd(_p(z), _p(mu), _p(rs), _p(src), 4, 1, EPS, _p(scratch), st) == HAV_EINVAL          # V < 2
    assert L.hav_inorm_relu_fwd(_p(z), _p(mu), _p(rs), _p(src), 0, 64, EPS, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_fwd(_p(z), _p(mu), _p(rs), _p(src), 2, 8192, EPS, None, st) == HAV_EINVAL               # cut form without scratch
    assert L.hav_inorm_relu_bwd(_p(dy), None, _p(src), _p(src), _p(src), 4, 64, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_bwd(_p(dy), _p(src), _p(src), _p(src), None, 4, 64, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_bwd(_p(dy), _p(src), _p(src), _p(src), _p(src), 4, 1, _p(scratch), st) == HAV_EINVAL
    assert L.hav_inorm_relu_chunks(4, 1) == 0 and L.hav_inorm_relu_scratch_bytes(4, 1) == 0
    vol, dx, dw, db = nan(4096), nan(4096), nan(4096), nan(4)
    fwd, bwd = L.hav_final_conv_sigmoid_fwd, L.hav_final_conv_sigmoid_bwd
    assert fwd(None, _p(src), _p(src), None, 1, 4, 1, 2, 2, 4, st) == HAV_EINVAL
    assert fwd(_p(vol), _p(src), None, None, 1, 4, 1, 2, 2, 4, st) == HAV_EINVAL
    assert fwd(_p(vol), _p(src), _p(src), None, 1, 65, 1, 2, 2, 4, st) == HAV_EUNSUP          # Cin over the bound
    assert fwd(_p(vol), _p(src), _p(src), None, 1, 4, 2, 2, 2, 4, st) == HAV_EUNSUP           # Cout != 1
    assert bwd(_p(dx), _p(dw), _p(db), None, _p(src), _p(src), _p(src), _p(scratch), 1, 4, 1, 2, 2, 4, st) == HAV_EINVAL
    assert bwd(_p(dx), _p(dw), _p(db), _p(src), _p(src), _p(src), _p(src), None, 1, 4, 1, 2, 2, 4, st) == HAV_EINVAL
    assert bwd(None, None, None, _p(src), _p(src), _p(src), _p(src), _p(scratch), 1, 4, 1, 2, 2, 4, st) == HAV_EINVAL
    assert bwd(_p(dx), _p(dw), _p(db), _p(src), _p(src), None, _p(src), _p(scratch), 1, 4, 1, 2, 2, 4, st) == HAV_EINVAL          # dw without x
    assert bwd(_p(dx), _p(dw), _p(db), _p(src), _p(src), _p(src), _p(src), _p(scratch), 1, 65, 1, 2, 2, 4, st) == HAV_EUNSUP
    assert bwd(_p(dx), _p(dw), _p(db), _p(src), _p(src), _p(src), _p(src), _p(scratch), 1, 4, 2, 2, 2, 4, st) == HAV_EUNSUP
    assert L.hav_final_conv_sigmoid_bwd_scratch_bytes(1, 65, 1, 2, 2, 4) == 0 and L.hav_final_conv_sigmoid_bwd_scratch_bytes(1, 4, 2, 2, 2, 4) == 0
    assert L.hav_final_conv_sigmoid_bwd_scratch_bytes(1, 4, 1, 2, 2, 4) > 0
    torch.cuda.synchronize()
    for t in (z, mu, rs, dy, vol, dx, dw, db):
        assert torch.isnan(t).all()


def test_eligibility_functions():
    from havatar_amd.native import train_ops
    y = torch.randn(1, 4, 3, 5, 6, device=DEV)
    norm = lambda **kw: torch.nn.InstanceNorm3d(4, **kw).to(DEV)
    assert train_ops.inorm_relu3d_eligible(y, norm())
    assert not train_ops.inorm_relu3d_eligible(y.half(), norm())
    assert not train_ops.inorm_relu3d_eligible(y.cpu(), norm())
    assert not train_ops.inorm_relu3d_eligible(y, norm(affine=True))
    assert not train_ops.inorm_relu3d_eligible(y, norm(track_running_stats=True))
    assert not train_ops.inorm_relu3d_eligible(y[..., :1, :1, :1], norm())          # V = 1
    assert not train_ops.inorm_relu3d_eligible(y[0], norm())
    x = torch.randn(1, 16, 3, 5, 7, device=DEV)
    mk = lambda cin=16, cout=1, **kw: torch.nn.Conv3d(cin, cout, 3, **{"padding": 1, **kw}).to(DEV)
    assert train_ops.final_conv_sigmoid_eligible(x, mk())
    assert not train_ops.final_conv_sigmoid_eligible(x.half(), mk())
    assert not train_ops.final_conv_sigmoid_eligible(x, mk().half())
    assert not train_ops.final_conv_sigmoid_eligible(x.cpu(), mk())
    assert not train_ops.final_conv_sigmoid_eligible(x, mk().cpu())
    assert not train_ops.final_conv_sigmoid_eligible(x, mk(padding_mode="replicate"))
    assert not train_ops.final_conv_sigmoid_eligible(x, mk(stride=2))
    assert not train_ops.final_conv_sigmoid_eligible(x, mk(cout=2, groups=2))
    assert not train_ops.final_conv_sigmoid_eligible(x, mk(cout=2))
    assert not train_ops.final_conv_sigmoid_eligible(x, mk(dilation=2, padding=2))
    assert not train_ops.final_conv_sigmoid_eligible(torch.randn(1, 65, 2, 2, 4, device=DEV), mk(cin=65))
    assert train_ops.final_conv_sigmoid_eligible(torch.randn(1, 64, 2, 2, 4, device=DEV), mk(cin=64))


def _capture_and_replay(step, fill, outs_of):
    fill()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    for _ in range(2):
        fill()
        graph.replay()
        torch.cuda.synchronize()
        got = [o.detach().clone() for o in outs]
        want = step()
        for a, b in zip(got, want):
            assert torch.equal(a, b.detach())


@pytest.mark.parametrize("node", ["norm_owner", "norm_cut", "final"])
def test_forward_and_backward_capture_in_a_graph(node):
    """Forward + backward of each node inside torch.cuda.graph (warmed up on a side stream first, as graph.py does): two replays with
    refreshed static inputs give the eager results bit for bit -- no host synchronisation, every buffer (scratch included) from
    torch.empty."""
    from havatar_amd.native import train_ops
    gen = torch.Generator().manual_seed(3)
    if node == "final":
        conv = torch.nn.Conv3d(16, 1, 3, padding=1).to(DEV)
        sx = torch.zeros(1, 16, 3, 5, 7, device=DEV, requires_grad=True)
        sg = torch.zeros(1, 2, 3, 5, 7, device=DEV)

        def step():
            vol = train_ops.final_conv_sigmoid(sx, conv)
            return (vol,) + torch.autograd.grad(vol, (sx, conv.weight, conv.bias), sg)
    else:
        shape = (1, 6, 3, 5, 7) if node == "norm_owner" else (1, 2, 8, 32, 32)
        assert (_lib().hav_inorm_relu_chunks(shape[1], shape[2] * shape[3] * shape[4]) > 1) == (node == "norm_cut")
        sx = torch.zeros(*shape, device=DEV, requires_grad=True)
        sg = torch.zeros(*shape, device=DEV)

        def step():
            z = train_ops.inorm_relu3d(sx, EPS)
            return (z,) + torch.autograd.grad(z, (sx,), sg)

    def fill():
        with torch.no_grad():
            sx.copy_(torch.randn(sx.shape, generator=gen))
            sg.copy_(torch.randn(sg.shape, generator=gen))

    _capture_and_replay(step, fill, None)


# ---------------------------------------------------------------------------------------------------------------- the decoder
def _decoder_grads(dec, up):
    vol = dec()
    gr = torch.autograd.grad(vol, list(dec.parameters()), up)
    return vol.detach(), gr


def _count(monkeypatch, train_ops, name, calls):
    real = getattr(train_ops, name)

    def wrapped(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    monkeypatch.setattr(train_ops, name, wrapped)


def test_decoder_route_and_untouched_default(monkeypatch):
    """VolumeDecoder(1024, final_res=32) with HAVATAR_DECODER=hip: exactly five inorm_relu3d calls, one final_conv_sigmoid call and two
    conv3d_k3 calls (the switch implies that route), and the volume and every parameter's gradient are as close to an fp64 CPU copy as
    the default route's, by the bar (floor = the default route's own error on the device, as in tests/test_conv3d_gpu.py).
    With the switch unset: no call, and the same volume bits as with both eligibility functions forced to False -- also with the switch
    set and all three eligibility functions forced to False, which is the per-layer fallback.  With HAVATAR_CONV3D=hip alone: no call
    to the new nodes."""
    from havatar_amd.model.network.voxel_encoder import VolumeDecoder
    from havatar_amd.native import train_ops
    torch.manual_seed(11)
    dec = VolumeDecoder(num_in=1024, final_res=32)
    ref = VolumeDecoder(num_in=1024, final_res=32).double()
    ref.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})
    dec = dec.to(DEV)
    up = torch.randn(1, 2, 32, 32, 32, generator=torch.Generator().manual_seed(12))
    t_vol, t_gr = _decoder_grads(ref, up.double())
    calls = []
    for name in ("inorm_relu3d", "final_conv_sigmoid", "conv3d_k3"):
        _count(monkeypatch, train_ops, name, calls)

    monkeypatch.delenv("HAVATAR_CONV3D", raising=False)
    monkeypatch.delenv("HAVATAR_DECODER", raising=False)
    d_vol, d_gr = _decoder_grads(dec, up.to(DEV))
    assert calls == []
    with monkeypatch.context() as m:
        m.setattr(train_ops, "inorm_relu3d_eligible", lambda y, norm: False)
        m.setattr(train_ops, "final_conv_sigmoid_eligible", lambda x, conv: False)
        o_vol, _ = _decoder_grads(dec, up.to(DEV))
        assert calls == [] and torch.equal(o_vol, d_vol)
        m.setattr(train_ops, "conv3d_k3_eligible", lambda x, conv: False)
        m.setenv("HAVATAR_DECODER", "hip")
        f_vol, _ = _decoder_grads(dec, up.to(DEV))
        assert calls == [] and torch.equal(f_vol, d_vol)

    monkeypatch.setenv("HAVATAR_CONV3D", "hip")
    _decoder_grads(dec, up.to(DEV))
    assert calls == ["conv3d_k3", "conv3d_k3"]
    monkeypatch.delenv("HAVATAR_CONV3D")
    del calls[:]

    monkeypatch.setenv("HAVATAR_DECODER", "hip")
    h_vol, h_gr = _decoder_grads(dec, up.to(DEV))
    assert calls.count("inorm_relu3d") == 5 and calls.count("final_conv_sigmoid") == 1 and calls.count("conv3d_k3") == 2, calls
    names = ["volume"] + [n for n, _ in dec.named_parameters()]
    bad = []
    for name, got, dflt, truth in zip(names, (h_vol,) + tuple(h_gr), (d_vol,) + tuple(d_gr), (t_vol,) + tuple(t_gr)):
        scale = truth.abs().max().item()
        err = (got.double().cpu() - truth).abs().max().item()
        floor = (dflt.double().cpu() - truth).abs().max().item()
        report("decoder HAVATAR_DECODER=hip %s: err %.3e floor %.3e scale %.3e" % (name, err, floor, scale))
        if not (torch.isfinite(got).all() and err <= 3.0 * floor + 2e-6 * scale):
            bad.append((name, err, floor, scale))
    assert not bad, bad


def test_fix_canonical_W_without_grad(monkeypatch):
    """Deformation_Field_new.fix_canonical_W() (the decoder under no_grad-like use: its result is detached) with the switch on: the nodes
    run without a graph, and the frozen volume meets the bar against an fp64 CPU copy, floor = the default route on the device."""
    from havatar_amd.model.Skinning_Field import Deformation_Field_new
    from havatar_amd.native import train_ops
    torch.manual_seed(21)
    opts = {"init_length": 1024, "vol_res": 32}
    net = Deformation_Field_new(options=opts)
    ref = Deformation_Field_new(options=opts).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    net = net.to(DEV)
    calls = []
    for name in ("inorm_relu3d", "final_conv_sigmoid"):
        _count(monkeypatch, train_ops, name, calls)
    with torch.no_grad():
        ref.fix_canonical_W()
        monkeypatch.delenv("HAVATAR_DECODER", raising=False)
        monkeypatch.delenv("HAVATAR_CONV3D", raising=False)
        net.fix_canonical_W()
        dflt = net.canonical_W.clone()
        assert calls == []
        monkeypatch.setenv("HAVATAR_DECODER", "hip")
        net.fix_canonical_W()
    assert calls.count("inorm_relu3d") == 5 and calls.count("final_conv_sigmoid") == 1
    got, truth = net.canonical_W, ref.canonical_W
    assert got.shape == (1, 2, 32, 32, 32) and not got.requires_grad and torch.isfinite(got).all()
    scale = truth.abs().max().item()
    err = (got.double().cpu() - truth).abs().max().item()
    floor = (dflt.double().cpu() - truth).abs().max().item()
    report("fix_canonical_W HAVATAR_DECODER=hip: err %.3e floor %.3e scale %.3e" % (err, floor, scale))
    assert err <= 3.0 * floor + 2e-6 * scale

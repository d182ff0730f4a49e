"""GPU: the native 3x3x3 convolution of the skinning-volume decoder (hav_conv3d_k3_*: csrc/hav_conv3d.hip; native/train_ops.py::Conv3dK3;
opt-in wiring HAVATAR_CONV3D=hip in model/network/voxel_encoder.py) -- forward, data gradient, weight gradient and bias gradient.

Truth is F.conv3d in fp64 on the CPU with its autograd; the yardstick ("floor") is the same statement in fp32; the bar is the project's
one for the split-fp16 convolutions (tests/test_ops_gpu.py): err <= 3 floor + 2e-6 max|truth|, for y, dx, dw and db alike.  Every figure
goes through helpers.report before its assertion.  References are computed once per (shape, scaling) and shared."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HAV_EUNSUP = -2
DECODER = [(128, 64, 16, 16, 16), (64, 32, 32, 32, 32), (32, 16, 64, 64, 64)]
ODD = (16, 16, 3, 5, 16)          # odd depth and height, a single tile row, every border
SLAB = (32, 16, 8, 64, 64)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(shape, B=1, gscale=1.0, xscale=1.0):
    """Inputs of one case and its references: {"x","w","b","g"} fp32 on the CPU, and per dtype name ("f64" truth, "f32" floor) the tuple
    (y with bias, y without bias, dx, dw, db)."""
    Cin, Cout, D, H, W = shape
    gen = torch.Generator().manual_seed(Cin * 1000 + Cout * 10 + D + B)
    x = torch.randn(B, Cin, D, H, W, generator=gen) * xscale
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=gen) / math.sqrt(27 * Cin)
    b = torch.randn(Cout, generator=gen) * 0.1
    g = torch.randn(B, Cout, D, H, W, generator=gen) * gscale
    out = {"x": x, "w": w, "b": b, "g": g}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        xx, ww, bb = (t.to(dt).requires_grad_(True) for t in (x, w, b))
        y = F.conv3d(xx, ww, bb, padding=1)
        dx, dw, db = torch.autograd.grad(y, (xx, ww, bb), g.to(dt))
        with torch.no_grad():
            ynb = F.conv3d(xx, ww, None, padding=1)
        out[name] = tuple(t.detach() for t in (y, ynb, dx, dw, db))
    return out


def _conv(shape, w, b):
    Cin, Cout = shape[:2]
    conv = torch.nn.Conv3d(Cin, Cout, 3, padding=1, bias=b is not None).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        if b is not None:
            conv.bias.copy_(b)
    return conv


def _run(shape, case, bias=True):
    """(y, dx, dw, db) of conv3d_k3 on the device for the case's inputs"""
    from havatar_amd.native import train_ops
    conv = _conv(shape, case["w"], case["b"] if bias else None)
    x = case["x"].to(DEV).requires_grad_(True)
    assert train_ops.conv3d_k3_eligible(x, conv)
    y = train_ops.conv3d_k3(x, conv)
    ps = (x, conv.weight) + ((conv.bias,) if bias else ())
    gr = torch.autograd.grad(y, ps, case["g"].to(DEV))
    return (y.detach(), gr[0], gr[1], gr[2] if bias else None)


def _bar(tag, got, truth, floor32):
    assert got.shape == truth.shape and torch.isfinite(got).all(), tag
    scale = truth.abs().max().item()
    err = (got.double().cpu() - truth).abs().max().item()
    floor = (floor32.double() - truth).abs().max().item()
    report("conv3d_k3 %s: err/scale %.3e floor/scale %.3e (scale %.3e)" % (tag, err / scale, floor / scale, scale))
    assert err <= 3.0 * floor + 2e-6 * scale, (tag, err / scale, floor / scale)


@pytest.mark.parametrize("shape,B", [(s, 1) for s in DECODER] + [(ODD, 1), (ODD, 2), (SLAB, 1)])
def test_layer_shapes_forward_and_gradients(shape, B):
    """conv3d_k3 with and without bias, then dx, dw, db by torch.autograd.grad, each against the bar: the decoder's three large layers,
    a volume with odd depth and height (border masks in every direction, B = 1 and 2) and a slab."""
    case = _case(shape, B)
    t64, t32 = case["f64"], case["f32"]
    tag = "%s B=%d" % ("x".join(map(str, shape)), B)
    y, dx, dw, db = _run(shape, case, bias=True)
    _bar(tag + " y", y, t64[0], t32[0])
    _bar(tag + " dx", dx, t64[2], t32[2])
    _bar(tag + " dw", dw, t64[3], t32[3])
    _bar(tag + " db", db, t64[4], t32[4])
    y0, dx0, dw0, _ = _run(shape, case, bias=False)
    _bar(tag + " y (no bias)", y0, t64[1], t32[1])
    assert torch.equal(dx0, dx) and torch.equal(dw0, dw)          # the bias takes no part in them


@pytest.mark.parametrize("gscale,xscale", [(1e-7, 1.0), (1.0, 1e5)])
def test_range_control_tiny_gradient_and_huge_activation(gscale, xscale):
    """The upstream gradient scaled by 1e-7 (below the fp16 subnormals: it vanishes without the hav_absmax words), and separately x scaled by
    1e5 (past the fp16 maximum: Inf without them): dx and dw meet the same relative bar against their own fp64 truth."""
    case = _case(SLAB, 1, gscale, xscale)
    t64, t32 = case["f64"], case["f32"]
    tag = "%s g*%g x*%g" % ("x".join(map(str, SLAB)), gscale, xscale)
    y, dx, dw, db = _run(SLAB, case, bias=True)
    _bar(tag + " y", y, t64[0], t32[0])
    _bar(tag + " dx", dx, t64[2], t32[2])
    _bar(tag + " dw", dw, t64[3], t32[3])
    _bar(tag + " db", db, t64[4], t32[4])


def test_refusals_leave_outputs_untouched_and_eligibility():
    """Through the C ABI: channel counts outside {16, 32, 64, 128}, W % 16 != 0 and a sample past 32-bit offsets return HAV_EUNSUP from the
    pack, the convolution and the weight gradient, and NaN-filled outputs stay all-NaN.  conv3d_k3_eligible refuses what the node cannot
    take."""
    from havatar_amd import _lib
    from havatar_amd.native import train_ops
    L = _lib.lib()
    nan = lambda n: torch.full((n,), float("nan"), device=DEV)
    src = torch.randn(1 << 16, device=DEV)
    blob = torch.zeros(int(L.hav_conv3d_k3_packed_bytes(128, 128)), dtype=torch.uint8, device=DEV)
    scratch = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    words = torch.zeros(256, dtype=torch.int32, device=DEV)
    for Cin, Cout, D, H, W in [(24, 16, 2, 4, 16), (16, 48, 2, 4, 16), (16, 16, 2, 4, 20), (16, 16, 2, 4, 8), (256, 16, 1, 1, 16),
                               (128, 16, 1 << 10, 1 << 10, 16)]:
        y, gw, gb, pk = nan(4096), nan(4096), nan(64), nan(64)
        assert L.hav_conv3d_k3_fwd(_p(y), _p(src), _p(blob), None, _p(words), 1, Cin, Cout, D, H, W, _p(scratch), _stream()) == HAV_EUNSUP
        assert L.hav_conv3d_k3_fwd(_p(y), _p(src), _p(blob), None, None, 1, Cout, Cin, D, H, W, None, _stream()) == HAV_EUNSUP
        assert L.hav_conv3d_k3_wgrad(_p(gw), _p(gb), _p(src), _p(src), _p(scratch), _p(words), _p(words), 1, Cin, Cout, D, H, W,
                                     _stream()) == HAV_EUNSUP
        assert L.hav_conv3d_k3_scratch_bytes(1, Cin, Cout, D, H, W) == 0 and L.hav_conv3d_k3_wgrad_scratch_bytes(1, Cin, Cout, D, H, W) == 0
        if W == 16 and D * H < 1 << 10:          # the pack sees the channel counts only
            assert L.hav_conv3d_k3_packed_bytes(Cout, Cin) == 0
            assert L.hav_conv3d_k3_pack(_p(pk), _p(src), Cout, Cin, 1.0, _stream()) == HAV_EUNSUP
            assert L.hav_conv3d_k3_pack_t(_p(pk), _p(src), Cout, Cin, 1.0, _stream()) == HAV_EUNSUP
        torch.cuda.synchronize()
        for t in (y, gw, gb, pk):
            assert torch.isnan(t).all()
    x = torch.randn(1, 16, 3, 5, 16, device=DEV)
    mk = lambda **kw: torch.nn.Conv3d(16, 16, 3, **{"padding": 1, **kw}).to(DEV)
    assert train_ops.conv3d_k3_eligible(x, mk())
    assert not train_ops.conv3d_k3_eligible(x, mk().half())
    assert not train_ops.conv3d_k3_eligible(x, mk(padding_mode="replicate"))
    assert not train_ops.conv3d_k3_eligible(x, mk(stride=2))
    assert not train_ops.conv3d_k3_eligible(x, mk(groups=2))
    assert not train_ops.conv3d_k3_eligible(x, mk().cpu())
    assert not train_ops.conv3d_k3_eligible(x, mk(dilation=2, padding=2))
    assert not train_ops.conv3d_k3_eligible(x[..., :8], mk())
    assert not train_ops.conv3d_k3_eligible(x.half(), mk())
    assert not train_ops.conv3d_k3_eligible(torch.randn(1, 24, 3, 5, 16, device=DEV), torch.nn.Conv3d(24, 16, 3, padding=1).to(DEV))


def test_weight_gradient_second_grid_trip():
    """The one launcher that sizes its grid by the CU count is the weight gradient's: its work units (sample, input plane, 16-column strip,
    16-row segment) are dealt to ceil(CUs / output blocks) workgroups, which walk them with a grid stride.  At 32 -> 16 channels on 64^3
    there is one output block and 64 * 4 * 4 = 1024 units: more than workgroups, so every workgroup takes a second unit (with its ring
    of staged rows restarted).  The convolution itself, its finish pass and the two reduce passes launch one thread or workgroup per
    output element / tile: no cap, nothing to reach there."""
    Cin, Cout, D, H, W = DECODER[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = ((Cin + 31) // 32) * ((Cout + 31) // 32)
    units, cap = 1 * D * (W // 16) * ((H + 15) // 16), (cus + blocks - 1) // blocks
    assert units > cap, (units, cap)
    case = _case(DECODER[2], 1)
    _, _, dw, db = _run(DECODER[2], case, bias=True)
    _bar("second trip dw", dw, case["f64"][3], case["f32"][3])
    _bar("second trip db", db, case["f64"][4], case["f32"][4])


def test_gradients_are_bit_reproducible():
    """dx and dw at 64 -> 32 channels on 32^3, twice from the same inputs: the same bits (no float atomics; K-split slices added in a fixed
    order)."""
    from havatar_amd.native import train_ops
    shape = DECODER[1]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(1, shape[0], *shape[2:], generator=gen).to(DEV).requires_grad_(True)
    g = (torch.randn(1, shape[1], *shape[2:], generator=gen) * 1e-4).to(DEV)
    conv = torch.nn.Conv3d(shape[0], shape[1], 3, padding=1).to(DEV)
    runs = []
    for _ in range(2):
        y = train_ops.conv3d_k3(x, conv)
        runs.append((y.detach(),) + torch.autograd.grad(y, (x, conv.weight, conv.bias), g))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_bias_gradient_alone():
    """Only the bias wants a gradient: the weight-gradient kernel is skipped (gw NULL through the C ABI) and db is the same bits as in the
    full backward."""
    from havatar_amd.native import train_ops
    case = _case(ODD, 2)
    _, _, _, db = _run(ODD, case, bias=True)
    conv = _conv(ODD, case["w"], case["b"])
    conv.weight.requires_grad_(False)
    y = train_ops.conv3d_k3(case["x"].to(DEV), conv)
    db1, = torch.autograd.grad(y, (conv.bias,), case["g"].to(DEV))
    assert torch.equal(db1, db)
    _bar("bias alone db", db1, case["f64"][4], case["f32"][4])


def _decoder_grads(dec, up):
    vol = dec()
    gr = torch.autograd.grad(vol, list(dec.parameters()), up)
    return vol.detach(), gr


def test_decoder_opt_in_route_and_untouched_default(monkeypatch):
    """VolumeDecoder(1024, final_res=32): its 16^3 and 32^3 layers take conv3d_k3 with HAVATAR_CONV3D=hip (exactly two calls; the first
    three layers take Conv3dSmall, final_conv stays on nn.Conv3d), and the volume and every parameter's gradient are as close to an fp64
    CPU copy as the default route's, by the bar.  With the variable unset nothing changes: no call, and the same bits as with
    conv3d_k3_eligible forced to False.
    The floor here is the default route's own error on the device, which is large on the weight gradients (0.09-0.36 at scales of 40-130:
    InstanceNorm3d amplifies it), so this test shows the wiring and that the route is no worse than the default; the tight check of the
    arithmetic is test_layer_shapes_forward_and_gradients."""
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
    real = train_ops.conv3d_k3
    monkeypatch.setattr(train_ops, "conv3d_k3", lambda x, conv: (calls.append(tuple(x.shape)), real(x, conv))[1])

    monkeypatch.delenv("HAVATAR_CONV3D", raising=False)
    d_vol, d_gr = _decoder_grads(dec, up.to(DEV))
    assert calls == []
    with monkeypatch.context() as m:
        m.setattr(train_ops, "conv3d_k3_eligible", lambda x, conv: False)
        o_vol, o_gr = _decoder_grads(dec, up.to(DEV))
    assert calls == [] and torch.equal(o_vol, d_vol)

    monkeypatch.setenv("HAVATAR_CONV3D", "hip")
    h_vol, h_gr = _decoder_grads(dec, up.to(DEV))
    assert calls == [(1, 128, 16, 16, 16), (1, 64, 32, 32, 32)]
    names = ["volume"] + [n for n, _ in dec.named_parameters()]
    bad = []
    for name, got, dflt, truth in zip(names, (h_vol,) + tuple(h_gr), (d_vol,) + tuple(d_gr), (t_vol,) + tuple(t_gr)):
        scale = truth.abs().max().item()
        err = (got.double().cpu() - truth).abs().max().item()
        floor = (dflt.double().cpu() - truth).abs().max().item()
        report("decoder HAVATAR_CONV3D=hip %s: err %.3e floor %.3e scale %.3e" % (name, err, floor, scale))
        if not (torch.isfinite(got).all() and err <= 3.0 * floor + 2e-6 * scale):
            bad.append((name, err, floor, scale))
    assert not bad, bad


def test_forward_and_backward_capture_in_a_graph():
    """One conv3d_k3 call, forward + backward, inside torch.cuda.graph (warmed up on a side stream first, as graph.py does): two replays
    with refreshed static inputs give the eager results bit for bit -- no host synchronisation, every buffer from torch.empty, and the
    weight blobs packed inside the captured region."""
    from havatar_amd.native import train_ops
    Cin, Cout, D, H, W = ODD
    gen = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv3d(Cin, Cout, 3, padding=1).to(DEV)
    sx = torch.zeros(1, Cin, D, H, W, device=DEV, requires_grad=True)
    sg = torch.zeros(1, Cout, D, H, W, device=DEV)

    def step():
        y = train_ops.conv3d_k3(sx, conv)
        return (y,) + torch.autograd.grad(y, (sx, conv.weight, conv.bias), sg)

    def fill():
        with torch.no_grad():
            sx.copy_(torch.randn(sx.shape, generator=gen))
            sg.copy_(torch.randn(sg.shape, generator=gen) * 1e-3)

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

"""GPU: the LPIPS head kernels (csrc/hav_lpips.hip), the frozen conv + ReLU node and the whole module (model/lpips.py on native/lpips_ops.py)
against float64 on the device, with ATen float32 as the yardstick: e_native <= max(FACTOR * e_aten, 4e-6), errors relative to the largest
entry of the float64 result (the rule of tests/test_ops_gpu.py; FACTOR = 2).  Inputs come from tests/lpips_util.py's host generator.

Every figure is printed before it is asserted (pytest -s shows them).

Kinks and the whole module's gradient.  With about 1e7 activations per pass, about one ReLU unit or max-pool pair per run sits within float32
rounding of its kink, and two float32 evaluations may put it on different sides.  The value does not notice; the gradient changes over that
unit's whole receptive field -- for a unit of slices 4 / 5 several per cent of in0's elements, by 1e-4 .. 4e-2 of the largest entry.  Measured
(ATen float32 on the CPU against float64, image seeds 11 .. 18, largest error at 1x3x128x256 / 2x3x64x128): 3.7e-2 / 3.6e-6, 3.8e-2 / 3.6e-6,
2.6e-2 / 3.4e-6, 3.9e-3 / 3.6e-6, 2.4e-2 / 1.1e-3, 1.3e-2 / 2.2e-2, 3.7e-6 / 2.5e-4, 3.6e-6 / 3.7e-6: ATen itself is kink-free at both sizes for
one seed in eight, and 3.6e-6 .. 3.8e-6 wherever it is.  The native route flips its own: for the pair of seed 18 it is 8.7e-3 / 1.3e-4 at most with
3.0e-3 / 8.1e-3 of the elements outside the bar (median 5.8e-7 / 5.3e-7); for the pair of seed 11 it is 4.9e-6 / 5.0e-6 with no element outside
(median 6.0e-7 / 5.6e-7) while ATen flips one at 1x3x128x256 on the CPU and on the device alike.  The allowance of 1e-3 of the elements absorbs a
flip in slices 1 .. 3, not one deeper.  The test therefore runs the pair of seed 11, on which the native route flips none, and caps ATen's figure
at its kink-free value; the median, asserted as well, is kink-proof at any seed.  A failure of the share after a change of arithmetic means
"look at where the elements outside lie" (one receptive field = a kink) before it means a wrong kernel; a wrong kernel moves the median.
The joint-step test runs the driver once on the CPU in float64 (the reference the comparison is defined against): about a minute.
Measured figures: DESIGN.md 7.8."""
import os

import pytest
import torch
import torch.nn.functional as F

import lpips_util as lu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 2.0, 4e-6


def _err(x, truth):
    return ((x.double() - truth).abs().max() / truth.abs().max()).item()


def _bar(e_aten):
    return max(FACTOR * e_aten, FLOOR)


def _feature_pair(shape, seed):
    """post-ReLU-like maps: f0 = relu(randn), f1 = relu(f0 + 0.3 randn) (no all-zero pixel at these channel counts but by design)"""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(*shape, generator=g).relu()
    f1 = (f0 + 0.3 * torch.randn(*shape, generator=g)).relu()
    if shape[1] < 8:          # few channels: keep every pixel away from all-zero
        f0, f1 = f0 + 0.1, f1 + 0.1
    return f0.to(DEV), f1.to(DEV), torch.rand(shape[1], generator=g).to(DEV), (torch.rand(shape[0], generator=g) + 0.5).to(DEV)


def _head_three_ways(f0, f1, w, gw):
    """(value, g0, g1) in float64, ATen float32 and native"""
    from havatar_amd.model import lpips
    from havatar_amd.native import lpips_ops
    out = []
    for kind in ("f64", "aten", "native"):
        a, b = (t.double() if kind == "f64" else t.clone() for t in (f0, f1))
        a.requires_grad_(True), b.requires_grad_(True)
        if kind == "f64":
            v = lu.head64(a, b, w.double())
        elif kind == "aten":
            v = lpips.head_aten(a, b, w.view(1, -1, 1, 1)).view(-1)
        else:
            v = lpips_ops.lpips_head(a, b, w.view(1, -1, 1, 1)).view(-1)
        ga, gb = torch.autograd.grad((v * gw.to(v)).sum(), (a, b))
        out.append((v.detach(), ga, gb))
    return out


HEAD_SHAPES = [(1, 64, 1, 1), (1, 64, 3, 5), (3, 256, 7, 9), (2, 512, 4, 8), (2, 128, 32, 64),
               (1, 5, 9, 15),          # one-pixel items over three workgroups, a channel count that is no multiple of the four waves
               (2, 3, 2, 2)]           # four-pixel items, fewer channels than waves


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_forward_and_both_gradients(shape):
    f0, f1, w, gw = _feature_pair(shape, 3)
    t, a, n = _head_three_ways(f0, f1, w, gw)
    for name, k in (("value", 0), ("d/df0", 1), ("d/df1", 2)):
        ea, en = _err(a[k], t[k]), _err(n[k], t[k])
        print("head %s %s: native %.2e aten %.2e bar %.2e" % (shape, name, en, ea, _bar(ea)))
        assert en <= _bar(ea), (shape, name, en, ea)


@pytest.mark.parametrize("shape", [(1, 64, 3, 5), (2, 128, 32, 64)])
def test_head_one_sided_gradients_and_same_bits_on_every_launch(shape):
    from havatar_amd.native import lpips_ops as o
    f0, f1, w, gw = _feature_pair(shape, 4)
    v = o.head_fwd(f0, f1, w)
    g0, g1 = o.head_bwd(gw, f0, f1, w)
    # g1 = NULL, g0 = NULL: the wanted side has the same bits
    a0, none1 = o.head_bwd(gw, f0, f1, w, want1=False)
    none0, b1 = o.head_bwd(gw, f0, f1, w, want0=False)
    assert none0 is None and none1 is None and torch.equal(a0, g0) and torch.equal(b1, g1)
    assert o.head_bwd(gw, f0, f1, w, want0=False, want1=False) == (None, None)
    # two launches, the same bits
    v2 = o.head_fwd(f0, f1, w)
    h0, h1 = o.head_bwd(gw, f0, f1, w)
    assert torch.equal(v, v2) and torch.equal(g0, h0) and torch.equal(g1, h1)
    # through the node: only the side that requires grad is computed
    a = f0.clone().requires_grad_(True)
    y = o.lpips_head(a, f1, w.view(1, -1, 1, 1))
    assert y.shape == (shape[0], 1, 1, 1) and torch.equal(y.view(-1), v)
    assert torch.equal(torch.autograd.grad((y.view(-1) * gw).sum(), a)[0], g0)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(o.lpips_head(a, f1, w.view(1, -1, 1, 1)).sum(), a, create_graph=True)


@pytest.mark.parametrize("shape", [(1, 64, 3, 5), (2, 512, 4, 8), (2, 128, 32, 64)])
def test_head_identical_inputs_give_exact_zeros(shape):
    from havatar_amd.native import lpips_ops as o
    f0, _, w, gw = _feature_pair(shape, 5)
    assert torch.equal(o.head_fwd(f0, f0.clone(), w), torch.zeros(shape[0], device=DEV))
    g0, g1 = o.head_bwd(gw, f0, f0.clone(), w)
    assert not g0.any() and not g1.any()


def test_head_zeroed_pixels_are_finite_where_aten_is_nan():
    """THE ONE DELIBERATE DIFFERENCE: at a pixel whose features are all zero the node's gradient is the formula with its second term dropped
    (the term's limit); ATen's autograd differentiates sqrt at 0 and returns NaN there."""
    shape = (3, 256, 7, 9)
    f0, f1, w, gw = _feature_pair(shape, 6)
    f0[0, :, 1, 2] = 0          # in f0 only
    f0[1, :, 3, 4] = 0          # in both
    f1[1, :, 3, 4] = 0
    t, a, n = _head_three_ways(f0, f1, w, gw)
    ref0, ref1 = lu.head_grad64_dropped(f0.double(), f1.double(), w.double(), gw.double())
    # the formula is the gradient wherever float64 autograd is finite
    for r, tt in ((ref0, t[1]), (ref1, t[2])):
        ok = torch.isfinite(tt)
        assert (r[ok] - tt[ok]).abs().max().item() <= 1e-10 * tt[ok].abs().max().item()
    print("zeroed pixels: NaN elements of", a[1].numel(), "-- ATen d/df0 %d d/df1 %d, float64 autograd d/df0 %d d/df1 %d, native 0" % (
        torch.isnan(a[1]).sum().item(), torch.isnan(a[2]).sum().item(), torch.isnan(t[1]).sum().item(), torch.isnan(t[2]).sum().item()))
    assert torch.isnan(a[1][0, :, 1, 2]).all() and torch.isnan(a[1][1, :, 3, 4]).all() and torch.isnan(a[2][1, :, 3, 4]).all()
    assert torch.isfinite(a[2][0, :, 1, 2]).all()
    assert torch.isfinite(n[0]).all() and torch.isfinite(n[1]).all() and torch.isfinite(n[2]).all()
    ea_v, en_v = _err(a[0], t[0]), _err(n[0], t[0])
    assert en_v <= _bar(ea_v), (en_v, ea_v)
    for name, got, ref, at in (("d/df0", n[1], ref0, a[1]), ("d/df1", n[2], ref1, a[2])):
        ok = torch.isfinite(at)
        ea = ((at.double() - ref)[ok].abs().max() / ref.abs().max()).item()
        en = _err(got, ref)
        print("zeroed pixels %s: native %.2e aten (finite part) %.2e" % (name, en, ea))
        assert en <= _bar(ea), (name, en, ea)


# ------------------------------------------------------------------------------------------------------------------------------------
# ConvReluFrozen and the ReLU mask
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,cin,cout,H,W", [(1, 64, 64, 4, 32), (2, 128, 256, 8, 16), (1, 512, 512, 8, 16), (2, 64, 128, 16, 48)])
def test_conv_relu_frozen_forward_and_data_gradient(B, cin, cout, H, W, monkeypatch):
    from havatar_amd.native import conv as nconv, lpips_ops as o
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, cin, H, W, generator=g).relu().to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(DEV)
    bias = (0.05 * torch.randn(cout, generator=g)).to(DEV)
    gy = torch.randn(B, cout, H, W, generator=g).to(DEV)
    assert o.conv_relu_eligible(x, wt)
    wcalls = []
    for name in ("wgrad3x3", "wgrad3x3s2"):
        monkeypatch.setattr(nconv, name, lambda *a, _n=name, **k: wcalls.append(_n))
    res = {}
    for kind in ("f64", "aten", "native"):
        xi = (x.double() if kind == "f64" else x.clone()).requires_grad_(True)
        if kind == "native":
            y = o.conv_relu_frozen(xi, bias, nconv.pack(wt), nconv.pack_t(wt), cout)
            assert type(y.grad_fn).__name__ == "ConvReluFrozenBackward" and len(y.grad_fn.saved_tensors) == 1          # y only: x is not kept
        else:
            y = F.relu(F.conv2d(xi, wt.to(xi), bias.to(xi), padding=1))
        res[kind] = (y.detach(), torch.autograd.grad(y, xi, gy.to(y))[0])
    assert wcalls == []          # no weight gradient is ever formed
    for name, k in (("forward", 0), ("data gradient", 1)):
        ea, en = _err(res["aten"][k], res["f64"][k]), _err(res["native"][k], res["f64"][k])
        print("conv_relu %s %s: native %.2e aten %.2e bar %.2e" % ((B, cin, cout, H, W), name, en, ea, _bar(ea)))
        assert en <= _bar(ea), (name, en, ea)
    xi = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(o.conv_relu_frozen(xi, bias, nconv.pack(wt), nconv.pack_t(wt), cout).sum(), xi, create_graph=True)


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (3, 64, 16, 16), (1, 3, 5, 7)])
def test_relu_mask_and_its_bias_sum(shape):
    from havatar_amd.native import lpips_ops as o
    g = torch.Generator().manual_seed(9)
    y = torch.randn(*shape, generator=g).relu().to(DEV)
    gr = torch.randn(*shape, generator=g).to(DEV)
    want = gr * (y > 0)
    gc = o.relu_mask_bwd(gr, y)
    gc2, gb = o.relu_mask_bwd(gr, y, want_bias=True)
    assert torch.equal(gc, want) and torch.equal(gc2, want)
    truth = want.double().sum((0, 2, 3))
    e = _err(gb, truth)
    print("relu mask bias sum %s: %.2e" % (shape, e))
    assert e <= 2.0 ** -23          # a float64 sum rounded once to float32


# ------------------------------------------------------------------------------------------------------------------------------------
# the whole module
# ------------------------------------------------------------------------------------------------------------------------------------
IMAGE_SEED = 11          # see the module's docstring: what a ReLU / max-pool kink does to this comparison, and what this pair is
ATEN_CPU_GRAD = 3.8e-6   # ATen float32 against float64, gradient into in0, on inputs where it flips no kink (the issue's figure; the fixture
#                          measures 3.6e-6 on the CPU at 2x3x64x128, and 3.6e-6 / 3.7e-6 at both sizes for the pair of seed 18)
CASES = {"1x3x128x256": ((1, 3, 128, 256), 5),          # every eligible layer native (slice 5 at 8 x 16)
         "2x3x64x128": ((2, 3, 64, 128), 4)}            # slice 5 at 4 x 8 falls back to ATen


def _expected_layers(shape, slices):
    """(Cin, Cout, H, W) of every convolution that must take ConvReluFrozen: all but conv1_1 (Cin = 3) in the first `slices` slices"""
    from havatar_amd.model import lpips
    return [(cin, cout, shape[2] >> (s - 1), shape[3] >> (s - 1)) for s, n, cin, cout in lpips.CONVS if n != 0 and s <= slices]


class _Routes:
    """call probe: which layers took the two nodes (wraps the functions model/lpips.py calls them through)"""

    def __enter__(self):
        from havatar_amd.native import lpips_ops as o
        self.o, self.real, self.conv, self.head = o, (o.conv_relu_frozen, o.lpips_head), [], []
        o.conv_relu_frozen = lambda x, bias, pack, pack_t, Cout: (self.conv.append((x.shape[1], Cout, x.shape[2], x.shape[3])), self.real[0](x, bias, pack, pack_t, Cout))[1]
        o.lpips_head = lambda f0, f1, w: (self.head.append(f0.shape[1]), self.real[1](f0, f1, w))[1]
        return self

    def __exit__(self, *a):
        self.o.conv_relu_frozen, self.o.lpips_head = self.real


def _grad_run(fn, in0, env="0"):
    """(value, gradient into in0, conv layers on the node, taps on the node) of fn(in0 with grad) under HAVATAR_LPIPS = env (None: unset)"""
    saved = os.environ.get("HAVATAR_LPIPS")
    try:
        os.environ.pop("HAVATAR_LPIPS", None)
        if env is not None:
            os.environ["HAVATAR_LPIPS"] = env
        with _Routes() as r:
            a = in0.clone().requires_grad_(True)
            v = fn(a)
            g = torch.autograd.grad(v.sum(), a)[0]
        return v.detach(), g, r.conv, r.head
    finally:
        os.environ.pop("HAVATAR_LPIPS", None)
        if saved is not None:
            os.environ["HAVATAR_LPIPS"] = saved


@pytest.fixture(scope="module")
def whole():
    """per case: float64 truth on the device; ATen float32 on the CPU (the yardstick as the issue measured it); the module with HAVATAR_LPIPS=0
    between two runs of the in-test ATen float32 restatement (one warm-up run of it first: MIOpen settles its solvers at a first call); the
    module with HAVATAR_LPIPS=1 twice and unset"""
    vgg, lin = lu.weights()
    m, mc = lu.module(DEV), lu.module("cpu")
    out = {}
    for name, (shape, _) in CASES.items():
        c0, c1 = lu.images(shape, IMAGE_SEED)
        in0, in1 = c0.to(DEV), c1.to(DEV)
        a = in0.double().requires_grad_(True)
        v = lu.lpips64(a, in1.double(), vgg, lin)
        r = {"f64": (v.detach(), torch.autograd.grad(v.sum(), a)[0]), "cpu": _grad_run(lambda x: mc(x, c1), c0)}
        ref = lambda x: lu.lpips_aten32(x, in1, vgg, lin)
        _grad_run(ref, in0)
        r["ref_a"], r["aten"], r["ref_b"] = _grad_run(ref, in0), _grad_run(lambda x: m(x, in1), in0, "0"), _grad_run(ref, in0)
        r["native"], r["native_again"], r["unset"] = (_grad_run(lambda x: m(x, in1), in0, e) for e in ("1", "1", None))
        out[name] = r
    return out


def _grad_err(x, tg):
    return (x.double() - tg).abs() / tg.abs().max()


def _yardstick(r):
    """ATen float32's distance to float64, value and gradient: the smallest of the device's, the CPU's and, for the gradient, its kink-free
    figure (a kink that a run flips is that run's accident, not the precision of float32: the cap only tightens the bar)"""
    tv, tg = r["f64"]
    ev = min(_err(r["aten"][0], tv), _err(r["cpu"][0].to(DEV), tv))
    eg = min(_grad_err(r["aten"][1], tg).max().item(), _grad_err(r["cpu"][1].to(DEV), tg).max().item(), ATEN_CPU_GRAD)
    return ev, eg


@pytest.mark.parametrize("case", list(CASES))
def test_whole_module_value_gradient_and_routes(whole, case):
    r = whole[case]
    tv, tg = r["f64"]
    shape, slices = CASES[case]
    # routes: exactly the expected layers took ConvReluFrozen (for both images, in order), all five taps took LpipsHead
    assert r["native"][2] == _expected_layers(shape, slices) * 2 and len(r["native"][2]) == (24 if slices == 5 else 18)
    assert r["native"][3] == [64, 128, 256, 512, 512]
    ev, eg = _yardstick(r)
    en = _err(r["native"][0], tv)
    print("module %s value: native %.2e, aten device %.2e cpu %.2e, bar %.2e" % (case, en, _err(r["aten"][0], tv), _err(r["cpu"][0].to(DEV), tv), _bar(ev)))
    assert en <= _bar(ev), (en, ev)
    dn, bar = _grad_err(r["native"][1], tg), _bar(eg)
    outside = (dn > bar).double().mean().item()
    print("module %s gradient: native max %.2e median %.2e, aten device max %.2e cpu max %.2e, bar %.2e, share outside %.2e" % (
        case, dn.max().item(), dn.median().item(), _grad_err(r["aten"][1], tg).max().item(), _grad_err(r["cpu"][1].to(DEV), tg).max().item(), bar, outside))
    # a ReLU / max-pool kink flipped by different rounding may put single elements outside: at most 1e-3 of them, and the median inside
    assert outside <= 1e-3 and dn.median().item() <= bar, (dn.max().item(), eg, outside)


@pytest.mark.parametrize("case", list(CASES))
def test_switch_set_and_unset_agree(whole, case):
    """HAVATAR_LPIPS=1 and unset take the same nodes, layer for layer, and agree within the bar -- one times the bar, no element excused.  (Both
    are the same calls: the nodes give the same bits on every launch; what may differ is ATen's own layers -- conv1_1 and the fallback slice --
    whose MIOpen gradient kernels this test does not pin.  Whether the bits were equal is printed.)"""
    from havatar_amd.native import lpips_ops as o
    assert o.DEFAULT == "1"
    r = whole[case]
    tv, tg = r["f64"]
    ev, eg = _yardstick(r)
    for other in ("unset", "native_again"):
        assert r[other][2] == r["native"][2] and r[other][3] == r["native"][3]
        dv = _err(r[other][0], r["native"][0].double())
        dg = ((r[other][1].double() - r["native"][1].double()).abs() / tg.abs().max()).max().item()
        print("switch %s: =1 against %s: value %.2e gradient %.2e of the largest entry (bits equal: %s, %s)" % (
            case, other, dv, dg, torch.equal(r[other][0], r["native"][0]), torch.equal(r[other][1], r["native"][1])))
        assert dv <= _bar(ev) and dg <= _bar(eg), (other, dv, dg)


def test_switch_off_head_scaling_and_pooling_are_atens_bits(monkeypatch):
    """the pieces of the HAVATAR_LPIPS=0 route that hold no 3x3 convolution, bit for bit against float32 statements written here"""
    from havatar_amd.model import lpips
    monkeypatch.setenv("HAVATAR_LPIPS", "0")
    m = lu.module(DEV)
    x = lu.images((2, 3, 16, 32), 3)[0].to(DEV)
    shift, scale = torch.tensor(lu.SHIFT, device=DEV).view(1, 3, 1, 1), torch.tensor(lu.SCALE, device=DEV).view(1, 3, 1, 1)
    assert torch.equal(m.scaling_layer(x), (x - shift) / scale)
    f = torch.randn(2, 64, 6, 10, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(m.net.slice2[0](f), F.max_pool2d(f, 2, 2))
    for shape in ((1, 64, 3, 5), (2, 128, 32, 64), (2, 512, 4, 8)):
        f0, f1, w, gw = _feature_pair(shape, 12)
        w4 = w.view(1, -1, 1, 1)
        res = []
        for fn in (lpips.head_aten, lambda a, b, ww: F.conv2d((a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
                                                               - b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)) ** 2, ww).mean([2, 3], keepdim=True)):
            a = f0.clone().requires_grad_(True)
            v = fn(a, f1, w4)
            res.append((v.detach(), torch.autograd.grad((v.view(-1) * gw).sum(), a)[0]))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), shape


@pytest.mark.parametrize("case", list(CASES))
def test_switch_off_is_the_aten_statement(whole, case):
    """HAVATAR_LPIPS=0: no node runs, and value and gradient are those of the in-test ATen float32 restatement (tests/lpips_util.py::
    lpips_aten32) run in the same process just before and just after.  Bit for bit this holds for the pieces without a 3x3 convolution
    (the test above) and on the CPU for the whole module at both sizes (tests/test_lpips_cpu.py::
    test_aten_route_is_the_float32_statement_bit_for_bit).  On the device it does not hold in general, and not because of the module: two
    IDENTICAL runs of the restatement themselves give other bits there -- measured, of the largest entry: gradient 1.5e-6 (1x3x128x256) and
    3.3e-6 (2x3x64x128), value 0 and 6.9e-8 (in another session 0 and 0 with the module 1 ulp off) -- and the module sits as far from either
    run (1.3e-6 / 2.6e-6, 0 / 6.9e-8).  Every figure is printed with whether the bits were equal.  So on the device the
    assertion is distance: one times the rule's bar of the largest entry, no element excused.  The =0 route is also bounded against float64:
    the value by the bar, the gradient by its median (ATen float32 flips kinks of its own, see the module's docstring)."""
    r = whole[case]
    tv, tg = r["f64"]
    assert r["aten"][2] == [] and r["aten"][3] == []
    ev, eg = _yardstick(r)
    for k, what, bar in ((0, "value", _bar(ev)), (1, "gradient", _bar(eg))):
        scale = (tv if k == 0 else tg).abs().max().item()
        spread = (r["ref_a"][k].double() - r["ref_b"][k].double()).abs().max().item() / scale
        dist = (r["aten"][k].double() - r["ref_a"][k].double()).abs().max().item() / scale
        print("switch off %s %s: the restatement's two runs: same bits %s (distance %.2e); module against the restatement: same bits %s (distance %.2e)" % (
            case, what, torch.equal(r["ref_a"][k], r["ref_b"][k]), spread, torch.equal(r["aten"][k], r["ref_a"][k]), dist))
        assert dist <= bar, (what, dist, spread)          # one times the rule's bar, no element excused
    assert _err(r["aten"][0], tv) <= _bar(ev)
    d = _grad_err(r["aten"][1], tg)
    print("switch off %s gradient against float64: max %.2e median %.2e share outside %.2e" % (case, d.max().item(), d.median().item(), (d > _bar(eg)).double().mean().item()))
    assert d.median().item() <= _bar(eg)


# ------------------------------------------------------------------------------------------------------------------------------------
# the joint step
# ------------------------------------------------------------------------------------------------------------------------------------
def test_joint_step_reaches_the_native_module_once(tmp_path, monkeypatch):
    """iteration 1 of harness/stage2_step_cases.py with the 0.1 * LPIPS term: on the device the module runs natively exactly once, and
    percep_loss agrees with the CPU float64 run within the bar tests/test_train_hd_gpu.py uses for the step's scalars (2e-3 of the value,
    float32 arithmetic in both radiance MLPs)."""
    from havatar_amd import synth
    from havatar_amd.harness import stage2_step_cases
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.model.styleUnet import Discriminator, SWGAN_unet
    from havatar_amd.utils import styleUnet_util
    split = synth.write_dataset(str(tmp_path / "dataset"), n_frames=2, img_res=128)
    for k in ("HAVATAR_HAAR_TRAIN", "HAVATAR_S2_LOSS", "HAVATAR_LPIPS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HAVATAR_TRAIN_MLP", "torch")
    monkeypatch.setenv("HAVATAR_MLP", "f32")
    monkeypatch.setenv("HAVATAR_LPIPS", "1")
    res = {}
    for device, dtype in (("cpu", torch.float64), (DEV, torch.float32)):
        with _Routes() as routes:
            out = stage2_step_cases.run(Trainer, SWGAN_unet, Discriminator, styleUnet_util, split, device=device, dtype=dtype, iterations=(1,),
                                        pinned=True, records="grads", percep=lu.module)
        res[device] = (float(out["i1_scalar_percep_loss"]), float(out["i1_scalar_g_loss"]), routes.conv, routes.head)
    assert res["cpu"][2] == [] and res["cpu"][3] == []
    # once: the five taps once each, and the layers of one 2 x 3 x 128 x 128 pair (slice 5 at 8 x 8 stays on ATen)
    assert res[DEV][3] == [64, 128, 256, 512, 512] and res[DEV][2] == _expected_layers((2, 3, 128, 128), 4) * 2
    for name, k in (("percep_loss", 0), ("g_loss", 1)):
        x, y = res[DEV][k], res["cpu"][k]
        print("joint step %s: device %.6e cpu float64 %.6e" % (name, x, y))
        assert abs(x - y) <= 2e-3 * max(abs(y), 1e-3), (name, x, y)
    assert res["cpu"][0] > 0

"""GPU: the image-space losses of the stage-two joint step as one autograd node (native/train_ops.py::Stage2ImageLoss on hav_s2_image_loss_fwd /
_bwd, csrc/hav_s2_loss.hip) against the float64 ATen statement of the reference's lines (train_avatarHD.py:246-247, :251, :268, :282-283).

Shapes (B, C, r, G), in the kernels' own terms: a forward thread owns 4 columns of one (b, c, row) of the G x G maps, a workgroup is 256 of
them and leaves one row of partials; a backward thread of the gather owns one low-resolution element.
  (1, 3, 2, 4)      smallest legal r: every pixel is an edge pixel; one ragged workgroup
  (2, 67, 5, 12)    non-integer ratio, the strided 67-channel view, r % 4 != 0
  (1, 3, 8, 8)      identity scale: lr == render exactly; gt_lr equals it at a tenth of the positions (sign(0) = 0)
  (2, 67, 32, 128)  the harness shape; 96 workgroups of partials
  (3, 3, 48, 192)   324 workgroups of partials: the one-workgroup reduction loops
  (1, 3, 3, 6), (2, 4, 5, 13)   G % 4 != 0: the 4-byte variant of both kernels, with a ragged last column group

The bar of every quantity is 4 x the distance of the float32 ATen statement (on the device, same inputs) to float64: another summation order,
not another precision.  Distances are relative: |x - x64| / |x64| for a scalar, max |g - g64| / max |g64| for a gradient.  Measured on an MI355X
(node / ATen float32, the largest over the eight quantities and both rgb_loss modes; every case prints all of them):
  (1, 3, 2, 4) 3.6e-7 / 2.7e-7 (mask_bce)   (2, 67, 5, 12) 2.7e-7 / 2.7e-7   (1, 3, 8, 8) 1.8e-7 / 1.8e-7   (2, 67, 32, 128) 1.4e-6 / 1.4e-6 (grad_render)
  (3, 3, 48, 192) 2.9e-6 / 3.0e-6 (grad_render)   (1, 3, 3, 6) 1.5e-7 / 1.4e-7   (2, 4, 5, 13) 1.8e-7 / 1.8e-7
The five sums are kept in float64 for this bar's sake: where ATen's float32 scalar happens to be the correctly rounded one (2e-8 away), a float32
sum in another order is a whole ulp (1.2e-7) away and 4 x 2e-8 does not cover it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 3, 2, 4), (2, 67, 5, 12), (1, 3, 8, 8), (2, 67, 32, 128), (3, 3, 48, 192), (1, 3, 3, 6), (2, 4, 5, 13)]
NAMES = ("rgb_loss", "hr_l1", "mask_bce", "lr_mse", "sr_mse", "grad_render", "grad_mask", "grad_fake")


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("HAVATAR_S2_LOSS", raising=False)


def _inputs(shape, seed=3):
    """float64 CPU tensors: the [B,r,r,C] leaf behind the render, the [B,r,r,1] one behind the mask, and the five constants / fake"""
    B, C, r, G = shape
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, r, r, C, generator=g, dtype=torch.float64).float().double()
    m = torch.rand(B, r, r, 1, generator=g, dtype=torch.float64) * 1.2 - 0.1          # [-0.1, 1.1]: both clip sides occur
    for bound in (1e-3, 1.0 - 1e-3):                                                   # ... but never within 1e-3 of a clip bound
        m = torch.where((m - bound).abs() < 1e-3, m + 2.5e-3, m)
    m = m.float().double()
    gt_mask = torch.rand(B, 1, r, r, generator=g, dtype=torch.float64).float().double()
    fake = torch.rand(B, 3, G, G, generator=g, dtype=torch.float64).float().double()
    gt_hr = torch.rand(B, 3, G, G, generator=g, dtype=torch.float64).float().double()
    gt_hr[:, :, ::3, ::5] = fake[:, :, ::3, ::5]                                       # sign(0) in grad_fake
    gt_lr = torch.rand(B, 3, G, G, generator=g, dtype=torch.float64).float().double()
    if r == G:                                                                         # identity scale: lr == render bit for bit
        lr = base.permute(0, 3, 1, 2)[:, :3]
        tenth = (torch.arange(B * 3 * G * G).reshape(B, 3, G, G) % 10) == 0
        gt_lr = torch.where(tenth, lr, gt_lr)
    return base, m, gt_lr, fake, gt_hr, gt_mask


def _run(inputs, device, dtype, rgb_loss, native):
    """-> the eight quantities of NAMES, float64 on the CPU"""
    from havatar_amd.native import train_ops as t
    base, m, gt_lr, fake, gt_hr, gt_mask = [x.to(device=device, dtype=dtype).detach().clone() for x in inputs]
    base.requires_grad_(True)
    m.requires_grad_(True)
    fake.requires_grad_(True)
    render, mask = base.permute(0, 3, 1, 2), m.permute(0, 3, 1, 2)
    out = t.stage2_image_loss(render, mask, gt_lr, fake, gt_hr, gt_mask, rgb_loss, native=native)
    assert (out[0].grad_fn is not None and type(out[0].grad_fn).__name__.startswith("Stage2ImageLoss")) == bool(native)
    (out[0] * 1.0 + out[1] * 0.7 + out[2] * 0.01).backward()
    res = [o.detach() for o in out] + [base.grad.permute(0, 3, 1, 2), m.grad.permute(0, 3, 1, 2), fake.grad]
    return [x.double().cpu() for x in res]


def _dist(x, ref):
    return ((x - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("rgb_loss", ["mse", "l1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_all_gradients_against_float64(shape, rgb_loss):
    inputs = _inputs(shape)
    ref = _run(inputs, "cpu", torch.float64, rgb_loss, False)
    aten = _run(inputs, DEV, torch.float32, rgb_loss, False)
    node = _run(inputs, DEV, torch.float32, rgb_loss, True)
    bad = []
    for name, r64, a, n in zip(NAMES, ref, aten, node):
        da, dn = _dist(a, r64), _dist(n, r64)
        print("%s %s %-12s node %.3e  aten32 %.3e" % (shape, rgb_loss, name, dn, da))
        if not dn <= 4 * da:
            bad.append((name, dn, da))
    # channels 3.. of the render take no part: exact zeros
    assert shape[1] == 3 or not node[5][:, 3:].any()
    assert torch.isfinite(torch.cat([x.reshape(-1) for x in node])).all()
    assert not bad, bad


def test_two_launches_give_identical_bits():
    inputs = _inputs((2, 67, 32, 128))
    for rgb_loss in ("mse", "l1"):
        a, b = _run(inputs, DEV, torch.float32, rgb_loss, True), _run(inputs, DEV, torch.float32, rgb_loss, True)
        for name, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), name


def test_gradient_of_the_unread_channels_is_exactly_zero():
    node = _run(_inputs((2, 67, 32, 128)), DEV, torch.float32, "mse", True)
    assert node[5].shape == (2, 67, 32, 32) and node[5][:, :3].abs().max() > 0
    assert torch.equal(node[5][:, 3:], torch.zeros_like(node[5][:, 3:]))


def test_sign_of_zero_is_zero():
    inputs = _inputs((1, 3, 8, 8))
    node = _run(inputs, DEV, torch.float32, "l1", True)
    tenth = (torch.arange(3 * 64).reshape(1, 3, 8, 8) % 10) == 0
    assert not node[5][tenth].any() and node[5][~tenth].abs().min() > 0
    assert not node[7][:, :, ::3, ::5].any()


def _route(monkeypatch, value, inputs, dtype=torch.float32, grad=True):
    from havatar_amd.native import train_ops as t
    monkeypatch.delenv("HAVATAR_S2_LOSS", raising=False)
    if value is not None:
        monkeypatch.setenv("HAVATAR_S2_LOSS", value)
    base, m, gt_lr, fake, gt_hr, gt_mask = [x.to(device=DEV, dtype=dtype).detach().clone() for x in inputs]
    base.requires_grad_(True)
    with torch.set_grad_enabled(grad):
        out = t.stage2_image_loss(base.permute(0, 3, 1, 2), m.permute(0, 3, 1, 2), gt_lr, fake, gt_hr, gt_mask, "mse")
    return type(out[0].grad_fn).__name__ if out[0].grad_fn is not None else None, out


def test_switch_selects_the_route(monkeypatch):
    inputs = _inputs((2, 67, 5, 12))
    for v in (None, "1"):          # the node is the default
        on, out_on = _route(monkeypatch, v, inputs)
        assert on.startswith("Stage2ImageLoss")
    off, out_off = _route(monkeypatch, "0", inputs)
    assert off is not None and not off.startswith("Stage2ImageLoss")
    for a, b in zip(out_on, out_off):
        assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item())
    # what the node does not take keeps the statement with the switch set: another dtype, grad mode off
    assert not _route(monkeypatch, "1", inputs, dtype=torch.float64)[0].startswith("Stage2ImageLoss")
    assert _route(monkeypatch, "1", inputs, grad=False)[0] is None


def test_first_order_only():
    from havatar_amd.native import train_ops as t
    base, m, gt_lr, fake, gt_hr, gt_mask = [x.to(device=DEV, dtype=torch.float32).detach().clone() for x in _inputs((1, 3, 2, 4))]
    base.requires_grad_(True)
    out = t.stage2_image_loss(base.permute(0, 3, 1, 2), m.permute(0, 3, 1, 2), gt_lr, fake, gt_hr, gt_mask, "mse", native=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|twice"):
        g, = torch.autograd.grad(out[0].pow(2), base, create_graph=True)
        g.pow(2).sum().backward()

"""GPU: the stage-two Discriminator on the device -- forward, the logistic-loss backward, the R1 backward (create_graph through every native
node it reaches: the 3x3 blocks, the stride-2 blocks, EqualLinearFn) and the generator's non-saturating loss through a frozen
discriminator, in float32 with HAVATAR_HAAR_TRAIN set and unset, each against the same module in float64 on the device (non-float32
tensors take the ATen routes).  The switch-set error is at most twice the switch-unset error, with a floor of 1e-6 of the largest
magnitude; at size 64 the float32 prediction also matches the reference's CPU value (tests/golden/discriminator.npz) within 1e-3."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [n for n, _ in f.next_functions]
    return names


def _run(size, B, dtype, switch):
    from havatar_amd.harness import stage2_cases
    from havatar_amd.utils import styleUnet_util as u
    old = os.environ.pop("HAVATAR_HAAR_TRAIN", None)
    if switch:
        os.environ["HAVATAR_HAAR_TRAIN"] = "1"
    try:
        from havatar_amd.model.styleUnet import Discriminator
        d = stage2_cases.make(Discriminator, size, 0, dtype).to(DEV)
        args = u.styleUnet_args()
        real, fake = stage2_cases.image(B, size, 40 + B, dtype).to(DEV), stage2_cases.image(B, size, 52, dtype).to(DEV)
        res = {}
        real_pred, fake_pred = d(real), d(fake)
        res["names"] = _graph_names(real_pred)
        res["pred"] = real_pred.detach()
        loss = u.d_logistic_loss(real_pred, fake_pred)
        d.zero_grad()
        loss.backward()
        res["d_loss"] = loss.detach()
        res["d_grads"] = {n: p.grad.detach().clone() for n, p in d.named_parameters()}
        real.requires_grad = True
        real_pred = d(real)
        res["names_r1"] = _graph_names(real_pred)          # (the image requires grad here: the wavelet pyramid is part of the graph)
        r1 = u.d_r1_loss(real_pred, real)
        d.zero_grad()
        (args.r1 / 2 * r1 * args.d_reg_every + 0 * real_pred[0]).backward()
        res["r1_loss"] = r1.detach()
        res["r1_grads"] = {n: p.grad.detach().clone() for n, p in d.named_parameters()}
        # the generator's side: a frozen discriminator, the gradient goes into the image
        u.requires_grad(d, False)
        d.zero_grad(set_to_none=True)
        img = fake.clone().requires_grad_(True)
        g_loss = u.g_nonsaturating_loss(d(img))
        g_loss.backward()
        res["g_loss"], res["g_input_grad"] = g_loss.detach(), img.grad.detach().clone()
        res["g_param_grads"] = [n for n, p in d.named_parameters() if p.grad is not None]
        return res
    finally:
        os.environ.pop("HAVATAR_HAAR_TRAIN", None)
        if old is not None:
            os.environ["HAVATAR_HAAR_TRAIN"] = old


@pytest.fixture(scope="module", params=[(64, 4), (128, 2)], ids=["64-b4", "128-b2"])
def runs(request):
    """MIOpen's default choice for the small stride-2 convolutions sums with float atomics: two runs of the SAME float32 route then differ in
    the last bits of the activations, a pre-activation next to zero lands on either side of the leaky-ReLU's kink, and R1's second-order
    gradients (piecewise constant in those signs) move by far more than rounding -- 0.2 of a bias gradient's magnitude between two runs
    of one route at size 128.  The routes are compared on deterministic convolutions, so that they see the same signs."""
    size, B = request.param
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield size, B, _run(size, B, torch.float64, False), _run(size, B, torch.float32, False), _run(size, B, torch.float32, True)
    finally:
        torch.backends.cudnn.deterministic = old


def _bar(what, on, off, ref):
    ref = ref.double()
    mag = ref.abs().max().item()
    e_on, e_off = (on.double() - ref).abs().max().item(), (off.double() - ref).abs().max().item()
    print("%s: set %.3e unset %.3e magnitude %.3e" % (what, e_on, e_off, mag))
    assert e_on <= max(2.0 * e_off, 1e-6 * mag), (what, e_on, e_off, mag)
    return e_off, mag


def test_the_switch_puts_the_wavelet_nodes_into_the_graph(runs):
    size, B, ref, off, on = runs
    for r in (ref, off):
        assert not any(n.startswith("Haar") for n in r["names"] | r["names_r1"])
    assert {"HaarDwtBackward", "HaarDown2Backward"} <= on["names_r1"]
    # the 3x3 block takes its native node at both sizes, the stride-2 block where its output is a multiple of 32 columns wide
    # (native/conv.py::s2_eligible): the 64 -> 32 layer of size 128, none at size 64 (32 -> 16) -- so R1 reaches both create_graph branches
    for r in (off, on):
        assert any("FusedConvBlock" in n for n in r["names"]), sorted(r["names"])
        assert any("S2ConvBlock" in n for n in r["names"]) == (size >= 128), sorted(r["names"])
        assert "EqualLinearFnBackward" in r["names"]


def test_prediction_and_losses(runs):
    size, B, ref, off, on = runs
    for k in ("pred", "d_loss", "r1_loss", "g_loss"):
        e_off, mag = _bar("%s %d" % (k, size), on[k], off[k], ref[k])
        assert e_off <= 2e-3 * mag, (k, e_off, mag)          # the unset route itself holds the project's float32 bar (R1 raised here before)
    if size == 64:
        want = np.load(os.path.join(ROOT, "tests", "golden", "discriminator.npz"))["fwd_f32_64_b4_c0"]
        for r in (off, on):
            assert np.abs(r["pred"].double().cpu().numpy() - want).max() <= 1e-3 * np.abs(want).max()


def test_logistic_loss_gradients(runs):
    size, B, ref, off, on = runs
    assert ref["d_grads"].keys() == off["d_grads"].keys() == on["d_grads"].keys()
    for n in ref["d_grads"]:
        _bar("d_logistic %s" % n, on["d_grads"][n], off["d_grads"][n], ref["d_grads"][n])


def test_r1_gradients(runs):
    size, B, ref, off, on = runs
    assert ref["r1_grads"].keys() == off["r1_grads"].keys() == on["r1_grads"].keys()
    for n in ref["r1_grads"]:
        _bar("r1 %s" % n, on["r1_grads"][n], off["r1_grads"][n], ref["r1_grads"][n])
    assert max(g.abs().max().item() for g in ref["r1_grads"].values()) > 0
    # the unset route is today's statement plus EqualLinearFn's new create_graph branch (it raised there before): its weight gets a gradient
    assert off["r1_grads"]["final_linear.1.weight"].abs().max().item() > 0


def test_runs_of_one_route_are_reproducible(runs):
    """what the comparison above rests on: with deterministic convolutions a route gives the same bits twice"""
    size, B, ref, off, on = runs
    again = _run(size, B, torch.float32, True)
    assert torch.equal(again["pred"], on["pred"]) and torch.equal(again["r1_loss"], on["r1_loss"])
    assert torch.equal(on["pred"], off["pred"])          # and the wavelet nodes' forward bits are the statement's


def test_generator_loss_through_a_frozen_discriminator(runs):
    size, B, ref, off, on = runs
    _bar("g input gradient %d" % size, on["g_input_grad"], off["g_input_grad"], ref["g_input_grad"])
    for r in (ref, off, on):
        assert r["g_param_grads"] == [] and r["g_input_grad"].abs().max().item() > 0

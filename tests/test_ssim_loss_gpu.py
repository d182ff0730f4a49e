"""Device: the SSIM training loss (csrc/hav_ssim_loss.hip through native/ssim_ops.py and havatar_amd.metrics.ssim_loss) against float64
autograd of metrics.aten_statement on the .double() pair (computed on the CPU, once per case), with the ATen float32 statement on the device
as the yardstick beside it; the exact behaviours (forward bits, identical pairs, every element written, reproducibility, streams, capture),
the routing, and the wiring into the two training steps.

Bar of the gradient: every element within 2^-22 max|g64| -- two float32 units in the last place at the largest entry: one for the single final
rounding that the float64 arithmetic implies, one of slack for summation order.

Measured on an MI355X (worst over the shapes below; e = max |g - g64| / max |g64|, the bar is 2.4e-7):
    kind      node      ATen float32 statement on the device
    uniform   5.0e-8    9.2e-7
    flat      4.7e-8    1.2e-2
    mixed     3.6e-8    3.4e-4
The node's error is the float32 rounding of the stored gradient (at most 6e-8 of an entry); the statement's on the flat and mixed kinds is the
cancellation of g * x^2 - mu^2 in float32 divided by C2 = 9e-4."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import helpers
import metrics_util as mu
from havatar_amd import metrics, synth
from havatar_amd.native import metrics_ops, ssim_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 11, 11),          # one window, map 1 x 1
          (2, 3, 12, 13),          # odd width, the 4-byte path, the rim
          (1, 3, 42, 44),          # a full map tile, the 16-byte path
          (1, 2, 43, 47),          # 2 x 2 map tiles with one-wide edge tiles, a second pixel tile
          (2, 3, 75, 76),          # an interior tile with neighbours on every side
          (2, 3, 64, 64)]          # the stage-one patch
KINDS = ("uniform", "flat", "mixed")
BAR = 2.0 ** -22


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def pair(kind, shape):
    """float32 [B,C,H,W] pair on the host:
    uniform  two independent draws from [0, 1)
    flat     1.0 everywhere against 0.9 everywhere
    mixed    white in both, with a block in the middle (half the height, half the width) of uniform texture, the second a noisy copy of it"""
    B, C, H, W = shape
    a = torch.rand(shape, generator=torch.Generator().manual_seed(21))
    b = torch.rand(shape, generator=torch.Generator().manual_seed(22))
    if kind == "flat":
        a, b = torch.full(shape, 1.0), torch.full(shape, 0.9)
    elif kind == "mixed":
        tex, other = a, (a + 0.1 * (b - 0.5)).clamp(0, 1)
        a, b = torch.ones(shape), torch.ones(shape)
        ys, xs = slice(H // 4, H // 4 + max(H // 2, 1)), slice(W // 4, W // 4 + max(W // 2, 1))
        a[:, :, ys, xs], b[:, :, ys, xs] = tex[:, :, ys, xs], other[:, :, ys, xs]
    elif kind != "uniform":
        raise ValueError(kind)
    return a.contiguous(), b.contiguous()


def weights(B):
    return torch.tensor([0.3, 1.7][:B])


@functools.lru_cache(maxsize=None)
def truth(kind, shape):
    """float64 autograd of the statement on the .double() pair, on the CPU: d(sum_b w_b ssim_b) / dx"""
    a, b = pair(kind, shape)
    x = a.double().requires_grad_(True)
    s = metrics.aten_statement(x, b.double())[0]
    g, = torch.autograd.grad(s, x, grad_outputs=weights(shape[0]).double())
    return g


def _node_grad(a, b, w):
    x = a.clone().requires_grad_(True)
    s = ssim_ops.ssim_mean(x, b)
    g, = torch.autograd.grad(s, x, grad_outputs=w)
    return s.detach(), g


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_bits_and_gradient_against_float64(kind, shape):
    a, b = (t.to(DEV) for t in pair(kind, shape))
    w = weights(shape[0]).to(DEV)
    g64 = truth(kind, shape)
    gmax = float(g64.abs().max())
    s, g = _node_grad(a, b, w)
    assert s.dtype == torch.float32 and tuple(s.shape) == (shape[0],) and g.dtype == torch.float32 and g.shape == a.shape and g.is_contiguous()
    assert torch.equal(s, metrics.ssim(a, b))          # the forward is the metric's, bit for bit
    e = float((g.double().cpu() - g64).abs().max())
    # the yardstick: the float32 statement under autograd on the device
    x = a.clone().requires_grad_(True)
    ga, = torch.autograd.grad(metrics.aten_statement(x, b)[0], x, grad_outputs=w)
    e_aten = float((ga.double().cpu() - g64).abs().max())
    helpers.report("ssim_loss grad %s %s: max|g64| %.3g  node %.3g (%.3g of it)  aten32 %.3g (%.3g of it)  bar %.3g of it"
                   % (kind, _ids(shape), gmax, e, e / gmax, e_aten, e_aten / gmax, BAR))
    assert torch.isfinite(g).all() and gmax > 0
    assert e <= BAR * gmax
    if e_aten > BAR * gmax:
        assert e <= e_aten


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_identical_pairs_have_no_gradient(shape):
    """the true gradient is zero (every window is at the maximum); what is left is float64 noise, nine orders below the bound"""
    B, C, H, W = shape
    for kind in ("uniform", "mixed"):
        a = pair(kind, shape)[0].to(DEV)
        s, g = _node_grad(a, a.clone(), weights(B).to(DEV))
        assert torch.equal(s, torch.ones_like(s))
        assert torch.isfinite(g).all() and float(g.abs().max()) <= BAR / (C * (H - 10) * (W - 10)), float(g.abs().max())


def test_every_element_is_written_and_the_bits_repeat():
    for shape in SHAPES:
        a, b = (t.to(DEV) for t in pair("mixed", shape))
        w = weights(shape[0]).to(DEV)
        outs = [torch.full(shape, float("nan"), device=DEV) for _ in range(2)]
        for o in outs:
            assert ssim_ops.ssim_grad(w, a, b, out=o) is o
        assert not torch.isnan(outs[0]).any(), shape
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        # a permuted view of the first image (how the stage-one patch arrives) is made contiguous inside: the same bits
        nhwc = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not nhwc.is_contiguous() or shape[1] == 1
        s, g = _node_grad(nhwc, b, w)
        assert torch.equal(g, outs[0]) and torch.equal(s, metrics.ssim(a, b))


def test_unaligned_views_take_the_narrow_accesses_and_agree():
    """a pair whose storage starts 4 bytes off a 16-byte boundary (W % 4 == 0): the 4- and 8-byte template, the same bits"""
    shape = (2, 3, 64, 64)
    a, b = pair("uniform", shape)
    buf_a, buf_b = torch.empty(a.numel() + 1, device=DEV), torch.empty(b.numel() + 1, device=DEV)
    va, vb = buf_a[1:].view(shape), buf_b[1:].view(shape)
    va.copy_(a); vb.copy_(b)
    assert va.data_ptr() % 16 == 4 and va.is_contiguous()
    w = weights(2).to(DEV)
    assert torch.equal(ssim_ops.ssim_grad(w, va, vb), ssim_ops.ssim_grad(w, a.to(DEV), b.to(DEV)))


def test_side_stream_and_graph_replays_return_the_eager_bits():
    shape = (2, 3, 64, 64)
    pairs = [tuple(t.to(DEV) for t in pair(k, shape)) for k in ("uniform", "mixed")]
    w = weights(2).to(DEV)
    eager = [_node_grad(a, b, w) for a, b in pairs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s, g = _node_grad(*pairs[0], w)
    side.synchronize()
    assert torch.equal(s, eager[0][0]) and torch.equal(g, eager[0][1])
    # capture forward and backward on one stream, replay on two different inputs
    sa, sb = pairs[0][0].clone().requires_grad_(True), pairs[0][1].clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs = ssim_ops.ssim_mean(sa, sb)
        gg, = torch.autograd.grad(gs, sa, grad_outputs=w)
    for k in (1, 0):
        with torch.no_grad():
            sa.copy_(pairs[k][0]); sb.copy_(pairs[k][1])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gs.detach(), eager[k][0]) and torch.equal(gg, eager[k][1])


def test_routing(monkeypatch):
    calls = []
    real_node, real_f = ssim_ops.ssim_mean, metrics_ops.image_metrics_f32
    monkeypatch.setattr(ssim_ops, "ssim_mean", lambda *a, **k: (calls.append("node"), real_node(*a, **k))[1])
    monkeypatch.setattr(metrics_ops, "image_metrics_f32", lambda *a, **k: (calls.append("f32"), real_f(*a, **k))[1])
    monkeypatch.delenv("HAVATAR_METRICS", raising=False)
    shape = (2, 3, 24, 28)
    a, b = (t.to(DEV) for t in pair("uniform", shape))
    x64 = pair("uniform", shape)[0].double().requires_grad_(True)
    l64 = 1.0 - metrics.aten_statement(x64, pair("uniform", shape)[1].double())[0].mean()
    g64, = torch.autograd.grad(l64, x64)

    def close(loss, grad, tol):
        assert loss.dim() == 0 and abs(float(loss.detach()) - float(l64.detach())) <= tol
        assert float((grad.double().cpu() - g64).abs().max()) <= tol * max(float(g64.abs().max()), 1.0)

    # a float32 HIP pair whose first image needs a gradient: the node, once (its forward is the metric's entry)
    x = a.clone().requires_grad_(True)
    loss = metrics.ssim_loss(x, b)
    assert calls == ["node", "f32"] and loss.dtype == torch.float32
    close(loss, torch.autograd.grad(loss, x)[0], 1e-6)
    # second order through the node is refused, and the message names the other route
    loss = metrics.ssim_loss(x, b)
    with pytest.raises(RuntimeError, match=r"once differentiable.*HAVATAR_METRICS=0"):
        torch.autograd.grad(loss, x, create_graph=True)
    calls.clear()
    # the switch, other dtypes, a target that needs a gradient: the statement under autograd, and its gradient arrives
    monkeypatch.setenv("HAVATAR_METRICS", "0")
    loss = metrics.ssim_loss(x, b)
    close(loss, torch.autograd.grad(loss, x)[0], 1e-4)
    monkeypatch.delenv("HAVATAR_METRICS")
    xd = a.double().requires_grad_(True)
    loss = metrics.ssim_loss(xd, b.double())
    assert loss.dtype == torch.float64
    close(loss, torch.autograd.grad(loss, xd)[0], 1e-10)
    y = b.clone().requires_grad_(True)
    loss = metrics.ssim_loss(x, y)
    gx, gy = torch.autograd.grad(loss, (x, y))
    close(loss, gx, 1e-4)
    assert torch.isfinite(gy).all() and float(gy.abs().max()) > 0
    assert calls == []
    # nothing needs a gradient: metrics.ssim, the native entry without the node
    with torch.no_grad():
        l0 = metrics.ssim_loss(x, b)
    l1 = metrics.ssim_loss(a, b)
    assert calls == ["f32", "f32"] and not l0.requires_grad and torch.equal(l0, l1) and abs(float(l0) - float(l64.detach())) <= 1e-6
    # refused on every route, by shape
    for env in ("1", "0"):
        monkeypatch.setenv("HAVATAR_METRICS", env)
        with pytest.raises(ValueError, match=r"H, W >= 11.*\(1, 3, 10, 64\)"):
            metrics.ssim_loss(torch.zeros(1, 3, 10, 64, device=DEV, requires_grad=True), torch.zeros(1, 3, 10, 64, device=DEV))
    with pytest.raises(RuntimeError, match="not covered"):
        ssim_ops.ssim_grad(torch.ones(1, device=DEV), torch.zeros(1, 3, 10, 64, device=DEV), torch.zeros(1, 3, 10, 64, device=DEV))


# ------------------------------------------------------------------------------------------------------------------------------------
# the training steps
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ssim_dataset"))
    return root, synth.write_dataset(root, n_frames=2, img_res=128)


def _probe(monkeypatch, calls):
    real = ssim_ops.ssim_mean
    monkeypatch.setattr(ssim_ops, "ssim_mean", lambda p, t, *a, **k: (calls.append((tuple(p.shape), p.requires_grad, t.requires_grad)),
                                                                     real(p, t, *a, **k))[1])


def test_stage_two_step_reaches_the_node_once(dataset, monkeypatch):
    """joint_step with ssim_weight on the synthetic 32 -> 128 case: one call on the [B,3,128,128] pair, a finite scalar, finite gradients"""
    from havatar_amd.harness import stage2_step_cases, train_hd
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.model.styleUnet import Discriminator, SWGAN_unet
    from havatar_amd.utils import styleUnet_util
    calls = []
    _probe(monkeypatch, calls)
    cfg, su_args, nets, optims, batch = stage2_step_cases.build(Trainer, SWGAN_unet, Discriminator, styleUnet_util, dataset[1], device=DEV,
                                                                pinned=True)
    grads = {}
    s = train_hd.joint_step(1, batch, nets, optims, cfg, su_args, None, ssim_weight=0.2,
                            probe=lambda name: grads.update({n: p.grad.detach().clone() for n, p in nets["generator"].named_parameters()
                                                             if p.grad is not None}) if name == "g_backward" else None)
    assert calls == [((2, 3, 128, 128), True, False)]
    assert np.isfinite(s["ssim_loss"]) and 0 < s["ssim_loss"] < 2 and np.isfinite(s["g_loss"])
    assert len(grads) > 0 and all(bool(torch.isfinite(g).all()) for g in grads.values())


def _patch_cfg(root):
    cfg = synth.harness_config(render_size=128, img_res=128)
    cfg["experiment"].update(patch_rgb=True)
    path = os.path.join(root, "cfg_patch.yml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path, cfg


def test_stage_one_cli_in_graph_mode(dataset, tmp_path, monkeypatch, capsys):
    """train_avatar's counterpart with the term inside the captured step: 4 steps (2 eager, the capture, replays), finite losses"""
    from havatar_amd.harness import train
    monkeypatch.setenv("HAVATAR_PRETRAIN_WC", "2")
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    monkeypatch.delenv("HAVATAR_TRAIN_GRAPH", raising=False)
    calls, scalars = [], []
    _probe(monkeypatch, calls)

    class Recorder:
        def add_scalar(self, name, value, step):
            scalars.append((name, float(value), int(step)))

        add_image = add_scalar

    monkeypatch.setattr(train, "make_writer", lambda logdir: Recorder())
    runners, real = [], train.StepRunner
    monkeypatch.setattr(train, "StepRunner", lambda *a, **k: (runners.append(real(*a, **k)), runners[-1])[1])
    cfg_path, _ = _patch_cfg(dataset[0])
    last = train.main(["--logdir", str(tmp_path / "log"), "--datadir", dataset[0], "--config", cfg_path, "--percep", "none", "--ssim-weight", "0.2",
                       "--val-metrics", "--max-steps", "4"], device=DEV)
    assert last == 3 and runners[0].graphed is not None and runners[0].ssim_weight == 0.2
    assert calls == [((2, 3, 64, 64), True, False)] * 3          # two eager steps and the capture; the replays call nothing
    terms = [v for n, v, _ in scalars if n == "train/patch_ssim_loss"]
    assert len(terms) == 4 and all(np.isfinite(v) and 0 < v < 2 for v in terms), terms
    assert all(np.isfinite(v) for _, v, _ in scalars)
    assert [n for n, _, _ in scalars].count("validation/ssim") == 1
    assert "nan" not in capsys.readouterr().out.lower()


def test_stage_one_captured_step_equals_the_eager_step(dataset, monkeypatch):
    """three steps from the same state, eager against (2 eager + 1 replayed): the loss of the first replayed iteration to the 1 % that
    tests/test_harness.py::test_training_steps_as_one_hipgraph_launch_follow_the_eager_trajectory allows without the term (fp32 MLP, as there)"""
    from havatar_amd.dataloader.dataloader import Loader
    from havatar_amd.harness import train
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    monkeypatch.setenv("HAVATAR_TRAIN_MLP", "torch")
    cfg = synth.harness_config(render_size=128, img_res=128)
    cfg["experiment"].update(patch_rgb=True)
    cfg = CfgNode(cfg)
    np.random.seed(7)
    tl = Loader(split_file=dataset[1], mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg, white_bg=True,
                shuffle=False)
    idx, batch = next(iter(tl))
    calls = []
    _probe(monkeypatch, calls)
    curves, terms = [], []
    for graph in (False, True):
        torch.manual_seed(5)
        trainer = synth.fill_state_dict(Trainer(cfg, len(tl.dataset))).to(DEV).train()
        opt = train.make_optimizer(cfg, trainer, graph)
        run = train.StepRunner(trainer, cfg, opt, torch.nn.functional.mse_loss, graph=graph, ssim_weight=0.2)
        inp, target, mask = train.step_inputs(idx, batch, DEV)
        losses, ssims = [], []
        for k in range(3):
            loss, parts, psnr = run(inp, target, mask)
            losses.append(loss.item())
            ssims.append(parts["patch_ssim_loss"].item())
        assert (run.graphed is not None) == graph
        curves.append(losses)
        terms.append(ssims)
    helpers.report("ssim_loss stage-one step: eager losses %s terms %s | graph losses %s terms %s" % (curves[0], terms[0], curves[1], terms[1]))
    assert len(calls) == 6          # eager: three; graph: two eager and the capture
    assert all(np.isfinite(v) for c in curves + terms for v in c)
    assert abs(curves[0][2] - curves[1][2]) <= 1e-2 * abs(curves[0][2]), curves
    assert abs(terms[0][2] - terms[1][2]) <= 1e-2 * abs(terms[0][2]), terms

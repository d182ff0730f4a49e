"""GPU: compositing for up to 128 samples per ray (hav_composite_long_*, csrc/hav_composite_long.hip) and its way into the Trainer
(HAVATAR_COMPOSITE_LONG=1).  Reference and bar are those of tests/test_ops_gpu.py::test_composite_forward_and_gradients_...: truth is
volume_render_radiance_field under ATen autograd in fp64, the yardstick the same statement in fp32, every one of the four maps carries
an upstream gradient, and per output  e_mine <= max(2 e_aten, 4e-6)  relative to the largest fp64 magnitude.  Every branch is reached by
shape (or, for the backward's arrangements, by hav_composite_long_bwd_form); each test asserts the launcher's own inequality that puts
it there.  The launcher's formulas, restated: a ray's staged block is pitch = roundup4(S (CH+1) + (CH+1)) floats + 1 KB per wave;
by shape the backward stages while pitch*4 + 1024 <= 64 KiB; grids are capped at 16 workgroups per CU (forward and direct backward:
4 waves each; staged, one wave: 1 wave each) and 8 per CU (staged, two waves)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from havatar_amd import synth
from helpers import report

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HAV_EUNSUP = -2
NAMES = ("rgb", "acc", "weights", "depth", "d_rf")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lds_one_wave(S, CH):
    """bytes of LDS one wave of the staged backward takes (hav_composite_long_bwd_form)"""
    return ((S * (CH + 1) + (CH + 1) + 3) // 4 * 4) * 4 + 2 * 128 * 4


def _staged_by_shape(S, CH):
    return _lds_one_wave(S, CH) <= 64 * 1024


def _inputs(n, S, CH, use_noise, use_bg, seed):
    """as tests/test_ops_gpu.py draws them: rf = 2 randn, z sorted in [3.4, 6.0], rd = randn, noise 0.5"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rf = (torch.randn(n, S, CH + 1, device=DEV, generator=g) * 2).requires_grad_(True)
    z = torch.sort(torch.rand(n, S, device=DEV, generator=g) * 2.6 + 3.4, -1)[0]
    rd = torch.randn(n, 3, device=DEV, generator=g)
    noise = torch.randn(n, S, device=DEV, generator=g) * 0.5 if use_noise else None
    bg = torch.rand(n, 3, device=DEV, generator=g) if use_bg else None
    ups = [torch.randn(s, device=DEV, generator=g) for s in ((n, CH), (n,), (n, S), (n,))]
    return rf, z, rd, noise, bg, ups


def _aten(rf, z, rd, noise, bg, ups, dt, act_feat=False):
    from havatar_amd.utils.nerf_util import volume_render_radiance_field
    r = rf.detach().to(dt).requires_grad_(True)
    r2 = r + 0                                               # the reference sigmoids its radiance field in place
    if noise is not None:                                    # inject the draw: sigma = relu(raw + noise)
        r2 = torch.cat([r2[..., :-1], r2[..., -1:] + noise.to(dt)[..., None]], -1)
    rgb, _, acc, w, depth = volume_render_radiance_field(r2, z.to(dt), rd.to(dt), 0.0, act_feat=act_feat,
                                                         background_prior=bg.to(dt) if bg is not None else None)
    outs = (rgb, acc, w, depth)
    return outs + torch.autograd.grad(outs, r, [u.to(dt) for u in ups])


def _run(rf, z, rd, noise, bg, ups, n_sigmoid=3, bwd_form=0, fn=None):
    from havatar_amd.native import train_ops
    if fn is None:
        got = train_ops.CompositeLong.apply(rf, z, rd, noise, bg, n_sigmoid, bwd_form)
    else:
        got = fn(rf, z, rd, noise, bg, n_sigmoid=n_sigmoid)
    return tuple(got) + torch.autograd.grad(got, rf, ups)


def _check(tag, rf, z, rd, noise, bg, ups, n_sigmoid=3, act_feat=False, bwd_form=0):
    ref32 = _aten(rf, z, rd, noise, bg, ups, torch.float32, act_feat)
    ref64 = _aten(rf, z, rd, noise, bg, ups, torch.float64, act_feat)
    got = _run(rf, z, rd, noise, bg, ups, n_sigmoid, bwd_form)
    fails = []
    for name, mine, r32, r64 in zip(NAMES, got, ref32, ref64):
        assert torch.isfinite(r32).all() and torch.isfinite(r64).all(), (tag, name)
        scale = r64.abs().max().item()
        assert scale > 0 and mine.shape == r64.shape and torch.isfinite(mine).all(), (tag, name)
        e_mine, e_aten = (mine.double() - r64).abs().max().item() / scale, (r32.double() - r64).abs().max().item() / scale
        report("composite_long %s %s: e_mine %.2e e_aten %.2e" % (tag, name, e_mine, e_aten))
        if not e_mine <= max(2.0 * e_aten, 4e-6):
            fails.append((name, e_mine, e_aten))
    assert not fails, (tag, fails)
    return got


SHAPES = [(5, 65, 3), (333, 80, 68), (211, 127, 67), (211, 127, 68), (333, 128, 68), (97, 128, 200), (300, 64, 68), (300, 7, 3)]


@pytest.mark.parametrize("use_bg", [True, False])
@pytest.mark.parametrize("use_noise", [True, False])
@pytest.mark.parametrize("n,S,CH", SHAPES)
def test_forward_and_gradients_match_volume_render_radiance_field(n, S, CH, use_noise, use_bg):
    """65 x 4: the first slot of the upper half alone (260 floats: they move as vectors).  80 x 69: the fine pass of a 64+48 step.  127 x 68: odd S, a block of
    8 636 floats, vector copy; 127 x 69 = 8 763: scalar copy.  128 x 69: the limit.  128 x 201: a block past the staged form's LDS.
    64 x 69 and 7 x 4: ground shared with hav_composite_*, where the two pairs also agree with each other to 1e-5 of the scale."""
    assert _staged_by_shape(S, CH) == ((S, CH) != (128, 200))
    assert ((S * (CH + 1)) % 4 == 0) == ((S, CH) != (127, 68))          # 16-byte vectors everywhere but at 127 x 69
    args = _inputs(n, S, CH, use_noise, use_bg, seed=1000 + S + CH)
    got = _check("n%d S%d CH%d noise%d bg%d" % (n, S, CH, use_noise, use_bg), *args)
    if S <= 64:
        from havatar_amd.native.train_ops import composite
        old = _run(*args, fn=composite)
        for name, a, b in zip(NAMES, got, old):
            scale = b.abs().max().item()
            d = (a - b).abs().max().item()
            report("composite_long vs composite S%d %s: %.2e of the scale" % (S, name, d / scale))
            assert d <= 1e-5 * scale, (name, d / scale)


def _bwd_raw(d_rf, ups, rf, z, rd, noise, bg, n_sigmoid=3, null_upstream=False, form=None):
    """hav_composite_long_bwd[_form] through the C ABI: the only way to null upstream pointers"""
    from havatar_amd import _lib
    n, S, RW = rf.shape
    d_rgb, d_acc, d_w, d_depth = ups
    if null_upstream:
        d_acc = d_w = d_depth = None
    L = _lib.lib()
    with torch.cuda.device(DEV):
        if form is None:
            rc = L.hav_composite_long_bwd(_p(d_rf), _p(d_rgb), _p(d_acc), _p(d_w), _p(d_depth), _p(rf), _p(z), _p(rd), _p(noise), _p(bg),
                                          n, S, RW - 1, n_sigmoid, _stream())
        else:
            rc = L.hav_composite_long_bwd_form(_p(d_rf), _p(d_rgb), _p(d_acc), _p(d_w), _p(d_depth), _p(rf), _p(z), _p(rd), _p(noise), _p(bg),
                                               n, S, RW - 1, n_sigmoid, form, _stream())
    torch.cuda.synchronize()
    return rc, d_rf


@pytest.mark.parametrize("n,S,CH", [(40, 128, 67), (50, 65, 3), (9, 128, 200)])
def test_null_upstream_gradients_mean_zeros(n, S, CH):
    """d_acc = d_weights = d_depth absent: through autograd with only rgb used (within the bar of the ATen statement), and through the C
    ABI with null pointers against zero tensors (the same bits); staged with the vector copy, staged with an odd S, direct"""
    rf, z, rd, noise, bg, ups = _inputs(n, S, CH, True, True, seed=2000 + S)
    from havatar_amd.native.train_ops import composite_long
    zeros = [ups[0]] + [torch.zeros_like(u) for u in ups[1:]]
    rgb = composite_long(rf, z, rd, noise, bg)[0]
    (d_auto,) = torch.autograd.grad(rgb, rf, ups[0])
    r32, r64 = _aten(rf, z, rd, noise, bg, zeros, torch.float32)[4], _aten(rf, z, rd, noise, bg, zeros, torch.float64)[4]
    scale = r64.abs().max().item()
    e_mine, e_aten = (d_auto.double() - r64).abs().max().item() / scale, (r32.double() - r64).abs().max().item() / scale
    report("composite_long rgb-only S%d CH%d d_rf: e_mine %.2e e_aten %.2e" % (S, CH, e_mine, e_aten))
    assert e_mine <= max(2.0 * e_aten, 4e-6)
    rfd = rf.detach()
    rc_a, a = _bwd_raw(torch.empty_like(rfd), zeros, rfd, z, rd, noise, bg)
    rc_b, b = _bwd_raw(torch.empty_like(rfd), zeros, rfd, z, rd, noise, bg, null_upstream=True)
    assert rc_a == 0 and rc_b == 0
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    assert torch.equal(a, b) and torch.equal(a, d_auto)


@pytest.mark.parametrize("n,S,CH", [(60, 97, 68), (9, 128, 200)])
def test_zero_upstream_gradient_gives_exactly_zero(n, S, CH):
    rf, z, rd, noise, bg, ups = _inputs(n, S, CH, True, True, seed=2100 + S)
    got = _run(rf, z, rd, noise, bg, [torch.zeros_like(u) for u in ups])
    assert (got[4] == 0).all()


@pytest.mark.parametrize("n,S,CH,n_sigmoid,act_feat", [(50, 80, 5, 5, True), (50, 80, 5, 0, None), (40, 97, 68, 68, True), (40, 97, 68, 0, None)])
def test_activation_variants(n, S, CH, n_sigmoid, act_feat):
    """n_sigmoid = CH against the reference's act_feat=True, n_sigmoid = 0 against act_feat=None"""
    _check("nsig%d n%d S%d CH%d" % (n_sigmoid, n, S, CH), *_inputs(n, S, CH, True, True, seed=2200 + S + n_sigmoid),
           n_sigmoid=n_sigmoid, act_feat=act_feat)


@pytest.mark.parametrize("n,S,CH", [(300, 128, 67), (84, 97, 4)])
def test_saturated_rays(n, S, CH):
    """As tests/test_train_edges_gpu.py::test_composite_saturated_rays builds them: ray r carries a run of r % 7 consecutive samples of raw
    density 6000 (alpha = 1 exactly in fp32, 1 - alpha + 1e-10 at its floor; runs of 5 and 6 take the transmittance through the
    subnormals to 0), every third ray repeats two depths, every eleventh has no density.  The run starts, in turn, in the lower half
    (sample 10: the first of a lane's pair; 33: the second, so the pair straddles the floor), across the two halves (63), and in the
    upper half (90 and 95, even and odd).  Depths at least half a bin apart and |rd| >= 0.8: 6000 x distance >= 38 on every sample of
    a run at S = 128.  Everything finite and inside the usual bar."""
    g = torch.Generator(device=DEV).manual_seed(2300 + S)
    rf = torch.randn(n, S, CH + 1, device=DEV, generator=g) * 2
    z = 3.4 + 2.6 * (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(n, S, device=DEV, generator=g)) / S
    rd = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=-1) * (0.8 + 0.4 * torch.rand(n, 1, device=DEV, generator=g))
    bg = torch.rand(n, 3, device=DEV, generator=g)
    ups = [torch.randn(s, device=DEV, generator=g) for s in ((n, CH), (n,), (n, S), (n,))]
    starts = (10, 33, 63, 90, 95)
    assert 6000 * 0.5 * 2.6 / 128 * 0.8 >= 38
    for r in range(n):
        run = r % 7
        if run:
            s0 = min(starts[(r // 7) % len(starts)], S - run)
            rf[r, s0:s0 + run, CH] = 6000.0
        if r % 3 == 0:
            z[r, 3] = z[r, 2]
            z[r, S - 1] = z[r, S - 2]
        if r % 11 == 0:
            rf[r, :, CH] = -rf[r, :, CH].abs()
    assert n // 7 >= len(starts)                                            # every start is used
    rf.requires_grad_(True)
    got = _check("saturated n%d S%d CH%d" % (n, S, CH), rf, z, rd, None, bg, ups)
    assert (got[1][::11] == 0).all()                                       # no density: nothing accumulated
    w = got[2]
    r = torch.arange(n, device=DEV)
    assert (w.max(-1)[0][(r % 7 > 0) & (r % 11 > 0)] > 0).all() and (w == 0).any()


@pytest.mark.parametrize("form", [1, 2, 3])
def test_second_grid_trip(form):
    """more rays than any of the capped grids has waves, at S = 65, CH = 3: the forward (4 waves x 16 workgroups per CU) and each form of
    the backward (staged, one wave: 1 x 16 per CU; staged, two waves: 2 x 8 per CU; rows from memory: 4 x 16 per CU)"""
    cus = _cus()
    n, S, CH = 4 * 16 * cus + 5, 65, 3
    assert n > 4 * 16 * cus and n > 1 * 16 * cus and n > 2 * 8 * cus
    assert _lds_one_wave(S, CH) <= 64 * 1024 and 2 * _lds_one_wave(S, CH) <= 160 * 1024
    _check("second trip form%d n%d" % (form, n), *_inputs(n, S, CH, True, True, seed=2400 + form), bwd_form=form)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_backward_forms_agree_at_the_model_size(form):
    """each arrangement of the backward at 128 x 69, named through hav_composite_long_bwd_form, inside the bar"""
    _check("form%d 128x69" % form, *_inputs(150, 128, 68, True, True, seed=2500), bwd_form=form)


def test_refusals():
    """S = 129: HAV_EUNSUP from every entry, sentinel-filled outputs untouched; composite_long raises; a staged form named for a block that
    does not fit is refused too; n = 0 gives empty outputs and an empty gradient"""
    from havatar_amd import _lib
    from havatar_amd.native.train_ops import composite_long
    n, S, CH = 4, 129, 3
    rf, z, rd = torch.randn(n, S, CH + 1, device=DEV), torch.rand(n, S, device=DEV).sort(-1)[0] + 3, torch.randn(n, 3, device=DEV)
    outs = [torch.full(s, 7.5, device=DEV) for s in ((n, CH), (n,), (n, S), (n,))]
    L = _lib.lib()
    with torch.cuda.device(DEV):
        rc = L.hav_composite_long_fwd(_p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(rf), _p(z), _p(rd), None, None, n, S, CH, 3, _stream())
    torch.cuda.synchronize()
    assert rc == HAV_EUNSUP and all((o == 7.5).all() for o in outs)
    d_rf = torch.full_like(rf, 7.5)
    ups = [torch.ones(s, device=DEV) for s in ((n, CH), (n,), (n, S), (n,))]
    for form in (None, 0, 1, 2, 3):
        rc, _ = _bwd_raw(d_rf, ups, rf, z, rd, None, None, form=form)
        assert rc == HAV_EUNSUP and (d_rf == 7.5).all(), form
    with pytest.raises(RuntimeError, match="HAV_EUNSUP"):
        composite_long(rf, z, rd)
    # 128 x 201: one wave's block is past 64 KB, two waves' past 160 KB
    rf2, z2 = torch.randn(n, 128, 201, device=DEV), torch.rand(n, 128, device=DEV).sort(-1)[0] + 3
    d2 = torch.full_like(rf2, 7.5)
    ups2 = [torch.ones(s, device=DEV) for s in ((n, 200), (n,), (n, 128), (n,))]
    assert _lds_one_wave(128, 200) > 64 * 1024 and 2 * _lds_one_wave(128, 200) > 160 * 1024
    for form in (1, 2):
        rc, _ = _bwd_raw(d2, ups2, rf2, z2, rd, None, None, form=form)
        assert rc == HAV_EUNSUP and (d2 == 7.5).all(), form
    e = torch.zeros(0, 80, 4, device=DEV, requires_grad=True)
    got = composite_long(e, torch.zeros(0, 80, device=DEV), torch.zeros(0, 3, device=DEV))
    assert [tuple(t.shape) for t in got] == [(0, 3), (0,), (0, 80), (0,)]
    (g,) = torch.autograd.grad(got, e, [torch.zeros_like(t) for t in got])
    assert tuple(g.shape) == (0, 80, 4)


def test_two_calls_give_the_same_bits():
    args = _inputs(700, 112, 68, True, True, seed=2600)
    a, b = _run(*args), _run(*args)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


def test_forward_and_backward_captured_in_one_graph_replay_the_eager_bits():
    """forward + backward captured in one torch.cuda.graph after a warm-up on a side stream, replayed twice with fresh inputs copied into
    the static buffers: both replays are bit-equal to the eager results on those inputs"""
    n, S, CH = 257, 96, 68
    static = _inputs(n, S, CH, True, True, seed=2700)
    rf, z, rd, noise, bg, ups = static
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _run(*static)
    for k in (1, 2):
        fresh = _inputs(n, S, CH, True, True, seed=2700 + k)
        with torch.no_grad():
            for dst, src in zip((rf, z, rd, noise, bg) + tuple(ups), fresh[:5] + tuple(fresh[5])):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(*fresh)
        for name, x, y in zip(NAMES, outs, eager):
            assert torch.equal(x, y), (k, name)


# =====================================================================================================================================
# the wiring: Trainer._render_torch with HAVATAR_COMPOSITE_LONG
# =====================================================================================================================================
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("dataset_long")
    return str(root), synth.write_dataset(str(root), n_frames=2, img_res=128)


def _train_step(dataset, tag, num_coarse, num_fine):
    """tests/test_harness.py::_train_step with the sample counts set"""
    from havatar_amd.dataloader.dataloader import Loader
    from havatar_amd.harness import train
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    perturb, noise = (False, 0.0) if tag == "det" else (True, 0.1)
    cfgd = synth.harness_config(perturb=perturb, noise_std=noise)
    cfgd["nerf"]["train"].update(num_coarse=num_coarse, num_fine=num_fine)
    cfg = CfgNode(cfgd)
    np.random.seed(7)
    tl = Loader(split_file=dataset[1], mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg,
                white_bg=True, shuffle=False)
    idx, batch = next(iter(tl))
    torch.manual_seed(5)
    trainer = synth.fill_state_dict(Trainer(cfg, len(tl.dataset))).to("cuda")
    trainer.train()
    inp, target, ray_mask = train.step_inputs(idx, batch, "cuda")
    torch.manual_seed(123)
    loss, parts, _ = train.training_loss(trainer, cfg, inp, target, ray_mask, torch.nn.functional.mse_loss)
    trainer.model_coarse.triPlane_embeddings.retain_grad()
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in trainer.named_parameters() if p.grad is not None}
    grads["planes"] = trainer.model_coarse.triPlane_embeddings.grad.detach().clone()
    return loss.item(), {k: v.item() for k, v in parts.items()}, grads


def _count_calls(monkeypatch):
    from havatar_amd.native import train_ops
    calls, real = [], train_ops.composite_long
    monkeypatch.setattr(train_ops, "composite_long", lambda *a, **k: (calls.append(a[1].shape[-1]), real(*a, **k))[1])
    return calls


def _compare_steps(a, b, loss_tol, grad_tol, planes_tol=None):
    (l0, p0, g0), (l1, p1, g1) = a, b
    assert abs(l0 - l1) <= loss_tol * abs(l0), (l0, l1)
    for k in p0:
        assert abs(p0[k] - p1[k]) <= loss_tol * max(abs(p0[k]), 1e-3), (k, p0[k], p1[k])
    assert g0.keys() == g1.keys() and len(g0) == 154
    worst = ("", 0.0)
    for n in g0:
        if n.startswith("headpose_skin_net.canonical_Wvolume.filters") and n.endswith(".bias"):
            continue                                   # a bias in front of InstanceNorm3d: its gradient is zero up to rounding
        scale = g0[n].abs().max().item()
        d = (g0[n] - g1[n]).abs().max().item()
        if d / max(scale, 1e-30) > worst[1]:
            worst = (n, d / max(scale, 1e-30))
        tol = planes_tol if (planes_tol and (n == "planes" or n.startswith("headpose_skin_net."))) else grad_tol
        assert d <= tol * scale + 1e-12, (n, d / max(scale, 1e-30))
    return worst


@pytest.mark.parametrize("tag", ["det", "rnd"])
@pytest.mark.parametrize("num_coarse,num_fine", [(64, 48), (64, 41), (96, 80)])
def test_training_step_with_the_switch_equals_the_aten_statement(dataset, monkeypatch, tag, num_coarse, num_fine):
    """64+48 (fine pass 80), 64+41 (73: no multiple of 16) and 96+80 (96 and 128) through the native route with HAVATAR_COMPOSITE_LONG=1
    against HAVATAR_HIP_TRAIN=0, the MLP fp32 nn.Linear on both sides: the bars of
    test_training_step_gpu_fused_field_ops_equal_the_aten_statement (loss and parts 1e-5, every gradient 2e-2 of its scale)."""
    calls = _count_calls(monkeypatch)
    monkeypatch.setenv("HAVATAR_TRAIN_MLP", "torch")
    monkeypatch.setenv("HAVATAR_COMPOSITE_LONG", "1")
    native = _train_step(dataset, tag, num_coarse, num_fine)
    fine = (num_coarse + 1) // 2 + num_fine
    assert sorted(calls) == sorted(s for s in (num_coarse, fine) if s > 64), calls          # passes above 64 samples, and only those
    n_calls = len(calls)
    monkeypatch.setenv("HAVATAR_HIP_TRAIN", "0")
    aten = _train_step(dataset, tag, num_coarse, num_fine)
    assert len(calls) == n_calls                                                             # never in the second run
    worst = _compare_steps(aten, native, 1e-5, 2e-2)
    report("composite_long step %d+%d %s: loss %.8f vs %.8f, worst gradient %s %.2e of its scale" % (
        num_coarse, num_fine, tag, aten[0], native[0], worst[0], worst[1]))


def test_without_the_switch_a_wide_step_takes_the_aten_statement_and_says_so_once(dataset, monkeypatch):
    from havatar_amd.model import nerf_trainer
    calls = _count_calls(monkeypatch)
    monkeypatch.setattr(nerf_trainer, "_warned_wide_sampling", False)
    monkeypatch.delenv("HAVATAR_COMPOSITE_LONG", raising=False)
    monkeypatch.setenv("HAVATAR_TRAIN_MLP", "torch")
    with pytest.warns(RuntimeWarning, match="HAVATAR_COMPOSITE_LONG=1"):
        _train_step(dataset, "det", 64, 48)
    assert not calls
    with warnings.catch_warnings(record=True) as rec:          # once per process
        warnings.simplefilter("always")
        _train_step(dataset, "det", 64, 48)
    assert not [w for w in rec if "HAVATAR_COMPOSITE_LONG" in str(w.message)] and not calls


def test_with_the_switch_a_64_16_step_keeps_its_bits(dataset, monkeypatch):
    """64+16 (passes of 64 and 48) never reaches composite_long, and loss and gradients are bit-equal to the switch unset.  Both runs
    under HAVATAR_DETERMINISTIC=1: without it the float atomics of the field-input scatter and MIOpen's solver choice make two runs
    of the SAME route differ (tests/test_harness.py::test_deterministic_switch_...), which would say nothing about the switch."""
    from havatar_amd.harness import train
    calls = _count_calls(monkeypatch)
    monkeypatch.setenv("HAVATAR_DETERMINISTIC", "1")
    train.enable_determinism(True)
    try:
        monkeypatch.delenv("HAVATAR_COMPOSITE_LONG", raising=False)
        unset = _train_step(dataset, "rnd", 64, 16)
        monkeypatch.setenv("HAVATAR_COMPOSITE_LONG", "1")
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            on = _train_step(dataset, "rnd", 64, 16)
        assert not [w for w in rec if "HAVATAR_COMPOSITE_LONG" in str(w.message)]
    finally:
        train.enable_determinism(False)
    assert not calls
    assert unset[0] == on[0] and unset[1] == on[1] and unset[2].keys() == on[2].keys()
    differ = [n for n in unset[2] if not torch.equal(unset[2][n], on[2][n])]
    assert not differ, differ[:8]


def test_training_step_bf16_mlp_with_the_switch(dataset, monkeypatch):
    """64+48 under the default bf16-MFMA radiance MLP (FieldMlp rows of 80 samples per ray) against the ATen route: the 2e-2 / 6e-2 bars
    of tests/test_harness.py::test_training_step_gpu (6e-2 on what reaches its tensor through dX: planes and the skinning volume)"""
    calls = _count_calls(monkeypatch)
    monkeypatch.delenv("HAVATAR_TRAIN_MLP", raising=False)
    monkeypatch.setenv("HAVATAR_COMPOSITE_LONG", "1")
    native = _train_step(dataset, "det", 64, 48)
    assert calls == [80]
    monkeypatch.setenv("HAVATAR_HIP_TRAIN", "0")
    aten = _train_step(dataset, "det", 64, 48)
    worst = _compare_steps(aten, native, 2e-2, 2e-2, planes_tol=6e-2)
    report("composite_long step 64+48 bf16 MLP: loss %.6f vs %.6f, worst gradient %s %.2e of its scale" % (aten[0], native[0], worst[0], worst[1]))

"""The G-buffer kernel (csrc/hav_gbuffer.hip) on the device: against the float32 statement on the CPU (z, mask, decisions and depth codes bit-equal)
and the float64 statement given float32's decisions (normals within their bar, with the CPU float32 statement as the yardstick) at every tile
edge on seven kinds of scene; every element written and nothing beyond; bit reproducibility, a side stream, a captured graph; routing and
refusals; Trainer.forward(return_depth=True) and avatarHD_reenactment.py --gbuffer on the device."""
import os

import numpy as np
import pytest
import torch

import gbuffer_util as gu
import iso_util as iu
from havatar_amd import geometry
from havatar_amd.native import gbuffer_ops
from test_gbuffer_cpu import SYNTH_ACC_MIN, _cli_runner, _read_maps, check_cli

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = gbuffer_ops.tile()
SHAPES = ([(1, 1), (1, 5), (5, 1), (2, 2)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)]
          + [(2 * TH + 1, 2 * TW + 3), (33, 31), (128, 128), (3, 12)])          # (3,12): dword stores in a tile the image does not fill
COMBOS = [(1, 8), (3, 11), (1, 11), (3, 8)]          # (B, stride)
SENTINEL = {"z": -1e30, "normal": -1e30, "mask": 0xEE, "depth16": 0x5A, "normal8": 0x5A, "shade8": 0x5A, "choice": 0xEE}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev(scene):
    return tuple(t.to(DEV) for t in scene)


@pytest.mark.parametrize("kind", gu.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_native_equals_the_statements(shape, kind):
    """z, mask, the decisions and depth16: the bits of the float32 statement on the CPU.  Normals: unit or zero; the angle to the float64
    statement (given float32's decisions) at most bar = 2 (Ey lx + ly Ex + 8u lx ly) / length + 1e-6 wherever that is below 0.1 rad, which
    must cover 95 % of the pixels with a normal; the worst angle / bar at most twice the CPU float32 statement's on the same scene plus 0.01.
    normal8 and shade8 within one code of the float64 statement's."""
    H, W = shape
    for B, stride in COMBOS:
        y = gu.yardsticks(kind, B, H, W, stride)
        s32, s64, tol = y["s32"], y["s64"], y["bar"]
        rays, depth, acc = _dev(gu.scene(kind, B, H, W, stride))
        got = {k: v.cpu() for k, v in gbuffer_ops.gbuffer(rays, depth, acc, H, W, 0.5).items()}
        assert torch.equal(_bits(got["z"]), _bits(s32.z)) and torch.equal(got["mask"], s32.mask)
        assert torch.equal(got["choice"], y["choice"]) and torch.equal(got["depth16"], s32.depth16)
        has = (got["mask"] & 2) != 0
        norm = got["normal"].double().norm(dim=-1)
        assert float((norm[has] - 1).abs().max()) <= 1e-6 if bool(has.any()) else True
        assert not bool(got["normal"][~has].any())
        worst, share = gu.normal_ratio(got["normal"], got["mask"], s64, y["aux64"], tol)
        same = torch.equal(_bits(got["normal"]), _bits(s32.normal))
        print("%s %dx%d B=%d stride=%d: %d normals, worst angle / bar %.4f (CPU float32 statement %.4f), asserted %.1f %%, normals %s the CPU "
              "float32 statement's bits" % (kind, H, W, B, stride, int(has.sum()), worst, y["ratio32"], 100 * share, "are" if same else "are not"))
        assert share >= 0.95
        assert worst <= 1.0 and worst <= 2.0 * y["ratio32"] + 0.01
        # the byte maps: where both evaluations have a normal and its sign is decided beyond the bar
        free = y["aux64"]["ndot"].abs() / y["aux64"]["length"] <= tol
        cmp = has & ((s64.mask & 2) != 0) & ~free
        for k, ref in (("normal8", s64.normal8), ("shade8", s64.shade8)):
            diff = (got[k].to(torch.int32) - ref.to(torch.int32)).abs()
            assert int(diff[cmp].max()) <= 1 if bool(cmp.any()) else True, k
        assert bool((got["shade8"][~has] == 255).all()) and not bool(got["normal8"][~has].any())
        if kind == "degenerate":
            assert not bool(has.any()) and bool((got["mask"] == 1).all())
        # the public entry takes the kernel and returns the same bits
        pub = geometry.gbuffer(rays, depth, acc, H, W, 0.5)
        assert all(torch.equal(_bits(getattr(pub, k).cpu()), _bits(got[k])) for k in pub._fields)


def _guarded(B, H, W, lead, names, sentinel=None):
    """sentinel-filled flat buffers with `lead` elements in front of and 64 behind each output, and the views the kernel writes"""
    bufs, views = {}, {}
    for k in names:
        tail, dt = gbuffer_ops.OUTPUTS[k]
        n = B * H * W * int(np.prod(tail, dtype=np.int64))
        unit = 1 if dt == torch.uint8 else 4          # float buffers stay dword-aligned; byte buffers start at any byte
        lead_k = lead if unit == 1 else (lead + 3) // 4 * 4
        bufs[k] = torch.full((lead_k + n + 64,), SENTINEL[k] if sentinel is None else sentinel[k], dtype=dt, device=DEV)
        views[k] = bufs[k][lead_k:lead_k + n].view((B, H, W) + tail)
    return bufs, views


@pytest.mark.parametrize("kind,B,H,W,stride,lead", [("sprinkled", 3, 5, 67, 11, 0), ("holes", 1, 9, 128, 8, 64), ("holes", 1, 9, 128, 8, 3),
                                                     ("noise", 2, 33, 31, 8, 64), ("sphere", 1, 3, 12, 8, 64)])
def test_every_element_is_written_and_nothing_beyond(kind, B, H, W, stride, lead):
    rays, depth, acc = _dev(gu.scene(kind, B, H, W, stride))
    want = gbuffer_ops.gbuffer(rays, depth, acc, H, W, 0.5)
    names = list(gbuffer_ops.OUTPUTS)
    other = {"z": 1e30, "normal": 1e30, "mask": 0xDD, "depth16": 0xA5, "normal8": 0xA5, "shade8": 0xA5, "choice": 0xDD}
    for sentinel in (SENTINEL, other):          # two fillings: an element that equals `want` under both was written
        bufs, views = _guarded(B, H, W, lead, names, sentinel)
        gbuffer_ops.gbuffer_into(views, rays, depth, acc, H, W, 0.5)
        for k in names:
            n = views[k].numel()
            lead_k = bufs[k].numel() - n - 64
            assert torch.equal(_bits(views[k]), _bits(want[k])), k
            assert bool((bufs[k][:lead_k] == sentinel[k]).all()) and bool((bufs[k][lead_k + n:] == sentinel[k]).all()), k
    # an output that is not asked for is not written, and the others do not change
    bufs, views = _guarded(B, H, W, lead, names)
    part = {k: views[k] for k in ("z", "depth16", "shade8")}
    gbuffer_ops.gbuffer_into(part, rays, depth, acc, H, W, 0.5)
    for k in names:
        if k in part:
            assert torch.equal(_bits(views[k]), _bits(want[k])), k
        else:
            assert bool((bufs[k] == SENTINEL[k]).all()), k
    for k in names:          # each output alone
        bufs, views = _guarded(B, H, W, lead, [k])
        gbuffer_ops.gbuffer_into({k: views[k]}, rays, depth, acc, H, W, 0.5)
        assert torch.equal(_bits(views[k]), _bits(want[k])), k


def test_two_launches_a_side_stream_and_graph_replays_return_the_eager_bits():
    B, H, W = 3, 2 * TH + 1, 2 * TW + 3
    scenes = [_dev(gu.scene(k, B, H, W, 8)) for k in ("sprinkled", "noise")]
    eager = [gbuffer_ops.gbuffer(*s, H, W, 0.5) for s in scenes]
    again = gbuffer_ops.gbuffer(*scenes[0], H, W, 0.5)
    assert all(torch.equal(_bits(again[k]), _bits(eager[0][k])) for k in again)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = gbuffer_ops.gbuffer(*scenes[0], H, W, 0.5)
    side.synchronize()
    assert all(torch.equal(_bits(there[k]), _bits(eager[0][k])) for k in there)
    # capture on one stream (a single chain, as graph.py captures), replay on fresh inputs
    static = [t.clone() for t in scenes[0]]
    out = {k: torch.empty_like(v) for k, v in eager[0].items()}
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        gbuffer_ops.gbuffer_into(out, *static, H, W, 0.5)
    for i in (1, 0):
        for dst, src in zip(static, scenes[i]):
            dst.copy_(src)
        for v in out.values():
            v.fill_(0x77 if v.dtype == torch.uint8 else -3.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(out[k]), _bits(eager[i][k])) for k in out)


def test_routing_and_refusals(monkeypatch):
    B, H, W = 1, 5, 7
    rays, depth, acc = _dev(gu.scene("holes", B, H, W, 11))
    calls, real = [], gbuffer_ops.gbuffer
    monkeypatch.setattr(gbuffer_ops, "gbuffer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    want = geometry.gbuffer(rays, depth, acc, H, W)
    assert len(calls) == 1 and want.z.is_cuda
    # float64, views and CPU tensors take the statement
    g64 = geometry.gbuffer(rays.double(), depth.double(), acc.double(), H, W)
    assert g64.z.dtype == torch.float64 and g64.z.is_cuda and torch.equal(g64.mask, want.mask)
    view = rays[..., :8]
    assert not view.is_contiguous()
    gv = geometry.gbuffer(view, depth, acc, H, W)
    assert torch.equal(gv.mask, want.mask) and torch.equal(gv.depth16, want.depth16) and torch.equal(_bits(gv.z), _bits(want.z))
    dview = torch.zeros(B, H * W, 2, device=DEV)[..., 0]
    dview.copy_(depth)
    assert torch.equal(geometry.gbuffer(rays, dview, acc, H, W).depth16, want.depth16)
    gc = geometry.gbuffer(rays.cpu(), depth.cpu(), acc.cpu(), H, W)
    assert not gc.z.is_cuda and torch.equal(gc.depth16, want.depth16.cpu())
    assert len(calls) == 1
    monkeypatch.setattr(gbuffer_ops, "gbuffer", real)
    # the binding refuses what the kernel does not take
    for bad in (lambda: gbuffer_ops.gbuffer(view, depth, acc, H, W), lambda: gbuffer_ops.gbuffer(rays.double(), depth.double(), acc.double(), H, W),
                lambda: gbuffer_ops.gbuffer(rays.cpu(), depth.cpu(), acc.cpu(), H, W), lambda: gbuffer_ops.gbuffer(rays, dview, acc, H, W),
                lambda: gbuffer_ops.gbuffer(rays, depth, acc, H, W + 1), lambda: gbuffer_ops.gbuffer(rays, depth[:, :-1].contiguous(), acc, H, W),
                lambda: gbuffer_ops.gbuffer(rays[..., :7].contiguous(), depth, acc, H, W), lambda: gbuffer_ops.gbuffer(rays, depth, acc, H, W, float("nan")),
                lambda: gbuffer_ops.gbuffer(rays, depth, acc, H, W, float("inf")), lambda: gbuffer_ops.gbuffer(rays, depth, acc, 0, 0),
                lambda: gbuffer_ops.gbuffer_into({}, rays, depth, acc, H, W), lambda: gbuffer_ops.gbuffer_into({"z": None}, rays, depth, acc, H, W),
                lambda: gbuffer_ops.gbuffer_into({"depth": torch.empty(B, H, W, device=DEV)}, rays, depth, acc, H, W),
                lambda: gbuffer_ops.gbuffer_into({"z": torch.empty(B, H, W + 1, device=DEV)}, rays, depth, acc, H, W),
                lambda: gbuffer_ops.gbuffer_into({"mask": torch.empty(B, H, W, device=DEV)}, rays, depth, acc, H, W),
                lambda: gbuffer_ops.gbuffer_into({"z": torch.empty(B, H, W)}, rays, depth, acc, H, W)):
        with pytest.raises(RuntimeError):
            bad()
    for bad in (lambda: geometry.gbuffer(rays, depth, acc, H, W + 1), lambda: geometry.gbuffer(rays, depth.double(), acc, H, W),
                lambda: geometry.gbuffer(rays, depth.cpu(), acc, H, W), lambda: geometry.gbuffer(rays, depth, acc, H, W, float("nan"))):
        with pytest.raises(ValueError):
            bad()


def test_forward_returns_the_marchs_depth_on_the_device():
    trainer = iu.make_trainer(DEV)
    S = trainer.render_size
    inp = dict(iu.frame(DEV, (S, S)), render_full_img=True)
    with torch.no_grad():
        plain = trainer(**inp)
        with_depth = trainer(**dict(inp, return_depth=True))
        maps = trainer.nerf_forward(ray_batch=inp["ray_batch"], background_prior=inp["background_prior"], latent_code=trainer.latent_codes[0:1],
                                    inv_head_T=inp["inv_head_T"], front_render_cond=inp["front_render_cond"],
                                    left_render_cond=inp["left_render_cond"], right_render_cond=inp["right_render_cond"], mode="validation")
    assert len(plain) == 3 and len(with_depth) == 4 and with_depth[3].shape == (1, 1, S, S)
    for a, b in zip(plain, with_depth):
        assert torch.equal(a, b)
    assert torch.equal(with_depth[3].reshape(-1), maps[5].reshape(-1)) and torch.equal(with_depth[1].reshape(-1), maps[6].reshape(-1))
    g = geometry.gbuffer(inp["ray_batch"], with_depth[3].reshape(1, -1), with_depth[1].reshape(1, -1), S, S, SYNTH_ACC_MIN)
    c = geometry.gbuffer_statement(inp["ray_batch"].cpu(), with_depth[3].reshape(1, -1).cpu(), with_depth[1].reshape(1, -1).cpu(), S, S, SYNTH_ACC_MIN)
    assert 0 < int((g.mask & 1).sum()) < S * S
    assert torch.equal(g.mask.cpu(), c.mask) and torch.equal(g.depth16.cpu(), c.depth16) and torch.equal(_bits(g.z.cpu()), _bits(c.z))


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graphed", "eager"])
def test_cli_gbuffer_on_the_device(tmp_path, monkeypatch, graph):
    """The files equal geometry.gbuffer of the frame's maps (which the kernel computed), their depth codes the CPU statement's, and the rgb PNGs
    are byte-identical to a run of the same process without --gbuffer.  Both runs restrict MIOpen to its deterministic solvers, as
    tests/test_metrics_gpu.py does and for its reason."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setenv("HAVATAR_GRAPH", graph)
    kernel_calls, real = [], gbuffer_ops.gbuffer
    monkeypatch.setattr(gbuffer_ops, "gbuffer", lambda *a, **k: (kernel_calls.append(1), real(*a, **k))[1])
    out, calls = check_cli(tmp_path, monkeypatch, "cuda", _cli_runner(tmp_path, monkeypatch, "cuda"))
    assert len(kernel_calls) >= 2          # both frames went through the kernel (and check_cli's own evaluations)
    for f, (rays, depth, acc, H, W, acc_min) in enumerate(calls):
        assert rays.is_contiguous() and rays.dtype == torch.float32
        c = geometry.gbuffer_statement(rays.cpu(), depth.cpu(), acc.cpu(), H, W, acc_min)
        d16, n8, s8 = _read_maps(out, "%d_00" % f)
        assert np.array_equal(d16, c.depth16[0].numpy())
        assert int(np.abs(n8.astype(np.int64) - c.normal8[0].numpy()).max()) <= 1 and int(np.abs(s8.astype(np.int64) - c.shade8[0].numpy()).max()) <= 1

"""Device: csrc/hav_metrics.hip through havatar_amd.metrics against the float64 restatement of tests/metrics_util.py, with the ATen float32
statement on the CPU as the yardstick of every accuracy bound; the exact behaviours (identical pairs, squared-error coverage, bit
reproducibility, streams, capture), the routing, and `avatarHD_reenactment.py --metrics` on the device.

Measured on an MI355X (worst over the shapes below; e = |value - float64 truth|):
    kind      native mean   native map   ATen float32 (CPU) mean   ATen float32 (CPU) map
    texture   2.9e-8        3.0e-8       2.0e-6                    2.4e-5
    quant8    2.2e-8        3.0e-8       9.1e-7                    2.0e-5
    flat      2.5e-8        2.8e-8       1.3e-4                    2.1e-4
    mixed     2.5e-8        3.0e-8       1.3e-6                    3.5e-4
    uint8     2.6e-8 (all kinds)         1.6e-4 (flat), <= 1.5e-6 (others)
The smallest ATen map error of a texture pair over the shapes is 2.0e-6, so the flat / mixed clause asks for 4.0e-6 at the least; the bars of
1e-6 (mean) hold with a factor of 35.  The moments are accumulated in float64, so what is left of the native error is the float32 rounding of
the stored result (3e-8 for values in [0.5, 1))."""
import json
import os

import numpy as np
import pytest
import torch

import metrics_util as mu
from havatar_amd import metrics, synth
from havatar_amd.native import metrics_ops as ops

pytestmark = pytest.mark.gpu

T_H, T_W = ops.TILE_H, ops.TILE_W
SHAPES = ([(1, 1, 11, 11), (2, 3, 12, 13)]
          + [(1, 3, T_H + d + 10, 26) for d in (-1, 0, 1)] + [(1, 3, 26, T_W + d + 10) for d in (-1, 0, 1)]
          + [(1, 3, 2 * T_H + 10 + 5, 3 * T_W + 10 + 3), (2, 3, 64, 64)])
SHAPES_U8 = list(dict.fromkeys((s[0], 3, s[2], s[3]) for s in SHAPES))          # the uint8 twins: every shape with C = 3


def _dev(t):
    return t.to("cuda")


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", mu.KINDS)
def test_float_accuracy(kind, shape):
    """mean: e_native <= max(2 e_aten, 1e-6); map: e_native <= max(2 e_aten_map, 2e-6), e_aten measured here for this very case.  On the flat and
    mixed kinds additionally e_native(mean) <= 1e-6 and e_native(map) <= 2 x the ATen map error of the texture pair at the same shape: the
    clause that shows the cancellation is gone.  mse against float64 to float32 rounding."""
    a, b = mu.pair(kind, shape)
    ref, ref_map = mu.truth(kind, shape)
    e_aten, e_aten_map = mu.aten32_errors(kind, shape)
    s, m = metrics.ssim(_dev(a), _dev(b), return_map=True)
    assert s.dtype == torch.float32 and tuple(m.shape) == tuple(ref_map.shape)
    e, e_map = float(np.abs(s.double().cpu().numpy() - ref).max()), float(np.abs(m.double().cpu().numpy() - ref_map).max())
    print("%s %s native mean %.3g map %.3g | aten32 mean %.3g map %.3g" % (kind, shape, e, e_map, e_aten, e_aten_map))
    assert e <= max(2 * e_aten, 1e-6) and e_map <= max(2 * e_aten_map, 2e-6)
    if kind in ("flat", "mixed"):
        tex_map = mu.aten32_errors("texture", shape)[1]
        print("    texture aten32 map error at this shape %.3g" % tex_map)
        assert e <= 1e-6 and e_map <= 2 * tex_map
    d = metrics.image_metrics(_dev(a), _dev(b))
    mse = mu.mse64(a.numpy(), b.numpy())
    assert np.abs(d["mse"].double().cpu().numpy() - mse).max() <= 2e-7 * mse.max() + 1e-12
    assert torch.equal(d["ssim"], s)


@pytest.mark.parametrize("shape", SHAPES_U8, ids=_ids)
@pytest.mark.parametrize("kind", mu.KINDS)
def test_uint8_accuracy(kind, shape):
    """SSIM mean to max(2 e_aten, 1e-6) with the float64 restatement on u8 / 255 as truth (e_aten: the ATen float32 statement on u8 / 255 on the
    CPU); mse equal to the exact integer sum / (255^2 N) to 1 ulp of float32; the map against the restatement's as well"""
    a, b = mu.pair_u8(kind, shape)
    ref, mse = mu.u8_truth(a.numpy(), b.numpy())
    x, y = (t.permute(0, 3, 1, 2).float() / 255 for t in (a, b))
    e_aten = float(np.abs(metrics.aten_statement(x, y)[0].double().numpy() - ref).max())
    d = metrics.image_metrics(_dev(a), _dev(b))
    e = float(np.abs(d["ssim"].double().cpu().numpy() - ref).max())
    print("%s %s u8 native mean %.3g | aten32 mean %.3g" % (kind, shape, e, e_aten))
    assert e <= max(2 * e_aten, 1e-6)
    got = d["mse"].cpu().numpy()
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - mse) <= np.spacing(mse.astype(np.float32))).all(), (got, mse)
    m = metrics.ssim(_dev(a), _dev(b), return_map=True)[1]
    ref_map = mu.ssim64(a.numpy().transpose(0, 3, 1, 2) / 255.0, b.numpy().transpose(0, 3, 1, 2) / 255.0)[1]
    assert float(np.abs(m.double().cpu().numpy() - ref_map).max()) <= 2e-6


def test_identical_pairs_give_exactly_one_and_zero():
    for shape in ((1, 3, 11, 11), (2, 3, 12, 13), (1, 3, 2 * T_H + 15, 3 * T_W + 13), (2, 3, 64, 64)):
        a = _dev(mu.pair("texture", shape)[0])
        u = _dev(mu.pair_u8("mixed", shape)[0])
        for x in (a, u):
            d = metrics.image_metrics(x, x.clone())
            s, m = metrics.ssim(x, x.clone(), return_map=True)
            assert torch.equal(d["ssim"], torch.ones_like(d["ssim"])) and torch.equal(d["mse"], torch.zeros_like(d["mse"]))
            assert torch.equal(m, torch.ones_like(m)) and torch.isinf(d["psnr"]).all()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_squared_error_counts_every_pixel_once(u8):
    """a pair that differs in one pixel -- at the corners, on the tile seams, in the rim only the last tiles own, in the last row / column --
    gives mse = d^2 / N every time, in every channel"""
    H, W = 2 * T_H + 15, 3 * T_W + 13          # 2 x 3 tiles, partial edges
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (T_H - 1, T_W - 1), (T_H, T_W), (T_H - 1, T_W), (2 * T_H - 1, 2 * T_W),
             (2 * T_H, 5), (5, 3 * T_W), (H - 11, W - 11), (H - 10, W - 10), (H - 1, T_W + 3), (T_H + 3, W - 1), (2 * T_H + 4, 3 * T_W + 2)]
    N = 3 * H * W
    for k, (y, x) in enumerate(spots):
        c = k % 3
        if u8:
            a = torch.full((1, H, W, 3), 100, dtype=torch.uint8)
            b = a.clone()
            b[0, y, x, c] = 108
            want = np.float32(64.0 / (255.0 ** 2 * N))
        else:
            a = torch.full((1, 3, H, W), 0.25)
            b = a.clone()
            b[0, c, y, x] = 0.75
            want = np.float32(0.25 / N)
        got = metrics.image_metrics(_dev(a), _dev(b))["mse"].cpu().numpy()[0]
        assert abs(float(got) - float(want)) <= float(np.spacing(want)), ((y, x, c), got, want)


def test_bit_reproducible_and_map_does_not_change_the_value():
    for a, b in (mu.pair("texture", (2, 3, 79, 109)), mu.pair_u8("quant8", (2, 3, 79, 109))):
        a, b = _dev(a), _dev(b)
        fn = ops.image_metrics_u8 if a.dtype == torch.uint8 else ops.image_metrics_f32
        o1, m1 = fn(a, b, want_map=True)
        o2, m2 = fn(a, b, want_map=True)
        o3, m3 = fn(a, b, want_map=False)
        assert m3 is None and torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(o1.view(torch.int32), o3.view(torch.int32))
        assert torch.equal(m1.view(torch.int32), m2.view(torch.int32))


def test_side_stream_and_graph_replays_return_the_eager_bits():
    pairs = [tuple(_dev(t) for t in mu.pair(k, (2, 3, 64, 64))) for k in ("texture", "mixed")]
    eager = [ops.image_metrics_f32(a, b, want_map=True) for a, b in pairs]
    pairs8 = [tuple(_dev(t) for t in mu.pair_u8(k, (2, 3, 64, 64))) for k in ("texture", "mixed")]
    eager8 = [ops.image_metrics_u8(a, b)[0] for a, b in pairs8]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o, m = ops.image_metrics_f32(*pairs[0], want_map=True)
        o8 = ops.image_metrics_u8(*pairs8[0])[0]
    side.synchronize()
    assert torch.equal(o, eager[0][0]) and torch.equal(m, eager[0][1]) and torch.equal(o8, eager8[0])
    # capture on one stream (a single chain, as graph.py captures), replay on two different inputs
    sa, sb = pairs[0][0].clone(), pairs[0][1].clone()
    ua, ub = pairs8[0][0].clone(), pairs8[0][1].clone()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        go, gm = ops.image_metrics_f32(sa, sb, want_map=True)
        go8 = ops.image_metrics_u8(ua, ub)[0]
    for k in (1, 0):
        sa.copy_(pairs[k][0]); sb.copy_(pairs[k][1]); ua.copy_(pairs8[k][0]); ub.copy_(pairs8[k][1])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(go, eager[k][0]) and torch.equal(gm, eager[k][1]) and torch.equal(go8, eager8[k])


def test_routing(monkeypatch):
    calls = []
    real_f, real_u = ops.image_metrics_f32, ops.image_metrics_u8
    monkeypatch.setattr(ops, "image_metrics_f32", lambda *a, **k: (calls.append("f32"), real_f(*a, **k))[1])
    monkeypatch.setattr(ops, "image_metrics_u8", lambda *a, **k: (calls.append("u8"), real_u(*a, **k))[1])
    a, b = (_dev(t) for t in mu.pair("texture", (1, 3, 24, 28)))
    ua, ub = (_dev(t) for t in mu.pair_u8("texture", (1, 3, 24, 28)))
    monkeypatch.delenv("HAVATAR_METRICS", raising=False)
    s = metrics.ssim(a, b)
    metrics.image_metrics(ua, ub)
    assert calls == ["f32", "u8"]
    # the switch: the ATen statement, in the input dtype on the device (float64 for uint8)
    monkeypatch.setenv("HAVATAR_METRICS", "0")
    s0 = metrics.ssim(a, b)
    d0 = metrics.image_metrics(ua, ub)
    assert calls == ["f32", "u8"] and s0.dtype == torch.float32 and s0.is_cuda and d0["ssim"].dtype == torch.float64
    assert abs(float(s0) - float(s)) <= 1e-5
    monkeypatch.delenv("HAVATAR_METRICS")
    # tensors that need a gradient take the statement, and the gradient arrives
    ag = a.clone().requires_grad_(True)
    sg = metrics.ssim(ag, b)
    assert calls == ["f32", "u8"] and sg.requires_grad
    assert torch.isfinite(torch.autograd.grad(sg.sum(), ag)[0]).all()
    with torch.no_grad():
        metrics.ssim(ag, b)
    assert calls == ["f32", "u8", "f32"]
    # other dtypes take the statement in their own dtype
    for dt in (torch.float16, torch.float64):
        sh = metrics.ssim(a.to(dt), b.to(dt))
        assert calls == ["f32", "u8", "f32"] and sh.dtype == dt and sh.is_cuda and bool(torch.isfinite(sh).all())
        if dt == torch.float64:
            assert abs(float(sh) - float(s)) <= 1e-5
    # ten rows: refused on both routes, by shape
    for env in ("1", "0"):
        monkeypatch.setenv("HAVATAR_METRICS", env)
        with pytest.raises(ValueError, match=r"H, W >= 11.*\(1, 3, 10, 64\)"):
            metrics.ssim(torch.zeros(1, 3, 10, 64, device="cuda"), torch.zeros(1, 3, 10, 64, device="cuda"))
        with pytest.raises(ValueError, match=r"H, W >= 11.*\(1, 10, 64, 3\)"):
            metrics.ssim(torch.zeros(1, 10, 64, 3, device="cuda", dtype=torch.uint8), torch.zeros(1, 10, 64, 3, device="cuda", dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="not covered"):
        ops.image_metrics_f32(torch.zeros(1, 3, 10, 64, device="cuda"), torch.zeros(1, 3, 10, 64, device="cuda"))


def test_unaligned_views_take_the_scalar_loads_and_agree():
    """a pair whose storage starts 4 bytes off a 16-byte boundary (W % 4 == 0): the 4-byte template, the same value"""
    a, b = mu.pair("texture", (1, 3, 64, 64))
    buf_a, buf_b = torch.empty(a.numel() + 1, device="cuda"), torch.empty(b.numel() + 1, device="cuda")
    va, vb = buf_a[1:].view(a.shape), buf_b[1:].view(b.shape)
    va.copy_(a); vb.copy_(b)
    assert va.data_ptr() % 16 == 4 and va.is_contiguous()
    o1, m1 = ops.image_metrics_f32(va, vb, want_map=True)
    o2, m2 = ops.image_metrics_f32(_dev(a), _dev(b), want_map=True)
    assert torch.equal(o1, o2) and torch.equal(m1, m2)


def test_cli_on_the_device(tmp_path, monkeypatch):
    """graph mode (the default): metrics.json equals the restatement computed from the PNGs of that run (SSIM to 1e-6, mse to 1 ulp of
    float32), and the PNGs are byte-identical to a run of the same process without --metrics.  Both runs restrict MIOpen to its deterministic
    solvers: with the default ones two runs of the command line differ in a pixel or two by 1 LSB whatever the flag -- the last section of
    profiles/metrics_ab.txt (`tools/bench_metrics.py --reenact`) has the run-by-run table: runs 0 and 1, both without the flag, already differ
    (DESIGN.md 7.9)."""
    import yaml
    from havatar_amd.harness import reenact
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    root = str(tmp_path / "data")
    os.makedirs(root)
    split = synth.write_dataset(root, n_frames=2, img_res=128)
    cfg_path, ckpt = str(tmp_path / "cfg.yml"), mu.checkpoint(tmp_path / "avatar.pth")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(synth.harness_config(), f)
    calls, real = [], ops.image_metrics_u8
    monkeypatch.setattr(ops, "image_metrics_u8", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = []
    for extra in (["--metrics"], []):
        out = str(tmp_path / ("with" if extra else "without"))
        written = reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", out, "--split", split] + extra, device="cuda")
        assert [os.path.basename(p) for p in written] == ["0_00.png", "1_00.png"]
        outs.append((out, written))
    assert len(calls) == 2          # the native entry scored both frames
    assert not os.path.exists(os.path.join(outs[1][0], "metrics.json"))
    for p, q in zip(outs[0][1], outs[1][1]):
        assert open(p, "rb").read() == open(q, "rb").read()
    with open(os.path.join(outs[0][0], "metrics.json")) as f:
        table = json.load(f)
    assert table["n"] == 2 and [f["fidx"] for f in table["frames"]] == [0, 1]
    mu.check_table(table, outs[0][0], mu.split_ground_truth(split), ssim_tol=1e-6, mse_tol_ulp32=1)

"""The G-buffer on CPU tensors (havatar_amd/geometry.py: gbuffer, gbuffer_statement): the ATen statement against a plain-loop float64 restatement
of the definition, the analytic sphere and depth step, the codes, the 16-bit PNG, Trainer.forward(return_depth=True), the binding, refusals and
code generation of csrc/hav_gbuffer.hip, and avatarHD_reenactment.py --gbuffer end to end."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import gbuffer_util as gu
import iso_util as iu
import metrics_util as mu
from havatar_amd import geometry, synth
from havatar_amd.dataloader import imgio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYNTH_ACC_MIN = 0.52          # inside the synthetic checkpoint's accumulations (0.45 .. 0.6): valid and invalid pixels both occur


# ------------------------------------------------------------------------------------------------------------------------------------
# the statement against the plain loops
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gu.KINDS)
@pytest.mark.parametrize("B,H,W,stride", [(1, 1, 1, 8), (1, 1, 5, 8), (1, 5, 1, 11), (1, 2, 2, 8), (2, 9, 11, 11)],
                         ids=lambda v: str(v))
def test_statement_equals_the_plain_loops(kind, B, H, W, stride):
    rays, depth, acc = (t.double() for t in gu.scene(kind, B, H, W, stride))
    aux = {}
    got = geometry.gbuffer_statement(rays, depth, acc, H, W, 0.5, aux=aux)
    want = gu.restate(rays, depth, acc, H, W, 0.5)
    assert got.z.dtype == torch.float64 and got.normal.shape == (B, H, W, 3) and got.depth16.shape == (B, H, W, 2)
    assert np.array_equal(aux["choice"].numpy(), want["choice"]) and np.array_equal(got.mask.numpy(), want["mask"])
    assert float(np.abs(got.z.numpy() - want["z"]).max()) <= 1e-12
    assert float(np.abs(got.normal.numpy() - want["normal"]).max()) <= 1e-12
    assert np.array_equal(got.depth16.numpy(), want["depth16"])
    for k in ("normal8", "shade8"):
        assert int(np.abs(getattr(got, k).numpy().astype(np.int64) - want[k].astype(np.int64)).max()) <= 1, k
    # float32 makes decisions of its own; given to the float64 evaluation they are the ones it reports, and the gbuffer() of CPU tensors is
    # the statement
    rays32, depth32, acc32 = gu.scene(kind, B, H, W, stride)
    aux32, aux64 = {}, {}
    s32 = geometry.gbuffer_statement(rays32, depth32, acc32, H, W, 0.5, aux=aux32)
    geometry.gbuffer_statement(rays, depth, acc, H, W, 0.5, choice=aux32["choice"], aux=aux64)
    assert torch.equal(aux64["choice"], aux32["choice"]) and s32.z.dtype == torch.float32
    via = geometry.gbuffer(rays32, depth32, acc32, H, W, 0.5)
    assert all(torch.equal(a, b) for a, b in zip((via.mask, via.depth16, via.normal8, via.shade8), (s32.mask, s32.depth16, s32.normal8, s32.shade8)))
    if kind == "degenerate":
        assert not bool((got.mask & 2).any()) and bool((got.mask & 1).all()) and bool((got.shade8 == 255).all()) and not bool(got.normal8.any())
    if kind == "flat" and H > 2 and W > 2:
        assert bool((aux["choice"][:, 1:-1, 1:-1] & 15 == 15).all())          # a tie on both axes: central
    if kind == "noise" and H * W >= 50:          # both clamps are reached
        assert float(got.z[(got.mask & 1) != 0].min()) == float(rays[0, 0, 6]) and float(got.z.max()) == float(rays[0, 0, 7])


def test_sphere_normals_are_the_analytic_ones():
    """128^2, float32 statement, over the pixels whose 3x3 neighbourhood all hits: mean angle to (p - c) / r at most 0.005 rad, worst at most
    0.05 rad.  Measured: 0.0017 and 0.029."""
    H = W = 128
    rays, depth, acc = gu.scene("sphere", 1, H, W)
    g = geometry.gbuffer(rays, depth, acc, H, W)
    o, d = gu.camera(H, W)
    hit, t = gu.sphere_hit(o, d)
    inner = hit.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = np.zeros_like(hit)
            sh[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = hit[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
            inner &= sh
    assert inner.sum() > 5000 and bool(((g.mask[0].numpy() & 3) == 3)[inner].all())
    ang = gu.angle(g.normal[0], torch.from_numpy((o + d * t[..., None]) / gu.RADIUS)).numpy()[inner]
    print("sphere 128^2: mean %.4f rad, worst %.4f rad over %d pixels" % (ang.mean(), ang.max(), inner.sum()))
    assert ang.mean() <= 0.005 and ang.max() <= 0.05
    assert float((g.z[0].numpy() - t)[inner].__abs__().max()) <= 4 * 2.0 ** -24 * gu.FAR          # depth / acc gives the hit's distance back


@pytest.mark.parametrize("S", [32, 128])
def test_no_normal_on_a_depth_step_turns_more_than_the_flat_parts(S):
    """Two levels of constant z split at W/2: the analytic normal of either level is -d(q).  A normal's turn is its angle to -d(q), counted in
    the pixel's own angular pitch (the largest angle between its ray and a 4-neighbour's): a difference quotient over a pitch resolves the
    normal to a fraction of that pitch -- half of it one-sided, none of it central -- and the pitch of a pinhole image shrinks from the centre
    (where the step is) to the corners by cos^2.  No pixel next to the step turns by more than the worst pixel of the flat part (an image
    corner, one-sided on both axes).  A tangent taken across the step would turn by ~1.5 rad = hundreds of pitches.
    Measured at 128^2: 0.695 pitches on the step, 0.743 on the flat part."""
    rays, depth, acc = gu.scene("step", 1, S, S)
    aux = {}
    g = geometry.gbuffer_statement(rays, depth, acc, S, S, aux=aux)
    assert bool((g.mask == 3).all())
    _, d = gu.camera(S, S)
    dt = torch.from_numpy(d)
    pitch = torch.zeros(S, S, dtype=torch.float64)
    ax = gu.angle(dt[:, 1:], dt[:, :-1])
    ay = gu.angle(dt[1:], dt[:-1])
    pitch[:, 1:], pitch[:, :-1] = torch.maximum(pitch[:, 1:], ax), torch.maximum(pitch[:, :-1], ax)
    pitch[1:], pitch[:-1] = torch.maximum(pitch[1:], ay), torch.maximum(pitch[:-1], ay)
    turn = gu.angle(g.normal[0], -dt) / pitch
    on_step = torch.zeros(S, S, dtype=torch.bool)
    on_step[:, S // 2 - 1:S // 2 + 1] = True
    print("step %d^2: %.3f pitches on the step, %.3f on the flat part" % (S, float(turn[on_step].max()), float(turn[~on_step].max())))
    assert float(turn[on_step].max()) <= float(turn[~on_step].max())
    # the decisions there: the side away from the step, never central
    sx = aux["choice"][0] & 3
    assert bool((sx[:, S // 2 - 1] == 2).all()) and bool((sx[:, S // 2] == 1).all()) and bool((sx[:, 1:S // 2 - 1] == 3).all())


@pytest.mark.parametrize("kind", gu.KINDS)
def test_codes(kind):
    """code 0 exactly where the pixel is invalid; the decoded depth within (far - near) / 65534 of z"""
    B, H, W = 2, 33, 31
    rays, depth, acc = gu.scene(kind, B, H, W)
    g = geometry.gbuffer(rays, depth, acc, H, W)
    code = g.depth16[..., 0].to(torch.int32) * 256 + g.depth16[..., 1].to(torch.int32)
    valid = (g.mask & 1) != 0
    want_valid = (acc > 0.5) & torch.isfinite(depth)
    assert torch.equal(valid.reshape(B, -1), want_valid) and torch.equal(code == 0, ~valid)
    if kind not in ("step", "flat", "degenerate"):
        assert bool(valid.any()) and bool((~valid).any())
    dec = geometry.decode_depth16(g.depth16, gu.NEAR, gu.FAR)
    assert bool(torch.isnan(dec[~valid]).all())
    err = float((dec[valid] - g.z[valid].double()).abs().max())
    assert err <= (gu.FAR - gu.NEAR) / 65534
    assert bool((g.z[~valid] == 0).all()) and bool((g.z[valid] >= np.float32(gu.NEAR)).all()) and bool((g.z[valid] <= np.float32(gu.FAR)).all())
    # a pixel without a normal is white in the shade and (0,0,0) in the normal map; with one, the normal faces the camera
    has = (g.mask & 2) != 0
    assert bool((g.shade8[~has] == 255).all()) and not bool(g.normal8[~has].any()) and not bool(g.normal[~has].any())
    assert bool((has <= valid).all())
    if bool(has.any()):
        d = rays.reshape(B, H, W, -1)[..., 3:6]
        assert float((g.normal * d).sum(-1)[has].max()) <= 1e-6
        assert float((g.normal[has].double().norm(dim=-1) - 1).abs().max()) <= 1e-6


def test_png_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.integers(0, 65536, (7, 5)).astype(np.uint16)
    v[0, :4] = (0, 1, 255, 65535)
    hi_lo = np.stack([(v >> 8).astype(np.uint8), (v & 255).astype(np.uint8)], -1)
    path = str(tmp_path / "d.png")
    imgio.imwrite_gray16(path, hi_lo)
    back = imgio.imread_gray16(path)
    assert back.dtype == np.uint8 and back.shape == (7, 5, 2) and np.array_equal(back, hi_lo)
    from PIL import Image
    with Image.open(path) as im:
        assert im.size == (5, 7) and im.mode.startswith("I;16") and np.array_equal(np.asarray(im).astype(np.uint16), v)
    g = rng.integers(0, 256, (7, 5)).astype(np.uint8)
    imgio.imwrite_gray8(str(tmp_path / "g.png"), g)
    with Image.open(str(tmp_path / "g.png")) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), g)
    with pytest.raises(ValueError):
        imgio.imwrite_gray16(path, v)
    with pytest.raises(ValueError):
        imgio.imwrite_gray8(path, hi_lo)
    with pytest.raises(ValueError):
        imgio.imread_gray16(str(tmp_path / "g.png"))


def test_refusals():
    rays, depth, acc = gu.scene("sphere", 1, 5, 7)
    for bad in (lambda: geometry.gbuffer(rays, depth, acc, 7, 7), lambda: geometry.gbuffer(rays[..., :7], depth, acc, 5, 7),
                lambda: geometry.gbuffer(rays, depth[:, :-1], acc, 5, 7), lambda: geometry.gbuffer(rays, depth.double(), acc, 5, 7),
                lambda: geometry.gbuffer(rays, depth, acc, 5, 7, float("nan")), lambda: geometry.gbuffer(rays, depth, acc, 5, 7, float("inf")),
                lambda: geometry.gbuffer(rays, depth, acc, 0, 35), lambda: geometry.gbuffer(rays[0], depth, acc, 5, 7),
                lambda: geometry.gbuffer(rays.numpy(), depth, acc, 5, 7), lambda: geometry.gbuffer(rays.int(), depth, acc, 5, 7)):
        with pytest.raises(ValueError):
            bad()


def test_cpu_maps_never_reach_the_kernel(monkeypatch):
    from havatar_amd.native import gbuffer_ops
    rays, depth, acc = gu.scene("holes", 1, 5, 7)
    with pytest.raises(RuntimeError, match="contiguous float32 HIP"):          # the binding refuses; it has no other path
        gbuffer_ops.gbuffer(rays, depth, acc, 5, 7)
    monkeypatch.setattr(gbuffer_ops, "gbuffer", lambda *a, **k: pytest.fail("a CPU tensor reached the kernel's binding"))
    assert geometry.gbuffer(rays, depth, acc, 5, 7).z.shape == (1, 5, 7)


# ------------------------------------------------------------------------------------------------------------------------------------
# Trainer.forward(return_depth=True)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_forward_returns_the_marchs_depth():
    trainer = iu.make_trainer("cpu")
    S = trainer.render_size
    inp = dict(iu.frame("cpu", (S, S)), render_full_img=True)
    with torch.no_grad():
        plain = trainer(**inp)
        with_depth = trainer(**dict(inp, return_depth=True))
        off = trainer(**dict(inp, return_depth=False))
        maps = trainer.nerf_forward(ray_batch=inp["ray_batch"], background_prior=inp["background_prior"], latent_code=trainer.latent_codes[0:1],
                                    inv_head_T=inp["inv_head_T"], front_render_cond=inp["front_render_cond"],
                                    left_render_cond=inp["left_render_cond"], right_render_cond=inp["right_render_cond"], mode="validation")
    assert len(plain) == 3 and len(off) == 3 and len(with_depth) == 4
    # without the key: what forward returned before, which is nerf_forward's fine maps reshaped
    assert torch.equal(plain[0], maps[4].reshape(1, S, S, -1).permute(0, 3, 1, 2)) and torch.equal(plain[1], maps[6].reshape(1, 1, S, S))
    for a, b, c in zip(plain, with_depth, off):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert with_depth[3].shape == (1, 1, S, S) and torch.equal(with_depth[3].reshape(-1), maps[5].reshape(-1))
    assert float(with_depth[3].min()) > 0
    # the statement of this module takes them as they come
    g = geometry.gbuffer(inp["ray_batch"], with_depth[3].reshape(1, -1), with_depth[1].reshape(1, -1), S, S, SYNTH_ACC_MIN)
    assert 0 < int((g.mask & 1).sum()) < S * S


# ------------------------------------------------------------------------------------------------------------------------------------
# the library
# ------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib, build
    from havatar_amd.native import gbuffer_ops
    L = _lib.lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    assert L.hav_gbuffer_tile.restype is i32 and L.hav_gbuffer_tile.argtypes == [i32]
    assert L.hav_gbuffer_f32.restype is i32 and L.hav_gbuffer_f32.argtypes == [vp] * 10 + [i32] * 4 + [f32, vp]
    assert _lib.ABI_VERSION == L.hav_abi_version() == 8          # additions within the version: nothing existing changed
    assert "hav_gbuffer.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    for name in ("hav_gbuffer_tile", "hav_gbuffer_f32"):
        assert re.search(r"\b%s\(" % name, hdr), name
    assert (gbuffer_ops.TILE_H, gbuffer_ops.TILE_W) == (L.hav_gbuffer_tile(0), L.hav_gbuffer_tile(1)) == gbuffer_ops.tile()
    assert gbuffer_ops.TILE_W % 64 == 0 and gbuffer_ops.TILE_H * gbuffer_ops.TILE_W == 256 and L.hav_gbuffer_tile(2) == 0
    # refusals that need no device: the checks come before the launch, the pointers are never dereferenced
    one = C.c_void_p(16)
    ok = dict(B=1, H=4, W=4, stride=8, acc_min=0.5)
    call = lambda outs, ins, **kw: L.hav_gbuffer_f32(*outs, *ins, *[dict(ok, **kw)[k] for k in ("B", "H", "W", "stride", "acc_min")], None)
    for miss in range(3):
        assert call([one] * 7, [None if k == miss else one for k in range(3)]) == -1
    assert call([None] * 7, [one] * 3) == -1          # no output at all
    for kw in (dict(H=0), dict(W=0), dict(B=0), dict(H=-1), dict(stride=7), dict(acc_min=float("nan")), dict(acc_min=float("inf")),
               dict(acc_min=float("-inf")), dict(B=4, H=8192, W=8192), dict(H=16384, W=16384), dict(H=4096, W=4096, stride=128)):
        assert call([one] * 7, [one] * 3, **kw) == -1, kw
    src = open(os.path.join(ROOT, "havatar_amd", "csrc", "hav_gbuffer.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "getenv" not in code and not re.search(r"atomic", code, re.I) and not re.search(r"hipMalloc|Synchronize", code)
    assert "fp contract(off)" in code          # the statement rounds after every operation; so does the kernel
    text = open(os.path.join(ROOT, "havatar_amd", "native", "gbuffer_ops.py")).read()
    assert "environ" not in text and "getenv" not in text and "gbuffer_statement" not in text          # no switch and no fallback in the binding


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_private_segment_no_spill(tmp_path):
    dst = str(tmp_path / "hav_gbuffer.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_gbuffer.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    kernels = re.findall(r"\.name:\s+(\S*_kernel\S*)", text)
    assert len(set(kernels)) == 1 and "gbuffer_kernel" in kernels[0], kernels
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert scratch == [0], scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert spills == [0, 0], spills
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert lds == [4 * 396 * 4 + 396]          # p and z of the 6 x 66 staged pixels, and a byte of validity each
    # every fused multiply-add belongs to a division's or a square root's refinement: the definition's own sums and products are not fused
    body = text[text.index("gbuffer_kernel"):]
    assert len(re.findall(r"\bv_div_fixup_f32\b", body)) >= 1 and not re.search(r"\bv_pk_fma_f32\b|\bv_mad_f32\b", body)


# ------------------------------------------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------------------------------------------
def _read_maps(savedir, stem):
    from PIL import Image
    d16 = imgio.imread_gray16(os.path.join(savedir, "depth", stem + ".png"))
    n8 = imgio.imread_rgb(os.path.join(savedir, "normal", stem + ".png"))
    with Image.open(os.path.join(savedir, "shade", stem + ".png")) as im:
        assert im.mode == "L"
        s8 = np.asarray(im).copy()
    return d16, n8, s8


def check_cli(tmp_path, monkeypatch, device, run):
    """shared with tests/test_gbuffer_gpu.py.  run(extra args, savedir name) -> (savedir, written, gbuffer_written, recorded gbuffer() calls)"""
    out, written, gb_written, calls = run(["--gbuffer", "--gbuffer-acc-min", str(SYNTH_ACC_MIN)], "with")
    out0, written0, gb_written0, _ = run([], "without")
    assert [os.path.basename(p) for p in written] == [os.path.basename(p) for p in written0] == ["0_00.png", "1_00.png"]
    assert gb_written0 == [] and not any(os.path.exists(os.path.join(out0, s)) for s in ("depth", "normal", "shade", "gbuffer.json"))
    for p, q in zip(written, written0):
        assert open(p, "rb").read() == open(q, "rb").read()          # the rgb PNGs are those of a run without the flag
    assert [os.path.relpath(p, out) for p in gb_written] == [os.path.join(s, "%d_00.png" % f) for f in (0, 1) for s in ("depth", "normal", "shade")]
    table = json.load(open(os.path.join(out, "gbuffer.json")))
    assert table["acc_min"] == SYNTH_ACC_MIN and table["size"] == 32 and table["files"] == [os.path.relpath(p, out) for p in gb_written]
    assert len(calls) == 2
    for f, (rays, depth, acc, H, W, acc_min) in enumerate(calls):
        assert (H, W, acc_min) == (32, 32, SYNTH_ACC_MIN) and rays.device.type == device and rays.shape[0] == 1
        assert table["near"] == float(rays[0, 0, 6]) and table["far"] == float(rays[0, 0, 7])
        want = geometry.gbuffer(rays, depth, acc, H, W, acc_min)
        d16, n8, s8 = _read_maps(out, "%d_00" % f)
        assert np.array_equal(d16, want.depth16[0].cpu().numpy()) and np.array_equal(n8, want.normal8[0].cpu().numpy())
        assert np.array_equal(s8, want.shade8[0].cpu().numpy())
        code = d16[..., 0].astype(np.int64) * 256 + d16[..., 1]
        assert 0 < int((code == 0).sum()) < code.size          # valid and invalid pixels both occur
        dec = geometry.decode_depth16(torch.from_numpy(d16), table["near"], table["far"])
        z = want.z[0].cpu().double()
        assert float((dec - z)[code > 0].abs().max()) <= (table["far"] - table["near"]) / 65534          # the table decodes the file
    return out, calls


def _cli_runner(tmp_path, monkeypatch, device):
    from havatar_amd.harness import reenact
    root = str(tmp_path / "data")
    os.makedirs(root)
    split = synth.write_dataset(root, n_frames=2, img_res=128, photos=False)
    cfg_path, ckpt = str(tmp_path / "cfg.yml"), mu.checkpoint(tmp_path / "avatar.pth")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(synth.harness_config(), f)
    real = geometry.gbuffer

    def run(extra, name):
        calls = []

        def recording(rays, depth, acc, H, W, acc_min=0.5):
            calls.append((rays.clone(), depth.clone(), acc.clone(), H, W, acc_min))
            return real(rays, depth, acc, H, W, acc_min)
        monkeypatch.setattr(geometry, "gbuffer", recording)
        out = str(tmp_path / name)
        try:
            written = reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", out, "--split", split] + extra, device=device)
        finally:
            monkeypatch.setattr(geometry, "gbuffer", real)
        return out, written, list(reenact.main.gbuffer_written), calls
    return run


def test_cli_gbuffer_on_cpu_tensors(tmp_path, monkeypatch):
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    run = _cli_runner(tmp_path, monkeypatch, "cpu")
    out, calls = check_cli(tmp_path, monkeypatch, "cpu", run)
    # two frames per call: the same files, each its own frame's maps
    monkeypatch.setenv("HAVATAR_FRAME_BATCH", "2")
    outb, _, gb_b, calls_b = run(["--gbuffer", "--gbuffer-acc-min", str(SYNTH_ACC_MIN)], "batched")
    assert len(calls_b) == 1 and calls_b[0][0].shape[0] == 2
    assert [os.path.relpath(p, outb) for p in gb_b] == [os.path.join(s, "%d_00.png" % f) for f in (0, 1) for s in ("depth", "normal", "shade")]
    want = geometry.gbuffer(*calls_b[0])
    for f in (0, 1):
        d16, n8, s8 = _read_maps(outb, "%d_00" % f)
        assert np.array_equal(d16, want.depth16[f].numpy()) and np.array_equal(n8, want.normal8[f].numpy()) and np.array_equal(s8, want.shade8[f].numpy())
        one = _read_maps(out, "%d_00" % f)
        print("frame %d: batched maps %s the one-frame run's" % (f, "equal" if all(np.array_equal(a, b) for a, b in zip(one, (d16, n8, s8))) else "differ from"))
    monkeypatch.delenv("HAVATAR_FRAME_BATCH")
    # two ranks: each writes its own frames and its own table
    monkeypatch.setenv("WORLD_SIZE", "2")
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        outr, written, gb_r, calls_r = run(["--gbuffer", "--gbuffer-acc-min", str(SYNTH_ACC_MIN)], "ranks")
        assert [os.path.basename(p) for p in written] == ["%d_00.png" % rank] and len(calls_r) == 1
        assert [os.path.relpath(p, outr) for p in gb_r] == [os.path.join(s, "%d_00.png" % rank) for s in ("depth", "normal", "shade")]
        table = json.load(open(os.path.join(outr, "gbuffer_rank%dof2.json" % rank)))
        assert table["files"] == [os.path.relpath(p, outr) for p in gb_r]
        for a, b in zip(_read_maps(outr, "%d_00" % rank), _read_maps(out, "%d_00" % rank)):
            assert np.array_equal(a, b)
    assert not os.path.exists(os.path.join(outr, "gbuffer.json"))

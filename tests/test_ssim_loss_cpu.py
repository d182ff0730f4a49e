"""CPU: havatar_amd.metrics.ssim_loss (the statement routes) against metrics.aten_statement in float64, its refusals, the binding of the
entries of csrc/hav_ssim_loss.hip within ABI 8, the compiler's output for gfx950, and the --ssim-weight / --val-metrics flags of the two
training command lines on CPU tensors."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import metrics_util as mu
from havatar_amd import metrics, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------------------------------------------
# the function
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", mu.KINDS)
def test_cpu_pairs_equal_the_float64_statement(kind, dtype):
    """value: 1 - mean of the statement on the .double() pair, rounded to the pair's dtype at most; so is the gradient"""
    a, b = (t.to(dtype) for t in mu.pair(kind, (2, 3, 12, 13)))
    want = 1.0 - metrics.aten_statement(a.double(), b.double())[0].mean()
    tol = 0.0 if dtype == torch.float64 else 2.0 ** -24
    with torch.no_grad():
        got = metrics.ssim_loss(a, b)
    assert got.dtype == dtype and got.dim() == 0 and abs(float(got) - float(want)) <= tol
    x = a.clone().requires_grad_(True)
    got = metrics.ssim_loss(x, b)
    assert got.dtype == dtype and got.requires_grad and abs(float(got.detach()) - float(want)) <= tol
    x64 = a.clone().double().requires_grad_(True)
    g64, = torch.autograd.grad(1.0 - metrics.aten_statement(x64, b.double())[0].mean(), x64)
    g, = torch.autograd.grad(got, x)
    assert g.dtype == dtype and float((g.double() - g64).abs().max()) <= tol * float(g64.abs().max())
    # a data range of its own: invariant under a common scale when L scales along
    if dtype == torch.float64:
        assert abs(float(metrics.ssim_loss(a * 255, b * 255, data_range=255.0)) - float(want)) <= 1e-12


def test_gradcheck_of_the_cpu_route():
    a, b = (t.double() for t in mu.pair("texture", (1, 2, 12, 13)))
    x = a.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: metrics.ssim_loss(t, b), (x,), eps=1e-6, atol=1e-7, rtol=1e-5)
    # the statement route also carries the gradient to the second image
    y = b.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: metrics.ssim_loss(a, t), (y,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_refusals():
    from havatar_amd.native import ssim_ops
    z = torch.zeros
    with pytest.raises(ValueError, match=r"ssim_loss takes float.*uint8.*\(1, 16, 16, 3\)"):
        metrics.ssim_loss(z(1, 16, 16, 3, dtype=torch.uint8), z(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(1, 3, 16, 16\) and \(1, 3, 16, 17\)"):
        metrics.ssim_loss(z(1, 3, 16, 16, requires_grad=True), z(1, 3, 16, 17))
    with pytest.raises(ValueError, match=r"H, W >= 11.*\(1, 3, 10, 64\)"):
        metrics.ssim_loss(z(1, 3, 10, 64, requires_grad=True), z(1, 3, 10, 64))
    with pytest.raises(ValueError, match=r"dtype.*float32.*float64"):
        metrics.ssim_loss(z(1, 3, 16, 16), z(1, 3, 16, 16, dtype=torch.float64))
    # the node's wrapper takes HIP tensors only, and its backward refuses to be differentiated again before it looks at anything
    with pytest.raises(RuntimeError, match="HIP"):
        ssim_ops.ssim_mean(z(1, 3, 16, 16, requires_grad=True), z(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="HIP"):
        ssim_ops.ssim_grad(z(1), z(1, 3, 16, 16), z(1, 3, 16, 16))
    with torch.enable_grad(), pytest.raises(RuntimeError, match=r"once differentiable.*HAVATAR_METRICS=0.*ATen statement"):
        ssim_ops.SsimMean.backward(None, z(1))


def test_cpu_pairs_never_reach_the_node(monkeypatch):
    from havatar_amd.native import ssim_ops
    ran = []
    monkeypatch.setattr(ssim_ops, "ssim_mean", lambda *a, **k: ran.append(1))
    monkeypatch.setenv("HAVATAR_METRICS", "1")
    a, b = mu.pair("texture", (1, 3, 16, 16))
    metrics.ssim_loss(a.clone().requires_grad_(True), b).backward()
    metrics.ssim_loss(a, b)
    assert ran == []


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's entries
# ------------------------------------------------------------------------------------------------------------------------------------
def _blocks(B, Cc, H, W):
    """workgroups of the two launches: one per 32 x 32 tile of the map, one per 32 x 32 tile of pixels, per (sample, channel)"""
    return B * Cc * ((-(-(H - 10) // 32)) * (-(-(W - 10) // 32)) + (-(-H // 32)) * (-(-W // 32)))


def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib, build
    L = _lib.lib()
    assert L.hav_ssim_grad_blocks.restype is C.c_int64 and L.hav_ssim_grad_blocks.argtypes == [C.c_int] * 4
    assert L.hav_ssim_loss_bwd_f32.restype is C.c_int
    assert L.hav_ssim_loss_bwd_f32.argtypes == [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_float, C.c_void_p]
    assert _lib.ABI_VERSION == L.hav_abi_version() == 8          # additions within the version: nothing existing changed
    assert "hav_ssim_loss.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    for name in ("hav_ssim_grad_blocks", "hav_ssim_loss_bwd_f32"):
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "#define HAV_ABI_VERSION 8" in hdr
    # the count: 0 for what is not covered, map tiles + pixel tiles otherwise
    assert _blocks(1, 3, 42, 44) == 3 * (2 + 4) and _blocks(2, 3, 75, 76) == 6 * (9 + 9)
    for B, Cc, H, W in ((1, 1, 11, 11), (2, 3, 12, 13), (1, 3, 42, 44), (1, 2, 43, 47), (2, 3, 75, 76), (2, 3, 64, 64), (1, 3, 1024, 1024)):
        assert L.hav_ssim_grad_blocks(B, Cc, H, W) == _blocks(B, Cc, H, W), (B, Cc, H, W)
    for B, Cc, H, W in ((0, 3, 64, 64), (1, 0, 64, 64), (1, 3, 10, 64), (1, 3, 64, 10), (-1, 3, 64, 64), (65536, 65536, 42, 42)):
        assert L.hav_ssim_grad_blocks(B, Cc, H, W) == 0, (B, Cc, H, W)
    # refusals that need no device: HAV_EINVAL for null pointers and sizes below 1, HAV_EUNSUP below the window, all before any launch
    one = C.c_void_p(16)          # never dereferenced: the checks come first
    for miss in range(5):
        ptrs = [None if k == miss else one for k in range(5)]
        assert L.hav_ssim_loss_bwd_f32(*ptrs, 1, 3, 16, 16, 1.0, None) == -1
    for B, Cc, H, W in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, -1)):
        assert L.hav_ssim_loss_bwd_f32(one, one, one, one, one, B, Cc, H, W, 1.0, None) == -1
    for dr in (0.0, -1.0, float("nan"), float("inf")):
        assert L.hav_ssim_loss_bwd_f32(one, one, one, one, one, 1, 3, 16, 16, dr, None) == -1
    for H, W in ((10, 64), (64, 10), (1, 1)):
        assert L.hav_ssim_loss_bwd_f32(one, one, one, one, one, 1, 3, H, W, 1.0, None) == -2
    assert L.hav_ssim_loss_bwd_f32(one, one, one, one, one, 65536, 65536, 42, 42, 1.0, None) == -2          # 2^32 workgroups
    src = open(os.path.join(ROOT, "havatar_amd", "csrc", "hav_ssim_loss.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "getenv" not in code and not re.search(r"atomic", code, re.I) and not re.search(r"hipMalloc|Synchronize", code)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_private_segment_no_spill_and_the_documented_lds(tmp_path):
    dst = str(tmp_path / "hav_ssim_loss.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_ssim_loss.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    kernels = re.findall(r"\.name:\s+(\S*_kernel\S*)", text)
    # each of the two kernels with 16-byte and with narrow accesses
    assert len(set(kernels)) == 4 and sum("ssim_deriv_tile" in k for k in kernels) == 2 and sum("ssim_adjoint_tile" in k for k in kernels) == 2, kernels
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == len(kernels) and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == 2 * len(kernels) and all(v == 0 for v in spills), spills
    lds = dict(zip(kernels, (int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text))))
    for k, v in lds.items():
        # 2 x 42 x 45 floats + 5 x 42 x 32 doubles (+ 8 bytes the compiler pads); 3 x (42 + 32) x 43 doubles
        assert v == (2 * 42 * 45 * 4 + 5 * 42 * 32 * 8 + 8 if "deriv" in k else 3 * (42 + 32) * 43 * 8), lds
        assert v <= 80 * 1024          # two workgroups per compute unit (160 KiB)


# ------------------------------------------------------------------------------------------------------------------------------------
# stage one
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s1(tmp_path_factory):
    """stage one with the reference's patch sampling: one 64 x 64 patch per frame of a 128 x 128 image"""
    root = str(tmp_path_factory.mktemp("ssim_s1"))
    split = synth.write_dataset(root, n_frames=2, img_res=128)
    cfg = synth.harness_config(render_size=128, img_res=128)
    cfg["experiment"].update(patch_rgb=True)
    path = os.path.join(root, "cfg.yml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    plain = os.path.join(root, "cfg_rays.yml")
    with open(plain, "w") as f:
        yaml.safe_dump(synth.harness_config(), f)
    return root, path, plain, split, cfg


def test_training_loss_adds_the_weighted_term(s1):
    from havatar_amd.dataloader.dataloader import Loader
    from havatar_amd.harness import train
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    cfg = CfgNode(s1[4])
    np.random.seed(7)
    tl = Loader(split_file=s1[3], mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg, white_bg=True,
                shuffle=False)
    idx, batch = next(iter(tl))
    torch.manual_seed(5)
    trainer = synth.fill_state_dict(Trainer(cfg, len(tl.dataset))).train()
    inp, target, ray_mask = train.step_inputs(idx, batch, "cpu")
    assert tuple(target.shape) == (2, 64 * 64, 3)
    seen = []
    real = trainer.forward

    def forward(**kw):          # the patch of the run with the term, for the restatement below
        out = real(**kw)
        seen.append((out[0] if out[4] is None else out[4]).detach())
        return out

    trainer.forward = forward
    loss0, parts0, _ = train.training_loss(trainer, cfg, inp, target, ray_mask, torch.nn.functional.mse_loss)
    loss1, parts1, _ = train.training_loss(trainer, cfg, inp, target, ray_mask, torch.nn.functional.mse_loss, ssim_weight=0.25)
    assert "patch_ssim_loss" not in parts0 and set(parts1) == set(parts0) | {"patch_ssim_loss"}
    assert torch.equal(seen[0], seen[1])          # deterministic sampling: the two forwards render the same patch
    img, gt = (t[..., :3].reshape(2, 64, 64, 3).permute(0, 3, 1, 2) for t in (seen[1], target))
    want = metrics.ssim_loss(img, gt)
    assert 0 < float(want) < 1 and abs(float(parts1["patch_ssim_loss"].detach()) - float(want)) <= 1e-7
    assert abs(float(loss1) - (float(loss0) + 0.25 * float(want))) <= 1e-6 * abs(float(loss0) + 0.25 * float(want))
    assert parts1["patch_ssim_loss"].requires_grad
    # rays that are no square image are refused
    with pytest.raises(RuntimeError, match=r"square patch.*patch_rgb"):
        train.patch_ssim_loss(torch.zeros(2, 256 + 1, 3), torch.zeros(2, 256 + 1, 3))
    with pytest.raises(RuntimeError, match=r"square patch.*patch_rgb"):
        train.patch_ssim_loss(torch.zeros(2, 100, 3), torch.zeros(2, 100, 3))


def test_stage_one_cli_refuses_the_weight_without_patch_rgb(s1, tmp_path):
    from havatar_amd.harness import train
    with pytest.raises(RuntimeError, match=r"--ssim-weight needs experiment.patch_rgb"):
        train.main(["--logdir", str(tmp_path / "x"), "--datadir", s1[0], "--config", s1[2], "--ssim-weight", "0.2", "--max-steps", "1"], device="cpu")
    assert not os.path.exists(tmp_path / "x")


class _Recorder:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, name, value, step):
        self.scalars.append((name, float(value), int(step)))

    def add_image(self, *a, **k):
        pass


@pytest.mark.parametrize("flags", [(), ("--val-metrics", "--ssim-weight", "0.2", "--percep", "none")], ids=["none", "both"])
def test_stage_one_cli_flags(s1, tmp_path, monkeypatch, flags):
    """without the flags the scalar stream has neither name; --val-metrics logs validation/ssim of the validation frame; --ssim-weight logs
    train/patch_ssim_loss"""
    from havatar_amd.harness import train
    monkeypatch.setenv("HAVATAR_PRETRAIN_WC", "2")
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    rec = _Recorder()
    monkeypatch.setattr(train, "make_writer", lambda logdir: rec)
    cfg_path = s1[1] if "--ssim-weight" in flags else s1[2]
    assert train.main(["--logdir", str(tmp_path / "log"), "--datadir", s1[0], "--config", cfg_path, "--max-steps", "1"] + list(flags),
                      device="cpu") == 0
    names = [n for n, _, _ in rec.scalars]
    assert "validation/psnr" in names and "validation/lpips" not in names
    assert ("validation/ssim" in names) == ("--val-metrics" in flags) and ("train/patch_ssim_loss" in names) == ("--ssim-weight" in flags)
    for n, v, _ in rec.scalars:
        if n in ("validation/ssim", "train/patch_ssim_loss"):
            assert np.isfinite(v) and 0 < v < 1, (n, v)


# ------------------------------------------------------------------------------------------------------------------------------------
# stage two
# ------------------------------------------------------------------------------------------------------------------------------------
def test_hd_cli_runs_with_a_finite_ssim_loss(tmp_path, monkeypatch):
    from havatar_amd.harness import train_hd
    root = str(tmp_path / "data")
    os.makedirs(root)
    synth.write_dataset(root, n_frames=2, img_res=64)
    cfg_path = os.path.join(root, "cfg.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(synth.harness_config(render_size=32, gen_size=64, img_res=64), f)
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    seen, real = [], train_hd.joint_step

    def spy(*a, **kw):
        s = real(*a, **kw)
        seen.append((kw.get("ssim_weight"), s))
        return s

    monkeypatch.setattr(train_hd, "joint_step", spy)
    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)
    assert train_hd.main(["--logdir", str(tmp_path / "log"), "--datadir", root, "--config", cfg_path, "--ssim-weight", "0.2", "--percep", "none",
                          "--iters", "2"], device="cpu") == 1
    assert [w for w, _ in seen] == [0.2, 0.2]
    for _, s in seen:
        assert np.isfinite(s["ssim_loss"]) and 0 < s["ssim_loss"] < 2 and np.isfinite(s["g_loss"])

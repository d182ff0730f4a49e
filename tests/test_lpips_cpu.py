"""CPU: the LPIPS-VGG module (model/lpips.py) against the float64 restatement of its definition (tests/lpips_util.py), its weight loading,
the refusal of an unloaded module, the binding of the three entries of csrc/hav_lpips.hip within ABI 8, the wrappers' refusals and
eligibility (native/lpips_ops.py), the switch, the compiler's output for gfx950, and `--percep native` of both command lines."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import lpips_util as lu
from havatar_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------------------------------------------
# the function
# ------------------------------------------------------------------------------------------------------------------------------------
def test_module_in_float64_matches_the_restatement():
    """value to 1e-12, gradient into in0 to 1e-10 of its largest entry (both sides float64; they differ in the order of a few sums)"""
    vgg, lin = lu.weights()
    m = lu.module(dtype=torch.float64)
    in0, in1 = (t.double() for t in lu.images((2, 3, 32, 64)))
    a, b = in0.clone().requires_grad_(True), in0.clone().requires_grad_(True)
    v, ref = m(a, in1), lu.lpips64(b, in1, vgg, lin)
    assert v.shape == (2, 1, 1, 1) and v.dtype == torch.float64
    assert (v - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    ga, gb = torch.autograd.grad(v.sum(), a)[0], torch.autograd.grad(ref.sum(), b)[0]
    assert gb.abs().max().item() > 0 and (ga - gb).abs().max().item() <= 1e-10 * gb.abs().max().item()
    # normalize=True maps [0, 1] to [-1, 1] first
    vn = m((in0 + 1) / 2, (in1 + 1) / 2, normalize=True)
    assert (vn - ref).abs().max().item() <= 1e-12
    # every parameter frozen, eval-only, the harnesses' call
    assert not any(p.requires_grad for p in m.parameters()) and not m.training and not m.train().training
    assert m.forward(in0, in1).mean().ndim == 0


@pytest.mark.parametrize("shape", [(1, 3, 128, 256), (2, 3, 64, 128)])
def test_aten_route_is_the_float32_statement_bit_for_bit(shape, monkeypatch):
    """the module without its nodes (CPU tensors; HAVATAR_LPIPS=0 takes the same code on the device) against the in-test ATen float32
    restatement, op for op what the `lpips` package states: the same bits, value and gradient into in0"""
    monkeypatch.setenv("HAVATAR_LPIPS", "0")
    vgg, lin = lu.weights()
    m = lu.module()
    in0, in1 = lu.images(shape)
    a, b = in0.clone().requires_grad_(True), in0.clone().requires_grad_(True)
    v, ref = m(a, in1), lu.lpips_aten32(b, in1, vgg, lin)
    assert torch.equal(v, ref)
    assert torch.equal(torch.autograd.grad(v.sum(), a)[0], torch.autograd.grad(ref.sum(), b)[0])


def test_identical_inputs_give_exactly_zero():
    m = lu.module()
    x = lu.images((1, 3, 32, 32))[0]
    assert torch.equal(m(x, x.clone()), torch.zeros(1, 1, 1, 1))


def test_unloaded_module_refuses_forward():
    from havatar_amd.model import lpips
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        lpips.LPIPS(net="vgg")(x, x)
    assert torch.isfinite(lpips.LPIPS(net="vgg", allow_random=True)(x, x)).all()
    with pytest.raises(ValueError, match="vgg"):
        lpips.LPIPS(net="alex")


# ------------------------------------------------------------------------------------------------------------------------------------
# weight files
# ------------------------------------------------------------------------------------------------------------------------------------
def _constant_files():
    """(vgg, lin, expected): every tensor filled with a constant of its own; expected maps the module's key to the constant"""
    from havatar_amd.model import lpips
    vgg, lin, expected = {}, {}, {}
    for i, (key, fkey, shape) in enumerate(lpips.key_table()):
        if fkey is None:
            continue
        c = 1.0 + i
        (lin if key.startswith("lin") else vgg)[fkey] = torch.full(shape, c)
        expected[key] = c
    return vgg, lin, expected


def _check_constants(m, expected):
    sd = m.state_dict()
    assert set(expected) | {"scaling_layer.shift", "scaling_layer.scale"} == set(sd)
    for key, c in expected.items():
        assert torch.equal(sd[key], torch.full_like(sd[key], c)), key
    assert torch.allclose(sd["scaling_layer.shift"].flatten(), torch.tensor(lu.SHIFT)) and torch.allclose(sd["scaling_layer.scale"].flatten(), torch.tensor(lu.SCALE))
    assert m.weights_loaded


def test_three_file_layouts_land_in_the_right_layers(tmp_path):
    from havatar_amd.model import lpips
    vgg, lin, expected = _constant_files()
    assert len(vgg) == 26 and len(lin) == 5
    # 1: torchvision's keys and the package's lin file (with its duplicate lins.K.* keys)
    lin_dup = dict(lin)
    lin_dup.update({"lins.%d.model.1.weight" % k: torch.zeros_like(lin["lin%d.model.1.weight" % k]) for k in range(5)})
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin_dup, tmp_path / "lin.pth")
    _check_constants(lpips.load_weights(lpips.LPIPS(), vgg=str(tmp_path / "vgg16.pth"), lin=str(tmp_path / "lin.pth")), expected)
    # 2: the same keys without the `features.` prefix
    torch.save({k[len("features."):]: v for k, v in vgg.items()}, tmp_path / "bare.pth")
    _check_constants(lpips.load_weights(lpips.LPIPS(), vgg=str(tmp_path / "bare.pth"), lin=str(tmp_path / "lin.pth")), expected)
    # 3: a whole LPIPS state dict, as the package's module writes it (lin layers named twice)
    whole = {key: torch.full(shape, expected[key]) for key, fkey, shape in lpips.key_table() if fkey is not None}
    whole["scaling_layer.shift"], whole["scaling_layer.scale"] = torch.tensor(lu.SHIFT).view(1, 3, 1, 1), torch.tensor(lu.SCALE).view(1, 3, 1, 1)
    whole.update({"lins.%d.model.1.weight" % k: whole["lin%d.model.1.weight" % k] for k in range(5)})
    torch.save(whole, tmp_path / "whole.pth")
    _check_constants(lpips.load_weights(lpips.LPIPS(), state=str(tmp_path / "whole.pth")), expected)
    m = lpips.LPIPS()
    m.load_state_dict(whole)
    _check_constants(m, expected)


def test_missing_and_misshaped_keys_are_refused_by_name():
    from havatar_amd.model import lpips
    vgg, lin, _ = _constant_files()
    short = {k: v for k, v in vgg.items() if k != "features.17.bias"}
    with pytest.raises(RuntimeError, match=r"'features\.17\.bias' is missing"):
        lpips.load_weights(lpips.LPIPS(), vgg=short, lin=lin)
    bad = dict(vgg)
    bad["features.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(RuntimeError, match=r"'features\.5\.weight'.*\(128, 64, 1, 1\).*\(128, 64, 3, 3\)"):
        lpips.load_weights(lpips.LPIPS(), vgg=bad, lin=lin)
    with pytest.raises(RuntimeError, match=r"'lin3\.model\.1\.weight' is missing"):
        lpips.load_weights(lpips.LPIPS(), vgg=vgg, lin={k: v for k, v in lin.items() if not k.startswith("lin3")})
    m = lpips.LPIPS()
    with pytest.raises(RuntimeError, match="both `vgg` and `lin`"):
        lpips.load_weights(m, vgg=vgg)
    assert not m.weights_loaded


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's entries and their wrappers
# ------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib, build
    L = _lib.lib()
    assert L.hav_lpips_head_blocks.restype is C.c_int64 and len(L.hav_lpips_head_blocks.argtypes) == 4
    assert L.hav_lpips_head_fwd.restype is C.c_int and len(L.hav_lpips_head_fwd.argtypes) == 10
    assert L.hav_lpips_head_bwd.restype is C.c_int and len(L.hav_lpips_head_bwd.argtypes) == 11
    assert L.hav_relu_mask_bwd.restype is C.c_int and len(L.hav_relu_mask_bwd.argtypes) == 8 and L.hav_relu_mask_bwd.argtypes[6] is C.c_int64
    for fn in (L.hav_lpips_head_fwd, L.hav_lpips_head_bwd, L.hav_relu_mask_bwd):
        assert fn.argtypes[-1] is C.c_void_p          # every entry takes the stream
    assert _lib.ABI_VERSION == L.hav_abi_version() == 8          # additions within the version: nothing existing changed
    assert "hav_lpips.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    for name in ("hav_lpips_head_blocks", "hav_lpips_head_fwd", "hav_lpips_head_bwd", "hav_relu_mask_bwd"):
        assert re.search(r"\b%s\(" % name, hdr), name
    # sizes and refusals that need no device: the partials' count, and HAV_EINVAL before any launch
    assert L.hav_lpips_head_blocks(2, 64, 3, 5) == 2 and L.hav_lpips_head_blocks(1, 512, 32, 64) == 32 and L.hav_lpips_head_blocks(0, 1, 1, 1) == 0
    assert L.hav_lpips_head_fwd(None, None, None, None, None, 1, 1, 1, 1, None) == -1
    assert L.hav_lpips_head_bwd(None, None, None, None, None, None, 1, 1, 1, 1, None) == -1
    assert L.hav_relu_mask_bwd(None, None, None, None, 1, 1, 1, None) == -1
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "havatar_amd", "csrc", "hav_lpips.hip")).read())
    assert "getenv" not in src and not re.search(r"atomic", src, re.I)          # no environment reads, no atomics in the file's code


def test_wrappers_refuse_cpu_tensors():
    from havatar_amd.native import lpips_ops as o
    f, w, g = torch.zeros(1, 64, 4, 32), torch.zeros(64), torch.zeros(1)
    blob = torch.zeros(8, dtype=torch.uint8)
    for call in (lambda: o.head_fwd(f, f, w), lambda: o.head_bwd(g, f, f, w), lambda: o.lpips_head(f, f, w.view(1, 64, 1, 1)),
                 lambda: o.relu_mask_bwd(f, f), lambda: o.relu_mask_bwd(f, f, want_bias=True),
                 lambda: o.conv_relu_frozen(f, w, blob, blob, 64), lambda: o.LpipsHead.apply(f, f, w),
                 lambda: o.ConvReluFrozen.apply(f, w, blob, blob, 64)):
        with pytest.raises(RuntimeError, match="HIP float32"):
            call()
    assert not o.conv_relu_eligible(f, torch.zeros(64, 64, 3, 3))


class _Like:
    """what eligibility reads of a tensor"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


@pytest.mark.parametrize("cin,cout,h,w,ok", [
    (64, 64, 4, 32, True), (128, 256, 8, 16, True), (512, 512, 8, 16, True), (64, 128, 16, 48, True), (64, 64, 128, 256, True),
    (3, 64, 128, 256, False),          # conv1_1
    (32, 64, 4, 32, False), (64, 32, 4, 32, False), (64, 96, 4, 32, False), (96, 64, 4, 32, False),          # Cin, Cout % 64
    (512, 512, 4, 8, False),           # slice 5 of a 64 x 128 image
    (64, 64, 4, 16, False), (64, 64, 6, 32, False), (64, 64, 8, 24, False), (64, 64, 12, 16, False), (64, 64, 4, 48, False),
    (64, 64, 8, 48, True), (64, 64, 12, 32, True)])
def test_eligibility_shape_by_shape(cin, cout, h, w, ok):
    from havatar_amd.native import lpips_ops as o
    assert o.conv_relu_eligible(_Like(2, cin, h, w), _Like(cout, cin, 3, 3)) is ok
    rule = cin % 64 == 0 and cout % 64 == 0 and ((h % 4 == 0 and w % 32 == 0) or (h % 8 == 0 and w % 16 == 0))
    assert rule is ok


def test_eligibility_wants_a_hip_float32_tensor():
    from havatar_amd.native import lpips_ops as o
    x, wt = _Like(1, 64, 4, 32), _Like(64, 64, 3, 3)
    assert o.conv_relu_eligible(x, wt)
    x.dtype = torch.float64
    assert not o.conv_relu_eligible(x, wt)
    x.dtype, x.is_cuda = torch.float32, False
    assert not o.conv_relu_eligible(x, wt)
    assert not o.conv_relu_eligible(_Like(1, 64, 4, 32), _Like(64, 64, 1, 1)) and not o.conv_relu_eligible(_Like(1, 128, 4, 32), wt)


def test_switch_is_read_at_the_call_and_changes_nothing_on_cpu_tensors(monkeypatch):
    from havatar_amd.native import lpips_ops as o
    monkeypatch.delenv("HAVATAR_LPIPS", raising=False)
    assert o.enabled() is (o.DEFAULT != "0")
    monkeypatch.setenv("HAVATAR_LPIPS", "1")
    assert o.enabled()
    monkeypatch.setenv("HAVATAR_LPIPS", "0")
    assert not o.enabled()
    m = lu.module()
    in0, in1 = lu.images((1, 3, 32, 32))
    res = []
    ran = []
    monkeypatch.setattr(o, "conv_relu_frozen", lambda *a, **k: ran.append("conv_relu"))
    monkeypatch.setattr(o, "lpips_head", lambda *a, **k: ran.append("head"))
    for v in ("0", "1", None):
        monkeypatch.delenv("HAVATAR_LPIPS", raising=False)
        if v is not None:
            monkeypatch.setenv("HAVATAR_LPIPS", v)
        a = in0.clone().requires_grad_(True)
        y = m(a, in1)
        res.append((y.detach(), torch.autograd.grad(y.sum(), a)[0]))
    assert all(torch.equal(p, q) for r in res[1:] for p, q in zip(res[0], r)) and ran == []


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_private_segment_and_no_spill(tmp_path):
    dst = str(tmp_path / "hav_lpips.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_lpips.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    kernels = re.findall(r"\.name:\s+(\S*_kernel\S*)", text)
    # head forward and backward and the mask with 16-byte and 4-byte accesses, the final sum, the mask with the bias sum
    assert len(set(kernels)) == 8 and sum("lpips_head" in k for k in kernels) == 5 and sum("relu_mask" in k for k in kernels) == 3, kernels
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == len(kernels) and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == 2 * len(kernels) and all(v == 0 for v in spills), spills


# ------------------------------------------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("lpips_files")
    vgg, lin = lu.weights()
    torch.save(dict(vgg), root / "vgg16.pth")
    torch.save(dict(lin), root / "lin.pth")
    return str(root / "vgg16.pth"), str(root / "lin.pth")


@pytest.fixture(scope="module")
def hd_cli(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("cli_hd"))
    synth.write_dataset(root, n_frames=2, img_res=64)
    cfg = synth.harness_config(render_size=32, gen_size=64, img_res=64)
    path = os.path.join(root, "cfg.yml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return root, path


def _hd_main(cli, logdir, *extra):
    from havatar_amd.harness import train_hd
    os.environ["HAVATAR_WORKERS"] = "0"
    try:
        random.seed(42)
        np.random.seed(42)
        torch.manual_seed(42)
        return train_hd.main(["--logdir", logdir, "--datadir", cli[0], "--config", cli[1]] + list(extra), device="cpu")
    finally:
        os.environ.pop("HAVATAR_WORKERS", None)


def test_hd_cli_native_refuses_without_files_or_package(hd_cli, tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "lpips", None)          # `import lpips` raises ImportError, installed or not
    with pytest.raises(RuntimeError, match=r"--percep-vgg.*--percep-lin"):
        _hd_main(hd_cli, str(tmp_path / "x"), "--percep", "native", "--iters", "1")
    with pytest.raises(RuntimeError, match=r"both --percep-vgg"):
        _hd_main(hd_cli, str(tmp_path / "x"), "--percep", "native", "--percep-vgg", "somewhere.pth", "--iters", "1")


def test_hd_cli_native_runs_an_iteration_with_a_finite_percep_loss(hd_cli, files, tmp_path, monkeypatch):
    from havatar_amd.harness import train_hd
    from havatar_amd.model import lpips
    monkeypatch.setitem(sys.modules, "lpips", None)
    seen, real = [], train_hd.joint_step

    def spy(i, batch, nets, optims, cfg, su_args, percep=None, **kw):
        s = real(i, batch, nets, optims, cfg, su_args, percep, **kw)
        seen.append((percep, s))
        return s

    monkeypatch.setattr(train_hd, "joint_step", spy)
    assert _hd_main(hd_cli, str(tmp_path / "log"), "--percep", "native", "--percep-vgg", files[0], "--percep-lin", files[1], "--iters", "1") == 0
    (percep, s), = seen
    assert isinstance(percep, lpips.LPIPS) and percep.weights_loaded
    assert np.isfinite(float(s["percep_loss"])) and float(s["percep_loss"]) > 0


@pytest.fixture(scope="module")
def s1_cli(tmp_path_factory):
    """stage one with the reference's patch sampling: one 64 x 64 patch per frame of a 128 x 128 image"""
    root = str(tmp_path_factory.mktemp("cli_s1"))
    synth.write_dataset(root, n_frames=2, img_res=128)
    cfg = synth.harness_config(render_size=128, img_res=128)
    cfg["experiment"].update(patch_rgb=True, validate_every=1000, save_every=1000)
    path = os.path.join(root, "cfg.yml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return root, path


def test_stage_one_cli_native_refuses_without_files_or_package(s1_cli, tmp_path, monkeypatch):
    from havatar_amd.harness import train
    monkeypatch.setitem(sys.modules, "lpips", None)
    with pytest.raises(RuntimeError, match=r"--percep-vgg.*--percep-lin"):
        train.main(["--logdir", str(tmp_path / "x"), "--datadir", s1_cli[0], "--config", s1_cli[1], "--percep", "native", "--max-steps", "1"],
                   device="cpu")


def test_stage_one_cli_native_runs_an_iteration_with_a_finite_percep_loss(s1_cli, files, tmp_path, monkeypatch):
    from havatar_amd.harness import train
    monkeypatch.setitem(sys.modules, "lpips", None)
    monkeypatch.setenv("HAVATAR_PRETRAIN_WC", "2")
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    seen, real = [], train.training_loss

    def spy(*a, **kw):
        loss, parts, psnr = real(*a, **kw)
        seen.append(parts)
        return loss, parts, psnr

    monkeypatch.setattr(train, "training_loss", spy)
    # (validation and the checkpoint of the first iteration are the harness's own; what is checked here is the loss term)
    monkeypatch.setattr(train, "validate", lambda trainer, cfg, batch, H, W, device, f: (torch.zeros(1, H, W, 3), torch.zeros(1, H, W, 3), 0.0, 0.0))
    last = train.main(["--logdir", str(tmp_path / "log"), "--datadir", s1_cli[0], "--config", s1_cli[1], "--percep", "native",
                       "--percep-vgg", files[0], "--percep-lin", files[1], "--max-steps", "1"], device="cpu")
    assert last == 0 and len(seen) == 1
    v = float(seen[0]["patch_percep_loss"].detach())
    assert np.isfinite(v) and v > 0

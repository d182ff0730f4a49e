"""CPU: the stage-two joint step (harness/train_hd.py::joint_step) against what the REFERENCE's Trainer, SWGAN_unet, Discriminator and helpers
give for the same driver (harness/stage2_step_cases.py, recorded in tests/golden/stage2_step.npz by tools/gen_golden_stage2_step.py), its
gradient flow, the command line (run, checkpoint keys, sample, resume, refusals), and what can be said of the loss node without a GPU
(binding, eligibility, refusals, code generation).

Bars.  Scalars and gradients: tests/test_harness.py::_check_step's (2e-4 of the value / of the tensor's largest gradient; 1e-2 for the
skinning-volume decoder, whose small gradients are differences of large cancelling terms; PSNR 1e-2 absolute).  Two kinds of parameter are
left out of the gradient comparison, as oracle/gen_golden_harness.py leaves them out of the stage-one fixture: the decoder's conv biases in
front of InstanceNorm3d(affine=False), whose gradient is identically zero (rounding noise of 1e-9 .. 1e-12 in float32), and the NoiseInjection
strengths, whose gradient is the sum over every pixel of (gradient x freshly drawn noise), a cancelling sum with 1e-3 of float32 rounding.
Discriminator scalars: tests/test_discriminator_cpu.py's float32 bar (1e-5 of max(|value|, 1)).
Parameter checksums after an optimiser step and g_ema have no precedent in float32: measured once against the fixture (relative distance of
sum |.|, the largest over the parameters and both iterations: discriminator 7.2e-8 after both steps, generator 4.4e-7, Trainer 3.4e-5 without
the decoder's conv biases -- Adam's first update is lr * sign(gradient) wherever |gradient| >> eps, so a gradient whose sign is rounding noise
moves its weight by 2 lr = 1e-3 of a unit weight -- and g_ema 1.2e-11), the bar is 4 x that with a floor of 1e-6: 1e-6, 1.8e-6, 1.4e-4, 1e-6."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

from havatar_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = "/opt/rocm/bin/hipcc"
STEP_BARS = {"discriminator": 1e-6, "generator": 1.8e-6, "nerf_render": 1.4e-4, "g_ema": 1e-6}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "stage2_step.npz"))


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    return synth.write_dataset(str(tmp_path_factory.mktemp("dataset")), n_frames=2, img_res=128)


@pytest.fixture(scope="module")
def ours(split):
    from havatar_amd.harness import stage2_step_cases
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.model.styleUnet import Discriminator, SWGAN_unet
    from havatar_amd.utils import styleUnet_util
    return stage2_step_cases.run(Trainer, SWGAN_unet, Discriminator, styleUnet_util, split)


def _rows(ours, golden, net):
    """row index in `ours` of every parameter of the fixture (the two sides may register their parameters in another order)"""
    mine = list(ours["names_" + net])
    names = [str(n) for n in golden["names_" + net]]
    assert sorted(mine) == sorted(names), net
    return names, [mine.index(n) for n in names]


def _zero_gradient(name):
    return bool(re.match(r"headpose_skin_net\..*filters\.\d+\..*\.bias$", name))


def _cancelling(name):
    return name.endswith("noise.weight")


D_SCALARS = ("d", "real_score", "fake_score", "r1", "g")


@pytest.mark.parametrize("it", ["i0", "i1"])
def test_scalars_match_the_reference(ours, golden, it):
    from havatar_amd.harness import stage2_step_cases
    for k in stage2_step_cases.SCALARS:
        a, b = float(ours["%s_scalar_%s" % (it, k)]), float(golden["%s_scalar_%s" % (it, k)])
        print(it, k, a, b)
        if k in ("psnr", "SR_psnr"):
            assert abs(a - b) <= 1e-2, k
        elif k in D_SCALARS:
            assert abs(a - b) <= 1e-5 * max(abs(b), 1.0), k
        else:
            assert abs(a - b) <= 2e-4 * max(abs(b), 1e-3), k
    assert float(golden["i0_scalar_r1"]) > 0 and float(golden["i1_scalar_r1"]) == 0          # R1 ran in iteration 0 only


@pytest.mark.parametrize("it", ["i0", "i1"])
def test_gradients_match_the_reference(ours, golden, it):
    worst = {}
    for net in ("nerf_render", "generator"):
        names, rows = _rows(ours, golden, net)
        a, b = ours["%s_grad_%s_slices" % (it, net)][rows], golden["%s_grad_%s_slices" % (it, net)]
        gmax = golden["%s_grad_%s_sums" % (it, net)][:, 3]
        has = golden["%s_grad_%s_has" % (it, net)]
        for i, n in enumerate(names):
            if not has[i] or _zero_gradient(n) or _cancelling(n):
                continue
            tol = 1e-2 if n.startswith("headpose_skin_net.") else 2e-4
            err = np.abs(a[i] - b[i]).max() / gmax[i]
            worst[net] = max(worst.get(net, (0, "")), (err / tol, n))
            assert err <= tol, "%s %s %s: %.3e of the largest gradient, bar %.1e" % (it, net, n, err, tol)
            mine_max = ours["%s_grad_%s_sums" % (it, net)][rows][i, 3]
            assert abs(mine_max - gmax[i]) <= tol * gmax[i], (it, net, n)
    print(it, "worst error / bar:", worst)


@pytest.mark.parametrize("it", ["i0", "i1"])
def test_parameters_after_every_optimiser_step_match_the_reference(ours, golden, it):
    for key, net in (("%s_d_step_d_sums", "discriminator"), ("%s_r1_step_d_sums", "discriminator"), ("%s_step_discriminator_sums", "discriminator"),
                     ("%s_step_generator_sums", "generator"), ("%s_step_nerf_render_sums", "nerf_render"), ("%s_g_ema_sums", "generator")):
        names, rows = _rows(ours, golden, net)
        a, b = ours[key % it][rows], golden[key % it]
        bar = STEP_BARS["g_ema" if "g_ema" in key else net]
        dist = max(abs(a[i, 1] - b[i, 1]) / b[i, 1] for i, n in enumerate(names) if not _zero_gradient(n) and b[i, 1] > 0)
        print(key % it, "%.3e" % dist, "bar %.1e" % bar)
        assert dist <= bar, (key % it, dist)
    assert not np.array_equal(golden["i0_d_step_d_sums"], golden["i0_r1_step_d_sums"])          # the R1 step moved the discriminator
    assert np.array_equal(golden["i1_d_step_d_sums"], golden["i1_r1_step_d_sums"])


@pytest.mark.parametrize("it", ["i0", "i1"])
def test_gradient_flow(ours, golden, it):
    """after the generator backward: every Trainer parameter the reference run gives a gradient to has a non-zero one, every generator parameter
    has one, the backward touched no discriminator parameter; the discriminator's backward touched no generator or Trainer parameter"""
    names, rows = _rows(ours, golden, "nerf_render")
    mine, ref = ours["%s_grad_nerf_render_has" % it][rows], golden["%s_grad_nerf_render_has" % it]
    assert 100 < ref.sum() < len(names)
    assert all(mine[i] for i in range(len(names)) if ref[i]), [n for i, n in enumerate(names) if ref[i] and not mine[i]]
    assert ours["%s_grad_generator_has" % it].all() and golden["%s_grad_generator_has" % it].all()
    assert int(ours["%s_g_backward_touched_d" % it][0]) == 0 == int(golden["%s_g_backward_touched_d" % it][0])
    assert list(ours["%s_d_backward_touched_outside_d" % it]) == [0, 0] == list(golden["%s_d_backward_touched_outside_d" % it])


# ------------------------------------------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """a 64 x 64 dataset rendered at 32 x 32: validation and `latest.pt` every iteration, a numbered checkpoint every second one"""
    root = str(tmp_path_factory.mktemp("cli"))
    synth.write_dataset(root, n_frames=2, img_res=64)
    cfg = synth.harness_config(render_size=32, gen_size=64, img_res=64)
    cfg["experiment"].update(validate_every=1, save_every=2)
    path = os.path.join(root, "cfg.yml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return root, path


def _main(cli, logdir, *extra):
    from havatar_amd.harness import train_hd
    os.environ["HAVATAR_WORKERS"] = "0"
    try:
        random.seed(42)
        np.random.seed(42)
        torch.manual_seed(42)
        return train_hd.main(["--logdir", logdir, "--datadir", cli[0], "--config", cli[1]] + list(extra), device="cpu")
    finally:
        os.environ.pop("HAVATAR_WORKERS", None)


def test_cli_runs_checkpoints_samples_and_resumes_bitwise(cli, tmp_path):
    from havatar_amd.dataloader import imgio
    from havatar_amd.harness import train_hd
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert _main(cli, a, "--percep", "none", "--iters", "3") == 2
    ck = torch.load(os.path.join(a, "latest.pt"), map_location="cpu")
    assert tuple(ck.keys()) == train_hd.CKPT_KEYS and ck["iter"] == 2
    assert sorted(os.listdir(os.path.join(a, "sample"))) == ["000000.png", "000001.png", "000002.png"]
    assert sorted(os.listdir(os.path.join(a, "checkpoint"))) == ["checkpoint00000.ckpt", "checkpoint00002.ckpt"]
    assert tuple(torch.load(os.path.join(a, "checkpoint", "checkpoint00002.ckpt"), map_location="cpu").keys()) == train_hd.CKPT_KEYS
    png = imgio.imread_rgb(os.path.join(a, "sample", "000002.png"))
    assert png.shape == (2 * 64, 3 * 64, 3) and png.std() > 0          # [sample | lr_img | gt] per frame, the frames stacked
    # 3 + 2 resumed against 5 uninterrupted
    assert _main(cli, a, "--percep", "none", "--iters", "5", "--ckpt", os.path.join(a, "latest.pt"), "--continue-training") == 4
    assert _main(cli, b, "--percep", "none", "--iters", "5") == 4
    ra, rb = (torch.load(os.path.join(d, "latest.pt"), map_location="cpu") for d in (a, b))
    assert ra["iter"] == rb["iter"] == 4
    for key in ("nerf_render", "g", "d", "g_ema"):
        for k in rb[key]:
            assert torch.equal(ra[key][k], rb[key][k]), (key, k)
    assert torch.equal(ra["latent_codes"], rb["latent_codes"])
    assert any(not torch.equal(ra["g"][k], ck["g"][k]) for k in ck["g"])          # the two resumed iterations moved the weights


def test_cli_refuses_to_start_without_lpips(cli, tmp_path, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "lpips", None)          # `import lpips` raises ImportError, installed or not
    with pytest.raises(RuntimeError, match="--percep none"):
        _main(cli, str(tmp_path / "x"), "--iters", "1")


def test_cli_names_the_flag_of_a_missing_gan_checkpoint(cli, tmp_path):
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    with open(cli[1]) as f:
        cfg = CfgNode(yaml.safe_load(f))
    stage_one = str(tmp_path / "stage_one.ckpt")
    torch.save({"trainer_state_dict": Trainer(cfg, 2).state_dict()}, stage_one)
    with pytest.raises(FileNotFoundError, match="--gan-ckpt"):
        _main(cli, str(tmp_path / "x"), "--percep", "none", "--iters", "1", "--ckpt", stage_one, "--gan-ckpt", str(tmp_path / "absent.ckpt"))


def test_cli_starts_from_a_stage_one_checkpoint_and_a_gan_checkpoint(cli, tmp_path, monkeypatch):
    """load mode one (reference train_avatarHD.py:141-150): trainer_state_dict from --ckpt, g / d / g_ema from --gan-ckpt, optimisers fresh,
    the count from 0 -- what joint_step is first called with are the files' weights, and the step then runs"""
    from havatar_amd.harness import train_hd
    from havatar_amd.utils.cfgnode import CfgNode
    with open(cli[1]) as f:
        cfg = CfgNode(yaml.safe_load(f))
    su = train_hd.styleUnet_util.styleUnet_args()
    src = train_hd.build_nets(cfg, su, 2, "cpu")
    for k, seed in (("nerf_render", 3), ("generator", 4), ("discriminator", 5), ("g_ema", 6)):
        synth.fill_state_dict(src[k], seed=seed)          # four different sets of weights, none the constructors'
    stage_one, gan = str(tmp_path / "stage_one.ckpt"), str(tmp_path / "gan.ckpt")
    torch.save({"trainer_state_dict": src["nerf_render"].state_dict()}, stage_one)
    torch.save({"g": src["generator"].state_dict(), "d": src["discriminator"].state_dict(), "g_ema": src["g_ema"].state_dict()}, gan)
    seen, real = [], train_hd.joint_step

    def first_call(i, batch, nets, optims, *a, **k):
        if not seen:
            seen.append(i)
            for name, key in (("nerf_render", "nerf_render"), ("generator", "generator"), ("discriminator", "discriminator"), ("g_ema", "g_ema")):
                want = src[key].state_dict()
                assert all(torch.equal(v, want[n]) for n, v in nets[name].state_dict().items()), name
            assert all(len(o.state_dict()["state"]) == 0 for o in optims.values())
        return real(i, batch, nets, optims, *a, **k)
    monkeypatch.setattr(train_hd, "joint_step", first_call)
    log = str(tmp_path / "log")
    assert _main(cli, log, "--percep", "none", "--iters", "1", "--ckpt", stage_one, "--gan-ckpt", gan) == 0 and seen == [0]
    ck = torch.load(os.path.join(log, "latest.pt"), map_location="cpu")
    assert ck["iter"] == 0 and any(not torch.equal(v, src["generator"].state_dict()[n]) for n, v in ck["g"].items())          # the step ran


def test_root_script_sets_the_capture_variable_first():
    src = open(os.path.join(ROOT, "train_avatarHD.py")).read()
    assert src.index('os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")') < src.index("import main")
    assert "from havatar_amd.harness.train_hd import main, seed_all" in src and "import torch" not in src


def test_gan_loss_weight_schedule():
    from havatar_amd.harness.train_hd import gan_loss_weight
    assert gan_loss_weight(0) == gan_loss_weight(499) == 1e-3 and abs(gan_loss_weight(500) - 1.1e-3) < 1e-12
    assert gan_loss_weight(10 ** 6) == 0.1


# ------------------------------------------------------------------------------------------------------------------------------------
# the loss node without a GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib, build
    L = _lib.lib()
    assert L.hav_s2_image_loss_fwd.restype is C.c_int and len(L.hav_s2_image_loss_fwd.argtypes) == 19
    assert L.hav_s2_image_loss_bwd.restype is C.c_int and len(L.hav_s2_image_loss_bwd.argtypes) == 26
    assert L.hav_s2_image_loss_blocks.restype is C.c_int64
    assert L.hav_s2_image_loss_blocks(2, 128) == 96 and L.hav_s2_image_loss_blocks(3, 192) == 324 and L.hav_s2_image_loss_blocks(1, 4) == 1
    assert L.hav_s2_image_loss_blocks(0, 4) == 0
    assert _lib.ABI_VERSION == L.hav_abi_version()          # additions within the version: nothing existing changed
    assert "hav_s2_loss.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    assert "int hav_s2_image_loss_fwd(float* out5, double* partials, const float* render," in hdr
    assert "int hav_s2_image_loss_bwd(float* gfake, float* grender," in hdr
    # refusals come before any launch: no device is touched
    assert L.hav_s2_image_loss_fwd(*([None] * 3), 0, 0, 0, 0, None, 0, 0, 0, None, None, None, None, 1, 2, 4, None) == -1          # HAV_EINVAL


class _Like:
    """what eligibility reads of a tensor"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_eligibility():
    from havatar_amd.native import train_ops as t

    def args(B=2, Cc=67, r=32, G=128):
        return [_Like(B, Cc, r, r), _Like(B, 1, r, r), _Like(B, 3, G, G), _Like(B, 3, G, G), _Like(B, 3, G, G), _Like(B, 1, r, r)]

    assert t.stage2_image_loss_eligible(*args()) and t.stage2_image_loss_eligible(*args(1, 3, 2, 4)) and t.stage2_image_loss_eligible(*args(1, 3, 8, 8))
    assert not t.stage2_image_loss_eligible(*args(r=1)) and not t.stage2_image_loss_eligible(*args(r=8, G=4))          # r = 1, r > G
    assert not t.stage2_image_loss_eligible(*args(Cc=2))
    for k in range(6):          # dtype and device of every operand
        for attr, val in (("dtype", torch.float64), ("dtype", torch.bfloat16), ("is_cuda", False)):
            a = args()
            setattr(a[k], attr, val)
            assert not t.stage2_image_loss_eligible(*a), (k, attr)
    a = args()
    a[3] = _Like(2, 3, 64, 64)
    assert not t.stage2_image_loss_eligible(*a)
    with torch.no_grad():
        assert not t.stage2_image_loss_eligible(*args())


def test_cpu_tensors_keep_the_statement_or_are_refused(monkeypatch):
    from havatar_amd.native import train_ops as t
    g = torch.Generator().manual_seed(0)
    B, r, G = 1, 4, 8
    render = torch.rand(B, r, r, 5, generator=g).permute(0, 3, 1, 2).requires_grad_(True)
    mask = torch.rand(B, 1, r, r, generator=g)
    imgs = [torch.rand(B, 3, G, G, generator=g) for _ in range(3)]
    gm = torch.rand(B, 1, r, r, generator=g)
    monkeypatch.setenv("HAVATAR_S2_LOSS", "1")
    assert t.s2_loss_enabled() and not t.stage2_image_loss_eligible(render, mask, imgs[0], imgs[1], imgs[2], gm)
    out = t.stage2_image_loss(render, mask, imgs[0], imgs[1], imgs[2], gm, "l1")          # the switch changes nothing on CPU tensors
    ref = t.stage2_image_loss_statement(render, mask, imgs[0], imgs[1], imgs[2], gm, "l1")
    assert all(torch.equal(a, b) for a, b in zip(out, ref)) and not out[3].requires_grad and not out[4].requires_grad
    lr = torch.nn.functional.interpolate(render[:, :3], size=(G, G), mode="bilinear", align_corners=True)
    assert torch.equal(out[0], torch.nn.functional.l1_loss(lr, imgs[0])) and torch.equal(out[3], torch.nn.functional.mse_loss(lr, imgs[0]).detach())
    with pytest.raises(RuntimeError, match="HIP float32"):
        t.stage2_image_loss(render, mask, imgs[0], imgs[1], imgs[2], gm, "l1", native=True)
    with pytest.raises(RuntimeError, match="HIP float32"):
        t.Stage2ImageLoss.apply(render[:, :3], mask, imgs[0], imgs[1], imgs[2], gm, True)
    monkeypatch.delenv("HAVATAR_S2_LOSS")
    assert t.s2_loss_enabled()          # the default
    monkeypatch.setenv("HAVATAR_S2_LOSS", "0")
    assert not t.s2_loss_enabled()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_registers_and_no_scratch(tmp_path):
    """what the compiler makes of csrc/hav_s2_loss.hip for gfx950: five kernels (forward and backward in a 16-byte and a 4-byte variant, the
    one-workgroup reduction), none with scratch or a spill, all under 64 vector registers (eight waves per SIMD stay possible)"""
    dst = str(tmp_path / "hav_s2_loss.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_s2_loss.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    kernels = re.findall(r"\.name:\s+(\S*s2_loss_\w+_kernel\S*)", text)
    assert len(set(kernels)) == 5 and sum("fwd" in k for k in set(kernels)) == 2 and sum("bwd" in k for k in set(kernels)) == 2, kernels
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == 5 and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == 10 and all(v == 0 for v in spills), spills
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    assert len(vgprs) == 5 and max(vgprs) <= 64, vgprs

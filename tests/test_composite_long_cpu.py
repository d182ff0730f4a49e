"""CPU: the compositing pair for 65-128 samples per ray (csrc/hav_composite_long.hip) as far as it can be checked without a GPU -- the
library exports and binds the entries, the autograd node refuses what it cannot take, HAVATAR_COMPOSITE_LONG changes nothing on CPU
tensors, and the compiler's output for gfx950 holds no FLAT access and no scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from havatar_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ENTRIES = {"hav_composite_long_fwd": 14, "hav_composite_long_bwd": 15, "hav_composite_long_bwd_form": 16}


def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib
    L = _lib.lib()
    for name, nargs in ENTRIES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.restype is C.c_int, name
        assert fn.argtypes[-1] is C.c_void_p and C.c_int64 in fn.argtypes, name
    assert _lib.ABI_VERSION == L.hav_abi_version()          # additions within the version: nothing existing changed


def test_a_stale_library_is_named_not_an_attribute_error(monkeypatch):
    """a library built before the entries existed has the same ABI version: the binding says which symbol is missing"""
    from havatar_amd import _lib

    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name.startswith("hav_composite_long"):
                raise AttributeError(name)
            return getattr(self._real, name)

    real_cdll = C.CDLL
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Stale(real_cdll(path)))
    with pytest.raises(_lib.HavatarLibraryError, match="hav_composite_long_fwd"):
        _lib.lib()
    assert _lib._lib is None


def test_composite_long_refuses_cpu_tensors():
    from havatar_amd.native.train_ops import composite_long, composite_long_eligible
    rf, z, rd = torch.zeros(2, 80, 4), torch.zeros(2, 80), torch.ones(2, 3)
    with pytest.raises(RuntimeError, match="HIP float32"):
        composite_long(rf, z, rd)
    assert not composite_long_eligible(80, rf)
    assert not composite_long_eligible(129, rf)

    class Like:          # what eligibility reads of a tensor: a HIP float32 one still fails on the sample count alone
        is_cuda, dtype = True, torch.float32
    assert composite_long_eligible(128, Like()) and composite_long_eligible(1, Like())
    assert not composite_long_eligible(129, Like()) and not composite_long_eligible(0, Like())
    Like.dtype = torch.float16
    assert not composite_long_eligible(80, Like())


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("dataset_long")
    return str(root), synth.write_dataset(str(root), n_frames=2, img_res=128)


def _cpu_step(dataset, num_coarse, num_fine):
    from havatar_amd.dataloader.dataloader import Loader
    from havatar_amd.harness import train
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    cfgd = synth.harness_config(perturb=True, noise_std=0.1, rays=64)
    cfgd["nerf"]["train"].update(num_coarse=num_coarse, num_fine=num_fine)
    cfg = CfgNode(cfgd)
    np.random.seed(7)
    tl = Loader(split_file=dataset[1], mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg,
                white_bg=True, shuffle=False)
    idx, batch = next(iter(tl))
    torch.manual_seed(5)
    trainer = synth.fill_state_dict(Trainer(cfg, len(tl.dataset))).train()
    inp, target, ray_mask = train.step_inputs(idx, batch, "cpu")
    torch.manual_seed(123)
    loss, parts, _ = train.training_loss(trainer, cfg, inp, target, ray_mask, torch.nn.functional.mse_loss)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in trainer.named_parameters() if p.grad is not None}


def test_switch_changes_nothing_on_cpu_tensors(dataset, monkeypatch, recwarn):
    """a CPU Trainer step at 40+48 samples (fine pass 68) with HAVATAR_COMPOSITE_LONG=1 and without: the same bits, and no warning
    either way (the warning is about leaving the native route, which CPU tensors never took)"""
    from havatar_amd.model import nerf_trainer
    monkeypatch.setattr(nerf_trainer, "_warned_wide_sampling", False)
    monkeypatch.delenv("HAVATAR_COMPOSITE_LONG", raising=False)
    l0, g0 = _cpu_step(dataset, 40, 48)
    monkeypatch.setenv("HAVATAR_COMPOSITE_LONG", "1")
    l1, g1 = _cpu_step(dataset, 40, 48)
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 100
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert not [w for w in recwarn.list if "HAVATAR_COMPOSITE_LONG" in str(w.message)]
    assert nerf_trainer._warned_wide_sampling is False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_flat_access_and_no_scratch(tmp_path):
    dst = str(tmp_path / "hav_composite_long.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_composite_long.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    bad = [l.strip() for l in text.splitlines() if re.match(r"\s+flat_(load|store|atomic)", l)]
    assert not bad, "%d FLAT instructions, e.g. %s" % (len(bad), bad[:3])
    kernels = re.findall(r"\.name:\s+(\S*composite_long_kernel\S*)", text)
    assert len(set(kernels)) == 4, kernels          # forward, direct backward, staged backward with one and with two waves
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == len(kernels) and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == len(kernels) and all(v == 0 for v in spills), spills

"""CPU: the stage-two kernel file (csrc/hav_stage2.hip) and the wavelet autograd nodes as far as they can be checked without a GPU -- the
library exports and binds hav_haar_down2 within ABI 8, the wrappers refuse CPU tensors, ineligible shapes come back as None, the switch
changes nothing on CPU tensors, and the compiler's output for gfx950 holds no FLAT access, no spill and no scratch."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_library_exports_and_binds_the_entry():
    from havatar_amd import _lib, build
    L = _lib.lib()
    fn = L.hav_haar_down2
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[5] is C.c_float and fn.argtypes[-1] is C.c_void_p
    assert _lib.ABI_VERSION == L.hav_abi_version() == 8          # an addition within the version: nothing existing changed
    assert "hav_stage2.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    assert re.search(r"int hav_haar_down2\(float\* out, const float\* in, const float\* ki4x2x2, const float\* fir4x4, const float\* kd4x2x2, float scale,",
                     hdr)


def test_wrappers_refuse_cpu_tensors():
    from havatar_amd.native import train_ops as t
    x, k4, fir = torch.zeros(1, 12, 8, 8), torch.zeros(4, 2, 2), torch.zeros(4, 4)
    for call in (lambda: t.haar_dwt(x, k4), lambda: t.haar_idwt(x, k4), lambda: t.haar_up2(x, k4, fir, k4),
                 lambda: t.haar_down2(x, k4, fir, k4), lambda: t.haar_down2_raw(x, k4, fir, k4),
                 lambda: t.HaarDwt.apply(x, k4), lambda: t.HaarIdwt.apply(x, k4), lambda: t.HaarUp2.apply(x, k4, fir, k4),
                 lambda: t.HaarDown2.apply(x, k4, fir, k4, 1.0)):
        with pytest.raises(RuntimeError, match="HIP float32"):
            call()
    assert not (t.haar_dwt_eligible(x) or t.haar_idwt_eligible(x) or t.haar_up2_eligible(x, fir) or t.haar_down2_eligible(x, fir))


class _Like:
    """what eligibility reads of a tensor"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape, ptr=256, contiguous=True):
        self.shape, self._ptr, self._c = shape, ptr, contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return self._ptr


def test_eligibility_and_none_for_ineligible_shapes():
    from havatar_amd.native import train_ops as t
    fir, fir3 = _Like(4, 4), _Like(3, 3)
    # dwt: H even, W % 8 == 0
    assert t.haar_dwt_eligible(_Like(1, 1, 2, 8)) and t.haar_dwt_eligible(_Like(2, 3, 34, 72))
    assert not t.haar_dwt_eligible(_Like(1, 1, 3, 8)) and not t.haar_dwt_eligible(_Like(1, 1, 2, 12)) and not t.haar_dwt_eligible(_Like(1, 2, 8))
    # idwt: four bands, W % 4 == 0
    assert t.haar_idwt_eligible(_Like(1, 4, 1, 4)) and t.haar_idwt_eligible(_Like(2, 12, 17, 36))
    assert not t.haar_idwt_eligible(_Like(1, 6, 4, 4)) and not t.haar_idwt_eligible(_Like(1, 4, 4, 6))
    # up2: four bands, W even, 4x4 FIR
    assert t.haar_up2_eligible(_Like(1, 4, 1, 2), fir) and t.haar_up2_eligible(_Like(2, 12, 17, 18), fir)
    assert not t.haar_up2_eligible(_Like(1, 4, 4, 5), fir) and not t.haar_up2_eligible(_Like(1, 4, 4, 4), fir3)
    # down2: four bands, H even, W % 4 == 0 (the kernel takes W even; the adjoint hav_haar_up2 wants W / 2 even), 4x4 FIR
    assert t.haar_down2_eligible(_Like(1, 4, 2, 4), fir) and t.haar_down2_eligible(_Like(2, 12, 34, 72), fir)
    assert not t.haar_down2_eligible(_Like(1, 4, 3, 4), fir) and not t.haar_down2_eligible(_Like(1, 4, 2, 6), fir)
    assert not t.haar_down2_eligible(_Like(1, 4, 2, 4), fir3) and not t.haar_down2_eligible(_Like(1, 5, 2, 4), fir)
    # a contiguous tensor off the 16-byte grid, another dtype
    assert not t.haar_dwt_eligible(_Like(1, 1, 2, 8, ptr=260)) and t.haar_dwt_eligible(_Like(1, 1, 2, 8, ptr=260, contiguous=False))
    half = _Like(1, 4, 2, 4)
    half.dtype = torch.float16
    assert not t.haar_down2_eligible(half, fir)
    # the wrappers hand None back for what is not eligible (the caller keeps its statement)
    k4 = _Like(4, 2, 2)
    assert t.haar_dwt(_Like(1, 1, 3, 8), k4) is None and t.haar_idwt(_Like(1, 4, 4, 6), k4) is None
    assert t.haar_up2(_Like(1, 4, 4, 5), k4, fir, k4) is None and t.haar_down2(_Like(1, 4, 3, 4), k4, fir, k4) is None


def test_switch_reads_the_environment_at_the_call(monkeypatch):
    from havatar_amd.native import train_ops as t
    monkeypatch.delenv("HAVATAR_HAAR_TRAIN", raising=False)
    assert not t.haar_enabled()
    monkeypatch.setenv("HAVATAR_HAAR_TRAIN", "1")
    assert t.haar_enabled()
    monkeypatch.setenv("HAVATAR_HAAR_TRAIN", "0")
    assert not t.haar_enabled()


def test_switch_changes_nothing_on_cpu_tensors(monkeypatch):
    from havatar_amd import synth
    from havatar_amd.model.styleUnet import Discriminator
    d = synth.fill_state_dict(Discriminator(32, 3))
    x = torch.from_numpy(synth.normal((2, 3, 32, 32), 5, 0.5))
    res = []
    for v in (None, "1"):
        monkeypatch.delenv("HAVATAR_HAAR_TRAIN", raising=False)
        if v:
            monkeypatch.setenv("HAVATAR_HAAR_TRAIN", v)
        xi = x.clone().requires_grad_(True)
        d.zero_grad()
        y = d(xi)
        y.sum().backward()
        res.append((y.detach(), xi.grad, d.final_linear[1].weight.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_flat_access_no_spill_and_no_scratch(tmp_path):
    dst = str(tmp_path / "hav_stage2.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_stage2.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    bad = [l.strip() for l in text.splitlines() if re.match(r"\s+flat_(load|store|atomic)", l)]
    assert not bad, "%d FLAT instructions, e.g. %s" % (len(bad), bad[:3])
    kernels = re.findall(r"\.name:\s+(\S*haar_down2_kernel\S*)", text)
    assert len(set(kernels)) == 2, kernels          # 16-byte and 4-byte accesses
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == len(kernels) and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == 2 * len(kernels) and all(v == 0 for v in spills), spills
    assert len(re.findall(r"\s+global_load_dwordx4", text)) >= 32 and len(re.findall(r"\s+global_store_dwordx4", text)) >= 4

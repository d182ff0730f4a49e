"""CPU: the library exports the decoder's InstanceNorm3d + ReLU and output-layer entries (csrc/hav_decoder.hip, ABI 8), and the
eligibility functions of their autograd nodes refuse CPU tensors (no compute without a GPU)."""
import ctypes

import torch

NEW = ["hav_inorm_relu_chunks", "hav_inorm_relu_scratch_bytes", "hav_inorm_relu_fwd", "hav_inorm_relu_bwd",
       "hav_final_conv_sigmoid_fwd", "hav_final_conv_sigmoid_bwd_scratch_bytes", "hav_final_conv_sigmoid_bwd"]


def test_library_exports_the_decoder_entries():
    from havatar_amd import _lib, build
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), n
    L = _lib.lib()
    assert L.hav_abi_version() == _lib.ABI_VERSION == 8
    for n in NEW:
        assert getattr(L, n).argtypes, n          # bound with its argument types


def test_size_queries_refuse_without_a_device():
    """The refusals of the size queries are decided on the host: V < 2, Cout != 1, Cin over the bound."""
    from havatar_amd import _lib
    L = _lib.lib()
    assert L.hav_inorm_relu_chunks(4, 1) == 0 and L.hav_inorm_relu_scratch_bytes(4, 1) == 0
    assert L.hav_inorm_relu_chunks(512, 8) == 1 and L.hav_inorm_relu_scratch_bytes(512, 8) == 0
    assert L.hav_final_conv_sigmoid_bwd_scratch_bytes(1, 16, 2, 4, 4, 4) == 0
    assert L.hav_final_conv_sigmoid_bwd_scratch_bytes(1, 65, 1, 4, 4, 4) == 0
    assert L.hav_final_conv_sigmoid_bwd_scratch_bytes(1, 16, 1, 4, 4, 4) > 0


def test_eligibility_functions_refuse_cpu_tensors():
    from havatar_amd.native import train_ops
    y = torch.randn(1, 4, 3, 5, 6)
    assert not train_ops.inorm_relu3d_eligible(y, torch.nn.InstanceNorm3d(4))
    assert not train_ops.final_conv_sigmoid_eligible(y, torch.nn.Conv3d(4, 1, 3, padding=1))


def test_switch_leaves_the_cpu_decoder_alone(monkeypatch):
    """HAVATAR_DECODER=hip on CPU tensors: the decoder keeps its ATen statements, the same bits as with the switch unset."""
    from havatar_amd.model.network.voxel_encoder import VolumeDecoder
    torch.manual_seed(3)
    dec = VolumeDecoder(num_in=64, final_res=4)
    monkeypatch.delenv("HAVATAR_DECODER", raising=False)
    a = dec()
    monkeypatch.setenv("HAVATAR_DECODER", "hip")
    b = dec()
    assert a.shape == (1, 2, 4, 4, 4) and torch.equal(a, b)

"""Shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: the float64 restatement of SSIM / mse that is the tests' truth (numpy, the
window as an outer product, explicit sums over valid windows -- written from the definition, not from havatar_amd/metrics.py), the image kinds
of the cancellation probe, and the checkpoint recipe of the reenactment command line."""
import functools

import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view

WIN = 11


def window2d():
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k * k) / (2.0 * 1.5 ** 2))
    g /= g.sum()
    return np.outer(g, g)


def ssim64(a, b, L=1.0):
    """a, b [B,C,H,W] -> (mean SSIM [B], map [B,C,H-10,W-10]), float64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = window2d()

    def blur(t):
        return np.einsum("bcijkl,kl->bcij", sliding_window_view(t, (WIN, WIN), axis=(2, 3)), w)

    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mx, my = blur(a), blur(b)
    sxx, syy, sxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return m.mean((1, 2, 3)), m


def mse64(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d * d).mean((1, 2, 3))


def u8_truth(a, b):
    """a, b uint8 [B,H,W,3] -> (ssim [B] on x / 255 with L = 1, mse [B] = the exact integer sum / (255^2 N)), float64"""
    x, y = (np.asarray(t).astype(np.float64).transpose(0, 3, 1, 2) for t in (a, b))
    d = x - y
    return ssim64(x / 255.0, y / 255.0)[0], (d * d).sum((1, 2, 3)) / (255.0 * 255.0 * x[0].size)


KINDS = ("texture", "quant8", "flat", "mixed")


@functools.lru_cache(maxsize=None)
def pair(kind, shape):
    """float32 [B,C,H,W] pair in [0, 1] (seeds 11 and 12):
    texture  a smooth pattern plus noise, and the same plus a little more noise
    quant8   that pair rounded to multiples of 1 / 255
    flat     1.0 everywhere against 0.999 in the lower half
    mixed    the texture pair with the left half white in both and one 4 x 4 patch of the second at 254 / 255"""
    B, C, H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = 0.5 + 0.3 * torch.sin(xx / 7.0 + 0.5) * torch.cos(yy / 5.0)
    a = (smooth + 0.1 * torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(11))).clamp(0, 1)
    b = (a + 0.05 * torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(12))).clamp(0, 1)
    if kind == "quant8":
        a, b = torch.round(a * 255) / 255, torch.round(b * 255) / 255
    elif kind == "flat":
        a, b = torch.ones(shape), torch.ones(shape)
        b[:, :, H // 2:, :] = 0.999
    elif kind == "mixed":
        a[..., : W // 2], b[..., : W // 2] = 1.0, 1.0
        b[:, :, H // 4: H // 4 + 4, W // 8: W // 8 + 4] = 254.0 / 255.0
    elif kind != "texture":
        raise ValueError(kind)
    return a.contiguous(), b.contiguous()


@functools.lru_cache(maxsize=None)
def pair_u8(kind, shape):
    """the uint8 [B,H,W,3] twin (shape is still (B, 3, H, W)); flat: 255 against 254 in the lower half"""
    a, b = pair(kind, shape)
    if kind == "flat":
        a, b = torch.full(shape, 255.0), torch.full(shape, 255.0)
        b[:, :, shape[2] // 2:, :] = 254.0
    else:
        a, b = torch.round(a * 255), torch.round(b * 255)
    return a.to(torch.uint8).permute(0, 2, 3, 1).contiguous(), b.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def truth(kind, shape):
    """(mean [B], map) of pair(kind, shape) in float64"""
    a, b = pair(kind, shape)
    return ssim64(a.numpy(), b.numpy())


@functools.lru_cache(maxsize=None)
def aten32_errors(kind, shape):
    """(error of the mean, error of the map) of the ATen float32 statement on the CPU against truth(): the yardstick"""
    from havatar_amd import metrics
    a, b = pair(kind, shape)
    s, _, m = metrics.aten_statement(a, b, 1.0, True)
    ref, ref_map = truth(kind, shape)
    return float(np.abs(s.double().numpy() - ref).max()), float(np.abs(m.double().numpy() - ref_map).max())


def checkpoint(path):
    """the reenactment checkpoint of the harness tests: weights are a function of the state_dict key (havatar_amd.synth)"""
    from havatar_amd import synth
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.model.styleUnet import SWGAN_unet
    from havatar_amd.utils.cfgnode import CfgNode
    cfg = CfgNode(synth.harness_config())
    state = torch.get_rng_state()
    tw = synth.fill_state_dict(Trainer(cfg, 3))
    sw = synth.fill_state_dict(SWGAN_unet(inp_size=32, inp_ch=64, out_size=128, out_ch=3, style_dim=64, c_dim=0, n_mlp=4, channel_multiplier=2), seed=1)
    torch.set_rng_state(state)
    torch.save({"nerf_render": synth.zero_noise_weights({k: v.clone() for k, v in tw.state_dict().items()}),
                "latent_codes": tw.state_dict()["latent_codes"].clone(),
                "g_ema": synth.zero_noise_weights({k: v.clone() for k, v in sw.state_dict().items()})}, path)
    return str(path)


def split_ground_truth(split_file):
    """{(fidx, view): uint8 [H,W,3]}: the photographs of a split, white where the mask is off, read here from the files the split names"""
    import json
    from havatar_amd.dataloader import imgio
    with open(split_file) as f:
        meta = json.load(f)
    out = {}
    for fd in meta["frames"]:
        for view in fd["mutiview_info_ls"]:
            img = np.array(imgio.imread_rgb(view["file_path"]))
            img[np.asarray(imgio.imread_rgb(view["mask_path"]))[:, :, 0] <= 127] = 255
            out[(int(fd["fidx"]), int(view["view_name"]))] = img
    return out


def check_table(table, savedir, gts, ssim_tol, mse_tol_ulp32=None):
    """every number of a metrics.json against the restatement computed from the PNGs the run wrote and the split's photographs"""
    import math
    import os
    from havatar_amd.dataloader import imgio
    assert [(f["fidx"], f["view"]) for f in table["frames"]] == sorted((f["fidx"], f["view"]) for f in table["frames"])
    assert table["n"] == len(table["frames"]) and table["n_identical"] == sum(f["psnr"] is None for f in table["frames"])
    for f in table["frames"]:
        png = np.asarray(imgio.imread_rgb(os.path.join(savedir, f["file"])))
        s, mse = u8_truth(png[None], gts[(f["fidx"], f["view"])][None])
        print(f["file"], "ssim", f["ssim"], "truth", s[0], "mse", f["mse"], "truth", mse[0])
        assert abs(f["ssim"] - s[0]) <= ssim_tol, (f["ssim"], s[0])
        if mse_tol_ulp32 is None:
            assert f["mse"] == mse[0], (f["mse"], mse[0])
        else:
            assert abs(f["mse"] - mse[0]) <= mse_tol_ulp32 * float(np.spacing(np.float32(mse[0]))), (f["mse"], mse[0])
        assert f["psnr"] is None if f["mse"] == 0 else f["psnr"] == -10.0 * math.log10(f["mse"])
    rows = table["frames"]
    assert table["mean"]["ssim"] == sum(r["ssim"] for r in rows) / len(rows)
    ps = [r["psnr"] for r in rows if r["psnr"] is not None]
    assert table["mean"]["psnr"] == (sum(ps) / len(ps) if ps else None)

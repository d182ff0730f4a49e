"""Image-quality metrics: SSIM, PSNR and their per-sequence table (`avatarHD_reenactment.py --metrics`).

Definition (DEFINITION below): SSIM of Wang et al. 2004 per channel with an 11-tap Gaussian window, sigma 1.5, normalised to sum 1 and
applied separably on VALID windows only (the map is [H-10, W-10]), C1 = (0.01 L)^2, C2 = (0.03 L)^2, the value the mean over map and channels
per sample -- what skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False) and pytorch-msssim
give.  PSNR = 10 log10(L^2 / mse) over all elements, inf at mse 0.

Pairs are float [B,C,H,W] or uint8 [B,H,W,3] (channels-last, what a PNG is; scored as x / 255 with L = 1).  Routing: float32 and uint8 HIP
tensors take csrc/hav_metrics.hip (native/metrics_ops.py); everything else -- CPU tensors, other dtypes, tensors that need a gradient,
HAVATAR_METRICS=0 -- takes the ATen statement of the same definition (depthwise conv2d, two passes), in float64 for uint8 and CPU pairs and in
the input dtype for floating HIP tensors.  These functions carry no autograd on the native route; the training loss is ssim_loss(): for a
float32 HIP pair whose first image needs a gradient it takes the node of native/ssim_ops.py (csrc/hav_ssim_loss.hip: the same forward bits,
float64 gradient kernels), otherwise the statement under autograd."""
import json
import math

import torch
import torch.nn.functional as F

from .native import metrics_ops, ssim_ops

WIN, SIGMA, K1, K2 = metrics_ops.WIN, 1.5, 0.01, 0.03
DEFINITION = {"ssim": "Wang et al. 2004, per channel, mean over map and channels", "window": "gaussian, %d taps, separable, normalised to sum 1" % WIN,
              "sigma": SIGMA, "windows": "valid only: the map is [H-%d, W-%d]" % (WIN - 1, WIN - 1), "K1": K1, "K2": K2,
              "constants": "C1 = (K1 L)^2, C2 = (K2 L)^2, L = 1 on uint8 / 255", "psnr": "10 log10(1 / mse), mse over all elements of uint8 / 255",
              "on": "uint8 as written"}


def gaussian_window(dtype=torch.float64):
    """[11] = exp(-k^2 / (2 sigma^2)), k = -5..5, normalised to sum 1 (formed in float64, then cast)"""
    k = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype)


def _check_pair(a, b):
    """-> 'u8' | 'float'; raises on what the definition does not cover"""
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        raise TypeError("metrics: tensors expected")
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError("metrics: a pair of equal 4-d shapes is needed, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.dtype != b.dtype:
        raise ValueError("metrics: the pair differs in dtype: %s %s and %s %s" % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    if a.dtype == torch.uint8:
        if a.shape[3] != 3:
            raise ValueError("metrics: uint8 pairs are channels-last [B,H,W,3], got %s" % (tuple(a.shape),))
        kind, (H, W) = "u8", a.shape[1:3]
    elif a.dtype.is_floating_point:
        kind, (H, W) = "float", a.shape[2:4]
    else:
        raise ValueError("metrics: float [B,C,H,W] or uint8 [B,H,W,3] pairs, got %s %s" % (a.dtype, tuple(a.shape)))
    if H < WIN or W < WIN:
        raise ValueError("metrics: the %d-tap window needs H, W >= %d, got shape %s" % (WIN, WIN, tuple(a.shape)))
    return kind


def aten_statement(a, b, data_range=1.0, return_map=False):
    """The definition on ATen, in the dtype of the float [B,C,H,W] pair: (ssim [B], mse [B], map [B,C,H-10,W-10] or None)."""
    C = a.shape[1]
    g = gaussian_window(a.dtype).to(a.device)
    wh, wv = g.view(1, 1, 1, WIN).repeat(C, 1, 1, 1), g.view(1, 1, WIN, 1).repeat(C, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, wh, groups=C), wv, groups=C)

    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu1, mu2 = blur(a), blur(b)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = blur(a * a) - mu11, blur(b * b) - mu22, blur(a * b) - mu12
    smap = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu11 + mu22 + C1) * (s11 + s22 + C2))
    d = a - b
    return smap.mean((1, 2, 3)), (d * d).mean((1, 2, 3)), (smap if return_map else None)


def _both(a, b, data_range, return_map):
    """(ssim [B], mse [B] in (data_range units)^2 -- [0,1]^2 for uint8 --, map or None) by the route the pair is eligible for"""
    kind = _check_pair(a, b)
    if metrics_ops.enabled() and metrics_ops.eligible(a, b):
        if kind == "u8":
            out, smap = metrics_ops.image_metrics_u8(a, b, return_map)
        else:
            out, smap = metrics_ops.image_metrics_f32(a, b, data_range, return_map)
        return out[:, 0], out[:, 1], smap
    if kind == "u8":
        # integers in float64: the squared-error sum is exact
        x, y = a.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
        s, _, smap = aten_statement(x, y, 255.0, return_map)
        d = x - y
        return s, (d * d).sum((1, 2, 3)) / (255.0 * 255.0 * x[0].numel()), smap
    if not a.is_cuda:
        return aten_statement(a.double(), b.double(), data_range, return_map)
    return aten_statement(a, b, data_range, return_map)


def ssim_mse(a, b, data_range=1.0):
    """[B,2] = (mean SSIM, mse) from one pass: what the reenactment loop appends per frame"""
    s, mse, _ = _both(a, b, data_range, False)
    return torch.stack([s, mse], 1)


def ssim(a, b, data_range=1.0, return_map=False):
    """[B] mean SSIM per sample; return_map: (that, the map [B,C,H-10,W-10])"""
    s, _, smap = _both(a, b, data_range, return_map)
    return (s, smap) if return_map else s


def ssim_loss(pred, target, data_range=1.0):
    """The scalar 1 - mean_b ssim_b of a float [B,C,H,W] pair, in the pair's dtype, differentiable in pred (and, on the statement route, in
    target).  Routing: nothing needs a gradient -> ssim(); a float32 HIP pair on one device whose target is a constant, HAVATAR_METRICS on ->
    the node of native/ssim_ops.py (forward bits of ssim(), float64 gradient kernels); everything else -> the ATen statement under autograd,
    in float64 for CPU pairs and in the pair's dtype for HIP ones."""
    if _check_pair(pred, target) == "u8":
        raise ValueError("metrics: ssim_loss takes float [B,C,H,W] pairs (uint8 carries no gradient), got %s %s" % (pred.dtype, tuple(pred.shape)))
    if not (torch.is_grad_enabled() and (pred.requires_grad or target.requires_grad)):
        return (1.0 - ssim(pred, target, data_range).mean()).to(pred.dtype)
    if (metrics_ops.enabled() and pred.is_cuda and target.is_cuda and pred.device == target.device and pred.dtype == torch.float32
            and not target.requires_grad):
        return 1.0 - ssim_ops.ssim_mean(pred, target, data_range).mean()
    if not pred.is_cuda:
        return (1.0 - aten_statement(pred.double(), target.double(), data_range)[0].mean()).to(pred.dtype)
    return 1.0 - aten_statement(pred, target, data_range)[0].mean()


def _psnr_of(mse, data_range):
    return 10.0 * torch.log10((data_range * data_range) / mse)          # mse == 0 -> inf


def psnr(a, b, data_range=1.0):
    """[B] = 10 log10(L^2 / mse); inf where the pair is identical.  uint8 pairs are scored as x / 255 with L = 1 whatever data_range says."""
    kind = _check_pair(a, b)
    _, mse, _ = _both(a, b, data_range, False)
    return _psnr_of(mse, 1.0 if kind == "u8" else data_range)


def image_metrics(pred, gt, data_range=1.0):
    """{"ssim", "mse", "psnr"}: [B] tensors, from one pass over the pair"""
    kind = _check_pair(pred, gt)
    s, mse, _ = _both(pred, gt, data_range, False)
    return {"ssim": s, "mse": mse, "psnr": _psnr_of(mse, 1.0 if kind == "u8" else data_range)}


# ----------------------------------------------------------------------------------------------------------------------------------------
# the per-sequence table
# ----------------------------------------------------------------------------------------------------------------------------------------
def table(frames, lpips_note=None):
    """The layout of metrics.json from per-frame records {"file", "fidx", "view", "mse", "ssim", "lpips"?}: frames sorted by (fidx, view), a
    frame with mse == 0 has "psnr": null, is counted in n_identical and left out of the PSNR mean; means are means of the per-frame values
    in float64, in frame order."""
    rows = []
    for f in sorted(frames, key=lambda f: (int(f["fidx"]), int(f["view"]))):
        mse = float(f["mse"])
        row = {"file": f["file"], "fidx": int(f["fidx"]), "view": int(f["view"]), "mse": mse,
               "psnr": None if mse == 0 else -10.0 * math.log10(mse), "ssim": float(f["ssim"])}
        if f.get("lpips") is not None:
            row["lpips"] = float(f["lpips"])
        rows.append(row)

    def mean(vals):
        vals = list(vals)
        return sum(vals) / len(vals) if vals else None

    means = {"psnr": mean(r["psnr"] for r in rows if r["psnr"] is not None), "ssim": mean(r["ssim"] for r in rows)}
    if rows and all("lpips" in r for r in rows):
        means["lpips"] = mean(r["lpips"] for r in rows)
    definition = dict(DEFINITION)
    if lpips_note is not None:
        definition["lpips"] = lpips_note
    return {"definition": definition, "frames": rows, "mean": means, "n": len(rows), "n_identical": sum(r["psnr"] is None for r in rows)}


def merge(paths, out=None):
    """The per-rank files of a sharded run (metrics_rank<r>of<w>.json) as the one-rank table; written to `out` when given."""
    frames, note = [], None
    for p in paths:
        with open(p) as f:
            part = json.load(f)
        frames += part["frames"]
        note = note or part["definition"].get("lpips")
    merged = table(frames, lpips_note=note)
    if out is not None:
        with open(out, "w") as f:
            json.dump(merged, f, indent=1)
    return merged

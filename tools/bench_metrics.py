#!/usr/bin/env python3
"""Image metrics (havatar_amd/metrics.py): (a) csrc/hav_metrics.hip against the ATen statement of the same definition (HAVATAR_METRICS=0) on
the device at 128^2, 512^2 and 1024^2, float32 [1,3,H,W] and uint8 [1,H,W,3] pairs, with the kernel's achieved bytes/s against what it must
read; (b) the cancellation table: the error of both float32 routes against the float64 restatement on the flat and mixed kinds at 512^2 and
1024^2 (and on a texture pair for scale).

Method (tools/bench_lpips.py): every timed call works on its OWN input buffers (K distinct pairs), the routes alternate round by round in one
process after two warm-up rounds, median and minimum over the rounds of the time per call, HIP events.  Eager launches: that is what the
reenactment loop pays per frame.
Bytes: the two images once (2 * 4 * C H W, uint8: 2 * C H W); the haloed tiles re-read 42^2 / 32^2 = 1.72 of that from the caches.
(c) --reenact (alone: (a) and (b) are skipped): the reenactment command line in ONE process, on synthetic splits -- first five runs of a two-frame
128^2 split (without --metrics, without, with, with, without) and the pixel differences between every two of them: whether runs are
bit-reproducible at all, with and without the flag; then six runs of a 24-frame 512 -> 1024 split, alternating without / with --metrics: the
harness's own `ms per frame` line is the end-to-end cost of the flag.
The kernel's own time: `rocprofv3 --kernel-trace --stats -- python tools/bench_metrics.py --no-accuracy`, in a run of its own.
Usage: python tools/bench_metrics.py [--out FILE] [--rounds N] [--no-accuracy] | --reenact"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from havatar_amd import metrics

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 9
SIZES = (128, 512, 1024)
K = 8


def texture_pair(S, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    a = (0.5 + 0.3 * torch.sin(xx / 7.0 + 0.5) * torch.cos(yy / 5.0) + 0.1 * torch.randn(1, 3, S, S, generator=g)).clamp(0, 1)
    return a, (a + 0.05 * torch.randn(1, 3, S, S, generator=g)).clamp(0, 1)


def kind_pair(kind, S):
    a, b = texture_pair(S, 11)
    if kind == "flat":
        a, b = torch.ones(1, 3, S, S), torch.ones(1, 3, S, S)
        b[:, :, S // 2:, :] = 0.999
    elif kind == "mixed":
        a[..., : S // 2], b[..., : S // 2] = 1.0, 1.0
        b[:, :, S // 4: S // 4 + 4, S // 8: S // 8 + 4] = 254.0 / 255.0
    return a, b


def timed(fns):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for f in fns:
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / len(fns)


def alternate(fns, warm=2):
    ts = {"native": [], "aten": []}
    for rnd in range(warm + REPS):
        for name, env in (("native", "1"), ("aten", "0")):
            os.environ["HAVATAR_METRICS"] = env
            t = timed(fns)
            if rnd >= warm:
                ts[name].append(t)
    os.environ.pop("HAVATAR_METRICS", None)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


def reenact_runs():
    import tempfile

    import numpy as np
    import yaml

    from havatar_amd import synth
    from havatar_amd.dataloader import imgio
    from havatar_amd.harness import reenact
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.model.styleUnet import SWGAN_unet
    from havatar_amd.utils.cfgnode import CfgNode

    def setup(render, gen, n):
        tmp = tempfile.mkdtemp()
        split = synth.write_dataset(tmp, n_frames=n, img_res=gen)
        cfgd = synth.harness_config(render_size=render, gen_size=gen, img_res=gen)
        with open(os.path.join(tmp, "cfg.yml"), "w") as f:
            yaml.safe_dump(cfgd, f)
        tw = synth.fill_state_dict(Trainer(CfgNode(cfgd), 3))
        sw = synth.fill_state_dict(SWGAN_unet(inp_size=render, inp_ch=64, out_size=gen, out_ch=3, style_dim=64, c_dim=0, n_mlp=4,
                                              channel_multiplier=2), seed=1)
        # noise strengths at 0: the generators' per-call random noise has no effect, so two runs can be compared pixel by pixel
        torch.save({"nerf_render": synth.zero_noise_weights({k: v.clone() for k, v in tw.state_dict().items()}),
                    "latent_codes": tw.state_dict()["latent_codes"].clone(),
                    "g_ema": synth.zero_noise_weights({k: v.clone() for k, v in sw.state_dict().items()})}, os.path.join(tmp, "avatar.pth"))
        return tmp, ["--config", os.path.join(tmp, "cfg.yml"), "--ckpt", os.path.join(tmp, "avatar.pth"), "--split", split]

    tmp, argv = setup(32, 128, 2)
    plan = ([], [], ["--metrics"], ["--metrics"], [])
    print("# runs of the command line in one process (32 -> 128, 2 frames): %s; max |diff| in LSB and pixels differing, per frame"
          % ", ".join("%d %s" % (k, "with --metrics" if e else "without") for k, e in enumerate(plan)), flush=True)
    runs = []
    for k, extra in enumerate(plan):
        written = reenact.main(argv + ["--savedir", os.path.join(tmp, "out%d" % k)] + extra)
        runs.append([imgio.imread_rgb(p).astype(np.int32) for p in written])
    for i in range(len(runs)):
        for j in range(i + 1, len(runs)):
            d = [np.abs(x - y) for x, y in zip(runs[i], runs[j])]
            print("runs %d %d: max diff %s, pixels differing %s" % (i, j, [int(x.max()) for x in d], [int((x > 0).sum()) for x in d]), flush=True)
    tmp, argv = setup(512, 1024, 24)
    print("# 512 -> 1024, 24 frames, one process, runs alternating: the harness's own line", flush=True)
    for k, extra in enumerate(([], ["--metrics"]) * 3):
        print("=== run %d %s" % (k, "with --metrics" if extra else "without"), flush=True)
        reenact.main(argv + ["--savedir", os.path.join(tmp, "out%d" % k)] + extra)


if "--reenact" in sys.argv:
    reenact_runs()
    sys.exit(0)

rows = []
for S in SIZES:
    for form in ("float32", "uint8"):
        pairs = []
        for k in range(K):
            a, b = texture_pair(S, 100 + k)
            if form == "uint8":
                a, b = ((t * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() for t in (a, b))
            pairs.append((a.to(dev), b.to(dev)))
        with torch.no_grad():
            res = alternate([lambda a=a, b=b: metrics.ssim_mse(a, b) for a, b in pairs])
        nbytes = 2 * 3 * S * S * (4 if form == "float32" else 1)
        rows.append({"size": S, "form": form, "native_us": round(res["native"][0] * 1e3, 1), "native_us_min": round(res["native"][1] * 1e3, 1),
                     "aten_us": round(res["aten"][0] * 1e3, 1), "aten_us_min": round(res["aten"][1] * 1e3, 1), "MB_read_once": round(nbytes / 1e6, 2),
                     "native_GBps_of_read_once": round(nbytes / (res["native"][0] * 1e-3) / 1e9, 1)})
        r = rows[-1]
        print("%4d^2 %-7s native %9.1f (%9.1f) us | HAVATAR_METRICS=0 %9.1f (%9.1f) us | x%.1f | %.2f MB once -> %.1f GB/s (call, two launches)" % (
            S, form, r["native_us"], r["native_us_min"], r["aten_us"], r["aten_us_min"], r["aten_us"] / r["native_us"], r["MB_read_once"],
            r["native_GBps_of_read_once"]), flush=True)
        del pairs
        torch.cuda.empty_cache()

acc = []
if "--no-accuracy" not in sys.argv:
    print("# error against the float64 statement (CPU): mean SSIM / SSIM map; ATen float32 on the device against the native route", flush=True)
    for S in (512, 1024):
        for kind in ("texture", "flat", "mixed"):
            a, b = kind_pair(kind, S)
            ref, _, ref_map = metrics.aten_statement(a.double(), b.double(), 1.0, True)
            with torch.no_grad():
                s0, _, m0 = metrics.aten_statement(a.to(dev), b.to(dev), 1.0, True)
                s1, m1 = metrics.ssim(a.to(dev), b.to(dev), return_map=True)
            e = [float((s0.double().cpu() - ref).abs().max()), float((m0.double().cpu() - ref_map).abs().max()),
                 float((s1.double().cpu() - ref).abs().max()), float((m1.double().cpu() - ref_map).abs().max())]
            acc.append({"size": S, "kind": kind, "aten32_mean": e[0], "aten32_map": e[1], "native_mean": e[2], "native_map": e[3]})
            print("%4d^2 %-7s ATen float32 mean %.2e map %.2e | native mean %.2e map %.2e" % (S, kind, *e), flush=True)

line = json.dumps({"ab": rows, "accuracy": acc})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""LPIPS-VGG (model/lpips.py): (a) the module on its native nodes (HAVATAR_LPIPS=1) against the same module on the ATen statement
(HAVATAR_LPIPS=0), forward and forward + backward into in0, at (2, 3, 64, 64) -- the stage-one patch --, (2, 3, 512, 512) and
(2, 3, 1024, 1024); (b) the head alone per tap of a 2 x 3 x 512 x 512 pair (hav_lpips_head_fwd / _bwd into f0) against a plain copy of the
same bytes (both maps, copy_); (c) the eager joint iteration of tools/bench_train_hd.py (128 -> 512, B = 2, i = 1) with the native module
against no perceptual term.  Synthetic weights (He-normal; the arithmetic does not depend on them).

Method (tools/bench_train_hd.py): every timed call works on its OWN input buffers (K distinct sets), the routes alternate round by round in
one process after two warm-up rounds (MIOpen's search, the packs), median and minimum over the rounds of the time per call.  Eager
launches: no step that holds LPIPS is captured, so this is what a training iteration pays.
(c)'s first iteration spends minutes in MIOpen's solver search (torch.backends.cudnn.benchmark = True, as tools/bench_train_hd.py): --step-only
runs it alone.
Usage: python tools/bench_lpips.py [--out FILE] [--rounds N] [--no-step | --step-only]"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from havatar_amd.model import lpips
from havatar_amd.native import lpips_ops

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 9
SIZES = [(2, 3, 64, 64), (2, 3, 512, 512), (2, 3, 1024, 1024)]


def he_module():
    m = lpips.LPIPS(net="vgg", allow_random=True)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif name.startswith("lin"):
                p.copy_(torch.rand(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (9 * p.shape[1])) ** 0.5)
    return m.to(dev)


def timed(fns):
    """ms per call of the K callables, one after the other"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for f in fns:
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / len(fns)


def alternate(routes, warm=2):
    """routes: name -> (list of K callables, env value or None)"""
    ts = {k: [] for k in routes}
    for rnd in range(warm + REPS):
        for name, (fns, env) in routes.items():
            os.environ.pop("HAVATAR_LPIPS", None)
            if env is not None:
                os.environ["HAVATAR_LPIPS"] = env
            t = timed(fns)
            if rnd >= warm:
                ts[name].append(t)
    os.environ.pop("HAVATAR_LPIPS", None)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


m = he_module()
module_rows = []
for shape in ([] if "--step-only" in sys.argv else SIZES):
    K = 8 if shape[-1] <= 512 else 4
    g = torch.Generator().manual_seed(11)
    sets = []
    for _ in range(K):
        in0 = torch.rand(*shape, generator=g) * 2 - 1
        sets.append((in0.to(dev).requires_grad_(True), (in0 + 0.3 * torch.randn(*shape, generator=g)).clamp(-1, 1).to(dev)))
    for op in ("forward", "forward + backward"):
        def mk(a, b):
            if op == "forward":
                def f():
                    with torch.no_grad():
                        return m(a, b)
                return f
            return lambda: torch.autograd.grad(m(a, b).mean(), a)
        fns = [mk(a, b) for a, b in sets]
        res = alternate({"native": (fns, "1"), "aten": (fns, "0")})
        module_rows.append({"shape": list(shape), "op": op, "K": K, "native_ms": round(res["native"][0], 3), "native_ms_min": round(res["native"][1], 3),
                            "aten_ms": round(res["aten"][0], 3), "aten_ms_min": round(res["aten"][1], 3)})
        r = module_rows[-1]
        print("%-14s %-19s native %9.3f (%9.3f) ms | HAVATAR_LPIPS=0 %9.3f (%9.3f) ms | x%.2f  (K=%d)" % (
            "x".join(map(str, shape)), op, r["native_ms"], r["native_ms_min"], r["aten_ms"], r["aten_ms_min"], r["aten_ms"] / r["native_ms"], K), flush=True)
    del sets, fns
    torch.cuda.empty_cache()

head_rows = []
if "--step-only" not in sys.argv:
    print("# head alone per tap of a 2x3x512x512 pair against a plain copy of the same bytes (both maps): median (min) us", flush=True)
for Cc, S in ([] if "--step-only" in sys.argv else [(64, 512), (128, 256), (256, 128), (512, 64), (512, 32)]):
    K = 8
    sets = [(torch.rand(2, Cc, S, S, device=dev), torch.rand(2, Cc, S, S, device=dev), torch.rand(Cc, device=dev), torch.rand(2, device=dev),
             torch.empty(2, Cc, S, S, device=dev), torch.empty(2, Cc, S, S, device=dev)) for _ in range(K)]

    def copy2(s):
        s[4].copy_(s[0])
        s[5].copy_(s[1])
    res = alternate({"fwd": ([lambda s=s: lpips_ops.head_fwd(s[0], s[1], s[2]) for s in sets], None),
                     "bwd": ([lambda s=s: lpips_ops.head_bwd(s[3], s[0], s[1], s[2], want1=False) for s in sets], None),
                     "copy": ([lambda s=s: copy2(s) for s in sets], None)})
    mb = 2 * 2 * Cc * S * S * 4 / 1e6
    head_rows.append({"shape": [2, Cc, S, S], "MB_both_maps": round(mb, 1), **{k + "_us": round(v[0] * 1e3, 1) for k, v in res.items()},
                      **{k + "_us_min": round(v[1] * 1e3, 1) for k, v in res.items()}})
    r = head_rows[-1]
    print("2x%dx%dx%d (%.1f MB) fwd %8.1f (%8.1f) us | bwd into f0 %8.1f (%8.1f) us | copy %8.1f (%8.1f) us" % (
        Cc, S, S, mb, r["fwd_us"], r["fwd_us_min"], r["bwd_us"], r["bwd_us_min"], r["copy_us"], r["copy_us_min"]), flush=True)
    del sets
    torch.cuda.empty_cache()

step_rows = []
if "--no-step" not in sys.argv:
    from havatar_amd import synth
    from havatar_amd.dataloader.dataloaderSR import Loader
    from havatar_amd.harness import train_hd
    from havatar_amd.utils import styleUnet_util as su
    from havatar_amd.utils.cfgnode import CfgNode
    root = tempfile.mkdtemp()
    split = synth.write_dataset(root, n_frames=2, img_res=512)
    cfg = CfgNode(synth.harness_config(render_size=128, gen_size=512, img_res=512))
    su_args = su.styleUnet_args()
    loader = Loader(split_file=split, mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg, white_bg=True,
                    shuffle=False)
    batch = next(iter(loader))
    torch.manual_seed(5)
    nets = train_hd.build_nets(cfg, su_args, len(loader.dataset), dev)
    for k, seed in (("nerf_render", 0), ("generator", 1), ("discriminator", 2)):
        synth.fill_state_dict(nets[k], seed=seed)
    su.accumulate(nets["g_ema"], nets["generator"], 0)
    nets["nerf_render"].train()
    optims = train_hd.build_optims(cfg, su_args, nets, lr=0.0)          # the weights stay where they are: every round times the same work
    for g in optims["nerf_optimizer"].param_groups:
        g["lr"] = 0.0

    def iteration(percep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        train_hd.joint_step(1, batch, nets, optims, cfg, su_args, percep)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    routes = {"none": (None, None), "native": (m, "1"), "native, HAVATAR_LPIPS=0": (m, "0")}
    ts = {k: [] for k in routes}
    for rnd in range(2 + REPS):
        for name, (percep, env) in routes.items():
            os.environ.pop("HAVATAR_LPIPS", None)
            if env is not None:
                os.environ["HAVATAR_LPIPS"] = env
            t = iteration(percep)
            print("round %d %s: %.3f ms" % (rnd, name, t), file=sys.stderr, flush=True)
            if rnd >= 2:
                ts[name].append(t)
    os.environ.pop("HAVATAR_LPIPS", None)
    print("# eager joint iteration, 128 -> 512, B = 2, i = 1, routes alternating, %d rounds after 2 warm-up rounds: median (min) ms" % REPS)
    for name, v in ts.items():
        step_rows.append({"percep": name, "ms": round(sorted(v)[len(v) // 2], 3), "ms_min": round(min(v), 3)})
        print("--percep %-24s %9.3f (%9.3f) ms" % (name, step_rows[-1]["ms"], step_rows[-1]["ms_min"]), flush=True)

line = json.dumps({"module": module_rows, "head": head_rows, "step": step_rows})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

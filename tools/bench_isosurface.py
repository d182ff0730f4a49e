#!/usr/bin/env python3
"""Mesh export (havatar_amd/geometry.py): what each stage of extract_mesh costs on the device, at 64^3 / 128^3 / 256^3, on the analytic sphere
field and on the density grid of the synthetic checkpoint (weights of havatar_amd.synth, planes of one synthetic frame):
  density_grid        the field evaluation (native/train_ops.field_inputs + the fp32 MLP on rocBLAS), chunked as the default
  native, classify    hav_iso_classify alone
  native, emit        hav_iso_emit alone (its two launches), on outputs sized once
  native, whole call  geometry.isosurface: classify + cumsum + the host read of the totals + allocation + emit
  ATen statement      geometry.isosurface_statement on the same device tensor
Method (tools/bench_metrics.py): routes alternate round by round in one process after two warm-up rounds; HIP events around the launches for
the two entries, wall clock around torch.cuda.synchronize() for the calls that read the totals back; median and minimum over the rounds.
Usage: python tools/bench_isosurface.py [--out FILE] [--rounds N] [--sizes 64,128,256]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from havatar_amd import geometry, synth
from havatar_amd.native import iso_ops

dev = torch.device("cuda:0")
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
SIZES = tuple(int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(",")) if "--sizes" in sys.argv else (64, 128, 256)
SYNTH_ISO = 0.5          # inside the synthetic checkpoint's densities (0 .. 1.1); geometry.DEFAULT_ISO finds nothing in that fog


def avatar():
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    trainer = synth.fill_state_dict(Trainer(CfgNode(synth.harness_config()), 3)).requires_grad_(False).to(dev).eval()
    cond = [torch.from_numpy(c).to(dev) for c in synth.cond_images(1)]
    T = torch.from_numpy(synth.inv_head_T())[None].to(dev)
    with torch.no_grad():
        trainer.model_coarse.set_conditional_embedding(front_render_cond=cond[0], left_render_cond=cond[1], right_render_cond=cond[2],
                                                       latents=trainer.latent_codes[0:1], cond_c=T.view(1, -1))
    return trainer, T


def sphere(res):
    ax = torch.linspace(-1.0, 1.0, res, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.7 - torch.sqrt(x * x + y * y + z * z)).contiguous(), 0.0, (-1.0,) * 3, (2.0 / (res - 1),) * 3


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def rounds(routes, warm=2):
    ts = {k: [] for k in routes}
    for rnd in range(warm + REPS):
        for name, (clock, fn) in routes.items():
            t = clock(fn)
            if rnd >= warm:
                ts[name].append(t)
    return {k: (float(np.median(v)), min(v)) for k, v in ts.items()}


def extraction(f, iso, origin, spacing):
    codes, counts = iso_ops.classify(f, iso)
    boff, V, T = iso_ops.offsets(counts)
    verts, normals = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int32, device=dev)
    routes = {"native, classify": (events, lambda: iso_ops.classify(f, iso)),
              "native, emit": (events, lambda: iso_ops.emit(verts, normals, tris, codes, boff, f, iso, origin, spacing)),
              "native, whole call": (wall, lambda: geometry.isosurface(f, iso, origin, spacing)),
              "ATen statement": (wall, lambda: geometry.isosurface_statement(f, iso, origin, spacing))}
    return V, T, rounds(routes)


def main():
    lines = ["mesh export on %s, torch %s; %d rounds after 2 warm-up rounds; ms, median (minimum)" % (torch.cuda.get_device_name(0),
                                                                                                    torch.__version__, REPS)]
    trainer, T = avatar()
    for res in SIZES:
        with torch.no_grad():
            grid = rounds({"density_grid": (wall, lambda: geometry.density_grid(trainer, T, res))})
            field, origin, spacing = geometry.density_grid(trainer, T, res)
        for name, case in (("sphere", sphere(res)), ("synthetic checkpoint, iso %.1f" % SYNTH_ISO, (field, SYNTH_ISO, origin, spacing))):
            with torch.no_grad():
                V, Tn, r = extraction(*case)
            lines.append("%d^3 %s: V = %d, T = %d" % (res, name, V, Tn))
            if not name.startswith("sphere"):
                lines.append("    %-20s %9.3f (%9.3f)" % ("density_grid", *grid["density_grid"]))
            for k, (med, lo) in r.items():
                lines.append("    %-20s %9.3f (%9.3f)" % (k, med, lo))
            lines.append("    statement / native whole call = %.1f" % (r["ATen statement"][0] / r["native, whole call"][0]))
        print("\n".join(lines[-14:]), flush=True)
    text = "\n".join(lines) + "\n"
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

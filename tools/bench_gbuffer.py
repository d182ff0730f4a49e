#!/usr/bin/env python3
"""The G-buffer (havatar_amd/geometry.py: gbuffer): the kernel of csrc/hav_gbuffer.hip against the ATen statement of the same definition on the
device, on the analytic sphere scene (radius 0.7, 30 % of the pixels without a surface) at 128^2, 512^2 and 1024^2, B = 1 and 4:
  native, kernel      hav_gbuffer_f32 on outputs allocated once (the six maps of geometry.gbuffer), called back to back: at the small sizes
                      this is the rate at which the host enqueues (the binding's checks + one launch), not the kernel's time
  native, in a graph  the same launches captured into one hipGraph and replayed: the kernel's time plus the boundary to the next launch
  native, whole call  geometry.gbuffer: allocation of the six maps + the launch
  ATen statement      geometry.gbuffer_statement on the same device tensors
Method (tools/bench_metrics.py): routes alternate round by round in one process; two warm-up rounds are discarded, the median (and minimum) of
the rounds after them is taken; HIP events around `--calls` back-to-back calls of a route, divided by their number.  The kernel's bytes (every
input read once, every output written once: 40 + 23 bytes per pixel at stride 8) over its time are set against the 6.3 TB/s a float4 copy reaches
on an MI355X (8 TB/s specified).  Every scene but the largest (264 MB) fits the 256 MiB Infinity Cache: their figures are rates out of that
cache, not out of HBM.
Usage: python tools/bench_gbuffer.py [--out FILE] [--rounds N] [--calls K]"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from havatar_amd import geometry
from havatar_amd.native import gbuffer_ops

dev = torch.device("cuda:0")
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
CALLS = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 20
COPY_TBS = 6.3


def scene(B, S, seed=0):
    """rays [B, S S, 8], depth, acc [B, S S]: a pinhole camera of focal 1.6 S, 3 units from a sphere of radius 0.7, near 1.7, far 4.3"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ax = (torch.arange(S, dtype=torch.float64) + 0.5 - S / 2) / (1.6 * S)
    y, x = torch.meshgrid(ax, ax, indexing="ij")
    d = torch.stack([x, y, torch.ones_like(x)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    c, s = math.cos(0.3), math.sin(0.3)
    R = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], dtype=torch.float64)
    o, d = R @ torch.tensor([0.0, 0.0, -3.0], dtype=torch.float64), d @ R.T
    b = d @ o
    disc = b * b - (o @ o - 0.49)
    hit = disc > 0
    t = torch.where(hit, -b - disc.clamp_min(0).sqrt(), torch.full_like(b, 3.0))
    rays = torch.cat([o.expand(S, S, 3), d, torch.full((S, S, 1), 1.7, dtype=torch.float64), torch.full((S, S, 1), 4.3, dtype=torch.float64)], -1)
    acc = torch.where(hit, 0.6 + 0.4 * torch.rand(B, S, S, generator=g, dtype=torch.float64), 0.3 * torch.rand(B, S, S, generator=g, dtype=torch.float64))
    acc = torch.where(torch.rand(B, S, S, generator=g) < 0.3, torch.zeros_like(acc), acc)
    f = lambda a, *tail: a.float().reshape(B, S * S, *tail).contiguous().to(dev)
    return f(rays.expand(B, S, S, 8), 8), f(acc * t), f(acc)


def events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def rounds(routes, warm=2):
    """routes: name -> (calls per round, what one call does, launches per call)"""
    ts = {k: [] for k in routes}
    for rnd in range(warm + REPS):
        for name, (calls, fn, per) in routes.items():
            t = events(fn, calls) / per
            if rnd >= warm:
                ts[name].append(t)
    return {k: (float(np.median(v)), min(v)) for k, v in ts.items()}


def main():
    lines = ["G-buffer on %s, torch %s; tile %d x %d; %d rounds after 2 warm-up rounds, %d calls per round (statement: %d); ms per call, median "
             "(minimum)" % (torch.cuda.get_device_name(0), torch.__version__, *gbuffer_ops.tile(), REPS, CALLS, max(CALLS // 5, 1))]
    names = geometry.GBuffer._fields
    for S in (128, 512, 1024):
        for B in (1, 4):
            rays, depth, acc = scene(B, S)
            out = {k: torch.empty((B, S, S) + gbuffer_ops.OUTPUTS[k][0], dtype=gbuffer_ops.OUTPUTS[k][1], device=dev) for k in names}
            with torch.no_grad():
                gbuffer_ops.gbuffer_into(out, rays, depth, acc, S, S, 0.5)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(CALLS):
                        gbuffer_ops.gbuffer_into(out, rays, depth, acc, S, S, 0.5)
                r = rounds({"native, kernel": (CALLS, lambda: gbuffer_ops.gbuffer_into(out, rays, depth, acc, S, S, 0.5), 1),
                            "native, in a graph": (1, graph.replay, CALLS),
                            "native, whole call": (CALLS, lambda: geometry.gbuffer(rays, depth, acc, S, S, 0.5), 1),
                            "ATen statement": (max(CALLS // 5, 1), lambda: geometry.gbuffer_statement(rays, depth, acc, S, S, 0.5), 1)})
                got, ref = geometry.gbuffer(rays, depth, acc, S, S, 0.5), geometry.gbuffer_statement(rays, depth, acc, S, S, 0.5)
            same = all(torch.equal(getattr(got, k), getattr(ref, k)) for k in ("mask", "depth16")) and torch.equal(got.z.view(torch.int32),
                                                                                                                    ref.z.view(torch.int32))
            nbytes = B * S * S * (rays.shape[2] * 4 + 8 + sum(int(np.prod(gbuffer_ops.OUTPUTS[k][0], dtype=np.int64)) * out[k].element_size()
                                                                for k in names))
            tbs = nbytes / (r["native, in a graph"][0] * 1e-3) / 1e12
            lines.append("%d^2, B = %d: %d pixels with a surface, %d with a normal; z, mask and depth16 %s the statement's on the device"
                         % (S, B, int((got.mask & 1).sum()), int(((got.mask & 2) != 0).sum()), "equal" if same else "DIFFER FROM"))
            for k, (med, lo) in r.items():
                lines.append("    %-20s %9.4f (%9.4f)" % (k, med, lo))
            lines.append("    kernel in a graph: %.2f MB in and out, %.3f TB/s = %.0f %% of a float4 copy's %.1f TB/s; statement / native whole call = %.1f"
                         % (nbytes / 1e6, tbs, 100 * tbs / COPY_TBS, COPY_TBS, r["ATen statement"][0] / r["native, whole call"][0]))
            print("\n".join(lines[-6:]), flush=True)
    text = "\n".join(lines) + "\n"
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""hav_composite_long_{fwd,bwd} (native/train_ops.py::composite_long, csrc/hav_composite_long.hip) against the ATen statement it
replaces on the training route (utils/nerf_util.py::volume_render_radiance_field under autograd), at 8 192 rays x S in {80, 96, 128}
x 69 words per sample; the existing composite at S = 64 next to it for a per-sample comparison; every arrangement of the backward
(by shape / staged, one wave per workgroup / staged, two waves / rows from memory).

Method (tools/bench_decoder.py): every timed launch works on its OWN buffers, K distinct sets covering >= 1 GiB; the K launches of a
route are captured back to back in one hipGraph and the graph is replayed; the routes alternate, round by round, in one process; median
and minimum of the time per launch.  All routes run under autograd ("forward" = the statement, "forward + backward" = the statement
and torch.autograd.grad of it with an upstream gradient on all four maps).  One exception: the backward of ATen's cumprod asks the
host whether its input holds a zero and cannot be captured, so the ATen "forward + backward" is timed eagerly -- the same K launches
on the same K buffer sets between two events (about 60 ATen launches of 2-25 MB each per statement: the device, not the host, sets
the pace).
Usage: python tools/bench_composite_long.py [--out FILE]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from havatar_amd.native import train_ops
from havatar_amd.utils.nerf_util import volume_render_radiance_field

dev = torch.device("cuda:0")
FOOTPRINT = 1 << 30
N, CH = 8192, 68
REPS = 9
FORMS = [("by shape", 0), ("staged 1 wave", 1), ("staged 2 waves", 2), ("rows from memory", 3)]


def graphed(make, bytes_per_launch, kmax=16):
    K = int(min(kmax, max(4, -(-FOOTPRINT // max(1, bytes_per_launch)))))
    fns = [make(i) for i in range(K)]
    for f in fns[:3]:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [f() for f in fns]
    return g, K, (fns, keep)


class Eager:
    """the K launches run eagerly: what replay() does for a route that cannot be captured"""

    def __init__(self, fns):
        self.fns = fns

    def replay(self):
        for f in self.fns:
            f()


def eager(make, bytes_per_launch, kmax=16):
    K = int(min(kmax, max(4, -(-FOOTPRINT // max(1, bytes_per_launch)))))
    fns = [make(i) for i in range(K)]
    for f in fns[:3]:
        f()
    torch.cuda.synchronize()
    return Eager(fns), K, fns


def alternate(graphs):
    ts = {k: [] for k in graphs}
    for _ in range(REPS):
        for name, (g, K, _) in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); g.replay(); b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b) / K * 1e3)
    return {k: (round(sorted(v)[len(v) // 2], 1), round(min(v), 1)) for k, v in ts.items()}


def aten(rf, z, rd, noise, bg):
    r2 = torch.cat([rf[..., :-1], rf[..., -1:] + noise[..., None]], -1)          # inject the draw: sigma = relu(raw + noise)
    rgb, _, acc, w, depth = volume_render_radiance_field(r2, z, rd, 0.0, act_feat=False, background_prior=bg)
    return rgb, acc, w, depth


rows = []
for S in (64, 80, 96, 128):
    sets = {}

    def bufs(i):
        if i not in sets:
            g = torch.Generator(device=dev).manual_seed(100 * S + i)
            rf = (torch.randn(N, S, CH + 1, device=dev, generator=g) * 2).requires_grad_(True)
            z = torch.sort(torch.rand(N, S, device=dev, generator=g) * 2.6 + 3.4, -1)[0]
            rd = torch.randn(N, 3, device=dev, generator=g)
            noise = torch.randn(N, S, device=dev, generator=g) * 0.5
            bg = torch.rand(N, 3, device=dev, generator=g)
            ups = [torch.randn(s, device=dev, generator=g) for s in ((N, CH), (N,), (N, S), (N,))]
            sets[i] = (rf, z, rd, noise, bg, ups)
        return sets[i]

    def mk(fn, bwd):
        def make(i):
            rf, z, rd, noise, bg, ups = bufs(i)
            if bwd:
                return lambda: torch.autograd.grad(fn(rf, z, rd, noise, bg), (rf,), ups)
            return lambda: [t.detach() for t in fn(rf, z, rd, noise, bg)]
        return make

    by = 4 * N * S * (CH + 1)
    routes_f = {"aten": mk(aten, False), "composite_long": mk(lambda *a: train_ops.composite_long(*a, n_sigmoid=3), False)}
    routes_b = {"aten": mk(aten, True)}          # (eager: see the head of this file)
    for name, form in FORMS:
        routes_b["composite_long, " + name] = mk(lambda *a, form=form: train_ops.composite_long(*a, n_sigmoid=3, bwd_form=form), True)
    if S <= 64:
        routes_f["composite"] = mk(lambda *a: train_ops.composite(*a, n_sigmoid=3), False)
        routes_b["composite"] = mk(lambda *a: train_ops.composite(*a, n_sigmoid=3), True)
    for op, routes, factor in (("forward", routes_f, 1), ("forward + backward", routes_b, 3)):
        gs = {k: (eager if (k == "aten" and factor == 3) else graphed)(v, factor * by) for k, v in routes.items()}
        r = alternate(gs)
        for k, (med, mn) in r.items():
            rows.append({"S": S, "op": op, "route": k, "us_median": med, "us_min": mn, "distinct_buffer_sets": gs[k][1],
                         "timed": "eager" if isinstance(gs[k][0], Eager) else "graph"})
        del gs
    sets.clear()
    torch.cuda.empty_cache()

print("# %d rays x S x %d words; per launch, K launches on K distinct buffer sets replayed as one hipGraph, routes alternating, %d rounds: "
      "median (min) us" % (N, CH + 1, REPS))
for r in rows:
    print("S %3d  %-19s %-34s %9.1f (%9.1f) us   (K=%d, %s)" % (r["S"], r["op"], r["route"], r["us_median"], r["us_min"], r["distinct_buffer_sets"],
                                                                 r["timed"]))
get = lambda S, op, route: next(r["us_median"] for r in rows if (r["S"], r["op"], r["route"]) == (S, op, route))
for op, long_route in (("forward", "composite_long"), ("forward + backward", "composite_long, by shape")):
    print("# per sample, %s: composite_long at 128 / composite at 64 = x%.2f (twice the samples)" % (
        op, get(128, op, long_route) / get(64, op, "composite")))
    for S in (80, 96, 128):
        print("# S %d %s: aten / composite_long = x%.2f" % (S, op, get(S, op, "aten") / get(S, op, long_route)))
line = json.dumps({"rows": rows})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

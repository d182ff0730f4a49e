#!/usr/bin/env python3
"""The skinning-volume decoder's InstanceNorm3d + ReLU node and its output layer (native/train_ops.py::InormRelu3d, FinalConvSigmoid:
csrc/hav_decoder.hip) against the ATen statements they replace, and VolumeDecoder(1024, final_res=64) forward + backward on its three
routes (default, HAVATAR_CONV3D=hip, HAVATAR_DECODER=hip).

Method (tools/bench_conv3d.py): every timed launch works on its OWN buffers, K distinct sets covering >= 1 GiB (the decoder: K copies of
the module); the K launches of a route are captured back to back in one hipGraph and the graph is replayed; the routes alternate, round
by round, in one process; median and minimum of the time per launch.  Both routes run under autograd, as the decoder runs them
("forward" = the statement, "forward + backward" = the statement and torch.autograd.grad of it); the closures, which own the buffers a
graph writes, are kept alive next to their graph until its last replay.
(a) per node and decoder shape; (b) the whole decoder.
Usage: python tools/bench_decoder.py [--out FILE]"""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from havatar_amd.model.network.voxel_encoder import VolumeDecoder
from havatar_amd.native import train_ops

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True          # as tools/bench_train.py and the training harness run
FOOTPRINT = 1 << 30
NORM_SHAPES = [(512, 2), (256, 4), (128, 8), (64, 16), (32, 32), (16, 64)]
FINAL_SHAPES = [(32, 32), (16, 64)]
REPS = 9
EPS = 1e-5


def graphed(make, bytes_per_launch, kmax=64):
    """make(i) -> a launch closure on buffer set i.  -> (graph of the K launches, K, the closures: they own the buffers the graph writes)"""
    K = int(min(kmax, max(8, -(-FOOTPRINT // max(1, bytes_per_launch)))))
    fns = [make(i) for i in range(K)]
    for f in fns[:3]:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [f() for f in fns]
    return g, K, (fns, keep)


def alternate(graphs):
    """graphs: {name: (graph, K, closures)} -> {name: (median us, min us) per launch}, the graphs replayed in turn, REPS rounds"""
    ts = {k: [] for k in graphs}
    for _ in range(REPS):
        for name, (g, K, _) in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b) / K * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


rows = []


def compare(layer, op, nat, aten, by):
    gs = {"native": graphed(nat, by), "aten": graphed(aten, by)}
    r = alternate(gs)
    rows.append({"node": layer, "op": op, "distinct_buffer_sets": gs["native"][1], "native_us_median": round(r["native"][0], 1),
                 "native_us_min": round(r["native"][1], 1), "aten_us_median": round(r["aten"][0], 1), "aten_us_min": round(r["aten"][1], 1)})
    del gs


# (a) the norm
for Cc, R in NORM_SHAPES:
    sets = {}

    def bufs(i):
        if i not in sets:
            sets[i] = (torch.randn(1, Cc, R, R, R, device=dev, requires_grad=True), torch.randn(1, Cc, R, R, R, device=dev))
        return sets[i]

    def mk(fn, bwd):
        def make(i):
            y, g = bufs(i)
            if bwd:
                return lambda: torch.autograd.grad(fn(y), (y,), g)
            return lambda: fn(y).detach()
        return make

    nat = lambda y: train_ops.inorm_relu3d(y, EPS)
    aten = lambda y: torch.relu(F.instance_norm(y, eps=EPS))
    by = 4 * Cc * R ** 3 * 2
    name = "inorm_relu3d %d x %d^3" % (Cc, R)
    compare(name, "forward", mk(nat, False), mk(aten, False), by)
    compare(name, "forward + backward", mk(nat, True), mk(aten, True), 2 * by)
    sets.clear()
    torch.cuda.empty_cache()

# (a) the output layer
for Cin, R in FINAL_SHAPES:
    conv = torch.nn.Conv3d(Cin, 1, 3, padding=1).to(dev)
    sets = {}

    def bufs(i):
        if i not in sets:
            sets[i] = (torch.randn(1, Cin, R, R, R, device=dev, requires_grad=True), torch.randn(1, 2, R, R, R, device=dev))
        return sets[i]

    def aten(x):
        s = torch.sigmoid(conv(x))
        return torch.cat([s, 1 - s], 1)

    def mk(fn, bwd):
        def make(i):
            x, g = bufs(i)
            if bwd:
                return lambda: torch.autograd.grad(fn(x), (x, conv.weight, conv.bias), g)
            return lambda: fn(x).detach()
        return make

    nat = lambda x: train_ops.final_conv_sigmoid(x, conv)
    by = 4 * (Cin + 2) * R ** 3
    name = "final_conv_sigmoid %d ch @ %d^3" % (Cin, R)
    compare(name, "forward", mk(nat, False), mk(aten, False), by)
    compare(name, "forward + backward", mk(nat, True), mk(aten, True), 2 * by)
    sets.clear()
    torch.cuda.empty_cache()

# (b) the decoder, forward + backward, K copies of the module
ROUTES = [("default", {}), ("HAVATAR_CONV3D=hip", {"HAVATAR_CONV3D": "hip"}), ("HAVATAR_DECODER=hip", {"HAVATAR_DECODER": "hip"})]
torch.manual_seed(0)
base = VolumeDecoder(num_in=1024, final_res=64).to(dev)
decs = [copy.deepcopy(base) for _ in range(8)]
ups = [torch.randn(1, 2, 64, 64, 64, device=dev) for _ in decs]
graphs = {}
for name, env in ROUTES:
    for k in ("HAVATAR_CONV3D", "HAVATAR_DECODER"):
        os.environ.pop(k, None)
    os.environ.update(env)          # the switches are read at call time: what the capture runs is what the replay runs

    def make(i):
        d, u = decs[i], ups[i]
        return lambda: torch.autograd.grad(d(), list(d.parameters()), u)
    graphs[name] = graphed(make, FOOTPRINT // 8, kmax=8)
for k in ("HAVATAR_CONV3D", "HAVATAR_DECODER"):
    os.environ.pop(k, None)
r = alternate(graphs)
dec_rows = [{"decoder": "VolumeDecoder(1024, 64) forward + backward", "route": name, "us_median": round(r[name][0], 1), "us_min": round(r[name][1], 1),
             "copies": graphs[name][1]} for name, _ in ROUTES]

print("# per launch, K launches on K distinct buffer sets replayed as one hipGraph, routes alternating, %d rounds: median (min) us" % REPS)
for r in rows:
    print("%-34s %-19s native %8.1f (%8.1f) us | aten %8.1f (%8.1f) us | x%.2f   (K=%d)" % (
        r["node"], r["op"], r["native_us_median"], r["native_us_min"], r["aten_us_median"], r["aten_us_min"],
        r["aten_us_median"] / r["native_us_median"], r["distinct_buffer_sets"]))
for r in dec_rows:
    print("%-44s %-20s %8.1f (%8.1f) us   (K=%d)" % (r["decoder"], r["route"], r["us_median"], r["us_min"], r["copies"]))
line = json.dumps({"nodes": rows, "decoder": dec_rows})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

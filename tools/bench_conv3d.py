#!/usr/bin/env python3
"""The three large 3x3x3 layers of VolumeDecoder(num_in=1024, final_res=64) -- forward, data gradient, weight (+ bias) gradient -- on this
library's split-fp16 kernels (hav_conv3d_k3_*, what native/train_ops.py::Conv3dK3 launches) against the ATen route the decoder takes by
default (F.conv3d / aten::convolution_backward, fp32, NCDHW: MIOpen / CK with their layout conversions).

Method (tools/bench_ops.py): every timed launch works on its OWN buffers, K distinct sets covering >= 1 GiB; the K launches of a route
are captured back to back in one hipGraph (no host gaps) and the graph is replayed; the two routes alternate, round by round, in one
process; median and minimum of the time per launch.  A captured graph holds raw addresses only: the closures, and with them every output
and scratch buffer they own, are kept alive next to their graph until its last replay (a buffer that dies after the capture goes back to
the allocator, the cache flush of the next capture or of MIOpen's solver search returns it to the driver, and the replay writes to
unmapped memory).
Native rows include what the autograd node pays around the convolution: hav_absmax(x) in the forward, hav_absmax(g) in the data
gradient (the weight gradient reuses both sets of words); the weight packs are timed apart (once per step and layer each).
Usage: python tools/bench_conv3d.py [--out FILE]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from havatar_amd import _lib
from havatar_amd.native import train_ops
from havatar_amd.native.conv import absmax

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True          # as tools/bench_train.py and the training harness run
FOOTPRINT = 1 << 30
LAYERS = [(128, 64, 16), (64, 32, 32), (32, 16, 64)]
REPS = 9


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def graphed(make, bytes_per_launch):
    """make(i) -> a launch closure on buffer set i.  -> (graph of the K launches, K, the closures: they own the buffers the graph writes)"""
    K = int(min(64, max(8, -(-FOOTPRINT // max(1, bytes_per_launch)))))
    fns = [make(i) for i in range(K)]
    for f in fns[:3]:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    return g, K, fns


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


L = _lib.lib()
rows = []
for Cin, Cout, R in LAYERS:
    vox = R ** 3
    flop = 2.0 * 27 * Cin * Cout * vox
    w = torch.randn(Cout, Cin, 3, 3, 3, device=dev) / (27 * Cin) ** 0.5
    bias = torch.randn(Cout, device=dev) * 0.1
    blob, blob_t = train_ops._conv3d_k3_blob(w, False), train_ops._conv3d_k3_blob(w, True)
    by = 4 * vox * (Cin + Cout)
    sets = {}

    def bufs(i):
        if i not in sets:
            x, g = torch.randn(1, Cin, R, R, R, device=dev), torch.randn(1, Cout, R, R, R, device=dev) * 1e-4
            sets[i] = (x, g, absmax(x), absmax(g))
        return sets[i]

    def nat_fwd(i):
        x = bufs(i)[0]
        y = torch.empty(1, Cout, R, R, R, device=dev)

        def f():
            train_ops._conv3d_k3_run(y, x, blob, bias, absmax(x), 1, Cin, Cout, R, R, R)
        return f

    def nat_dgrad(i):
        g = bufs(i)[1]
        dx = torch.empty(1, Cin, R, R, R, device=dev)

        def f():
            train_ops._conv3d_k3_run(dx, g, blob_t, None, absmax(g), 1, Cout, Cin, R, R, R)
        return f

    def nat_wgrad(i):
        x, g, xa, ga = bufs(i)
        dw, db = torch.empty_like(w), torch.empty_like(bias)
        scratch = torch.empty(int(L.hav_conv3d_k3_wgrad_scratch_bytes(1, Cin, Cout, R, R, R)), dtype=torch.uint8, device=dev)

        def f():
            _lib.check(L.hav_conv3d_k3_wgrad(_p(dw), _p(db), _p(g), _p(x), _p(scratch), _p(ga), _p(xa), 1, Cin, Cout, R, R, R, _st()), "wgrad")
        return f

    def nat_pack(i):
        return lambda: (_lib.check(L.hav_conv3d_k3_pack(_p(blob), _p(w), Cout, Cin, 1.0, _st()), "pack"),
                        _lib.check(L.hav_conv3d_k3_pack_t(_p(blob_t), _p(w), Cout, Cin, 1.0, _st()), "pack_t"))

    def aten_fwd(i):
        x = bufs(i)[0]
        return lambda: F.conv3d(x, w, bias, padding=1)

    def aten_bwd(mask):
        def mk(i):
            x, g = bufs(i)[:2]
            return lambda: torch.ops.aten.convolution_backward(g, x, w, [Cout], [1, 1, 1], [1, 1, 1], [1, 1, 1], False, [0, 0, 0], 1, mask)
        return mk

    ops = (("forward", nat_fwd, aten_fwd), ("data gradient", nat_dgrad, aten_bwd([True, False, False])),
           ("weight + bias gradient", nat_wgrad, aten_bwd([False, True, True])))
    for op, nat, aten in ops:
        gs = {"native": graphed(nat, by), "aten": graphed(aten, by)}
        r = alternate(gs)
        rows.append({"layer": "%d->%d @ %d^3" % (Cin, Cout, R), "op": op, "gflop": round(flop / 1e9, 2), "distinct_buffer_sets": gs["native"][1],
                     "native_us_median": round(r["native"][0], 1), "native_us_min": round(r["native"][1], 1),
                     "aten_us_median": round(r["aten"][0], 1), "aten_us_min": round(r["aten"][1], 1),
                     "native_tflops": round(flop / r["native"][0] / 1e6, 1), "aten_tflops": round(flop / r["aten"][0] / 1e6, 1)})
        del gs
    r = alternate({"pack": graphed(nat_pack, FOOTPRINT // 8)})
    rows.append({"layer": "%d->%d @ %d^3" % (Cin, Cout, R), "op": "pack + pack_t (once per step)", "native_us_median": round(r["pack"][0], 1),
                 "native_us_min": round(r["pack"][1], 1)})
    sets.clear()
    torch.cuda.empty_cache()

print("# per launch, K launches on K distinct buffer sets replayed as one hipGraph, routes alternating, %d rounds: median (min) us" % REPS)
for r in rows:
    if "aten_us_median" in r:
        print("%-18s %-24s native %8.1f (%8.1f) us %6.1f TFLOP/s | aten %8.1f (%8.1f) us %6.1f TFLOP/s | x%.2f   (K=%d)" % (
            r["layer"], r["op"], r["native_us_median"], r["native_us_min"], r["native_tflops"], r["aten_us_median"], r["aten_us_min"],
            r["aten_tflops"], r["aten_us_median"] / r["native_us_median"], r["distinct_buffer_sets"]))
    else:
        print("%-18s %-24s native %8.1f (%8.1f) us" % (r["layer"], r["op"], r["native_us_median"], r["native_us_min"]))
line = json.dumps(rows)
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

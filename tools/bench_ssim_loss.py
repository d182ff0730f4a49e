#!/usr/bin/env python3
"""SSIM training loss (havatar_amd.metrics.ssim_loss), forward + backward: the node of native/ssim_ops.py (csrc/hav_metrics.hip forward,
csrc/hav_ssim_loss.hip backward) against the ATen statement under autograd (HAVATAR_METRICS=0: the route a pair that needs a gradient took
before the node existed), float32 pairs on the device at (2,3,64,64) -- the stage-one patch --, (2,3,512,512) and (1,3,1024,1024).

Method (tools/bench_metrics.py, tools/bench_train_hd.py): K distinct buffer sets; per route ONE hipGraph that holds the K forward + backward
passes (what a captured training step pays: kernel time without launch overhead), the two graphs replayed alternately in one process after
two warm-up rounds, median and minimum over the rounds of the time per pass, HIP events.  The same K passes are also timed as eager launches,
routes alternating: what the eager stage-two step pays.  The statement uploads its 11-tap window from the host at every call, which a capture
refuses; for the captures alone the window is made on the device once (metrics.gaussian_window is replaced for their duration), which favours
the statement: the graph column compares kernels only.  The last column is the largest difference of the two routes' gradients over the
largest gradient entry (a sanity check, not an accuracy statement: tests/test_ssim_loss_gpu.py holds that).
The kernels' own times: `rocprofv3 --kernel-trace --stats -- python tools/bench_ssim_loss.py`, in a run of its own.
Usage: python tools/bench_ssim_loss.py [--out FILE] [--rounds N]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from havatar_amd import metrics

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 9
SHAPES = ((2, 3, 64, 64), (2, 3, 512, 512), (1, 3, 1024, 1024))
K = 8
ROUTES = (("node", "1"), ("aten", "0"))


def pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    S = shape[-1]
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    a = (0.5 + 0.3 * torch.sin(xx / 7.0 + 0.5) * torch.cos(yy / 5.0) + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return a.to(dev).requires_grad_(True), (a + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1).to(dev)


_windows, _host_window = {}, metrics.gaussian_window


def device_window(dtype=torch.float64):
    if dtype not in _windows:
        _windows[dtype] = _host_window(dtype).to(dev)
    return _windows[dtype]


def passes(pairs):
    """the K forward + backward passes under the route the environment selects; -> the gradients"""
    return [torch.autograd.grad(metrics.ssim_loss(x, y), x)[0] for x, y in pairs]


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, n, warm=2):
    ts = {name: [] for name in fns}
    for rnd in range(warm + REPS):
        for name, env in ROUTES:
            os.environ["HAVATAR_METRICS"] = env
            t = timed(fns[name], n)
            if rnd >= warm:
                ts[name].append(t)
    os.environ.pop("HAVATAR_METRICS", None)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


rows = []
for shape in SHAPES:
    pairs = [pair(shape, 100 + k) for k in range(K)]
    graphs, grads = {}, {}
    side = torch.cuda.Stream()
    metrics.gaussian_window = device_window
    device_window(torch.float32)
    for name, env in ROUTES:
        os.environ["HAVATAR_METRICS"] = env
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # solver selection and lazy initialisation before the capture
            passes(pairs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            grads[name] = passes(pairs)
    os.environ.pop("HAVATAR_METRICS", None)
    metrics.gaussian_window = _host_window
    res_g = alternate({name: graphs[name].replay for name, _ in ROUTES}, K)
    res_e = alternate({name: (lambda: passes(pairs)) for name, _ in ROUTES}, K)
    gmax = max(float(g.abs().max()) for g in grads["aten"])
    apart = max(float((a - b).abs().max()) for a, b in zip(grads["node"], grads["aten"])) / gmax
    r = {"shape": list(shape), "apart_over_max": apart}
    for mode, res in (("graph", res_g), ("eager", res_e)):
        for name, _ in ROUTES:
            r["%s_%s_us" % (mode, name)], r["%s_%s_us_min" % (mode, name)] = round(res[name][0] * 1e3, 1), round(res[name][1] * 1e3, 1)
    rows.append(r)
    print("%-16s graph: node %9.1f (%9.1f) us | HAVATAR_METRICS=0 %9.1f (%9.1f) us | x%.1f || eager: node %9.1f (%9.1f) us | "
          "HAVATAR_METRICS=0 %9.1f (%9.1f) us | x%.1f || routes apart %.1e of max|g|" % (
              "x".join(map(str, shape)), r["graph_node_us"], r["graph_node_us_min"], r["graph_aten_us"], r["graph_aten_us_min"],
              r["graph_aten_us"] / r["graph_node_us"], r["eager_node_us"], r["eager_node_us_min"], r["eager_aten_us"], r["eager_aten_us_min"],
              r["eager_aten_us"] / r["eager_node_us"], apart), flush=True)
    del pairs, graphs, grads
    torch.cuda.empty_cache()

line = json.dumps({"ab": rows, "K": K, "rounds": REPS})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

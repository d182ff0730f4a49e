#!/usr/bin/env python3
"""The wavelet autograd nodes of stage two (native/train_ops.py::HaarDwt / HaarIdwt / HaarUp2 / HaarDown2, HAVATAR_HAAR_TRAIN=1) against
the statements they replace under autograd, at the shapes stage two uses, and the Discriminator's two iterations with the switch set
and unset.

Method (tools/bench_decoder.py): every timed launch works on its OWN buffers, K distinct sets covering >= 1 GiB; the K launches of a route
are captured back to back in one hipGraph and the graph is replayed; the routes alternate, round by round, in one process; median and
minimum of the time per launch.  (a) per node and shape, forward and forward + backward, with the algorithmic bytes (input + output, both
ways for the backward) per second next to a plain copy that moves the same bytes.  (b) Discriminator(1024, 3) and Discriminator(512, 3)
at B = 2: the logistic-loss iteration (two forwards, loss, backward) and the R1 iteration (forward, d_r1_loss, backward); these run
eagerly (the R1 step builds its second-order graph on the fly), on K distinct input sets, switch set and unset alternating.
Progress of (b) goes to stderr round by round (the first rounds at 1024^2 spend minutes in MIOpen's search).
Usage: python tools/bench_discriminator.py [--out FILE] [--nodes-only | --discriminator-only] [--sizes 512,1024]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from havatar_amd import synth
from havatar_amd.model.styleUnet import Discriminator, Downsample, HaarTransform, InverseHaarTransform, Upsample, _haar_bank
from havatar_amd.native import train_ops
from havatar_amd.utils import styleUnet_util as su

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True          # as tools/bench_train.py and the training harness run
FOOTPRINT = 1 << 30
REPS = 9
os.environ.pop("HAVATAR_HAAR_TRAIN", None)
# (node, input shape): dwt takes the image, the others the wavelet-domain tensor
SHAPES = ([("dwt", (2, 3, 1024, 1024)), ("dwt", (2, 3, 512, 512))] + [("down2", (2, 12, r, r)) for r in (512, 256, 128, 64, 32)]
          + [("up2", (2, 12, r, r)) for r in (512, 256, 128, 64, 32)] + [("idwt", (2, 12, 512, 512))])

dwt, iwt, up, down = (m.to(dev) for m in (HaarTransform(3), InverseHaarTransform(3), Upsample((1, 3, 3, 1)), Downsample((1, 3, 3, 1))))
kd, ki = _haar_bank(dwt, (dwt.ll, dwt.lh, dwt.hl, dwt.hh)), _haar_bank(iwt, (iwt.ll, iwt.lh, iwt.hl, iwt.hh))
NODE = {"dwt": lambda x: train_ops.haar_dwt(x, kd), "idwt": lambda x: train_ops.haar_idwt(x, ki),
        "up2": lambda x: train_ops.haar_up2(x, ki, up.kernel, kd), "down2": lambda x: train_ops.haar_down2(x, ki, down.kernel, kd)}
STATEMENT = {"dwt": lambda x: dwt(x), "idwt": lambda x: iwt(x), "up2": lambda x: dwt(up(iwt(x))), "down2": lambda x: dwt(down(iwt(x)))}


def graphed(make, bytes_per_launch, kmax=64):
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
    ts = {k: [] for k in graphs}
    for _ in range(REPS):
        for name, (g, K, _) in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b) / K * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


rows = []
for node, shape in ([] if "--discriminator-only" in sys.argv else SHAPES):
    with torch.no_grad():
        out_shape = tuple(STATEMENT[node](torch.zeros(shape, device=dev)).shape)
    n_in, n_out = 1, 1
    for s in shape:
        n_in *= s
    for s in out_shape:
        n_out *= s
    sets = {}

    def bufs(i):
        if i not in sets:
            sets[i] = (torch.randn(shape, device=dev, requires_grad=True), torch.randn(out_shape, device=dev),
                       torch.empty((n_in + n_out) // 2, device=dev), torch.empty((n_in + n_out) // 2, device=dev))
        return sets[i]

    def mk(fn, bwd):
        def make(i):
            x, g = bufs(i)[:2]
            if bwd:
                return lambda: torch.autograd.grad(fn(x), (x,), g)
            return lambda: fn(x).detach()
        return make

    def mk_copy(times):
        def make(i):
            src, dst = bufs(i)[2:]
            return lambda: [dst.copy_(src) for _ in range(times)]
        return make

    for op, bwd in (("forward", False), ("forward + backward", True)):
        by = 4 * (n_in + n_out) * (2 if bwd else 1)
        gs = {"node": graphed(mk(NODE[node], bwd), by), "statement": graphed(mk(STATEMENT[node], bwd), by), "copy": graphed(mk_copy(2 if bwd else 1), by)}
        r = alternate(gs)
        rows.append({"node": node, "shape": list(shape), "op": op, "K": gs["node"][1], "bytes": by,
                     "node_us": round(r["node"][0], 1), "node_us_min": round(r["node"][1], 1),
                     "statement_us": round(r["statement"][0], 1), "statement_us_min": round(r["statement"][1], 1),
                     "copy_us": round(r["copy"][0], 1), "node_GBps": round(by / r["node"][0] / 1e3, 1),
                     "statement_GBps": round(by / r["statement"][0] / 1e3, 1), "copy_GBps": round(by / r["copy"][0] / 1e3, 1)})
        del gs
    sets.clear()
    torch.cuda.empty_cache()

if rows:
    print("# (a) per launch, K launches on K distinct buffer sets replayed as one hipGraph, routes alternating, %d rounds: median (min) us; GB/s of" % REPS)
    print("#     algorithmic bytes (input + output, twice for forward + backward); copy = dst.copy_(src) moving the same bytes")
for r in rows:
    print("%-6s %-20s %-19s node %8.1f (%8.1f) us %7.1f GB/s | statement %8.1f (%8.1f) us %7.1f GB/s | x%.2f | copy %8.1f us %7.1f GB/s  (K=%d)" % (
        r["node"], "x".join(map(str, r["shape"])), r["op"], r["node_us"], r["node_us_min"], r["node_GBps"], r["statement_us"],
        r["statement_us_min"], r["statement_GBps"], r["statement_us"] / r["node_us"], r["copy_us"], r["copy_GBps"], r["K"]))

disc_rows = []
if "--nodes-only" not in sys.argv:
    K, B = 4, 2
    args = su.styleUnet_args()
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [1024, 512]
    for size in sizes:
        torch.manual_seed(0)
        d = synth.fill_state_dict(Discriminator(size, 3, channel_multiplier=2)).to(dev)
        reals = [torch.randn(B, 3, size, size, device=dev) for _ in range(K)]
        fakes = [torch.randn(B, 3, size, size, device=dev) for _ in range(K)]

        def logistic(i):
            loss = su.d_logistic_loss(d(reals[i]), d(fakes[i]))
            d.zero_grad(set_to_none=True)
            loss.backward()

        def r1(i):
            x = reals[i].detach().requires_grad_(True)
            pred = d(x)
            loss = su.d_r1_loss(pred, x)
            d.zero_grad(set_to_none=True)
            (args.r1 / 2 * loss * args.d_reg_every + 0 * pred[0]).backward()

        for it_name, it in (("logistic-loss iteration", logistic), ("R1 iteration", r1)):
            ts = {"unset": [], "set": []}
            for rnd in range(2 + REPS):          # two warm-up rounds (MIOpen's search, code objects), then REPS timed ones
                for route in ("unset", "set"):
                    os.environ.pop("HAVATAR_HAAR_TRAIN", None)
                    if route == "set":
                        os.environ["HAVATAR_HAAR_TRAIN"] = "1"
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for i in range(K):
                        it(i)
                    b.record()
                    torch.cuda.synchronize()
                    print("%d %s round %d %s: %.3f ms" % (size, it_name, rnd, route, a.elapsed_time(b) / K), file=sys.stderr, flush=True)
                    if rnd >= 2:
                        ts[route].append(a.elapsed_time(b) / K)
            os.environ.pop("HAVATAR_HAAR_TRAIN", None)
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            disc_rows.append({"discriminator": "Discriminator(%d, 3), B = %d" % (size, B), "iteration": it_name, "unset_ms": round(med["unset"], 3),
                              "unset_ms_min": round(min(ts["unset"]), 3), "set_ms": round(med["set"], 3), "set_ms_min": round(min(ts["set"]), 3)})
        del d, reals, fakes
        torch.cuda.empty_cache()
    print("# (b) eager, %d distinct input sets per round, switch unset / set alternating, %d rounds after 2 warm-up rounds: median (min) ms per iteration" % (K, REPS))
    for r in disc_rows:
        print("%-30s %-24s unset %9.3f (%9.3f) ms | set %9.3f (%9.3f) ms | x%.2f" % (
            r["discriminator"], r["iteration"], r["unset_ms"], r["unset_ms_min"], r["set_ms"], r["set_ms_min"], r["unset_ms"] / r["set_ms"]))
line = json.dumps({"nodes": rows, "discriminator": disc_rows})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""Stage-two joint training: (a) the image-space loss node (native/train_ops.py::Stage2ImageLoss, HAVATAR_S2_LOSS=1) against the ATen
statement it replaces, forward and forward + backward, at 32 -> 128 and 128 -> 512 (B = 2, the 67-channel strided render); (b) eager joint
iterations (harness/train_hd.py::joint_step) on a synthetic two-frame dataset at 128 -> 512, B = 2, with R1 (i = 0) and without (i = 1), on the
node and with HAVATAR_S2_LOSS=0, and the share of the iteration spent in each of its five phases.

Method (tools/bench_discriminator.py): (a) every timed launch works on its OWN buffers, K distinct sets covering >= 1 GiB (at most 64 sets);
the K launches of a route are captured back to back in one hipGraph and replayed; the routes alternate round by round in one process; median
and minimum of the time per launch.  (b) runs eagerly, routes alternating round by round after two warm-up rounds (MIOpen's search); the
phases are cut by events recorded at joint_step's probe points, read after the iteration's one synchronisation.
Usage: python tools/bench_train_hd.py [--out FILE] [--node-only | --step-only] [--rounds N]"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from havatar_amd import synth
from havatar_amd.native import train_ops

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
FOOTPRINT = 1 << 30
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 9
os.environ.pop("HAVATAR_S2_LOSS", None)
SIZES = [(2, 67, 32, 128), (2, 67, 128, 512)]


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


node_rows = []
for B, Cc, r, G in ([] if "--step-only" in sys.argv else SIZES):
    by = 4 * (B * Cc * r * r + 2 * B * r * r + 3 * B * 3 * G * G)
    sets = {}

    def bufs(i):
        if i not in sets:
            sets[i] = (torch.rand(B, r, r, Cc, device=dev, requires_grad=True), torch.rand(B, r, r, 1, device=dev).mul_(0.9).add_(0.05).requires_grad_(True),
                       torch.rand(B, 3, G, G, device=dev), torch.rand(B, 3, G, G, device=dev, requires_grad=True), torch.rand(B, 3, G, G, device=dev),
                       torch.rand(B, 1, r, r, device=dev))
        return sets[i]

    def mk(native, bwd):
        def make(i):
            base, m, gt_lr, fake, gt_hr, gt_mask = bufs(i)

            def fwd():
                o = train_ops.stage2_image_loss(base.permute(0, 3, 1, 2), m.permute(0, 3, 1, 2), gt_lr, fake, gt_hr, gt_mask, "mse", native=native)
                return o[0] + o[1] + 0.01 * o[2], o[3], o[4]
            if bwd:
                return lambda: torch.autograd.grad(fwd()[0], (base, m, fake))
            return lambda: [t.detach() for t in fwd()]
        return make

    for op, bwd in (("forward", False), ("forward + backward", True)):
        gs = {"node": graphed(mk(True, bwd), by), "statement": graphed(mk(False, bwd), by)}
        res = alternate(gs)
        node_rows.append({"shape": [B, Cc, r, G], "op": op, "K": gs["node"][1], "node_us": round(res["node"][0], 1), "node_us_min": round(res["node"][1], 1),
                          "statement_us": round(res["statement"][0], 1), "statement_us_min": round(res["statement"][1], 1)})
        del gs
    sets.clear()
    torch.cuda.empty_cache()
if node_rows:
    print("# (a) per call, K calls on K distinct buffer sets replayed as one hipGraph, routes alternating, %d rounds: median (min) us" % REPS)
for row in node_rows:
    print("%-14s %-19s node %8.1f (%8.1f) us | statement %8.1f (%8.1f) us | x%.2f  (K=%d)" % (
        "x".join(map(str, row["shape"])), row["op"], row["node_us"], row["node_us_min"], row["statement_us"], row["statement_us_min"],
        row["statement_us"] / row["node_us"], row["K"]))

step_rows = []
if "--node-only" not in sys.argv:
    from havatar_amd.harness import stage2_step_cases, train_hd
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.model.styleUnet import Discriminator, SWGAN_unet
    from havatar_amd.utils import styleUnet_util as su
    from havatar_amd.utils.cfgnode import CfgNode
    root = tempfile.mkdtemp()
    split = synth.write_dataset(root, n_frames=2, img_res=512)
    cfg = CfgNode(synth.harness_config(render_size=128, gen_size=512, img_res=512))
    su_args = su.styleUnet_args()
    from havatar_amd.dataloader.dataloaderSR import Loader
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
    CUTS = ("render_nograd", "d_step", "r1_step", "g_forward", "ema")

    def iteration(i):
        ev = {"start": torch.cuda.Event(enable_timing=True)}
        ev["start"].record()

        def probe(name):
            if name in CUTS:
                ev[name] = torch.cuda.Event(enable_timing=True)
                ev[name].record()
        train_hd.joint_step(i, batch, nets, optims, cfg, su_args, None, probe=probe)
        torch.cuda.synchronize()
        t, prev, out = 0.0, "start", {}
        for name, phase in zip(CUTS, train_hd.PHASES):
            out[phase] = ev[prev].elapsed_time(ev[name])
            prev = name
        out["total"] = ev["start"].elapsed_time(ev["ema"])
        return out

    print("# (b) eager joint iteration, 128 -> 512, B = 2, the node and HAVATAR_S2_LOSS=0 alternating, %d rounds after 2 warm-up rounds: median (min) ms; phases: median ms (share)" % REPS,
          flush=True)
    for i, label in ((1, "without R1 (i = 1)"), (0, "with R1 (i = 0)")):
        ts = {"node": [], "0": []}
        for rnd in range(2 + REPS):
            for route in ("node", "0"):          # the default (the node) and HAVATAR_S2_LOSS=0 (the statement)
                os.environ.pop("HAVATAR_S2_LOSS", None)
                if route == "0":
                    os.environ["HAVATAR_S2_LOSS"] = "0"
                res = iteration(i)
                print("%s round %d %s: %.3f ms" % (label, rnd, route, res["total"]), file=sys.stderr, flush=True)
                if rnd >= 2:
                    ts[route].append(res)
        os.environ.pop("HAVATAR_S2_LOSS", None)
        for route in ("node", "0"):
            med = {k: sorted(x[k] for x in ts[route])[len(ts[route]) // 2] for k in ts[route][0]}
            step_rows.append({"iteration": label, "HAVATAR_S2_LOSS": route, "ms": round(med["total"], 3), "ms_min": round(min(x["total"] for x in ts[route]), 3),
                              "phase_ms": {k: round(med[k], 3) for k in train_hd.PHASES}})
            row = step_rows[-1]
            print("%-20s HAVATAR_S2_LOSS %-5s %9.3f (%9.3f) ms | %s" % (row["iteration"], row["HAVATAR_S2_LOSS"], row["ms"], row["ms_min"], "  ".join(
                "%s %.2f (%.0f%%)" % (k, v, 100 * v / max(row["ms"], 1e-9)) for k, v in row["phase_ms"].items())), flush=True)
line = json.dumps({"node": node_rows, "step": step_rows})
print(line)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write(line + "\n")

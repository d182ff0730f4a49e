#!/usr/bin/env python3
"""The stage-one optimisation step of tools/bench_train.py (B = 2 frames x 4 096 rays, jittered depths, density noise) at sample counts
above what hav_composite_* holds: 64+48 (passes of 64 and 80 samples) and 128+64 (128 and 128), with HAVATAR_COMPOSITE_LONG=1 (the
native route, hav_composite_long_* on the passes above 64) and with it unset (the ATen statement of the whole march).

Every measurement is a fresh child process (the switch is read at the call, but the two routes leave different solver caches and
allocator states behind); the children run one after the other, switch set and unset alternating, ROUNDS rounds, in one call.  A child
times the step eagerly (forward + backward + optimiser update) and then, on the native route, as one hipGraph launch
(harness/train.py::StepRunner, the default of the training harness); the ATen statement of the march is timed eagerly only.
Usage: python tools/bench_train_long.py [--out FILE]          (child: --child NUM_COARSE NUM_FINE)"""
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = [(64, 48), (128, 64)]
ROUNDS = 2
STEPS = 8


def child(num_coarse, num_fine):
    import tempfile

    import numpy as np
    import torch

    from havatar_amd import synth
    from havatar_amd.dataloader.dataloader import Loader
    from havatar_amd.harness import train
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode

    dev = torch.device("cuda:0")
    split = synth.write_dataset(tempfile.mkdtemp(), n_frames=2, img_res=512)
    cfgd = synth.harness_config(render_size=128, gen_size=512, img_res=512, perturb=True, noise_std=0.1, rays=4096)
    cfgd["experiment"]["patch_rgb"] = True            # 64x64 patch = 4096 rays per frame, as the reference trains
    cfgd["nerf"]["train"].update(num_coarse=num_coarse, num_fine=num_fine)
    cfg = CfgNode(cfgd)
    torch.backends.cudnn.benchmark = True
    out = {"num_coarse": num_coarse, "num_fine": num_fine, "switch": os.environ.get("HAVATAR_COMPOSITE_LONG", "0")}

    def measure(graph):
        np.random.seed(0); torch.manual_seed(0)
        tl = Loader(split_file=split, mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg, white_bg=True,
                    shuffle=False)
        idx, batch = next(iter(tl))
        trainer = synth.fill_state_dict(Trainer(cfg, len(tl.dataset))).to(dev).train()
        opt = train.make_optimizer(cfg, trainer, graph)
        inp, target, mask = train.step_inputs(idx, batch, dev)
        runner = train.StepRunner(trainer, cfg, opt, torch.nn.functional.mse_loss, graph=graph)
        for _ in range(4):
            loss = runner(inp, target, mask)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            loss = runner(inp, target, mask)[0]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3, float(loss)

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out["eager_ms"], out["loss"] = measure(False)
        # the ATen statement of the march reads host tensors and is not captured (harness/train.py::graph_training_enabled leaves it eager
        # under HAVATAR_HIP_TRAIN=0 for the same reason): only the native route is also timed as one graph launch
        out["graph_ms"] = measure(True)[0] if out["switch"] == "1" else None
    print("RESULT " + json.dumps(out), flush=True)


def main():
    rows = []
    for _ in range(ROUNDS):
        for nc, nf in CONFIGS:
            for switch in ("1", "0"):
                env = dict(os.environ, HAVATAR_COMPOSITE_LONG=switch, HAVATAR_TRAIN_GRAPH="1")
                env.pop("HAVATAR_HIP_TRAIN", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(nc), str(nf)], env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.STDOUT, text=True, timeout=600)
                got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not got:
                    # a child that died says why and ends the run: nothing further is started on the device
                    print(r.stdout[-3000:])
                    raise SystemExit("child %d+%d switch %s failed with status %d" % (nc, nf, switch, r.returncode))
                rows.append(json.loads(got[-1][7:]))
                d = rows[-1]
                print("%3d+%-3d HAVATAR_COMPOSITE_LONG=%s  eager %8.2f ms | one hipGraph launch %s   loss %.5f" % (
                    nc, nf, switch, d["eager_ms"], "%8.2f ms" % d["graph_ms"] if d["graph_ms"] is not None else "   (eager only)",
                    d["loss"]), flush=True)
    for nc, nf in CONFIGS:
        sel = lambda sw, key: [r[key] for r in rows if (r["num_coarse"], r["num_fine"], r["switch"]) == (nc, nf, sw) and r[key] is not None]
        off = min(sel("0", "eager_ms"))
        for key in ("eager_ms", "graph_ms"):
            a = min(sel("1", key))
            print("# %d+%d: switch set (%s) %.2f ms, unset (eager) %.2f ms: %+.1f %%" % (nc, nf, key[:-3], a, off, (a - off) / off * 100))
    line = json.dumps({"rows": rows})
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    else:
        main()

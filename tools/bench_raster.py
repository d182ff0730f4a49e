#!/usr/bin/env python3
"""Condition images from a tracked mesh (havatar_amd/conditions.py): the kernels of csrc/hav_raster.hip per frame (3 views, 256^2) on sphere
tessellations of F ~ 2 k, 20 k and 70 k triangles, B = 1 and 4, against
  (a) the ATen statement of the same definition on the device, at the sizes it can hold in a few seconds (F ~ 2 k, B = 1), and
  (b) the condition path it replaces, per frame: six PNG reads, make_render_cond_ and the host-to-device copy of the three [256,256,7] tensors,
and avatarHD_reenactment.py end to end on a synthetic set with and without --cond-mesh, two repeats each.
  native, launches    hav_raster_ortho_f32 on outputs and workspaces allocated once (cond only, as the frame loop needs), called back to back
  native, in a graph  the same calls captured into one hipGraph and replayed: the three kernels' time
  native, whole call  conditions.render_conditions: allocation of the six outputs and the workspaces + the launches
  face only, graph    the call with `face` as its only output, captured: what the planes' stores add is the difference to the line above
Method (tools/bench_metrics.py): routes alternate round by round in one process; two warm-up rounds are discarded, the median (and minimum) of
the rounds after them is taken; HIP events around `--calls` back-to-back calls of a route, divided by their number.
Usage: python tools/bench_raster.py [--out FILE] [--rounds N] [--calls K] [--no-cli]"""
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from havatar_amd import conditions as cd
from havatar_amd import synth
from havatar_amd.native import raster_ops

dev = torch.device("cuda:0")
REPS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
CALLS = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 20
RES = 256


def sphere(F):
    """a UV sphere of about F triangles filling most of the reference's box; (verts [V,3], colors [V,3], tris [F,3]) numpy"""
    n_lat = int(round(math.sqrt(F / 2.0))) + 1
    n_lon = max(3, -(-F // (2 * (n_lat - 1))))
    th = np.linspace(0.0, math.pi, n_lat + 1)[1:-1]
    ph = np.arange(n_lon) * (2.0 * math.pi / n_lon) + 0.1234
    ring = np.stack([np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon)), np.outer(np.sin(th), np.cos(ph))], -1).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]], 0)
    last, tris = 1 + (n_lat - 1) * n_lon, []
    for j in range(n_lon):
        jn = (j + 1) % n_lon
        tris += [(0, 1 + j, 1 + jn), (last, 1 + (n_lat - 2) * n_lon + jn, 1 + (n_lat - 2) * n_lon + j)]
        for i in range(n_lat - 2):
            a, b, c, d = 1 + i * n_lon + j, 1 + i * n_lon + jn, 1 + (i + 1) * n_lon + j, 1 + (i + 1) * n_lon + jn
            tris += [(a, c, d), (a, d, b)]
    verts = unit * np.array([1.1, 1.3, 1.2]) + np.array([0.0, -0.1, -0.2])
    return verts.astype(np.float32), (125.0 + 100.0 * unit).astype(np.float32), np.asarray(tris, np.int32)


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


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    return g


def kernels(lines):
    th, tw, big = raster_ops.params()
    lines.append("Rasteriser on %s, torch %s; tile %d x %d, wave walk above %d box pixels; %d^2, 3 views; %d rounds after 2 warm-up rounds, %d calls "
                 "per round; ms per call (= per B frames), median (minimum)" % (torch.cuda.get_device_name(0), torch.__version__, th, tw, big, RES,
                                                                                 REPS, CALLS))
    for F in (2000, 20000, 70000):
        vs, col, tris = sphere(F)
        for B in (1, 4):
            v = torch.from_numpy(np.stack([vs * (1 - 0.02 * b) for b in range(B)])).to(dev)
            c, t = torch.from_numpy(col).to(dev), torch.from_numpy(tris).to(dev)
            keys, screen = raster_ops.workspaces(B, v.shape[1], RES, dev)
            cond = {"cond": torch.empty(B, 3, 7, RES, RES, device=dev)}
            face = {"face": torch.empty(B, 3, RES, RES, dtype=torch.int32, device=dev)}
            args = (keys, screen, v, c, t, RES, cd.ORTHO_ROTS, cd.ORTHO_BOUNDS, 10.0)
            with torch.no_grad():
                routes = {"native, launches": (CALLS, lambda: raster_ops.raster_into(cond, *args), 1),
                          "native, in a graph": (1, graph_of(lambda: raster_ops.raster_into(cond, *args)).replay, CALLS),
                          "  face only, graph": (1, graph_of(lambda: raster_ops.raster_into(face, *args)).replay, CALLS),
                          "native, whole call": (CALLS, lambda: cd.render_conditions(v, c, t), 1)}
                if F <= 2000 and B == 1:
                    routes["ATen statement"] = (1, lambda: cd.conditions_statement(v, c, t), 1)
                r = rounds(routes)
                got = cd.render_conditions(v, c, t)
            hits = int((got.face >= 0).sum())
            lines.append("F = %d (V = %d), B = %d: %d covered pixels of %d" % (len(tris), v.shape[1], B, hits, got.face.numel()))
            for k, (med, lo) in r.items():
                lines.append("    %-20s %9.4f (%9.4f)" % (k, med, lo))
            g = r["native, in a graph"][0]
            lines.append("    per frame in a graph: %.4f ms; %.1f M triangle-views/s; cond planes written at %.3f TB/s"
                         % (g / B, B * 3 * len(tris) / (g * 1e-3) / 1e6, B * 3 * 7 * RES * RES * 4 / (g * 1e-3) / 1e12)
                         + ("; statement / native whole call = %.0f" % (r["ATen statement"][0] / r["native, whole call"][0]) if "ATen statement" in r
                            else ""))
            print("\n".join(lines[-(3 + len(r)):]), flush=True)


def png_path(lines, tmp):
    """(b): what the frame loop does per frame today for its conditions"""
    from havatar_amd.dataloader._base import COND_VIEWS, make_render_cond_
    split = synth.write_dataset(os.path.join(tmp, "png"), n_frames=1, img_res=128, photos=False, cond_mesh=True)
    inst = json.load(open(split))["frames"][0]["inst_dir"]

    def read():
        return [make_render_cond_(os.path.join(inst, cd.png_names(v)[1]), os.path.join(inst, cd.png_names(v)[0]), 256) for v in COND_VIEWS]

    def copy(ts):
        out = [t.to(dev, non_blocking=True).permute(2, 0, 1) for t in ts]
        torch.cuda.synchronize()
        return out
    pinned = [t.pin_memory() for t in read()]
    t_read, t_copy = [], []
    for rnd in range(2 + REPS):
        t0 = time.perf_counter()
        ts = read()
        t1 = time.perf_counter()
        copy(pinned)
        t2 = time.perf_counter()
        if rnd >= 2:
            t_read.append(1e3 * (t1 - t0))
            t_copy.append(1e3 * (t2 - t1))
    lines.append("The PNG condition path per frame (one host thread; the loader's workers overlap it with the GPU): six PNG reads + make_render_cond_ "
                 "%.3f ms (%.3f), host-to-device copy of 3 x [256,256,7] float32 from pinned memory %.3f ms (%.3f); mesh mode ships %d bytes of vertices "
                 "and colours instead of %d" % (float(np.median(t_read)), min(t_read), float(np.median(t_copy)), min(t_copy),
                                                2 * synth.head_mesh(0)[0].nbytes, 3 * 256 * 256 * 7 * 4))
    print(lines[-1], flush=True)


def cli(lines, tmp, n_frames=24):
    import yaml

    import metrics_util as mu
    from havatar_amd.harness import reenact
    root = os.path.join(tmp, "cli")
    split = synth.write_dataset(root, n_frames=n_frames, img_res=128, photos=False, cond_mesh=True)
    cfg_path, ckpt = os.path.join(tmp, "cfg.yml"), mu.checkpoint(os.path.join(tmp, "avatar.pth"))
    with open(cfg_path, "w") as f:
        yaml.safe_dump(synth.harness_config(), f)
    rates = {"PNG": [], "--cond-mesh": []}
    for rep in range(2):
        for name, extra in (("PNG", []), ("--cond-mesh", ["--cond-mesh", os.path.join(root, "tri.npy")])):
            t0 = time.perf_counter()
            reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", os.path.join(tmp, "out_%s_%d" % (name.strip("-"), rep)),
                          "--split", split] + extra, device=dev)
            rates[name].append(n_frames / (time.perf_counter() - t0))
    lines.append("avatarHD_reenactment.py, %d synthetic frames (32^2 render, 128^2 output, %d-triangle head), whole runs incl. model load and graph "
                 "capture, frames/s, two repeats: PNG %.2f, %.2f; --cond-mesh %.2f, %.2f" % (n_frames, len(synth.head_mesh(0)[2]), *rates["PNG"],
                                                                                              *rates["--cond-mesh"]))
    spread = abs(rates["--cond-mesh"][0] - rates["--cond-mesh"][1])
    slower = float(np.mean(rates["PNG"])) - float(np.mean(rates["--cond-mesh"]))
    lines.append("    --cond-mesh is %s than the PNG loop by %.2f frames/s; the spread of its own two repeats is %.2f"
                 % ("SLOWER" if slower > 0 else "faster", abs(slower), spread))
    print("\n".join(lines[-2:]), flush=True)


def main():
    lines = []
    kernels(lines)
    with tempfile.TemporaryDirectory() as tmp:
        png_path(lines, tmp)
        if "--no-cli" not in sys.argv:
            cli(lines, tmp)
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""H1 -- reenactment harness (reference: avatarHD_reenactment.py:103-172).

    python avatarHD_reenactment.py --config <yml> --ckpt <pth> --savedir <dir> --split <split.json>

Same flags, same checkpoint keys (`nerf_render`, `latent_codes`, `g_ema`), same per-frame sequence:
test-mode frame (B=1) -> `Trainer(**inp)` (validation mode, full image) -> `SWGAN_unet(styles=[style], condition_img=render[:, 3:])`
-> clip(x*255, 0, 255) uint8 -> `<savedir>/rgb/<fidx>_<view:02d>.png`.
What is different by design: the frame is one hipGraph launch per stage when shapes are static (HAVATAR_GRAPH=0 disables), and
with more than one process (torchrun) the frames of the split are dealt round-robin to the ranks (no data-path collective).
Throughput mode: HAVATAR_FRAME_BATCH=B (default 1 = the reference's sequence) renders B of this rank's frames per call -- the encoders
and the upsampler see a batch, the march takes B x R rays in one launch; files and pixels are those of the one-frame loop (frames of a batch
differ from the same frames rendered alone by the encoders' rounding, 1e-4 on the render; a ragged last batch is rendered at its own size).
"""
import argparse
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import yaml

from . import per_rank_miopen_cache
from .. import switches
from ..dataloader import imgio
from ..dataloader.dataloaderSR import Loader
from ..frames import shard_frames
from ..graph import GraphedForward
from ..model.nerf_trainer import Trainer
from ..model.styleUnet import SWGAN_unet
from ..utils.cfgnode import CfgNode
from ..utils.training_util import load_partial_state_dict


class styleUnet_args:
    """The generator hyper-parameters the reference hard-codes in the script (avatarHD_reenactment.py:17-45); only the three the
    inference path reads are kept."""
    latent = 64
    n_mlp = 4
    channel_multiplier = 2


su_args = styleUnet_args()


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", type=str, default="config/singleview_512_HD_base.yml", help="Path to (.yml) config file.")
    p.add_argument("--ckpt", type=str, default="", help="Path to load saved checkpoint from.")
    p.add_argument("--savedir", type=str, default="./renders/", help="Save images to this directory, if specified.")
    p.add_argument("--split", type=str, default=None, help="Split file (json) listing the frames to render.")
    p.add_argument("--metrics", action="store_true", help="Score every frame against the split's photograph (PSNR, SSIM, LPIPS with both "
                   "--percep paths) and write <savedir>/metrics.json.")
    p.add_argument("--percep-vgg", type=str, default="", help="--metrics: torchvision VGG16 weights for LPIPS.")
    p.add_argument("--percep-lin", type=str, default="", help="--metrics: lpips linear-layer weights for LPIPS.")
    p.add_argument("--mesh", action="store_true", help="Extract every frame's density iso-surface (havatar_amd.geometry) and write "
                   "<savedir>/mesh/<fidx>_<view>.ply with normals and vertex colours.")
    p.add_argument("--mesh-res", type=int, default=128, help="--mesh: lattice points per axis.")
    p.add_argument("--mesh-iso", type=float, default=None, help="--mesh: density level of the surface (default: geometry.DEFAULT_ISO).")
    p.add_argument("--mesh-space", choices=("canonical", "posed"), default="canonical", help="--mesh: the canonical box (pose-free) or the "
                   "frame's posed box.")
    p.add_argument("--gbuffer", action="store_true", help="Write every frame's geometry as images at the render size (havatar_amd.geometry."
                   "gbuffer): <savedir>/depth/<fidx>_<view>.png (16-bit), normal/ (RGB8), shade/ (grey8), and <savedir>/gbuffer.json with "
                   "near, far and the codes' definition.")
    p.add_argument("--gbuffer-acc-min", type=float, default=0.5, help="--gbuffer: a pixel shows a surface where the accumulated opacity "
                   "exceeds this.")
    p.add_argument("--cond-mesh", type=str, default="", metavar="TRI.npy", help="Mesh mode: drive the avatar with every frame's tracked mesh "
                   "(<inst_dir>/cond_mesh.npz: vs [V,3], color [V,3]) and this integer [F,3] topology; the three condition renders are "
                   "rasterised per frame (havatar_amd.conditions.render_conditions) instead of being read from the six PNGs.")
    p.add_argument("--cond-cam-dist", type=float, default=10.0, help="--cond-mesh: distance of the orthographic camera.")
    p.add_argument("--cond-write", action="store_true", help="--cond-mesh: also write the six condition PNGs into each frame's inst_dir.")
    return p.parse_args(argv)


def build_models(cfg, checkpoint, device):
    render_size, gen_size = cfg.models.StyleUnet.inp_size, cfg.models.StyleUnet.out_size
    nerf_render = Trainer(cfg, 0).requires_grad_(False).to(device)
    img_trans = SWGAN_unet(inp_size=render_size, inp_ch=cfg.models.StyleUnet.inp_ch, out_size=gen_size, out_ch=3,
                           style_dim=su_args.latent, c_dim=0, n_mlp=su_args.n_mlp,
                           channel_multiplier=su_args.channel_multiplier).to(device)
    load_partial_state_dict(nerf_render, checkpoint["nerf_render"], except_keys=["latent_codes"])
    nerf_render.latent_codes = checkpoint["latent_codes"].to(device)
    img_trans.load_state_dict(checkpoint["g_ema"])
    nerf_render.headpose_skin_net.fix_canonical_W()
    return nerf_render.eval(), img_trans.eval()


def frame_conditions(batch, device, mesh):
    """--cond-mesh: the frame's Conditions from its tracked vertices, on the frame's device.  mesh = (Topology, cam_dist)"""
    from .. import conditions
    topo, cam_dist = mesh
    return conditions.render_conditions(batch["cond_vs"].to(device, non_blocking=True), batch["cond_color"].to(device, non_blocking=True), topo,
                                        cam_dist=cam_dist)


def frame_inputs(idx, batch, device, size=None, cache=None, mesh=None):
    """The dict the reference builds per frame (:151-159).  With a `camera` record in the batch (device-ray mode) the ray table is
    generated on the device (hav_gen_rays) and the white background prior is a cached constant.  With `mesh` (--cond-mesh) the three
    condition tensors are rasterised from the frame's tracked mesh, eagerly, and the Conditions is left in cache["conditions"]."""
    if "camera" in batch:
        from ..render import gen_rays
        n = batch["camera"].shape[0]
        cache = cache if cache is not None else {}
        if ("rays", n) not in cache:
            cache[("rays", n)] = torch.empty(n, size * size, 8, device=device)
            cache[("bg", n)] = torch.ones(n, size * size, 3, device=device)
        for b in range(n):
            cam = batch["camera"][b]
            gen_rays(size, size, cam[0:4], cam[4:16], float(cam[16]), float(cam[17]), device, out=cache[("rays", n)][b:b + 1])
        ray_batch, bg = cache[("rays", n)], cache[("bg", n)]
    else:
        rays = batch["mv_rays"]
        ray_batch, bg = rays[..., :-3].to(device), rays[..., -3:].to(device)
    if mesh is not None:
        out = frame_conditions(batch, device, mesh)
        if cache is not None:
            cache["conditions"] = out
        # the kernel wrote [n,3,7,H,W]; nothing crosses PCIe but the vertices.  The PNG route hands over channels-last views of [n,H,W,7]:
        # the same strides here (one device copy of 0.46 MB per view), so that both routes hand the encoders identical tensors, strides
        # included, and a convolution that picks its kernel by memory format picks the same one
        view = lambda k: out.cond[:, k].contiguous(memory_format=torch.channels_last)
        return {"mode": "validation", "fidx": idx, "render_full_img": True, "ray_batch": ray_batch, "background_prior": bg,
                "front_render_cond": view(0), "left_render_cond": view(1), "right_render_cond": view(2),
                "inv_head_T": batch["inv_head_T"].to(device)}
    return {"mode": "validation", "fidx": idx, "render_full_img": True,
            "ray_batch": ray_batch, "background_prior": bg,
            # channels-last host images go over PCIe as they are (contiguous, pinned by the loader); the NHWC -> NCHW permutation
            # happens on the device (a strided host-side copy of 3 x 1.8 MB costs more than the frame's GPU work at 128^2)
            "front_render_cond": batch["front_render_cond"].to(device, non_blocking=True).permute(0, 3, 1, 2),
            "left_render_cond": batch["left_render_cond"].to(device, non_blocking=True).permute(0, 3, 1, 2),
            "right_render_cond": batch["right_render_cond"].to(device, non_blocking=True).permute(0, 3, 1, 2),
            "inv_head_T": batch["inv_head_T"].to(device)}


def to_png_array(gen_img):
    """[1,3,H,W] float -> uint8 [H,W,3] RGB exactly as :164 (x*255 in float32, clip, truncating cast) -- done on the device, so
    0.75 MB instead of 3 MB cross PCIe per 512^2 frame."""
    return (gen_img[0].permute(1, 2, 0) * 255).clamp_(0, 255).to(torch.uint8).cpu().numpy()


class FrameScores:
    """--metrics: the scores of this rank's frames in a buffer on the frames' device, [n, 3] float64 = (ssim, mse, lpips).  add() enqueues work
    on the current stream and reads nothing back; write() reads the buffer once, after the last frame."""

    def __init__(self, n, device, percep):
        self.buf = torch.zeros(max(n, 1), 3, dtype=torch.float64, device=device)
        self.percep, self.rows = percep, []

    def add(self, path, fidx, view, pred_u8, gt_u8):
        """pred_u8, gt_u8 [H,W,3] uint8 on the buffer's device: the image as it is written, and the photograph"""
        from .. import metrics
        i = len(self.rows)
        self.rows.append({"file": os.path.join("rgb", os.path.basename(path)), "fidx": fidx, "view": view})
        self.buf[i, :2].copy_(metrics.ssim_mse(pred_u8[None], gt_u8[None])[0])
        if self.percep is not None:
            a, b = (t.permute(2, 0, 1)[None].float() / 127.5 - 1.0 for t in (pred_u8, gt_u8))
            self.buf[i, 2].copy_(self.percep(a, b).reshape(()))

    def write(self, savedir, rank, world):
        from .. import metrics
        vals = self.buf.cpu().numpy()
        for row, v in zip(self.rows, vals):
            row.update(ssim=float(v[0]), mse=float(v[1]), lpips=float(v[2]) if self.percep is not None else None)
        note = "LPIPS-VGG on uint8 / 127.5 - 1" if self.percep is not None else "not evaluated: needs --percep-vgg and --percep-lin"
        path = os.path.join(savedir, "metrics.json" if world == 1 else "metrics_rank%dof%d.json" % (rank, world))
        with open(path, "w") as f:
            json.dump(metrics.table(self.rows, lpips_note=note), f, indent=1)
        return path


def check_metric_sizes(cfg, split):
    """--metrics compares the written image with the photograph pixel by pixel: refuse before anything is rendered when the two differ in size"""
    with open(split) as f:
        img_res = json.load(f)["img_res"]
    out_size = cfg.models.StyleUnet.out_size
    if out_size != img_res:
        raise RuntimeError("--metrics: StyleUnet.out_size %d differs from the split's img_res %d: the frames cannot be scored against its "
                           "photographs" % (out_size, img_res))


def frame_mesh(nerf_render, inv_head_T, bidx, args):
    """--mesh: the mesh of sample bidx of the frames just rendered (their planes are still the trainer's current ones; extraction only reads),
    as host arrays for write_ply"""
    from .. import geometry
    iso = geometry.DEFAULT_ISO if args.mesh_iso is None else args.mesh_iso
    mesh = geometry.extract_mesh(nerf_render, inv_head_T, res=args.mesh_res, iso=iso, space=args.mesh_space, colors=True, bidx=bidx)
    return [t.cpu().numpy() for t in mesh]


def frame_gbuffer(inp, outs, n, args):
    """--gbuffer: the maps of the n frames just rendered, from the ray table the march read and the depth and accumulation it returned, on the
    current stream after the frame; (depth16 [n,S,S,2], normal8 [n,S,S,3], shade8 [n,S,S]) as host arrays for the PNG writers"""
    from .. import geometry
    S = outs[0].shape[-1]
    gb = geometry.gbuffer(inp["ray_batch"], outs[3].reshape(n, S * S), outs[1].reshape(n, S * S), S, S, args.gbuffer_acc_min)
    return [t.cpu().numpy() for t in (gb.depth16, gb.normal8, gb.shade8)]


def write_gbuffer_table(savedir, rank, world, args, near, far, size, files):
    from ..geometry import DEPTH16_CODE
    path = os.path.join(savedir, "gbuffer.json" if world == 1 else "gbuffer_rank%dof%d.json" % (rank, world))
    with open(path, "w") as f:
        json.dump({"near": near, "far": far, "acc_min": args.gbuffer_acc_min, "size": size,
                   "depth": "16-bit grey, metres along the ray: " + DEPTH16_CODE,
                   "normal": "RGB8 = round((n * 0.5 + 0.5) * 255), n the unit normal facing the camera in the frame's posed world space; "
                             "(0,0,0) = no normal",
                   "shade": "grey8 = round(255 * max(0, -n . d)), d the pixel's ray direction; 255 = no normal",
                   "files": files}, f, indent=1)
    return path


def main(argv=None, device=None, style=None):
    """Returns the PNG paths; main.mesh_written lists the PLY paths of the last call (empty without --mesh), main.gbuffer_written the
    depth / normal / shade PNG paths (empty without --gbuffer), main.cond_written the condition PNG paths (empty without --cond-write)."""
    args = parse_args(argv)
    main.mesh_written = []
    main.gbuffer_written = []
    main.cond_written = []
    if args.cond_write and not args.cond_mesh:
        raise RuntimeError("--cond-write writes the condition PNGs rendered from the tracked mesh: it needs --cond-mesh TRI.npy")
    if args.cond_mesh and not np.isfinite(args.cond_cam_dist):
        raise RuntimeError("--cond-cam-dist %r: the distance must be finite" % args.cond_cam_dist)
    if args.gbuffer:
        if not np.isfinite(args.gbuffer_acc_min):
            raise RuntimeError("--gbuffer-acc-min %r: the threshold must be finite" % args.gbuffer_acc_min)
        for sub in ("depth", "normal", "shade"):
            os.makedirs(os.path.join(args.savedir, sub), exist_ok=True)
    os.makedirs(os.path.join(args.savedir, "rgb"), exist_ok=True)
    if args.mesh:
        if args.mesh_res < 2:
            raise RuntimeError("--mesh-res %d: the lattice needs at least 2 points per axis" % args.mesh_res)
        os.makedirs(os.path.join(args.savedir, "mesh"), exist_ok=True)
    with open(args.config, "r") as f:
        cfg = CfgNode(yaml.load(f, Loader=yaml.FullLoader))
    if args.metrics:
        check_metric_sizes(cfg, args.split)
        if bool(args.percep_vgg) != bool(args.percep_lin):
            raise RuntimeError("--metrics: LPIPS needs both --percep-vgg PATH (torchvision VGG16 weights) and --percep-lin PATH (lpips linear "
                               "layers); pass both, or neither for PSNR and SSIM only")
    seed = cfg.experiment.randomseed
    np.random.seed(seed)
    torch.manual_seed(seed)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    per_rank_miopen_cache()
    if device is None:
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))       # the reference is GPU-only as well (:133)
    device = torch.device(device)
    if device.type == "cuda":
        device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        torch.cuda.set_device(device)
    print(args.ckpt)
    checkpoint = torch.load(args.ckpt, map_location="cpu")
    nerf_render, img_trans = build_models(cfg, checkpoint, device)
    if style is None:
        style = torch.mean(torch.randn(1000, 1, su_args.latent), dim=0)            # :147, after the constructors consumed the RNG
    style = style.to(device)
    val_loader = Loader(split_file=args.split, mode="test", batch_size=1, options=cfg, down_sample=cfg.dataset.down_sample)
    mine = list(shard_frames(len(val_loader.dataset), rank, world))
    # HIP: the loader ships 18 camera floats per frame and the ray table is built on the device
    val_loader.dataset.device_rays = device.type == "cuda" and switches.on("HAVATAR_DEVICE_RAYS")
    ray_cache = {}
    cond_mesh = None
    if args.cond_mesh:
        from .. import conditions
        first = val_loader.dataset.frames[0]["inst_dir"] if len(val_loader.dataset) else None
        V = conditions.read_cond_mesh(first)[0].shape[0] if first is not None else None
        cond_mesh = (conditions.Topology.load(args.cond_mesh, V), args.cond_cam_dist)
        val_loader.dataset.cond_mesh, val_loader.dataset.cond_mesh_verts = True, cond_mesh[0].V
    scores = None
    if args.metrics:
        val_loader.dataset.with_gt = True
        percep = None
        if args.percep_vgg and args.percep_lin:
            from ..model.lpips import build_for_harness
            percep = build_for_harness(args.percep_vgg, args.percep_lin, device)
        else:
            print("[metrics] no --percep-vgg / --percep-lin: LPIPS is omitted, PSNR and SSIM only")
        scores = FrameScores(len(mine), device, percep)
    # this rank's frames only, read ahead by worker processes (the reference reads every frame in the main process)
    fbatch = max(1, switches.integer("HAVATAR_FRAME_BATCH"))
    frames = torch.utils.data.DataLoader(torch.utils.data.Subset(val_loader.dataset, mine), batch_size=fbatch, shuffle=False,
                                         num_workers=switches.integer("HAVATAR_WORKERS", 4), pin_memory=device.type == "cuda")
    use_graph = device.type == "cuda" and switches.on("HAVATAR_GRAPH")
    graphed, graphed2, written = {}, {}, []            # hipGraphs per batch size (the last batch of a split may be ragged)
    writers = ThreadPoolExecutor(max_workers=switches.integer("HAVATAR_PNG_THREADS"))    # PNG deflate off the critical path (a 1024^2 frame is ~70 ms of zlib on one core)
    pending, ring, in_flight = [], [None, None], None
    gb_range = None
    t_first = t_loop = None
    with torch.no_grad():
        for idx, val_batch in frames:
            if t_first is None:
                t_first = time.perf_counter()
            elif t_loop is None:
                t_loop = time.perf_counter()             # steady state starts after the first frame (solver search, graph capture)
            n = int(val_batch["fidx"].shape[0])
            inp = frame_inputs(idx, val_batch, device, size=val_loader.dataset.img_h, cache=ray_cache, mesh=cond_mesh)
            if args.cond_write:
                cond_maps = [t.cpu().numpy() for t in (ray_cache["conditions"].render8, ray_cache["conditions"].normal8)]
            if args.gbuffer:
                inp["return_depth"] = True          # not a tensor: part of the captured callable's fixed arguments below
            styles = [style if n == 1 else style.expand(n, -1)]
            gt_imgs = val_batch["gt_img"].to(device, non_blocking=True) if scores is not None else None
            if use_graph:
                tens = {k_: v for k_, v in inp.items() if torch.is_tensor(v) and k_ != "fidx"}
                if n not in graphed:
                    fixed = {k_: v for k_, v in inp.items() if k_ not in tens}
                    graphed[n] = GraphedForward(lambda fixed=fixed, **kw: nerf_render(**kw, **fixed), tens)
                outs = graphed[n](**tens)
                render = outs[0]
                cond = {"condition_img": render[:, 3:].contiguous()}
                if n not in graphed2:
                    graphed2[n] = GraphedForward(lambda condition_img, styles=styles: img_trans(styles=styles, condition_img=condition_img), cond)
                gen_imgs = graphed2[n](**cond)
            else:
                outs = nerf_render(**inp)
                render = outs[0]
                gen_imgs = img_trans(styles=styles, condition_img=render[:, 3:])
            if args.gbuffer:
                gb_maps = frame_gbuffer(inp, outs, n, args)
                if gb_range is None:
                    gb_range = [float(v) for v in inp["ray_batch"][0, 0, 6:8].cpu()]
            for b in range(n):
                gen_img = gen_imgs[b:b + 1]
                name, k = str(int(val_batch["fidx"][b])), int(val_batch["vidx"][0][b])          # ("vidx" is a one-element list per item: collated to [tensor[n]])
                path = os.path.join(args.savedir, "rgb", f"{name}_{k:02d}.png")
                written.append(path)
                if args.cond_write:
                    from ..conditions import VIEWS, png_names
                    inst = val_loader.dataset.frames[int(idx[b])]["inst_dir"]
                    for v, view in enumerate(VIEWS):
                        for fname, arr in zip(png_names(view), cond_maps):
                            main.cond_written.append(os.path.join(inst, fname))
                            pending.append(writers.submit(imgio.imwrite_rgb, main.cond_written[-1], np.ascontiguousarray(arr[b, v])))
                if args.mesh:
                    from ..geometry import write_ply
                    main.mesh_written.append(os.path.join(args.savedir, "mesh", f"{name}_{k:02d}.ply"))
                    pending.append(writers.submit(write_ply, main.mesh_written[-1], *frame_mesh(nerf_render, inp["inv_head_T"], b, args)))
                if args.gbuffer:
                    for sub, fn, arr in zip(("depth", "normal", "shade"), (imgio.imwrite_gray16, imgio.imwrite_rgb, imgio.imwrite_gray8), gb_maps):
                        main.gbuffer_written.append(os.path.join(args.savedir, sub, f"{name}_{k:02d}.png"))
                        pending.append(writers.submit(fn, main.gbuffer_written[-1], arr[b]))
                if device.type != "cuda":
                    arr = to_png_array(gen_img)
                    if scores is not None:
                        scores.add(path, int(name), k, torch.from_numpy(arr), gt_imgs[b])
                    pending.append(writers.submit(imgio.imwrite_rgb, path, arr))
                    continue
                # two-slot read-back ring: frame n's uint8 image is copied to pinned memory asynchronously and handed to the PNG
                # threads while frame n+1 is being prepared and launched, so the GPU does not idle during host work
                slot = len(written) & 1
                if ring[slot] is None:
                    H2, W2 = gen_img.shape[-2:]
                    ring[slot] = (torch.empty(H2, W2, 3, dtype=torch.uint8, device=device), torch.empty(H2, W2, 3, dtype=torch.uint8).pin_memory(),
                                  torch.cuda.Event())
                dev_u8, host_u8, ev = ring[slot]
                if in_flight is not None and in_flight[1] == slot:                         # (batched frames: the slot's previous image must have left)
                    ring[slot][2].synchronize()
                dev_u8.copy_((gen_img[0].permute(1, 2, 0) * 255).clamp_(0, 255))          # float -> uint8 truncation, as to_png_array
                host_u8.copy_(dev_u8, non_blocking=True)
                ev.record()
                if scores is not None:                                                     # on the device, after the read-back was enqueued
                    scores.add(path, int(name), k, dev_u8, gt_imgs[b])
                if in_flight is not None:                                                  # finish the PREVIOUS frame now
                    p_path, p_slot = in_flight
                    ring[p_slot][2].synchronize()
                    pending.append(writers.submit(imgio.imwrite_rgb, p_path, ring[p_slot][1].numpy().copy()))
                in_flight = (path, slot)
    if in_flight is not None:
        p_path, p_slot = in_flight
        ring[p_slot][2].synchronize()
        pending.append(writers.submit(imgio.imwrite_rgb, p_path, ring[p_slot][1].numpy().copy()))
    for f in pending:
        f.result()
    writers.shutdown()
    if t_loop is not None and len(written) > 1:
        dt = time.perf_counter() - t_loop
        print("[rank %d] %d frames; first frame %.2f s (solver search + graph capture), then %.1f ms per frame end to end "
              "(read, render %dx%d, upsample %dx%d, PNG)" % (rank, len(written), t_loop - t_first, 1e3 * dt / (len(written) - 1),
                                                            nerf_render.render_size, nerf_render.render_size, gen_img.shape[-1], gen_img.shape[-2]))
    if scores is not None:
        print("[metrics] %s" % scores.write(args.savedir, rank, world))
    if args.gbuffer and gb_range is not None:
        print("[gbuffer] %s" % write_gbuffer_table(args.savedir, rank, world, args, gb_range[0], gb_range[1], nerf_render.render_size,
                                                   [os.path.relpath(p, args.savedir) for p in main.gbuffer_written]))
    print("Done!")
    return written


if __name__ == "__main__":
    main()

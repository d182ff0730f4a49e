"""H3 -- stage-two (HD) joint training harness (reference: train_avatarHD.py:79-379).

    python train_avatarHD.py --logdir <dir> --datadir <dir with sv_v31_all.json> --config <yml> --ckpt <ckpt> [--continue-training]

Same flags, optimisers (:117-122), per-iteration statements (:181-303, `joint_step`) and checkpoint keys (:347-357: `iter, nerf_optimizer,
g_optim, d_optim, nerf_render, g, d, g_ema, latent_codes`), both load modes (:137-159).  Added flags: `--gan-ckpt` (the reference hard-codes
pretrained_models/img_translation.ckpt, :144), `--percep {lpips,none}` (LPIPS needs the `lpips` package and its VGG weights; without them the
harness refuses to start unless `none` is given, which drops the 0.1 * LPIPS term and says so; `--percep native --percep-vgg PATH
--percep-lin PATH` takes the term from this package's own module, model/lpips.py, with no `lpips` / torchvision import), `--ssim-weight W`
(adds W * (1 - SSIM(fake, gt)), metrics.ssim_loss; default 0: no such term), `--iters` / `--batch` for short runs.
What is different by design: scalars go to tensorboard only if it is installed (and to stdout every experiment.print_every iterations),
there is no code tarball and no progress bar, the sample image is written through imgio, `latest.pt` is also written after the run's last
iteration, and `--continue-training` continues the iteration count from the checkpoint's `iter` (the reference has that line commented out
and restarts at 0) and, if `<ckpt>.rng` sits next to the checkpoint, the random streams from where they stood.  Eager execution only.
"""
import argparse
import os
import random
import time

import numpy as np
import torch
import torch.nn.functional as F
import yaml

from .. import metrics, switches
from ..dataloader import imgio
from ..dataloader.dataloaderSR import Loader
from ..model.nerf_trainer import Trainer
from ..model.styleUnet import Discriminator, SWGAN_unet
from ..native import train_ops
from ..utils import styleUnet_util
from ..utils.cfgnode import CfgNode
from ..utils.training_util import mse2psnr
from .train import _NullWriter, deterministic_requested, enable_determinism

CKPT_KEYS = ("iter", "nerf_optimizer", "g_optim", "d_optim", "nerf_render", "g", "d", "g_ema", "latent_codes")
PHASES = ("render_nograd", "d_step", "r1_step", "g_forward", "g_backward_step")


def lpips_loss(img0, img1, lpips_fn):
    """[B,3,H,W] in [0,1] -> mean LPIPS (utils/training_util.py:114-121 of the reference)."""
    return lpips_fn.forward(img0 * 2.0 - 1.0, img1 * 2.0 - 1.0).mean()


def gan_loss_weight(i):
    """train_avatarHD.py:205-206"""
    return min(1e-3 * 1.1 ** (i // 500), 0.1)


def step_inputs(batch, device, render_size, gen_size):
    """train_avatarHD.py:186-198: mv_rays [B,r*r,12] = rays(8) | background(3) | mask(1); the ground truth is at the generator's size."""
    fidx, tb = batch
    n = len(fidx)
    gt_hr_img = tb["mv_rays_gt_color"].permute(0, 2, 1).reshape(n, 3, gen_size, gen_size).to(device)
    gt_lr_mask = tb["mv_rays"][..., -1:].permute(0, 2, 1).reshape(n, 1, render_size, render_size).to(device)
    inp = {"mode": "train", "fidx": fidx, "render_full_img": True,
           "ray_batch": tb["mv_rays"][..., :-4].to(device), "background_prior": tb["mv_rays"][..., -4:-1].to(device),
           "front_render_cond": tb["front_render_cond"].permute(0, 3, 1, 2).to(device),
           "left_render_cond": tb["left_render_cond"].permute(0, 3, 1, 2).to(device),
           "right_render_cond": tb["right_render_cond"].permute(0, 3, 1, 2).to(device),
           "inv_head_T": tb["inv_head_T"].to(device)}
    return inp, gt_hr_img, gt_lr_mask


def joint_step(i, batch, nets, optims, cfg, su_args, percep=None, util=None, probe=None, aux=None, ssim_weight=0.0):
    """One iteration of the joint NeRF + GAN training, the reference's statements in the reference's order (train_avatarHD.py:186-303):
      1. no-grad render and fake image (the fused march kernel on HIP tensors)           :211-217
      2. the discriminator's logistic step                                                :219-231
      3. the R1 step when i % d_reg_every == 0, with the `0 * real_pred[0]` term          :233-241
      4. the grad-mode render                                                             :244-245
      5. rgb loss, code loss, mask BCE                                                    :246-254
      6. the generator's forward on render[:, 3:]                                         :257-260
      7. the non-saturating loss through the frozen discriminator, times gan_loss_weight  :262-266
      8. HR L1 (+ 0.1 * LPIPS when `percep` is given; + ssim_weight * (1 - SSIM(fake, gt)), metrics.ssim_loss, when ssim_weight is
         not 0 -- not in the reference)                                                   :268-274
      9. one backward; 10. g_optim.step(), nerf_optimizer.step()                          :276-280
     11. accumulate(g_ema, generator, 0.5 ** (32 / 10000))                                :303
    The path-length block of the reference (:285-301) is dead code there (`if False`) and is not here.  Random numbers are consumed as the
    reference consumes them: mixing_noise twice (Python `random`, then torch.randn on the device), whatever the networks draw in between.
    Steps 5 and 8's image-space terms and the two PSNR mse (:282-283) are one call, native/train_ops.py::stage2_image_loss: the native
    Stage2ImageLoss node on eligible HIP tensors, the ATen statement elsewhere and with HAVATAR_S2_LOSS=0.

    batch = (fidx, dict) of dataloaderSR.Loader(mode="train"); nets = {nerf_render, generator, discriminator, g_ema};
    optims = {nerf_optimizer, g_optim, d_optim}; util: the module with the stage-two helpers (default utils/styleUnet_util);
    probe(name): called after "render_nograd", "d_backward", "d_step", "r1_step", "g_forward", "g_backward", "g_step", "ema" (tests, timing).
    The `r1` scalar is 0 in an iteration without R1 (the reference logs the last R1 iteration's value again).  aux: a dict that receives
    the tensors the validation sample needs (render, gt_hr_img).  Returns a dict of Python floats."""
    util = styleUnet_util if util is None else util
    probe = probe if probe is not None else (lambda name: None)
    nerf_render, generator, discriminator, g_ema = nets["nerf_render"], nets["generator"], nets["discriminator"], nets["g_ema"]
    nerf_optimizer, g_optim, d_optim = optims["nerf_optimizer"], optims["g_optim"], optims["d_optim"]
    device, dtype = next(generator.parameters()).device, next(generator.parameters()).dtype
    render_size, gen_size = cfg.models.StyleUnet.inp_size, cfg.models.StyleUnet.out_size
    inp, gt_hr_img, gt_lr_mask = step_inputs(batch, device, render_size, gen_size)
    batch_num = gt_hr_img.shape[0]
    gt_lr_img = F.interpolate(F.interpolate(gt_hr_img, size=(render_size, render_size), mode="bilinear", align_corners=True),
                              size=(gen_size, gen_size), mode="bilinear", align_corners=True)
    glw = gan_loss_weight(i)
    d_regularize = i % su_args.d_reg_every == 0
    scalars = {}

    # 1-2: discriminator
    util.requires_grad(nerf_render, False)
    util.requires_grad(generator, False)
    util.requires_grad(discriminator, True)
    with torch.no_grad():
        render, _, _ = nerf_render(**inp)
        noise = [z.to(dtype) for z in util.mixing_noise(batch_num, su_args.latent, su_args.mixing, device)]          # (float64 runs of the tests)
        fake_img = generator(noise, render[:, 3:])
    probe("render_nograd")
    fake_pred = discriminator(fake_img, flat_pose=None)
    real_pred = discriminator(gt_hr_img, flat_pose=None)
    d_loss = util.d_logistic_loss(real_pred, fake_pred) * glw
    scalars["d"] = d_loss / glw
    scalars["real_score"] = real_pred.mean()
    scalars["fake_score"] = fake_pred.mean()
    discriminator.zero_grad()
    d_loss.backward()
    probe("d_backward")
    d_optim.step()
    probe("d_step")

    # 3: R1 (the reference turns requires_grad on gt_hr_img itself; a leaf of its own computes the same and leaves the target a constant)
    r1_loss = torch.zeros((), device=device)
    if d_regularize:
        real_img = gt_hr_img.detach().requires_grad_(True)
        real_pred = discriminator(real_img, flat_pose=None)
        r1_loss = util.d_r1_loss(real_pred, real_img) * glw
        discriminator.zero_grad()
        (su_args.r1 / 2 * r1_loss * su_args.d_reg_every + 0 * real_pred[0]).backward()
        d_optim.step()
    scalars["r1"] = r1_loss / glw
    probe("r1_step")

    # 4-8: generator and NeRF
    util.requires_grad(nerf_render, True)
    render, mask, latent_code_loss = nerf_render(**inp)
    util.requires_grad(generator, True)
    noise = [z.to(dtype) for z in util.mixing_noise(batch_num, su_args.latent, su_args.mixing, device)]
    fake_img = generator(noise, render[:, 3:])
    rgb_loss, hr_l1_loss, mask_bce, lr_mse, sr_mse = train_ops.stage2_image_loss(render, mask, gt_lr_img, fake_img, gt_hr_img, gt_lr_mask,
                                                                                 cfg.experiment.rgb_loss)
    nerf_loss = rgb_loss + 1.0 * latent_code_loss
    scalars["rgb_loss"], scalars["code_loss"] = rgb_loss, latent_code_loss
    if cfg.experiment.mask_weight > 0:
        mask_loss = cfg.experiment.mask_weight * mask_bce
        scalars["mask_loss"] = mask_loss
        nerf_loss = nerf_loss + mask_loss
    scalars["nerf_loss"] = nerf_loss
    g_loss = nerf_loss
    util.requires_grad(discriminator, False)
    fake_pred = discriminator(fake_img, flat_pose=None)
    g_nonsat = util.g_nonsaturating_loss(fake_pred)
    g_loss = g_loss + g_nonsat * glw
    scalars["g"] = g_nonsat
    g_loss = g_loss + hr_l1_loss
    scalars["hr_l1"] = hr_l1_loss
    if percep is not None:
        percep_loss = lpips_loss(fake_img, gt_hr_img, percep)
        g_loss = g_loss + percep_loss * 0.1
        scalars["percep_loss"] = percep_loss
    if ssim_weight:
        ssim_term = metrics.ssim_loss(fake_img, gt_hr_img)
        g_loss = g_loss + ssim_weight * ssim_term
        scalars["ssim_loss"] = ssim_term
    probe("g_forward")

    # 9-11
    nerf_render.zero_grad()
    generator.zero_grad()
    g_loss.backward()
    probe("g_backward")
    g_optim.step()
    nerf_optimizer.step()
    probe("g_step")
    util.accumulate(g_ema, generator, 0.5 ** (32 / (10 * 1000)))
    probe("ema")

    if aux is not None:
        aux.update(render=render.detach(), gt_hr_img=gt_hr_img, batch_num=batch_num)
    # every scalar in one transfer (one synchronisation per iteration; float32 values pass through float64 unchanged)
    tail = {"g_loss": g_loss, "psnr": lr_mse, "SR_psnr": sr_mse}
    host = torch.stack([v.detach().float().mean().double() for v in scalars.values()] + [v.detach().double().reshape(()) for v in tail.values()]).tolist()
    out = dict(zip(list(scalars) + list(tail), host))
    out["psnr"], out["SR_psnr"] = mse2psnr(out["psnr"]), mse2psnr(out["SR_psnr"])
    out["gan_loss_weight"] = glw
    return out


def build_nets(cfg, su_args, n_frames, device):
    """train_avatarHD.py:109-116"""
    render_size, gen_size = cfg.models.StyleUnet.inp_size, cfg.models.StyleUnet.out_size
    kw = dict(inp_size=render_size, inp_ch=cfg.models.StyleUnet.inp_ch, out_size=gen_size, out_ch=3, style_dim=su_args.latent, c_dim=0,
              n_mlp=su_args.n_mlp, channel_multiplier=su_args.channel_multiplier)
    nerf_render = Trainer(cfg, n_frames).to(device)
    generator = SWGAN_unet(**kw).to(device)
    discriminator = Discriminator(gen_size, 3, channel_multiplier=su_args.channel_multiplier, c_dim=0).to(device)
    g_ema = SWGAN_unet(**kw).to(device)
    g_ema.eval()
    styleUnet_util.accumulate(g_ema, generator, 0)
    return {"nerf_render": nerf_render, "generator": generator, "discriminator": discriminator, "g_ema": g_ema}


def build_optims(cfg, su_args, nets, lr=1e-3):
    """train_avatarHD.py:117-122 (su_args.lr is overwritten with 1e-3 there)"""
    g_ratio = su_args.g_reg_every / (su_args.g_reg_every + 1)
    d_ratio = su_args.d_reg_every / (su_args.d_reg_every + 1)
    return {"g_optim": torch.optim.Adam(nets["generator"].parameters(), lr=lr * g_ratio, betas=(0 ** g_ratio, 0.99 ** g_ratio)),
            "d_optim": torch.optim.Adam(nets["discriminator"].parameters(), lr=lr * d_ratio, betas=(0 ** d_ratio, 0.99 ** d_ratio)),
            "nerf_optimizer": getattr(torch.optim, cfg.optimizer.type)([{"params": nets["nerf_render"].parameters()}], lr=cfg.optimizer.lr)}


def checkpoint_dict(i, nets, optims):
    """train_avatarHD.py:347-357"""
    return {"iter": i, "nerf_optimizer": optims["nerf_optimizer"].state_dict(), "g_optim": optims["g_optim"].state_dict(),
            "d_optim": optims["d_optim"].state_dict(), "nerf_render": nets["nerf_render"].state_dict(), "g": nets["generator"].state_dict(),
            "d": nets["discriminator"].state_dict(), "g_ema": nets["g_ema"].state_dict(), "latent_codes": nets["nerf_render"].latent_codes.data}


def load_checkpoint(args, nets, optims):
    """Both load modes of train_avatarHD.py:137-159.  Returns the iteration the run continues after (-1: from the start)."""
    if not os.path.exists(args.ckpt):
        return -1
    print(args.ckpt)
    checkpoint = torch.load(args.ckpt, map_location="cpu")
    if not args.continue_training:          # a stage-one checkpoint (train_avatar.py) + the pretrained image-translation GAN
        nets["nerf_render"].load_state_dict(checkpoint["trainer_state_dict"])
        if not os.path.exists(args.gan_ckpt):
            raise FileNotFoundError("--gan-ckpt %s does not exist: starting stage two from a stage-one checkpoint needs the pretrained "
                                    "image-translation GAN (keys g, d, g_ema); pass its path with --gan-ckpt" % args.gan_ckpt)
        gan = torch.load(args.gan_ckpt, map_location="cpu")
        nets["generator"].load_state_dict(gan["g"])
        nets["discriminator"].load_state_dict(gan["d"])
        nets["g_ema"].load_state_dict(gan["g_ema"])
        return -1
    nets["nerf_render"].load_state_dict(checkpoint["nerf_render"])
    optims["nerf_optimizer"].load_state_dict(checkpoint["nerf_optimizer"])
    nets["generator"].load_state_dict(checkpoint["g"])
    nets["discriminator"].load_state_dict(checkpoint["d"])
    nets["g_ema"].load_state_dict(checkpoint["g_ema"])
    optims["g_optim"].load_state_dict(checkpoint["g_optim"])
    optims["d_optim"].load_state_dict(checkpoint["d_optim"])
    return int(checkpoint["iter"])


def rng_state(device):
    st = {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state()}
    if torch.device(device).type == "cuda":
        st["device"] = torch.cuda.get_rng_state(device)
    return st


def set_rng_state(st, device):
    random.setstate(st["python"])
    np.random.set_state(st["numpy"])
    torch.set_rng_state(st["torch"])
    if "device" in st and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(st["device"], device)


def write_sample(path, g_ema, sample_z, render, gt_hr_img, batch_num):
    """train_avatarHD.py:333-345: g_ema on the fixed latent, next to the up-sampled render and the ground truth, clamped to [0, 1];
    the frames of the batch side by side.  lr_img is the ATen statement here (the loss node never writes it)."""
    with torch.no_grad():
        g_ema.eval()
        sample = g_ema([sample_z[:batch_num]], render[:, 3:])
        lr_img = F.interpolate(render[:, :3], size=gt_hr_img.shape[-2:], mode="bilinear", align_corners=True)
        grid = torch.cat([sample, lr_img, gt_hr_img], dim=3).clamp(0, 1)          # [B,3,G,3G]
        grid = torch.cat(list(grid), dim=1)                                       # [3, B*G, 3G]
    imgio.imwrite_rgb(path, (grid.permute(1, 2, 0) * 255).round().byte().cpu().numpy())


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--logdir", type=str, required=True)
    p.add_argument("--datadir", type=str, required=True)
    p.add_argument("--config", type=str, default="config/singleview_512_HD_base.yml", help="Path to (.yml) config file.")
    p.add_argument("--ckpt", type=str, default="", help="Path to load saved checkpoint from.")
    p.add_argument("--continue-training", action="store_true", default=False)
    p.add_argument("--gan-ckpt", type=str, default="pretrained_models/img_translation.ckpt",
                   help="pretrained image-translation GAN (g, d, g_ema) loaded next to a stage-one --ckpt")
    p.add_argument("--percep", type=str, default="lpips", choices=["lpips", "native", "none"],
                   help="'native': this package's LPIPS-VGG module (model/lpips.py) on its own kernels; 'none' drops the 0.1 * LPIPS term "
                        "(no lpips package / weights)")
    p.add_argument("--percep-vgg", type=str, default="", help="--percep native: torchvision VGG16 weights (vgg16-*.pth)")
    p.add_argument("--percep-lin", type=str, default="", help="--percep native: the lpips package's linear layers (weights/v0.1/vgg.pth)")
    p.add_argument("--ssim-weight", type=float, default=0.0, help="adds this times (1 - SSIM(fake, gt)) to the generator's loss (metrics.ssim_loss)")
    p.add_argument("--iters", type=int, default=0, help="run iterations up to this one, exclusive (0 = styleUnet_args.iter)")
    p.add_argument("--batch", type=int, default=0, help="batch size (0 = styleUnet_args.batch)")
    return p.parse_args(argv)


def main(argv=None, device=None):
    args = parse_args(argv)
    su_args = styleUnet_util.styleUnet_args()
    if args.iters:
        su_args.iter = args.iters
    if args.batch:
        su_args.batch = args.batch
    with open(args.config, "r") as f:
        cfg = CfgNode(yaml.load(f, Loader=yaml.FullLoader))
    device = torch.device(device if device is not None else "cuda")
    percep = None
    if args.percep == "lpips":
        try:
            import lpips
        except ImportError as e:
            raise RuntimeError("the 0.1 * LPIPS term of the stage-two loss needs the `lpips` package (VGG weights); install it or pass "
                               "--percep none") from e
        percep = lpips.LPIPS(net="vgg").to(device)
    elif args.percep == "native":
        from ..model.lpips import build_for_harness
        percep = build_for_harness(args.percep_vgg, args.percep_lin, device)
    else:
        print("[train-hd] --percep none: the 0.1 * LPIPS(fake, gt) term of the reference loss is dropped")
    if deterministic_requested():
        enable_determinism()
    workers = switches.integer("HAVATAR_WORKERS", 8)
    train_loader = Loader(split_file=os.path.join(args.datadir, "sv_v31_all.json"), down_sample=cfg.dataset.down_sample, mode="train",
                          batch_size=su_args.batch, num_workers=workers, options=cfg, white_bg=True)
    nets = build_nets(cfg, su_args, len(train_loader.dataset), device)
    optims = build_optims(cfg, su_args, nets)
    os.makedirs(args.logdir, exist_ok=True)
    save_dir = os.path.join(args.logdir, "sample")
    os.makedirs(save_dir, exist_ok=True)
    os.makedirs(os.path.join(args.logdir, "checkpoint"), exist_ok=True)
    with open(os.path.join(args.logdir, "config.yml"), "w") as f:
        f.write(cfg.dump())
    start_iter = load_checkpoint(args, nets, optims)
    sample_z = torch.randn(su_args.batch, su_args.latent, device=device)
    if args.continue_training and os.path.exists(args.ckpt + ".rng"):
        set_rng_state(torch.load(args.ckpt + ".rng", map_location="cpu", weights_only=False), device)
    try:
        from torch.utils.tensorboard import SummaryWriter
        writer = SummaryWriter(args.logdir)
    except Exception:  # tensorboard is optional here
        writer = _NullWriter()
    loader = styleUnet_util.sample_data(train_loader)
    last = su_args.iter - 1
    t0 = time.time()
    i = start_iter
    for i in range(start_iter + 1, su_args.iter):
        aux = {}
        s = joint_step(i, next(loader), nets, optims, cfg, su_args, percep, aux=aux, ssim_weight=args.ssim_weight)
        for k, v in s.items():
            writer.add_scalar("train/" + k, v, i)
        if i % cfg.experiment.print_every == 0 or i == last:
            print("[TRAIN-HD] Iter: %d PSNR: %.4f SR_PSNR: %.4f d: %.4f g: %.4f r1: %.4f hr_l1: %.4f TIME: %.02f" % (
                i, s["psnr"], s["SR_psnr"], s["d"], s["g"], s["r1"], s["hr_l1"], time.time() - t0))
            t0 = time.time()
        if i % cfg.experiment.validate_every == 0 or i == start_iter + 1 or i == last:
            write_sample(os.path.join(save_dir, "%s.png" % str(i).zfill(6)), nets["g_ema"], sample_z, aux["render"], aux["gt_hr_img"], aux["batch_num"])
            torch.save(checkpoint_dict(i, nets, optims), os.path.join(args.logdir, "latest.pt"))
            torch.save(rng_state(device), os.path.join(args.logdir, "latest.pt.rng"))
        if i % cfg.experiment.save_every == 0 or i == cfg.experiment.train_iters - 1 or i == start_iter + 1:
            torch.save(checkpoint_dict(i, nets, optims), os.path.join(args.logdir, "checkpoint", "checkpoint" + str(i).zfill(5) + ".ckpt"))
            print("================== Saved Checkpoint =================")
    print("Done!")
    return i


def seed_all(seed=42):
    """the entry script's seeds; mixing_noise draws from Python's generator, which the reference leaves unseeded"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


if __name__ == "__main__":
    seed_all()
    main()

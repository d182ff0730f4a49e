"""The joint stage-two step as one driver: given the classes (`Trainer`, `SWGAN_unet`, `Discriminator`) and a module with the stage-two
helpers, build the three networks with key-derived weights (synth.fill_state_dict), read the two frames of synth.write_dataset through
dataloaderSR.Loader and run iterations i = 0 (R1 on) and i = 1 of harness/train_hd.py::joint_step with synth.harness_config() (render 32 ->
128, deterministic sampling), both RNGs seeded, no percep term.  Results are checksums and strided slices only (the size of
tests/golden/discriminator.npz, not of a weight file).  tools/gen_golden_stage2_step.py runs it on the reference's classes and stores
tests/golden/stage2_step.npz; tests/test_train_hd_cpu.py and tests/test_train_hd_gpu.py run it on this package's classes and compare."""
import random

import numpy as np
import torch

from .. import synth
from ..dataloader.dataloaderSR import Loader
from ..utils.cfgnode import CfgNode
from . import train_hd
from .stage2_cases import SLICE, checksum, strided

NETS = ("nerf_render", "generator", "discriminator")
STEP_SLICE = 16          # values kept of a gradient (every fourth of stage2_cases.strided)
SCALARS = ("d", "real_score", "fake_score", "r1", "rgb_loss", "code_loss", "mask_loss", "nerf_loss", "g", "hr_l1", "g_loss", "psnr", "SR_psnr")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


class _HostDraws:
    """the helper module with mixing_noise drawn from host generators of its own and moved to the device: a run on the device then sees the
    latents of the same run on the CPU.  (torch.randn on a device draws from that device's stream, and the host's global stream advances by
    the generator's per-call noise maps on a CPU run only.)"""

    def __init__(self, util):
        self._util, self._random, self._gen = util, random.Random(11), torch.Generator().manual_seed(123)

    def __getattr__(self, name):
        return getattr(self._util, name)

    def mixing_noise(self, batch, latent_dim, prob, device):
        n = 2 if prob > 0 and self._random.random() < prob else 1
        return [torch.randn(batch, latent_dim, generator=self._gen).to(device) for _ in range(n)]


def build(Trainer, SWGAN_unet, Discriminator, util, split, device="cpu", dtype=torch.float32, cfg=None, pinned=False):
    """(cfg, su_args, nets, optims, the one batch of both frames) -- construction-time random numbers pinned by torch.manual_seed(5).
    pinned: the generator's NoiseInjection strengths are zeroed (its per-call noise is drawn on the device the run is on, so two devices never
    see the same maps), as the harness tests of stage one do."""
    cfg = CfgNode(synth.harness_config()) if cfg is None else cfg
    su_args = util.styleUnet_args()
    loader = Loader(split_file=split, mode="train", batch_size=2, num_workers=0, down_sample=cfg.dataset.down_sample, options=cfg,
                    white_bg=True, shuffle=False)
    batch = next(iter(loader))
    torch.manual_seed(5)
    kw = dict(inp_size=32, inp_ch=cfg.models.StyleUnet.inp_ch, out_size=128, out_ch=3, style_dim=su_args.latent, c_dim=0, n_mlp=su_args.n_mlp,
              channel_multiplier=su_args.channel_multiplier)
    nets = {"nerf_render": synth.fill_state_dict(Trainer(cfg, len(loader.dataset))),
            "generator": synth.fill_state_dict(SWGAN_unet(**kw), seed=1),
            "discriminator": synth.fill_state_dict(Discriminator(128, 3, channel_multiplier=su_args.channel_multiplier, c_dim=0), seed=2),
            "g_ema": SWGAN_unet(**kw)}
    if pinned:
        nets["generator"].load_state_dict(synth.zero_noise_weights(nets["generator"].state_dict()))
    if dtype != torch.float32:
        batch = (batch[0], {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch[1].items()})
    for k in nets:
        nets[k] = nets[k].to(device=device, dtype=dtype)
    nets["g_ema"].eval()
    util.accumulate(nets["g_ema"], nets["generator"], 0)
    nets["nerf_render"].train()
    optims = train_hd.build_optims(cfg, su_args, nets)
    return cfg, su_args, nets, optims, batch


def _sums(module):
    return np.stack([checksum(_np(p)) for _, p in module.named_parameters()])


def _grads(module):
    return [None if p.grad is None else p.grad.detach().clone() for p in module.parameters()]


def _changed(module, before):
    """how many parameters' .grad a backward touched: a gradient that was not there, or other values in it"""
    return sum((p.grad is not None) and (b is None or not torch.equal(p.grad, b)) for p, b in zip(module.parameters(), before))


def run_iteration(i, batch, nets, optims, cfg, su_args, util, out, tag, records="all", percep=None):
    """one joint_step with the records taken at its probe points.  A backward leaves the gradients of the modules it does not reach as they
    were (None at first, the previous backward's afterwards): `*_touched_*` counts the parameters whose .grad it changed."""
    snap = {}

    def probe(name):
        if name == "render_nograd":
            snap.update({n: _grads(nets[n]) for n in ("nerf_render", "generator")})
        elif name == "d_backward":
            out[tag + "_d_backward_touched_outside_d"] = np.array([_changed(nets[n], snap[n]) for n in ("nerf_render", "generator")])
        elif name in ("d_step", "r1_step") and records == "all":
            out["%s_%s_d_sums" % (tag, name)] = _sums(nets["discriminator"])
        elif name == "g_forward":
            snap["discriminator"] = _grads(nets["discriminator"])
        elif name == "g_backward":
            out[tag + "_g_backward_touched_d"] = np.array([_changed(nets["discriminator"], snap["discriminator"])])
            for n in ("nerf_render", "generator"):
                ps = list(nets[n].named_parameters())
                out["%s_grad_%s_has" % (tag, n)] = np.array([p.grad is not None and bool(p.grad.abs().sum() > 0) for _, p in ps])
                out["%s_grad_%s_sums" % (tag, n)] = np.stack([checksum(_np(p.grad)) if p.grad is not None else np.zeros(4) for _, p in ps])
                out["%s_grad_%s_slices" % (tag, n)] = np.stack([np.resize(strided(_np(p.grad))[::SLICE // STEP_SLICE], STEP_SLICE)
                                                                if p.grad is not None else np.zeros(STEP_SLICE) for _, p in ps])
        elif name == "g_step" and records == "all":
            for n in NETS:
                out["%s_step_%s_sums" % (tag, n)] = _sums(nets[n])
        elif name == "ema" and records == "all":
            out[tag + "_g_ema_sums"] = _sums(nets["g_ema"])

    s = train_hd.joint_step(i, batch, nets, optims, cfg, su_args, percep, util=util, probe=probe)
    for k in SCALARS + (("percep_loss",) if percep is not None else ()):
        out["%s_scalar_%s" % (tag, k)] = np.array(s[k])
    return s


def run(Trainer, SWGAN_unet, Discriminator, util, split, device="cpu", dtype=torch.float32, iterations=(0, 1), out=None, prefix="", records="all",
        pinned=False, percep=None):
    """Every iteration starts from the freshly built state and the same seeds (iteration 1 is the step without R1, not the step after
    iteration 0: one Adam update with beta1 = 0 moves every weight by lr * sign(gradient), which turns the rounding noise of the small
    gradients into full-size differences between any two float32 implementations).  pinned: every random number the step consumes is the
    same on every device (comparisons between devices): latents drawn on the host, the generator's noise strengths zeroed.  percep: a callable
    (device, dtype) -> the LPIPS module of the step's 0.1 * LPIPS term (None: no such term, as the fixture was recorded)."""
    out = {} if out is None else out
    for i in iterations:
        if pinned:
            util = _HostDraws(util._util if isinstance(util, _HostDraws) else util)
        cfg, su_args, nets, optims, batch = build(Trainer, SWGAN_unet, Discriminator, util, split, device, dtype, pinned=pinned)
        for n in NETS:
            out["names_" + n] = np.array([k for k, _ in nets[n].named_parameters()])
        random.seed(11)
        torch.manual_seed(123)
        run_iteration(i, batch, nets, optims, cfg, su_args, util, out, "%si%d" % (prefix, i), records,
                      percep=None if percep is None else percep(device, dtype))
    return out

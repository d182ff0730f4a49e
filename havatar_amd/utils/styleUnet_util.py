"""Stage-two (HD) training helpers: the hyper-parameter record, the GAN losses with their two regularisers, the EMA update and the
latent-noise draws -- names, signatures and results of the reference's utils/styleUnet_util.py:10-117, so `from utils.styleUnet_util
import ...` of a training script finds them here.  Plain PyTorch: everything heavy runs inside the networks these are applied to."""
import math
import random

import torch
from torch import autograd, nn
from torch.nn import functional as F

from ..model.op import conv2d_gradfix


class styleUnet_args(nn.Module):
    """the reference's stage-two settings (:10-37)"""

    def __init__(self):
        super().__init__()
        self.iter = 800000                 # total training iterations
        self.latent = 64
        self.n_mlp = 4
        self.channel_multiplier = 2
        self.start_iter = 0
        self.batch = 2                     # per GPU; <= 4 or a multiple of 4 (the discriminator's stddev group)
        self.wandb = True
        self.lr = 0.0005
        self.mixing = 0.9                  # probability of latent mixing
        self.augment = True
        self.augment_p = 0.                # 0 = adaptive
        self.ada_target = 0.6
        self.ada_length = 500 * 1000
        self.ada_every = 256
        self.path_regularize = 2.          # weight of the path-length regulariser
        self.path_batch_shrink = 2
        self.g_reg_every = 4
        self.view_dis_every = 0
        self.r1 = 10.                      # weight of the R1 regulariser
        self.d_reg_every = 16


def requires_grad(model, flag=True):
    """a Parameter, a list of them, or a module"""
    if type(model) == nn.parameter.Parameter:
        model.requires_grad = flag
    elif type(model) == list:
        for p in model:
            p.requires_grad = flag
    else:
        for p in model.parameters():
            p.requires_grad = flag


def accumulate(model1, model2, decay=0.999):
    """model1 <- decay * model1 + (1 - decay) * model2, parameter by parameter (the EMA generator)"""
    par2 = dict(model2.named_parameters())
    for k, p in model1.named_parameters():
        p.data.mul_(decay).add_(par2[k].data, alpha=1 - decay)


def sample_data(loader):
    while True:
        for batch in loader:
            yield batch


def d_logistic_loss(real_pred, fake_pred):
    return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean()


def d_r1_loss(real_pred, real_img):
    """mean over the batch of |d sum(real_pred) / d real_img|^2, differentiable (create_graph): the networks' native nodes restate their
    backward with ATen ops for this, and form no weight gradient in the first differentiation"""
    with conv2d_gradfix.no_weight_gradients():
        grad_real, = autograd.grad(outputs=real_pred.sum(), inputs=real_img, create_graph=True)
    return grad_real.pow(2).reshape(grad_real.shape[0], -1).sum(1).mean()


def g_nonsaturating_loss(fake_pred):
    return F.softplus(-fake_pred).mean()


def g_path_regularize(fake_img, latents, mean_path_length, decay=0.01):
    noise = torch.randn_like(fake_img) / math.sqrt(fake_img.shape[2] * fake_img.shape[3])
    grad, = autograd.grad(outputs=(fake_img * noise).sum(), inputs=latents, create_graph=True)
    path_lengths = torch.sqrt(grad.pow(2).sum(2).mean(1))
    path_mean = mean_path_length + decay * (path_lengths.mean() - mean_path_length)
    path_penalty = (path_lengths - path_mean).pow(2).mean()
    return path_penalty, path_mean.detach(), path_lengths


def make_noise(batch, latent_dim, n_noise, device):
    if n_noise == 1:
        return torch.randn(batch, latent_dim, device=device)
    return torch.randn(n_noise, batch, latent_dim, device=device).unbind(0)


def mixing_noise(batch, latent_dim, prob, device):
    if prob > 0 and random.random() < prob:
        return make_noise(batch, latent_dim, 2, device)
    return [make_noise(batch, latent_dim, 1, device)]

"""Shared by tests/test_isosurface_{cpu,gpu}.py: the test fields, the topology measures of a triangle list, and the avatar fixture."""
import functools
from collections import Counter

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------------------------------------------
# fields: (field float32 [D0,D1,D2], iso, origin, spacing)
# ------------------------------------------------------------------------------------------------------------------------------------
def _axes(shape):
    return np.meshgrid(*[np.linspace(-1.0, 1.0, d) for d in shape], indexing="ij")


def _box(shape):
    return (-1.0, -1.0, -1.0), tuple(2.0 / (d - 1) for d in shape)


def sphere(shape):
    x, y, z = _axes(shape)
    return torch.from_numpy((0.7 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)), 0.0, *_box(shape)


def torus(shape):
    x, y, z = _axes(shape)
    return torch.from_numpy((0.2 - np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z)).astype(np.float32)), 0.0, *_box(shape)


def _noise(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def noise(shape, seed=1):
    return _noise(shape, seed), 0.0, (-1.0, 2.0, 0.5), (0.5, 0.25, 1.0)


def ties(shape, seed=2):
    """5 x noise rounded to integers: about 8 % of the values EQUAL the level"""
    return torch.round(5.0 * _noise(shape, seed)), 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def all_inside(shape):
    return torch.ones(shape), 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def all_outside(shape):
    return -torch.ones(shape), 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def sprinkled(shape, seed=3):
    """noise with NaN, +inf and -inf in about 5 % of the points each"""
    f = _noise(shape, seed)
    u = torch.rand(shape, generator=torch.Generator().manual_seed(seed + 100))
    f[u < 0.05] = float("nan")
    f[(u >= 0.05) & (u < 0.10)] = float("inf")
    f[(u >= 0.10) & (u < 0.15)] = float("-inf")
    return f, 0.25, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def padded(case):
    """the field inside one layer of -10: the surface cannot leave the grid"""
    f, iso, origin, spacing = case
    return torch.nn.functional.pad(f, (1, 1, 1, 1, 1, 1), value=-10.0), iso, origin, spacing


FIELDS = {"sphere": sphere, "torus": torus, "noise": noise, "ties": ties, "all_inside": all_inside, "all_outside": all_outside,
          "sprinkled": sprinkled}


# ------------------------------------------------------------------------------------------------------------------------------------
# topology of a triangle list
# ------------------------------------------------------------------------------------------------------------------------------------
def edge_uses(tris):
    """Counter of undirected edges, Counter of directed edges"""
    t = np.asarray(tris).reshape(-1, 3)
    und, dire = Counter(), Counter()
    for a, b, c in t.tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            dire[(p, q)] += 1
            und[(min(p, q), max(p, q))] += 1
    return und, dire


def is_closed(tris):
    und, _ = edge_uses(tris)
    return all(v == 2 for v in und.values())


def is_oriented(tris):
    """every directed edge is used once (with is_closed: its reverse is used once too)"""
    _, dire = edge_uses(tris)
    return all(v == 1 for v in dire.values())


def euler(n_verts, tris):
    und, _ = edge_uses(tris)
    return n_verts - len(und) + len(np.asarray(tris).reshape(-1, 3))


def all_referenced(n_verts, tris):
    return np.array_equal(np.unique(np.asarray(tris)), np.arange(n_verts))


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def angles(a, b):
    """angle between unit rows of a and of b, radians, float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.einsum("ij,ij->i", a, b))


# ------------------------------------------------------------------------------------------------------------------------------------
# the avatar: a Trainer with the synthetic weights and one synthetic frame's planes
# ------------------------------------------------------------------------------------------------------------------------------------
def frame(device="cpu", n_rays_hw=(2, 4)):
    """the inputs of Trainer.forward for one synthetic frame (validation mode, a few rays)"""
    from havatar_amd import synth
    cond = [torch.from_numpy(c).to(device) for c in synth.cond_images(1)]
    rays = torch.from_numpy(synth.camera_rays(*n_rays_hw))[None].to(device)
    return {"mode": "validation", "fidx": torch.zeros(1, dtype=torch.long), "render_full_img": False, "ray_batch": rays,
            "background_prior": torch.ones(1, rays.shape[1], 3, device=device), "front_render_cond": cond[0], "left_render_cond": cond[1],
            "right_render_cond": cond[2], "inv_head_T": torch.from_numpy(synth.inv_head_T())[None].to(device)}


def make_trainer(device="cpu"):
    """a Trainer with the synthetic weights (a function of the state_dict keys: the same on every call)"""
    from havatar_amd import synth
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    state = torch.get_rng_state()
    trainer = synth.fill_state_dict(Trainer(CfgNode(synth.harness_config()), 3)).requires_grad_(False).to(device).eval()
    torch.set_rng_state(state)
    return trainer


@functools.lru_cache(maxsize=None)
def avatar(device="cpu"):
    """(trainer, frame inputs, what forward returned; None on a device, where only the planes are set) -- the trainer's planes are that frame's"""
    trainer = make_trainer(device)
    inp = frame(device)
    with torch.no_grad():
        if device == "cpu":
            out = trainer(**inp)
        else:          # the planes alone: what nerf_forward does ahead of the march
            out = None
            trainer.model_coarse.set_conditional_embedding(
                front_render_cond=inp["front_render_cond"], left_render_cond=inp["left_render_cond"], right_render_cond=inp["right_render_cond"],
                latents=trainer.latent_codes[0:1], cond_c=inp["inv_head_T"].view(1, -1))
    return trainer, inp, out

"""Deterministic synthetic inputs for the ray-march path (numpy only, no torch RNG).

Everything here is a pure function of (shape, seed): a counter-based splitmix64 hash, so the
same tensors can be regenerated bit-for-bit in the golden-fixture generator (which runs next to
the reference), in the parity tests and in ``bench.py`` on the GPU box, without shipping the
8 MB tri-plane / 2 MB skinning volume / 190 KB MLP as fixture files.

The scene follows SURVEY.md section 8(d): pinhole camera at (0,0,5) looking at the origin
(reference ray convention: dataloader/data_util.py:28-56), near/far = 5-1.6 / 5+1.0
(dataloader/dataloader.py:174-177), white background, ``inv_head_T = [R^-1; -t]``
(dataloader/dataloader.py:215-216).
"""
import math

import numpy as np

_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x += np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _counter(n, seed, stream):
    base = np.uint64((seed * 0x100000001B3 + stream * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        return np.arange(n, dtype=np.uint64) * np.uint64(2) + base


def uniform(shape, seed, lo=0.0, hi=1.0):
    """float32 U[lo,hi) with 24 random mantissa bits, element i depends only on (seed, i)."""
    n = int(np.prod(shape)) if len(shape) else 1
    z = _splitmix64(_counter(n, seed, 1))
    u = (z >> np.uint64(40)).astype(np.float64) * (1.0 / 16777216.0)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def normal(shape, seed, std=1.0):
    """float32 N(0, std^2) by Box-Muller on two hash streams."""
    n = int(np.prod(shape)) if len(shape) else 1
    z1 = _splitmix64(_counter(n, seed, 2))
    z2 = _splitmix64(_counter(n, seed, 3))
    u1 = ((z1 >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    u2 = (z2 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
    return (std * g).astype(np.float32).reshape(shape)


# ----------------------------------------------------------------------------------------------
# Scene pieces
# ----------------------------------------------------------------------------------------------
XYZ_BOUNDING = [[-1.5, 1.5], [-1.6, 1.4], [-1.6, 1.2]]  # config/singleview_512_HD_base.yml:49


def box_warp_param(xb, yb, zb):
    """scale = 2/(max-min), trans = -scale*(max+min)/2  (utils/util.py:179-186)."""
    out_s, out_t = [], []
    for lo, hi in (xb, yb, zb):
        f = 2.0 / (hi - lo)
        c = f * (lo + hi) * 0.5
        out_s.append(float(f))
        out_t.append(float(-c))
    return tuple(out_s), tuple(out_t)


def nerf_box():
    return box_warp_param(*XYZ_BOUNDING)


def skin_box():
    """Skin box = XYZ_bounding with Y_min := 0.3*Y_max (model/nerf_trainer.py:29-34)."""
    yb = [0.3 * XYZ_BOUNDING[1][1], XYZ_BOUNDING[1][1]]
    return box_warp_param(XYZ_BOUNDING[0], yb, XYZ_BOUNDING[2])


def euler_deg_to_R(yaw, pitch, roll):
    y, p, r = (math.radians(a) for a in (yaw, pitch, roll))
    Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    Rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float64)


def inv_head_T(yaw=15.0, pitch=-8.0, roll=3.0, t=(0.02, -0.03, 0.01)):
    """[4,3] = [R^-1 ; -t]  (dataloader/dataloader.py:215-216; right-multiplied row vectors)."""
    R = euler_deg_to_R(yaw, pitch, roll)
    return np.concatenate([np.linalg.inv(R), -np.asarray(t, np.float64)[None]], 0).astype(np.float32)


def frame_pose(k, n=64):
    """Head pose of frame k of an n-frame self-reenactment batch."""
    return inv_head_T(yaw=20.0 * math.sin(2.0 * math.pi * k / n))


def camera_rays(H, W, cam_dist=5.0, focal=1.7, near_off=-1.6, far_off=1.0, y0=0, y1=None):
    """[rows*W, 8] = (o3, d3, near, far), row-major pixels, for image rows y0:y1.

    Pinhole K = [[focal*W,0,0.5*W],[0,focal*H,0.5*H],[0,0,1]], dirs = K^-1 [i,j,1], camera looks
    down +z in its own frame; c2w = diag(1,-1,-1) with origin (0,0,cam_dist); directions are
    normalised (dataloader/data_util.py:28-56, normalize=True).
    """
    if y1 is None:
        y1 = H
    fx, fy, cx, cy = focal * W, focal * H, 0.5 * W, 0.5 * H
    j, i = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones_like(i)], -1)
    c2w = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)
    d = dirs @ c2w.T
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.array([0.0, 0.0, cam_dist]), d.shape)
    near = np.full(d.shape[:-1] + (1,), cam_dist + near_off)
    far = np.full(d.shape[:-1] + (1,), cam_dist + far_off)
    return np.concatenate([o, d, near, far], -1).reshape(-1, 8).astype(np.float32)


def triplane(B=1, C=64, res=128, seed=2, std=0.5, lowres=32):
    """[2,B,C,res,res] NCHW like Trainer.model_coarse.triPlane_embeddings (model/nerf_model.py:85-86).

    lowres=None: white noise (every texel independent: the worst case for the gather and for the
    conditioning of the fine pass).  lowres=n: n x n noise upsampled bilinearly (align_corners) to
    res x res and renormalised to `std` -- band-limited like the output of the StyleGAN encoders.
    """
    if lowres is None or lowres >= res:
        return normal((2, B, C, res, res), seed, std)
    lo = normal((2, B, C, lowres, lowres), seed, 1.0).astype(np.float64)
    t = np.linspace(0.0, lowres - 1.0, res)
    i0 = np.floor(t).astype(np.int64)
    i1 = np.minimum(i0 + 1, lowres - 1)
    f = t - i0
    a = lo[..., i0, :] * (1.0 - f)[:, None] + lo[..., i1, :] * f[:, None]
    b = a[..., i0] * (1.0 - f) + a[..., i1] * f
    return (b / b.std() * std).astype(np.float32)


def skin_volume(res=64, seed=3):
    """[2,res,res,res] frozen skinning volume as fix_canonical_W leaves it (model/Skinning_Field.py:57-62).

    x = sigmoid(2*N(0,1)); slab W1[:, 0, :] = 1; W1[:1, :res//8, :] = 1; W0 = 1 - W1.
    """
    g = normal((res, res, res), seed, 2.0).astype(np.float64)
    w1 = (1.0 / (1.0 + np.exp(-g))).astype(np.float32)
    w1[:, 0, :] = 1.0
    w1[:1, : res // 8, :] = 1.0
    return np.stack([1.0 - w1, w1], 0).astype(np.float32)


def mlp_weights(seed=10, alpha_gain=5.0, alpha_bias=0.2, in_dim=176, hid=128, feat=64):
    """Radiance-MLP parameters in the reference's nn.Linear layout (model/nerf_model.py:46-51).

    U(-1/sqrt(fan_in), 1/sqrt(fan_in)) like torch's default Linear init, then the density head is
    rescaled so that the accumulated opacity is not vacuous (primary recipe
    gain 5 / bias 0.2, stress recipe gain 20 / bias -0.5).
    """
    def lin(o, i, s):
        b = 1.0 / math.sqrt(i)
        return uniform((o, i), s, -b, b), uniform((o,), s + 1000, -b, b)

    W1, b1 = lin(hid, in_dim, seed)
    W2, b2 = lin(hid, hid, seed + 1)
    Wa, ba = lin(1, hid, seed + 2)
    Wf, bf = lin(feat, hid, seed + 3)
    Wc, bc = lin(3, feat, seed + 4)
    Wa = (Wa * np.float32(alpha_gain)).astype(np.float32)
    ba = np.full_like(ba, alpha_bias)
    return dict(W1=W1, b1=b1, W2=W2, b2=b2, Wa=Wa, ba=ba, Wf=Wf, bf=bf, Wc=Wc, bc=bc)


# recipe -> (density-head rescale, tri-plane smoothness).  Conditioning of the fine pass, measured as the
# reference's own fp32-vs-fp64 L-inf on rgb_fine / depth_fine / acc_fine over a 16x16 frame:
#   primary 8e-6 / 9e-5 / 2e-5   |   stress 2e-4 / 3e-3 / 4e-4   |   white 6e-5 / 6e-4 / 1e-4
RECIPES = {
    "primary": dict(mlp=dict(alpha_gain=5.0, alpha_bias=0.2), lowres=32),
    "stress": dict(mlp=dict(alpha_gain=40.0, alpha_bias=0.0), lowres=16),
    "white": dict(mlp=dict(alpha_gain=5.0, alpha_bias=0.2), lowres=None),
}


def scene(H, W, recipe="primary", y0=0, y1=None, B=1, pose=None):
    """Everything one ray-march call needs, as numpy float32 (NCHW planes, reference layouts)."""
    rays = camera_rays(H, W, y0=y0, y1=y1)
    R = rays.shape[0]
    ns, nt = nerf_box()
    ss, st = skin_box()
    return dict(
        rays=np.broadcast_to(rays[None], (B, R, 8)).copy(),
        bg=np.ones((B, R, 3), np.float32),
        inv_T=np.broadcast_to((inv_head_T() if pose is None else pose)[None], (B, 4, 3)).copy(),
        planes=triplane(B=B, lowres=RECIPES[recipe]["lowres"]),
        vol=skin_volume(),
        mlp=mlp_weights(**RECIPES[recipe]["mlp"]),
        nerf_scale=ns, nerf_trans=nt, skin_scale=ss, skin_trans=st,
    )


# ----------------------------------------------------------------------------------------------
# Deterministic parameters for whole modules (encoders, upsampler, volume decoder): value = f(key name, shape)
# ----------------------------------------------------------------------------------------------
_KEEP = ("kernel", ".ll", ".lh", ".hl", ".hh", "scale_factor", "trans_factor", "identity_trans")


def fill_state_dict(module, seed=0, mlp_recipe="primary"):
    """Overwrite every parameter/buffer of `module` (a torch.nn.Module) with values that depend only on the state_dict key
    and shape, so the reference model and this repo's mirror can be given identical weights without shipping them.
    FIR / wavelet / box-warp buffers are left alone; the radiance MLP gets `mlp_weights(recipe)`."""
    import zlib

    import torch
    mlp = mlp_weights(**RECIPES[mlp_recipe]["mlp"])
    mlp_keys = {"layers_xyz.0.weight": "W1", "layers_xyz.0.bias": "b1", "layers_xyz.1.weight": "W2", "layers_xyz.1.bias": "b2",
                "fc_alpha.weight": "Wa", "fc_alpha.bias": "ba", "fc_rgbFeat.weight": "Wf", "fc_rgbFeat.bias": "bf",
                "fc_rgb.weight": "Wc", "fc_rgb.bias": "bc"}
    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        if any(k.endswith(s) or s + "." in k for s in _KEEP) or not torch.is_floating_point(v):
            continue
        hit = [mk for mk in mlp_keys if k.endswith("model_coarse." + mk) or k == mk]
        if hit:
            new[k] = torch.from_numpy(mlp[mlp_keys[hit[0]]].reshape(tuple(v.shape)))
            continue
        s = (zlib.crc32(k.encode()) + 7919 * seed) & 0x7FFFFFFF
        shape = tuple(v.shape)
        if k.endswith("init_lc"):
            a = uniform(shape, s)
        elif "canonical_Wvolume" in k:
            a = normal(shape, s, 0.05 if k.endswith("weight") else 0.01)
        elif k.endswith("latent_codes"):
            a = normal(shape, s, 0.3)
        elif k.endswith("bias"):
            a = normal(shape, s, 0.1) + (1.0 if "modulation" in k else 0.0)
        elif "noise" in k and k.endswith("weight"):
            a = normal(shape, s, 0.1)
        else:
            a = normal(shape, s, 1.0)
        new[k] = torch.from_numpy(a.reshape(shape))
    sd.update(new)
    module.load_state_dict(sd)
    return module


def cond_images(B=1, res=256, seed=60):
    """front/left/right condition renders [B,7,res,res] in [0,1]: smooth pseudo-renders (rgb, normal, mask)."""
    out = []
    for v in range(3):
        lo = uniform((B, 7, 16, 16), seed + v).astype(np.float64)
        t = np.linspace(0.0, 15.0, res)
        i0 = np.floor(t).astype(np.int64)
        i1 = np.minimum(i0 + 1, 15)
        f = t - i0
        a = lo[..., i0, :] * (1 - f)[:, None] + lo[..., i1, :] * f[:, None]
        img = a[..., i0] * (1 - f) + a[..., i1] * f
        img[:, 6] = (img[:, 6] > 0.45).astype(np.float64)
        out.append(img.astype(np.float32))
    return out


def head_mesh(k=0, n_lat=12, n_lon=16):
    """A small tracked-head stand-in in the fitted model's space: a UV sphere with a nose towards -z (the front view's camera looks along +z), turned and scaled a little with the
    frame number k.  (vs [V,3] float32, color [V,3] float32 in 30...250, tris [F,3] int32); the topology does not depend on k."""
    th = np.linspace(0.0, math.pi, n_lat + 1)[1:-1]
    ph = np.arange(n_lon) * (2.0 * math.pi / n_lon)
    ring = np.stack([np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon)), np.outer(np.sin(th), np.cos(ph))], -1).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]], 0)
    nose = np.exp(-((unit[:, 0] / 0.35) ** 2 + ((unit[:, 1] + 0.1) / 0.35) ** 2)) * (unit[:, 2] < 0)
    rad = (0.95 + 0.01 * k) * (1.0 + 0.25 * nose)
    yaw = 0.15 * math.sin(1.3 * k)
    R = np.array([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
    vs = (unit * rad[:, None] * np.array([0.9, 1.15, 1.0])) @ R.T + np.array([0.03, -0.12, -0.15])
    color = np.stack([140.0 + 100.0 * unit[:, 0], 130.0 + 90.0 * unit[:, 1], 120.0 + 80.0 * unit[:, 2]], -1) + 10.0 * nose[:, None]
    last = 1 + (n_lat - 1) * n_lon
    tris = []
    for j in range(n_lon):
        jn = (j + 1) % n_lon
        tris.append((0, 1 + j, 1 + jn))
        tris.append((last, 1 + (n_lat - 2) * n_lon + jn, 1 + (n_lat - 2) * n_lon + j))
        for i in range(n_lat - 2):
            a, b, c, d = 1 + i * n_lon + j, 1 + i * n_lon + jn, 1 + (i + 1) * n_lon + j, 1 + (i + 1) * n_lon + jn
            tris += [(a, c, d), (a, d, b)]
    return vs.astype(np.float32), np.clip(color, 30.0, 250.0).astype(np.float32), np.asarray(tris, np.int32)


def write_dataset(root, n_frames=2, img_res=128, focal=1.7, cam_dist=5.0, seed=60, views=("0",), photos=True, cond_mesh=False):
    """A tiny synthetic dataset in the reference's on-disk layout (split file `sv_v31_all.json` + PNGs, see
    havatar_amd/dataloader/_base.py) for the harness tests and demos: pinhole camera of SURVEY 8(d), per-frame head pose
    `frame_pose(k)`, 256^2 3DMM condition renders from `cond_images`, a shaded-disc photograph and its mask per view
    (`photos=False` skips those two: test-mode readers never open them).  Returns the split-file path.
    cond_mesh=True: every frame also gets `cond_mesh.npz` (vs, color of `head_mesh(k)`), `tri.npy` lies next to the split file, and the six
    condition PNGs are that mesh rendered by `conditions.conditions_statement`, so the PNGs and the mesh describe the same frame."""
    import json
    import os

    from .dataloader import imgio
    os.makedirs(root, exist_ok=True)
    if cond_mesh:
        import torch

        from . import conditions
        np.save(os.path.join(root, "tri.npy"), head_mesh(0)[2])
    c2w = [[1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, cam_dist], [0.0, 0.0, 0.0, 1.0]]
    yy, xx = np.meshgrid(np.arange(img_res), np.arange(img_res), indexing="ij")
    frames = []
    for k in range(n_frames):
        inst = os.path.join(root, "frame_%04d" % k)
        os.makedirs(inst, exist_ok=True)
        if cond_mesh:
            vs, color, tris = head_mesh(k)
            np.savez(os.path.join(inst, conditions.MESH_FILE), vs=vs, color=color)
            conditions.write_condition_pngs(inst, conditions.conditions_statement(torch.from_numpy(vs)[None], torch.from_numpy(color)[None],
                                                                                  torch.from_numpy(tris)), 0)
        for name, img in () if cond_mesh else zip(("front", "left", "right"), cond_images(1, 256, seed + 10 * k)):
            m = img[0, 6][..., None]
            render = np.floor(img[0, 0:3].transpose(1, 2, 0) * m * 255 + 0.5).astype(np.uint8)
            normal = np.floor((0.02 + 0.98 * img[0, 3:6].transpose(1, 2, 0)) * m * 255 + 0.5).astype(np.uint8)
            imgio.imwrite_rgb(os.path.join(inst, "ortho_%s_render_256_baseGama.png" % name), render)
            imgio.imwrite_rgb(os.path.join(inst, "ortho_%s_normal_256_baseGama.png" % name), normal)
        R = euler_deg_to_R(20.0 * math.sin(2.0 * math.pi * k / 64.0), -8.0, 3.0)
        head = np.eye(4)
        head[:3, :3], head[:3, 3] = R.T, (0.02, -0.03, 0.01)      # stored for row vectors p.T ("right-multiplied", dataloader.py:203)
        infos = []
        for v in views:
            cx, cy, rad = img_res * (0.5 + 0.02 * k), img_res * 0.48, img_res * 0.3
            d2 = ((xx - cx) ** 2 + (yy - cy) ** 2) / rad ** 2
            mask = (d2 < 1.0)
            shade = np.sqrt(np.clip(1.0 - d2, 0.0, 1.0))
            photo = np.stack([0.8 * shade, 0.6 * shade + 0.1, 0.5 * shade + 0.2], -1) * mask[..., None]
            fp, mp = os.path.join(inst, "img_%s.png" % v), os.path.join(inst, "mask_%s.png" % v)
            if photos:
                imgio.imwrite_rgb(fp, np.floor(photo * 255 + 0.5).astype(np.uint8))
                imgio.imwrite_rgb(mp, np.repeat((mask * 255).astype(np.uint8)[..., None], 3, -1))
            infos.append({"view_name": v, "transform_matrix": c2w, "transform_matrix_ori": c2w, "file_path": fp, "mask_path": mp})
        frames.append({"fidx": k, "inst_dir": inst, "head_transformation": head.tolist(), "mutiview_info_ls": infos})
    meta = {"img_res": img_res, "mutiview_intr_ls": [[focal * img_res, focal * img_res, 0.5, 0.5] for _ in views], "frames": frames}
    path = os.path.join(root, "sv_v31_all.json")
    with open(path, "w") as f:
        json.dump(meta, f)
    return path


def harness_config(render_size=32, gen_size=128, img_res=128, perturb=False, noise_std=0.0, rays=256):
    """Config dict (the reference's YAML layout) for the harness tests / demos: a `img_res` dataset rendered at
    `render_size` (down_sample = render_size / img_res), stage-two output `gen_size`, deterministic sampling by default."""
    import copy
    import os

    import yaml
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "config", "hd_base.yml")) as f:
        cfg = copy.deepcopy(yaml.safe_load(f))
    cfg["dataset"].update(down_sample=render_size / img_res, num_random_rays=rays)
    cfg["models"]["StyleUnet"].update(inp_size=render_size, out_size=gen_size)
    cfg["models"]["coarse"]["Head_bounding"] = [[-1.2, 1.2], [-1.6, 1.0], [-1.6, 1.2]]
    cfg["experiment"].update(train_iters=4, validate_every=1000, save_every=1000, print_every=1, mask_weight=0.01, rgb_loss="mse",
                             patch_rgb=False)
    cfg["optimizer"] = {"type": "Adam", "lr": 5.0e-4}
    cfg["scheduler"] = {"lr_decay": 250, "lr_decay_factor": 0.1}
    for mode in ("train", "validation"):
        cfg["nerf"][mode].update(perturb=bool(perturb), radiance_field_noise_std=float(noise_std) if mode == "train" else 0.0)
    return cfg


def zero_noise_weights(state_dict):
    """Set every NoiseInjection strength to 0 (in place): the generators' per-call random noise then has no effect, which
    makes a harness run reproducible without pinning RNG streams."""
    for k in state_dict:
        if k.endswith("noise.weight"):
            state_dict[k].zero_()
    return state_dict

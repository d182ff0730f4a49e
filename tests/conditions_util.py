"""Shared by tests/test_conditions_cpu.py and tests/test_conditions_gpu.py: the condition-image definition restated in plain float64 loops,
pixel by pixel and triangle by triangle, and the scenes both files render."""
import math

import numpy as np
import torch

from havatar_amd import conditions as cd
from havatar_amd.utils.util import get_box_warp_param

UNIT = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))          # scale 1, trans 0: the front view's screen coordinates are the vertices


def loops(verts, colors, tris, res, rots=cd.ORTHO_ROTS, bounds=cd.ORTHO_BOUNDS, cam_dist=10.0):
    """the definition of havatar_amd/conditions.py in Python floats (IEEE double, every operation rounded on its own): dict of numpy arrays"""
    verts, colors, tris = np.asarray(verts, np.float64), np.asarray(colors, np.float64), np.asarray(tris, np.int64)
    B, V = verts.shape[:2]
    H = W = res
    scale, trans = get_box_warp_param(*bounds)
    face = np.full((B, 3, H, W), -1, np.int32)
    D = np.full((B, 3, H, W), -1.0)
    bary = np.zeros((B, 3, H, W, 3))
    normal = np.zeros((B, 3, H, W, 3))
    render8 = np.zeros((B, 3, H, W, 3), np.uint8)
    normal8 = np.zeros((B, 3, H, W, 3), np.uint8)
    cond = np.zeros((B, 3, 7, H, W))
    fin = math.isfinite
    for b in range(B):
        col = colors[b] if colors.ndim == 3 else colors
        for k in range(3):
            R = rots[k]
            scr = []
            for v in range(V):
                x, y, z = (float(verts[b, v, c]) * scale[c] + trans[c] for c in range(3))
                r = [(x * R[0][c] + y * R[1][c]) + z * R[2][c] for c in range(3)]
                scr.append((r[0], r[1], r[2] + cam_dist))
            for i in range(H):
                Y = (2 * i + 1) / H - 1
                for j in range(W):
                    X = (2 * j + 1) / W - 1
                    best = None
                    for f, (ia, ib, ic) in enumerate(tris.tolist()):
                        if not (0 <= ia < V and 0 <= ib < V and 0 <= ic < V):
                            continue
                        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = scr[ia], scr[ib], scr[ic]
                        if not all(fin(t) for t in (ax, ay, az, bx, by, bz, cx, cy, cz)):
                            continue
                        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
                        if area == 0:
                            continue
                        if not (min(ax, bx, cx) <= X <= max(ax, bx, cx) and min(ay, by, cy) <= Y <= max(ay, by, cy)):
                            continue
                        w0 = (bx - X) * (cy - Y) - (by - Y) * (cx - X)
                        w1 = (cx - X) * (ay - Y) - (cy - Y) * (ax - X)
                        w2 = (ax - X) * (by - Y) - (ay - Y) * (bx - X)
                        b0, b1, b2 = w0 / area, w1 / area, w2 / area
                        if not (b0 >= 0 and b1 >= 0 and b2 >= 0):
                            continue
                        z = (b0 * az + b1 * bz) + b2 * cz
                        if not z >= 0:
                            continue
                        z = z + 0.0          # -0 -> +0
                        if best is None or z < best[0]:          # ascending f: a tie keeps the smaller index
                            best = (z, f, b0, b1, b2)
                    if best is not None:
                        z, f, b0, b1, b2 = best
                        face[b, k, i, j], D[b, k, i, j], bary[b, k, i, j] = f, z, (b0, b1, b2)
                        ia, ib, ic = tris[f]
                        for c in range(3):
                            v = (b0 * float(col[ia, c]) + b1 * float(col[ib, c])) + b2 * float(col[ic, c])
                            render8[b, k, i, j, c] = 0 if v != v else int(min(max(v, 0.0), 255.0))
            dx, dy = -2.0 / W, -2.0 / H

            def nrm(u):
                n = math.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
                d = max(n, 1e-8)
                return [u[0] / d, u[1] / d, u[2] / d]

            def cross(u, v):
                return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            for i in range(1, H - 1):
                for j in range(1, W - 1):
                    p = lambda ii, jj: (jj * dx, ii * dy, float(D[b, k, ii, jj]))
                    sub = lambda u, v: [u[0] - v[0], u[1] - v[1], u[2] - v[2]]
                    c0 = p(i, j)
                    vw, vs, ve, vn = sub(c0, p(i, j + 1)), sub(p(i + 1, j), c0), sub(c0, p(i, j - 1)), sub(p(i - 1, j), c0)
                    n1, n2 = nrm(cross(vs, vw)), nrm(cross(vn, ve))
                    normal[b, k, i, j] = nrm([n1[0] + n2[0], n1[1] + n2[1], n1[2] + n2[2]])
            for i in range(H):
                for j in range(W):
                    if face[b, k, i, j] >= 0 and all(render8[b, k, i, j] != 0):
                        normal8[b, k, i, j] = [int((float(n) + 1.0) * 127.5) for n in normal[b, k, i, j]]
            cond[b, k, 0:3] = render8[b, k].transpose(2, 0, 1) / 255.0
            cond[b, k, 3:6] = normal8[b, k].transpose(2, 0, 1) / 255.0
            cond[b, k, 6] = (normal8[b, k] > 0).any(-1)
    return dict(face=face, z=D, normal=normal, render8=render8, normal8=normal8, cond=cond, bary=bary)


# ------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------------------------
def uv_sphere(n_lat, n_lon, radius=0.8, centre=(0.0, 0.0, 0.0), squash=(1.0, 1.0, 1.0)):
    """(verts [V,3] float64, tris [F,3] int64), F = 2 n_lon (n_lat - 1)"""
    th = np.linspace(0.0, math.pi, n_lat + 1)[1:-1]
    ph = np.arange(n_lon) * (2.0 * math.pi / n_lon) + 0.1234
    ring = np.stack([np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon)), np.outer(np.sin(th), np.cos(ph))], -1).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]], 0)
    last = 1 + (n_lat - 1) * n_lon
    tris = []
    for j in range(n_lon):
        jn = (j + 1) % n_lon
        tris.append((0, 1 + j, 1 + jn))
        tris.append((last, 1 + (n_lat - 2) * n_lon + jn, 1 + (n_lat - 2) * n_lon + j))
        for i in range(n_lat - 2):
            a, b, c, d = 1 + i * n_lon + j, 1 + i * n_lon + jn, 1 + (i + 1) * n_lon + j, 1 + (i + 1) * n_lon + jn
            tris += [(a, c, d), (a, d, b)]
    return unit * radius * np.asarray(squash) + np.asarray(centre), np.asarray(tris, np.int64)


def vertex_colors(verts, lo=20.0, hi=250.0):
    """smooth colours in [lo, hi] from the positions, one channel per axis"""
    v = np.asarray(verts, np.float64)
    span = np.maximum(np.nanmax(np.where(np.isfinite(v), v, np.nan), 0) - np.nanmin(np.where(np.isfinite(v), v, np.nan), 0), 1e-9)
    u = (np.where(np.isfinite(v), v, 0.0) - np.nanmin(np.where(np.isfinite(v), v, np.nan), 0)) / span
    return lo + (hi - lo) * np.clip(u, 0.0, 1.0)


def small_scene(name):
    """(verts [1,V,3], colors [V,3], tris [F,3], res, bounds) float64 / int64: the corner cases of the definition, in the unit box"""
    q = lambda x0, y0, x1, y1, z00, z10, z11, z01: [(x0, y0, z00), (x1, y0, z10), (x1, y1, z11), (x0, y1, z01)]
    res, bounds = 8, UNIT
    if name == "sphere":
        v, t = uv_sphere(5, 6, 0.8)
        res = 11
    elif name == "quads":          # two quads through each other: the winner changes along x
        v = q(-0.8, -0.7, 0.7, 0.6, -0.5, 0.5, 0.5, -0.5) + q(-0.6, -0.8, 0.8, 0.7, 0.4, -0.6, -0.6, 0.4)
        t = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]
        res = 9
    elif name == "duplicates":          # coincident triangles: a tie at every pixel, the lower index wins
        v = [(-0.9, -0.8, 0.2), (0.8, -0.6, 0.1), (0.1, 0.9, -0.3)]
        t = [(0, 1, 2), (0, 1, 2), (1, 2, 0), (0, 1, 2)]          # the rotated copy's z may differ in the last bit
    elif name == "diagonal":          # W = 8: the quad's corners and its diagonal lie on pixel centres
        v = q(-0.875, -0.875, 0.875, 0.875, 0.25, 0.25, 0.25, 0.25)
        t = [(0, 1, 2), (0, 2, 3)]
    elif name == "windings":
        v = [(-0.9, -0.9, 0.0), (-0.1, -0.9, 0.1), (-0.5, 0.1, 0.2), (0.1, -0.2, 0.0), (0.9, -0.2, -0.1), (0.5, 0.9, 0.3)]
        t = [(0, 1, 2), (3, 5, 4)]
    elif name == "subpixel":          # between centres: nothing is covered but by the one that holds a centre
        v = [(-0.86, -0.86, 0.0), (-0.80, -0.86, 0.0), (-0.83, -0.80, 0.0), (0.40, 0.40, 0.0), (0.60, 0.42, 0.0), (0.48, 0.60, 0.0),
             (0.05, 0.05, 0.1), (0.20, 0.08, 0.1), (0.12, 0.22, 0.1)]
        t = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
    elif name == "offscreen":          # partly and wholly outside the image, and one that holds the whole image
        v = [(-1.7, -0.3, 0.0), (-0.4, -0.9, 0.0), (-0.6, 0.6, 0.1), (1.2, 1.2, 0.0), (2.5, 1.3, 0.0), (1.8, 2.4, 0.0),
             (-5.0, -4.0, 0.5), (6.0, -4.5, 0.6), (0.3, 7.0, 0.7)]
        t = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
    elif name == "behind":          # zv = z + 10 < 0 on one triangle, across zero on the other
        v = [(-0.8, -0.8, -12.0), (0.8, -0.8, -12.0), (0.0, 0.8, -11.0), (-0.9, -0.5, -10.5), (0.9, -0.5, -9.5), (0.0, 0.9, -9.5)]
        t = [(0, 1, 2), (3, 4, 5)]
    elif name == "degenerate":          # zero area, a repeated vertex, NaN and infinite vertices; one sound triangle
        v = [(-0.8, -0.8, 0.0), (0.0, 0.0, 0.0), (0.8, 0.8, 0.0), (float("nan"), 0.1, 0.0), (0.5, float("inf"), 0.0), (-0.7, 0.6, 0.1),
             (0.7, -0.6, 0.2), (0.6, 0.7, 0.0), (0.2, 0.1, float("nan"))]
        t = [(0, 1, 2), (0, 0, 5), (3, 5, 6), (4, 5, 6), (5, 6, 8), (5, 6, 7)]
    else:
        raise KeyError(name)
    v = np.asarray(v, np.float64)
    return v[None], vertex_colors(v), np.asarray(t, np.int64), res, bounds


SMALL_SCENES = ("sphere", "quads", "duplicates", "diagonal", "windings", "subpixel", "offscreen", "behind", "degenerate")


def tensors(verts, colors, tris, dtype=torch.float32, device="cpu"):
    return (torch.as_tensor(np.asarray(verts), dtype=dtype, device=device).contiguous(),
            torch.as_tensor(np.asarray(colors), dtype=dtype, device=device).contiguous(),
            torch.as_tensor(np.asarray(tris), dtype=torch.int32, device=device).contiguous())


def normals64(z32):
    """The yardstick of float32 normals: the float64 definition given float32's decisions -- step 8 in float64 on float32's depth map
    (which holds its `face` and `z`).  [B,3,H,W,3] float64 on the CPU."""
    res = z32.shape[-1]
    return cd.depth_normals(z32.detach().cpu().double(), -2.0 / res, -2.0 / res)


def check_normals(got, cpu32, label=""):
    """`got` (a Conditions whose face, z and render8 already equal cpu32's) against the float64 yardstick: the float normal within twice
    the CPU float32 statement's own error + 1e-6; the codes equal to float64's, or one off where float64's (n + 1) 127.5 lies within
    127.5 x that bar of an integer -- on at most 2 % of the covered pixels.  Prints both error figures."""
    n64 = normals64(cpu32.z)
    e_cpu = float((cpu32.normal.double() - n64).abs().max())
    e_got = float((got.normal.cpu().double() - n64).abs().max())
    bar = 2.0 * e_cpu + 1e-6
    print("%s normal: worst component error %.3e, the CPU float32 statement's %.3e, bar %.3e" % (label, e_got, e_cpu, bar))
    assert e_got <= bar
    covered = cpu32.face >= 0
    keep = (covered & (cpu32.render8 != 0).all(-1))[..., None]
    val = (n64 + 1.0) * 127.5
    code64 = torch.where(keep, val.floor(), torch.zeros_like(val))
    diff = (got.normal8.cpu().double() - code64).abs()
    near = (val - val.round()).abs() <= 127.5 * bar
    assert bool(((diff == 0) | ((diff == 1) & near & keep)).all()), "a normal code differs from float64's away from a rounding boundary"
    off = int((diff != 0).any(-1).sum())
    print("%s normal8: %d of %d covered pixels one code off float64's" % (label, off, int(covered.sum())))
    assert off <= 0.02 * max(int(covered.sum()), 1)
    # cond follows from the codes bit for bit
    g = got.cond.cpu()
    assert torch.equal(g[:, :, 0:3], got.render8.cpu().permute(0, 1, 4, 2, 3).float() / 255.0)
    assert torch.equal(g[:, :, 3:6], got.normal8.cpu().permute(0, 1, 4, 2, 3).float() / 255.0)
    assert torch.equal(g[:, :, 6], (got.normal8.cpu() > 0).any(-1).float())
    return e_got, e_cpu

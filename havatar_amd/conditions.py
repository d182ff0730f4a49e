"""Condition images from a tracked mesh: the three orthographic renders of the fitted 3DMM head that drive the renderer
(`ortho_{front,left,right}_{render,normal}_256_baseGama.png`, the `[B,7,256,256]` `*_render_cond` tensors), rasterised here instead of
offline with pytorch3d (reference: data_preprocessing/fit_video.py::render_canonical_ortho, core/FaceVerseModel_v3.py::get_renderer,
core/utils.py::depth2normal_ortho).

Definition (DESIGN.md 7.13 derives the camera; `conditions_statement` states it on ATen, tests/test_conditions_cpu.py in plain loops, and
csrc/hav_raster.hip is held to the same operations in the same order):
  1 warp     w = v * scale + trans with get_box_warp_param(*bounds)
  2 view     r = w @ R per view, summed as (x R0c + y R1c) + z R2c
  3 depth    zv = r.z + cam_dist
  4 pixels   pixel (i, j) samples X_j = (2 j + 1) / W - 1, Y_i = (2 i + 1) / H - 1
  5 cover    per triangle (a, b, c): area = (bx-ax)(cy-ay) - (by-ay)(cx-ax); skipped when area == 0, a coordinate is not finite or an index
             lies outside [0, V).  w0 = (bx-X)(cy-Y) - (by-Y)(cx-X), w1 = (cx-X)(ay-Y) - (cy-Y)(ax-X), w2 = (ax-X)(by-Y) - (ay-Y)(bx-X),
             b_k = w_k / area.  Covered iff every b_k >= 0 and X, Y lie in the closed bounding box of the three vertices.
             z = (b0 za + b1 zb) + b2 zc; hits with !(z >= 0) are dropped, -0 becomes +0.  The smallest z wins, a tie goes to the smaller index.
  6 colour   c = (b0 ca + b1 cb) + b2 cc; render8 = trunc(clamp(c, 0, 255)), NaN -> 0
  7 depth    D = z where covered, -1 elsewhere
  8 normal   depth2normal_ortho with dx = -2 / W, dy = -2 / H on p = (j dx, i dy, D); border pixels 0; normal8 = trunc((n + 1) 127.5), then
             0 where the pixel is uncovered or a render8 channel is 0
  9 cond     render8 / 255, normal8 / 255, any(normal8 > 0)

  python -m havatar_amd.conditions --split S --tri T [--device D]      writes the six PNGs of every frame of a split from its cond_mesh.npz
"""
import collections
import os

import numpy as np
import torch

from .utils.util import get_box_warp_param

ORTHO_BOUNDS = ((-1.5, 1.5), (-1.6, 1.4), (-1.6, 1.2))          # fit_video.py:108
# r = w @ R: front r = (x, y, z); left r = (-z, y, x); right r = (z, y, -x).  Exact quarter turns: the reference's float32 cos(pi/2) is dropped.
ORTHO_ROTS = (((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
              ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0)),
              ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
VIEWS = ("front", "left", "right")
MESH_FILE = "cond_mesh.npz"

Conditions = collections.namedtuple("Conditions", "face z normal render8 normal8 cond")


def png_names(view):
    return "ortho_%s_render_256_baseGama.png" % view, "ortho_%s_normal_256_baseGama.png" % view


# ------------------------------------------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------------------------------------------
class Topology:
    """The triangle list of a tracked mesh, validated once on the host: tris [F,3] integer with every index in [0, V).  on(device) is an
    int32 copy there, made once per device."""

    def __init__(self, tris, V):
        t = torch.as_tensor(np.asarray(tris) if not torch.is_tensor(tris) else tris).detach().cpu()
        V = int(V)
        if t.dim() != 2 or t.shape[1] != 3 or t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError("Topology: tris is an integer [F,3] array (got %s %s)" % (t.dtype, tuple(t.shape)))
        if t.shape[0] == 0:
            raise ValueError("Topology: no triangle (F == 0)")
        if V < 1 or V >= 2 ** 31 or t.shape[0] >= 2 ** 31:
            raise ValueError("Topology: V = %d and F = %d must lie in [1, 2^31)" % (V, t.shape[0]))
        t = t.to(torch.int64)
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= V:
            raise ValueError("Topology: vertex indices span [%d, %d] but the mesh has V = %d vertices" % (lo, hi, V))
        self.V, self.F = V, int(t.shape[0])
        self.tris = t.to(torch.int32).contiguous()
        self._on = {}

    @classmethod
    def load(cls, path, V=None):
        t = np.load(path)
        if V is None:
            V = int(t.max()) + 1 if t.size and np.issubdtype(t.dtype, np.integer) else 1
        return cls(t, V)

    def on(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = self.tris.to(device)
        return self._on[device]


def _args(verts, colors, tris, res, rots, bounds, cam_dist):
    if not torch.is_tensor(verts) or verts.dtype not in (torch.float32, torch.float64) or verts.dim() != 3 or verts.shape[2] != 3 \
            or verts.shape[0] < 1 or verts.shape[1] < 1:
        raise ValueError("conditions: verts is a float32 or float64 tensor [B,V,3] (got %s)"
                         % ("%s %s" % (verts.dtype, tuple(verts.shape)) if torch.is_tensor(verts) else type(verts).__name__))
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if not torch.is_tensor(colors) or colors.dtype != verts.dtype or colors.device != verts.device \
            or tuple(colors.shape) not in ((B, V, 3), (V, 3)):
        raise ValueError("conditions: colors is [B,V,3] or [V,3] = [%d,%d,3] of the vertices' dtype on their device (got %s)"
                         % (B, V, "%s %s on %s" % (colors.dtype, tuple(colors.shape), colors.device) if torch.is_tensor(colors)
                            else type(colors).__name__))
    if isinstance(tris, Topology):
        if tris.V != V:
            raise ValueError("conditions: the topology was made for V = %d vertices, the mesh has %d" % (tris.V, V))
        tris = tris.on(verts.device)
    if not torch.is_tensor(tris) or tris.is_floating_point() or tris.dtype == torch.bool or tris.dim() != 2 or tris.shape[1] != 3 \
            or tris.shape[0] < 1 or tris.device != verts.device:
        raise ValueError("conditions: tris is an integer tensor [F >= 1, 3] on the vertices' device (got %s)"
                         % ("%s %s on %s" % (tris.dtype, tuple(tris.shape), tris.device) if torch.is_tensor(tris) else type(tris).__name__))
    res = int(res)
    if res < 1:
        raise ValueError("conditions: res >= 1 (got %d)" % res)
    rots = tuple(tuple(tuple(float(v) for v in row) for row in R) for R in rots)
    if len(rots) != 3 or any(len(R) != 3 or any(len(row) != 3 for row in R) for R in rots):
        raise ValueError("conditions: rots holds three 3 x 3 matrices")
    bounds = tuple((float(lo), float(hi)) for lo, hi in bounds)
    if len(bounds) != 3 or not all(np.isfinite(lo) and np.isfinite(hi) and hi > lo for lo, hi in bounds):
        raise ValueError("conditions: bounds holds three finite (lo, hi) pairs with hi > lo")
    cam_dist = float(cam_dist)
    if not np.isfinite(cam_dist):
        raise ValueError("conditions: cam_dist must be finite (got %r)" % cam_dist)
    return B, V, tris, res, rots, bounds, cam_dist


# ------------------------------------------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------------------------------------------
def _screen(verts, rots, bounds, cam_dist):
    """steps 1-3: [B,3,V,3] = (x, y, zv) per view"""
    dt, dev = verts.dtype, verts.device
    scale, trans = get_box_warp_param(*bounds)
    w = verts * torch.tensor(scale, dtype=dt, device=dev) + torch.tensor(trans, dtype=dt, device=dev)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    views = []
    for R in rots:
        r = [(x * R[0][c] + y * R[1][c]) + z * R[2][c] for c in range(3)]
        views.append(torch.stack([r[0], r[1], r[2] + cam_dist], -1))
    return torch.stack(views, 1)


def _centres(n, dt, dev):
    return (2 * torch.arange(n, device=dev) + 1).to(dt) / n - 1


def _corners(scr, tris, V):
    """the three corners of every triangle [B,3,F,3] each, and which triangles take part (step 5's skips)"""
    t = tris.to(torch.int64)
    inside = ((t >= 0) & (t < V)).all(1)
    t = t.clamp(0, V - 1)
    a, b, c = scr[:, :, t[:, 0]], scr[:, :, t[:, 1]], scr[:, :, t[:, 2]]
    area = (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    finite = torch.isfinite(a).all(-1) & torch.isfinite(b).all(-1) & torch.isfinite(c).all(-1)
    return a, b, c, area, inside & finite & (area != 0)


def _hit(a, b, c, area, live, X, Y):
    """step 5 for corners [..., 3] against pixel centres X, Y that broadcast with a[..., 0]: (hit, z, b0, b1, b2)"""
    ax, ay, bx, by, cx, cy = a[..., 0], a[..., 1], b[..., 0], b[..., 1], c[..., 0], c[..., 1]
    w0 = (bx - X) * (cy - Y) - (by - Y) * (cx - X)
    w1 = (cx - X) * (ay - Y) - (cy - Y) * (ax - X)
    w2 = (ax - X) * (by - Y) - (ay - Y) * (bx - X)
    b0, b1, b2 = w0 / area, w1 / area, w2 / area
    lo_x, hi_x = torch.minimum(torch.minimum(ax, bx), cx), torch.maximum(torch.maximum(ax, bx), cx)
    lo_y, hi_y = torch.minimum(torch.minimum(ay, by), cy), torch.maximum(torch.maximum(ay, by), cy)
    z = (b0 * a[..., 2] + b1 * b[..., 2]) + b2 * c[..., 2]
    z = torch.where(z == 0, torch.zeros_like(z), z)
    hit = live & (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (X >= lo_x) & (X <= hi_x) & (Y >= lo_y) & (Y <= hi_y) & (z >= 0)
    return hit, z, b0, b1, b2


def _cross(u, v):
    return torch.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                        u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _normalize(u):
    n = ((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]).sqrt()
    return u / torch.clamp(n, min=1e-8)[..., None]


def depth_normals(D, dx, dy):
    """step 8's float part: the reference's depth2normal_ortho on D [..., H, W] -> [..., H, W, 3], every operation rounded on its own"""
    H, W = D.shape[-2:]
    dt, dev = D.dtype, D.device
    xs = (torch.arange(W, device=dev).to(dt) * dx).expand(D.shape)
    ys = (torch.arange(H, device=dev).to(dt) * dy)[:, None].expand(D.shape)
    p = torch.stack([xs, ys, D], -1)
    out = torch.zeros_like(p)
    if H < 3 or W < 3:
        return out
    ctr = p[..., 1:-1, 1:-1, :]
    vw = ctr - p[..., 1:-1, 2:, :]
    vs = p[..., 2:, 1:-1, :] - ctr
    ve = ctr - p[..., 1:-1, :-2, :]
    vn = p[..., :-2, 1:-1, :] - ctr
    out[..., 1:-1, 1:-1, :] = _normalize(_normalize(_cross(vs, vw)) + _normalize(_cross(vn, ve)))
    return out


def finish(scr, colors, tris, V, face, res):
    """steps 5 (the winner's barycentrics, recomputed) to 9 from the winning face per pixel: the part of the definition that follows the
    depth test.  A float64 call with float32's `face` is the yardstick of float32's normals."""
    dt, dev = scr.dtype, scr.device
    B = scr.shape[0]
    H = W = res
    X, Y = _centres(W, dt, dev)[None, None, None, :], _centres(H, dt, dev)[None, None, :, None]
    covered = face >= 0
    f = face.clamp(min=0).to(torch.int64).reshape(B, 3, H * W)
    t = tris.to(torch.int64).clamp(0, V - 1)
    idx = [t[:, k][f] for k in range(3)]                                    # [B,3,HW] vertex indices of the winner
    pick = lambda k: torch.gather(scr, 2, idx[k][..., None].expand(-1, -1, -1, 3)).reshape(B, 3, H, W, 3)
    a, b, c = pick(0), pick(1), pick(2)
    area = (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    _, z, b0, b1, b2 = _hit(a, b, c, area, covered, X, Y)
    col = colors if colors.dim() == 3 else colors[None].expand(B, -1, -1)
    cpick = lambda k: torch.gather(col[:, None].expand(-1, 3, -1, -1), 2, idx[k][..., None].expand(-1, -1, -1, 3)).reshape(B, 3, H, W, 3)
    cc = (b0[..., None] * cpick(0) + b1[..., None] * cpick(1)) + b2[..., None] * cpick(2)
    cc = torch.where(torch.isnan(cc), torch.zeros_like(cc), cc.clamp(0, 255))
    render8 = torch.where(covered[..., None], cc, torch.zeros_like(cc)).to(torch.uint8)
    D = torch.where(covered, z, torch.full_like(z, -1.0))
    normal = depth_normals(D, -2.0 / W, -2.0 / H)
    keep = covered & (render8 != 0).all(-1)
    normal8 = torch.where(keep[..., None], (normal + 1.0) * 127.5, torch.zeros_like(normal)).to(torch.uint8)
    mask = (normal8 > 0).any(-1)
    cond = torch.cat([render8.to(dt).permute(0, 1, 4, 2, 3) / 255.0, normal8.to(dt).permute(0, 1, 4, 2, 3) / 255.0,
                      mask.to(dt)[:, :, None]], 2)
    return Conditions(face, D, normal, render8, normal8, cond)


def conditions_statement(verts, colors, tris, res=256, rots=ORTHO_ROTS, bounds=ORTHO_BOUNDS, cam_dist=10.0, chunk_elems=1 << 22):
    """The definition (module docstring) on ATen, in the vertices' dtype on their device: Conditions(face [B,3,H,W] int32, -1 for none;
    z [B,3,H,W], the depth map D; normal [B,3,H,W,3]; render8, normal8 [B,3,H,W,3] uint8; cond [B,3,7,H,W]).  The depth test runs over
    chunks of triangles, each on the pixel rectangle that holds the chunk's bounding boxes -- exact, since a pixel outside a triangle's
    bounding box is not covered by definition."""
    B, V, tris, res, rots, bounds, cam_dist = _args(verts, colors, tris, res, rots, bounds, cam_dist)
    with torch.no_grad():
        dt, dev = verts.dtype, verts.device
        H = W = res
        scr = _screen(verts, rots, bounds, cam_dist)
        a, b, c, area, live = _corners(scr, tris, V)
        F = tris.shape[0]
        Xs, Ys = _centres(W, dt, dev), _centres(H, dt, dev)
        best_z = torch.full((B, 3, H, W), float("inf"), dtype=dt, device=dev)
        face = torch.full((B, 3, H, W), -1, dtype=torch.int32, device=dev)
        # pixel rectangle of a triangle: the centres inside its closed bounding box (searchsorted on the exact centres, nothing is rounded)
        xy = torch.stack([a[..., :2], b[..., :2], c[..., :2]], 0)
        lo, hi = xy.amin(0), xy.amax(0)
        nan0 = lambda t_, v: torch.where(torch.isfinite(t_), t_, torch.full_like(t_, v))
        j0 = torch.searchsorted(Xs, nan0(lo[..., 0], 2.0).contiguous(), right=False)
        j1 = torch.searchsorted(Xs, nan0(hi[..., 0], -2.0).contiguous(), right=True)
        i0 = torch.searchsorted(Ys, nan0(lo[..., 1], 2.0).contiguous(), right=False)
        i1 = torch.searchsorted(Ys, nan0(hi[..., 1], -2.0).contiguous(), right=True)
        some = live & (j1 > j0) & (i1 > i0)
        big = torch.iinfo(torch.int64).max
        step = max(1, min(F, 64))
        for s in range(0, F, step):
            e = min(s + step, F)
            m = some[:, :, s:e]
            if not bool(m.any()):
                continue
            y0, y1 = int(torch.where(m, i0[:, :, s:e], big).min()), int(torch.where(m, i1[:, :, s:e], 0).max())
            x0, x1 = int(torch.where(m, j0[:, :, s:e], big).min()), int(torch.where(m, j1[:, :, s:e], 0).max())
            rows = max(1, chunk_elems // max(1, B * 3 * (x1 - x0) * (e - s)))
            for r0 in range(y0, y1, rows):
                r1 = min(r0 + rows, y1)
                X, Y = Xs[None, None, None, x0:x1, None], Ys[None, None, r0:r1, None, None]
                sl = lambda t_: t_[:, :, None, None, s:e]
                hit, z, _, _, _ = _hit(sl(a), sl(b), sl(c), sl(area), sl(live), X, Y)          # [B,3,rows,cols,chunk]
                zc = torch.where(hit, z, torch.full_like(z, float("inf")))
                zmin = zc.amin(-1)
                ids = torch.arange(s, e, device=dev, dtype=torch.int32)
                first = torch.where(hit & (zc == zmin[..., None]), ids, torch.full_like(ids, 2 ** 31 - 1)).amin(-1)
                bz, bf = best_z[:, :, r0:r1, x0:x1], face[:, :, r0:r1, x0:x1]
                better = hit.any(-1) & ((bf < 0) | (zmin < bz))          # later chunks hold larger indices: a tie keeps the earlier face
                best_z[:, :, r0:r1, x0:x1] = torch.where(better, zmin, bz)
                face[:, :, r0:r1, x0:x1] = torch.where(better, first, bf)
        return finish(scr, colors, tris, V, face, res)


def render_conditions(verts, colors, tris, res=256, rots=ORTHO_ROTS, bounds=ORTHO_BOUNDS, cam_dist=10.0):
    """Conditions(...) of B tracked meshes: verts [B,V,3] in the fitted model's space, colors [B,V,3] or [V,3] in 0...255, tris [F,3] integer
    (or a Topology).  Contiguous float32 HIP tensors take the kernels (native/raster_ops.py): three launches for all B x 3 views on the
    current stream, nothing read back.  Any other tensor takes the ATen statement."""
    B, V, tris, res, rots, bounds, cam_dist = _args(verts, colors, tris, res, rots, bounds, cam_dist)
    with torch.no_grad():
        if verts.is_cuda and verts.dtype == torch.float32 and verts.is_contiguous() and colors.is_contiguous():
            from .native import raster_ops
            if tris.dtype != torch.int32 or not tris.is_contiguous():
                tris = tris.to(torch.int32).contiguous()
            out = raster_ops.raster(verts, colors, tris, res, rots, bounds, cam_dist, outputs=Conditions._fields)
            return Conditions(*[out[k] for k in Conditions._fields])
        return conditions_statement(verts, colors, tris, res, rots, bounds, cam_dist)


# ------------------------------------------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------------------------------------------
def read_cond_mesh(inst_dir, V=None):
    """(vs [V,3], color [V,3]) float32 of <inst_dir>/cond_mesh.npz: pred_dict['vs'] and pred_dict['color'] of the reference's fit"""
    path = os.path.join(inst_dir, MESH_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing: mesh mode (--cond-mesh) reads every frame's tracked vertices `vs` [V,3] and colours `color` "
                                "[V,3] from it" % path)
    with np.load(path) as f:
        if "vs" not in f or "color" not in f:
            raise ValueError("%s holds %s; it must hold `vs` [V,3] and `color` [V,3]" % (path, sorted(f.keys())))
        vs, color = np.asarray(f["vs"], np.float32), np.asarray(f["color"], np.float32)
    vs, color = vs.reshape(-1, 3) if vs.ndim == 3 and vs.shape[0] == 1 else vs, color.reshape(-1, 3) if color.ndim == 3 and color.shape[0] == 1 else color
    if vs.ndim != 2 or vs.shape[1] != 3 or color.shape != vs.shape:
        raise ValueError("%s: vs %s and color %s must both be [V,3]" % (path, vs.shape, color.shape))
    if V is not None and vs.shape[0] != V:
        raise ValueError("%s holds %d vertices, the topology has %d" % (path, vs.shape[0], V))
    return vs, color


def write_condition_pngs(inst_dir, out, b=0):
    """the six files of sample b of a Conditions under the reference's names; returns their paths"""
    from .dataloader import imgio
    os.makedirs(inst_dir, exist_ok=True)
    r8, n8 = out.render8[b].cpu().numpy(), out.normal8[b].cpu().numpy()
    paths = []
    for v, view in enumerate(VIEWS):
        for name, arr in zip(png_names(view), (r8[v], n8[v])):
            paths.append(os.path.join(inst_dir, name))
            imgio.imwrite_rgb(paths[-1], np.ascontiguousarray(arr))
    return paths


def main(argv=None):
    import argparse
    import json
    p = argparse.ArgumentParser(description="Write the six condition PNGs of every frame of a split from its cond_mesh.npz.")
    p.add_argument("--split", required=True, help="Split file (json).")
    p.add_argument("--tri", required=True, help="Topology: an integer [F,3] .npy file.")
    p.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    p.add_argument("--cam-dist", type=float, default=10.0)
    args = p.parse_args(argv)
    with open(args.split) as f:
        frames = json.load(f)["frames"]
    topo, written = None, []
    for fd in frames:
        vs, color = read_cond_mesh(fd["inst_dir"], None if topo is None else topo.V)
        if topo is None:
            topo = Topology.load(args.tri, vs.shape[0])
        dev = torch.device(args.device)
        out = render_conditions(torch.from_numpy(vs)[None].to(dev), torch.from_numpy(color)[None].to(dev), topo, cam_dist=args.cam_dist)
        written += write_condition_pngs(fd["inst_dir"], out, 0)
    print("%d frames, %d files" % (len(frames), len(written)))
    return written


if __name__ == "__main__":
    main()

"""Geometry export: the avatar's density field as a triangle mesh.  No reference counterpart (the only geometry file the reference writes is
the 20^3 .obj lattice of visualize_motion_weight_vol).

  density(trainer, pts, inv_head_T)            sigma at arbitrary points: skinning field -> tri-plane features -> radiance MLP, relu(alpha)
  density_grid(trainer, inv_head_T, res)       that on a lattice over the canonical box, or over the posed box of one frame
  isosurface(field, iso, origin, spacing)      marching tetrahedra on the Kuhn subdivision (definition below)
  extract_mesh(trainer, inv_head_T)            grid -> iso-surface -> vertex colours (the radiance takes no view direction: one colour)
  write_ply / read_ply                         binary little-endian PLY, numpy only

Contiguous float32 HIP fields take the kernels of csrc/hav_isosurface.hip (native/iso_ops.py, no fallback in there); every other tensor takes
the vectorised ATen statement of the same definition in this file, in the same order.  HIP float32 points take native/train_ops.field_inputs +
the MLP; every other tensor the modules' own forward.

Definition of the iso-surface (include/havatar.h carries it too; tests/test_isosurface_cpu.py restates it in plain loops).
  f [D0,D1,D2], every D >= 2; lattice point (i,j,k): n = (i D1 + j) D2 + k at origin + (i,j,k) spacing.  Inside iff f > iso (NaN: outside).
  Point n owns the edges n -> n + d, d in {0,1}^3 \\ {0}, e = 4 di + 2 dj + dk - 1.  An edge inside the grid whose ends differ in inside-ness
  carries a vertex at t = (iso - f[n]) / (f[n+d] - f[n]) (field dtype; 0.5 when not finite, else clamped to [0,1]), ordered by n, then e.
  The cube at n splits into six tetrahedra, one per permutation (a1,a2,a3) of the axes in lexicographic order, c0 = n, c1 = c0 + e_a1,
  c2 = c1 + e_a2, c3 = c2 + e_a3.  I / O = inside / outside corners in c0..c3 order, (p,q) = the vertex between corners p and q:
  |I| = 1: (I0,O0),(I0,O1),(I0,O2); |I| = 3: (O0,I0),(O0,I1),(O0,I2); |I| = 2: (I0,O0),(I0,O1),(I1,O1) then (I0,O0),(I1,O1),(I1,O0).  The
  last two entries are swapped where that makes the right-handed normal (crossings at edge midpoints, index space) point from the inside
  corners' centroid to the outside corners': a table of (tetrahedron, case).  Triangles are ordered by n, tetrahedron, first / second.
  Normal of a vertex: -(g(n) + t (g(n+d) - g(n))) normalised, g = central difference (one-sided at a face) / spacing; (0,0,0) when the
  length is zero or not finite.

  gbuffer(rays, depth, acc, H, W, acc_min)     image-space geometry of rendered frames: metric depth, camera-facing normals, headlight shade
  gbuffer_statement(...)                       the same on ATen, in any dtype; decode_depth16 reads the 16-bit codes back

Contiguous float32 HIP maps take the kernel of csrc/hav_gbuffer.hip (native/gbuffer_ops.py, no fallback in there), every other tensor the
statement.

Definition of the G-buffer (include/havatar.h carries it too; tests/test_gbuffer_cpu.py restates it in plain loops).
  rays [B, H W, stride >= 8]: origin 0-2, unit direction 3-5, near 6, far 7 -- the table the march reads; depth [B, H W] = sum w z,
  acc [B, H W] = sum w; pixel q = (y, x) is row-major.
  valid(q) = acc > acc_min and isfinite(depth): strict, NaN is invalid.
  z(q) = min(max(depth / acc, near), far) where valid, else 0 (r < near ? near : r, then > far ? far : that: a NaN quotient stays NaN).
  p(q) = o + d z.
  Tangent along an axis (x: neighbours (y, x +- 1); y: (y +- 1, x)).  A side is usable if the neighbour is inside the image and the neighbour
  and q are both valid.  a+ = |z(q+) - z(q)|, a- = |z(q) - z(q-)|.
    both usable and max(a+, a-) <= 4 min(a+, a-): central, t = p(q+) - p(q-)  (times 4 is exact, so the choice is);
    otherwise the usable side with the smaller a, a tie going to +: t = p(q+) - p(q) or p(q) - p(q-);  no usable side: no tangent.
    The choice keeps silhouettes and depth steps from smearing into the normals next to them.
  n = tx x ty, negated where n . d(q) > 0, so it faces the camera; normal = n / |n| where both tangents exist and |n| is finite and positive,
  else (0,0,0).
  mask: bit 0 = valid, bit 1 = has a normal.  depth16 [..,2] uint8, high byte first: 0 where invalid, else
  1 + round((z - near) / (far - near) 65534) clamped to [1, 65535].  normal8 = round((n 0.5 + 0.5) 255), (0,0,0) without a normal.
  shade8 = round(255 max(0, -normal . d)), 255 without a normal.  round: to nearest, ties to even."""
import collections
import functools

import numpy as np
import torch

# Default level of extract_mesh: the density at which one coarse step of the shipped configuration is half opaque, 1 - exp(-sigma delta) = 1/2
# with delta = (far - near) / (num_coarse - 1) = 2.6 / 63: sigma = ln 2 / delta = 16.8
DEFAULT_ISO = 16.8


# ------------------------------------------------------------------------------------------------------------------------------------
# the tables, generated from the definition
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """corner [6,4]: cube-corner offset 4 di + 2 dj + dk of corner c of tetrahedron tau; cnt [6,16]: triangles of (tau, case), case bit c =
    corner c inside; own [6,16,2,3], edge [6,16,2,3]: owner corner offset and owned-edge number e of each triangle entry, winding applied"""
    perms = [(a, b, 3 - a - b) for a in range(3) for b in range(3) if b != a]          # ascending loops: lexicographic
    corner = np.zeros((6, 4), np.int64)
    cnt = np.zeros((6, 16), np.int64)
    own = np.zeros((6, 16, 2, 3), np.int64)
    edge = np.zeros((6, 16, 2, 3), np.int64)
    pos = lambda off: np.array([(off >> 2) & 1, (off >> 1) & 1, off & 1])
    for tau, (a1, a2, _) in enumerate(perms):
        corner[tau] = (0, 4 >> a1, (4 >> a1) | (4 >> a2), 7)
        for case in range(16):
            I = [c for c in range(4) if (case >> c) & 1]
            O = [c for c in range(4) if not (case >> c) & 1]
            if len(I) == 1:
                tris = [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
            elif len(I) == 3:
                tris = [[(O[0], I[0]), (O[0], I[1]), (O[0], I[2])]]
            elif len(I) == 2:
                tris = [[(I[0], O[0]), (I[0], O[1]), (I[1], O[1])], [(I[0], O[0]), (I[1], O[1]), (I[1], O[0])]]
            else:
                tris = []
            cnt[tau, case] = len(tris)
            if not tris:
                continue
            out = np.mean([pos(corner[tau, c]) for c in O], 0) - np.mean([pos(corner[tau, c]) for c in I], 0)
            for s, tri in enumerate(tris):
                m = [0.5 * (pos(corner[tau, p]) + pos(corner[tau, q])) for p, q in tri]
                if np.dot(np.cross(m[1] - m[0], m[2] - m[0]), out) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                for v, (p, q) in enumerate(tri):
                    lo, hi = corner[tau, min(p, q)], corner[tau, max(p, q)]
                    own[tau, case, s, v], edge[tau, case, s, v] = lo, (hi ^ lo) - 1
    return corner, cnt, own, edge


# ------------------------------------------------------------------------------------------------------------------------------------
# the iso-surface
# ------------------------------------------------------------------------------------------------------------------------------------
def _gradient(f, spacing):
    """[3,D0,D1,D2]: central differences, one-sided at the faces, each axis divided by its spacing"""
    g = []
    for a in range(3):
        n = f.shape[a]
        fp = torch.cat([f.narrow(a, 1, n - 1), f.narrow(a, n - 1, 1)], a)
        fm = torch.cat([f.narrow(a, 0, 1), f.narrow(a, 0, n - 1)], a)
        den = torch.full((n,), 2.0, dtype=f.dtype, device=f.device)
        den[0] = den[-1] = 1.0
        shape = [1, 1, 1]
        shape[a] = n
        g.append((fp - fm) / (den * spacing[a]).reshape(shape))
    return torch.stack(g, 0)


def isosurface_statement(field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals=True, aux=None):
    """the definition on ATen, vectorised, in the field's dtype and on its device: (verts [V,3], tris [T,3] int32, normals [V,3] | None).
    aux: a dict that receives the conditioning of the normals, "length" [V] (before normalisation) and "gsum" [V] (sum of |g(n)| + |g(n+d)|
    over the axes) -- an error of the gradients of eps gsum turns the normal by about eps gsum / length"""
    f = field
    dev, dt = f.device, f.dtype
    D0, D1, D2 = f.shape
    corner, cnt, own, edge = (torch.from_numpy(t).to(dev) for t in tables())
    o = torch.tensor([float(v) for v in origin], dtype=dt, device=dev)
    h = torch.tensor([float(v) for v in spacing], dtype=dt, device=dev)
    if dt == torch.float32:
        iso = float(np.float32(iso))          # the level in the field's precision, as the kernels take it
    inside = f > iso
    lin = lambda off: ((off >> 2) & 1) * (D1 * D2) + ((off >> 1) & 1) * D2 + (off & 1)
    # vertices: the crossing mask [N,7], numbered in (n, e) order
    cross = torch.zeros(D0, D1, D2, 7, dtype=torch.bool, device=dev)
    for e in range(7):
        di, dj, dk = ((e + 1) >> 2) & 1, ((e + 1) >> 1) & 1, (e + 1) & 1
        cross[:D0 - di, :D1 - dj, :D2 - dk, e] = inside[:D0 - di, :D1 - dj, :D2 - dk] != inside[di:, dj:, dk:]
    cross = cross.reshape(-1)
    vid = torch.cumsum(cross, 0) - 1          # [N*7] int64: the vertex on edge (n, e) where cross
    sel = cross.nonzero()[:, 0]
    vn, ve = sel // 7, sel % 7
    V = int(sel.numel())
    if V == 0:
        z = torch.zeros(0, 3, dtype=dt, device=dev)
        return z, torch.zeros(0, 3, dtype=torch.int32, device=dev), (z.clone() if normals else None)
    d = torch.stack([((ve + 1) >> 2) & 1, ((ve + 1) >> 1) & 1, (ve + 1) & 1], 1)          # [V,3]
    vp = vn + lin(ve + 1)
    flat = f.reshape(-1)
    a, b = flat[vn], flat[vp]
    t = (iso - a) / (b - a)
    t = torch.where(torch.isfinite(t), t.clamp(0.0, 1.0), torch.full_like(t, 0.5))
    ijk = torch.stack([vn // (D1 * D2), (vn // D2) % D1, vn % D2], 1)
    verts = o + (ijk.to(dt) + t[:, None] * d.to(dt)) * h
    nrm = None
    if normals:
        g = _gradient(f, h).reshape(3, -1)
        g0, g1 = g[:, vn].t(), g[:, vp].t()
        nv = -(g0 + t[:, None] * (g1 - g0))
        length = nv.square().sum(1, keepdim=True).sqrt()
        ok = torch.isfinite(length) & (length > 0)
        nrm = torch.where(ok, nv / length, torch.zeros_like(nv))
        if aux is not None:
            aux.update(length=length[:, 0], gsum=g0.abs().sum(1) + g1.abs().sum(1))
    # triangles: the cubes with a mixed corner set, in n order
    bits = torch.zeros(D0 - 1, D1 - 1, D2 - 1, dtype=torch.int64, device=dev)
    for off in range(8):
        di, dj, dk = (off >> 2) & 1, (off >> 1) & 1, off & 1
        bits |= inside[di:D0 - 1 + di, dj:D1 - 1 + dj, dk:D2 - 1 + dk].to(torch.int64) << off
    act = ((bits != 0) & (bits != 255)).nonzero()
    cn = (act[:, 0] * D1 + act[:, 1]) * D2 + act[:, 2]          # ascending: nonzero() is row-major
    cb = bits[act[:, 0], act[:, 1], act[:, 2]]
    case = ((cb[:, None, None] >> corner[None]) & 1)          # [A,6,4]
    case = case[..., 0] | (case[..., 1] << 1) | (case[..., 2] << 2) | (case[..., 3] << 3)          # [A,6]
    tau = torch.arange(6, device=dev)[None].expand_as(case)
    c_own, c_edge, c_cnt = own[tau, case], edge[tau, case], cnt[tau, case]          # [A,6,2,3], [A,6]
    idx = vid[(cn[:, None, None, None] + lin(c_own)) * 7 + c_edge]          # [A,6,2,3]
    keep = torch.arange(2, device=dev)[None, None] < c_cnt[..., None]          # [A,6,2]
    tris = idx[keep].to(torch.int32)
    return verts, tris, nrm


def isosurface(field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals=True):
    """Iso-surface of field [D0,D1,D2] at level iso (inside = field > iso: the higher value, as for a density) by marching tetrahedra on the
    Kuhn subdivision -- the module docstring has the definition.  Returns (verts [V,3] field dtype, tris [T,3] int32, normals [V,3] | None);
    a field without a crossing returns empty tensors.  The mesh is watertight wherever the surface does not leave the grid, and consistently
    wound with outward normals (towards lower values).

    A contiguous float32 HIP field takes the HIP kernels (native/iso_ops.py): three launches and a cumsum, and ONE host read of the two totals
    (V, T) per call to size the outputs -- the call synchronises with the stream once.  Any other tensor takes the ATen statement."""
    if not torch.is_tensor(field) or field.dim() != 3 or not field.is_floating_point() or min(field.shape) < 2:
        raise ValueError("isosurface takes a floating-point field [D0,D1,D2] with every D >= 2 (got %s)"
                         % ((tuple(field.shape),) if torch.is_tensor(field) else type(field).__name__))
    iso = float(iso)
    if not np.isfinite(iso):
        raise ValueError("isosurface: the level must be finite (got %r)" % iso)
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("isosurface: origin and spacing are three numbers each")
    with torch.no_grad():
        if field.is_cuda and field.dtype == torch.float32 and field.is_contiguous():
            from .native import iso_ops
            return iso_ops.isosurface(field, iso, origin, spacing, normals)
        return isosurface_statement(field, iso, origin, spacing, normals)


# ------------------------------------------------------------------------------------------------------------------------------------
# the field
# ------------------------------------------------------------------------------------------------------------------------------------
def _planes(trainer, bidx):
    planes = getattr(trainer.model_coarse, "triPlane_embeddings", None)
    if planes is None:
        raise RuntimeError("geometry: model_coarse.triPlane_embeddings is not set -- render a frame (Trainer.forward) or call "
                           "model_coarse.set_conditional_embedding(...) first: the density is a function of that frame's planes")
    return planes if bidx is None else planes[:, bidx:bidx + 1]


def _density_out(rf, B, N, colors):
    rf = rf.reshape(B, N, -1)
    sigma = torch.relu(rf[..., -1])
    return (sigma, torch.sigmoid(rf[..., :3])) if colors else sigma


def _density_args(trainer, pts, inv_head_T, bidx):
    planes = _planes(trainer, bidx)
    if pts.dim() != 3 or pts.shape[-1] != 3 or inv_head_T.dim() != 3 or tuple(inv_head_T.shape[1:]) != (4, 3) \
            or not (pts.shape[0] == inv_head_T.shape[0] == planes.shape[1]):
        raise ValueError("geometry.density takes pts [B,N,3] and inv_head_T [B,4,3] with the planes' B = %d (got %s, %s)"
                         % (planes.shape[1], tuple(pts.shape), tuple(inv_head_T.shape)))
    return planes


def density_statement(trainer, pts, inv_head_T, colors=False, bidx=None):
    """density() as the modules state it, on any device and dtype: headpose_skin_net -> tri-plane features -> model_coarse"""
    from .utils.util import sample_from_triplane_new
    mc = trainer.model_coarse
    planes = _density_args(trainer, pts, inv_head_T, bidx)
    with torch.no_grad():
        rot, _ = trainer.headpose_skin_net(pts, None, inv_head_T)
        feat = sample_from_triplane_new(mc.gridwarper(rot), planes, padding_mode="zeros")
        rf = mc(rot.reshape(-1, 3), feat.reshape(-1, feat.shape[-1] * feat.shape[-2]))
        return _density_out(rf, pts.shape[0], pts.shape[1], colors)


def density(trainer, pts, inv_head_T, colors=False, bidx=None):
    """sigma [B,N] = relu(rf[..., -1]) of the trainer's field at pts [B,N,3] under inv_head_T [B,4,3], with the trainer's CURRENT
    triPlane_embeddings (bidx: that sample of them, for B = 1); colors=True: also sigmoid(rf[..., :3]) [B,N,3].  Under no_grad.
    HIP float32: native/train_ops.field_inputs + model_coarse.mlp (fp32 rows + rocBLAS); anything else: density_statement()."""
    mc = trainer.model_coarse
    planes = _density_args(trainer, pts, inv_head_T, bidx)
    if not (pts.is_cuda and pts.dtype == torch.float32 and planes.dtype == torch.float32 and mc.sh_deg == 0):
        return density_statement(trainer, pts, inv_head_T, colors, bidx)
    from .native.train_ops import field_inputs
    with torch.no_grad():
        if getattr(trainer, "_boxes", None) is None:
            f = lambda t: t.detach().reshape(3).cpu().tolist()
            gw, sw = mc.gridwarper, trainer.headpose_skin_net.gridwarper
            trainer._boxes = ((f(gw.scale_factor), f(gw.trans_factor)), (f(sw.scale_factor), f(sw.trans_factor)))
        vol = trainer.headpose_skin_net.current_volume().detach()
        X = field_inputs(pts.contiguous(), inv_head_T.to(pts.dtype).contiguous(), vol, planes.detach(), *trainer._boxes)
        return _density_out(mc.mlp(X), pts.shape[0], pts.shape[1], colors)


def posed_bounds(bounds, inv_T):
    """axis-aligned box of the canonical box's eight corners mapped to the posed space of inv_T [4,3] = [M; tau]: Skinning_Field.forward takes
    a posed point p to (p + tau) M, so a canonical corner c comes from c M^-1 - tau.  float64 on the host."""
    T = np.asarray(inv_T.detach().cpu().numpy() if torch.is_tensor(inv_T) else inv_T, dtype=np.float64).reshape(4, 3)
    b = np.asarray(bounds, dtype=np.float64).reshape(3, 2)
    corners = np.array([[b[0, (c >> 2) & 1], b[1, (c >> 1) & 1], b[2, c & 1]] for c in range(8)])
    mapped = corners @ np.linalg.inv(T[:3]) - T[3]
    return [[float(mapped[:, a].min()), float(mapped[:, a].max())] for a in range(3)]


def density_grid(trainer, inv_head_T, res, space="canonical", bounds=None, bidx=0, chunk=1 << 21):
    """(field [res,res,res] float, origin (3), spacing (3)): density() on a lattice whose first and last points lie on the bounds.
    canonical: the identity transform over cfg.models.coarse.XYZ_bounding -- pose-free, expression-dependent.  posed: sample bidx of
    inv_head_T over posed_bounds() of that box.  bounds=[[lo,hi]]*3 overrides the box.  res: one number or three.  The evaluation is chunked:
    at most `chunk` points (rows of the [n,176] MLP input) at a time."""
    if space not in ("canonical", "posed"):
        raise ValueError("density_grid: space is 'canonical' or 'posed' (got %r)" % (space,))
    res = tuple(int(r) for r in (res if isinstance(res, (tuple, list)) else (res,) * 3))
    if len(res) != 3 or min(res) < 2:
        raise ValueError("density_grid: res is one number or three, each >= 2 (got %r)" % (res,))
    planes = _planes(trainer, bidx)
    dev, dt = planes.device, planes.dtype
    if space == "canonical":
        T = trainer.headpose_skin_net.identity_trans.to(device=dev, dtype=dt)[None]
    else:
        T = inv_head_T[bidx:bidx + 1].to(device=dev, dtype=dt)
    if bounds is None:
        bounds = [[float(v) for v in ax] for ax in trainer.cfg.models.coarse.XYZ_bounding]
        if space == "posed":
            bounds = posed_bounds(bounds, T[0])
    origin = tuple(float(ax[0]) for ax in bounds)
    spacing = tuple((float(ax[1]) - float(ax[0])) / (r - 1) for ax, r in zip(bounds, res))
    o = torch.tensor(origin, dtype=dt, device=dev)
    h = torch.tensor(spacing, dtype=dt, device=dev)
    n_all = res[0] * res[1] * res[2]
    field = torch.empty(n_all, dtype=dt, device=dev)
    chunk = max(int(chunk), 1)
    for s in range(0, n_all, chunk):
        n = torch.arange(s, min(s + chunk, n_all), device=dev)
        ijk = torch.stack([n // (res[1] * res[2]), (n // res[2]) % res[1], n % res[2]], 1).to(dt)
        field[s:s + chunk] = density(trainer, (o + ijk * h)[None], T, bidx=bidx)[0]
    return field.reshape(res), origin, spacing


def extract_mesh(trainer, inv_head_T, res=128, iso=DEFAULT_ISO, space="canonical", colors=True, bidx=0):
    """(verts [V,3], tris [T,3] int32, normals [V,3], colors [V,3] in [0,1] | None) of the trainer's current frame: density_grid ->
    isosurface -> one density(..., colors=True) at the vertices."""
    field, origin, spacing = density_grid(trainer, inv_head_T, res, space=space, bidx=bidx)
    verts, tris, normals = isosurface(field, iso, origin, spacing, normals=True)
    col = None
    if colors:
        if verts.shape[0] == 0:
            col = verts.new_zeros(0, 3)
        else:
            T = (trainer.headpose_skin_net.identity_trans.to(verts)[None] if space == "canonical" else inv_head_T[bidx:bidx + 1].to(verts))
            col = density(trainer, verts[None].contiguous(), T, colors=True, bidx=bidx)[1][0]
    return verts, tris, normals, col


# ------------------------------------------------------------------------------------------------------------------------------------
# the G-buffer: depth, normal and shade maps of a rendered frame
# ------------------------------------------------------------------------------------------------------------------------------------
GBuffer = collections.namedtuple("GBuffer", "z normal mask depth16 normal8 shade8")
GBUFFER_U = 2.0 ** -24          # float32's unit round-off: the scale of the conditioning figures in aux


def _gb_args(rays, depth, acc, H, W, acc_min):
    H, W = int(H), int(W)
    for name, t in (("rays", rays), ("depth", depth), ("acc", acc)):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError("gbuffer: %s is a floating-point tensor (got %s)" % (name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if rays.dim() != 3 or H < 1 or W < 1 or rays.shape[0] < 1 or rays.shape[1] != H * W or rays.shape[2] < 8:
        raise ValueError("gbuffer: rays is [B, H W, stride >= 8] with H, W >= 1 (got %s for %d x %d)" % (tuple(rays.shape), H, W))
    B = rays.shape[0]
    for name, t in (("depth", depth), ("acc", acc)):
        if t.dim() < 2 or t.shape[0] != B or t.numel() != B * H * W or t.dtype != rays.dtype or t.device != rays.device:
            raise ValueError("gbuffer: %s holds [B, H W] = [%d, %d] values of the rays' dtype on their device (got %s %s on %s)"
                             % (name, B, H * W, t.dtype, tuple(t.shape), t.device))
    acc_min = float(acc_min)
    if not np.isfinite(acc_min):
        raise ValueError("gbuffer: acc_min must be finite (got %r)" % acc_min)
    return B, H, W, acc_min


def _gb_shift(t, axis, k):
    """t at the neighbour q + k along axis (k = +1 / -1), zero / False where that lies outside the image"""
    out = torch.zeros_like(t)
    n = t.shape[axis]
    if k > 0:
        out.narrow(axis, 0, n - 1).copy_(t.narrow(axis, 1, n - 1))
    else:
        out.narrow(axis, 1, n - 1).copy_(t.narrow(axis, 0, n - 1))
    return out


def gbuffer_statement(rays, depth, acc, H, W, acc_min=0.5, choice=None, aux=None):
    """The definition of the G-buffer (module docstring) on ATen, vectorised, in the inputs' dtype and on their device: GBuffer(z [B,H,W],
    normal [B,H,W,3], mask [B,H,W] uint8, depth16 [B,H,W,2] uint8, normal8 [B,H,W,3] uint8, shade8 [B,H,W] uint8).  Every operation is rounded
    on its own and sums run left to right, as in the kernel.
    choice [B,H,W] uint8: the decisions of another evaluation (bits 0-1 the x tangent's sides, 1 = +, 2 = -, 3 = central, 0 = none; bits 2-3
    the y tangent's; bit 4 = n was negated) are taken instead of being made -- a float64 evaluation given float32's decisions is the
    yardstick of the float32 ones.
    aux: a dict that receives, per pixel, "choice" (this evaluation's decisions, in that coding), "length" = |n| before normalisation,
    "lx" = |tx|, "ly" = |ty|, "ndot" = n . d before the negation, and "Ex", "Ey": the 2-norm over the components c of
    3u (M_a + M_b) + u |t_c| with M = |o_c| + |d_c| z at the two pixels the tangent uses and u = 2^-24 -- a bound on float32's error of
    that tangent."""
    B, H, W, acc_min = _gb_args(rays, depth, acc, H, W, acc_min)
    r = rays.reshape(B, H, W, -1)
    o, d, near, far = r[..., 0:3], r[..., 3:6], r[..., 6], r[..., 7]
    dep, a = depth.reshape(B, H, W), acc.reshape(B, H, W)
    zero = torch.zeros((), dtype=rays.dtype, device=rays.device)
    valid = (a > acc_min) & torch.isfinite(dep)
    q = dep / a
    q = torch.where(q < near, near, q)
    q = torch.where(q > far, far, q)
    z = torch.where(valid, q, zero)
    p = o + d * z[..., None]
    M = o.abs() + d.abs() * z[..., None]
    tangents, sides, errs = [], [], []
    for axis, shift in ((2, 0), (1, 2)):          # x: neighbours (y, x +- 1); y: (y +- 1, x)
        if choice is None:
            vp, vm = valid & _gb_shift(valid, axis, 1), valid & _gb_shift(valid, axis, -1)
            ap, am = (_gb_shift(z, axis, 1) - z).abs(), (z - _gb_shift(z, axis, -1)).abs()
            gt = ap > am
            mx, mn = torch.where(gt, ap, am), torch.where(gt, am, ap)
            central = vp & vm & (mx <= 4.0 * mn)
            plus = ~central & vp & (~vm | (ap <= am))
            minus = ~central & ~plus & vm
            side = central.to(torch.uint8) * 3 + plus.to(torch.uint8) + minus.to(torch.uint8) * 2
        else:
            side = (choice.reshape(B, H, W).to(device=rays.device, dtype=torch.uint8) >> shift) & 3
        up, um = ((side & 1) != 0)[..., None], ((side & 2) != 0)[..., None]
        t = torch.where(up, _gb_shift(p, axis, 1), p) - torch.where(um, _gb_shift(p, axis, -1), p)
        e = 3.0 * GBUFFER_U * (torch.where(up, _gb_shift(M, axis, 1), M) + torch.where(um, _gb_shift(M, axis, -1), M)) + GBUFFER_U * t.abs()
        tangents.append(t)
        sides.append(side)
        errs.append((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]).sqrt())
    (tx, ty), (sx, sy) = tangents, sides
    n = torch.stack([tx[..., 1] * ty[..., 2] - tx[..., 2] * ty[..., 1], tx[..., 2] * ty[..., 0] - tx[..., 0] * ty[..., 2],
                     tx[..., 0] * ty[..., 1] - tx[..., 1] * ty[..., 0]], -1)
    ndot = n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1] + n[..., 2] * d[..., 2]
    flip = ndot > 0 if choice is None else (choice.reshape(B, H, W).to(device=rays.device, dtype=torch.uint8) & 16) != 0
    n = torch.where(flip[..., None], -n, n)
    length = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]).sqrt()
    has = (sx != 0) & (sy != 0) & torch.isfinite(length) & (length > 0)
    normal = torch.where(has[..., None], n / length[..., None], zero)
    if aux is not None:
        norm3 = lambda t: (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1] + t[..., 2] * t[..., 2]).sqrt()
        aux.update(choice=sx | (sy << 2) | (flip.to(torch.uint8) << 4), length=length, lx=norm3(tx), ly=norm3(ty), Ex=errs[0], Ey=errs[1],
                   ndot=ndot)
    # the codes
    mask = valid.to(torch.uint8) | (has.to(torch.uint8) << 1)
    dc = torch.round((z - near) / (far - near) * 65534.0)
    code = torch.where(dc >= 65534.0, torch.full_like(dc, 65535.0), torch.where(dc >= 0, dc + 1.0, torch.ones_like(dc)))
    code = torch.where(valid, code, zero).to(torch.int32)
    depth16 = torch.stack([code >> 8, code & 255], -1).to(torch.uint8)
    normal8 = torch.where(has[..., None], torch.round((normal * 0.5 + 0.5) * 255.0), zero).to(torch.uint8)
    lam = -(normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1] + normal[..., 2] * d[..., 2])
    lam = torch.where(lam > 0, lam, zero)
    sc = torch.round(255.0 * lam)
    shade8 = torch.where(has, torch.where(sc >= 255.0, torch.full_like(sc, 255.0), sc), torch.full_like(sc, 255.0)).to(torch.uint8)
    return GBuffer(z, normal, mask, depth16, normal8, shade8)


def gbuffer(rays, depth, acc, H, W, acc_min=0.5):
    """Depth, normal and shade maps of B rendered frames from what the ray march read and wrote: rays [B, H W, stride >= 8] (origin, unit
    direction, near, far), depth [B, H W] = sum w z and acc [B, H W] = sum w (Trainer.nerf_forward's depth_fine and acc_fine).  Returns
    GBuffer(z, normal, mask, depth16, normal8, shade8) -- the module docstring has the definition; depth16 / normal8 / shade8 are what
    imgio.imwrite_gray16 / imwrite_rgb / imwrite_gray8 write.

    Contiguous float32 HIP tensors take the kernel (native/gbuffer_ops.py): one launch for all frames on the current stream, nothing read
    back.  Any other tensor takes the ATen statement."""
    B, H, W, acc_min = _gb_args(rays, depth, acc, H, W, acc_min)
    with torch.no_grad():
        if rays.is_cuda and rays.dtype == torch.float32 and rays.is_contiguous() and depth.is_contiguous() and acc.is_contiguous():
            from .native import gbuffer_ops
            out = gbuffer_ops.gbuffer(rays, depth, acc, H, W, acc_min, outputs=GBuffer._fields)
            return GBuffer(*[out[k] for k in GBuffer._fields])
        return gbuffer_statement(rays, depth, acc, H, W, acc_min)


DEPTH16_CODE = "0 = no surface (acc <= acc_min or depth not finite); else z = near + (code - 1) / 65534 * (far - near)"


def decode_depth16(depth16, near, far):
    """float64 z of the 16-bit codes ([...,2] uint8, high byte first), NaN where the code is 0"""
    c = depth16[..., 0].to(torch.float64) * 256.0 + depth16[..., 1].to(torch.float64)
    z = near + (c - 1.0) / 65534.0 * (far - near)
    return torch.where(c > 0, z, torch.full_like(z, float("nan")))


# ------------------------------------------------------------------------------------------------------------------------------------
# PLY
# ------------------------------------------------------------------------------------------------------------------------------------
def _np(t, dtype):
    return np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype, copy=False))


def write_ply(path, verts, tris, normals=None, colors=None):
    """Binary little-endian PLY: vertex x y z [nx ny nz] [red green blue uchar], face = uchar count + int indices.  colors: uint8, or
    floats in [0,1] (rounded to nearest)."""
    v, t = _np(verts, "<f4").reshape(-1, 3), _np(tris, "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += ["element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rec = np.zeros(len(v), dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        nn = _np(normals, "<f4").reshape(len(v), 3)
        rec["nx"], rec["ny"], rec["nz"] = nn[:, 0], nn[:, 1], nn[:, 2]
    if colors is not None:
        c = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
        if c.dtype != np.uint8:
            c = np.floor(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        c = c.reshape(len(v), 3)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    faces = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"], faces["i"] = 3, t
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())
    return path


def read_ply(path):
    """what write_ply wrote: {"verts" [V,3] f32, "tris" [T,3] i32, "normals" [V,3] f32 | None, "colors" [V,3] u8 | None} as numpy arrays"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY" % path)
    counts, props, cur = {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur], props[cur] = int(w[2]), []
        elif w[:1] == ["property"]:
            props[cur].append(w[1:])
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    if props.get("face") != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError("%s: faces are not `property list uchar int vertex_indices`" % path)
    vdt = np.dtype([(p[1], types[p[0]]) for p in props["vertex"]])
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    V, T = counts["vertex"], counts["face"]
    if len(data) != end + V * vdt.itemsize + T * fdt.itemsize:
        raise ValueError("%s: %d bytes after the header, the header announces %d" % (path, len(data) - end, V * vdt.itemsize + T * fdt.itemsize))
    rec = np.frombuffer(data, dtype=vdt, count=V, offset=end)
    faces = np.frombuffer(data, dtype=fdt, count=T, offset=end + V * vdt.itemsize)
    if T and not (faces["n"] == 3).all():
        raise ValueError("%s: a face is not a triangle" % path)
    names = vdt.names
    col = lambda ks: np.stack([rec[k] for k in ks], 1) if all(k in names for k in ks) else None
    return {"verts": col(("x", "y", "z")), "tris": faces["i"].copy(), "normals": col(("nx", "ny", "nz")), "colors": col(("red", "green", "blue"))}

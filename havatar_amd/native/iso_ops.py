"""The iso-surface kernels (csrc/hav_isosurface.hip): marching tetrahedra on the Kuhn subdivision of a contiguous float32 HIP field.
  classify(field, iso)                     -> codes [D0,D1,D2] int32 (the uint32 code words), block_counts [blocks,2] int32
  offsets(block_counts)                    -> block_offsets [blocks,2] int32, V, T        (torch.cumsum + ONE host read of the two totals)
  emit(verts, normals | None, tris, ...)   writes rows [0,V) / [0,T) of the caller's buffers and nothing beyond
  isosurface(field, iso, origin, spacing)  the three together: (verts [V,3] f32, tris [T,3] i32, normals [V,3] f32 | None)
No atomics: the same field gives the same bits on every call.  No fallback in here -- havatar_amd.geometry.isosurface decides which fields come
this way and states the same definition on ATen for the others."""
import ctypes as C

import torch

from .. import _lib
from .conv import _p, _stream

POINTS_PER_BLOCK = 256          # lattice points a workgroup owns (ISO_P of the source)


def _need(field):
    if not (torch.is_tensor(field) and field.is_cuda and field.dtype == torch.float32 and field.dim() == 3 and field.is_contiguous()):
        raise RuntimeError("iso_ops: the field is a contiguous float32 HIP tensor [D0,D1,D2] (got %s); there is no fallback path"
                           % ("%s %s %s" % (field.device, field.dtype, tuple(field.shape)) if torch.is_tensor(field) else type(field).__name__))


def blocks(shape):
    n = int(_lib.lib().hav_iso_blocks(*[int(d) for d in shape]))
    if n == 0:
        raise RuntimeError("hav_iso_*: a field of shape %s is not covered (every D >= 2, fewer than 2^31 lattice points)" % (tuple(shape),))
    return n


def classify(field, iso):
    _need(field)
    nb = blocks(field.shape)
    codes = torch.empty(field.shape, dtype=torch.int32, device=field.device)
    counts = torch.empty(nb, 2, dtype=torch.int32, device=field.device)
    with torch.cuda.device(field.device):
        _lib.check(_lib.lib().hav_iso_classify(_p(codes), _p(counts), _p(field), *[int(d) for d in field.shape], float(iso),
                                               _stream(field.device)), "hav_iso_classify")
    return codes, counts


def offsets(block_counts):
    """exclusive prefix of the per-workgroup counts and the two totals (the host read: this synchronises with the stream)"""
    rows = block_counts.t().contiguous()          # [2,blocks]: the scan runs along contiguous rows (along dim 0 of [blocks,2] it took 9 ms at 256^3)
    inc = torch.cumsum(rows, 1, dtype=torch.int64)
    V, T = (int(v) for v in inc[:, -1].tolist())
    if V > 0x7fffffff or T > 0x7fffffff:
        raise RuntimeError("hav_iso_*: %d vertices / %d triangles do not fit int32 indices" % (V, T))
    return (inc - rows).to(torch.int32).t().contiguous(), V, T


def emit(verts, normals, tris, codes, block_offsets, field, iso, origin, spacing):
    """rows [0,V) of verts (and normals, unless None) and [0,T) of tris are written, each element once; returns vbase [D0,D1,D2] int32"""
    _need(field)
    for name, t, dt in (("verts", verts, torch.float32), ("normals", normals, torch.float32), ("tris", tris, torch.int32),
                        ("codes", codes, torch.int32), ("block_offsets", block_offsets, torch.int32)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == field.device):
            raise RuntimeError("iso_ops.emit: %s is a contiguous %s HIP tensor on the field's device" % (name, dt))
    vbase = torch.empty(field.shape, dtype=torch.int32, device=field.device)
    o, h = ((C.c_float * 3)(*[float(v) for v in x]) for x in (origin, spacing))
    with torch.cuda.device(field.device):
        _lib.check(_lib.lib().hav_iso_emit(_p(verts), _p(normals), _p(tris), _p(vbase), _p(codes), _p(block_offsets), _p(field),
                                           *[int(d) for d in field.shape], float(iso), o, h, _stream(field.device)), "hav_iso_emit")
    return vbase


def isosurface(field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals=True):
    _need(field)
    codes, counts = classify(field, iso)
    boff, V, T = offsets(counts)
    verts = torch.empty(V, 3, dtype=torch.float32, device=field.device)
    nrm = torch.empty(V, 3, dtype=torch.float32, device=field.device) if normals else None
    tris = torch.empty(T, 3, dtype=torch.int32, device=field.device)
    if V > 0:          # (a crossing edge lies in a cube, whose tetrahedron over it is mixed: V > 0 means T > 0)
        emit(verts, nrm, tris, codes, boff, field, iso, origin, spacing)
    return verts, tris, nrm

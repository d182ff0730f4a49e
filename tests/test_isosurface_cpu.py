"""CPU: havatar_amd.geometry -- the ATen statement of the iso-surface against a plain-loop restatement of the definition, the topology and
geometry of its meshes, density / density_grid against the renderer, the PLY files, the binding of the entries of csrc/hav_isosurface.hip
within ABI 8, the compiler's output for gfx950, and avatarHD_reenactment.py --mesh on CPU tensors."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import iso_util as iu
import metrics_util as mu
from havatar_amd import geometry, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH_ISO = 0.5          # a level inside the synthetic checkpoint's range of densities (0 .. 1.1)
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------------------------------------------
# the definition, in plain loops: float64 positions and normals from the float32 field values
# ------------------------------------------------------------------------------------------------------------------------------------
def restate(field, iso, origin, spacing):
    """{"verts" [V,3] f64, "tris" [T,3], "normals" [V,3] f64, "nlen" [V]: length of the normal before it is normalised, "gsum" [V]: |g(n)| + |g(n+d)|}"""
    f32 = field.numpy()
    f = f32.astype(np.float64)
    D = f.shape
    iso32 = np.float32(iso)
    inside = f32 > iso32          # NaN > x is False: outside
    iso64 = float(iso32)
    o, h = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)

    def grad(p):
        g = np.zeros(3)
        for a in range(3):
            lo, up = p[a] > 0, p[a] + 1 < D[a]
            pm, pp = list(p), list(p)
            pm[a] -= int(lo)
            pp[a] += int(up)
            g[a] = (f[tuple(pp)] - f[tuple(pm)]) / ((2.0 if lo and up else 1.0) * h[a])
        return g

    verts, normals, nlen, gsum, index = [], [], [], [], {}
    with np.errstate(all="ignore"):
        for i in range(D[0]):
            for j in range(D[1]):
                for k in range(D[2]):
                    for e in range(7):
                        d = (((e + 1) >> 2) & 1, ((e + 1) >> 1) & 1, (e + 1) & 1)
                        q = (i + d[0], j + d[1], k + d[2])
                        if q[0] >= D[0] or q[1] >= D[1] or q[2] >= D[2] or inside[i, j, k] == inside[q]:
                            continue
                        a, b = f[i, j, k], f[q]
                        t = (iso64 - a) / (b - a)
                        t = min(max(t, 0.0), 1.0) if np.isfinite(t) else 0.5
                        index[(i, j, k, e)] = len(verts)
                        verts.append(o + (np.array([i, j, k]) + t * np.array(d)) * h)
                        g0, g1 = grad((i, j, k)), grad(q)
                        nv = -(g0 + t * (g1 - g0))
                        ln = np.sqrt((nv * nv).sum())
                        normals.append(nv / ln if np.isfinite(ln) and ln > 0 else np.zeros(3))
                        nlen.append(ln)
                        gsum.append(np.abs(g0).sum() + np.abs(g1).sum())
    tris = []
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    for i in range(D[0] - 1):
        for j in range(D[1] - 1):
            for k in range(D[2] - 1):
                for perm in perms:
                    c = [np.array([i, j, k])]
                    for a in perm:
                        step = np.zeros(3, np.int64)
                        step[a] = 1
                        c.append(c[-1] + step)
                    ins = [bool(inside[tuple(p)]) for p in c]
                    I = [m for m in range(4) if ins[m]]
                    O = [m for m in range(4) if not ins[m]]
                    if len(I) == 1:
                        out = [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
                    elif len(I) == 3:
                        out = [[(O[0], I[0]), (O[0], I[1]), (O[0], I[2])]]
                    elif len(I) == 2:
                        out = [[(I[0], O[0]), (I[0], O[1]), (I[1], O[1])], [(I[0], O[0]), (I[1], O[1]), (I[1], O[0])]]
                    else:
                        continue
                    away = np.mean([c[m] for m in O], 0) - np.mean([c[m] for m in I], 0)
                    for tri in out:
                        mid = [0.5 * (c[p] + c[q]) for p, q in tri]
                        if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), away) < 0:
                            tri = [tri[0], tri[2], tri[1]]
                        row = []
                        for p, q in tri:
                            lo, hi = c[min(p, q)], c[max(p, q)]
                            d = hi - lo
                            row.append(index[(int(lo[0]), int(lo[1]), int(lo[2]), int(4 * d[0] + 2 * d[1] + d[2] - 1))])
                        tris.append(row)
    return {"verts": np.array(verts, np.float64).reshape(-1, 3), "tris": np.array(tris, np.int64).reshape(-1, 3),
            "normals": np.array(normals, np.float64).reshape(-1, 3), "nlen": np.array(nlen), "gsum": np.array(gsum)}


def position_bar(shape, origin, spacing):
    """per axis: 2^-21 (max |corner coordinate| + spacing).  The float32 statement rounds t three times (subtraction, subtraction, division:
    3 x 2^-24 of t <= 1, times the spacing) and the coordinate once (2^-24 of at most the corner coordinate + spacing): under 2^-22 of that
    sum together; the bar is twice it."""
    o, h = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    far = o + (np.asarray(shape) - 1) * h
    return 2.0 ** -21 * (np.maximum(np.abs(o), np.abs(far)) + h)


def check_against(ref, got, shape, origin, spacing):
    verts, tris, _ = got
    assert tuple(verts.shape) == ref["verts"].shape and tuple(tris.shape) == ref["tris"].shape, (verts.shape, tris.shape, ref["verts"].shape,
                                                                                               ref["tris"].shape)
    assert tris.dtype == torch.int32 and np.array_equal(tris.cpu().numpy(), ref["tris"])          # order, winding and diagonal
    if len(ref["verts"]):
        err = np.abs(verts.double().cpu().numpy() - ref["verts"]).max(0)
        print("position error per axis", err, "bar", position_bar(shape, origin, spacing))
        assert (err <= position_bar(shape, origin, spacing)).all(), err


@pytest.mark.parametrize("kind", ["noise", "ties", "all_inside", "all_outside", "sprinkled"])
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 2), (5, 4, 3), (9, 8, 7)], ids=lambda s: "x".join(map(str, s)))
def test_statement_equals_the_plain_loops(shape, kind):
    f, iso, origin, spacing = iu.FIELDS[kind](shape)
    ref = restate(f, iso, origin, spacing)
    got = geometry.isosurface(f, iso, origin, spacing)
    check_against(ref, got, shape, origin, spacing)
    assert got[0].dtype == torch.float32 and got[2].shape == got[0].shape
    if kind in ("all_inside", "all_outside"):
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    elif shape != (2, 2, 2):
        assert len(ref["tris"]) > 0
    # normals=False changes nothing else
    v2, t2, n2 = geometry.isosurface(f, iso, origin, spacing, normals=False)
    assert n2 is None and torch.equal(v2, got[0]) and torch.equal(t2, got[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# topology
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere17():
    case = iu.sphere((17, 17, 17))
    return case, restate(*case), geometry.isosurface(*case)


@pytest.mark.parametrize("kind,shape,counts,chi", [("sphere", (9, 9, 9), (386, 768), 2), ("sphere", (17, 17, 17), (1730, 3456), 2),
                                                   ("torus", (17, 17, 11), (868, 1736), 0)])
def test_sphere_and_torus_are_closed_oriented_surfaces(kind, shape, counts, chi):
    case = iu.FIELDS[kind](shape)
    ref = restate(*case)
    verts, tris, _ = geometry.isosurface(*case)
    assert (len(ref["verts"]), len(ref["tris"])) == counts and (verts.shape[0], tris.shape[0]) == counts
    assert np.array_equal(tris.numpy(), ref["tris"])
    t = tris.numpy()
    assert iu.is_closed(t) and iu.is_oriented(t) and iu.all_referenced(verts.shape[0], t) and iu.euler(verts.shape[0], t) == chi


@pytest.mark.parametrize("kind", ["noise", "ties"])
def test_padded_fields_are_closed_and_oriented_and_bare_ones_have_no_edge_in_three_triangles(kind):
    case = iu.FIELDS[kind]((9, 8, 7))
    verts, tris, _ = geometry.isosurface(*iu.padded(case))
    assert tris.shape[0] > 100 and iu.is_closed(tris.numpy()) and iu.is_oriented(tris.numpy()) and iu.all_referenced(verts.shape[0], tris.numpy())
    if kind == "ties":
        assert 0.05 < float((case[0] == case[1]).float().mean()) < 0.12
    und, dire = iu.edge_uses(geometry.isosurface(*case)[1].numpy())
    assert set(und.values()) == {1, 2} and set(dire.values()) == {1}


# ------------------------------------------------------------------------------------------------------------------------------------
# geometry on the 17^3 sphere
# ------------------------------------------------------------------------------------------------------------------------------------
def test_sphere_radius_volume_and_normals(sphere17):
    """h = 0.125, r = 0.7.  Radius: linear interpolation of 0.7 - |x| over an edge of length l <= sqrt(3) h errs by at most l^2 / (8 r); a
    quarter of margin.  Volume: positive (outward winding) and within 3 % of the ball's.  Normals: the float64 restatement's worst angle to
    v / |v| is 0.01362 rad (measured); the float32 statement is held to that figure + 1e-4 rad."""
    _, ref, (verts, tris, normals) = sphere17
    h, r = 0.125, 0.7
    v = verts.double().numpy()
    rad = np.linalg.norm(v, axis=1)
    print("worst radius error / h", np.abs(rad - r).max() / h)
    assert np.abs(rad - r).max() <= 3 * h * h / (8 * r) * 1.25
    vol = iu.signed_volume(v, tris.numpy())
    print("volume / ball", vol / (4 / 3 * math.pi * r ** 3))
    assert vol > 0 and abs(vol / (4 / 3 * math.pi * r ** 3) - 1) <= 0.03
    worst64 = iu.angles(ref["normals"], ref["verts"] / np.linalg.norm(ref["verts"], axis=1, keepdims=True)).max()
    worst32 = iu.angles(normals.double().numpy(), v / rad[:, None]).max()
    print("worst normal angle: restatement %.5f rad, statement %.5f rad" % (worst64, worst32))
    assert abs(worst64 - 0.01362) <= 5e-5          # the figure of the docstring
    assert worst32 <= worst64 + 1e-4
    assert np.allclose(np.linalg.norm(normals.double().numpy(), axis=1), 1.0, atol=1e-6)


def test_zero_gradient_gives_a_zero_normal_and_refusals():
    f = torch.zeros(2, 2, 2)
    f[0, 0, 0] = float("nan")          # outside; its neighbours' differences are NaN: the length is not finite
    f[1, 1, 1] = 1.0
    _, _, n = geometry.isosurface(f, 0.5)
    assert n.shape[0] == 7 and torch.isfinite(n).all()
    with pytest.raises(ValueError, match=r"every D >= 2.*\(1, 4, 4\)"):
        geometry.isosurface(torch.zeros(1, 4, 4), 0.0)
    with pytest.raises(ValueError, match="finite"):
        geometry.isosurface(torch.zeros(2, 2, 2), float("nan"))
    from havatar_amd.native import iso_ops
    with pytest.raises(RuntimeError, match="HIP"):
        iso_ops.isosurface(torch.zeros(2, 2, 2), 0.0)
    with pytest.raises(RuntimeError, match="HIP"):
        iso_ops.classify(torch.zeros(2, 2, 2), 0.0)


def test_cpu_fields_never_reach_the_kernels(monkeypatch):
    from havatar_amd.native import iso_ops
    ran = []
    monkeypatch.setattr(iso_ops, "isosurface", lambda *a, **k: ran.append(1))
    geometry.isosurface(*iu.noise((3, 3, 3)))
    geometry.isosurface(iu.noise((3, 3, 3))[0].double(), 0.0)
    assert ran == []


# ------------------------------------------------------------------------------------------------------------------------------------
# the field
# ------------------------------------------------------------------------------------------------------------------------------------
def test_density_composites_to_the_renderers_accumulation():
    """the coarse samples of a few rays (perturb off), density() at those points, composited here in float64: acc_coarse of _render_torch"""
    trainer, inp, out = iu.avatar()
    acc = out[2].double().reshape(-1)
    rays = inp["ray_batch"][0]
    ro, rd, near, far = rays[:, :3], rays[:, 3:6], rays[:, 6:7], rays[:, 7:8]
    S = int(trainer.cfg.nerf.validation.num_coarse)
    t = torch.linspace(0.0, 1.0, S)
    z = near * (1.0 - t) + far * t
    pts = ro[:, None] + rd[:, None] * z[..., None]
    sigma, rgb = geometry.density(trainer, pts.reshape(1, -1, 3), inp["inv_head_T"], colors=True)
    assert sigma.shape == (1, rays.shape[0] * S) and rgb.shape == (1, rays.shape[0] * S, 3) and float(sigma.min()) >= 0
    assert 0 <= float(rgb.min()) and float(rgb.max()) <= 1
    sigma = sigma.double().reshape(-1, S)
    dist = (z[:, 1:] - z[:, :-1]).double()
    dist = torch.cat([dist, dist[:, -1:]], 1) * rd.double().norm(dim=-1, keepdim=True)
    alpha = 1.0 - torch.exp(-sigma * dist)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha[:, :-1] + 1e-10], 1), 1)
    got = (alpha * trans).sum(1)
    print("acc", acc.tolist(), "restated", got.tolist())
    assert float(acc.max()) > 0.5          # the rays hit the head
    assert float((got - acc).abs().max()) <= 1e-5
    assert torch.equal(geometry.density(trainer, pts.reshape(1, -1, 3), inp["inv_head_T"]), sigma.float().reshape(1, -1))


def test_density_refuses_without_an_embedding():
    from havatar_amd.model.nerf_trainer import Trainer
    from havatar_amd.utils.cfgnode import CfgNode
    trainer = Trainer(CfgNode(synth.harness_config()), 0)
    T = torch.from_numpy(synth.inv_head_T())[None]
    with pytest.raises(RuntimeError, match=r"triPlane_embeddings is not set.*set_conditional_embedding"):
        geometry.density(trainer, torch.zeros(1, 4, 3), T)
    with pytest.raises(RuntimeError, match=r"triPlane_embeddings is not set"):
        geometry.density_grid(trainer, T, 4)
    trainer, inp, _ = iu.avatar()
    with pytest.raises(ValueError, match=r"pts \[B,N,3\].*\(4, 3\)"):
        geometry.density(trainer, torch.zeros(4, 3), inp["inv_head_T"])
    with pytest.raises(ValueError, match="'canonical' or 'posed'"):
        geometry.density_grid(trainer, inp["inv_head_T"], 4, space="world")


def test_density_grid_spans_the_bounds():
    trainer, inp, _ = iu.avatar()
    box = [[float(v) for v in ax] for ax in trainer.cfg.models.coarse.XYZ_bounding]
    field, origin, spacing = geometry.density_grid(trainer, inp["inv_head_T"], (5, 4, 3), chunk=7)
    assert field.shape == (5, 4, 3) and field.dtype == torch.float32
    for a, r in enumerate((5, 4, 3)):
        assert origin[a] == box[a][0] and abs(origin[a] + (r - 1) * spacing[a] - box[a][1]) <= 1e-12
    # chunking changes nothing, and a lattice point is density() at its position under the identity transform
    whole, _, _ = geometry.density_grid(trainer, inp["inv_head_T"], (5, 4, 3))
    assert float((whole - field).abs().max()) <= 1e-5 * max(1.0, float(whole.abs().max()))          # (the GEMMs block 7 rows and 60 differently)
    p = torch.tensor([[origin[0] + 2 * spacing[0], origin[1] + 1 * spacing[1], origin[2] + 2 * spacing[2]]])
    ident = torch.eye(4)[:, :3][None]
    assert abs(float(geometry.density(trainer, p[None], ident)[0, 0]) - float(field[2, 1, 2])) <= 1e-5 * max(1.0, float(field[2, 1, 2]))
    # posed: the box contains the canonical corners mapped by the inverse of [M; tau], and (p + tau) M takes its corners' hull back
    T = inp["inv_head_T"][0].double().numpy()
    pb = geometry.posed_bounds(box, inp["inv_head_T"][0])
    for c in range(8):
        corner = np.array([box[0][(c >> 2) & 1], box[1][(c >> 1) & 1], box[2][c & 1]])
        posed = corner @ np.linalg.inv(T[:3]) - T[3]
        assert np.allclose((posed + T[3]) @ T[:3], corner, atol=1e-12)
        for a in range(3):
            assert pb[a][0] - 1e-12 <= posed[a] <= pb[a][1] + 1e-12
    fp, op, sp = geometry.density_grid(trainer, inp["inv_head_T"], 3, space="posed")
    assert fp.shape == (3, 3, 3) and all(abs(op[a] - pb[a][0]) <= 1e-12 and abs(op[a] + 2 * sp[a] - pb[a][1]) <= 1e-12 for a in range(3))


def test_extract_mesh_on_the_cpu():
    trainer, inp, _ = iu.avatar()
    # the synthetic weights are a fog (sigma <= 1.1 everywhere): the default level finds nothing in it
    assert geometry.extract_mesh(trainer, inp["inv_head_T"], res=12)[0].shape == (0, 3)
    verts, tris, normals, colors = geometry.extract_mesh(trainer, inp["inv_head_T"], res=12, iso=SYNTH_ISO)
    assert verts.shape[0] > 0 and tris.shape[0] > 0 and normals.shape == verts.shape and colors.shape == verts.shape
    assert 0 <= float(colors.min()) and float(colors.max()) <= 1
    und, _ = iu.edge_uses(tris.numpy())
    assert set(und.values()) <= {1, 2}


# ------------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normals,with_colors", [(False, False), (True, False), (True, True), (False, True)])
def test_ply_round_trip(tmp_path, with_normals, with_colors):
    verts, tris, normals = geometry.isosurface(*iu.sphere((9, 9, 9)))
    colors = torch.rand(verts.shape, generator=torch.Generator().manual_seed(0))
    path = geometry.write_ply(str(tmp_path / "m.ply"), verts, tris, normals if with_normals else None, colors if with_colors else None)
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n") + 11]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 386\n") and b"element face 768\n" in head
    assert b"property list uchar int vertex_indices\n" in head
    per_vertex = 12 + (12 if with_normals else 0) + (3 if with_colors else 0)
    assert len(data) == len(head) + 386 * per_vertex + 768 * 13
    assert (b"property float nx" in head) == with_normals and (b"property uchar red" in head) == with_colors
    back = geometry.read_ply(path)
    assert np.array_equal(back["verts"], verts.numpy()) and np.array_equal(back["tris"], tris.numpy()) and back["tris"].dtype == np.int32
    assert (back["normals"] is None) == (not with_normals) and (back["colors"] is None) == (not with_colors)
    if with_normals:
        assert np.array_equal(back["normals"], normals.numpy())
    if with_colors:
        assert back["colors"].dtype == np.uint8 and np.array_equal(back["colors"], np.floor(colors.double().numpy() * 255 + 0.5).astype(np.uint8))
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError, match="the header announces"):
        geometry.read_ply(path)
    # an empty mesh is a file too
    e = geometry.read_ply(geometry.write_ply(str(tmp_path / "e.ply"), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)))
    assert e["verts"].shape == (0, 3) and e["tris"].shape == (0, 3)


def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib, build
    L = _lib.lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    assert L.hav_iso_blocks.restype is C.c_int64 and L.hav_iso_blocks.argtypes == [i32] * 3
    assert L.hav_iso_classify.restype is i32 and L.hav_iso_classify.argtypes == [vp] * 3 + [i32] * 3 + [f32, vp]
    assert L.hav_iso_emit.restype is i32 and L.hav_iso_emit.argtypes == [vp] * 7 + [i32] * 3 + [f32, C.POINTER(f32), C.POINTER(f32), vp]
    assert _lib.ABI_VERSION == L.hav_abi_version() == 8          # additions within the version: nothing existing changed
    assert "hav_isosurface.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    for name in ("hav_iso_blocks", "hav_iso_classify", "hav_iso_emit"):
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "#define HAV_ABI_VERSION 8" in hdr and hdr.count("No reference counterpart") >= 3
    from havatar_amd.native import iso_ops
    P = iso_ops.POINTS_PER_BLOCK
    for D in ((2, 2, 2), (3, 2, 2), (2, 2, P // 4), (2, 2, P // 4 + 1), (64, 64, 64), (1290, 1290, 1290)):
        assert L.hav_iso_blocks(*D) == -(-(D[0] * D[1] * D[2]) // P), D
    for D in ((1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 4, 4), (-3, 4, 4), (2048, 1024, 1024), (1291, 1291, 1291)):
        assert L.hav_iso_blocks(*D) == 0, D
    # refusals that need no device: HAV_EINVAL for null pointers, a D < 2 and a level that is not finite, HAV_EUNSUP from 2^31 points on
    one = C.c_void_p(16)          # never dereferenced: the checks come first
    vec = (f32 * 3)(0.0, 0.0, 0.0)
    for miss in range(3):
        assert L.hav_iso_classify(*[None if k == miss else one for k in range(3)], 4, 4, 4, 0.0, None) == -1
    for miss in (0, 2, 3, 4, 5, 6):          # (1 = normals: NULL is allowed)
        assert L.hav_iso_emit(*[None if k == miss else one for k in range(7)], 4, 4, 4, 0.0, vec, vec, None) == -1
    assert L.hav_iso_emit(*[one] * 7, 4, 4, 4, 0.0, None, vec, None) == -1 and L.hav_iso_emit(*[one] * 7, 4, 4, 4, 0.0, vec, None, None) == -1
    for D in ((1, 4, 4), (4, 1, 4), (4, 4, 0)):
        assert L.hav_iso_classify(one, one, one, *D, 0.0, None) == -1 and L.hav_iso_emit(*[one] * 7, *D, 0.0, vec, vec, None) == -1
    for iso in (float("nan"), float("inf"), float("-inf")):
        assert L.hav_iso_classify(one, one, one, 4, 4, 4, iso, None) == -1 and L.hav_iso_emit(*[one] * 7, 4, 4, 4, iso, vec, vec, None) == -1
    for D in ((2048, 1024, 1024), (1291, 1291, 1291)):
        assert L.hav_iso_classify(one, one, one, *D, 0.0, None) == -2 and L.hav_iso_emit(*[one] * 7, *D, 0.0, vec, vec, None) == -2
    src = open(os.path.join(ROOT, "havatar_amd", "csrc", "hav_isosurface.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "getenv" not in code and not re.search(r"atomic", code, re.I) and not re.search(r"hipMalloc|Synchronize", code)
    # the new modules read no environment and nothing of the package imports the checker
    for mod in ("geometry.py", os.path.join("native", "iso_ops.py")):
        text = open(os.path.join(ROOT, "havatar_amd", mod)).read()
        assert "environ" not in text and "getenv" not in text and "oracle" not in text, mod


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_private_segment_no_spill(tmp_path):
    dst = str(tmp_path / "hav_isosurface.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_isosurface.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    kernels = re.findall(r"\.name:\s+(\S*_kernel\S*)", text)
    assert len(set(kernels)) == 4 and sum("iso_emit" in k for k in kernels) == 2, kernels          # classify, vbase, emit with / without normals
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == len(kernels) and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == 2 * len(kernels) and all(v == 0 for v in spills), spills
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert lds == [16] * 4          # the four wave totals of the scan


def test_tables_of_the_statement_are_the_definitions():
    corner, cnt, own, edge = geometry.tables()
    assert corner.tolist() == [[0, 4, 6, 7], [0, 4, 5, 7], [0, 2, 6, 7], [0, 2, 3, 7], [0, 1, 5, 7], [0, 1, 3, 7]]
    assert cnt.sum() == 6 * (4 + 4 + 2 * 6) and (cnt[:, 0] == 0).all() and (cnt[:, 15] == 0).all()
    assert ((edge >= 0) & (edge <= 6)).all() and ((own & (edge + 1)) == 0).all()          # an owned edge leaves its owner along fresh axes


# ------------------------------------------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------------------------------------------
def test_cli_mesh_on_cpu_tensors(tmp_path, monkeypatch):
    """--mesh --mesh-res 24: one parseable PLY per frame under <savedir>/mesh, and the PNG bytes of a run without the flag; with a level
    inside the synthetic checkpoint's densities (--mesh-iso) the files hold a surface that follows the frame's expression"""
    from havatar_amd.harness import reenact
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    root = str(tmp_path / "data")
    os.makedirs(root)
    split = synth.write_dataset(root, n_frames=2, img_res=128, photos=False)
    cfg_path, ckpt = str(tmp_path / "cfg.yml"), mu.checkpoint(tmp_path / "avatar.pth")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(synth.harness_config(), f)
    runs = []
    for extra in (["--mesh", "--mesh-res", "24"], []):
        out = str(tmp_path / ("run%d" % len(runs)))
        written = reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", out, "--split", split] + extra, device="cpu")
        assert [os.path.basename(p) for p in written] == ["0_00.png", "1_00.png"]          # what main() returned before
        runs.append((out, written, list(reenact.main.mesh_written)))
    assert [os.path.relpath(p, runs[0][0]) for p in runs[0][2]] == [os.path.join("mesh", "0_00.ply"), os.path.join("mesh", "1_00.ply")]
    assert runs[1][2] == [] and not os.path.exists(os.path.join(runs[1][0], "mesh"))
    for p, q in zip(runs[0][1], runs[1][1]):
        assert open(p, "rb").read() == open(q, "rb").read()
    for p in runs[0][2]:
        m = geometry.read_ply(p)
        assert m["normals"].shape == m["verts"].shape and m["colors"].shape == m["verts"].shape and m["tris"].shape[1] == 3
    # a level inside the synthetic densities, two frames per call: each file holds its own sample's surface (bidx)
    monkeypatch.setenv("HAVATAR_FRAME_BATCH", "2")
    out = str(tmp_path / "batched")
    reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", out, "--split", split, "--mesh", "--mesh-res", "24", "--mesh-iso",
                  str(SYNTH_ISO)], device="cpu")
    assert [os.path.basename(p) for p in reenact.main.mesh_written] == ["0_00.ply", "1_00.ply"]
    a, b = (geometry.read_ply(p) for p in reenact.main.mesh_written)
    for m in (a, b):
        assert m["verts"].shape[0] > 0 and m["tris"].shape[0] > 0 and m["normals"].shape == m["verts"].shape and m["colors"].shape == m["verts"].shape
        assert m["tris"].min() == 0 and m["tris"].max() == m["verts"].shape[0] - 1
    assert a["verts"].shape != b["verts"].shape or not np.array_equal(a["verts"], b["verts"])          # the surface follows the expression

"""GPU: the iso-surface kernels (csrc/hav_isosurface.hip, native/iso_ops.py) against the ATen statement of havatar_amd.geometry on the CPU,
their exact behaviours, the topology of their meshes, density() on the device, extract_mesh and avatarHD_reenactment.py --mesh.

Tolerances.  Triangles: bit-equal to the float32 statement's on the CPU (classification compares the same float32 values).  Positions:
position_bar of tests/test_isosurface_cpu.py against the statement evaluated on the field in float64.  Normals: on the sphere the angle to
v / |v|, barred at the float64 statement's worst + 1e-4 rad; on every field the angle to the float64 statement's normal, barred by the
conditioning of the vertex: a float32 evaluation of -(g(n) + t (g(n+d) - g(n))) errs by at most 8 x 2^-24 gsum in norm (two roundings per
gradient component, three of t, two of the interpolation; gsum = sum over the axes of |g(n)| + |g(n+d)|), which turns a vector of length L by
8 x 2^-24 gsum / L; the bar is twice that plus 1e-6 rad for the normalisation, asserted where it is below 0.1 rad; where the float64 length is
not finite the normal is exactly zero.  Every figure is printed before it is asserted (pytest -s shows them)."""
import os

import numpy as np
import pytest
import torch

import iso_util as iu
import metrics_util as mu
from havatar_amd import geometry, synth
from havatar_amd.native import iso_ops
from test_isosurface_cpu import SYNTH_ISO, position_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = iso_ops.POINTS_PER_BLOCK
SHAPES = [(2, 2, 2), (3, 2, 2), (5, 4, 3), (2, 2, P // 4 - 1), (2, 2, P // 4), (2, 2, P // 4 + 1), (3, 5, 67), (17, 17, 17), (33, 31, 29),
          (64, 64, 64)]


def _bits(t):
    return t.cpu().contiguous().view(torch.int32) if t is not None else None


@pytest.mark.parametrize("kind", sorted(iu.FIELDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_native_equals_the_cpu_statement(shape, kind):
    f, iso, origin, spacing = iu.FIELDS[kind](shape)
    want32 = geometry.isosurface(f, iso, origin, spacing)
    aux = {}
    want64 = geometry.isosurface_statement(f.double(), float(np.float32(iso)), origin, spacing, aux=aux)
    verts, tris, normals = geometry.isosurface(f.to(DEV), iso, origin, spacing)
    assert verts.is_cuda and verts.dtype == torch.float32 and tris.dtype == torch.int32 and normals.dtype == torch.float32
    assert tuple(verts.shape) == tuple(want32[0].shape) and tuple(tris.shape) == tuple(want32[1].shape) and normals.shape == verts.shape
    assert torch.equal(tris.cpu(), want32[1]) and torch.equal(want64[1], want32[1])
    assert (verts.shape[0] == 0) == (kind in ("all_inside", "all_outside") or (kind in ("sphere", "torus") and min(shape) == 2))
    if verts.shape[0] == 0:          # (the coarse lattices have no point inside the sphere or the torus)
        return
    err = (verts.cpu().double() - want64[0]).abs().max(0)[0].numpy()
    print("position error per axis", err, "bar", position_bar(shape, origin, spacing))
    assert (err <= position_bar(shape, origin, spacing)).all()
    n = normals.cpu().double().numpy()
    assert np.isfinite(n).all()
    ln = np.linalg.norm(n, axis=1)
    assert (np.abs(ln[ln > 0] - 1.0) <= 1e-6).all()
    length, gsum = aux["length"].numpy(), aux["gsum"].numpy()
    bad = ~np.isfinite(length)
    assert (n[bad] == 0).all()
    with np.errstate(all="ignore"):
        bar = 2.0 * 8.0 * 2.0 ** -24 * gsum / length + 1e-6
    sel = ~bad & (length > 0) & np.isfinite(bar) & (bar < 0.1)
    if sel.any():
        ang = iu.angles(n[sel], want64[2].numpy()[sel])
        print("normals: %d of %d vertices conditioned, worst angle / bar %.3f" % (sel.sum(), len(sel), (ang / bar[sel]).max()))
        assert (ang <= bar[sel]).all()
    if kind == "sphere" and shape[0] >= 17:
        unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
        worst64 = iu.angles(want64[2].numpy(), unit(want64[0].numpy())).max()
        worst = iu.angles(n, unit(verts.cpu().double().numpy())).max()
        print("sphere: worst normal angle %.5f rad, float64 statement %.5f rad" % (worst, worst64))
        assert worst <= worst64 + 1e-4


# ------------------------------------------------------------------------------------------------------------------------------------
# exact behaviours
# ------------------------------------------------------------------------------------------------------------------------------------
def _emit(f, iso, origin, spacing, with_normals=True, guard=8):
    """the three entries on buffers of the test's own: sentinels everywhere, `guard` rows more than the totals"""
    codes, counts = iso_ops.classify(f, iso)
    boff, V, T = iso_ops.offsets(counts)
    verts = torch.full((V + guard, 3), -1e30, device=f.device)
    normals = torch.full((V + guard, 3), -1e30, device=f.device) if with_normals else None
    tris = torch.full((T + guard, 3), -123456, dtype=torch.int32, device=f.device)
    iso_ops.emit(verts, normals, tris, codes, boff, f, iso, origin, spacing)
    return verts, normals, tris, V, T


@pytest.mark.parametrize("kind,shape", [("noise", (3, 5, 67)), ("sprinkled", (33, 31, 29)), ("torus", (17, 17, 11))])
def test_every_element_is_written_once_and_nothing_beyond(kind, shape):
    f, iso, origin, spacing = iu.FIELDS[kind](shape)
    f = f.to(DEV)
    verts, normals, tris, V, T = _emit(f, iso, origin, spacing)
    assert V > 0 and T > 0
    assert (verts[:V] != -1e30).all() and (normals[:V] != -1e30).all() and (tris[:T] != -123456).all()
    assert (verts[V:] == -1e30).all() and (normals[V:] == -1e30).all() and (tris[T:] == -123456).all()
    assert int(tris[:T].min()) == 0 and int(tris[:T].max()) == V - 1
    got = geometry.isosurface(f, iso, origin, spacing)
    assert torch.equal(_bits(got[0]), _bits(verts[:V])) and torch.equal(got[1], tris[:T]) and torch.equal(_bits(got[2]), _bits(normals[:V]))
    # a second launch gives the same bits
    again = _emit(f, iso, origin, spacing)
    for a, b in zip(again[:3], (verts, normals, tris)):
        assert torch.equal(_bits(a), _bits(b))
    # so does a launch on a side stream
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = _emit(f, iso, origin, spacing)
    side.synchronize()
    for a, b in zip(there[:3], (verts, normals, tris)):
        assert torch.equal(_bits(a), _bits(b))
    # without normals nothing else changes
    v2, n2, t2, _, _ = _emit(f, iso, origin, spacing, with_normals=False)
    assert n2 is None and torch.equal(_bits(v2), _bits(verts)) and torch.equal(t2, tris)
    v3, t3, n3 = geometry.isosurface(f, iso, origin, spacing, normals=False)
    assert n3 is None and torch.equal(_bits(v3), _bits(verts[:V])) and torch.equal(t3, tris[:T])


def test_fields_the_kernels_do_not_take_use_the_statement_on_the_device():
    f, iso, origin, spacing = iu.noise((5, 4, 3))
    want = geometry.isosurface(f.to(DEV), iso, origin, spacing)
    view = torch.zeros(5, 4, 6, device=DEV)[:, :, ::2]          # not contiguous
    view.copy_(f)
    got = geometry.isosurface(view, iso, origin, spacing)
    assert torch.equal(got[1], want[1]) and float((got[0] - want[0]).abs().max()) <= 1e-6
    got64 = geometry.isosurface(f.double().to(DEV), iso, origin, spacing)
    assert got64[0].dtype == torch.float64 and torch.equal(got64[1], want[1])
    with pytest.raises(RuntimeError, match="contiguous float32 HIP"):
        iso_ops.isosurface(view, iso)


# ------------------------------------------------------------------------------------------------------------------------------------
# topology on the device's own output
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,counts,chi", [("sphere", (17, 17, 17), (1730, 3456), 2), ("torus", (17, 17, 11), (868, 1736), 0)])
def test_device_meshes_are_closed_oriented_surfaces(kind, shape, counts, chi):
    f, iso, origin, spacing = iu.FIELDS[kind](shape)
    verts, tris, _ = geometry.isosurface(f.to(DEV), iso, origin, spacing)
    t = tris.cpu().numpy()
    assert (verts.shape[0], tris.shape[0]) == counts
    assert iu.is_closed(t) and iu.is_oriented(t) and iu.all_referenced(verts.shape[0], t) and iu.euler(verts.shape[0], t) == chi
    if kind == "sphere":
        vol = iu.signed_volume(verts.cpu().numpy(), t)
        assert vol > 0 and abs(vol / (4 / 3 * np.pi * 0.7 ** 3) - 1) <= 0.03


@pytest.mark.parametrize("kind", ["noise", "ties"])
def test_device_padded_fields_are_closed_and_oriented(kind):
    case = iu.padded(iu.FIELDS[kind]((9, 8, 7)))
    verts, tris, _ = geometry.isosurface(case[0].to(DEV), *case[1:])
    t = tris.cpu().numpy()
    assert iu.is_closed(t) and iu.is_oriented(t) and iu.all_referenced(verts.shape[0], t)


# ------------------------------------------------------------------------------------------------------------------------------------
# the field on the device
# ------------------------------------------------------------------------------------------------------------------------------------
def test_density_on_the_device():
    """4 096 points of the canonical box under the synthetic pose: the native route (field_inputs + MLP) and the float32 ATen statement on the
    device, both against the statement in float64 on the CPU; errors relative to the largest float64 entry; the rule of tests/test_lpips_gpu.py,
    e_native <= max(2 e_aten, 4e-6).  Measured on an MI355X: sigma native 7.2e-6 / ATen 7.6e-6, colours native 2.8e-7 / ATen 3.1e-7."""
    trainer, inp, _ = iu.avatar(DEV)
    box = np.asarray(trainer.cfg.models.coarse.XYZ_bounding, np.float64)
    u = torch.rand(4096, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    pts = (torch.from_numpy(box[:, 0]) + u * torch.from_numpy(box[:, 1] - box[:, 0])).float()[None]
    ref = iu.make_trainer("cpu").double()          # the same weights, float64
    assert all(torch.equal(v.float(), trainer.state_dict()[k].cpu()) for k, v in ref.state_dict().items() if v.is_floating_point())
    ref.model_coarse.triPlane_embeddings = trainer.model_coarse.triPlane_embeddings.detach().cpu().double()
    s64, c64 = geometry.density_statement(ref, pts.double(), inp["inv_head_T"].cpu().double(), colors=True)
    s_n, c_n = geometry.density(trainer, pts.to(DEV), inp["inv_head_T"], colors=True)
    s_a, c_a = geometry.density_statement(trainer, pts.to(DEV), inp["inv_head_T"], colors=True)
    assert float(s64.max()) > 0.3 and float((s64 > 0).double().mean()) > 0.5
    for name, truth, nat, aten in (("sigma", s64, s_n, s_a), ("colours", c64, c_n, c_a)):
        scale = float(truth.abs().max())
        e_n, e_a = (float((t.cpu().double() - truth).abs().max()) / scale for t in (nat, aten))
        print("%s: native %.2e, ATen float32 on the device %.2e (relative to %.3f)" % (name, e_n, e_a, scale))
        assert e_n <= max(2.0 * e_a, 4e-6)


def test_extract_mesh_on_the_device():
    trainer, inp, _ = iu.avatar(DEV)
    verts, tris, normals, colors = geometry.extract_mesh(trainer, inp["inv_head_T"], res=32, iso=SYNTH_ISO)
    assert verts.is_cuda and verts.shape[0] > 1000 and tris.shape[0] > 1000 and normals.shape == verts.shape and colors.shape == verts.shape
    assert 0 <= float(colors.min()) and float(colors.max()) <= 1
    und, _ = iu.edge_uses(tris.cpu().numpy())
    assert set(und.values()) <= {1, 2}
    # an edge used once is where the surface leaves the grid: both ends on one face of the box
    box = np.asarray(trainer.cfg.models.coarse.XYZ_bounding, np.float64)
    v = verts.cpu().double().numpy()
    on_face = np.concatenate([np.abs(v - box[:, 0]) <= 1e-5, np.abs(v - box[:, 1]) <= 1e-5], 1)          # [V,6]
    open_edges = [e for e, c in und.items() if c == 1]
    assert all((on_face[p] & on_face[q]).any() for p, q in open_edges)
    print("vertices %d, triangles %d, open edges %d" % (verts.shape[0], tris.shape[0], len(open_edges)))
    # the posed box holds a surface too
    vp, tp, _, _ = geometry.extract_mesh(trainer, inp["inv_head_T"], res=32, iso=SYNTH_ISO, space="posed", colors=False)
    assert vp.shape[0] > 1000 and set(iu.edge_uses(tp.cpu().numpy())[0].values()) <= {1, 2}


def test_cli_mesh_on_the_device(tmp_path, monkeypatch):
    """graph mode (the default): PLYs are written by the native route and the PNGs are byte-identical to a run of the same process without
    --mesh.  Both runs restrict MIOpen to its deterministic solvers, as tests/test_metrics_gpu.py does and for its reason."""
    import yaml
    from havatar_amd.harness import reenact
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    root = str(tmp_path / "data")
    os.makedirs(root)
    split = synth.write_dataset(root, n_frames=2, img_res=128, photos=False)
    cfg_path, ckpt = str(tmp_path / "cfg.yml"), mu.checkpoint(tmp_path / "avatar.pth")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(synth.harness_config(), f)
    calls, real = [], iso_ops.isosurface
    monkeypatch.setattr(iso_ops, "isosurface", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = []
    for extra in (["--mesh", "--mesh-res", "32", "--mesh-iso", str(SYNTH_ISO)], []):
        out = str(tmp_path / ("with" if extra else "without"))
        written = reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", out, "--split", split] + extra, device="cuda")
        assert [os.path.basename(p) for p in written] == ["0_00.png", "1_00.png"]
        outs.append((out, written, list(reenact.main.mesh_written)))
    assert len(calls) == 2          # the kernels extracted both frames
    assert [os.path.relpath(p, outs[0][0]) for p in outs[0][2]] == [os.path.join("mesh", "0_00.ply"), os.path.join("mesh", "1_00.ply")]
    assert outs[1][2] == [] and not os.path.exists(os.path.join(outs[1][0], "mesh"))
    for p, q in zip(outs[0][1], outs[1][1]):
        assert open(p, "rb").read() == open(q, "rb").read()
    for p in outs[0][2]:
        m = geometry.read_ply(p)
        assert m["verts"].shape[0] > 1000 and m["tris"].max() == m["verts"].shape[0] - 1 and m["colors"].shape == m["verts"].shape

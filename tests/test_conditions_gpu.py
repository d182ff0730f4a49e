"""The rasteriser kernels (csrc/hav_raster.hip) on the device: face, z, render8 and coverage are the bits of the float32 statement on the CPU;
the normals against the float64 statement given float32's face and z, with the CPU float32 statement as the yardstick; every element
written and nothing beyond; bit reproducibility (two launches, a side stream, graph replays, a permuted triangle order); routing and
refusals; avatarHD_reenactment.py --cond-mesh on the device."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import conditions_util as cu
from havatar_amd import conditions as cd
from havatar_amd.native import raster_ops
from test_conditions_cpu import cli_setup, same_files

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW, BIG = raster_ops.params()
# (res, B, F): tile edges and one past (the tile is TH x TW), one and three meshes, triangle counts around a wave and a workgroup
CASES = [(8, 1, 1), (33, 1, 63), (33, 3, 64), (TW - 1, 1, 64), (TW, 1, 65), (TW + 1, 3, 64), (TW + 3, 3, 257), (TW, 1, 2046), (TW + 3, 1, 2046),
         (256, 1, 2046)]
POISON = {torch.int32: -7, torch.float32: -1e30, torch.uint8: 0xA5}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def threshold_triangles(res, z):
    """right triangles whose pixel boxes hold BIG - 1, BIG and BIG + 1 centres (w x h with w the largest divisor below the root), so the
    thread walk, its last size and the wave walk are all taken; and a column and a row of BIG + 1 pixels where they fit"""
    pitch, verts = 2.0 / res, []
    X = lambda j: (2 * j + 1) / res - 1
    sizes = []
    for n in (BIG - 1, BIG, BIG + 1):
        w = next(w for w in range(int(math.isqrt(n)), 0, -1) if n % w == 0)
        sizes.append((w, n // w))
    sizes += [(1, BIG + 1), (BIG + 1, 1)]
    for k, (w, h) in enumerate(sizes):
        if max(w, h) + 2 > res:
            continue
        j0, i0, d = 1 + k % 2, 1 + (k // 2) % 2, 0.25 * pitch
        verts += [(X(j0) - d, X(i0) - d, z + 0.01 * k), (X(j0 + w - 1) + d, X(i0) - d, z + 0.01 * k), (X(j0) - d, X(i0 + h - 1) + d, z + 0.01 * k)]
    return verts


@functools.lru_cache(maxsize=None)
def scene(res, B, F):
    """(verts [B,V,3], colors [B,V,3], tris [F',3]) numpy, in the unit box: the first F triangles of a sphere tessellation, the threshold
    triangles behind it, and at 256^2 two full-frame triangles behind everything.  Frame b is turned and shrunk a little."""
    n_lat = 2 if F < 8 else max(3, int(round(math.sqrt(F / 2.0))) + 1)
    n_lon = max(3, -(-F // (2 * (n_lat - 1))))
    sv, st = cu.uv_sphere(n_lat, n_lon, 0.75, centre=(0.05, -0.03, 0.0), squash=(1.0, 1.1, 0.9))
    assert len(st) >= F
    st = st[:F]
    extra = threshold_triangles(res, 0.9) if res >= 33 else []
    if res == 256:
        extra += [(-3.0, -3.0, 1.5), (3.5, -3.0, 1.41), (-3.0, 3.5, 1.37), (3.0, 3.0, 1.6), (-3.5, 3.0, 1.7), (3.0, -3.5, 1.8)]
    n_s = len(sv)
    if extra:
        sv = np.concatenate([sv, np.asarray(extra)], 0)
        st = np.concatenate([st, n_s + np.arange(len(extra)).reshape(-1, 3)], 0)
    frames = []
    for b in range(B):
        a = 0.3 * b
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        m = sv.copy()
        m[:n_s] = (sv[:n_s] * (1 - 0.07 * b)) @ R.T
        frames.append(m)
    verts = np.stack(frames)
    return verts, np.stack([cu.vertex_colors(v) for v in verts]), st


@functools.lru_cache(maxsize=None)
def cpu32(res, B, F):
    v, c, t = cu.tensors(*scene(res, B, F))
    return cd.conditions_statement(v, c, t, res, bounds=cu.UNIT)


def native(res, B, F, **kw):
    v, c, t = cu.tensors(*scene(res, B, F), device=DEV)
    return raster_ops.raster(v, c, t, res, cd.ORTHO_ROTS, cu.UNIT, **kw)


@pytest.mark.parametrize("res,B,F", CASES, ids=lambda v: str(v))
def test_native_equals_the_statements(res, B, F):
    want = cpu32(res, B, F)
    got = cd.Conditions(**{k: v.cpu() for k, v in native(res, B, F).items()})
    covered = int((want.face >= 0).sum())
    wide = int(len(scene(res, B, F)[2]) - F)
    print("res %d B %d F %d (+%d threshold / full-frame triangles): %d covered pixels, %d faces win" % (res, B, F, wide, covered,
                                                                                                       len(torch.unique(want.face)) - 1))
    assert covered > 0
    assert torch.equal(got.face, want.face)          # which is coverage too: -1 where none
    assert torch.equal(_bits(got.z), _bits(want.z)) and torch.equal(got.render8, want.render8)
    if res == 256:          # both full-frame triangles and the sphere in front of them win somewhere: both raster paths were taken
        assert bool((want.face[:, 0] >= 0).all()) and {F + wide - 2, F + wide - 1} <= set(torch.unique(want.face).tolist())
    cu.check_normals(got, want, "res %d B %d F %d" % (res, B, F))


def test_shared_colours_and_the_default_view():
    """colors [V,3] for every frame, the reference's bounds and a camera distance off the default"""
    verts, colors, tris = scene(33, 3, 64)
    v, c, t = cu.tensors(verts * 1.4, colors[0], tris)
    want = cd.conditions_statement(v, c, t, 40, cam_dist=7.5)
    got = cd.render_conditions(v.to(DEV), c.to(DEV), t.to(DEV), 40, cam_dist=7.5)
    assert got.cond.device.type == "cuda" and torch.equal(got.face.cpu(), want.face) and torch.equal(_bits(got.z.cpu()), _bits(want.z))
    assert torch.equal(got.render8.cpu(), want.render8) and float(want.z.max()) > 6.0
    cu.check_normals(cd.Conditions(*[x.cpu() for x in got]), want, "shared colours")


@pytest.mark.parametrize("res,B,F", [(33, 1, 63), (TW + 3, 3, 257)], ids=lambda v: str(v))
def test_every_element_is_written_and_nothing_beyond(res, B, F):
    v, c, t = cu.tensors(*scene(res, B, F), device=DEV)
    want = raster_ops.raster(v, c, t, res, cd.ORTHO_ROTS, cu.UNIT)
    keys, screen = raster_ops.workspaces(B, v.shape[1], res, DEV)
    G = 64

    def guarded(k):          # the output starts an odd number of elements into its allocation, guard bands on both sides
        base = torch.full((want[k].numel() + 2 * G + 1,), POISON[want[k].dtype], dtype=want[k].dtype, device=DEV)
        return base, base[G + 1:G + 1 + want[k].numel()].view(want[k].shape)
    bufs = {k: guarded(k) for k in want}
    raster_ops.raster_into({k: view for k, (_, view) in bufs.items()}, keys, screen, v, c, t, res, cd.ORTHO_ROTS, cu.UNIT)
    for k, (base, view) in bufs.items():
        assert torch.equal(_bits(view), _bits(want[k])), k
        assert bool((base[:G + 1] == POISON[base.dtype]).all()) and bool((base[G + 1 + view.numel():] == POISON[base.dtype]).all()), k
    # poisoned prefill: every element is overwritten, whatever was there; a missing output is not written and changes no other
    for k in want:
        base, view = guarded(k)
        raster_ops.raster_into({k: view}, keys, screen, v, c, t, res, cd.ORTHO_ROTS, cu.UNIT)
        assert torch.equal(_bits(view), _bits(want[k])), k
        assert bool((base[:G + 1] == POISON[base.dtype]).all()) and bool((base[G + 1 + view.numel():] == POISON[base.dtype]).all()), k


def test_launches_streams_graph_replays_and_triangle_order_return_the_eager_bits():
    res, B = TW + 3, 3
    v, c, t = cu.tensors(*scene(res, B, 257), device=DEV)
    eager = raster_ops.raster(v, c, t, res, cd.ORTHO_ROTS, cu.UNIT)
    again = raster_ops.raster(v, c, t, res, cd.ORTHO_ROTS, cu.UNIT)
    assert all(torch.equal(_bits(again[k]), _bits(eager[k])) for k in eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = raster_ops.raster(v, c, t, res, cd.ORTHO_ROTS, cu.UNIT)
    side.synchronize()
    assert all(torch.equal(_bits(there[k]), _bits(eager[k])) for k in eager)
    # a permuted triangle order: another arrival order at every pixel, the same winners once the indices are mapped back
    perm = torch.from_numpy(np.random.RandomState(5).permutation(t.shape[0])).to(DEV)
    shuffled = raster_ops.raster(v, c, t[perm].contiguous(), res, cd.ORTHO_ROTS, cu.UNIT)
    back = torch.where(shuffled["face"] >= 0, perm[shuffled["face"].clamp(min=0).long()].to(torch.int32), shuffled["face"])
    exact_ties = int((back != eager["face"]).sum())          # a tie goes to the smaller index OF THE LAUNCH: only exact ties may differ
    print("permuted order: %d pixels change their winner (exact depth ties)" % exact_ties)
    assert torch.equal(_bits(shuffled["z"]), _bits(eager["z"])) and exact_ties == 0
    assert all(torch.equal(_bits(shuffled[k]), _bits(eager[k])) for k in eager if k != "face")
    # five replays of a captured raster_into, inputs changed in between
    torch.cuda.current_stream().wait_stream(side)
    other = raster_ops.raster((v * 0.9).contiguous(), c, t, res, cd.ORTHO_ROTS, cu.UNIT)
    sv, sc = v.clone(), c.clone()
    out = {k: torch.empty_like(x) for k, x in eager.items()}
    keys, screen = raster_ops.workspaces(B, v.shape[1], res, DEV)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        raster_ops.raster_into(out, keys, screen, sv, sc, t, res, cd.ORTHO_ROTS, cu.UNIT)
    for i in (1, 0, 0, 1, 0):
        sv.copy_(v if i == 0 else v * 0.9)
        want = eager if i == 0 else other
        for x in out.values():
            x.fill_(POISON[x.dtype])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(out[k]), _bits(want[k])) for k in out)


def test_routing_and_refusals(monkeypatch):
    res = 33
    v, c, t = cu.tensors(*scene(res, 1, 63), device=DEV)
    calls, real = [], raster_ops.raster
    monkeypatch.setattr(raster_ops, "raster", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    on = cd.render_conditions(v, c, t, res, bounds=cu.UNIT)
    assert calls == [1] and on.cond.is_cuda and on.face.dtype == torch.int32
    assert torch.equal(cd.render_conditions(v, c, t.long(), res, bounds=cu.UNIT).face, on.face) and calls == [1, 1]          # any integer indices
    assert torch.equal(cd.render_conditions(v, c, cd.Topology(t.cpu(), v.shape[1]), res, bounds=cu.UNIT).face, on.face) and len(calls) == 3
    # float64 and non-contiguous tensors take the statement, on the device
    d = cd.render_conditions(v.double(), c.double(), t, res, bounds=cu.UNIT)
    assert len(calls) == 3 and d.cond.is_cuda and d.cond.dtype == torch.float64
    assert float((d.face != on.face).float().mean()) < 0.01          # another rounding at a silhouette pixel at most
    strided = torch.stack([v, v], -1)[..., 0]
    assert not strided.is_contiguous()
    s = cd.render_conditions(strided, c, t, res, bounds=cu.UNIT)
    assert len(calls) == 3 and float((s.face != on.face).float().mean()) < 0.01
    monkeypatch.setattr(raster_ops, "raster", real)
    # the binding refuses what the kernels do not take; nothing falls back
    args = (res, cd.ORTHO_ROTS, cu.UNIT)
    for bad in (lambda: real(strided, c, t, *args), lambda: real(v.double(), c, t, *args), lambda: real(v, c.half(), t, *args),
                lambda: real(v, c, t.long(), *args), lambda: real(v.cpu(), c, t, *args), lambda: real(v, c.cpu(), t, *args),
                lambda: real(v, c, t.cpu(), *args), lambda: real(v, c[:, :-1], t, *args), lambda: real(v, c, t[:, :2].contiguous(), *args),
                lambda: real(v, c, t, 26755, cd.ORTHO_ROTS, cu.UNIT), lambda: real(v, c, t, 0, cd.ORTHO_ROTS, cu.UNIT),
                lambda: real(v, c, t, *args, cam_dist=float("nan")), lambda: real(v, c, t, *args, cam_dist=float("inf")),
                lambda: real(v, c, t, *args, outputs=("face", "depth"))):
        with pytest.raises((RuntimeError, KeyError)):
            bad()
    keys, screen = raster_ops.workspaces(1, v.shape[1], res, DEV)
    out = {"face": torch.empty(1, 3, res, res, dtype=torch.int32, device=DEV)}
    for bad in (lambda: raster_ops.raster_into(out, keys[:, :2], screen, v, c, t, *args), lambda: raster_ops.raster_into(out, keys, screen[..., :3], v, c, t, *args),
                lambda: raster_ops.raster_into({}, keys, screen, v, c, t, *args), lambda: raster_ops.raster_into({"face": out["face"].float()}, keys, screen, v, c, t, *args),
                lambda: raster_ops.raster_into(out, keys.int(), screen, v, c, t, *args)):
        with pytest.raises(RuntimeError):
            bad()
    # out-of-range indices handed to the kernel directly (render_conditions would take them as well): those triangles take no part
    t_bad = torch.cat([torch.tensor([[0, 1, v.shape[1]]], dtype=torch.int32, device=DEV), t, torch.tensor([[-1, 1, 2]], dtype=torch.int32, device=DEV)])
    got = real(v, c, t_bad, *args)
    assert torch.equal(torch.where(got["face"] >= 0, got["face"] - 1, got["face"]), on.face) and torch.equal(got["cond"], on.cond)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graphed", "eager"])
def test_cli_cond_mesh_on_the_device(tmp_path, monkeypatch, graph):
    """--cond-mesh --cond-write on the device, then a run that reads the PNGs it wrote: the tensors handed to the Trainer are bit-identical in
    value and stride, frame by frame, and the rgb PNGs are byte-identical.
    Both runs restrict MIOpen to its deterministic solvers, as HAVATAR_DETERMINISTIC=1 does for training (harness/train.py::enable_determinism:
    "the default solver of the 16^2 convolutions is what makes even the FORWARD differ between runs").  Measured on an MI355X, PNG route against
    PNG route on three frames: with the default solvers 0-3 of a frame's 49 152 bytes differ between arbitrary runs of one process, on this set and
    on the noise set of the other harness tests alike, graphed, eager and with serialised kernels; with deterministic solvers 0 bytes in 18 pairs
    of runs (three processes, graphed and eager).  Without the restriction a byte comparison of two device runs says nothing about the route."""
    from havatar_amd.harness import reenact
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    monkeypatch.setenv("HAVATAR_GRAPH", graph)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    run, tri, frames = cli_setup(tmp_path)
    for d in frames:          # the set's PNGs came from the CPU statement: remove them, the device run writes its own
        for f in os.listdir(d):
            if f.startswith("ortho_"):
                os.remove(os.path.join(d, f))
    real, seen = reenact.frame_inputs, {}

    def recording(route):
        def frame_inputs(*a, **k):
            inp = real(*a, **k)
            seen.setdefault(route, []).append({n: (inp[n].clone(), inp[n].stride()) for n in inp if n.endswith("_render_cond")})
            return inp
        return frame_inputs
    monkeypatch.setattr(reenact, "frame_inputs", recording("mesh"))
    _, from_mesh, cond_written = run(["--cond-mesh", tri, "--cond-write"], "mesh", DEV)
    assert len(cond_written) == 12 and all(os.path.exists(p) for p in cond_written)
    monkeypatch.setattr(reenact, "frame_inputs", recording("png"))
    _, from_png, _ = run([], "png", DEV)          # reads the PNGs the kernels' output was written to
    monkeypatch.setattr(reenact, "frame_inputs", real)
    assert len(seen["mesh"]) == len(seen["png"]) == 2
    for a, b in zip(seen["mesh"], seen["png"]):
        assert sorted(a) == sorted(b) == ["front_render_cond", "left_render_cond", "right_render_cond"]
        for n in a:
            assert a[n][0].is_cuda and a[n][1] == b[n][1] and torch.equal(a[n][0], b[n][0]), n
    assert not torch.equal(seen["mesh"][0]["front_render_cond"][0], seen["mesh"][1]["front_render_cond"][0])
    assert [os.path.basename(p) for p in from_mesh] == ["0_00.png", "1_00.png"]
    from havatar_amd.dataloader import imgio
    print("bytes that differ per frame:", [int((imgio.imread_rgb(p) != imgio.imread_rgb(q)).sum()) for p, q in zip(from_mesh, from_png)])
    assert same_files(from_mesh, from_png)
    assert not same_files(from_mesh[:1], from_mesh[1:])

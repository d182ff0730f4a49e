"""GPU: the branches and sizes of the training kernels (hav_composite_*, hav_field_inputs_*, hav_triplane_gather_*, hav_mlp_train_*) that
the reference checks of tests/test_ops_gpu.py and tests/test_mlp_train_gpu.py do not reach -- the second trip of every grid-stride loop,
several tiles per weight-gradient slice, the direct and the scalar-copy compositing backward, the C > 64 field kernels, one-sided
backwards, non-square planes, exact texel nodes, saturated rays.  Same references and bars as those files: fp64 ATen autograd is the
truth, ATen fp32 (or the bf16-operand emulation) the yardstick.  Every branch is reached by shape alone; each test asserts the
inequality that puts it there, with the launchers' cap formulas (comp_blocks, field_blocks, tile_grid, weight_slices) restated on the
device's CU count.  DESIGN.md ("Which test reaches which training kernel") has the map."""
import ctypes as C

import pytest
import torch

from helpers import _field_inputs_reference, _inputs, _weights, check_mlp_backward, check_mlp_forward, report

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NERF_BOX, SKIN_BOX = ([0.66, 0.65, 0.7], [0.0, 0.07, 0.14]), ([0.66, 1.9, 0.7], [0.0, -1.7, 0.14])
HAV_EUNSUP = -2


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _errs(tag, name, mine, r32, r64):
    """(e_mine, e_aten) relative to max |fp64|, reported before the caller asserts on them"""
    scale = r64.abs().max().item()
    assert scale > 0, (tag, name)
    assert mine.shape == r64.shape and torch.isfinite(mine).all(), (tag, name)
    e_mine, e_aten = (mine.double() - r64).abs().max().item() / scale, (r32.double() - r64).abs().max().item() / scale
    report("train_edges %s %s: e_mine %.2e e_aten %.2e" % (tag, name, e_mine, e_aten))
    return e_mine, e_aten


# =====================================================================================================================================
# compositing
# =====================================================================================================================================
def _composite_inputs(n, S, CH, use_noise, use_bg, seed, misaligned=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    RW = CH + 1
    if misaligned:          # contiguous, but one float into a larger buffer: the row base is 4-byte, not 16-byte aligned
        big = torch.zeros(n * S * RW + 8, device=DEV)
        rf = big[1:1 + n * S * RW].view(n, S, RW)
        rf.copy_(torch.randn(n, S, RW, device=DEV, generator=g) * 2)
        assert rf.is_contiguous() and rf.data_ptr() % 16 == 4
        rf.requires_grad_(True)
    else:
        rf = (torch.randn(n, S, RW, device=DEV, generator=g) * 2).requires_grad_(True)
    z = torch.sort(torch.rand(n, S, device=DEV, generator=g) * 2.6 + 3.4, -1)[0]
    rd = torch.randn(n, 3, device=DEV, generator=g)
    noise = torch.randn(n, S, device=DEV, generator=g) * 0.5 if use_noise else None
    bg = torch.rand(n, 3, device=DEV, generator=g) if use_bg else None
    ups = [torch.randn(s, device=DEV, generator=g) for s in ((n, CH), (n,), (n, S), (n,))]
    return rf, z, rd, noise, bg, ups


def _composite_check(tag, rf, z, rd, noise, bg, ups, n_sigmoid=3, act_feat=False):
    """hav_composite_{fwd,bwd} vs volume_render_radiance_field under ATen autograd: the statement and the bar of
    test_composite_forward_and_gradients_match_volume_render_radiance_field.  Returns the kernel's outputs + d_rf."""
    from havatar_amd.native.train_ops import composite
    from havatar_amd.utils.nerf_util import volume_render_radiance_field

    def aten(r, dt):
        r2 = r + 0                                           # the reference sigmoids its radiance field in place
        if noise is not None:                                # inject the draw: sigma = relu(raw + noise)
            r2 = torch.cat([r2[..., :-1], r2[..., -1:] + noise.to(dt)[..., None]], -1)
        rgb, _, acc, w, depth = volume_render_radiance_field(r2, z.to(dt), rd.to(dt), 0.0, act_feat=act_feat,
                                                             background_prior=bg.to(dt) if bg is not None else None)
        outs = (rgb, acc, w, depth)
        return outs + torch.autograd.grad(outs, r, [u.to(dt) for u in ups])

    ref32 = aten(rf, torch.float32)
    ref64 = aten(rf.detach().double().requires_grad_(True), torch.float64)
    got = composite(rf, z, rd, noise, bg, n_sigmoid=n_sigmoid)
    got = tuple(got) + torch.autograd.grad(got, rf, ups)
    for name, mine, r32, r64 in zip(("rgb", "acc", "weights", "depth", "d_rf"), got, ref32, ref64):
        assert torch.isfinite(r32).all() and torch.isfinite(r64).all(), (tag, name)
        e_mine, e_aten = _errs("composite " + tag, name, mine, r32, r64)
        assert e_mine <= max(2.0 * e_aten, 4e-6), (tag, name, e_mine, e_aten)
    return got


def _composite_bwd_raw(d_rf, ups, rf, z, rd, noise, bg, n_sigmoid=3, null_upstream=False):
    """hav_composite_bwd through the C ABI: the only way to a d_rf that is not a fresh allocation and to null upstream pointers"""
    from havatar_amd import _lib
    n, S, RW = rf.shape
    d_rgb, d_acc, d_w, d_depth = ups
    if null_upstream:
        d_acc = d_w = d_depth = None
    with torch.cuda.device(DEV):
        rc = _lib.lib().hav_composite_bwd(_p(d_rf), _p(d_rgb), _p(d_acc), _p(d_w), _p(d_depth), _p(rf), _p(z), _p(rd), _p(noise), _p(bg),
                                          n, S, RW - 1, n_sigmoid, _stream())
    _lib.check(rc, "hav_composite_bwd")
    torch.cuda.synchronize()
    return d_rf


@pytest.mark.parametrize("n,S,CH", [(37, 64, 100), (9, 33, 200)])
def test_composite_direct_backward_by_shape(n, S, CH):
    """composite_kernel<1>: the block of a ray does not fit the staged form's LDS (2 waves x S x (CH + 1) floats > 48 KiB)"""
    assert 2 * S * (CH + 1) * 4 > 48 * 1024
    _composite_check("direct n%d S%d CH%d" % (n, S, CH), *_composite_inputs(n, S, CH, True, True, seed=100 + S))


@pytest.mark.parametrize("n,S,CH,misaligned", [(50, 7, 4, False), (50, 63, 66, False), (40, 64, 67, True)])
def test_composite_staged_backward_scalar_copy(n, S, CH, misaligned):
    """composite_kernel<2> where the block cannot move as 16-byte vectors: S (CH + 1) = 35 and 4 221 are no multiples of 4; 64 x 68 is, but
    the radiance field starts one float into a larger buffer"""
    assert 2 * S * (CH + 1) * 4 <= 48 * 1024
    assert (S * (CH + 1)) % 4 != 0 or misaligned
    rf, z, rd, noise, bg, ups = _composite_inputs(n, S, CH, True, True, seed=200 + S, misaligned=misaligned)
    got = _composite_check("scalar-copy n%d S%d CH%d%s" % (n, S, CH, " misaligned" if misaligned else ""), rf, z, rd, noise, bg, ups)
    if misaligned:
        # ... and a d_rf that is such a view too (autograd's is a fresh allocation): the same bits, and nothing outside the view is written
        RW = CH + 1
        big = torch.full((n * S * RW + 8,), float("nan"), device=DEV)
        view = big[1:1 + n * S * RW].view(n, S, RW)
        assert view.data_ptr() % 16 == 4
        _composite_bwd_raw(view, ups, rf.detach(), z, rd, noise, bg)
        assert torch.equal(view, got[4])
        assert torch.isnan(big[:1]).all() and torch.isnan(big[1 + n * S * RW:]).all()


def test_composite_second_grid_trip():
    """composite_kernel<0> and <2> with more rays than the capped grids have waves (4 per workgroup x 16 per CU forward, 2 x 32 backward):
    every wave takes a second ray"""
    cus = _cus()
    n, S, CH = 4 * 16 * cus + 5, 8, 4
    assert n > 4 * 16 * cus and n > 2 * 32 * cus and 2 * S * (CH + 1) * 4 <= 48 * 1024
    _composite_check("second trip n%d S%d CH%d" % (n, S, CH), *_composite_inputs(n, S, CH, True, True, seed=301))


def test_composite_direct_backward_second_grid_trip():
    """composite_kernel<1> past its grid of 4 x 16 x CUs waves, at the smaller of the two direct shapes (33 x 201 floats per ray: 0.4 GB
    of radiance field at 256 CUs, 0.9 GB in fp64 -- a second or two on the device)"""
    cus = _cus()
    n, S, CH = 4 * 16 * cus + 5, 33, 200
    assert n > 4 * 16 * cus and 2 * S * (CH + 1) * 4 > 48 * 1024
    _composite_check("direct second trip n%d S%d CH%d" % (n, S, CH), *_composite_inputs(n, S, CH, False, True, seed=302))


@pytest.mark.parametrize("n,S,CH", [(300, 64, 67), (77, 7, 4)])
def test_composite_saturated_rays(n, S, CH):
    """Where the backward divides by tt = 1 - alpha + 1e-10: ray r carries a run of r % 7 consecutive samples of raw density 3000 (alpha = 1
    exactly in fp32, tt = 1e-10; runs of 5 and 6 take the transmittance through the subnormals to 0), every third ray repeats two depths
    (distance 0), every eleventh has no density at all (acc = 0).  Depths are jittered but at least half a bin apart and |rd| >= 0.8, so
    that 3000 x distance >= 40 on every sample of a run.  Everything finite and inside the usual bar."""
    g = torch.Generator(device=DEV).manual_seed(400 + S)
    rf = torch.randn(n, S, CH + 1, device=DEV, generator=g) * 2
    z = 3.4 + 2.6 * (torch.arange(S, device=DEV)[None, :] + 0.5 * torch.rand(n, S, device=DEV, generator=g)) / S
    rd = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=-1) * (0.8 + 0.4 * torch.rand(n, 1, device=DEV, generator=g))
    bg = torch.rand(n, 3, device=DEV, generator=g)
    ups = [torch.randn(s, device=DEV, generator=g) for s in ((n, CH), (n,), (n, S), (n,))]
    for r in range(n):
        run = r % 7
        if run:
            s0 = (5 * r) % (S - run + 1)
            rf[r, s0:s0 + run, CH] = 3000.0
        if r % 3 == 0:
            z[r, 3] = z[r, 2]
            z[r, S - 1] = z[r, S - 2]
        if r % 11 == 0:
            rf[r, :, CH] = -rf[r, :, CH].abs()
    rf.requires_grad_(True)
    got = _composite_check("saturated n%d S%d CH%d" % (n, S, CH), rf, z, rd, None, bg, ups)
    assert (got[1][::11] == 0).all()                                       # no density: nothing accumulated
    # the recipe does what it says: opaque samples, and transmittances that reach 0
    w = got[2]
    r = torch.arange(n, device=DEV)
    assert (w.max(-1)[0][(r % 7 > 0) & (r % 11 > 0)] > 0).all() and (w == 0).any()


@pytest.mark.parametrize("n,S,CH,n_sigmoid,act_feat,use_bg", [(50, 16, 5, 5, True, True), (50, 16, 5, 0, None, True), (20, 2, 3, 3, False, True),
                                                              (20, 9, 1, 1, True, False), (20, 9, 1, 0, None, False)])
def test_composite_activation_variants(n, S, CH, n_sigmoid, act_feat, use_bg):
    """n_sigmoid = CH against the reference's act_feat=True, n_sigmoid = 0 against act_feat=None, CH = 3 at the smallest S the reference
    takes (its last distance repeats the one before), CH = 1 without a background (the background term reads three channels)"""
    _composite_check("nsig%d n%d S%d CH%d" % (n_sigmoid, n, S, CH), *_composite_inputs(n, S, CH, True, use_bg, seed=500 + S + CH + n_sigmoid),
                     n_sigmoid=n_sigmoid, act_feat=act_feat)


@pytest.mark.parametrize("n,S,CH", [(40, 64, 67), (50, 7, 4), (9, 33, 200)])
def test_composite_backward_null_upstream_pointers_mean_zeros(n, S, CH):
    """d_acc = d_weights = d_depth = NULL (autograd always materialises them) against zero tensors: the same bits; staged, staged with
    the scalar copy, direct"""
    rf, z, rd, noise, bg, ups = _composite_inputs(n, S, CH, True, True, seed=600 + S)
    rf = rf.detach()
    zeros = [ups[0]] + [torch.zeros_like(u) for u in ups[1:]]
    a = _composite_bwd_raw(torch.empty_like(rf), zeros, rf, z, rd, noise, bg)
    b = _composite_bwd_raw(torch.empty_like(rf), zeros, rf, z, rd, noise, bg, null_upstream=True)
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    assert torch.equal(a, b)


# =====================================================================================================================================
# field inputs and tri-plane gather
# =====================================================================================================================================
def _field_tensors(B, N, Cc, H, W, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    planes = torch.randn(2, B, Cc, H, W, device=DEV, generator=g, requires_grad=True)
    vol0 = torch.sigmoid(2 * torch.randn(1, 1, D, D, D, device=DEV, generator=g))
    vol = torch.cat([vol0, 1 - vol0], 1).requires_grad_(True)
    pts = torch.rand(B, N, 3, device=DEV, generator=g) * 3.6 - 1.8
    ang = torch.tensor([0.3, -0.2, 0.5][:B], device=DEV)
    Rm = torch.stack([torch.stack([torch.cos(ang), torch.zeros_like(ang), torch.sin(ang)], -1),
                      torch.tensor([0.0, 1.0, 0.0], device=DEV).expand(B, 3),
                      torch.stack([-torch.sin(ang), torch.zeros_like(ang), torch.cos(ang)], -1)], 1)
    inv_T = torch.cat([Rm, torch.tensor([[[0.02, -0.03, 0.01]]], device=DEV).expand(B, 1, 3)], 1).contiguous()
    up = torch.randn(B * N, 2 * Cc + 48, device=DEV, generator=g)
    return planes, vol, pts, inv_T, up


def _field_reference(planes, vol, pts, inv_T, up, nerf_box, wrt):
    """(X, gradients by `wrt`) of the PyTorch statement in fp32 and in fp64"""
    def aten(dt):
        pp, vv = planes.detach().to(dt).requires_grad_(True), vol.detach().to(dt).requires_grad_(True)
        r = _field_inputs_reference(pts.to(dt), inv_T.to(dt), vv, pp, nerf_box, SKIN_BOX)
        return (r,) + torch.autograd.grad(r, [dict(planes=pp, vol=vv)[k] for k in wrt], up.to(dt))
    return aten(torch.float32), aten(torch.float64)


def _field_check(tag, planes, vol, pts, inv_T, up, nerf_box=NERF_BOX):
    """hav_field_inputs_{fwd,bwd} vs the PyTorch statement: X, d/dplanes, d/dvolume with the bar of
    test_field_inputs_forward_and_gradients_match_the_pytorch_statement"""
    from havatar_amd.native.train_ops import field_inputs
    ref32, ref64 = _field_reference(planes, vol, pts, inv_T, up, nerf_box, ("planes", "vol"))
    got = field_inputs(pts, inv_T, vol, planes, nerf_box, SKIN_BOX)
    gp, gv = torch.autograd.grad(got, (planes, vol), up)
    for name, mine, r32, r64 in (("X", got, ref32[0], ref64[0]), ("dplanes", gp, ref32[1], ref64[1]), ("dvol", gv, ref32[2], ref64[2])):
        e_mine, e_aten = _errs("field_inputs " + tag, name, mine, r32, r64)
        assert e_mine <= max(2.0 * e_aten, 4e-6), (tag, name, e_mine, e_aten)
    assert gv.abs().max().item() > 0 and gp.abs().max().item() > 0
    return got, gp, gv, ref64


def _gather_check(tag, B, N, Cc, H, W, seed):
    """hav_triplane_gather_{fwd,bwd} vs sample_from_triplane_new under ATen autograd with the bar of
    test_triplane_gather_forward_and_gradients_match_grid_sample"""
    from havatar_amd.native.gather import triplane_gather
    from havatar_amd.utils.util import sample_from_triplane_new
    g = torch.Generator(device=DEV).manual_seed(seed)
    planes = torch.randn(2, B, Cc, H, W, device=DEV, generator=g, requires_grad=True)
    q = (torch.rand(B, N, 3, device=DEV, generator=g) * 2.4 - 1.2).requires_grad_(True)      # 17 % of the taps fall outside
    up = torch.randn(B * N, 2 * Cc, device=DEV, generator=g)

    def aten(qq, pp, upp):
        r = sample_from_triplane_new(qq, pp, padding_mode="zeros")
        r = r.reshape(-1, r.shape[-1] * r.shape[-2])
        return (r,) + torch.autograd.grad(r, (pp, qq), upp)

    ref32 = aten(q, planes, up)
    ref64 = aten(q.detach().double().requires_grad_(True), planes.detach().double().requires_grad_(True), up.double())
    got = triplane_gather(q, planes)
    gp, gq = torch.autograd.grad(got, (planes, q), up)
    for name, mine, r32, r64 in (("feat", got, ref32[0], ref64[0]), ("dplanes", gp, ref32[1], ref64[1]), ("dq", gq, ref32[2], ref64[2])):
        e_mine, e_aten = _errs("gather " + tag, name, mine, r32, r64)
        assert e_mine <= max(2.0 * e_aten, 2e-6), (tag, name, e_mine, e_aten)


def _batches(n):
    """a batch count that divides n (queries of a later batch element land in the second trip too)"""
    return next(b for b in (3, 2, 1) if n % b == 0)


@pytest.mark.parametrize("B,N,Cc,H,W,D", [(2, 500, 72, 9, 9, 5), (1, 130, 130, 6, 6, 4)])
def test_field_inputs_more_than_64_channels(B, N, Cc, H, W, D):
    """field_inputs_kernel<0> / <1>: one query per wave, the lanes loop over the channels (two and three trips)"""
    assert Cc > 64
    _field_check("C%d B%d N%d %dx%d D%d" % (Cc, B, N, H, W, D), *_field_tensors(B, N, Cc, H, W, D, seed=700 + Cc))


@pytest.mark.parametrize("Cc", [72, 130])
def test_triplane_gather_more_than_64_channels(Cc):
    _gather_check("C%d 5x7" % Cc, 2, 300, Cc, 5, 7, seed=710 + Cc)


@pytest.mark.parametrize("B,N,Cc,H,W,D", [(2, 211, 7, 6, 11, 5), (2, 211, 1, 11, 6, 3), (1, 333, 8, 6, 11, 2), (2, 211, 72, 11, 6, 2), (1, 97, 65, 6, 11, 3)])
def test_field_inputs_odd_channels_non_square_planes_and_two_voxel_volume(B, N, Cc, H, W, D):
    """odd and single channel counts (idle lanes of the window kernel take channel C - 1), H != W both ways (d/dz scales with W - 1,
    d/dy with H - 1: only dvol sees a mix-up), D = 2 (every query between the only two voxels of an axis); on both kernel routes"""
    assert H != W
    _field_check("C%d B%d N%d %dx%d D%d" % (Cc, B, N, H, W, D), *_field_tensors(B, N, Cc, H, W, D, seed=720 + Cc + D))


@pytest.mark.parametrize("Cc", [8, 72])
def test_field_inputs_one_sided_backward(Cc):
    """Only the planes, or only the volume, want a gradient (a null dvol skips the whole d/dp' block, a null dplanes every plane atomic):
    each equals the two-sided call's up to the order of the float atomics, and meets the fp64 bar on its own"""
    from havatar_amd.native.train_ops import field_inputs
    planes, vol, pts, inv_T, up = _field_tensors(2, 400, Cc, 6, 11, 5, seed=730 + Cc)
    tag = "one-sided C%d" % Cc
    _, gp2, gv2, _ = _field_check(tag + " both", planes, vol, pts, inv_T, up)
    ref32, ref64 = _field_reference(planes, vol, pts, inv_T, up, NERF_BOX, ("planes", "vol"))
    gp1, = torch.autograd.grad(field_inputs(pts, inv_T, vol.detach(), planes, NERF_BOX, SKIN_BOX), planes, up)
    gv1, = torch.autograd.grad(field_inputs(pts, inv_T, vol, planes.detach(), NERF_BOX, SKIN_BOX), vol, up)
    for name, one, two, r32, r64 in (("dplanes", gp1, gp2, ref32[1], ref64[1]), ("dvol", gv1, gv2, ref32[2], ref64[2])):
        scale = two.abs().max().item()
        assert scale > 0 and (one - two).abs().max().item() <= 2e-5 * scale, (name, (one - two).abs().max().item() / scale)
        e_mine, e_aten = _errs("field_inputs " + tag + " alone", name, one, r32, r64)
        assert e_mine <= max(2.0 * e_aten, 4e-6), (name, e_mine, e_aten)


@pytest.mark.parametrize("Cc", [8, 72])
@pytest.mark.parametrize("box", ["dyadic", "nerf"])
def test_field_inputs_on_exact_texel_nodes(Cc, box):
    """Queries whose warped plane coordinates are -1, +1, every texel centre of a 5 x 7 plane (last row and column included), and a hair
    outside +-1 (one ulp, which (u + 1) rounds back onto the node in fp32, and 2^-20): identity pose and a constant volume, so that the
    blended point h0 p + h1 p is the query itself up to the rounding of h0 + h1.
    "dyadic": a box warp of scale 1/2, translation 0 and a volume of 0.5 / 0.5 -- every step is exact in fp32, the kernel's plane
    coordinates ARE the nodes.  "nerf": the model's box (nodes up to the rounding of the warp: a hair either side) and a volume of
    0.3 / 0.7.  Not 0.5 / 0.5 there, because of what that does to the yardstick: with w0 == w1 ATen's w / (w + w + 1e-8) is 0.5 without
    any rounding, so its blended point is exact and its X error (1.3e-6 measured) is that of sin() alone, while any evaluation that
    rounds the quotient once -- the kernel's reciprocal + Newton step is within 1 ulp of it by design -- moves the point by 2^-23
    relative, which the encoding's top frequency multiplies by 128 |p| = 197: 4.2e-6 (C = 8) and 3.9e-6 (C = 72) of max |X| measured
    against the 4e-6 floor.  With unequal weights ATen rounds its quotients too and the yardstick measures the statement in fp32.
    X and dplanes only: on a node d/dq and dvol are one-sided derivatives, and fp32 and fp64 may pick different sides."""
    from havatar_amd.native.train_ops import field_inputs
    H, W, D, B = 5, 7, 3, 2
    nerf_box = ([0.5, 0.5, 0.5], [0.0, 0.0, 0.0]) if box == "dyadic" else NERF_BOX
    hair = [s * (1.0 + e) for s in (-1.0, 1.0) for e in (2.0 ** -23, 2.0 ** -20)]
    ax = lambda k: torch.tensor([2.0 * i / (k - 1) - 1.0 for i in range(k)] + hair, dtype=torch.float64)
    q = torch.cartesian_prod(ax(W), ax(H), ax(W))                                     # (x along W, y along H, z along W)
    pts = ((q - torch.tensor(nerf_box[1], dtype=torch.float64)) / torch.tensor(nerf_box[0], dtype=torch.float64)).float()
    if box == "dyadic":
        assert torch.equal((pts * 0.5).double(), q.float().double())                  # the warp returns the nodes exactly
    pts = pts.to(DEV)[None].expand(B, -1, -1).contiguous()
    N = pts.shape[1]
    g = torch.Generator(device=DEV).manual_seed(740 + Cc)
    planes = torch.randn(2, B, Cc, H, W, device=DEV, generator=g, requires_grad=True)
    v0 = 0.5 if box == "dyadic" else 0.3
    vol = torch.cat([torch.full((1, 1, D, D, D), v0, device=DEV), torch.full((1, 1, D, D, D), 1.0 - v0, device=DEV)], 1)
    inv_T = torch.cat([torch.eye(3, device=DEV), torch.zeros(1, 3, device=DEV)], 0)[None].expand(B, 4, 3).contiguous()
    up = torch.randn(B * N, 2 * Cc + 48, device=DEV, generator=g)
    ref32, ref64 = _field_reference(planes, vol, pts, inv_T, up, nerf_box, ("planes",))
    got = field_inputs(pts, inv_T, vol, planes, nerf_box, SKIN_BOX)
    gp, = torch.autograd.grad(got, planes, up)
    for name, mine, r32, r64 in (("X", got, ref32[0], ref64[0]), ("dplanes", gp, ref32[1], ref64[1])):
        e_mine, e_aten = _errs("field_inputs nodes %s C%d" % (box, Cc), name, mine, r32, r64)
        assert e_mine <= max(2.0 * e_aten, 4e-6), (name, e_mine, e_aten)
    # the last row and column did receive gradient
    assert gp[:, :, :, H - 1, :].abs().max().item() > 0 and gp[:, :, :, :, W - 1].abs().max().item() > 0


def test_triplane_gather_second_grid_trip():
    cus = _cus()
    n = 4 * 32 * cus + 37
    assert n > 4 * 32 * cus
    B = _batches(n)
    _gather_check("second trip n%d C8" % n, B, n // B, 8, 5, 7, seed=750)


def test_field_inputs_one_query_per_wave_second_grid_trip():
    """field_inputs_kernel<0> / <1> (C = 72) past field_blocks' 4 x 32 x CUs waves"""
    cus = _cus()
    n, Cc = 4 * 32 * cus + 37, 72
    assert n > 4 * 32 * cus and Cc > 64
    B = _batches(n)
    _field_check("second trip n%d C%d" % (n, Cc), *_field_tensors(B, n // B, Cc, 5, 7, 4, seed=751))


def test_field_inputs_run_kernels_second_grid_trip():
    """field_inputs_run_kernel<0> and field_inputs_kernel<2> (C = 8): a wave takes 16 queries per trip, so the loop repeats past
    16 x 4 x 32 x CUs queries -- half a million at 256 CUs, on 5 x 7 planes and a 4^3 volume"""
    cus = _cus()
    n, Cc = 16 * 4 * 32 * cus + 37, 8
    assert (n + 15) // 16 > 4 * 32 * cus and Cc <= 64
    B = _batches(n)
    _field_check("run kernels second trip n%d C%d" % (n, Cc), *_field_tensors(B, n // B, Cc, 5, 7, 4, seed=752))


@pytest.mark.parametrize("Cc", [7, 72])
def test_field_inputs_bf16_rows_refuse_odd_and_wide_channel_counts(Cc):
    """hav_field_inputs_fwd_bf16 packs two channels per word on the run kernel: odd C and C > 64 are HAV_EUNSUP, nothing is launched"""
    from havatar_amd import _lib
    from havatar_amd.native.train_ops import _field_params
    planes, vol, pts, inv_T, _ = _field_tensors(1, 10, Cc, 5, 7, 3, seed=760)
    planes_cl = planes.detach().permute(0, 1, 3, 4, 2).contiguous()
    p = _field_params(pts, planes_cl, vol.detach(), NERF_BOX + SKIN_BOX)
    Xb = torch.full((10, 2 * Cc + 48), 7.0, device=DEV, dtype=torch.bfloat16)
    with torch.cuda.device(DEV):
        rc = _lib.lib().hav_field_inputs_fwd_bf16(_p(Xb), C.byref(p), _p(pts), _p(inv_T), _p(vol.detach()), _p(planes_cl), _stream())
    torch.cuda.synchronize()
    assert rc == HAV_EUNSUP
    assert (Xb == 7.0).all()


# =====================================================================================================================================
# training MLP
# =====================================================================================================================================
@pytest.mark.parametrize("n", [1, 31, 33])
def test_mlp_less_than_one_tile_and_one_row_into_the_second(n):
    """a tile is 32 rows: one row, one short of a tile, one into the second tile -- the rows that do not exist must not reach the bias
    and weight sums"""
    check_mlp_forward(n)
    check_mlp_backward(n)


def test_mlp_forward_second_grid_trip():
    """mlp_fwd_kernel: tile_grid(nt, 4 waves, 4 workgroups per CU) -- more than 16 x CUs tiles of 32 rows"""
    cus = _cus()
    n = 32 * 16 * cus + 17
    assert (n + 31) // 32 > 4 * 4 * cus
    check_mlp_forward(n)


def test_mlp_backward_data_second_grid_trip():
    """mlp_bwd_data_kernel: tile_grid(nt, 4 waves, 1 workgroup per CU) -- more than 4 x CUs tiles"""
    cus = _cus()
    n = 32 * 4 * cus + 17
    assert (n + 31) // 32 > 4 * 1 * cus
    check_mlp_backward(n)


def test_mlp_weight_gradients_several_tiles_per_slice_and_empty_slices():
    """mlp_bwd_weights_kernel: weight_slices() = min(tiles, CUs x 8 / 11) slices of per = ceil(tiles / slices) tiles.  With 3 x slices + 1
    tiles per = 4: every working slice sums four tiles (the last one three) and the last quarter of the slices is empty and must
    contribute zeros"""
    from havatar_amd import _lib
    s = _cus() * 8 // 11
    n = 32 * (3 * s) + 17
    nt = (n + 31) // 32
    assert nt > s
    per = (nt + s - 1) // s
    assert per == 4 and (nt + per - 1) // per < s                          # several tiles per slice; trailing slices without any
    assert _lib.lib().hav_mlp_train_partial_bytes(n) == s * 61 * 64 * 16 * 4          # the library slices as restated here
    check_mlp_backward(n)


def _mlp_bwd_raw(X, d, blob, grads, accumulate):
    from havatar_amd import _lib
    L = _lib.lib()
    n = X.shape[0]
    dX = torch.empty_like(X)
    ops = torch.empty(int(L.hav_mlp_train_ops_bytes(n)), dtype=torch.uint8, device=DEV)
    partial = torch.empty(int(L.hav_mlp_train_partial_bytes(n)), dtype=torch.uint8, device=DEV)
    hg = _lib.HavMlpGrads(*[g.data_ptr() for g in grads])
    with torch.cuda.device(DEV):
        rc = L.hav_mlp_train_bwd(_p(dX), C.byref(hg), int(accumulate), _p(X), _p(d), _p(blob), _p(ops), _p(partial), n, _stream())
    _lib.check(rc, "hav_mlp_train_bwd")
    torch.cuda.synchronize()
    return dX


def test_mlp_backward_accumulate_adds_to_what_is_there():
    """hav_mlp_train_bwd(accumulate=1) (no caller in the package: reached through the C ABI): every gradient is g0 + r in one fp32
    addition, r = what accumulate=0 writes for the same inputs (a fixed-order reduction: the same bits every time)"""
    from havatar_amd.native import mlp_train
    ws = [w.detach() for w in _weights(DEV)]
    X, d = _inputs(1000, DEV, seed=7)
    d = d * 1000.0
    blob = mlp_train.pack(ws)
    g = torch.Generator(device=DEV).manual_seed(800)
    r = [torch.full_like(w, float("nan")) for w in ws]
    dX0 = _mlp_bwd_raw(X, d, blob, r, 0)
    g0 = [torch.randn(w.shape, device=DEV, generator=g) for w in ws]
    acc = [t.clone() for t in g0]
    dX1 = _mlp_bwd_raw(X, d, blob, acc, 1)
    assert torch.equal(dX0, dX1)
    for name, a, b, c in zip(("W1", "b1", "W2", "b2", "Wa", "ba", "Wf", "bf", "Wc", "bc"), acc, g0, r):
        assert torch.isfinite(c).all() and c.abs().max().item() > 0, name
        assert torch.equal(a, b + c), name


@pytest.mark.parametrize("n", [33, 1000])
def test_mlp_zero_upstream_gradient_gives_exact_zeros(n):
    from havatar_amd.native import mlp_train
    ws = _weights(DEV)
    X, d = _inputs(n, DEV, seed=9)
    Xg = X.clone().requires_grad_(True)
    mlp_train.fused_mlp(Xg, ws).backward(torch.zeros_like(d))
    for name, t in zip(("X", "W1", "b1", "W2", "b2", "Wa", "ba", "Wf", "bf", "Wc", "bc"), [Xg.grad] + [w.grad for w in ws]):
        assert t is not None and torch.isfinite(t).all() and float(t.abs().max()) == 0.0, name

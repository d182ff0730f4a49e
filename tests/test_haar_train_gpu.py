"""GPU: the wavelet autograd nodes of stage two (native/train_ops.py::HaarDwt / HaarIdwt / HaarUp2 / HaarDown2, HAVATAR_HAAR_TRAIN=1) and
the one new kernel behind them, hav_haar_down2 (csrc/hav_stage2.hip).

Shapes, in the kernels' own terms.  A workgroup of hav_haar_down2 is 256 consecutive items of the flattened [plane, output row, group of 4
output columns] list (no grid cap); the three existing kernels walk the same kind of list with a capped grid.  So: the smallest eligible map of
each node (less than one workgroup), 34 x 72 input positions (rows of 9 column groups, a ragged last workgroup), a 6 x 4104 map whose single row
of 513 column groups spans more than two workgroups, W % 8 != 0 (the 4-byte path of hav_haar_down2 and a ragged last column group), C = 1 and 3,
B = 1 and 2, and for the capped launchers one size past their cap, derived from multi_processor_count with their own formula."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODES = ("dwt", "idwt", "up2", "down2")
# (B, C, H, W) of the INPUT's spatial positions; C = channels of the image domain (wavelet-domain tensors carry 4C)
SHAPES = {
    "dwt": [(1, 1, 2, 8), (2, 3, 34, 72), (1, 1, 6, 4104), (1, 3, 66, 136)],
    "idwt": [(1, 1, 1, 4), (2, 3, 34, 72), (1, 1, 6, 4104), (1, 3, 17, 36)],
    "up2": [(1, 1, 1, 2), (2, 3, 34, 72), (1, 1, 6, 4104), (1, 3, 17, 18)],
    "down2": [(1, 1, 2, 4), (2, 3, 34, 72), (1, 1, 6, 4104), (1, 3, 10, 36), (2, 1, 66, 136)],
}


class _Mods:
    """the modules whose statements the nodes replace, in float32 on the device (yardstick) and float64 on the CPU (reference)"""

    def __init__(self):
        from havatar_amd.model.styleUnet import Downsample, HaarTransform, InverseHaarTransform, Upsample
        mk = lambda: (HaarTransform(3), InverseHaarTransform(3), Upsample((1, 3, 3, 1)), Downsample((1, 3, 3, 1)))
        self.d32 = [m.to(DEV) for m in mk()]
        self.c64 = [m.double() for m in mk()]

    @staticmethod
    def statement(mods, node, x):
        dwt, iwt, up, down = mods
        return {"dwt": lambda: dwt(x), "idwt": lambda: iwt(x), "up2": lambda: dwt(up(iwt(x))), "down2": lambda: dwt(down(iwt(x)))}[node]()

    def banks(self):
        from havatar_amd.model.styleUnet import _haar_bank
        dwt, iwt, up, down = self.d32
        return (_haar_bank(dwt, (dwt.ll, dwt.lh, dwt.hl, dwt.hh)), _haar_bank(iwt, (iwt.ll, iwt.lh, iwt.hl, iwt.hh)), up.kernel, down.kernel)

    def node(self, node, x):
        from havatar_amd.native import train_ops as t
        kd, ki, fu, fd = self.banks()
        return {"dwt": lambda: t.haar_dwt(x, kd), "idwt": lambda: t.haar_idwt(x, ki), "up2": lambda: t.haar_up2(x, ki, fu, kd),
                "down2": lambda: t.haar_down2(x, ki, fd, kd)}[node]()


@pytest.fixture(scope="module")
def mods():
    return _Mods()


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("HAVATAR_HAAR_TRAIN", raising=False)


def _input(node, shape, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C if node == "dwt" else 4 * C, H, W, generator=g)


def _cases():
    return [(n, s) for n in NODES for s in SHAPES[n]]


@pytest.mark.parametrize("shape", SHAPES["down2"] + [(1, 1, 2, 2), (1, 2, 6, 10)])
def test_down2_kernel_equals_the_three_launch_sequence_bit_for_bit(mods, shape):
    """hav_haar_down2 at scale 1 against fused.haar(inverse) -> upfirdn2d(down 2, pad (1, 1)) -> fused.haar (the modules without autograd: the
    one-launch transforms where they take the shape, their bit-identical four-call statements elsewhere); at scale 4 exactly 4 times that"""
    from havatar_amd.model.op import upfirdn2d
    from havatar_amd.native import train_ops as t
    x = _input("down2", shape, 11).to(DEV)
    kd, ki, fu, fd = mods.banks()
    dwt, iwt, up, down = mods.d32
    with torch.no_grad():
        want = dwt(upfirdn2d(iwt(x), fd, down=2, pad=(1, 1)))
    got = t.haar_down2_raw(x, ki, fd, kd, 1.0)
    assert got.shape == want.shape == (shape[0], 4 * shape[1], shape[2] // 2, shape[3] // 2)
    assert torch.equal(got, want)
    assert torch.equal(t.haar_down2_raw(x, ki, fd, kd, 4.0), 4.0 * want)
    assert t.haar_down2_raw(x[:, :, :, :-1], ki, fd, kd) is None and t.haar_down2_raw(x[:, :, :-1], ki, fd, kd) is None          # odd W, odd H


@pytest.mark.parametrize("node,shape", _cases())
def test_forward_backward_and_double_backward(mods, node, shape):
    """forward: the statement's bits.  backward and double backward: against float64 autograd of the PyTorch statement, at most twice the
    error of the float32 statement on the device, with a floor of 1e-6 of the largest magnitude"""
    x = _input(node, shape, 21)
    xd = x.to(DEV).requires_grad_(True)
    y = mods.node(node, xd)
    assert type(y.grad_fn).__name__ == {"dwt": "HaarDwtBackward", "idwt": "HaarIdwtBackward", "up2": "HaarUp2Backward", "down2": "HaarDown2Backward"}[node]
    x32 = x.to(DEV).requires_grad_(True)
    y32 = mods.statement(mods.d32, node, x32)          # switch unset, grad mode on: today's statement under autograd
    assert "Haar" not in type(y32.grad_fn).__name__
    assert torch.equal(y.detach(), y32.detach())
    x64 = x.double().requires_grad_(True)
    y64 = mods.statement(mods.c64, node, x64)
    g = torch.Generator().manual_seed(22)
    c1, c2 = torch.randn(y64.shape, generator=g), torch.randn(x.shape, generator=g)

    def bar(name, got, aten, ref):
        ref = ref.detach()
        mag = ref.abs().max().item()
        e_got = (got.detach().double().cpu() - ref).abs().max().item()
        e_aten = (aten.detach().double().cpu() - ref).abs().max().item()
        print("%s %s %s: node %.3e statement %.3e magnitude %.3e" % (node, shape, name, e_got, e_aten, mag))
        assert e_got <= max(2.0 * e_aten, 1e-6 * mag), (name, e_got, e_aten, mag)

    # first order, graph kept; the cotangent is a leaf so that the second differentiation has something to reach
    c1d, c132, c164 = c1.to(DEV).requires_grad_(True), c1.to(DEV).requires_grad_(True), c1.double().requires_grad_(True)
    gd, = torch.autograd.grad(y, xd, c1d, create_graph=True)
    g32, = torch.autograd.grad(y32, x32, c132, create_graph=True)
    g64, = torch.autograd.grad(y64, x64, c164, create_graph=True)
    bar("dx", gd, g32, g64)
    # second order: d <A^T c1, c2> / d c1 = A c2, the forward map applied to the second cotangent
    hd, = torch.autograd.grad(gd, c1d, c2.to(DEV))
    h32, = torch.autograd.grad(g32, c132, c2.to(DEV))
    h64, = torch.autograd.grad(g64, c164, c2.double())
    bar("A c2", hd, h32, h64)
    with torch.no_grad():
        assert torch.equal(hd, mods.node(node, c2.to(DEV)))          # it IS the forward kernel


@pytest.mark.parametrize("node,shape", _cases())
def test_inner_product_identity(mods, node, shape):
    """<A x, y> = <x, A^T y> with both sides accumulated in float64: the bank, flip and gain each adjoint takes.  A wrong sign, flip or factor
    moves the two sides apart by the order of |A x| |y|; float32 rounding of the roughly 40 operations behind an element moves them by
    40 * 2^-24 = 2.4e-6 of that at the very most -- the bar is 1e-5 |A x| |y|"""
    x = _input(node, shape, 31).to(DEV).requires_grad_(True)
    ax = mods.node(node, x)
    y = torch.randn(ax.shape, generator=torch.Generator().manual_seed(32)).to(DEV)
    aty, = torch.autograd.grad(ax, x, y)
    lhs = (ax.detach().double() * y.double()).sum().item()
    rhs = (x.detach().double() * aty.double()).sum().item()
    scale = ax.detach().double().norm().item() * y.double().norm().item()
    print("%s %s: <Ax,y> %.9e <x,ATy> %.9e scale %.3e" % (node, shape, lhs, rhs, scale))
    assert abs(lhs - rhs) <= 1e-5 * scale
    assert scale > 0 and aty.abs().max().item() > 0


def test_adjoint_banks_are_the_flipped_ones(mods):
    """what the derivation in native/train_ops.py says of the Haar banks: flipping the analysis bank gives the synthesis module's bank"""
    from havatar_amd.native.train_ops import _flipped
    kd, ki, fu, fd = mods.banks()
    assert torch.equal(_flipped(kd), ki) and torch.equal(_flipped(ki), kd)
    assert torch.equal(_flipped(fu, 0.25), fd) and torch.equal(_flipped(fd, 4.0), fu)


def _graph_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [n for n, _ in f.next_functions]
    return names


def test_modules_take_the_nodes_only_with_the_switch_set_and_an_eligible_shape(mods, monkeypatch):
    from havatar_amd import synth
    from havatar_amd.model.styleUnet import FromRGB, ToRGB
    torch.manual_seed(0)
    dwt, iwt = mods.d32[0], mods.d32[1]
    frgb = synth.fill_state_dict(FromRGB(16, 3)).to(DEV)
    trgb = synth.fill_state_dict(ToRGB(16, 8)).to(DEV)
    g = torch.Generator().manual_seed(41)
    img = torch.randn(2, 3, 16, 16, generator=g).to(DEV).requires_grad_(True)
    wav = torch.randn(2, 12, 8, 8, generator=g).to(DEV).requires_grad_(True)
    feat, style = torch.randn(2, 16, 16, 16, generator=g).to(DEV), torch.randn(2, 8, generator=g).to(DEV)
    odd = torch.randn(1, 3, 6, 12, generator=g).to(DEV).requires_grad_(True)          # W % 8 != 0: not a shape hav_haar_dwt takes

    def run():
        return dwt(img), iwt(wav), frgb(wav)[0], trgb(feat, style, wav), dwt(odd)

    off = run()
    assert not any(n.startswith("Haar") for o in off for n in _graph_names(o))
    monkeypatch.setenv("HAVATAR_HAAR_TRAIN", "1")
    on = run()
    for o, name in zip(on[:4], ("HaarDwtBackward", "HaarIdwtBackward", "HaarDown2Backward", "HaarUp2Backward")):
        assert name in _graph_names(o), name
    assert not any(n.startswith("Haar") for n in _graph_names(on[4]))
    for a, b in zip(on, off):
        assert torch.equal(a.detach(), b.detach())          # the same bits either way
    # other dtypes and no-grad calls keep their routes
    from havatar_amd.model.styleUnet import HaarTransform
    assert not any(n.startswith("Haar") for n in _graph_names(HaarTransform(3).double().to(DEV)(img.double())))
    with torch.no_grad():
        assert dwt(img).grad_fn is None
    # gradients through the wired modules: the same numbers as with the switch unset, to float32 rounding
    gon = torch.autograd.grad([o.sum() for o in on[:4]], [img, wav])
    goff = torch.autograd.grad([o.sum() for o in off[:4]], [img, wav])
    for a, b in zip(gon, goff):
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


@pytest.mark.parametrize("node", NODES)
def test_a_node_is_capturable(mods, node):
    """forward + backward captured once in a torch.cuda.graph after a warm-up on a side stream, replayed once with fresh values in the static
    buffers: the eager bits"""
    shape = (2, 3, 34, 72)
    x = _input(node, shape, 51).to(DEV).requires_grad_(True)
    cot = torch.randn(mods.node(node, x).shape, generator=torch.Generator().manual_seed(52)).to(DEV)

    def run():
        y = mods.node(node, x)
        gx, = torch.autograd.grad(y, x, cot)
        return y.detach(), gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    with torch.no_grad():
        x.copy_(_input(node, shape, 53).to(DEV))
        cot.copy_(torch.randn(cot.shape, generator=torch.Generator().manual_seed(54)).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, run()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("node", ["dwt", "idwt", "up2"])
def test_second_grid_trip_of_the_capped_launchers(mods, node):
    """hav_haar_dwt / _idwt cap their grids at 16 workgroups per CU, hav_haar_up2 at 32 (csrc/hav_ops.hip), and loop: one map with more items
    than 256 threads x the cap, forward against the statement's bits and backward (the partner's capped kernel) against the statement's
    gradient.  hav_haar_down2 has no cap."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if node == "dwt":          # items: B C (H/2) (W/8)
        shape = (1, 1, 2 * (32 * cus + 1), 1024)
        items, cap = shape[2] // 2 * (shape[3] // 8), 16 * cus * 256
    elif node == "idwt":       # items: B C H (W/4)
        shape = (1, 1, 32 * cus + 1, 512)
        items, cap = shape[2] * (shape[3] // 4), 16 * cus * 256
    else:                      # items: B C (2H) (W/2)
        shape = (1, 1, 16 * cus + 1, 512)
        items, cap = 2 * shape[2] * (shape[3] // 2), 32 * cus * 256
    assert items > cap
    x = _input(node, shape, 61).to(DEV).requires_grad_(True)
    y = mods.node(node, x)
    x32 = x.detach().clone().requires_grad_(True)
    y32 = mods.statement(mods.d32, node, x32)
    assert torch.equal(y.detach(), y32.detach())
    cot = torch.randn(y.shape, generator=torch.Generator(device=DEV).manual_seed(62), device=DEV)
    gx, = torch.autograd.grad(y, x, cot)
    g32, = torch.autograd.grad(y32, x32, cot)
    assert (gx - g32).abs().max().item() <= 1e-5 * g32.abs().max().item()

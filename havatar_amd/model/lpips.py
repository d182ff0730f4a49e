"""LPIPS-VGG, the perceptual term of both training scripts' loss (reference train_avatar.py:24-29,138-142: 0.05 * LPIPS on the 64 x 64 patch;
train_avatarHD.py:268-274: 0.1 * LPIPS(fake_img, gt_hr_img)), as a module of this package: it needs neither the `lpips` package nor
torchvision, loads the weight files those two ship, and on HIP float32 tensors runs its 3x3 convolutions and per-tap heads on this
library's kernels (native/lpips_ops.py; HAVATAR_LPIPS, read at the call).

The function, for in0, in1 [B,3,H,W] in [-1, 1] (normalize=True maps from [0, 1] first):
    x <- (x - shift) / scale per channel, shift = [-.030, -.088, -.188], scale = [.458, .448, .450]
    VGG16 features[0:30]: 3x3 / padding 1 convolutions with bias, each followed by ReLU, widths 64,64 | 128,128 | 256,256,256 | 512,512,512 |
    512,512,512, a 2x2 / 2 max-pool in front of groups 2..5; the five taps are the ReLU outputs that end the groups
    per tap l:  a^ = a / (sqrt(sum_c a^2) + 1e-10), b^ likewise;  d_l[b] = mean_{h,w} sum_c w_l[c] (a^ - b^)^2
    result [B,1,1,1] = sum_l d_l
Eval-only: every parameter has requires_grad=False and dropout is the identity.

A freshly constructed module holds random weights and refuses forward() until load_weights() / load_state_dict() has run (allow_random=True
lifts that, for tests and benchmarks): a perceptual loss on random weights must never run silently."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10
# (slice, index in torchvision's vgg16().features, Cin, Cout) of the thirteen convolutions; a max-pool leads slices 2..5
CONVS = ((1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
         (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)


def key_table():
    """THE key map, one row per tensor: (this module's state-dict key = the `lpips` 0.1.x package's, the key in a torchvision VGG16 file or in
    an lpips linear-layer file, shape).  A key that turns out to be spelled differently in a file is a one-line fix here."""
    rows = [("scaling_layer.shift", None, (1, 3, 1, 1)), ("scaling_layer.scale", None, (1, 3, 1, 1))]
    for s, n, cin, cout in CONVS:
        rows.append(("net.slice%d.%d.weight" % (s, n), "features.%d.weight" % n, (cout, cin, 3, 3)))
        rows.append(("net.slice%d.%d.bias" % (s, n), "features.%d.bias" % n, (cout,)))
    for k, c in enumerate(TAP_CHANNELS):
        rows.append(("lin%d.model.1.weight" % k, "lin%d.model.1.weight" % k, (1, c, 1, 1)))
    return rows


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))

    def _apply(self, fn, *a, **k):
        # the two are constants of the function, not weights: after a dtype change they are the decimal values rounded ONCE to the new
        # dtype (a float32 buffer widened to float64 would carry float32's rounding, 2e-10 in the result)
        super()._apply(fn, *a, **k)
        self.shift = torch.tensor(SHIFT, dtype=self.shift.dtype, device=self.shift.device).view(1, 3, 1, 1)
        self.scale = torch.tensor(SCALE, dtype=self.scale.dtype, device=self.scale.device).view(1, 3, 1, 1)
        return self

    def forward(self, x):
        return (x - self.shift) / self.scale


class NetLinLayer(nn.Module):
    """the tap's 1x1 convolution without bias behind a dropout (the identity in eval): `model.1.weight`"""

    def __init__(self, chn_in):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


class _Vgg16(nn.Module):
    """features[0:30] cut into the five slices, every layer under torchvision's index"""

    def __init__(self):
        super().__init__()
        layers = {}
        for s, n, cin, cout in CONVS:
            layers[n] = (s, nn.Conv2d(cin, cout, 3, padding=1))
            layers[n + 1] = (s, nn.ReLU(inplace=False))
        for s, n in ((2, 4), (3, 9), (4, 16), (5, 23)):
            layers[n] = (s, nn.MaxPool2d(2, 2))
        for s in range(1, 6):
            seq = nn.Sequential()
            for n in sorted(layers):
                if layers[n][0] == s:
                    seq.add_module(str(n), layers[n][1])
            setattr(self, "slice%d" % s, seq)


def head_aten(a, b, w):
    """one tap, the PyTorch statement: a, b [B,C,H,W], w [1,C,1,1] -> [B,1,1,1]"""
    an = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + EPS)
    bn = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + EPS)
    return F.conv2d((an - bn) ** 2, w).mean([2, 3], keepdim=True)


class LPIPS(nn.Module):
    def __init__(self, net="vgg", allow_random=False):
        super().__init__()
        if net != "vgg":
            raise ValueError("LPIPS: only net='vgg' is built here (got %r)" % (net,))
        self.scaling_layer = ScalingLayer()
        self.net = _Vgg16()
        for k, c in enumerate(TAP_CHANNELS):
            setattr(self, "lin%d" % k, NetLinLayer(c))
        for p in self.parameters():
            p.requires_grad = False
        self.weights_loaded = bool(allow_random)
        self._packs = {}          # (conv index, device) -> (forward blob, data-gradient blob): the weights are frozen, packed once
        self.eval()

    def train(self, mode=True):
        return super().train(False)          # eval-only

    def _apply(self, fn, *a, **k):
        self._packs = {}
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict=True, **k):
        self._packs = {}
        # (the package's state dict names every lin layer twice: lin{K}.* and lins.K.*)
        state_dict = {key: v for key, v in state_dict.items() if not key.startswith("lins.")}
        r = super().load_state_dict(state_dict, strict=strict, **k)
        for name, const in (("shift", SHIFT), ("scale", SCALE)):
            got = getattr(self.scaling_layer, name).detach().flatten().double().cpu()
            if not torch.allclose(got, torch.tensor(const, dtype=torch.float64), rtol=0, atol=1e-6):
                raise RuntimeError("LPIPS: scaling_layer.%s = %s in the state dict, but the function fixes it at %s" % (name, got.tolist(), const))
        if strict:
            self.weights_loaded = True
        return r

    def packs(self, n, conv):
        from ..native import conv as nconv
        key = (n, conv.weight.device)
        if key not in self._packs:
            self._packs[key] = (nconv.pack(conv.weight, 1.0), nconv.pack_t(conv.weight, 1.0))
        return self._packs[key]

    def features(self, x, native):
        """the five taps of scaled x"""
        from ..native import lpips_ops
        taps = []
        for s in range(1, 6):
            seq = getattr(self.net, "slice%d" % s)
            names = list(seq._modules)
            i = 0
            while i < len(names):
                m = seq._modules[names[i]]
                if isinstance(m, nn.Conv2d):
                    if native and lpips_ops.conv_relu_eligible(x, m.weight):
                        x = lpips_ops.conv_relu_frozen(x, m.bias, *self.packs(int(names[i]), m), m.weight.shape[0])
                    else:          # conv1_1 (Cin = 3) and every shape the kernel does not take: ATen, inside the same forward
                        x = F.relu(F.conv2d(x, m.weight, m.bias, padding=1))
                    i += 2          # the ReLU behind it
                else:
                    x = m(x)
                    i += 1
            taps.append(x)
        return taps

    def forward(self, in0, in1, normalize=False):
        if not self.weights_loaded:
            raise RuntimeError("LPIPS: no weights loaded (load_weights(module, vgg=..., lin=...) or load_state_dict); a perceptual loss on "
                               "random weights is refused -- construct with allow_random=True to run one on purpose")
        from ..native import lpips_ops
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        native = lpips_ops.enabled() and in0.is_cuda and in0.dtype == torch.float32 and in1.dtype == torch.float32
        f0 = self.features(self.scaling_layer(in0), native)
        if in1.requires_grad or not torch.is_grad_enabled():
            f1 = self.features(self.scaling_layer(in1), native)
        else:
            with torch.no_grad():          # the target: its half of the backward never runs
                f1 = self.features(self.scaling_layer(in1), native)
        val = None
        for k in range(5):
            w = getattr(self, "lin%d" % k).model[1].weight
            d = lpips_ops.lpips_head(f0[k], f1[k], w) if native else head_aten(f0[k], f1[k], w)
            val = d if val is None else val + d
        return val


def _read(src):
    if src is None or isinstance(src, dict):
        return src
    obj = torch.load(os.fspath(src), map_location="cpu", weights_only=True)
    if isinstance(obj, dict) and "state_dict" in obj and isinstance(obj["state_dict"], dict):
        obj = obj["state_dict"]
    return obj


def load_weights(module, vgg=None, lin=None, state=None):
    """Fill `module` from any of: `vgg`, a torchvision VGG16 file or dict (`features.N.weight/bias`, or the same keys without the `features.`
    prefix); `lin`, an lpips linear-layer file or dict (`lin{K}.model.1.weight`; the duplicate `lins.K.*` keys are ignored); `state`, a
    whole LPIPS state dict (file or dict).  vgg and lin go together.  Refuses, naming the first missing or mis-shaped key.
    `scaling_layer.shift / .scale` are constants of the function, not weights: they are kept at the decimal values rounded once to the
    module's dtype (so the float64 module is exact), and a state dict that holds other values -- an LPIPS variant with its own input
    normalisation -- is refused by load_state_dict rather than silently overridden."""
    vgg, lin, state = _read(vgg), _read(lin), _read(state)
    if state is None and (vgg is None or lin is None):
        raise RuntimeError("load_weights: give `state`, or both `vgg` and `lin`")
    own = module.state_dict()
    new = {}
    for key, fkey, shape in key_table():
        if state is not None:
            src, names, what = state, (key,), "the LPIPS state dict"
        elif fkey is None:          # the scaling constants are not in either file
            new[key] = own[key]
            continue
        elif key.startswith("lin"):
            src, names, what = lin, (fkey,), "the linear-layer file"
        else:
            src, names, what = vgg, (fkey, fkey[len("features."):]), "the VGG16 file"
        name = next((n for n in names if n in src), None)
        if name is None:
            raise RuntimeError("load_weights: key %r is missing from %s" % (names[0], what))
        t = src[name]
        if tuple(t.shape) != shape:
            raise RuntimeError("load_weights: key %r of %s has shape %s, expected %s" % (name, what, tuple(t.shape), shape))
        new[key] = t.detach().to(device=own[key].device, dtype=own[key].dtype)
    module.load_state_dict(new, strict=True)
    return module


def from_package(device=None):
    """the weights of an installed `lpips` package copied into this module (ImportError if there is none)"""
    import lpips
    m = LPIPS(net="vgg")
    load_weights(m, state=lpips.LPIPS(net="vgg").state_dict())
    return m if device is None else m.to(device)


def build_for_harness(vgg_path, lin_path, device):
    """what `--percep native` of both harnesses builds: from the two files, else from an installed `lpips` package, else a refusal"""
    if vgg_path or lin_path:
        if not (vgg_path and lin_path):
            raise RuntimeError("--percep native needs both --percep-vgg PATH (torchvision VGG16 weights) and --percep-lin PATH (lpips linear "
                               "layers)")
        return load_weights(LPIPS(net="vgg"), vgg=vgg_path, lin=lin_path).to(device)
    try:
        return from_package(device)
    except ImportError as e:
        raise RuntimeError("--percep native needs --percep-vgg PATH (torchvision VGG16 weights) and --percep-lin PATH (lpips linear layers), "
                           "or an installed `lpips` package to copy them from; or pass --percep none") from e

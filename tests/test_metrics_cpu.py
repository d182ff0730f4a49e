"""CPU: havatar_amd.metrics (the ATen statement of SSIM / mse / PSNR) against the float64 restatement of tests/metrics_util.py, its analytic cases
and refusals, the binding of the three entries of csrc/hav_metrics.hip within ABI 8, the compiler's output for gfx950, the reader's `with_gt`, and
`avatarHD_reenactment.py --metrics` end to end on CPU tensors."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import lpips_util as lu
import metrics_util as mu
from havatar_amd import metrics, synth
from havatar_amd.dataloader import imgio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------------------------------------------
# the function
# ------------------------------------------------------------------------------------------------------------------------------------
def test_window_is_the_normalised_gaussian():
    g = metrics.gaussian_window(torch.float64).numpy()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1])
    assert np.abs(np.outer(g, g) - mu.window2d()).max() <= 1e-16
    assert metrics.gaussian_window(torch.float32).dtype == torch.float32


@pytest.mark.parametrize("kind", mu.KINDS)
@pytest.mark.parametrize("shape", [(2, 3, 12, 13), (1, 2, 40, 57)])
def test_statement_in_float64_matches_the_restatement(kind, shape):
    """value and map to 1e-12 (both sides float64; one sums the window separably, the other as an outer product)"""
    a, b = (t.double() for t in mu.pair(kind, shape))
    s, m = metrics.ssim(a, b, return_map=True)
    ref, ref_map = mu.ssim64(a.numpy(), b.numpy())
    assert s.dtype == torch.float64 and tuple(m.shape) == (shape[0], shape[1], shape[2] - 10, shape[3] - 10)
    assert np.abs(s.numpy() - ref).max() <= 1e-12 and np.abs(m.numpy() - ref_map).max() <= 1e-12
    d = metrics.image_metrics(a, b)
    assert np.abs(d["mse"].numpy() - mu.mse64(a.numpy(), b.numpy())).max() <= 1e-15
    assert torch.equal(d["ssim"], s) and torch.equal(d["psnr"], metrics.psnr(a, b))
    assert np.abs(d["psnr"].numpy() - (-10 * np.log10(mu.mse64(a.numpy(), b.numpy())))).max() <= 1e-10
    # a data range of its own: SSIM is invariant under a common scale when L scales along
    s255 = metrics.ssim(a * 255, b * 255, data_range=255.0)
    assert np.abs(s255.numpy() - ref).max() <= 1e-12


@pytest.mark.parametrize("kind", mu.KINDS)
def test_statement_on_uint8_matches_the_restatement(kind):
    """uint8 [B,H,W,3]: SSIM of x / 255 to 1e-12, mse the exact integer sum / (255^2 N)"""
    a, b = mu.pair_u8(kind, (2, 3, 23, 31))
    d = metrics.image_metrics(a, b)
    s, mse = mu.u8_truth(a.numpy(), b.numpy())
    assert d["ssim"].dtype == torch.float64 and np.abs(d["ssim"].numpy() - s).max() <= 1e-12
    assert np.array_equal(d["mse"].numpy(), mse)
    assert np.abs(metrics.ssim(a, b).numpy() - s).max() <= 1e-12
    assert np.abs(metrics.psnr(a, b).numpy() - (-10 * np.log10(mse))).max() <= 1e-10


def test_float32_cpu_pairs_are_scored_in_float64():
    a, b = mu.pair("flat", (1, 3, 32, 32))
    s = metrics.ssim(a, b)
    assert s.dtype == torch.float64 and np.abs(s.numpy() - mu.truth("flat", (1, 3, 32, 32))[0]).max() <= 1e-12


def test_analytic_cases():
    a = mu.pair("texture", (2, 3, 24, 24))[0]
    for x in (a, a.double(), (a * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()):
        d = metrics.image_metrics(x, x.clone())
        assert torch.equal(d["ssim"], torch.ones(2, dtype=torch.float64)) and torch.equal(d["mse"], torch.zeros(2, dtype=torch.float64))
        assert torch.isinf(d["psnr"]).all() and (d["psnr"] > 0).all()
        s, m = metrics.ssim(x, x.clone(), return_map=True)
        assert torch.equal(m, torch.ones_like(m))
    # two constant images: every variance and the covariance vanish
    for c1, c2, L in ((0.25, 0.75, 1.0), (1.0, 0.999, 1.0), (40.0, 200.0, 255.0)):
        x, y = torch.full((1, 2, 16, 20), c1, dtype=torch.float64), torch.full((1, 2, 16, 20), c2, dtype=torch.float64)
        C1 = (0.01 * L) ** 2
        want = (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)
        assert abs(float(metrics.ssim(x, y, data_range=L)) - want) <= 1e-12
        assert abs(float(metrics.psnr(x, y, data_range=L)) - 10 * math.log10(L * L / (c1 - c2) ** 2)) <= 1e-9


def test_refusals_name_the_shape():
    z = torch.zeros
    with pytest.raises(ValueError, match=r"H, W >= 11.*\(1, 3, 10, 64\)"):
        metrics.ssim(z(1, 3, 10, 64), z(1, 3, 10, 64))
    with pytest.raises(ValueError, match=r"H, W >= 11.*\(1, 64, 10, 3\)"):
        metrics.image_metrics(z(1, 64, 10, 3, dtype=torch.uint8), z(1, 64, 10, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(1, 3, 16, 16\) and \(1, 3, 16, 17\)"):
        metrics.psnr(z(1, 3, 16, 16), z(1, 3, 16, 17))
    with pytest.raises(ValueError, match=r"dtype.*float32.*float64"):
        metrics.ssim(z(1, 3, 16, 16), z(1, 3, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"channels-last.*\(1, 3, 16, 16\)"):
        metrics.ssim(z(1, 3, 16, 16, dtype=torch.uint8), z(1, 3, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(3, 16, 16\)"):
        metrics.ssim(z(3, 16, 16), z(3, 16, 16))


def test_switch_is_read_at_the_call_and_cpu_tensors_never_reach_the_library(monkeypatch):
    from havatar_amd.native import metrics_ops as o
    monkeypatch.delenv("HAVATAR_METRICS", raising=False)
    assert o.enabled() is (o.DEFAULT != "0") and o.DEFAULT == "1"
    monkeypatch.setenv("HAVATAR_METRICS", "0")
    assert not o.enabled()
    monkeypatch.setenv("HAVATAR_METRICS", "1")
    assert o.enabled()
    ran = []
    monkeypatch.setattr(o, "image_metrics_f32", lambda *a, **k: ran.append("f32"))
    monkeypatch.setattr(o, "image_metrics_u8", lambda *a, **k: ran.append("u8"))
    a, b = mu.pair("texture", (1, 3, 16, 16))
    metrics.ssim(a, b)
    metrics.image_metrics(*mu.pair_u8("texture", (1, 3, 16, 16)))
    assert ran == [] and not o.eligible(a, b)


def test_wrappers_refuse_cpu_tensors():
    from havatar_amd.native import metrics_ops as o
    f, u = torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    for call in (lambda: o.image_metrics_f32(f, f), lambda: o.image_metrics_u8(u, u), lambda: o.image_metrics_f32(u, u)):
        with pytest.raises(RuntimeError, match="HIP"):
            call()


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's entries
# ------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_entries():
    from havatar_amd import _lib, build
    from havatar_amd.native import metrics_ops as o
    L = _lib.lib()
    assert L.hav_image_metrics_blocks.restype is C.c_int64 and L.hav_image_metrics_blocks.argtypes == [C.c_int] * 4
    assert L.hav_image_metrics_f32.restype is C.c_int
    assert L.hav_image_metrics_f32.argtypes == [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_float, C.c_void_p]
    assert L.hav_image_metrics_u8.restype is C.c_int and L.hav_image_metrics_u8.argtypes == [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]
    assert _lib.ABI_VERSION == L.hav_abi_version() == 8          # additions within the version: nothing existing changed
    assert "hav_metrics.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "havatar.h")).read()
    for name in ("hav_image_metrics_blocks", "hav_image_metrics_f32", "hav_image_metrics_u8"):
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "#define HAV_ABI_VERSION 8" in hdr
    # refusals that need no device: HAV_EINVAL for null pointers and sizes below 1, HAV_EUNSUP below the window, all before any launch
    one = C.c_void_p(16)          # never dereferenced: the checks come first
    assert L.hav_image_metrics_f32(None, None, None, None, None, 1, 3, 16, 16, 1.0, None) == -1
    assert L.hav_image_metrics_u8(None, None, None, None, None, 1, 16, 16, None) == -1
    for miss in range(4):
        ptrs = [None if k == miss else one for k in range(4)]
        assert L.hav_image_metrics_f32(ptrs[0], ptrs[1], None, ptrs[2], ptrs[3], 1, 3, 16, 16, 1.0, None) == -1
        assert L.hav_image_metrics_u8(ptrs[0], ptrs[1], None, ptrs[2], ptrs[3], 1, 16, 16, None) == -1
    for B, Cc, H, W in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, -1)):
        assert L.hav_image_metrics_f32(one, one, None, one, one, B, Cc, H, W, 1.0, None) == -1
    assert L.hav_image_metrics_u8(one, one, None, one, one, 0, 16, 16, None) == -1
    for dr in (0.0, -1.0, float("nan"), float("inf")):
        assert L.hav_image_metrics_f32(one, one, None, one, one, 1, 3, 16, 16, dr, None) == -1
    for H, W in ((10, 64), (64, 10), (1, 1)):
        assert L.hav_image_metrics_f32(one, one, None, one, one, 1, 3, H, W, 1.0, None) == -2
        assert L.hav_image_metrics_u8(one, one, None, one, one, 1, H, W, None) == -2
    assert L.hav_image_metrics_f32(one, one, None, one, one, 65536, 65536, 42, 42, 1.0, None) == -2          # 2^32 workgroups
    # the tile extents the wrappers export are the kernel's
    src = open(os.path.join(ROOT, "havatar_amd", "csrc", "hav_metrics.hip")).read()
    assert int(re.search(r"#define MET_TH (\d+)", src).group(1)) == o.TILE_H and int(re.search(r"#define MET_TW (\d+)", src).group(1)) == o.TILE_W
    code = re.sub(r"//[^\n]*", "", src)
    assert "getenv" not in code and not re.search(r"atomic", code, re.I)          # no environment reads, no atomics in the file's code


def test_partials_count():
    """two float64 per workgroup of TILE_H x TILE_W map elements; 0 for refused sizes"""
    from havatar_amd import _lib
    from havatar_amd.native import metrics_ops as o
    L = _lib.lib()
    for B, Cc, H, W in ((1, 1, 11, 11), (2, 3, 12, 13), (1, 3, 42, 42), (1, 3, 43, 42), (1, 3, 42, 43), (1, 3, 79, 109), (2, 3, 64, 64),
                        (1, 3, 512, 512), (4, 3, 1024, 1024)):
        want = 2 * B * Cc * (-(-(H - 10) // o.TILE_H)) * (-(-(W - 10) // o.TILE_W))
        assert L.hav_image_metrics_blocks(B, Cc, H, W) == want, (B, Cc, H, W)
    for B, Cc, H, W in ((0, 3, 64, 64), (1, 0, 64, 64), (1, 3, 10, 64), (1, 3, 64, 10), (-1, 3, 64, 64), (65536, 65536, 42, 42)):
        assert L.hav_image_metrics_blocks(B, Cc, H, W) == 0, (B, Cc, H, W)
    assert L.hav_image_metrics_blocks(32768, 65535, 42, 42) == 2 * 32768 * 65535          # just inside 2^31 - 1 workgroups


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_codegen_no_private_segment_and_no_spill(tmp_path):
    dst = str(tmp_path / "hav_metrics.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                    os.path.join(ROOT, "havatar_amd", "csrc", "hav_metrics.hip")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    text = open(dst).read()
    kernels = re.findall(r"\.name:\s+(\S*_kernel\S*)", text)
    # the tile kernel for float with 16-byte and 4-byte loads and for uint8, and the final sum
    assert len(set(kernels)) == 4 and sum("metrics_tile" in k for k in kernels) == 3 and sum("metrics_final" in k for k in kernels) == 1, kernels
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(scratch) == len(kernels) and all(v == 0 for v in scratch), scratch
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)] + [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == 2 * len(kernels) and all(v == 0 for v in spills), spills
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert max(lds) <= 80 * 1024, lds          # two workgroups per compute unit (160 KiB)


# ------------------------------------------------------------------------------------------------------------------------------------
# the reader
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("metrics_dataset")
    return str(root), synth.write_dataset(str(root), n_frames=2, img_res=128)


def test_reader_with_gt(dataset):
    from havatar_amd.dataloader.dataloaderSR import MultiView_ImgDataset
    from havatar_amd.utils.cfgnode import CfgNode
    cfg = CfgNode(synth.harness_config())
    ds = MultiView_ImgDataset(dataset[1], "test", cfg, cfg.dataset.down_sample)
    assert MultiView_ImgDataset.with_gt is False
    base = {"fidx", "vidx", "front_render_cond", "left_render_cond", "right_render_cond", "inv_head_T"}
    assert set(ds[0][1]) == base | {"mv_rays"}
    ds.device_rays = True
    assert set(ds[0][1]) == base | {"camera"}
    train = MultiView_ImgDataset(dataset[1], "train", cfg, cfg.dataset.down_sample)
    gts = mu.split_ground_truth(dataset[1])
    for rays in (False, True):
        ds = MultiView_ImgDataset(dataset[1], "test", cfg, cfg.dataset.down_sample)
        ds.device_rays, ds.with_gt = rays, True
        for k in range(len(ds)):
            item = ds[k][1]
            assert set(item) == base | {"camera" if rays else "mv_rays", "gt_img"}
            gt = item["gt_img"]
            assert gt.dtype == torch.uint8 and tuple(gt.shape) == (128, 128, 3)
            want = torch.round(train[k][1]["mv_rays_gt_color"] * 255).to(torch.uint8).reshape(128, 128, 3)
            assert torch.equal(gt, want) and np.array_equal(gt.numpy(), gts[(int(item["fidx"]), 0)])
            assert (gt == 255).all(-1).float().mean() > 0.05          # the white background is in it


# ------------------------------------------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------------------------------------------
def _write_cfg(path, **kw):
    with open(path, "w") as f:
        yaml.safe_dump(synth.harness_config(**kw), f)
    return str(path)


def _run(tmp, dataset, *extra):
    from havatar_amd.harness import reenact
    os.makedirs(tmp, exist_ok=True)
    cfg_path, ckpt = _write_cfg(os.path.join(tmp, "cfg.yml")), mu.checkpoint(os.path.join(tmp, "avatar.pth"))
    out = os.path.join(tmp, "renders")
    written = reenact.main(["--config", cfg_path, "--ckpt", ckpt, "--savedir", out, "--split", dataset[1]] + list(extra), device="cpu")
    return out, written


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory, dataset):
    os.environ["HAVATAR_WORKERS"] = "0"
    try:
        out, written = _run(str(tmp_path_factory.mktemp("metrics_cli")), dataset, "--metrics")
    finally:
        os.environ.pop("HAVATAR_WORKERS", None)
    with open(os.path.join(out, "metrics.json")) as f:
        return out, written, json.load(f)


def test_cli_writes_the_table(one_rank, dataset):
    out, written, table = one_rank
    assert [os.path.basename(p) for p in written] == ["0_00.png", "1_00.png"]
    assert set(table) == {"definition", "frames", "mean", "n", "n_identical"} and table["n"] == 2 and table["n_identical"] == 0
    assert [f["file"] for f in table["frames"]] == [os.path.join("rgb", "0_00.png"), os.path.join("rgb", "1_00.png")]
    assert all(set(f) == {"file", "fidx", "view", "mse", "psnr", "ssim"} for f in table["frames"]) and set(table["mean"]) == {"psnr", "ssim"}
    d = table["definition"]
    assert d["sigma"] == 1.5 and d["on"] == "uint8 as written" and "valid" in d["windows"] and "11 taps" in d["window"] and "not evaluated" in d["lpips"]
    mu.check_table(table, out, mu.split_ground_truth(dataset[1]), ssim_tol=1e-9)
    assert all(0 < f["ssim"] < 1 and 0 < f["psnr"] < 60 for f in table["frames"])


def test_cli_batched_frames_give_the_same_table(one_rank, dataset, tmp_path, monkeypatch):
    monkeypatch.setenv("HAVATAR_FRAME_BATCH", "2")
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    out, _ = _run(str(tmp_path), dataset, "--metrics")
    with open(os.path.join(out, "metrics.json")) as f:
        table = json.load(f)
    mu.check_table(table, out, mu.split_ground_truth(dataset[1]), ssim_tol=1e-9)
    same_png = all(np.array_equal(imgio.imread_rgb(os.path.join(out, f["file"])), imgio.imread_rgb(os.path.join(one_rank[0], f["file"])))
                   for f in table["frames"])
    assert [(f["file"], f["fidx"], f["view"]) for f in table["frames"]] == [(f["file"], f["fidx"], f["view"]) for f in one_rank[2]["frames"]]
    # on CPU tensors a batch renders the pixels of its frames rendered alone, so the whole file is the same
    assert same_png, "the batched run wrote other pixels: the tables cannot be compared"
    assert table == one_rank[2]


def test_cli_two_ranks_merge_to_the_one_rank_table(one_rank, dataset, tmp_path, monkeypatch):
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        out, written = _run(str(tmp_path), dataset, "--metrics")
        assert [os.path.basename(p) for p in written] == ["%d_00.png" % rank]
    assert not os.path.exists(os.path.join(out, "metrics.json"))
    parts = [os.path.join(out, "metrics_rank%dof2.json" % r) for r in (1, 0)]
    merged = metrics.merge(parts, out=os.path.join(out, "metrics.json"))
    assert merged == one_rank[2]
    with open(os.path.join(out, "metrics.json")) as f:
        assert json.load(f) == one_rank[2]


def test_cli_refuses_a_size_mismatch_before_rendering(dataset, tmp_path):
    from havatar_amd.harness import reenact
    cfg_path = _write_cfg(tmp_path / "cfg.yml", gen_size=64)
    with pytest.raises(RuntimeError, match=r"out_size 64 .*img_res 128"):          # (before the checkpoint is even opened: there is none)
        reenact.main(["--config", cfg_path, "--ckpt", str(tmp_path / "none.pth"), "--savedir", str(tmp_path / "o"), "--split", dataset[1],
                      "--metrics"], device="cpu")
    assert not os.path.exists(tmp_path / "o" / "metrics.json") and os.listdir(tmp_path / "o" / "rgb") == []


def test_cli_refuses_one_lpips_path_by_its_own_flags(dataset, tmp_path):
    from havatar_amd.harness import reenact
    cfg_path = _write_cfg(tmp_path / "cfg.yml")
    for flag in ("--percep-vgg", "--percep-lin"):
        with pytest.raises(RuntimeError, match=r"--metrics: LPIPS needs both --percep-vgg .* --percep-lin"):
            reenact.main(["--config", cfg_path, "--ckpt", str(tmp_path / "none.pth"), "--savedir", str(tmp_path / "o"), "--split", dataset[1],
                          "--metrics", flag, str(tmp_path / "w.pth")], device="cpu")


def test_cli_without_the_flag_writes_no_table_and_the_same_pngs(one_rank, dataset, tmp_path, monkeypatch):
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    out, written = _run(str(tmp_path), dataset)
    assert sorted(os.listdir(out)) == ["rgb"] and sorted(os.listdir(os.path.join(out, "rgb"))) == ["0_00.png", "1_00.png"]
    for p, q in zip(written, one_rank[1]):
        assert open(p, "rb").read() == open(q, "rb").read()


def test_cli_with_lpips_files_reports_lpips(dataset, tmp_path, monkeypatch):
    monkeypatch.setenv("HAVATAR_WORKERS", "0")
    vgg, lin = lu.weights()
    torch.save(dict(vgg), tmp_path / "vgg16.pth")
    torch.save(dict(lin), tmp_path / "lin.pth")
    out, _ = _run(str(tmp_path / "run"), dataset, "--metrics", "--percep-vgg", str(tmp_path / "vgg16.pth"), "--percep-lin", str(tmp_path / "lin.pth"))
    with open(os.path.join(out, "metrics.json")) as f:
        table = json.load(f)
    assert all(np.isfinite(f["lpips"]) and f["lpips"] > 0 for f in table["frames"]) and "LPIPS-VGG" in table["definition"]["lpips"]
    assert table["mean"]["lpips"] == sum(f["lpips"] for f in table["frames"]) / 2
    mu.check_table(table, out, mu.split_ground_truth(dataset[1]), ssim_tol=1e-9)
    # its value is the module's on the same pair
    m = lu.module()
    gts = mu.split_ground_truth(dataset[1])
    for f in table["frames"]:
        png = torch.from_numpy(np.asarray(imgio.imread_rgb(os.path.join(out, f["file"]))))
        a, b = (t.permute(2, 0, 1)[None].float() / 127.5 - 1.0 for t in (png, torch.from_numpy(gts[(f["fidx"], f["view"])])))
        with torch.no_grad():
            assert abs(float(m(a, b)) - f["lpips"]) <= 1e-6

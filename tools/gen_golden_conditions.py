"""Record the reference's own numbers for the condition-image definition into tests/golden/conditions.npz (a few KB).

    python tools/gen_golden_conditions.py --reference <reference checkout>

Runs the reference's `depth2normal_ortho` (data_preprocessing/core/utils.py, imported by path with an empty stand-in for the absent cv2) on
three small depth maps and `get_box_warp_param` (utils/util.py) on the orthographic bounds.  Numbers only; never imported by a test.
Sizes: B = 1 and no dimension of length 3 -- the reference calls torch.cross without `dim`, and legacy ATen then takes the first axis of
size 3 (so H - 2 and W - 2 must not be 3 either)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def depth_maps():
    """name -> (D [1,H,W] float32, dx, dy)"""
    out = {}
    H = W = 33
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    X, Y = (2 * xx + 1) / W - 1, (2 * yy + 1) / H - 1
    r2 = (X ** 2 + Y ** 2) / 0.8 ** 2
    out["sphere"] = (np.where(r2 < 1, 10.0 - 0.8 * np.sqrt(np.clip(1 - r2, 0, 1)), -1.0), -2.0 / W, -2.0 / H)
    H, W = 12, 17
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out["step"] = (np.where(xx < 6, -1.0, np.where(xx < 11, 9.25, 9.75)) + 0.0 * yy, -2.0 / W, -2.0 / H)
    H, W = 9, 14
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out["ramp"] = (9.0 + 0.031 * xx - 0.017 * yy + 0.002 * xx * yy, -2.0 / W, -2.0 / H)
    return {k: (np.asarray(d, np.float32)[None], dx, dy) for k, (d, dx, dy) in out.items()}


def load(path, name, stubs=()):
    for s in stubs:
        sys.modules.setdefault(s, types.ModuleType(s))
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reference", required=True)
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conditions.npz"))
    args = p.parse_args()
    core = load(os.path.join(args.reference, "data_preprocessing", "core", "utils.py"), "_ref_core_utils", stubs=("cv2",))
    util = load(os.path.join(args.reference, "utils", "util.py"), "_ref_util")
    rec = {}
    for name, (D, dx, dy) in depth_maps().items():
        assert D.shape[0] == 1 and 3 not in D.shape and 5 not in D.shape[1:], D.shape
        n = core.depth2normal_ortho(torch.from_numpy(D), dx=dx, dy=dy).numpy()
        rec[name + "_depth"], rec[name + "_dxdy"], rec[name + "_normal"] = D, np.asarray([dx, dy], np.float64), n.astype(np.float32)
    scales, trans = util.get_box_warp_param(np.asarray([-1.5, 1.5]), np.asarray([-1.6, 1.4]), np.asarray([-1.6, 1.2]))
    rec["warp_scale"], rec["warp_trans"] = np.asarray(scales, np.float64), np.asarray(trans, np.float64)
    np.savez_compressed(args.out, **rec)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()

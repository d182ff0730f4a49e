#!/usr/bin/env python3
"""tests/golden/discriminator.npz from the reference's own Discriminator and stage-two helpers (model/styleUnet.py:470-562,
utils/styleUnet_util.py), imported from a reference checkout through oracle/gen_golden.py::import_reference() and run on the CPU by the
driver both sides share (havatar_amd/harness/stage2_cases.py).  The file holds key lists, checksums, slices and the few predictions and
losses -- numbers only; weights come from synth.fill_state_dict on both sides.  Needs the reference checkout; never imported by a test.

    python tools/gen_golden_discriminator.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True


def main():
    from oracle import gen_golden
    gen_golden.import_reference()
    from model.styleUnet import Discriminator          # the reference's (its checkout is first on sys.path now)
    import utils.styleUnet_util as ref_util
    from havatar_amd.harness import stage2_cases
    out = stage2_cases.run(Discriminator, ref_util)
    dst = os.path.join(gen_golden.OUT, "discriminator.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()

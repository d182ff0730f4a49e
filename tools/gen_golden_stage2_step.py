#!/usr/bin/env python3
"""tests/golden/stage2_step.npz from the reference's own Trainer, SWGAN_unet, Discriminator and stage-two helpers, imported from a reference
checkout through oracle/gen_golden.py::import_reference() and run on the CPU by the driver both sides share
(havatar_amd/harness/stage2_step_cases.py: two joint iterations, i = 0 with R1 and i = 1).  The file holds names, scalars, checksums and
slices -- numbers only; weights come from synth.fill_state_dict on both sides.  Needs the reference checkout; never imported by a test.

    python tools/gen_golden_stage2_step.py
"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True


def main():
    from oracle import gen_golden
    _, Trainer, _ = gen_golden.import_reference()
    from model.styleUnet import Discriminator, SWGAN_unet          # the reference's (its checkout is first on sys.path now)
    import utils.styleUnet_util as ref_util
    from havatar_amd import synth
    from havatar_amd.harness import stage2_step_cases
    split = synth.write_dataset(tempfile.mkdtemp(), n_frames=2, img_res=128)
    out = stage2_step_cases.run(Trainer, SWGAN_unet, Discriminator, ref_util, split)
    dst = os.path.join(gen_golden.OUT, "stage2_step.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Entry script with the reference's name and flags (train_avatarHD.py); see havatar_amd/harness/train_hd.py."""
import os

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the first HIP call (havatar_amd/__init__.py)

from havatar_amd.harness.train_hd import main, seed_all

if __name__ == "__main__":
    seed_all()
    main()

#!/usr/bin/env python3
"""Generate tests/golden/g22_long_clips.npz: the REAL reference's D3DP at 243-frame clips (the reference's in-the-wild
default, ``MixSTE2(num_frame=243)`` per part), on CPU.

Runs only in the build container, next to make_golden.py (same shims, same FakeDataset, same NoiseTape, same writer;
nothing of the reference is copied).  Real widths, depth 2 (``model.dep``; keeps the CPU run short), seeded weights
(golden_util.seeded_state_dict, seed 243) pinned by their SHA-256.  The inputs are not stored: they are re-generated from
seeds by the synthetic helpers (``frames=243``) and pinned by a SHA-256 of their own.

  flip_out     D3DP.forward, flip-TTA, B=1 P=1 T=2 (both steps)   [1, 2, 1, 243, 134, 3]   (~680 KB)

The no-flip sampler at 243 frames is compared with the CPU oracle only (tests/test_hip_long_clips.py).

Usage:  python tests/golden/make_golden_long.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

from tests.golden import golden_util as gu  # noqa: E402
from tests.golden.g22_inputs import DEPTH, FRAMES, SEED, P, T, digest, inputs  # noqa: E402


def build(P, T, flip):
    from common.diffusionpose import D3DP
    args = mg.make_args()
    args.model.number_of_frames, args.model.dep, args.model.test_time_augmentation = FRAMES, DEPTH, flip
    m = D3DP(args, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, mg.FakeDataset(), is_train=False, num_proposals=P,
             sampling_timesteps=T)
    m.device = "cpu"
    return m.eval()


def main():
    mg.install_shims()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    z = inputs()
    m = build(P, T, True)
    sd = gu.seeded_state_dict(m.state_dict(), seed=SEED)
    m.load_state_dict(sd)
    assert tuple(sd["pose_estimator.body.Temporal_pos_embed"].shape) == (1, FRAMES, 384)
    with mg.NoiseTape(list(z["noise_flip"])) as tape, torch.no_grad():
        flip_out = m(z["x2d"], None, input_2d_flip=z["x2d_flip"])
        assert tape.k == T
    assert flip_out.shape == (1, T, P, FRAMES, 134, 3)
    mg.save("g22_long_clips.npz", sha=np.frombuffer(gu.sha256_of(sd), dtype=np.uint8),
            inputs_sha=np.frombuffer(digest(z), dtype=np.uint8), flip_out=flip_out)


if __name__ == "__main__":
    main()

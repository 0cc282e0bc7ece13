"""Inputs of G21's random case, re-generated from a seed: the fixture stores their SHA-256, not the arrays
(tests/golden/make_golden_p2.py)."""
import torch

from oracle import d3dp_oracle as orc
from tests.golden import golden_util as gu

RANDOM_SEED = 211
RANDOM_SIZES = (2, 3, 5, 27)         # B, T, P, F (J = 134)


def random_inputs(seed=RANDOM_SEED, sizes=RANDOM_SIZES):
    """G9-style random part-centred predictions and target, 2-D input and root trajectory"""
    B, T, P, Fr = sizes
    g = torch.Generator().manual_seed(seed)
    return {"pred_parts": orc.center_pose_parts(torch.randn(B, T, P, Fr, 134, 3, generator=g) * 0.3),
            "gt_parts": orc.center_pose_parts(torch.randn(B, Fr, 134, 3, generator=g) * 0.3),
            "x2d": torch.rand(B, Fr, 134, 2, generator=g) * 2 - 1,
            "traj": torch.randn(B, Fr, 1, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])}


def digest(inputs):
    return gu.sha256_of(inputs)

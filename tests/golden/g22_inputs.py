"""Inputs of G22 (243-frame clips), re-generated from seeds: the fixture stores their SHA-256, not the arrays
(tests/golden/make_golden_long.py)."""
import torch

from tests.golden import golden_util as gu

FRAMES, DEPTH, SEED = 243, 2, 243     # clip length, model.dep, weight seed (golden_util.seeded_state_dict)
P, T = 1, 2                           # flip-TTA loop


def inputs():
    """2-D clip and its flip, the two noise draws of the loop"""
    x2d, x2f = gu.synthetic_inputs_2d(B=1, seed=2431, frames=FRAMES)
    return {"x2d": x2d, "x2d_flip": x2f,
            "noise_flip": torch.stack(gu.synthetic_noises(B=1, P=P, n=T, seed=2432, frames=FRAMES))}


def digest(z):
    return gu.sha256_of(z)

"""Noise stream v1 on the host (pafuse_amd/noise.py): the generator against its published
known-answer vectors, the slicing property that makes sharding and chunking invisible, the moments of the normals, and
the interface of the "device" noise source of pafuse_amd.D3DP as far as it can be checked without a GPU.

The statistical bounds are five standard errors of the estimator under the hypothesis "independent N(0, 1)":
  mean of n values            sigma = 1 / sqrt(n)
  variance of n values        sigma = sqrt(2 / n)       (fourth central moment 3)
  correlation of two streams  sigma = 1 / sqrt(n)
A correct stream misses one of them with probability 6e-7; they are derived, not tuned.
"""
import os
import re

import numpy as np
import pytest

from pafuse_amd import noise
from tests.conftest import ROOT


def test_philox4x32_10_known_answers():
    """The three known-answer vectors of Random123 (kat_vectors: philox4x32 10)."""
    f = 0xFFFFFFFF
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = tuple(int(v) for v in noise.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(v) for v in got])
    # vectorised: the three at once
    got = noise.philox4x32_10([np.array([c[0][i] for c in cases], dtype=np.uint32) for i in range(4)],
                              [np.array([c[1][i] for c in cases], dtype=np.uint32) for i in range(2)])
    assert [tuple(int(got[i][n]) for i in range(4)) for n in range(3)] == [c[2] for c in cases]


def test_uniform_is_exact_and_open():
    r = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    u = noise.uniform(r)
    assert u.dtype == np.float64 and u[0] == 2.0 ** -33 and u[-1] == 1.0 - 2.0 ** -33 and u[2] == 0.5 + 2.0 ** -33
    assert np.all(u > 0) and np.all(u < 1)


def test_sincos_fold_is_accurate_next_to_the_zeros():
    """the words next to a quarter / half turn: sin or cos is ~ +-2 pi 2^-33 there, and must be good RELATIVELY"""
    import math
    from fractions import Fraction
    words = [0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, 2 ** 31, 3 * 2 ** 30 - 1, 3 * 2 ** 30, 2 ** 32 - 1, 12345, 2 ** 29, 2 ** 29 - 1]
    s, c = noise.sincos_turns(np.array(words, dtype=np.uint32))
    for i, r in enumerate(words):
        # reference: the angle relative to the nearest quarter turn, exactly, then a Taylor series in rationals
        n = 2 * r + 1
        q = ((r >> 29) + 1) >> 1
        d = Fraction(n - q * 2 ** 31, 2 ** 33)
        pi = Fraction(3141592653589793238462643383279502884197, 10 ** 39)
        x = 2 * pi * d
        sin = sum(Fraction((-1) ** k) * x ** (2 * k + 1) / math.factorial(2 * k + 1) for k in range(14))
        cos = sum(Fraction((-1) ** k) * x ** (2 * k) / math.factorial(2 * k) for k in range(14))
        want_s, want_c = [(sin, cos), (cos, -sin), (-sin, -cos), (-cos, sin)][q & 3]
        for got, want in ((s[i], want_s), (c[i], want_c)):
            assert abs(Fraction(float(got)) - want) <= abs(want) * Fraction(8, 2 ** 53), (r, float(got), float(want))


def test_reference_draw_of_a_shard_or_a_clip_range_is_the_slice_of_the_full_draw():
    full = noise.reference_draw(seed=11, call=3, k=2, b0=0, p0=0, B=4, P=8, F=5, J=134)
    assert full.shape == (4, 8, 5, 134, 3) and full.dtype == np.float32
    for lo, hi in ((0, 3), (3, 6), (6, 8), (5, 6)):
        assert np.array_equal(noise.reference_draw(11, 3, 2, 0, lo, 4, hi - lo, 5, 134), full[:, lo:hi])
    for b0, b1 in ((0, 1), (1, 4), (3, 4)):
        assert np.array_equal(noise.reference_draw(11, 3, 2, b0, 0, b1 - b0, 8, 5, 134), full[b0:b1])
    assert np.array_equal(noise.reference_draw(11, 3, 2, 2, 5, 2, 2, 5, 134), full[2:4, 5:7])
    for other in (dict(seed=12), dict(call=4), dict(k=1)):      # another key word or another draw: other values
        kw = dict(seed=11, call=3, k=2, b0=0, p0=0, B=4, P=8, F=5, J=134)
        kw.update(other)
        assert not np.array_equal(noise.reference_draw(**kw), full), other
    with pytest.raises(ValueError):
        noise.reference_draw(2 ** 32, 0, 0, 0, 0, 1, 1, 1, 1)


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_moments_and_independence_of_neighbouring_streams():
    F, J, B, P = 27, 134, 4, 24                            # 4 * 24 * 27 * 134 * 3 = 1 041 984 values per draw
    x = noise.reference_draw(seed=5, call=0, k=0, b0=0, p0=0, B=B, P=P, F=F, J=J)
    n = x.size
    assert n >= 10 ** 6
    v = x.astype(np.float64)
    print(f"n = {n}: mean {v.mean():+.3e} (bound {5 / np.sqrt(n):.3e}), var - 1 {v.var() - 1:+.3e} (bound {5 * np.sqrt(2 / n):.3e})")
    assert np.isfinite(v).all()
    assert abs(v.mean()) <= 5 / np.sqrt(n)
    assert abs(v.var() - 1) <= 5 * np.sqrt(2 / n)
    # the three coordinates of a joint come from one Philox block: x and y share a radius and must still be uncorrelated
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(_corr(x[..., a], x[..., b])) <= 5 / np.sqrt(n / 3), (a, b)
    pairs = {"adjacent p": (x[:, :-1], x[:, 1:]),
             "adjacent b": (x[:-1], x[1:]),
             "adjacent k": (x, noise.reference_draw(5, 0, 1, 0, 0, B, P, F, J)),
             "adjacent call": (x, noise.reference_draw(5, 1, 0, 0, 0, B, P, F, J)),
             "adjacent seed": (x, noise.reference_draw(6, 0, 0, 0, 0, B, P, F, J))}
    for name, (a, b) in pairs.items():
        r, bound = _corr(a, b), 5 / np.sqrt(a.size)
        print(f"{name}: correlation {r:+.3e} (bound {bound:.3e}, n = {a.size})")
        assert abs(r) <= bound, name


def test_new_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pafuse_hip.h")).read()
    for name in ("pafuse_noise_fill", "pafuse_d3dp_sample_seeded"):
        assert re.search(r"\bint\s+%s\s*\(\s*const" % name, header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "const uint32_t *key4_dev" in header
    assert _lib.ABI_VERSION == 8 and lib.pafuse_abi_version() == 8      # no struct changed


def test_noise_source_attributes():
    from __graft_entry__ import make_model
    model, _ = make_model(2, 2, device="cpu")
    assert model.noise == "torch" and model.noise_fn is None and model.noise_seed == 0 and model.noise_call == 0
    with pytest.raises(ValueError):
        model.noise = "bogus"
    assert model.noise == "torch"
    model.noise_fn = lambda k, shape, device: None
    with pytest.raises(ValueError):
        model.noise = "device"                 # noise_fn is set
    assert model.noise == "torch"
    model.noise_fn = None
    model.noise = "device"
    with pytest.raises(ValueError):
        model.noise_fn = lambda k, shape, device: None
    assert model.noise_fn is None
    for bad in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError):
            model.noise_seed = bad
    model.noise_call = 7
    model.noise_seed = 2 ** 32 - 1
    assert model.noise_seed == 2 ** 32 - 1 and model.noise_call == 0      # a new seed restarts the call count
    model.advance_noise_call()
    assert model.noise_call == 1
    model.noise = "torch"
    model.advance_noise_call()
    assert model.noise_call == 1               # only the 'device' source counts calls


def test_noise_ops_refuse_host_tensors():
    import torch
    from pafuse_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.pafuse.*)
    assert hasattr(torch.ops.pafuse, "noise_fill")
    with pytest.raises(ValueError):
        ops.noise_fill(torch.zeros(4, dtype=torch.int32), 0, 1, 1, 27, 134)
    with pytest.raises(ValueError):
        ops.noise_key(2 ** 32, 0, device="cpu")
    key = ops.noise_key(2 ** 32 - 1, 5, 2, 3, device="cpu")
    assert key.dtype == torch.int32 and key.tolist() == [-1, 5, 2, 3]
    with pytest.raises(NotImplementedError):
        torch.ops.pafuse.noise_fill(key, 0, 1, 1, 27, 134)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.pafuse.noise_fill(torch.empty(4, dtype=torch.int32, device="cuda"), 1, 2, 3, 27, 134)
        assert out.shape == (2, 3, 27, 134, 3) and out.dtype == torch.float32

"""Noise stream v1 - the host statement, in numpy, of the normals the ``"device"`` noise source of
pafuse_amd.D3DP draws inside the loop's kernels (noise_normals in csrc/kernels.hpp).

For draw k (0 = the initial img, k >= 1 = the update after step k-1), global clip index b, global hypothesis index p,
frame f and joint j:

  (r0, r1, r2, r3) = Philox4x32-10(counter = (f*J + j, p, b, k), key = (seed, call))
  u(r) = (r + 0.5) * 2^-32                        exact in fp64, never 0 or 1
  x = sqrt(-2 ln u(r0)) * cos(2 pi u(r1))
  y = sqrt(-2 ln u(r0)) * sin(2 pi u(r1))
  z = sqrt(-2 ln u(r2)) * cos(2 pi u(r3))         (the fourth normal is dropped)

evaluated in fp64 and rounded once to fp32.  A value is a pure function of (seed, call, k, b, p, f, j): the sharding, the
hypothesis chunk, the clip chunk and the launch schedule cannot change it.

This module is test infrastructure and the documentation of the stream.  The product path never calls it.
"""
import numpy as np

__all__ = ["philox4x32_10", "uniform", "sincos_turns", "reference_draw", "STREAM_VERSION"]

STREAM_VERSION = 1
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # Weyl increments of the key


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; the Random123 known-answer vectors are in tests/test_noise_host.py).
    counter: four uint32 values or arrays that broadcast against each other, key: two of them -> four uint32 arrays."""
    c = [np.asarray(v).astype(np.uint64) for v in counter]
    k0, k1 = (np.asarray(v).astype(np.uint64) for v in key)
    shape = np.broadcast(*c, k0, k1).shape
    c = [np.broadcast_to(v, shape) for v in c]
    mask = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]           # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0 = (k0 + np.uint64(PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(PHILOX_W1)) & mask
    return tuple(v.astype(np.uint32) for v in c)


def uniform(r):
    """u = (r + 0.5) * 2^-32 in fp64: exact (33 significant bits), inside (0, 1)."""
    return (np.asarray(r).astype(np.float64) + 0.5) * 2.0 ** -32


def sincos_turns(r):
    """(sin, cos) of 2 pi u(r).  The angle is folded EXACTLY to d in [-1/8, 1/8] of a turn around the nearest quarter turn
    (integer arithmetic on 2 r + 1, the numerator of u over 2^33) before sin / cos see it, so both results carry a few
    fp64 ulp of RELATIVE error also next to their zeros - which the fp32 rounding of a normal near 0 needs."""
    r = np.asarray(r).astype(np.int64)
    n = 2 * r + 1                                   # u = n / 2^33, odd: d is never 0
    q = ((r >> 29) + 1) >> 1                        # nearest quarter turn, 0 .. 4
    d = (n - (q << 31)).astype(np.float64) * 2.0 ** -33
    s, c = np.sin(2.0 * np.pi * d), np.cos(2.0 * np.pi * d)
    q = q & 3
    sin = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    cos = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    return sin, cos


def reference_draw(seed, call, k, b0, p0, B, P, F, J):
    """Draw k of the stream for clips [b0, b0 + B) and hypotheses [p0, p0 + P) -> float32 [B, P, F, J, 3]."""
    for name, v in (("seed", seed), ("call", call), ("k", k), ("b0 + B", b0 + B), ("p0 + P", p0 + P), ("F * J", F * J)):
        if not 0 <= int(v) < 2 ** 32:
            raise ValueError(f"noise stream v1: {name} = {v} is not a uint32")
    fj = np.arange(F * J, dtype=np.uint32).reshape(1, 1, F * J)
    p = (p0 + np.arange(P, dtype=np.uint32)).reshape(1, P, 1)
    b = (b0 + np.arange(B, dtype=np.uint32)).reshape(B, 1, 1)
    r0, r1, r2, r3 = philox4x32_10((fj, p, b, np.uint32(k)), (np.uint32(seed), np.uint32(call)))
    rad_xy = np.sqrt(-2.0 * np.log(uniform(r0)))
    rad_z = np.sqrt(-2.0 * np.log(uniform(r2)))
    s1, c1 = sincos_turns(r1)
    _, c3 = sincos_turns(r3)
    out = np.stack([rad_xy * c1, rad_xy * s1, rad_z * c3], axis=-1).astype(np.float32)
    return out.reshape(B, P, F, J, 3)

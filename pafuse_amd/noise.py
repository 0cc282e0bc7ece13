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

The training draws (``train_draws = "device"`` of pafuse_amd.D3DP, qsample_seeded_kernel and
droppath_fill_kernel in csrc/train_kernels.hpp) extend the stream without changing it.  The key is (seed, call) with call = the
model's training forward passes (D3DP.train_call, a counter of its own); g is the GLOBAL index of a clip - its position in the
global batch, not in a rank's slice.  Counter word 3 takes three values reserved at the top of its range; the sampling loop's
word 3 is its draw number k, which pafuse_d3dp_sample_seeded counts in an int32 from 0 to at most its number of steps
(<= 2^31 - 1, and <= num_timesteps from pafuse_amd.D3DP), so the two families never share a counter:

  noise of (f, j)    counter (f*J + j, 0, g, K_NOISE = 0xFFFFFFFF)     the three normals above: reference_draw with k = K_NOISE,
                                                                       b = g, p = 0
  timestep of g      counter (0, 0, g, K_TIMESTEP = 0xFFFFFFFE)        t = (uint64(r0) * num_timesteps) >> 32: integer arithmetic,
                                                                       0 <= t < num_timesteps, each value's probability within
                                                                       2^-32 of 1 / num_timesteps
  DropPath           counter (s, (d << 16) | (k << 1) | br, g, K_DROPPATH = 0xFFFFFFFD)
                                                                       keep iff u(r0) < keep_k in fp64; the factor is factor_k
                                                                       if kept, else 0
for block k in [0, 2 depth) in execution order (STE0, TTE0, STE1, ...), branch br (0 attention, 1 MLP), denoiser d (its index
in D3DP.denoisers(); d < 2^16, depth <= 2^14) and sequence s of the block's batch axis: the frame f for even k (spatial, rows
(b f)), the joint j for odd k (temporal, rows (b n)).  keep_k = 1.0 - rate as a double with rate =
torch.linspace(0, drop_path_rate, depth)[k // 2].item(), factor_k = the fp32 value torch.ones(()).div_(keep_k) gives: both are
made on the host and handed to the kernel, which compares and selects.

This module is test infrastructure and the documentation of the stream.  The product path never calls it.
"""
import numpy as np

__all__ = ["philox4x32_10", "uniform", "sincos_turns", "reference_draw", "reference_train_draws", "reference_droppath",
           "K_NOISE", "K_TIMESTEP", "K_DROPPATH", "STREAM_VERSION"]

STREAM_VERSION = 1
K_NOISE, K_TIMESTEP, K_DROPPATH = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD     # reserved values of counter word 3 (training draws)
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
    out = _normals(philox4x32_10((fj, p, b, np.uint32(k)), (np.uint32(seed), np.uint32(call))))
    return out.reshape(B, P, F, J, 3)


def _normals(words):
    """the three normals of four Philox words (arrays of one shape) -> float32 [..., 3]"""
    r0, r1, r2, r3 = words
    rad_xy = np.sqrt(-2.0 * np.log(uniform(r0)))
    rad_z = np.sqrt(-2.0 * np.log(uniform(r2)))
    s1, c1 = sincos_turns(r1)
    _, c3 = sincos_turns(r3)
    return np.stack([rad_xy * c1, rad_xy * s1, rad_z * c3], axis=-1).astype(np.float32)


def _clip_indices(seed, call, clips, **more):
    clips = [int(g) for g in clips]
    for name, v in [("seed", seed), ("call", call)] + [("clip", g) for g in clips] + list(more.items()):
        if not 0 <= int(v) < 2 ** 32:
            raise ValueError(f"noise stream v1: {name} = {v} is not a uint32")
    return np.array(clips, dtype=np.uint32)


def reference_train_draws(seed, call, clips, F, J, num_timesteps):
    """The (t, noise) draws of one training forward for the clips with the global indices `clips` (an explicit list: a
    rank's clips are strided) -> (t int64 [n], noise float32 [n, F, J, 3]).  1 <= num_timesteps <= 2^32."""
    g = _clip_indices(seed, call, clips, **{"F * J": F * J, "num_timesteps - 1": num_timesteps - 1})
    key = (np.uint32(seed), np.uint32(call))
    r0 = philox4x32_10((np.uint32(0), np.uint32(0), g, np.uint32(K_TIMESTEP)), key)[0]
    t = ((r0.astype(np.uint64) * np.uint64(num_timesteps)) >> np.uint64(32)).astype(np.int64)     # < 2^64: no overflow
    fj = np.arange(F * J, dtype=np.uint32).reshape(1, F * J)
    noise = _normals(philox4x32_10((fj, np.uint32(0), g.reshape(-1, 1), np.uint32(K_NOISE)), key))
    return t, noise.reshape(len(g), F, J, 3)


def reference_droppath(seed, call, clips, d, F, J, keep, factor):
    """The DropPath table of denoiser d for one training forward on the clips `clips` -> float32 [2 depth, 2, n max(F, J)]:
    row (k, br), column i * L_k + s = sequence s of the i-th clip (L_k = F for even k, J for odd k); the columns beyond
    n * L_k hold 1.  keep: 2 depth doubles, factor: 2 depth float32 values (see the module text)."""
    g = _clip_indices(seed, call, clips, **{"F * J": F * J})
    keep, factor = np.asarray(keep, dtype=np.float64), np.asarray(factor, dtype=np.float32)
    rows = len(keep)
    if rows % 2 or rows != len(factor) or not 0 <= int(d) < 2 ** 16 or rows > 2 ** 15:
        raise ValueError("noise stream v1: keep / factor hold 2 * depth <= 2^15 values each, d < 2^16")
    n = len(g)
    out = np.ones((rows, 2, n * max(F, J)), dtype=np.float32)
    for k in range(rows):
        L = J if k % 2 else F
        s = np.arange(L, dtype=np.uint32).reshape(1, L)
        for br in range(2):
            word1 = np.uint32((int(d) << 16) | (k << 1) | br)
            r0 = philox4x32_10((s, word1, g.reshape(-1, 1), np.uint32(K_DROPPATH)), (np.uint32(seed), np.uint32(call)))[0]
            out[k, br, :n * L] = np.where(uniform(r0) < keep[k], factor[k], np.float32(0)).reshape(-1)
    return out

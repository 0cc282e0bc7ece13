"""pafuse_amd.posepath, the numpy statement of J-Agg coherent in time (pose_path_kernel), on the CPU.

The brute-force cases are built so that every cost is exact in fp64: the offsets are integer multiples of 3-4-5 triangles
(every distance an integer), e2 values are multiples of 1/8 and the weight is a multiple of 1/4 - sums of a few such
numbers have no rounding, so the recursion's minimum, its normalised total and the plainly added cost of the returned
path must be EQUAL to the minimum over all P**F paths, not close to it.
"""
import numpy as np
import pytest

from pafuse_amd import posepath

INF, NAN = np.float32(np.inf), np.float32(np.nan)
LEGS = np.array([[3, 4, 0], [0, 3, 4], [4, 0, 3], [-3, 0, 4], [0, -4, 3], [5, 12, 0], [0, 5, -12], [8, 0, 15], [0, 0, 0]], dtype=np.float64)


def exact_case(P, F, seed):
    """offsets along one ray of a 3-4-5 (5-12-13, 8-15-17) direction per line: all differences are integer multiples of one
    leg, so every distance is an integer; e2 in multiples of 1/8"""
    g = np.random.default_rng(seed)
    leg = LEGS[g.integers(0, len(LEGS) - 1)]
    off = (g.integers(-3, 4, size=(P, F, 1)) * leg).astype(np.float32)
    e2 = (g.integers(0, 64, size=(P, F)) / 8).astype(np.float32)
    return e2, off


@pytest.mark.parametrize("P,F", [(3, 4), (4, 5)])
def test_statement_is_the_brute_force_minimum(P, F):
    moved = 0
    for seed in range(6):
        e2, off = exact_case(P, F, 100 * P + seed)
        for lam in (0.0, 0.25, 1.0, 16.0):
            idx, total = posepath.path(e2, off, lam)
            best, _ = posepath.brute_force(e2, off, lam)
            assert idx.shape == (F,) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < P
            assert posepath.path_cost(e2, off, lam, idx) == best, (seed, lam)
            assert total == best, (seed, lam)
            moved += int((idx != np.argmin(e2, axis=0)).any())
    assert moved > 0          # the penalty changed a path somewhere: the comparison is not the lam = 0 case in disguise


def test_zero_weight_is_the_first_minimum_per_frame():
    g = np.random.default_rng(3)
    P, F = 7, 11
    off = g.standard_normal((5, P, F, 3)).astype(np.float32)
    e2 = g.random((5, P, F)).astype(np.float32)
    e2[1] = (10.0 ** g.uniform(-30, 0, size=(P, F))).astype(np.float32)      # 1e-30 .. 1: the normalisation keeps them apart
    e2[2, 3] = e2[2, 1]                                                      # ties go to the lower hypothesis
    e2[3] *= np.float32(1e30)
    idx, total = posepath.path(e2, off, 0.0)
    assert np.array_equal(idx, np.argmin(e2, axis=1).astype(np.int32))
    assert not (idx[2] == 3).any()
    assert np.isfinite(total).all()


def test_constant_offsets_and_a_large_weight_give_one_hypothesis():
    g = np.random.default_rng(4)
    P, F = 5, 9
    off = np.repeat(g.integers(-4, 5, size=(P, 1, 3)).astype(np.float32), F, axis=1)
    off[3] = off[1] + np.float32(0.5)
    e2 = (g.integers(0, 32, size=(P, F)) / 8).astype(np.float32)
    e2[3] = e2[1]                                                            # an equal sum: the first minimum of sum_f e2 wins
    idx, total = posepath.path(e2, off, 1e6)
    want = int(np.argmin(e2.astype(np.float64).sum(axis=1)))
    assert (idx == want).all() and total == e2[want].astype(np.float64).sum()
    e2[1] = e2[3] = 0
    idx, _ = posepath.path(e2, off, 1e6)
    assert (idx == 1).all()


def test_an_unobserved_frame_inherits_its_neighbours():
    P, F = 3, 5
    off = np.zeros((P, F, 3), dtype=np.float32)
    off[:, :, 0] = np.arange(P)[:, None]                                     # hypotheses 1 m apart, still
    e2 = np.ones((P, F), dtype=np.float32)
    e2[2] = 0                                                                # hypothesis 2 fits every observed frame
    e2[:, 2] = [0, INF, NAN]                                                 # frame 2 ...
    gone = e2.copy()
    gone[:, 2] = INF                                                         # ... unobserved: nothing pulls to hypothesis 0
    idx, total = posepath.path(gone, off, 0.125)
    assert (idx == 2).all() and total == 0
    idx, _ = posepath.path(e2, off, 0.125)                                   # observed: 2 is +inf there, 0 costs two jumps of 0.25
    assert list(idx) == [2, 2, 0, 2, 2]
    idx, _ = posepath.path(gone, off, 0.0)                                   # no penalty: the gap takes the first available
    assert list(idx) == [2, 2, 0, 2, 2]


def test_lines_without_a_path():
    g = np.random.default_rng(6)
    P, F = 4, 6
    off = g.standard_normal((3, P, F, 3)).astype(np.float32)
    e2 = g.random((3, P, F)).astype(np.float32)
    off[0, :, 4, 1] = NAN                                                    # a frame with no available hypothesis
    e2[1] = INF                                                              # a line with no observed frame
    idx, total = posepath.path(e2, off, 0.5)
    assert (idx[:2] == -1).all() and np.isnan(total[:2]).all()
    assert (idx[2] >= 0).all() and np.isfinite(total[2])
    alone, t = posepath.path(e2[2], off[2], 0.5)                             # lines do not see each other
    assert np.array_equal(alone, idx[2]) and t == total[2]


def test_a_nan_removes_only_its_hypothesis_and_frame():
    g = np.random.default_rng(7)
    P, F = 4, 6
    off = g.standard_normal((P, F, 3)).astype(np.float32)
    e2 = g.random((P, F)).astype(np.float32)
    e2[2], off[2] = 0, 0                                                     # hypothesis 2, at rest, wins everywhere ...
    clean, _ = posepath.path(e2, off, 0.01)
    assert (clean == 2).all()
    for plant in ("off", "e2"):
        o, e = off.copy(), e2.copy()
        if plant == "off":
            o[2, 3, 0] = NAN
        else:
            e[2, 3] = NAN
        idx, total = posepath.path(e, o, 0.01)
        assert idx[3] != 2 and idx[3] >= 0 and (np.delete(idx, 3) == 2).all() and np.isfinite(total), plant   # ... but there


def test_total_does_not_decrease_with_the_weight():
    g = np.random.default_rng(8)
    off = g.standard_normal((20, 6, 12, 3)).astype(np.float32) * 0.05
    e2 = g.random((20, 6, 12)).astype(np.float32) * 0.02
    last = None
    for lam in (0.0, 0.01, 0.1, 0.5, 2.0, 50.0):
        _, total = posepath.path(e2, off, lam)
        # the minimum over paths of (A + lam * B) with B >= 0 is non-decreasing in lam; the recursion's own rounding is
        # a few ulp of the total
        assert last is None or (total >= last - 1e-12 * np.abs(last)).all(), lam
        last = total


def test_helpers_build_the_operands():
    from pafuse_amd import rootfit
    g = np.random.default_rng(9)
    B, T, P, F, J = 2, 2, 3, 4, 5
    conn = np.array([0, 0, 1, 1, 2])
    wb = rootfit.whole_body(g.standard_normal((B, T, P, F, J, 3)).astype(np.float32) * 0.25, conn)
    x2d = (g.random((B, F, J, 2)) * 2 - 1).astype(np.float32)
    traj = np.tile(np.array([0, 0, 4], dtype=np.float32), (B, F, 1))
    cam = np.array([1.1, 1.1, 0.0, 0.0, 0, 0, 0, 0, 0], dtype=np.float32)
    conf = np.ones((B, F, J), dtype=np.float32)
    conf[1, 2, 3], conf[0, 0, 1] = 0, NAN
    e2 = posepath.unary(wb, traj, x2d, cam, conf)
    per_h = np.broadcast_to(traj[:, None, None], (B, T, P, F, 3))
    assert np.array_equal(e2, posepath.unary(wb, per_h, x2d, cam, conf))
    plain = rootfit.reproj_error(wb, per_h, x2d, cam)
    seen = conf > 0
    seen5 = np.broadcast_to(seen[:, None, None], e2.shape)
    assert np.array_equal(e2[seen5], plain[seen5]) and np.isinf(e2[~seen5]).all() and int((~seen5).sum()) == 2 * T * P
    mean = wb.astype(np.float64).mean(axis=2).astype(np.float32)
    off = posepath.offsets(wb, mean)
    assert off.dtype == np.float64 and np.array_equal(off, wb.astype(np.float64) - mean.astype(np.float64)[:, :, None])
    assert np.array_equal(posepath.offsets(wb), wb.astype(np.float64))
    out = posepath.pick(wb, e2, 0.5, mean)
    idx = out["idx"]
    assert idx.shape == (B, T, F, J) and out["cost"].shape == (B, T, J) and out["pick"].shape == (B, T, F, J, 3)
    for b, t, j in ((0, 0, 1), (1, 1, 3), (1, 0, 4)):                        # line by line
        i, c = posepath.path(e2[b, t, :, :, j], off[b, t, :, :, j], 0.5)
        assert np.array_equal(i, idx[b, t, :, j]) and c == out["cost"][b, t, j]
        for f in range(F):
            assert np.array_equal(out["pick"][b, t, f, j], wb[b, t, i[f], f, j])
            assert out["e2"][b, t, f, j] == (e2[b, t, i[f], f, j] if seen[b, f, j] else INF)

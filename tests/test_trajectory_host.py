"""Host side of the camera-space root trajectory (no GPU): the numpy statement pafuse_amd/trajectory.py - the per-frame fit
on the finished pose and the local-linear smoother - and the refusals of pafuse_frames_root_fit / pafuse_trajectory_smooth,
which happen before the first HIP call.

The recovery bound is the one tests/test_rootfit_host.py sets for exact pinhole data: the fit is exact up to the rounding of the
detections to fp32 (relative 6e-8 of a coordinate of size <= 1 seen through a depth of 4.5 m), bound 1e-6 m.  The residual of
such data is of the same size (metres), so the same bound holds for it.

The smoother's exact cases use r = 3: (r+1)^2 = 16, so the taper g = (1 - d*d/16)^2 is dyadic, and with integer-valued roots and
unit weights every product and sum below 2^53 is exact in fp64 - the local line through points on a line is that line, bit
for bit, and so is the final divide (the quotient is an integer).
"""
import ctypes as C

import numpy as np
import pytest
import torch

E_ARG = -1
CAM = np.array([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001], dtype=np.float32)
T, N, J = 2, 6, 134


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def planted(J=J, seed=0, cam=CAM):
    """poses [T,N,J,3] with |X/Z| < 1, a root walking across the room near 4.5 m, and the exact pinhole detections of
    step 0's absolute points rounded to fp32 (step 1 holds the same pose: x2d is shared by the steps)"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((1, N, J, 3)) * 0.3).astype(np.float32)
    w[:, :, 0] = 0
    w = np.repeat(w, T, axis=0)
    root = np.stack([np.linspace(-0.8, 0.9, N), np.linspace(0.1, -0.2, N), 4.5 + 0.1 * np.sin(np.arange(N))], axis=-1)   # [N,3]
    X = w[0].astype(np.float64) + root[:, None]
    assert (X[..., 2] > 0).all() and (np.abs(X[..., :2] / X[..., 2:]) < 1).all()
    fx, fy, cx, cy = (np.float64(v) for v in cam[:4])
    uv = np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], axis=-1).astype(np.float32)
    return w, uv, root


def test_fit_frames_is_fit_roots_on_a_finite_pose():
    from pafuse_amd import rootfit, trajectory
    w, uv, _ = planted(seed=1)
    c = np.random.default_rng(2).uniform(0.1, 1.0, (N, J)).astype(np.float32)
    c[:, 5:20] = 0
    traj, wsum, resid = trajectory.fit_frames(w, uv, c, CAM)
    want = rootfit.fit_roots(w[:, None, None], np.broadcast_to(uv, (T, N, J, 2)), np.broadcast_to(c, (T, N, J)), CAM)[:, 0, 0]
    assert traj.dtype == np.float32 and traj.shape == (T, N, 3) and wsum.shape == resid.shape == (T, N)
    assert np.array_equal(traj, want) and not np.isnan(traj).any()
    assert np.array_equal(wsum, np.broadcast_to(rootfit.lane_sum(c.astype(np.float64)).astype(np.float32), (T, N)))


@pytest.mark.parametrize("J_", [134, 5])
def test_planted_trajectory_is_recovered(J_):
    from pafuse_amd import trajectory
    w, uv, root = planted(J_, seed=3 + J_)
    t, fit = trajectory.fit_frames_f64(w, uv, None, CAM)
    err = np.abs(t - root[None]).max()
    print(f"J = {J_}: |t - t_true| = {err:.3g} m over {T * N} (t, frame)")
    assert fit.all() and err <= 1e-6
    traj, _, _ = trajectory.fit_frames(w, uv, None, CAM)
    assert np.array_equal(traj, t.astype(np.float32))                   # the two spellings agree


def test_zero_weight_joints_take_no_part_whatever_they_hold():
    from pafuse_amd import trajectory
    w, uv, root = planted(seed=5)
    full, _ = trajectory.fit_frames_f64(w, uv, None, CAM)
    lost = np.random.default_rng(6).permutation(J)[:40]
    c = np.ones((N, J), dtype=np.float32)
    c[:, lost] = 0
    uv0 = uv.copy()
    uv0[:, lost] = 0                                                    # what OpenPifPaf writes for a keypoint it did not find
    t, fit = trajectory.fit_frames_f64(w, uv0, c, CAM)
    err, err_full = np.abs(t - root[None]).max(), np.abs(full - root[None]).max()
    print(f"40 of 134 weights 0: |t - t_true| = {err:.3g} m (all weights: {err_full:.3g} m)")
    assert fit.all() and err <= 1e-6 and err_full <= 1e-6


def test_nan_pose_joint_is_a_zero_weight_joint():
    from pafuse_amd import trajectory
    w, uv, _ = planted(seed=7)
    c = np.random.default_rng(8).uniform(0.1, 1.0, (N, J)).astype(np.float32)
    w_nan = w.copy()
    w_nan[0, 2, 17, 1] = np.nan                                         # one component is enough
    w_nan[1, 4, 99] = np.inf
    got = trajectory.fit_frames(w_nan, uv, c, CAM)
    for (t, n, j) in ((0, 2, 17), (1, 4, 99)):                          # per (t, n): the weight is zeroed in that step's frame only
        c0 = c.copy()
        c0[n, j] = 0
        want = trajectory.fit_frames(w, uv, c0, CAM)
        for g, x in zip(got, want):
            assert np.array_equal(g[t, n], x[t, n])
    clean = trajectory.fit_frames(w, uv, c, CAM)
    untouched = np.ones((T, N), dtype=bool)
    untouched[0, 2] = untouched[1, 4] = False
    for g, x in zip(got, clean):
        assert np.array_equal(g[untouched], x[untouched])


def test_all_nan_frame_has_no_fit():
    from pafuse_amd import trajectory
    w, uv, _ = planted(seed=9)
    w[1, 3] = np.nan
    one = w.copy()
    one[0, 0, 1:] = np.nan                                              # a single joint left: no fit either
    for pose, where in ((w, (1, 3)), (one, (0, 0))):
        traj, wsum, resid = trajectory.fit_frames(pose, uv, None, CAM)
        assert np.isnan(traj[where]).all() and wsum[where] == 0 and np.isnan(resid[where])
        rest = np.ones((T, N), dtype=bool)
        rest[where] = False
        rest[1, 3] = False
        assert np.isfinite(traj[rest]).all() and (wsum[rest] > 0).all() and np.isfinite(resid[rest]).all()


def test_resid_is_small_on_exact_data_and_grows_with_a_wrong_focal_length():
    from pafuse_amd import trajectory
    w, uv, _ = planted(seed=10)
    _, _, resid = trajectory.fit_frames(w, uv, None, CAM)
    wrong = CAM.copy()
    wrong[0] = CAM[0] / 2
    _, _, resid_wrong = trajectory.fit_frames(w, uv, None, wrong)
    print(f"resid: exact data {resid.max():.3g} m, fx halved {resid_wrong.min():.3g} .. {resid_wrong.max():.3g} m")
    assert (resid < 1e-6).all()
    assert (resid_wrong > resid).all()


# ------------------------------------------------------------------------------------------------------- the smoother
def line(n_frames, T_=2):
    n = np.arange(n_frames, dtype=np.float32)
    y = np.stack([3 * n - 7, -2 * n + 40, n + 4000], axis=-1)          # integer-valued, linear in n
    return np.stack([y, y + 5][:T_]).astype(np.float32)


def test_smooth_returns_a_line_exactly_ends_included():
    from pafuse_amd import trajectory
    y = line(12)
    assert np.array_equal(trajectory.smooth(y, None, 3), y)
    assert np.array_equal(trajectory.smooth(y, np.ones(y.shape[:2], dtype=np.float32), 3), y)


def test_smooth_fills_an_unfitted_frame_from_the_line():
    from pafuse_amd import trajectory
    y = line(12)
    w = np.ones(y.shape[:2], dtype=np.float32)
    hole = y.copy()
    w[0, 5] = 0
    hole[0, 5] = 123.0                                                  # weight 0: whatever it holds
    hole[1, 7] = np.nan                                                 # no fit, weight still 1
    hole[1, 0, 2] = np.nan                                              # an end frame, one component
    assert np.array_equal(trajectory.smooth(hole, w, 3), y)


def test_smooth_isolated_frame_and_long_gap():
    from pafuse_amd import trajectory
    r, n_frames = 2, 16
    y = np.full((1, n_frames, 3), np.nan, dtype=np.float32)
    w = np.ones((1, n_frames), dtype=np.float32)
    y[0, 1] = (1.5, -2.25, 4.0)                                         # isolated: no partner within r
    y[0, 12:] = line(4, 1)[0]
    w[0, 1] = 0.3
    out = trajectory.smooth(y, w, r)
    om0 = np.float64(np.float32(0.3))                                   # Q0/S0 at d = 0 (g = 1) ...
    assert np.array_equal(out[0, 1], ((om0 * y[0, 1].astype(np.float64)) / om0).astype(np.float32))
    h1, h2 = 1.0 - 1.0 / 9.0, 1.0 - 4.0 / 9.0                           # ... and at d = -1, +1, +2 of it
    for n, g in ((0, h1 * h1 * om0), (2, h1 * h1 * om0), (3, h2 * h2 * om0)):
        assert np.array_equal(out[0, n], ((g * y[0, 1].astype(np.float64)) / g).astype(np.float32))
    # frames 2 .. 11 have no fit: 10 > 2r + 1; those further than r from a fitted frame stay NaN
    assert np.isnan(out[0, 4:10]).all() and not np.isnan(out[0, :4]).any() and not np.isnan(out[0, 10:]).any()


def test_smooth_is_local():
    from pafuse_amd import trajectory
    rng = np.random.default_rng(11)
    r, n_frames, n = 3, 20, 9
    y = rng.standard_normal((2, n_frames, 3)).astype(np.float32)
    w = rng.uniform(0.1, 1, (2, n_frames)).astype(np.float32)
    base = trajectory.smooth(y, w, r)
    y2, w2 = y.copy(), w.copy()
    far = np.abs(np.arange(n_frames) - n) > r
    y2[:, far] = rng.standard_normal((2, int(far.sum()), 3)).astype(np.float32) * 100
    y2[0, 0] = np.nan
    w2[:, far] = 7.0
    other = trajectory.smooth(y2, w2, r)
    assert np.array_equal(other[:, n], base[:, n])
    assert not np.array_equal(other[:, n + 1], base[:, n + 1])          # frame n + 1 does see frame n - r ... n + r + 1
    assert not np.array_equal(base, y)                                  # and it is a filter
    with pytest.raises(ValueError):
        trajectory.smooth(y, w, 0)
    with pytest.raises(ValueError):
        trajectory.smooth(y, w, 65)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    assert L.pafuse_abi_version() == 8
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ok = [p, p, p, p, 1, 1, 1, p, p, p, None]      # pose, x2d, conf, cam, T, N, J, traj, wsum, resid, stream
    for i in (0, 1, 3, 7):                         # pose, x2d, cam, traj
        a = list(ok)
        a[i] = None
        assert L.pafuse_frames_root_fit(*a) == E_ARG, i
    for i in (4, 5, 6):
        for v in (0, -1):
            a = list(ok)
            a[i] = v
            assert L.pafuse_frames_root_fit(*a) == E_ARG, (i, v)
    assert b"frames_root_fit" in L.pafuse_last_error()
    q = p + 128
    ok = [p, p, 1, 1, 3, q, None]                  # traj, weight, T, N, radius, out, stream
    for i, v in ((0, None), (5, None), (2, 0), (3, 0), (2, -1), (3, -1), (4, 0), (4, 65), (4, -1), (5, p)):
        a = list(ok)
        a[i] = v
        assert L.pafuse_trajectory_smooth(*a) == E_ARG, (i, v)
    assert b"trajectory_smooth" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import harness, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.fit_trajectory(z(1, 2, 3, 3), z(2, 3, 2), z(9))
    with pytest.raises(ValueError, match="must match"):
        ops.fit_trajectory(z(1, 2, 3, 3), z(2, 4, 2), z(9))
    with pytest.raises(ValueError, match="must match"):
        ops.fit_trajectory(z(1, 2, 3, 3), z(2, 3, 2), z(9), conf=z(2, 4))
    with pytest.raises(ValueError, match="want"):
        ops.fit_trajectory(z(1, 2, 3, 3), z(2, 3, 2), z(9), want=("traj", "mean"))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.smooth_trajectory(z(1, 2, 3), None, 3)
    for r in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="radius"):
            ops.smooth_trajectory(z(1, 2, 3), None, r)
    with pytest.raises(ValueError, match="weight"):
        ops.smooth_trajectory(z(1, 2, 3), z(1, 3), 3)
    t = z(1, 2, 3)
    with pytest.raises(ValueError, match="alias"):
        ops.smooth_trajectory(t, None, 3, out=t)
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    seq = z(60, 134, 2)
    with pytest.raises(ValueError, match="harness.fit_trajectory"):
        harness.infer_sequence(model, None, seq, [], [], aggregate="mean", cam=z(9), trajectory=True)
    with pytest.raises(ValueError, match="cam"):
        harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, trajectory=3)
    for bad in (0, 65, 2.5, False):
        with pytest.raises(ValueError, match="trajectory"):
            harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, cam=z(9), trajectory=bad)
    with pytest.raises(ValueError, match="conf"):
        harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, cam=z(9), trajectory=3, conf=z(60, 133))
    with pytest.raises(ValueError, match="conf belongs"):           # unchanged without a trajectory
        harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, conf=z(60, 134))
    with pytest.raises(ValueError, match="poses must be"):
        harness.fit_trajectory(z(2, 60, 134, 3), z(61, 134, 2), z(9))
    with pytest.raises(ValueError, match="radius"):
        harness.fit_trajectory(z(2, 60, 134, 3), seq, z(9), smooth=0)


def test_torch_ops_have_schemas_and_fakes():
    import pafuse_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "Tensor? conf=None" in str(torch.ops.pafuse.fit_trajectory.default._schema)
    s = str(torch.ops.pafuse.smooth_trajectory.default._schema)
    assert "Tensor? weight" in s and "radius" in s and s.endswith("-> Tensor")
    with FakeTensorMode():
        pose = torch.empty(2, 5, 7, 3, device="cuda")
        traj, wsum, resid = torch.ops.pafuse.fit_trajectory(pose, torch.empty(5, 7, 2, device="cuda"), torch.empty(9, device="cuda"))
        assert traj.shape == (2, 5, 3) and wsum.shape == resid.shape == (2, 5) and traj.device.type == "cuda"
        out = torch.ops.pafuse.smooth_trajectory(traj, wsum, 3)
        assert out.shape == (2, 5, 3) and out.dtype == torch.float32

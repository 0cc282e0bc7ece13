"""Host side of the focal-length estimate (no GPU): the numpy statement pafuse_amd/focal.py - thirteen weighted sums per
(t, frame), three projected inner products, one division per video - and the refusals of pafuse_frames_focal_sums /
pafuse_focal_solve, which happen before the first HIP call.

What is asserted and why it can be asserted:
  * the closed form IS ordinary weighted least squares: with p = u - cx, q = (v - cy)/rho the pinhole is linear in
    (1/f; tx_n, ty_n, tz_n/f), and sum K / sum H is the 1/phi of np.linalg.lstsq on the stacked system - both are fp64 solutions of
    one well-conditioned problem -> rtol 1e-9.
  * planted recovery: exact pinhole data rounded to fp32 (relative 6e-8 per detection) -> relative error <= 1e-5 and r2 within
    1e-6 of 1; the margin covers the rounding of the inputs, which is what limits it (worst case seen: J = 5, N = 1).
  * the direction of the regression: with 2 cm of pose noise K/H stays within 5 % of the planted value while H/G, the form one
    writes first, falls below 0.7 of it - the noise of the pose sits in G.
"""
import ctypes as C

import numpy as np
import pytest
import torch

E_ARG = -1
F_TRUE, RHO = 2.30, 0.9987
CAM_TRUE = np.array([F_TRUE, RHO * F_TRUE, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001], dtype=np.float32)
RECOVERY_CASES = [(J, N) for J in (5, 64, 65, 134, 300) for N in (1, 2, 7, 70)]


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def guess(cam=CAM_TRUE, factor=0.5):
    """the caller's camera: the true principal point and aspect, the focal length a guess (a power of two keeps the ratio's bits)"""
    out = cam.copy()
    out[:2] *= np.float32(factor)
    return out


def planted(J, N, seed, T=1, pose_noise=0.0, det_noise=0.0, depth=4.0, lose=True):
    """a person of about 1.7 m x 0.5 m x 0.3 m at `depth` metres, walking; the exact pinhole detections of the true camera rounded
    to fp32; the pose handed to the estimator is the true one plus `pose_noise` (iid, metres), the detections plus `det_noise`;
    lose: a fifth of the weights 0 with their detections at (0, 0), joints 0 - 3 kept"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, J, 3)) * np.array([0.25, 0.45, 0.15])).astype(np.float32)
    w[:, 0] = 0
    n = np.arange(N)
    root = np.stack([-0.5 + 0.02 * n, 0.1 - 0.001 * n, depth + 0.2 * np.sin(0.3 * n)], axis=-1)
    X = w.astype(np.float64) + root[:, None]
    assert (X[..., 2] > 1).all()
    f, fy, cx, cy = (np.float64(v) for v in CAM_TRUE[:4])
    uv = np.stack([f * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], axis=-1)
    uv = (uv + det_noise * rng.standard_normal(uv.shape)).astype(np.float32)
    pose = np.repeat(w[None], T, axis=0)
    pose = (pose + pose_noise * rng.standard_normal(pose.shape)).astype(np.float32)
    pose[:, :, 0] = 0
    c = rng.uniform(0.1, 1.0, (N, J)).astype(np.float32)
    if lose:
        lost = rng.uniform(size=(N, J)) < 0.2
        lost[:, :4] = False
        c[lost] = 0
        uv[lost] = 0
    return pose, uv, c, root


def estimate(pose, uv, c, cam):
    from pafuse_amd import focal
    state = focal.focal_sums(pose, uv, c, cam)
    return state, focal.focal_solve(state, cam)


def test_closed_form_is_least_squares_on_the_stacked_system():
    from pafuse_amd import focal
    J, N = 134, 7
    pose, uv, c, _ = planted(J, N, seed=1, pose_noise=0.02, det_noise=0.004)
    cam = guess()
    tot = focal.totals(focal.focal_sums(pose, uv, c, cam))[0]
    rho = np.float64(cam[1]) / np.float64(cam[0])
    p = uv[..., 0].astype(np.float64) - np.float64(cam[2])
    q = (uv[..., 1].astype(np.float64) - np.float64(cam[3])) / rho
    X, Y, Z = (pose[0, ..., k].astype(np.float64) for k in range(3))
    sw = np.sqrt(c.astype(np.float64))
    A = np.zeros((2 * N * J, 1 + 3 * N))
    b = np.zeros(2 * N * J)
    for n in range(N):                      # X = phi*p*Z - tx + gamma*p ; Y = phi*q*Z - ty + gamma*q
        rx, ry = slice(2 * n * J, (2 * n + 1) * J), slice((2 * n + 1) * J, (2 * n + 2) * J)
        A[rx, 0], A[ry, 0] = sw[n] * p[n] * Z[n], sw[n] * q[n] * Z[n]
        A[rx, 1 + 3 * n], A[ry, 2 + 3 * n] = -sw[n], -sw[n]
        A[rx, 3 + 3 * n], A[ry, 3 + 3 * n] = sw[n] * p[n], sw[n] * q[n]
        b[rx], b[ry] = sw[n] * X[n], sw[n] * Y[n]
    sol = np.linalg.lstsq(A, b, rcond=None)[0]
    f_closed, f_lstsq = tot[0] / tot[1], 1.0 / sol[0]
    print(f"closed form {f_closed!r}, lstsq {f_lstsq!r}: relative difference {abs(f_closed / f_lstsq - 1):.3g}")
    assert tot[3] == N
    assert abs(f_closed / f_lstsq - 1) <= 1e-9


@pytest.mark.parametrize("case", RECOVERY_CASES)
def test_planted_focal_length_is_recovered(case):
    from pafuse_amd import focal
    J, N = case
    pose, uv, c, _ = planted(J, N, seed=10 + 3 * J + N)
    state, (f, r2, frames, cam_out) = estimate(pose, uv, c, guess())
    tot = focal.totals(state)[0]
    f64, r64 = tot[0] / tot[1], (tot[1] * tot[1]) / (tot[2] * tot[0])
    print(f"(J, N) = {case}: f = {f64!r}, relative error {abs(f64 / F_TRUE - 1):.3g}, 1 - r2 = {1 - r64:.3g}")
    assert frames.dtype == np.int32 and frames[0] == N
    assert abs(f64 / np.float64(CAM_TRUE[0]) - 1) <= 1e-5
    assert abs(r64 - 1) <= 1e-6
    assert f.dtype == r2.dtype == cam_out.dtype == np.float32 and cam_out.shape == (1, 9)
    assert f[0] == np.float32(f64) and r2[0] == np.float32(r64)
    rho = np.float64(CAM_TRUE[1]) / np.float64(CAM_TRUE[0])
    assert cam_out[0, 0] == f[0] and cam_out[0, 1] == np.float32(rho * f64) and np.array_equal(cam_out[0, 2:], CAM_TRUE[2:])


def test_only_the_ratio_of_fx_and_fy_is_read():
    pose, uv, c, _ = planted(134, 7, seed=3, T=2, pose_noise=0.02)
    s1, o1 = estimate(pose, uv, c, guess(factor=0.5))
    s2, o2 = estimate(pose, uv, c, guess(factor=1.0))
    assert s1.tobytes() == s2.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(o1, o2))
    short = estimate(pose, uv, c, guess()[:4])[1]
    assert short[3].shape == (2, 4) and np.array_equal(short[3][:, :2], o1[3][:, :2]) and short[0].tobytes() == o1[0].tobytes()


def test_planar_pose_has_no_estimate_but_counts_its_frames():
    N = 7
    pose, uv, c, _ = planted(134, N, seed=4)
    pose[..., 2] = 0
    state, (f, r2, frames, cam_out) = estimate(pose, uv, c, guess())
    assert np.isnan(f).all() and np.isnan(r2).all() and frames[0] == N
    assert np.isnan(cam_out[0, :2]).all() and np.array_equal(cam_out[0, 2:], CAM_TRUE[2:])
    assert np.array_equal(state[..., 3], np.ones((1, N)))


def test_frames_that_take_no_part_and_empty_input():
    from pafuse_amd import focal
    N, J = 7, 134
    pose, uv, c, _ = planted(J, N, seed=5, lose=False)
    c3 = c.copy()
    c3[2, 3:] = 0                                                   # frame 2 keeps three joints: not enough
    pose_nan = pose.copy()
    pose_nan[0, 4] = np.nan                                         # frame 4 has no pose
    pose_nan[0, 5, 7:] = np.nan                                     # frame 5 keeps seven joints
    state = focal.focal_sums(pose_nan, uv, c3, guess())
    assert np.array_equal(state[0, :, 3], [1, 1, 0, 1, 0, 1, 1])
    assert np.array_equal(state[0, 2], np.zeros(4)) and np.array_equal(state[0, 4], np.zeros(4))
    f, r2, frames, _ = focal.focal_solve(state, guess())
    assert frames[0] == 5 and abs(f[0] / F_TRUE - 1) <= 1e-5
    lone = np.zeros_like(c)
    lone[:, :4] = 1
    four = focal.focal_sums(pose, uv, lone, guess())                # four joints are enough
    assert np.array_equal(four[0, :, 3], np.ones(N))
    same_dir = uv.copy()
    same_dir[1] = CAM_TRUE[2:4]                                     # every joint on the optical axis: p = q = 0, den = 0 exactly
    assert focal.focal_sums(pose, same_dir, c, guess())[0, 1, 3] == 0
    empty = focal.focal_sums(np.full_like(pose, np.nan), uv, c, guess())
    assert not empty.any()
    f, r2, frames, cam_out = focal.focal_solve(empty, guess())
    assert np.isnan(f[0]) and np.isnan(r2[0]) and frames[0] == 0 and np.isnan(cam_out[0, :2]).all()
    neg = focal.focal_sums(pose, uv, np.where(np.arange(J) % 2 == 0, c, -c), guess())     # a weight that is not > 0 is no weight
    zero = focal.focal_sums(pose, uv, np.where(np.arange(J) % 2 == 0, c, 0).astype(np.float32), guess())
    assert neg.tobytes() == zero.tobytes()


def test_states_of_two_videos_concatenate():
    from pafuse_amd import focal
    a = planted(134, 70, seed=6, T=2, pose_noise=0.02, det_noise=0.004)
    b = planted(134, 7, seed=7, T=2, pose_noise=0.02, det_noise=0.004, depth=3.0)
    cam = guess()
    sa, sb = focal.focal_sums(a[0], a[1], a[2], cam), focal.focal_sums(b[0], b[1], b[2], cam)
    both = focal.focal_sums(np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]), cam)
    assert both.shape == (2, 77, 4) and np.concatenate([sa, sb], axis=1).tobytes() == both.tobytes()
    f, _, frames, _ = focal.focal_solve(both, cam)
    assert frames.tolist() == [77, 77] and np.isfinite(f).all()


def test_noisy_case_pins_the_direction_of_the_regression():
    from pafuse_amd import focal
    pose, uv, c, _ = planted(134, 70, seed=8, pose_noise=0.02, det_noise=0.004)
    state, (f, r2, frames, _) = estimate(pose, uv, c, guess())
    K, H, G, cnt = focal.totals(state)[0]
    built, rejected = K / H, H / G
    print(f"2 cm / 0.004 noise, J = 134, N = 70: K/H = {built:.4f} ({abs(built / F_TRUE - 1):.2%} off), H/G = {rejected:.4f} "
          f"({rejected / F_TRUE:.3f} of the planted {F_TRUE}), r2 = {float(r2[0]):.3f}")
    assert cnt == 70 and frames[0] == 70
    assert abs(built / F_TRUE - 1) <= 0.05
    assert rejected < 0.7 * F_TRUE
    assert 0 < r2[0] < 1


def test_depth_scale_error_is_inherited_one_for_one():
    """what the estimate is not: a pose whose depth is scaled by 0.8 gives 0.8 f on otherwise exact data"""
    pose, uv, c, _ = planted(134, 7, seed=9)
    pose[..., 2] *= np.float32(0.8)
    f = estimate(pose, uv, c, guess())[1][0]
    assert abs(f[0] / (0.8 * F_TRUE) - 1) <= 1e-4


# ------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    from pafuse_amd import _lib
    assert L.pafuse_abi_version() == 8 and _lib.ABI_VERSION == 8        # new entries only: no struct changed
    assert len(_lib.SIGNATURES["pafuse_frames_focal_sums"][1]) == 9 and len(_lib.SIGNATURES["pafuse_focal_solve"][1]) == 10
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok = [p, p, p, p, 1, 1, 1, p, None]            # pose, x2d, conf, cam, T, N, J, state, stream
    for i in (0, 1, 3, 7):                         # pose, x2d, cam, state
        a = list(ok)
        a[i] = None
        assert L.pafuse_frames_focal_sums(*a) == E_ARG, i
    for i in (4, 5, 6):
        for v in (0, -1):
            a = list(ok)
            a[i] = v
            assert L.pafuse_frames_focal_sums(*a) == E_ARG, (i, v)
    a = list(ok)
    a[7] = p + 4
    assert L.pafuse_frames_focal_sums(*a) == E_ARG
    assert b"frames_focal_sums" in L.pafuse_last_error()
    ok = [p, 1, 1, p, 9, p, p, p, p, None]         # state, T, N, cam, cam_len, focal, r2, frames, cam_out, stream
    for i, v in ((0, None), (3, None), (5, None), (1, 0), (1, -1), (2, 0), (2, -1), (4, 3), (4, 10), (4, 0), (0, p + 4)):
        a = list(ok)
        a[i] = v
        assert L.pafuse_focal_solve(*a) == E_ARG, (i, v)
    assert b"focal_solve" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import harness, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.focal_sums(z(1, 2, 5, 3), z(2, 5, 2), z(9))
    with pytest.raises(ValueError, match="must match"):
        ops.focal_sums(z(1, 2, 5, 3), z(2, 4, 2), z(9))
    with pytest.raises(ValueError, match="must match"):
        ops.focal_sums(z(1, 2, 5, 3), z(2, 5, 2), z(9), conf=z(2, 4))
    with pytest.raises(ValueError, match="x2d and cam"):
        ops.focal_sums(z(1, 2, 5, 3), None, z(9))
    with pytest.raises(ValueError, match="HIP device"):
        ops.focal_solve(z(1, 2, 4, dtype=torch.float64), z(9))
    with pytest.raises(ValueError, match="HIP device"):
        ops.focal_solve(z(1, 2, 4), z(9))
    with pytest.raises(ValueError, match="want"):
        ops.focal_solve(z(1, 2, 4, dtype=torch.float64), z(9), want=("r2",))
    with pytest.raises(ValueError, match="focal must be"):
        harness.fit_trajectory(z(1, 2, 5, 3), z(2, 5, 2), z(9), focal=2.3)
    with pytest.raises(ValueError, match="cam"):
        harness.fit_trajectory(z(1, 2, 5, 3), z(2, 5, 2))
    with pytest.raises(ValueError, match="4 .. 9"):
        harness.estimate_focal(z(1, 2, 5, 3), z(2, 5, 2), cam=z(3))
    with pytest.raises(ValueError, match=r"\[T,N,J,3\]"):
        harness.estimate_focal(z(2, 5, 3), z(2, 5, 2))
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    with pytest.raises(ValueError, match="belongs to a trajectory"):
        harness.infer_sequence(model, None, z(30, 5, 2), [], [], aggregate="mean", stride=9, focal="estimate")
    with pytest.raises(ValueError, match="focal must be"):
        harness.infer_sequence(model, None, z(30, 5, 2), [], [], aggregate="mean", stride=9, trajectory=3, focal="guess")
    with pytest.raises(ValueError, match="belongs to a trajectory"):
        harness.evaluate_frames(model, None, z(30, 5, 2), z(30, 5, 3), z(9), [], [], focal="estimate")


def test_torch_ops_have_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import pafuse_amd.torch_ops  # noqa: F401
    with FakeTensorMode():
        pose, x2d, cam = torch.empty(2, 7, 134, 3, device="cuda"), torch.empty(7, 134, 2, device="cuda"), torch.empty(9, device="cuda")
        state = torch.ops.pafuse.focal_sums(pose, x2d, cam)
        assert state.shape == (2, 7, 4) and state.dtype == torch.float64
        f, r2, frames, cam_out = torch.ops.pafuse.focal_solve(state, cam)
        assert f.shape == r2.shape == frames.shape == (2,) and frames.dtype == torch.int32 and cam_out.shape == (2, 9)

"""Frame-level errors of the per-frame pose against ground truth - the host statement, in numpy, of
what frame_errors_kernel and frame_errors_reduce_kernel (csrc/kernels.hpp; pafuse_frame_errors, pafuse_frame_errors_reduce)
compute.

Inputs: pose [T,N,J,3] fp32, whole-body and root-relative (infer_sequence(stride=)["pose"] or stitch_poses; NaN where no
window covered the frame or a pick has no candidate); gt [N,J,3] fp32 likewise; traj [T,N,3] fp32 or None, the fitted or
smoothed root, and gt_root [N,3] fp32 with it; pbroot / part int [J], the root joint of every joint's part and the part's
number (evaluate._tables, evaluate._part_table); num_parts <= 4.

Everything is fp64 with no fused multiply-add; every fp32 input is converted to double once.

  d[n,j] = pose[t,n,j] - gt[n,j]  per component          r[n] = traj[t,n] - gt_root[n]
  |v| = sqrt((v0*v0 + v1*v1) + v2*v2)

A joint takes part in a frame only if the three components of its pose and of its gt are finite.  K = 6 + num_parts slots
per (t, n), each a sum over the joints that take part and an int32 count of them (SLOTS names them):

  0 mpjpe      |d[n,j]|
  1 mpjve      |d[n,j] - d[n-1,j]|                              n >= 1, the joint in both frames
  2 accel      |(d[n+1,j] - d[n,j]) - (d[n,j] - d[n-1,j])|      1 <= n <= N-2, the joint in all three frames
  3 root       |r[n]|               one term per frame, count 1 if traj[t,n] and gt_root[n] are finite
  4 root_vel   |r[n] - r[n-1]|      one term, n >= 1, both frames
  5 abs_mpjpe  |d[n,j] + r[n]|      the camera-space error
  6+i          |d[n,j] - d[n,pbroot[j]]| over the joints of part i; the part root must take part too (center_pose_parts'
               re-centring - the quantity metrics_kernel calls epb)

Slots 3 .. 5 need traj; a slot that is not defined for a frame, or has no participant, holds sum 0.0 and count 0.  Slots 1
and 2 are the reference's mean_velocity_error (common/loss.py:488-497) and its second-difference analogue.  A metric is
(sum of sums) / (sum of counts), in metres (per frame, per frame squared); millimetres are formed on the host.

Every sum over j is taken in rootfit.SUM_ORDER (lane l of 64 adds its joints l, l + 64, ... in ascending order from 0.0,
then v = v + v[lane ^ o] for o = 32 .. 1; a joint that takes no part feeds 0.0).  reduce() adds the frames of every (t, k)
in the same order: lane l adds frames l, l + 64, ..., then the butterfly.  Counts are integers: their order does not matter.

This is deliberately NOT metrics_kernel's fp32 expression: frame-level numbers have no reference log to diff against, so
one rule (fp64) keeps the statement short.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

from .rootfit import lane_sum

SLOTS = ("mpjpe", "mpjve", "accel", "root", "root_vel", "abs_mpjpe")   # then one slot per part
MAX_PARTS = 4


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def _shift(x, by, axis=1):
    """x[n - by] along the frame axis, zeros (False) where there is no such frame"""
    out = np.zeros_like(x)
    n = x.shape[axis]
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    if by > 0:
        src[axis], dst[axis] = slice(0, max(n - by, 0)), slice(by, n)
    else:
        src[axis], dst[axis] = slice(-by, n), slice(0, max(n + by, 0))
    out[tuple(dst)] = x[tuple(src)]
    return out


def frame_errors(pose, gt, traj, gt_root, pbroot, part, num_parts):
    """-> (err [T,N,K] float64, cnt [T,N,K] int32), K = 6 + num_parts: what pafuse_frame_errors writes."""
    pose = np.asarray(pose, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32)
    T, N, J, _ = pose.shape
    assert pose.shape == (T, N, J, 3) and gt.shape == (N, J, 3)
    assert (traj is None) == (gt_root is None), "traj and gt_root come together"
    num_parts = int(num_parts)
    assert 1 <= num_parts <= MAX_PARTS
    pbroot = np.asarray(pbroot, dtype=np.int64)
    part = np.asarray(part, dtype=np.int64)
    assert pbroot.shape == part.shape == (J,) and (pbroot >= 0).all() and (pbroot < J).all()
    K = 6 + num_parts
    err = np.zeros((T, N, K), dtype=np.float64)
    cnt = np.zeros((T, N, K), dtype=np.int32)
    with np.errstate(all="ignore"):
        on = np.isfinite(pose).all(axis=-1) & np.isfinite(gt).all(axis=-1)[None]          # [T,N,J]
        d = pose.astype(np.float64) - gt.astype(np.float64)[None]                            # [T,N,J,3]
        a, z = _shift(d, 1), _shift(d, -1)                                                   # d[n-1], d[n+1]
        on_a, on_z = _shift(on, 1), _shift(on, -1)

        def put(k, term, take):
            err[..., k] = lane_sum(np.where(take, term, 0.0))
            cnt[..., k] = take.sum(axis=-1)

        put(0, _norm(d), on)
        put(1, _norm(d - a), on & on_a)
        put(2, _norm((z - d) - (d - a)), on & on_a & on_z)
        if traj is not None:
            traj = np.asarray(traj, dtype=np.float32)
            gt_root = np.asarray(gt_root, dtype=np.float32)
            assert traj.shape == (T, N, 3) and gt_root.shape == (N, 3)
            ron = np.isfinite(traj).all(axis=-1) & np.isfinite(gt_root).all(axis=-1)[None]   # [T,N]
            r = traj.astype(np.float64) - gt_root.astype(np.float64)[None]                   # [T,N,3]
            r_a, ron_a = _shift(r, 1), _shift(ron, 1)
            err[..., 3] = np.where(ron, _norm(r), 0.0)
            cnt[..., 3] = ron
            err[..., 4] = np.where(ron & ron_a, _norm(r - r_a), 0.0)
            cnt[..., 4] = ron & ron_a
            put(5, _norm(d + r[:, :, None]), on & ron[:, :, None])
        eb, onb = _norm(d - d[:, :, pbroot]), on & on[:, :, pbroot]
        for i in range(num_parts):
            put(6 + i, eb, onb & (part == i)[None, None])
    return err, cnt


def reduce(err, cnt):
    """err [T,N,K] float64, cnt [T,N,K] int32 -> (sums [T,K] float64, counts [T,K] int64): what pafuse_frame_errors_reduce
    writes - the frames of every (t, k) added in the lane-then-butterfly order."""
    err = np.asarray(err, dtype=np.float64)
    cnt = np.asarray(cnt)
    assert err.ndim == 3 and cnt.shape == err.shape
    return lane_sum(err.transpose(0, 2, 1)), cnt.astype(np.int64).sum(axis=1)

#!/usr/bin/env python3
"""Generate tests/golden/g23_frame_metrics.npz: the frame-level errors of a per-frame pose against ground truth as the REAL
reference's metric functions compute them in fp64 (common/loss.py: mpjpe :9-27, mean_velocity_error :488-497, p_mpjpe
:209-249), on CPU.

Runs only in the build container, next to make_golden.py (same shims, same FakeDataset, same writer; nothing of the
reference is copied).  One case, T = 2 sampling steps, N = 9 frames, J = 134:

  gt      [N,J,3] fp32   a whole-body, root-relative pose per frame (joint 0 at 0) that drifts smoothly along the frames
  pose    [T,N,J,3] fp32 gt + N(0, 3 cm) per coordinate and frame (so that velocity and acceleration errors are not zero),
                         joint 0 at 0

All inputs are fp32-representable; their float64 copies are handed to the reference, so that the reference computes in fp64.
Per step t: mpjpe(pose[t], gt); mpjve = mean_velocity_error(pose[t], gt, axis=0); accel, its second-difference analogue formed
here with np.diff(..., n=2) and the same norm and mean; p_mpjpe(pose[t], gt); mpjpe_pb and mpjpe_pb_<part>, mpjpe of the part
re-centred poses - the project's center_pose_parts, checked here against the reference's bit for bit.

Usage:  python tests/golden/make_golden_frames.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

T, N, J = 2, 9, 134
SEED = 2301


def inputs():
    g = torch.Generator().manual_seed(SEED)
    base = torch.randn(J, 3, generator=g) * 0.3
    drift = torch.randn(J, 3, generator=g) * 0.02
    n = torch.arange(N, dtype=torch.float32)[:, None, None]
    gt = base[None] + drift[None] * n + 0.005 * torch.sin(n * 0.7) * torch.randn(J, 3, generator=g)[None]
    gt[:, 0] = 0
    pose = gt[None] + torch.randn(T, N, J, 3, generator=g) * 0.03
    pose[:, :, 0] = 0
    return pose.float().contiguous(), gt.float().contiguous()


def main():
    mg.install_shims()
    from common.loss import mean_velocity_error, mpjpe, p_mpjpe
    from common.utils import center_pose_parts as ref_center
    from pafuse_amd.harness import center_pose_parts
    ds = mg.FakeDataset()
    pose, gt = inputs()
    pose64, gt64 = pose.double(), gt.double()
    centred, gt_centred = center_pose_parts(pose64, ds), center_pose_parts(gt64, ds)
    assert torch.equal(centred, ref_center(pose64, ds)) and torch.equal(gt_centred, ref_center(gt64, ds))   # reference bits
    out = {k: np.zeros(T) for k in ("mpjpe", "mpjve", "accel", "p_mpjpe", "mpjpe_pb")}
    out.update({"mpjpe_pb_" + part: np.zeros(T) for part in ds.parts_joint_indices})
    for t in range(T):
        p, x = pose64[t].numpy(), gt64.numpy()
        out["mpjpe"][t] = float(mpjpe(pose64[t], gt64))
        out["mpjve"][t] = float(mean_velocity_error(p, x, axis=0))
        out["accel"][t] = float(np.mean(np.linalg.norm(np.diff(p, n=2, axis=0) - np.diff(x, n=2, axis=0), axis=len(x.shape) - 1)))
        out["p_mpjpe"][t] = float(p_mpjpe(p.copy(), x.copy()))
        out["mpjpe_pb"][t] = float(mpjpe(centred[t], gt_centred))
        for part, idx in ds.parts_joint_indices.items():
            out["mpjpe_pb_" + part][t] = float(mpjpe(centred[t][:, idx], gt_centred[:, idx]))
    for k, v in out.items():
        print(k, v.tolist())
    assert all(v.dtype == np.float64 and np.isfinite(v).all() and (v > 0).all() for v in out.values())
    mg.save("g23_frame_metrics.npz", pose=pose, gt=gt, **out)


if __name__ == "__main__":
    main()

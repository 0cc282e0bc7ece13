#!/usr/bin/env python3
"""Generate tests/golden/g21_p2_metrics.npz: Protocol #2 (P-MPJPE after similarity alignment) as the REAL reference
computes it (common/loss.py:251-458 on the whole-body poses of main_h3wb.py:326-395), on CPU.

Runs only in the build container, next to make_golden.py (same shims, same FakeDataset, same writer; nothing of the
reference is copied).  Three cases, stored under the prefixes ``random__``, ``rigid__`` and ``degenerate__``:

  random      G9-style random part-centred inputs, B=2 T=3 P=5 F=27 J=134.  The inputs are not stored: they are
              re-generated from a seed by tests/golden/g21_inputs.py (torch's CPU generator; the project's
              center_pose_parts, checked here to give the reference's bits) and pinned by their SHA-256.
  rigid       B=1 T=2 P=3 F=3: every hypothesis is a similarity transform of its whole-body target (scale 0.7-1.4,
              random rotation) plus N(0, 0.5 mm) per coordinate; hypothesis 1 is mirrored (det R = -1), so the
              reference's reflection fix is taken.  wb_pose_from_parts pins joint 0 of every whole-body pose at the
              origin, so a transform that keeps the pose representable fixes joint 0: it has no translation of its
              own (the alignment still translates, the centroids differ).  The part-based inputs are the exact
              inverse of wb_pose_from_parts.
  degenerate  B=1 T=2 P=3 F=3, hypothesis 1 of step 0 all zeros (|Y0| = 0): the reference's NaNs.  This numpy raises
              LinAlgError for an SVD of a NaN matrix where a LAPACK that reports no error returns NaN factors; the
              generator patches np.linalg.svd to the latter for non-finite matrices only (finite ones go to numpy).

Per case: the inputs (pred_parts, gt_parts, x2d, traj, cam; for the random case cam and sha256 only) and the four per-step vectors p2_j_best, p2_p_best,
p2_p_agg, p2_j_agg [T] in metres (p_mpjpe_diffusion_all_min, p_mpjpe_diffusion, ..._all_min(mean_pos=True),
p_mpjpe_diffusion_reproj), plus the Protocol #1 vectors j_best and p_best for the rigid case.

Usage:  python tests/golden/make_golden_p2.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

CAM = [[2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001]]


def _svd_nan_for_nonfinite(svd):
    def wrapped(a, *args, **kwargs):
        a = np.asarray(a)
        bad = ~np.isfinite(a).all(axis=(-2, -1))
        if not bad.any():
            return svd(a, *args, **kwargs)
        u, s, vt = svd(np.where(bad[..., None, None], 0.0, a).astype(a.dtype), *args, **kwargs)
        u[bad], s[bad], vt[bad] = np.nan, np.nan, np.nan
        return u, s, vt
    return wrapped


def wb_inverse(wb, ds):
    """part-based pose whose wb_pose_from_parts is `wb` (joint 0 of `wb` must be 0): body joints as they are,
    every other joint relative to its part's connection joint"""
    out = wb.clone()
    for part, idx in ds.parts_joint_indices.items():
        if part != "body":
            c = ds.parts_connection_indices[part]
            out[..., idx, :] = wb[..., idx, :] - wb[..., c:c + 1, :]
    return out


def reference_p2(pred_parts, gt_parts, x2d, traj, cam, ds, with_p1=False):
    from common.camera import project_to_2d
    from common.loss import (mpjpe_diffusion, mpjpe_diffusion_all_min, p_mpjpe_diffusion, p_mpjpe_diffusion_all_min,
                             p_mpjpe_diffusion_reproj)
    from common.utils import wb_pose_from_parts
    B, T, P, Fr, J, _ = pred_parts.shape
    pred = wb_pose_from_parts(pred_parts.clone(), ds)
    gt = wb_pose_from_parts(gt_parts.clone(), ds)
    absolute = (pred + traj.unsqueeze(1).unsqueeze(1)).reshape(B * T * P * Fr, J, 3)
    reproj = project_to_2d(absolute, cam.repeat(B * T * P * Fr, 1)).reshape(B, T, P, Fr, J, 2)
    out = {"p2_j_best": p_mpjpe_diffusion_all_min(pred, gt), "p2_p_best": p_mpjpe_diffusion(pred, gt),
           "p2_p_agg": p_mpjpe_diffusion_all_min(pred, gt, mean_pos=True),
           "p2_j_agg": p_mpjpe_diffusion_reproj(pred, gt, reproj, x2d)}
    if with_p1:
        out["j_best"] = mpjpe_diffusion_all_min(pred, gt)
        out["p_best"] = mpjpe_diffusion(pred, gt)[0]
    return {k: torch.as_tensor(np.asarray(v)) for k, v in out.items()}, pred


def random_case(seed, B, T, P, Fr, ds):
    from common.utils import center_pose_parts
    g = torch.Generator().manual_seed(seed)
    pred_parts = center_pose_parts(torch.randn(B, T, P, Fr, 134, 3, generator=g) * 0.3, ds)
    gt_parts = center_pose_parts(torch.randn(B, Fr, 134, 3, generator=g) * 0.3, ds)
    x2d = torch.rand(B, Fr, 134, 2, generator=g) * 2 - 1
    traj = torch.randn(B, Fr, 1, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    return pred_parts, gt_parts, x2d, traj


def main():
    mg.install_shims()
    from common.utils import wb_pose_from_parts
    np.linalg.svd = _svd_nan_for_nonfinite(np.linalg.svd)
    ds = mg.FakeDataset()
    cam = torch.tensor(CAM)
    arrays = {}

    # random: inputs re-generated from the seed wherever the fixture is read
    from tests.golden import g21_inputs
    z = g21_inputs.random_inputs()
    pred_parts, gt_parts, x2d, traj = random_case(g21_inputs.RANDOM_SEED, *g21_inputs.RANDOM_SIZES, ds)
    assert all(torch.equal(a, b) for a, b in zip((pred_parts, gt_parts, x2d, traj), z.values()))   # reference bits
    out, _ = reference_p2(pred_parts, gt_parts, x2d, traj, cam, ds)
    sha = np.frombuffer(g21_inputs.digest(z), dtype=np.uint8)
    arrays.update({"random__" + k: v for k, v in dict(cam=cam, sha256=sha, **out).items()})

    # rigid: hypotheses = a X R (+ noise) of the whole-body target, hypothesis 1 mirrored
    B, T, P, Fr = 1, 2, 3, 3
    _, gt_parts, x2d, traj = random_case(212, B, T, P, Fr, ds)
    g = np.random.default_rng(213)
    X = wb_pose_from_parts(gt_parts.clone(), ds).double()                       # [B,F,J,3], joint 0 at 0
    Y = torch.empty(B, T, P, Fr, 134, 3, dtype=torch.float64)
    for t in range(T):
        for h in range(P):
            q, _ = np.linalg.qr(g.normal(size=(3, 3)))
            q *= np.sign(np.linalg.det(q))                                      # a proper rotation
            if h == 1:
                q[:, 0] *= -1                                                   # ... mirrored
            a = g.uniform(0.7, 1.4)
            Y[:, t, h] = a * X @ torch.from_numpy(q) + torch.from_numpy(g.normal(size=(B, Fr, 134, 3)) * 5e-4)
    Y[..., 0, :] = 0.0
    pred_parts = wb_inverse(Y, ds).float()
    out, pred = reference_p2(pred_parts, gt_parts, x2d, traj, cam, ds, with_p1=True)
    assert (pred.double() - Y).abs().max() < 1e-6                              # the inverse is exact up to fp32 rounding
    assert (out["p2_j_best"] * 1000 < 2).all() and (out["j_best"] > 0.1).all(), out
    arrays.update({"rigid__" + k: v for k, v in dict(pred_parts=pred_parts, gt_parts=gt_parts, x2d=x2d, traj=traj,
                                                     cam=cam, **out).items()})

    # degenerate: one all-zero hypothesis at step 0
    pred_parts, gt_parts, x2d, traj = random_case(214, 1, 2, 3, 3, ds)
    pred_parts[:, 0, 1] = 0.0
    out, _ = reference_p2(pred_parts, gt_parts, x2d, traj, cam, ds)
    assert torch.isnan(out["p2_j_best"][0]) and torch.isfinite(out["p2_j_best"][1])
    arrays.update({"degenerate__" + k: v for k, v in dict(pred_parts=pred_parts, gt_parts=gt_parts, x2d=x2d,
                                                          traj=traj, cam=cam, **out).items()})
    for k, v in arrays.items():
        if k.split("__")[1].startswith(("p2_", "j_best", "p_best")):
            print(k, v.tolist())
    mg.save("g21_p2_metrics.npz", **arrays)


if __name__ == "__main__":
    main()

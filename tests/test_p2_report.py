"""Protocol #2 (P-MPJPE, ``ft2d.p2``) on the host side: the log lines of main_h3wb.py:511-519 and an fp64 statement of
the metric (common/loss.py:251-458 on whole-body poses) checked against the reference-generated fixture G21.

``p2_truth`` is the yardstick of tests/test_hip_procrustes.py as well."""
import io

import pytest
import torch

from oracle import d3dp_oracle as orc
from tests.conftest import load_golden
from tests.golden import golden_util as gu

CASES = ("random", "rigid", "degenerate")


def conn_table(J=134):
    """connection joint of every joint as wb_pose_from_parts uses it (body -> 0)"""
    conn = torch.zeros(J, dtype=torch.int32)
    for part, idx in gu.DATASET_PART_JOINTS.items():
        conn[list(idx)] = 0 if part == "body" else gu.CONNECTION_INDICES[part]
    return conn


def wb(pose, conn):
    """closed form of wb_pose_from_parts for any connection table: pose[j] + pose[conn[j]], joint 0 at the origin"""
    out = pose + pose[..., conn.long(), :]
    out[..., 0, :] = 0
    return out


def align_errors(Y, X):
    """per-joint errors [..., J] of the poses Y [..., J, 3] after the reference's similarity alignment onto X, in fp64
    (SVD with the reflection fix, row vectors as numpy writes it); NaN for a pose whose SVD input is not finite"""
    Y, X = Y.double(), X.double()
    muX, muY = X.mean(-2, keepdim=True), Y.mean(-2, keepdim=True)
    X0, Y0 = X - muX, Y - muY
    nX = X0.pow(2).sum((-2, -1), keepdim=True).sqrt()
    nY = Y0.pow(2).sum((-2, -1), keepdim=True).sqrt()
    H = (X0 / nX).transpose(-1, -2) @ (Y0 / nY)
    ok = torch.isfinite(H).all(-1).all(-1)
    U, s, Vt = torch.linalg.svd(torch.where(ok[..., None, None], H, torch.zeros_like(H)))
    V = Vt.transpose(-1, -2)
    d = torch.sign(torch.linalg.det(V @ U.transpose(-1, -2)))
    V = torch.cat([V[..., :2], V[..., 2:] * d[..., None, None]], dim=-1)
    s = torch.cat([s[..., :2], s[..., 2:] * d[..., None]], dim=-1)
    R = V @ U.transpose(-1, -2)
    a = s.sum(-1)[..., None, None] * nX / nY
    t = muX - a * (muY @ R)
    err = (a * (Y @ R) + t - X).norm(dim=-1)
    return torch.where(ok[..., None], err, torch.full_like(err, float("nan")))


def reprojection_pick(pred_wb, x2d, traj, cam):
    """J-Agg's hypothesis: smallest 2-D reprojection error of the UNALIGNED absolute pose, first minimum (fp32)"""
    B, T, P, F, J, _ = pred_wb.shape
    absolute = (pred_wb + traj.reshape(B, 1, 1, F, 1, 3)).reshape(-1, J, 3)
    reproj = orc.project_to_2d(absolute, cam.reshape(1, 9).repeat(absolute.shape[0], 1)).reshape(B, T, P, F, J, 2)
    return (reproj - x2d[:, None, None]).norm(dim=-1).min(dim=2).indices           # [B,T,F,J]


def p2_truth(pred_parts, gt_parts, x2d, traj, cam, conn=None, pick=None):
    """fp64 Protocol #2 of the contract: per-pose errors e [B,T,P,F,J], mean-pose errors [B,T,F,J], the pick and the
    four per-step vectors [T] (metres).  `pick` [B,T,F,J] replaces the fp32 reprojection pick when given."""
    pred_parts, gt_parts, x2d, traj, cam = (t.detach().cpu().float() for t in (pred_parts, gt_parts, x2d, traj, cam))
    B, T, P, F, J, _ = pred_parts.shape
    conn = conn_table(J) if conn is None else conn.cpu()
    pred, gt = wb(pred_parts, conn), wb(gt_parts, conn)                        # fp32, as the reference forms them
    e = align_errors(pred, gt[:, None, None].expand(B, T, P, F, J, 3))
    e_mean = align_errors(pred.double().mean(dim=2), gt[:, None].expand(B, T, F, J, 3))
    if pick is None:
        pick = reprojection_pick(pred, x2d, traj, cam)
    pick = pick.cpu().long()
    jbest = e.amin(dim=2)                                                       # propagates NaN, like np.min
    jagg = e.gather(2, pick.unsqueeze(2)).squeeze(2)

    def per_t(x):
        return x.transpose(0, 1).reshape(T, -1).mean(-1)

    per_h = e.permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1)
    return {"e": e, "e_mean": e_mean, "pick": pick, "jbest": jbest, "jagg": jagg,
            "p2_j_best": per_t(jbest), "p2_p_best": per_h.min(dim=1).values, "p2_p_agg": per_t(e_mean),
            "p2_j_agg": per_t(jagg)}


def g21_case(name):
    """one case of G21; the random case's inputs re-generated from their seed and checked against the stored SHA-256"""
    from tests.golden import g21_inputs
    z = load_golden("g21_p2_metrics.npz")
    case = {k.split("__", 1)[1]: v for k, v in z.items() if k.startswith(name + "__")}
    if "sha256" in case:
        inputs = g21_inputs.random_inputs()
        assert g21_inputs.digest(inputs) == case.pop("sha256").numpy().tobytes(), "G21 inputs did not re-generate"
        case.update(inputs)
    return case


# G21 is float32: its poses (~1 m) carry ~6e-8 m of rounding per coordinate, which every aligned error inherits
# whatever its size - the rigid case's 0.5 mm errors sit 8e-6 relative from fp64.  Hence an absolute floor of
# 1e-7 m (under 2 fp32 ulps of a 1 m coordinate) beside the relative 1e-6.
G21_ATOL = 1e-7


def same_nan_and_close(got, want, rtol, atol=0.0):
    got, want = got.double().cpu(), want.double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (got, want)
    ok = ~torch.isnan(want)
    assert torch.allclose(got[ok], want[ok], rtol=rtol, atol=atol), (got, want, (got - want).abs().max())


@pytest.mark.parametrize("case", CASES)
def test_fp64_truth_reproduces_g21(case):
    """G21 holds the reference's float32 numpy results; the fp64 statement of the contract lands within rtol 1e-6
    (fp32 SVD and means of ~7000 errors: a few ulps, 1 ulp = 6e-8 relative) + G21_ATOL, NaN exactly where the
    reference has NaN."""
    z = g21_case(case)
    got = p2_truth(z["pred_parts"], z["gt_parts"], z["x2d"], z["traj"], z["cam"])
    for k in ("p2_j_best", "p2_p_best", "p2_p_agg", "p2_j_agg"):
        same_nan_and_close(got[k], z[k], 1e-6, G21_ATOL)
    if case == "degenerate":
        assert torch.isnan(z["p2_j_best"][0]) and torch.isnan(got["e"][:, 0, 1]).all()
    if case == "rigid":       # similarity transforms + 0.5 mm noise: P2 three orders below P1
        assert (z["p2_j_best"] < 2e-3).all() and (z["p2_p_best"] < 2e-3).all() and (z["j_best"] > 0.5).all()


def _rep(T=2, p2=True):
    from pafuse_amd import harness
    keys = harness.ACCUMULATORS_P2 if p2 else harness.ACCUMULATORS
    return {k: [float(i + 1) + 0.125 * j + (1.0 / 3.0 if k.startswith("p2_") else 0.0) for j in range(T)]
            for i, k in enumerate(keys)}


def test_format_report_protocol2_lines_are_the_reference_s():
    """main_h3wb.py:511-519 restated as data: the printed lines are what ``print(fmt % ii, value, 'mm')`` prints
    (str of the float), the written ones use %f, all four (P_Best included) are written, and they close each step's
    block right after the P_Agg Part-Based RIGHT HAND line."""
    from pafuse_amd import harness
    rep = _rep()
    printed, written = harness.format_report(rep, True)
    statements = (("step %d : Protocol #2 Error (MPJPE) J_Best:", "step %d : Protocol #2 Error (MPJPE) J_Best: %f mm\n", "p2_j_best"),
                  ("step %d : Protocol #2 Error (MPJPE) P_Best:", "step %d : Protocol #2 Error (MPJPE) P_Best: %f mm\n", "p2_p_best"),
                  ("step %d : Protocol #2 Error (MPJPE) P_Agg:", "step %d : Protocol #2 Error (MPJPE) P_Agg: %f mm\n", "p2_p_agg"),
                  ("step %d : Protocol #2 Error (MPJPE) J_Agg:", "step %d : Protocol #2 Error (MPJPE) J_Agg: %f mm\n", "p2_j_agg"))
    for ii in range(2):
        out, f = io.StringIO(), io.StringIO()
        for pfmt, wfmt, key in statements:
            print(pfmt % ii, rep[key][ii], "mm", file=out)
            f.write(wfmt % (ii, rep[key][ii]))
        want_p, want_w = out.getvalue().splitlines(), f.getvalue().splitlines()
        assert want_p[0] == "step %d : Protocol #2 Error (MPJPE) J_Best: %r mm" % (ii, rep["p2_j_best"][ii])
        last = "step %d : Protocol #1 Error (MPJPE) P_Agg Part-Based RIGHT HAND: %f mm" % (ii, rep["p_agg_pb_right_hand"][ii])
        i, k = printed.index(last), written.index(last)
        assert printed[i + 1:i + 5] == want_p and written[k + 1:k + 5] == want_w
    assert printed[-1] == written[-1] == "----------"
    assert len(printed) == 2 + 2 * 22 + 1 and sum("Protocol #2" in line for line in written) == 8


def test_format_report_without_protocol2_is_unchanged():
    """without p2_* keys: the Protocol #1 report line for line (dropping the P2 lines of a P2 report gives it too)"""
    from pafuse_amd import harness
    rep = _rep(p2=False)
    printed, written = harness.format_report(rep, True, action="Walking")
    assert not any("Protocol #2" in line for line in printed + written)
    assert len(printed) == 2 + 2 * 18 + 1 and printed[2] == "step 0 : Protocol #1 Error (MPJPE) J_Best: 1.000000 mm"
    p2p, p2w = harness.format_report(dict(rep, **{k: v for k, v in _rep().items() if k.startswith("p2_")}), True,
                                     action="Walking")
    assert [l for l in p2p if "Protocol #2" not in l] == printed and [l for l in p2w if "Protocol #2" not in l] == written


def test_accumulator_names():
    from pafuse_amd import harness
    assert len(harness.ACCUMULATORS) == 14 and harness.ACCUMULATORS_P2[:14] == harness.ACCUMULATORS
    assert harness.ACCUMULATORS_P2[14:] == ("p2_j_best", "p2_p_best", "p2_p_agg", "p2_j_agg")


def test_evaluate_accumulators_p2_refuses_cpu_tensors():
    """no CPU fallback for P2 either (raises before touching a device)"""
    from types import SimpleNamespace
    from pafuse_amd import _lib
    from pafuse_amd.evaluate import evaluate_accumulators
    z = g21_case("degenerate")
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                         parts_connection_indices=dict(gu.CONNECTION_INDICES))
    with pytest.raises(_lib.PafuseError):
        evaluate_accumulators(z["pred_parts"], z["gt_parts"], z["x2d"], z["traj"], z["cam"], ds, p2=True)

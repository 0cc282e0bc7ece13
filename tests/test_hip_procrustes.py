"""Protocol #2 on the device: procrustes_kernel (pafuse_procrustes_errors) and evaluate_accumulators(p2=True).

Bounds, derived:
  * per-(b,t,f,j) errors against the fp64 truth of tests/test_p2_report.py: 1e-6 m.  The kernel works in fp64 on the
    same fp32 whole-body poses; the only fp32 step is the stored error (half an ulp of a <= 4 m error is 1.2e-7 m).
    The SVD route and Horn's route agree to 1e-13 m in fp64, 8 Jacobi sweeps being 3 past convergence on 4x4.
  * per-pose sums over J: 1e-6 relative (fp64 sums, both sides; the slack is for the different summation order only).
  * per-step vectors: rtol 1e-6 against the truth (means of fp32-rounded per-joint values: < 1e-7 relative).
  * against G21 (the reference's float32 numpy): rtol 1e-6 + 1e-7 m, the floor for the fp32 rounding of ~1 m poses
    that the fixture's own errors carry (tests/test_p2_report.py, G21_ATOL).
  * end to end against the oracle's loop: rtol 5e-6, the bound test_h3wb_files_to_protocol_numbers uses for the HIP
    loop's predictions (~1e-6 m apart from the oracle's) feeding the same metric.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from oracle import d3dp_oracle as orc
from tests.golden import golden_util as gu
from tests.test_p2_report import CASES, G21_ATOL, conn_table, g21_case, p2_truth, same_nan_and_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
P2_KEYS = ("p2_j_best", "p2_p_best", "p2_p_agg", "p2_j_agg")


def dataset():
    return SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                           parts_connection_indices=dict(gu.CONNECTION_INDICES))


def random_inputs(B, T, P, F, J, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, T, P, F, J, 3, generator=g) * 0.3
    gt = torch.randn(B, F, J, 3, generator=g) * 0.3
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    traj = torch.randn(B, F, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    return pred, gt, x2d, traj, cam


def small_conn(J, seed):
    """a connection table for J joints: a body (conn 0) and parts hanging off random body joints"""
    g = torch.Generator().manual_seed(seed)
    nb = max(2, J // 3)
    conn = torch.zeros(J, dtype=torch.int32)
    conn[nb:] = torch.randint(1, nb, (J - nb,), generator=g, dtype=torch.int32)
    return conn


def run(pred, gt, x2d, traj, cam, conn, pick=True):
    from pafuse_amd import ops
    return ops.procrustes_errors(*(t.contiguous().to(DEV) for t in (pred, gt, x2d, traj, cam, conn)), pick=pick)


def accumulators(z, p2=True):
    from pafuse_amd.evaluate import evaluate_accumulators
    return evaluate_accumulators(z["pred_parts"].to(DEV), z["gt_parts"].to(DEV), z["x2d"].to(DEV), z["traj"].to(DEV),
                                 z["cam"].to(DEV), dataset(), p2=p2)


@pytest.mark.parametrize("case", CASES)
def test_g21_through_evaluate_accumulators(case):
    z = g21_case(case)
    got = accumulators(z)
    assert set(P2_KEYS) <= set(got) and len(got) == 18
    for k in P2_KEYS:
        same_nan_and_close(got[k], z[k], 1e-6, G21_ATOL)
    if case == "rigid":       # similarity transforms + 0.5 mm noise: P2 <= 2 mm where P1 is ~1 m
        assert (got["p2_j_best"] <= 2e-3).all() and (got["p2_p_best"] <= 2e-3).all()
        assert (got["j_best"] > 0.5).all() and (got["p_best"] > 0.5).all()


def test_rigid_mirrored_hypothesis_stays_unaligned():
    """hypothesis 1 of the rigid case is a mirror image: no proper rotation aligns it, so its aligned error stays far
    above the noise level of the others (an alignment that allowed det R = -1 would bring it down to ~0.5 mm)"""
    z = g21_case("rigid")
    J = z["pred_parts"].shape[-2]
    r = run(z["pred_parts"], z["gt_parts"], z["x2d"], z["traj"].reshape(*z["traj"].shape[:2], 3), z["cam"].reshape(9),
            conn_table(J))
    per_pose = r["pbest_sums"].cpu() / J                                        # [B,T,P,F] mean aligned error
    others = torch.cat([per_pose[:, :, :1], per_pose[:, :, 2:]], dim=2)
    assert (others < 2e-3).all() and (per_pose[:, :, 1] > 20e-3).all(), per_pose


@pytest.mark.parametrize("B,T,P,F,J", [(2, 2, 5, 9, 134), (2, 3, 3, 5, 17), (1, 1, 160, 3, 134), (1, 2, 1, 4, 256)])
def test_kernel_vs_fp64_truth(B, T, P, F, J):
    """random inputs, J = 134 (three lane slots), 17 (a partial wave), 256 (the limit); P up to 160 (8 gathered
    shards of 20): every output against the fp64 truth; the J-Agg error taken at the kernel's own pick, which must be
    the fp32 reprojection pick of the truth"""
    pred, gt, x2d, traj, cam = random_inputs(B, T, P, F, J, seed=1000 + J + P)
    conn = conn_table(J) if J == 134 else small_conn(J, J)
    r = run(pred, gt, x2d, traj, cam, conn)
    truth = p2_truth(pred, gt, x2d, traj, cam, conn=conn, pick=r["pick"])
    want_pick = p2_truth(pred, gt, x2d, traj, cam, conn=conn)["pick"]
    assert (r["pick"].cpu().long() == want_pick).float().mean() > 0.999          # fp32 near-ties aside
    for k, w in (("jbest", truth["jbest"]), ("pagg", truth["e_mean"]), ("jagg", truth["jagg"])):
        d = (r[k].cpu().double() - w).abs().max().item()
        assert d <= 1e-6, (k, d)
    sums = truth["e"].sum(-1)                                                   # [B,T,P,F]
    assert torch.allclose(r["pbest_sums"].cpu(), sums, rtol=1e-6, atol=0)
    if J == 134:
        z = {"pred_parts": pred, "gt_parts": gt, "x2d": x2d, "traj": traj, "cam": cam}
        got = accumulators(z)
        for k in P2_KEYS:
            assert torch.allclose(got[k].cpu().double(), truth[k], rtol=1e-6, atol=0), (k, got[k], truth[k])


def test_single_hypothesis_all_equal():
    """P = 1: the minimum, the pick and the mean pose are that one pose -> bit-equal per joint; the P-Best sum is the
    same errors summed in the kernel's lane order"""
    pred, gt, x2d, traj, cam = random_inputs(2, 2, 1, 6, 134, seed=7)
    r = run(pred, gt, x2d, traj, cam, conn_table())
    assert (r["pick"] == 0).all()
    assert torch.equal(r["jbest"], r["jagg"]) and torch.equal(r["jbest"], r["pagg"])
    assert torch.allclose(r["pbest_sums"][:, :, 0], r["jbest"].double().sum(-1), rtol=1e-6, atol=0)


def test_hypothesis_permutation_and_repeats_are_bit_equal():
    pred, gt, x2d, traj, cam = random_inputs(2, 2, 7, 5, 134, seed=11)
    conn = conn_table()
    r1, r2 = run(pred, gt, x2d, traj, cam, conn), run(pred, gt, x2d, traj, cam, conn)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    perm = torch.tensor([3, 6, 0, 5, 1, 4, 2])
    rp = run(pred[:, :, perm], gt, x2d, traj, cam, conn)
    assert torch.equal(rp["jbest"], r1["jbest"])
    assert torch.equal(rp["pbest_sums"], r1["pbest_sums"][:, :, perm.to(DEV)])
    z = {"pred_parts": pred, "gt_parts": gt, "x2d": x2d, "traj": traj, "cam": cam}
    zp = dict(z, pred_parts=pred[:, :, perm])
    a, b = accumulators(z), accumulators(zp)
    assert torch.equal(a["p2_j_best"], b["p2_j_best"]) and torch.equal(a["p2_p_best"], b["p2_p_best"])


def test_picks_agree_with_protocol1():
    """the J-Agg pick of both protocols is one pick: pafuse_hypothesis_errors' e3 gathered at the P2 pick is its jagg"""
    from pafuse_amd import _lib
    from pafuse_amd.evaluate import _tables
    B, T, P, F, J = 2, 3, 6, 9, 134
    pred, gt, x2d, traj, cam = (t.to(DEV) for t in random_inputs(B, T, P, F, J, seed=21))
    conn, pbroot = _tables(dataset(), J, DEV)
    e3, epb = torch.empty(B, T, P, F, J, device=DEV), torch.empty(B, T, P, F, J, device=DEV)
    jbest, pagg, jagg, paggpb = (torch.empty(B, T, F, J, device=DEV) for _ in range(4))
    lib = _lib.load()
    _lib.check(lib.pafuse_hypothesis_errors(
        pred.data_ptr(), gt.data_ptr(), x2d.data_ptr(), traj.data_ptr(), cam.data_ptr(), conn.data_ptr(),
        pbroot.data_ptr(), B, T, P, F, J, e3.data_ptr(), epb.data_ptr(), jbest.data_ptr(), pagg.data_ptr(),
        jagg.data_ptr(), paggpb.data_ptr(), torch.cuda.current_stream().cuda_stream))
    r = run(pred, gt, x2d, traj, cam, conn)
    assert (r["pick"] >= 0).all()
    assert torch.equal(e3.gather(2, r["pick"].long().unsqueeze(2)).squeeze(2), jagg)


def test_protocol1_unchanged_by_p2():
    z = g21_case("random")
    a, b = accumulators(z, p2=False), accumulators(z, p2=True)
    assert len(a) == 14 and set(b) == set(a) | set(P2_KEYS)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_degenerate_pose_gives_nan_not_a_fault():
    """|Y0| = 0 (an all-zero hypothesis): NaN for that pose, the NaN carried into the minimum (no fminf dropping it),
    other steps untouched"""
    z = g21_case("degenerate")
    r = run(z["pred_parts"], z["gt_parts"], z["x2d"], z["traj"].reshape(*z["traj"].shape[:2], 3), z["cam"].reshape(9),
            conn_table())
    assert torch.isnan(r["pbest_sums"][:, 0, 1]).all() and torch.isfinite(r["pbest_sums"][:, 1]).all()
    assert torch.isnan(r["jbest"][:, 0]).all() and torch.isfinite(r["jbest"][:, 1]).all()
    assert torch.isfinite(r["pagg"]).all()


def test_refusals():
    from pafuse_amd import _lib
    from pafuse_amd.evaluate import evaluate_accumulators
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()
    s = torch.cuda.current_stream().cuda_stream

    def call(*sizes, ptrs=None):
        ptrs = ptrs or [p] * 6
        return lib.pafuse_procrustes_errors(*ptrs, *sizes, p, p, p, p, None, s)

    assert call(1, 1, 1, 1, 257) == _lib_e_arg()
    for sizes in ((0, 1, 1, 1, 17), (1, 0, 1, 1, 17), (1, 1, 0, 1, 17), (1, 1, 1, 0, 17), (1, 1, 1, 1, 0), (-1, 1, 1, 1, 17)):
        assert call(*sizes) == _lib_e_arg(), sizes
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert call(1, 1, 1, 1, 17, ptrs=ptrs) == _lib_e_arg(), i
    assert lib.pafuse_procrustes_errors(p, p, p, p, p, p, 1, 1, 1, 1, 17, None, p, p, p, None, s) == _lib_e_arg()
    z = g21_case("degenerate")
    with pytest.raises(_lib.PafuseError):
        evaluate_accumulators(z["pred_parts"], z["gt_parts"], z["x2d"], z["traj"], z["cam"], dataset(), p2=True)
    torch.cuda.synchronize()


def _lib_e_arg():
    return -1     # PAFUSE_E_ARG


def test_h3wb_files_to_protocol2_numbers():
    """evaluate() from files with p2=True: the Protocol #2 numbers against the oracle loop's predictions scored by the
    fp64 truth, and the Protocol #2 block in the log"""
    import os
    from __graft_entry__ import make_model
    from pafuse_amd import h3wb, harness
    from tests.conftest import ROOT
    ds = h3wb.Human3WBDataset(os.path.join(ROOT, "tests", "golden", "h3wb_synth", "train_h3wb.npz"))
    keypoints = h3wb.prepare_keypoints(ds)
    kps_left, kps_right = ds.keypoints_metadata["keypoints_symmetry"]
    cams, p3, p2 = h3wb.fetch(["S8"], keypoints, ds)
    P, T = 2, 1
    model, sd = make_model(P, T, seed=87)
    noises = gu.synthetic_noises(B=1, P=P, n=T, seed=14)
    model.noise_fn = lambda k, shape, device: noises[k]
    lines = []
    rep = h3wb.evaluate(model, ds, cams, p3, p2, kps_left, kps_right, log=lines.append, p2=True)
    assert set(rep) == set(harness.ACCUMULATORS_P2)
    total, n = None, 0
    for cam, s3, s2 in zip(cams, p3, p2):
        s2, s3 = torch.as_tensor(s2, dtype=torch.float32), torch.as_tensor(s3, dtype=torch.float32)
        x2d, gt = harness.cut_clips(s2), harness.cut_clips(s3)
        x2f = harness.cut_clips(harness.flip_2d(s2, kps_left, kps_right))
        pred = orc.ddim_sample(sd, x2d, noises, T, model.joints_left, model.joints_right, inputs_2d_flip=x2f)
        acc = p2_truth(pred, orc.center_pose_parts(gt), x2d, gt[:, :, 0], torch.as_tensor(cam, dtype=torch.float32))
        mult = x2d.shape[0] * 27
        total = {k: mult * acc[k] for k in P2_KEYS} if total is None else {k: total[k] + mult * acc[k] for k in P2_KEYS}
        n += mult
    for k in P2_KEYS:
        want = total[k] / n * 1000.0
        assert torch.allclose(torch.tensor(rep[k], dtype=torch.float64), want, rtol=5e-6, atol=0), (k, rep[k], want)
    for name in ("J_Best", "P_Best", "P_Agg", "J_Agg"):
        assert any(line.startswith("step 0 : Protocol #2 Error (MPJPE) %s: " % name) for line in lines), name

"""J-Agg without a trajectory: pose_fit_partials_kernel (pafuse_pose_partials_fit), torch.ops.pafuse.aggregate_poses_fit,
evaluate.accumulate_poses(fit=True) and infer_sequence(aggregate="reproj_fit").

What is asserted and why it can be asserted:
  * tfit: the kernel and pafuse_amd/rootfit.py perform the same IEEE fp64 operations in the same order (every sum over
    the joints in the pinned lane order, contraction off, correctly rounded divides), then round once to fp32 -> the design
    goal is equal bits; the test accepts equal or ADJACENT fp32 values, as the spread tests do, and prints how many differ.
  * the pick: e2 is pose_partials_kernel's fp32 expression with the fitted root in the place of traj -> the state's
    (e2, idx, sel) are torch.equal to the first minimum over h of THAT kernel's e2, run on one hypothesis at a time with
    traj = tfit, with the joints without a weight and the hypotheses without a fit masked out (pose_partials_kernel
    itself would clamp a NaN root to a finite error).
  * sum: the adds of pose_partials_kernel -> torch.equal to the mean-only state's.
Shapes: B = 2, T = 2, F = 3 (12 waves: three workgroups of four) and J in {5, 64, 65, 134}: lanes without a joint, exactly
one round, one joint in a second round, the real three rounds with a ragged third; P_r in {1, 5} and once 70 (more than the
64 hypotheses the kernel takes at a time); h0 = 0 and h0 > 0.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, same_bits, sequence, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, F = 2, 2, 3
ROOT_TRUE = (0.3, -0.2, 4.5)
CAM = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
# (J, P_r, h0); P_r = 70: the kernel takes the hypotheses 64 at a time and carries a joint's element through the state between
CASES = [(5, 5, 0), (64, 5, 3), (65, 1, 0), (65, 5, 2), (134, 5, 0), (134, 1, 7), (134, 5, 4), (65, 70, 1)]


def conn_of(J):
    """the connection table: the dataset's for the whole body, any table with conn[j] < J otherwise"""
    return tables()[0] if J == 134 else (torch.arange(J, dtype=torch.int32) // 3).to(DEV)


def whole_body(pred, conn):
    from pafuse_amd import rootfit
    return rootfit.whole_body(pred.cpu().numpy(), conn.cpu().numpy())


def project(wb, root, cam):
    """exact pinhole detections (no distortion) of the absolute points wb + root, computed in fp64, rounded to fp32"""
    X = wb.astype(np.float64) + np.asarray(root, dtype=np.float64)
    fx, fy, cx, cy = (np.float64(v) for v in cam[:4].numpy())
    return np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], axis=-1).astype(np.float32)


def inputs(J, P, seed, weights=True):
    """hypotheses scattered 5 cm about a pose seen from ROOT_TRUE, its detections with 2 % noise; weights=True: a fifth of the
    joints of every frame not found (weight 0, detection (0, 0)), two joints with a negative and a NaN weight"""
    g = torch.Generator().manual_seed(seed)
    conn = conn_of(J)
    base = torch.randn(B, F, J, 3, generator=g) * 0.2
    pred = (base[:, None, None] + torch.randn(B, T, P, F, J, 3, generator=g) * 0.05).contiguous()
    x2d = torch.from_numpy(project(whole_body(base, conn), ROOT_TRUE, CAM)) + torch.randn(B, F, J, 2, generator=g) * 0.02
    conf = None
    if weights:
        conf = torch.rand(B, F, J, generator=g) * 0.9 + 0.1
        lost = torch.rand(B, F, J, generator=g) < 0.2
        lost[..., :2] = False                                   # at least two joints stay: every frame has a fit
        conf[lost] = 0
        x2d[lost] = 0
        if J > 4:
            conf[0, 0, 3], conf[1, 2, 4] = -0.5, float("nan")
    z = {"pred": pred, "x2d": x2d.contiguous(), "cam": CAM.clone(), "conf": conf}
    return {k: (None if v is None else v.to(DEV)) for k, v in z.items()}, conn


def fit(z, conn, h0=0, lo=0, hi=None, conf="own", x2d=None):
    """the fit state of the hypotheses [lo, hi) as global [h0 + lo, h0 + hi) -> (state, views, tfit)"""
    from pafuse_amd import ops
    pred = z["pred"][:, :, lo:hi].contiguous()
    J = pred.shape[4]
    tfit = torch.full((B, T, pred.shape[2], F, 3), 7.0, device=DEV)
    state = ops.pose_partials_fit(pred, conn, h0 + lo, z["x2d"] if x2d is None else x2d, z["cam"],
                                  conf=z["conf"] if isinstance(conf, str) else conf, tfit=tfit)
    return state, ops.pose_views(state, B, T, F, J), tfit


def weighted(z, J):
    return torch.ones(B, F, J, dtype=torch.bool, device=DEV) if z["conf"] is None else z["conf"] > 0


def equal_or_adjacent(a, b):
    """same NaN places; elsewhere equal or neighbours in fp32; -> the number of values that are not equal"""
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
    step = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).abs()
    assert bool(((a - b).abs() <= step).all()), float((a - b).abs().max())
    return int((a != b).sum())


@pytest.fixture(scope="module")
def cases():
    """inputs and the kernel's state and roots for every (J, P_r, h0), computed once and never modified"""
    out = {}
    for J, P, h0 in CASES:
        z, conn = inputs(J, P, seed=100 + J + P + h0)
        out[J, P, h0] = (z, conn) + fit(z, conn, h0)
    return out


@pytest.mark.parametrize("case", CASES)
def test_tfit_is_the_statement(cases, case):
    from pafuse_amd import rootfit
    z, conn, _, _, tfit = cases[case]
    want = rootfit.fit_roots(whole_body(z["pred"], conn), z["x2d"].cpu().numpy(),
                             None if z["conf"] is None else z["conf"].cpu().numpy(), z["cam"].cpu().numpy())
    assert not np.isnan(want).any()                                 # every frame of these inputs keeps two joints or more
    differ = equal_or_adjacent(tfit.cpu(), torch.from_numpy(want))
    print(f"(J, P_r, h0) = {case}: {differ} of {tfit.numel()} roots differ from the statement (by one fp32 step)")
    if case[0] == 134:      # and it is a root, not just a number: ~100 joints 8 cm off at 4.5 m put the depth within 0.12 m (1 sigma)
        assert (tfit[..., 2] - ROOT_TRUE[2]).abs().max() < 1.0


@pytest.mark.parametrize("case", CASES)
def test_pick_is_the_existing_kernels_pick_on_the_fitted_roots(cases, case):
    from pafuse_amd import ops
    J, P, h0 = case
    z, conn, _, v, tfit = cases[case]
    x2d_bt = z["x2d"][:, None].expand(B, T, F, J, 2).reshape(B * T, F, J, 2).contiguous()
    best = torch.full((B, T, F, J), float("inf"), device=DEV)
    idx = torch.full((B, T, F, J), -1, device=DEV, dtype=torch.int32)
    sel = torch.full((B, T, F, J, 3), float("nan"), device=DEV)
    keep = weighted(z, J)[:, None].expand(B, T, F, J)
    for h in range(P):
        one = z["pred"][:, :, h].reshape(B * T, 1, 1, F, J, 3).contiguous()
        traj = tfit[:, :, h].reshape(B * T, F, 3).contiguous()
        s = ops.pose_views(ops.pose_partials(one, conn, h0 + h, x2d_bt, traj, z["cam"]), B * T, 1, F, J)
        fitted = ~torch.isnan(tfit[:, :, h]).any(dim=-1)            # [B,T,F]
        better = (s["e2"].view(B, T, F, J) < best) & keep & fitted[..., None]      # strict: the first minimum wins
        best = torch.where(better, s["e2"].view(B, T, F, J), best)
        idx = torch.where(better, s["idx"].view(B, T, F, J), idx)
        sel = torch.where(better[..., None], s["sel"].view(B, T, F, J, 3), sel)
    assert same_bits(v["e2"], best) and torch.equal(v["idx"], idx) and same_bits(v["sel"], sel)
    assert bool((v["idx"][keep] >= h0).all()) and bool((v["idx"][~keep] == -1).all())
    if P == 5 and J > 5:
        assert len(v["idx"][keep].unique()) == P                    # every hypothesis wins somewhere: the test can tell them apart


@pytest.mark.parametrize("case", CASES)
def test_sum_is_the_mean_only_sum(cases, case):
    from pafuse_amd import ops
    J, P, h0 = case
    z, conn, _, v, _ = cases[case]
    plain = ops.pose_views(ops.pose_partials(z["pred"], conn, h0), B, T, F, J)
    assert same_bits(v["sum"], plain["sum"])


@pytest.mark.parametrize("J", [65, 134])
def test_splits_combine_to_the_same_bits(J):
    from pafuse_amd import ops
    z, conn = inputs(J, 5, seed=21)
    L = ops.pose_partials_bytes(B, T, F, J) // 8
    got = {}
    for sizes in ((5,), (2, 3), (4, 1), (1, 1, 1, 1, 1)):
        states = torch.full((len(sizes), L + 3), float("nan"), device=DEV, dtype=torch.float64)      # padded rows
        roots, lo = [], 0
        for r, n in enumerate(sizes):
            tfit = torch.empty(B, T, n, F, 3, device=DEV)
            ops.pose_partials_fit(z["pred"][:, :, lo:lo + n].contiguous(), conn, lo, z["x2d"], z["cam"], conf=z["conf"],
                                  out=states[r], tfit=tfit)
            roots.append(tfit)
            lo += n
        got[sizes] = (ops.combine_poses(states, (B, T, F, J), 5), torch.cat(roots, dim=2))
    one, roots = got[(5,)]
    assert bool((one["idx"] >= 0).any()) and bool((one["idx"] == -1).any())
    for sizes, (m, r) in got.items():
        assert same_bits(m["pick"], one["pick"]) and torch.equal(m["idx"], one["idx"]) and torch.equal(m["mean"], one["mean"]), sizes
        assert same_bits(r, roots), sizes


@pytest.mark.parametrize("J,with_weights", [(134, True), (5, False)])
def test_planted_truth(J, with_weights):
    """hypothesis 3 is exactly the pose that was projected, the others are 5 cm off: every weighted joint picks 3, and its
    root is the planted one to 1e-5 m (an fp32 output at depth 4.5 m: 1 ulp = 4.8e-7 m, plus the fp32 rounding of the
    detections, 1e-6 m at most through the fit - tests/test_rootfit_host.py)"""
    from pafuse_amd import ops
    z, conn = inputs(J, 5, seed=31, weights=with_weights)
    cam = CAM.clone()
    cam[4:] = 0
    x2d = torch.from_numpy(project(whole_body(z["pred"][:, 0, 3], conn), ROOT_TRUE, cam)).to(DEV)       # [B,F,J,2], t = 0's pose
    if z["conf"] is not None:
        x2d[~(z["conf"] > 0)] = 0
    z = dict(z, x2d=x2d, cam=cam.to(DEV))
    state, v, tfit = fit(z, conn, h0=0)
    keep = weighted(z, J)
    assert bool((v["idx"][:, 0][keep] == 3).all()) and bool((v["idx"][:, 0][~keep] == -1).all())
    err = (tfit[:, 0, 3].double().cpu() - torch.tensor(ROOT_TRUE, dtype=torch.float64)).abs().max()
    print(f"J = {J}: |tfit - planted root| = {float(err):.3g} m")
    assert err <= 1e-5
    m = ops.combine_poses(state.view(1, -1), (B, T, F, J), 5)
    wb3 = torch.from_numpy(whole_body(z["pred"][:, 0, 3], conn)).to(DEV)
    assert torch.equal(m["pick"][:, 0][keep], wb3[keep])


def test_zero_weight_joints_have_no_pick_and_no_say(cases):
    z, conn, state, v, tfit = cases[134, 5, 0]
    keep = weighted(z, 134)
    assert int((~keep).sum()) > 100
    none = ~keep[:, None].expand(B, T, F, 134)
    assert bool((v["idx"][none] == -1).all()) and bool(torch.isinf(v["e2"][none]).all()) and bool(torch.isnan(v["sel"][none]).all())
    x2d = z["x2d"].clone()
    x2d[~keep] = torch.tensor([float("nan"), 1e30], device=DEV)
    state2, _, tfit2 = fit(z, conn, 0, x2d=x2d)
    assert same_bits(tfit2, tfit) and same_bits(state2, state)


def test_a_frame_without_weights_has_no_fit_and_a_complete_sum():
    from pafuse_amd import ops
    J = 134
    z, conn = inputs(J, 5, seed=41)
    z["conf"][1, 2] = 0
    z["conf"][0, 1, 1:] = 0                                         # one weighted joint: no fit either
    _, v, tfit = fit(z, conn, 0)
    for b, f in ((1, 2), (0, 1)):
        assert bool((v["idx"][b, :, f] == -1).all()) and bool(torch.isnan(tfit[b, :, :, f]).all())
        assert bool(torch.isinf(v["e2"][b, :, f]).all()) and bool(torch.isnan(v["sel"][b, :, f]).all())
    assert not bool(torch.isnan(tfit[0, :, :, 0]).any()) and bool((v["idx"][0, :, 0, :2] >= 0).all())
    plain = ops.pose_views(ops.pose_partials(z["pred"], conn, 0), B, T, F, J)
    assert same_bits(v["sum"], plain["sum"])
    z["conf"][:] = 0                                                # nothing anywhere: still a state, and it combines
    state, v, tfit = fit(z, conn, 0)
    assert bool((v["idx"] == -1).all()) and bool(torch.isnan(tfit).all()) and same_bits(v["sum"], plain["sum"])
    m = ops.combine_poses(state.view(1, -1), (B, T, F, J), 5, no_pick_ok=True)
    assert bool(torch.isnan(m["pick"]).all()) and bool((m["idx"] == -1).all()) and not bool(torch.isnan(m["mean"]).any())


@pytest.mark.parametrize("J", [5, 134])
def test_no_conf_is_all_ones(J):
    z, conn = inputs(J, 5, seed=51, weights=False)
    state, _, tfit = fit(z, conn, 2)
    ones, _, tfit1 = fit(z, conn, 2, conf=torch.ones(B, F, J, device=DEV))
    assert same_bits(state, ones) and same_bits(tfit, tfit1) and not bool(torch.isnan(tfit).any())


def test_ties_go_to_the_lowest_hypothesis():
    J = 134
    z, conn = inputs(J, 5, seed=61)
    z["pred"][:, :, 2] = z["pred"][:, :, 1]
    z["pred"][:, :, 4] = z["pred"][:, :, 0]
    _, v, tfit = fit(z, conn, 3)
    keep = weighted(z, J)[:, None].expand(B, T, F, J)
    assert same_bits(tfit[:, :, 2], tfit[:, :, 1]) and same_bits(tfit[:, :, 4], tfit[:, :, 0])
    assert sorted(v["idx"][keep].unique().tolist()) == [3, 4, 6]     # 3 + {0, 1, 3}: never the later twin
    _, v, _ = fit(z, conn, 0, lo=1, hi=3)                            # the twins alone
    assert bool((v["idx"][keep] == 1).all())


def test_torch_op_is_the_ops_pair(cases):
    from pafuse_amd import ops, torch_ops  # noqa: F401
    z, conn, _, _, _ = cases[134, 5, 0]
    state, _, tfit = fit(z, conn, 0)
    want = ops.combine_poses(state.view(1, -1), (B, T, F, 134), 5)
    mean, pick, idx, roots = torch.ops.pafuse.aggregate_poses_fit(z["pred"], conn, z["x2d"], z["cam"], z["conf"])
    assert torch.equal(mean, want["mean"]) and same_bits(pick, want["pick"]) and torch.equal(idx, want["idx"])
    assert same_bits(roots, tfit)
    z1, conn1 = inputs(65, 1, seed=71, weights=False)
    state, _, tfit = fit(z1, conn1, 0)
    want = ops.combine_poses(state.view(1, -1), (B, T, F, 65), 1)
    mean, pick, idx, roots = torch.ops.pafuse.aggregate_poses_fit(z1["pred"], conn1, z1["x2d"], z1["cam"])
    assert torch.equal(mean, want["mean"]) and same_bits(pick, want["pick"]) and torch.equal(idx, want["idx"])
    assert same_bits(roots, tfit)


# ---------------------------------------------------------------------------------------------------- end to end
SEED, FRAMES = 3, 30


def e2e_inputs():
    """a 30-frame sequence (two overlapping 27-frame clips): 2-D input, weights with a fifth of the joints not found, intrinsics"""
    seq_2d, _, cam = sequence(FRAMES)
    g = torch.Generator().manual_seed(5)
    conf = torch.rand(FRAMES, 134, generator=g)
    conf[torch.rand(FRAMES, 134, generator=g) < 0.2] = 0
    return seq_2d, conf, cam


def infer(model, **kw):
    """one infer_sequence call from the start of noise stream (SEED, call 0)"""
    from pafuse_amd import harness
    seq_2d, conf, cam = e2e_inputs()
    model.noise, model.noise_seed = "device", SEED
    if kw.get("aggregate") == "reproj_fit":
        kw.update(cam=cam, conf=conf)
    return harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, **kw)


def test_infer_sequence_reproj_fit_is_the_ops_pair_on_its_hypotheses():
    from __graft_entry__ import make_model
    from pafuse_amd import harness, ops
    model = make_model(4, 1)[0]
    wb = infer(model)                                               # [clips, T, P, F, J, 3] whole-body, on the host
    assert tuple(wb.shape) == (2, 1, 4, 27, 134, 3) and bool((wb[..., 0, :] == 0).all())
    seq_2d, conf, cam = e2e_inputs()
    x2d = harness.cut_clips(seq_2d, 27).contiguous().to(DEV)
    cf = harness.cut_clips(conf.unsqueeze(-1), 27).squeeze(-1).contiguous().to(DEV)
    # with a connection table of zeros wb_joint adds joint 0, which a whole-body pose pins at 0: every joint goes through unchanged
    state = ops.pose_partials_fit(wb.to(DEV), torch.zeros(134, dtype=torch.int32, device=DEV), 0, x2d, cam.to(DEV), conf=cf)
    want = ops.combine_poses(state.view(1, -1), (2, 1, 27, 134), 4)
    none = want["idx"] < 0
    assert bool(none.any()) and bool((~none).any()) and torch.equal(none, ~(cf > 0)[:, None])
    want_pose = torch.where(none[..., None], want["mean"], want["pick"]).cpu()
    pose, idx = infer(model, aggregate="reproj_fit")
    assert not pose.is_cuda and torch.equal(idx, want["idx"].cpu()) and torch.equal(pose, want_pose)
    assert not bool(torch.isnan(pose).any())                        # a joint without a pick carries the mean
    assert torch.equal(pose[none.cpu()], want["mean"].cpu()[none.cpu()]) and len(idx.unique()) == 5
    pose2, idx2 = infer(model, aggregate="reproj_fit", hypothesis_chunk=2)
    assert torch.equal(idx2, idx) and same_bits(pose2, pose)
    out = infer(model, aggregate="reproj_fit", spread="std")
    assert torch.equal(out["pose"], pose) and torch.equal(out["idx"], idx) and tuple(out["std"].shape) == (2, 1, 27, 134)

"""The frame-level evaluation on the device: frame_errors_kernel / frame_errors_reduce_kernel (pafuse_frame_errors,
pafuse_frame_errors_reduce), ops.frame_errors, torch.ops.pafuse.frame_errors, evaluate.frame_metrics and
harness.evaluate_frames.

What is asserted and why it can be asserted:
  * kernel vs statement: the kernels and pafuse_amd/framemetrics.py perform the same IEEE fp64 operations in the same order (every
    fp32 input converted once, contraction off, a correctly rounded square root, every sum over the joints and over the frames in
    the pinned lane-then-butterfly order) -> the design goal is equal bits; the test accepts equal or ADJACENT fp64 values - the
    acceptance rule of tests/test_hip_rootfit.py, one level up - and prints how many differ.  Counts are integers -> torch.equal;
    a slot without a participant is 0.0 exactly.
  * closed forms (tests/test_frame_metrics_host.py): dyadic inputs, every operation exact -> ==.
  * against the existing evaluation: frame-level mpjpe / mpjpe_pb of the P-Agg mean pose against evaluate_accumulators_sharded's
    p_agg / p_agg_pb at rtol 1e-5: that side has fp32 per-joint expressions (~2e-7 relative) and an fp32 mean over 7 236 values
    (~log2(n) * 2^-24 ~ 8e-7) - about 1e-6, with a 10x margin.
  * p_mpjpe against the reference's (G23) at rtol 1e-6 + 1e-7 m, the tolerance tests/test_hip_procrustes.py uses against G21.
Shapes: J in {5, 64, 65, 134} - lanes without a joint, exactly one round, one joint in a second round, the real three ragged
rounds - and 300 for the round-by-round form; N in {1, 2, 3, 7, 70} - no neighbour, one neighbour, the first frame with all
three, a ragged last workgroup of waves, more frames than a reduce wave has lanes; T in {1, 2}; with and without traj.
"""
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden import golden_util as gu
from tests.test_frame_metrics_host import PARTS, closed_form_cases, tables
from tests.test_hip_partials import dataset, inputs, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(J, N, T) for J in (5, 64, 65, 134, 300) for N in (1, 2, 3, 7, 70) for T in (1, 2)]
PAD = 5


def planted(J, N, T, seed, nan_frame=True):
    """a pose 5 cm about its gt and a root 2 cm about its own; planted: one NaN joint (one component), one NaN part root, one
    NaN gt joint, one NaN traj row and (nan_frame) one frame entirely NaN"""
    g = torch.Generator().manual_seed(seed)
    pbroot, part = tables(J)
    gt = torch.randn(N, J, 3, generator=g) * 0.3
    gt[:, 0] = 0
    pose = gt[None] + torch.randn(T, N, J, 3, generator=g) * 0.05
    pose[:, :, 0] = 0
    root = torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    traj = root[None] + torch.randn(T, N, 3, generator=g) * 0.02
    pose[0, min(1, N - 1), min(3, J - 1), 1] = float("nan")
    pose[0, N // 2, int(pbroot[J - 1])] = float("nan")
    gt[N // 3, J - 1, 2] = float("nan")
    traj[0, N // 2, 2] = float("nan")
    if nan_frame:
        pose[T - 1, N - 1] = float("nan")
    z = {"pose": pose, "gt": gt, "traj": traj, "gt_root": root, "pbroot": torch.from_numpy(pbroot), "part": torch.from_numpy(part)}
    return {k: v.contiguous().to(DEV) for k, v in z.items()}


def statement(z, with_traj):
    from pafuse_amd import framemetrics as fm
    n = lambda k: z[k].cpu().numpy()
    err, cnt = fm.frame_errors(n("pose"), n("gt"), n("traj") if with_traj else None, n("gt_root") if with_traj else None,
                               n("pbroot"), n("part"), 4)
    sums, counts = fm.reduce(err, cnt)
    return {k: torch.from_numpy(v) for k, v in (("err", err), ("cnt", cnt), ("sums", sums), ("counts", counts))}


def check(z, case, with_traj, note=""):
    from pafuse_amd import framemetrics as fm
    from pafuse_amd import ops
    kw = dict(traj=z["traj"], gt_root=z["gt_root"]) if with_traj else {}
    got = {k: v.cpu() for k, v in ops.frame_errors(z["pose"], z["gt"], z["pbroot"], z["part"], 4, per_frame=True, **kw).items()}
    want = statement(z, with_traj)
    T, N = z["pose"].shape[:2]
    assert tuple(got["err"].shape) == tuple(got["cnt"].shape) == (T, N, 10) and tuple(got["sums"].shape) == tuple(got["counts"].shape) == (T, 10)
    assert got["err"].dtype == got["sums"].dtype == torch.float64 and got["cnt"].dtype == torch.int32 and got["counts"].dtype == torch.int64
    assert torch.equal(got["cnt"], want["cnt"]) and torch.equal(got["counts"], want["counts"])
    assert bool((got["err"][want["cnt"] == 0] == 0.0).all()) and bool((got["sums"][want["counts"] == 0] == 0.0).all())
    differ = {k: equal_or_adjacent(got[k], want[k]) for k in ("err", "sums")}
    # the reduce on its own: the statement's reduce of the kernel's own maps
    sums, counts = fm.reduce(got["err"].numpy(), got["cnt"].numpy())
    differ["reduce"] = equal_or_adjacent(got["sums"], torch.from_numpy(sums))
    assert torch.equal(got["counts"], torch.from_numpy(counts))
    print(f"(J, N, T) = {case}, traj {with_traj}{note}: values that differ from the statement (by one fp64 step): {differ} of "
          f"{got['err'].numel()} / {got['sums'].numel()} / {got['sums'].numel()}")
    if not with_traj:
        assert not bool(got["err"][..., 3:6].any()) and not bool(got["cnt"][..., 3:6].any())
    return got, want


@pytest.mark.parametrize("case", CASES)
def test_kernels_are_the_statement(case):
    J, N, T = case
    seed = 1000 + 11 * J + 5 * N + T
    z = planted(J, N, T, seed)
    for with_traj in (True, False):
        got, want = check(z, case, with_traj)
        assert not bool(want["cnt"][T - 1, N - 1, [0, 1, 2, 5, 6, 7, 8, 9]].any())        # the all-NaN frame
        if with_traj:
            assert int(want["cnt"][0, N // 2, 3]) == 0 and int(want["cnt"][0, N // 2, 5]) == 0   # the NaN traj row
    if T * N == 1:      # the only frame is the NaN frame: the arithmetic itself runs on the same inputs without it
        z = planted(J, N, T, seed, nan_frame=False)
        for with_traj in (True, False):
            got, want = check(z, case, with_traj, " without the NaN frame")
            assert int(want["cnt"][0, 0, 0]) > 0


@pytest.mark.parametrize("name", ["constant", "linear", "quadratic", "root"])
@pytest.mark.parametrize("J", [134, 300])
def test_closed_forms_are_exact_on_the_device(name, J):
    from pafuse_amd import ops
    pose, gt, traj, gt_root, want = closed_form_cases(N=6, J_=J)[name]
    pbroot, part = tables(J)
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    m = ops.frame_errors(d(pose), d(gt), d(pbroot), d(part), 4, traj=d(traj), gt_root=d(gt_root), per_frame=True)
    for k, v in want.items():
        s, c = m["sums"][:, k].cpu(), m["counts"][:, k].cpu()
        assert bool((c > 0).all()) and bool((s / c == v).all()), (name, k, (s / c).tolist(), v)
        e, n = m["err"][..., k].cpu(), m["cnt"][..., k].cpu()
        assert bool((e[n > 0] / n[n > 0] == v).all())


def raw(name, *args):
    from pafuse_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 7, 2), (65, 1, 1), (300, 3, 1)])
def test_canaries_and_the_torch_op(case):
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import ops
    J, N, T = case
    z = planted(J, N, T, seed=77)
    K, n = 10, T * N * 10
    err = torch.full((n + PAD,), 7.0, device=DEV, dtype=torch.float64)
    cnt = torch.full((n + PAD,), 7, device=DEV, dtype=torch.int32)
    sums = torch.full((T * K + PAD,), 7.0, device=DEV, dtype=torch.float64)
    counts = torch.full((T * K + PAD,), 7, device=DEV, dtype=torch.int64)
    assert raw("pafuse_frame_errors", z["pose"], z["gt"], z["traj"], z["gt_root"], z["pbroot"], z["part"], 4, T, N, J, err, cnt) == 0
    assert raw("pafuse_frame_errors_reduce", err, cnt, T, N, K, sums, counts) == 0
    want = ops.frame_errors(z["pose"], z["gt"], z["pbroot"], z["part"], 4, traj=z["traj"], gt_root=z["gt_root"], per_frame=True)
    for buf, k, m in ((err, "err", n), (cnt, "cnt", n), (sums, "sums", T * K), (counts, "counts", T * K)):
        assert bool((buf[m:] == 7).all()), k
        assert same_bits(buf[:m], want[k].reshape(-1)), k
    got = torch.ops.pafuse.frame_errors(z["pose"], z["gt"], z["pbroot"], z["part"], 4, z["traj"], z["gt_root"])
    assert all(same_bits(g, want[k]) for g, k in zip(got, ("sums", "counts", "err", "cnt")))
    plain = ops.frame_errors(z["pose"], z["gt"], z["pbroot"], z["part"], 4, traj=z["traj"], gt_root=z["gt_root"])
    assert set(plain) == {"sums", "counts"} and same_bits(plain["sums"], want["sums"])
    three = torch.ops.pafuse.frame_errors(z["pose"], z["gt"], z["pbroot"], z["part"], 3)       # K = 9: part 3 is dropped
    assert tuple(three[0].shape) == (T, 9) and same_bits(three[2][..., :3].contiguous(), want["err"][..., :3].contiguous())
    assert same_bits(three[2][..., 6:].contiguous(), want["err"][..., 6:9].contiguous())


def test_frame_level_mpjpe_is_the_clip_level_p_agg():
    """random hypotheses through the P-Agg mean pose and the frame-level evaluator against the same through the clip-level one"""
    from pafuse_amd import evaluate, harness
    B, T, P, F = 2, 2, 5, 27
    pred, gt_parts, x2d, traj, cam = inputs(B, T, P, F, seed=61, special=False)
    ds = dataset()
    mean = evaluate.aggregate_poses_sharded(pred, 0, P, ds)["mean"]                    # [B,T,F,J,3]
    pose = mean.permute(1, 0, 2, 3, 4).reshape(T, B * F, 134, 3).contiguous()
    gt_wb = harness.wb_pose_from_parts(gt_parts, ds).reshape(B * F, 134, 3)
    m = evaluate.frame_metrics(pose, gt_wb, ds)
    assert set(m) == {"mpjpe", "mpjve", "accel", "mpjpe_pb"} | {"mpjpe_pb_" + p for p in PARTS}
    acc = evaluate.evaluate_accumulators_sharded(pred, 0, P, gt_parts, x2d, traj, cam, ds)
    for mine, theirs in [("mpjpe", "p_agg"), ("mpjpe_pb", "p_agg_pb")] + [("mpjpe_pb_" + p, "p_agg_pb_" + p) for p in PARTS]:
        s, c = m[mine]
        got, want = (s / c).cpu(), acc[theirs].double().cpu()
        print(f"{mine} {got.tolist()} vs {theirs} {want.tolist()}: rel {float(((got - want).abs() / want).max()):.2g}")
        assert s.dtype == torch.float64 and c.dtype == torch.int64 and tuple(s.shape) == (T,)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=0)
    assert bool((m["mpjpe"][1] == B * F * 134).all()) and bool((m["mpjpe_pb"][1] == B * F * 134).all())


def test_p_mpjpe_is_the_references():
    from pafuse_amd import evaluate
    z = np.load(os.path.join(ROOT, "tests", "golden", "g23_frame_metrics.npz"))
    pose, gt = torch.from_numpy(z["pose"]).to(DEV), torch.from_numpy(z["gt"]).to(DEV)
    T, N = pose.shape[:2]
    ds = dataset()
    m = evaluate.frame_metrics(pose, gt, ds, p2=True)
    s, c = m["p_mpjpe"]
    got = (s / c).cpu().numpy()
    print(f"p_mpjpe {got.tolist()} reference {z['p_mpjpe'].tolist()}")
    assert bool((c == N).all())
    np.testing.assert_allclose(got, z["p_mpjpe"], rtol=1e-6, atol=1e-7)
    for k in ("mpjpe", "mpjve", "accel", "mpjpe_pb"):                                   # and the device agrees with G23 elsewhere too
        np.testing.assert_allclose((m[k][0] / m[k][1]).cpu().numpy(), z[k], rtol=1e-12, atol=0)
    # a frame with a NaN joint is left out and counted out; the other frames' aligned errors are what they were
    hurt = pose.clone()
    hurt[0, 4, 77, 0] = float("nan")
    h = evaluate.frame_metrics(hurt, gt, ds, p2=True)
    assert h["p_mpjpe"][1].tolist() == [N - 1, N] and bool(torch.isfinite(h["p_mpjpe"][0]).all())
    assert same_bits(h["p_mpjpe"][0][1:], s[1:])
    rest = torch.ones(N, dtype=torch.bool)
    rest[4] = False
    only = evaluate.frame_metrics(pose[:, rest].contiguous(), gt[rest].contiguous(), ds, p2=True)["p_mpjpe"]
    torch.testing.assert_close(h["p_mpjpe"][0][0], only[0][0], rtol=1e-14, atol=0)     # the same frames, summed in another grouping


# ------------------------------------------------------------------------------------------------------------ end to end
SEED = 2468
F27 = 27
N_VIDEO = 2 * F27 + 5


def test_evaluate_frames_end_to_end_and_infer_sequence_is_unchanged():
    from __graft_entry__ import make_model
    from pafuse_amd import evaluate, harness
    model = make_model(5, 2, depth=2)[0]
    ds = dataset()
    seq_2d, seq_3d, cam = sequence(N_VIDEO)
    kw = dict(batch_size=2, aggregate="mean", stride=9, cam=cam, trajectory=3)

    def infer():
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED            # setting the seed restarts the call index
        return harness.infer_sequence(model, ds, seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, **kw)

    before = infer()
    model.noise_seed = SEED
    sums, counts, maps = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                                                 aggregate="mean", stride=9, trajectory=3, per_frame=True, p2=True)
    after = infer()
    assert set(before) == set(after) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"}
    for k in before:
        assert same_bits(before[k], after[k]), k
    names = evaluate.frame_metric_names(ds)
    assert maps["names"] == names and set(sums) == set(counts) == set(names) | {"mpjpe_pb", "p_mpjpe"}
    T = before["pose"].shape[0]
    for k in sums:
        assert not sums[k].is_cuda and sums[k].dtype == torch.float64 and counts[k].dtype == torch.int64 and tuple(sums[k].shape) == (T,)
        assert bool(torch.isfinite(sums[k]).all()), k
    assert counts["mpjpe"].tolist() == [N_VIDEO * 134] * T and counts["abs_mpjpe"].tolist() == [N_VIDEO * 134] * T
    assert counts["mpjve"].tolist() == [(N_VIDEO - 1) * 134] * T and counts["accel"].tolist() == [(N_VIDEO - 2) * 134] * T
    assert counts["root"].tolist() == [N_VIDEO] * T and counts["p_mpjpe"].tolist() == [N_VIDEO] * T
    assert tuple(maps["err"].shape) == tuple(maps["cnt"].shape) == (T, N_VIDEO, len(names))
    # it scored the pose and the root infer_sequence returns
    gt_root = seq_3d[:, 0].contiguous()
    m = evaluate.frame_metrics(before["pose"].to(DEV), (seq_3d - seq_3d[:, :1]).to(DEV), ds, traj=before["traj"].to(DEV), gt_root=gt_root.to(DEV))
    for k in m:
        assert same_bits(m[k][0].cpu(), sums[k]) and torch.equal(m[k][1].cpu(), counts[k]), k
    rep = harness.frame_report(sums, counts)
    lines = harness.format_frame_report(rep)
    assert len(lines) == 2 + T * len(sums) and all(np.isfinite(v).all() for v in rep.values())
    prof = harness.seam_profile(maps["err"], maps["cnt"], F27)
    assert tuple(prof.shape) == (T, F27) and bool(torch.isfinite(prof).all())
    # stride=None is the clips laid end to end, and "reproj" takes its root from the ground truth
    model.noise_seed = SEED
    s0, c0 = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT)
    model.noise_seed = SEED
    s1, c1 = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, stride=F27)
    assert "root" not in s0 and all(same_bits(s0[k], s1[k]) and torch.equal(c0[k], c1[k]) for k in s0)
    s2, c2 = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="reproj", stride=9)
    assert bool(torch.isfinite(s2["mpjpe"]).all()) and bool((c2["mpjpe"] > 0).all())


# ------------------------------------------------------------------------------- the whole chain against its own parts
N_CHAIN, STRIDE_CHAIN = 2 * F27 + 1, 26     # windows at 0, 26 and a last one at N - F = 28 that lies almost wholly over its predecessor


def chain_video(seed=97):
    """-> (seq_2d [N,J,2], seq_3d, conf [N,J], cam): a person drifting across the screen with a little detector noise, a few gross
    outliers for the screen and a few lost detections (confidence 0) for the repair"""
    g = torch.Generator().manual_seed(seed)
    _, seq_3d, cam = sequence(N_CHAIN)
    t = torch.arange(N_CHAIN, dtype=torch.float32)[:, None, None]
    seq_2d = (torch.rand(1, 134, 2, generator=g) - 0.5) + t * 0.004 * (torch.rand(1, 134, 2, generator=g) - 0.5)
    seq_2d = seq_2d + torch.randn(N_CHAIN, 134, 2, generator=g) * 0.002
    conf = torch.rand(N_CHAIN, 134, generator=g) * 0.5 + 0.5
    for n, j in ((4, 7), (20, 100), (30, 16), (N_CHAIN - 2, 50)):
        seq_2d[n, j] += 0.3
    for n, j in ((0, 3), (10, 22), (11, 22), (26, 40), (27, 40), (N_CHAIN - 1, 120)):
        seq_2d[n, j], conf[n, j] = 0.0, 0.0
    return seq_2d.contiguous(), seq_3d, conf.contiguous(), cam


def test_the_whole_chain_in_one_call_is_its_stages_one_by_one_and_evaluate_frames_names_its_dicts():
    """infer_sequence with every stage on against the stand-alone stages run in the chain's order from the same start of the noise
    stream: screen, repair, the lift with its spread, pose smoothing, bones, the trajectory with the focal estimate, the ground -
    every key the same bits.  Then evaluate_frames' tail of optional dicts: its order, told by the key sets, and the named
    internal result under its names."""
    from __graft_entry__ import make_model
    from pafuse_amd import h3wb, harness
    model = make_model(5, 2, depth=2)[0]
    ds = dataset()
    left, right = gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT
    seq_2d, seq_3d, conf, cam = chain_video()

    def restart():
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED            # setting the seed restarts the call index

    restart()
    whole = harness.infer_sequence(model, ds, seq_2d, left, right, batch_size=2, aggregate="reproj_fit", spread="cov", stride=STRIDE_CHAIN,
                                   cam=cam, conf=conf, screen=3, repair=3, pose_smooth=2, bone_lengths="symmetric", trajectory=3,
                                   focal="estimate", ground=True)
    restart()
    screened = harness.screen_detections(seq_2d, conf, left, right, radius=3)
    fixed = harness.repair_detections(screened["x2d"], screened["conf"], dataset=ds, radius=3)
    lifted = harness.infer_sequence(model, ds, fixed["x2d"], left, right, batch_size=2, aggregate="reproj_fit", spread="cov",
                                    stride=STRIDE_CHAIN, cam=cam, conf=fixed["conf"])
    smoothed = harness.smooth_poses(lifted["pose"], lifted["cov"], radius=2)
    held = harness.constrain_bones(smoothed["pose"], lifted["cov"], tables=h3wb.bone_tables(ds, True, left, right), lengths="symmetric")
    rooted = harness.fit_trajectory(held["pose"], fixed["x2d"], cam=cam, conf=fixed["conf"], smooth=3, focal="estimate")
    ground = harness.estimate_ground(held["pose"], rooted["traj"], radius=3)
    parts = {"screened": screened["status"], "repaired": fixed["status"],
             **{k: lifted[k] for k in ("count", "idx", "window", "std", "cov")},
             "pose_raw": lifted["pose"], "pose_smooth_code": smoothed["pose_smooth_code"], "pose_free": smoothed["pose"],
             **{k: held[k] for k in ("pose", "bone_length", "bone_dev", "bone_frames", "bone_code", "bone_resid")},
             **rooted, **ground}
    assert set(lifted) == {"pose", "count", "idx", "window", "std", "cov"} and set(ground) == set(harness.GROUND_KEYS)
    assert set(rooted) == {"traj", "traj_raw", "traj_weight", "traj_resid", "focal", "focal_r2", "focal_frames", "cam"}
    assert set(whole) == set(parts)
    for k in sorted(whole):
        assert not whole[k].is_cuda and same_bits(whole[k], parts[k]), k
    assert same_bits(smoothed["pose_raw"], lifted["pose"]) and same_bits(held["pose_free"], smoothed["pose"])
    # the shapes did their work: frames pooled from two windows (0, 26 and the last one at N - F = 28, in two batches), something
    # rejected, something filled, a pose all the way through
    P = model.num_proposals
    assert whole["count"][25:29].tolist() == [P, 2 * P, P, 2 * P] and whole["count"][52:].tolist() == [2 * P, P, P]
    assert bool((whole["screened"] == 1).any()) and bool((whole["repaired"] == 1).any())
    assert tuple(whole["pose_world"].shape) == (2, N_CHAIN, 134, 3) and bool(torch.isfinite(whole["pose"]).all())

    options = dict(stride=STRIDE_CHAIN, trajectory=3, focal="estimate", bone_lengths="video", ground=True,
                   drop=(0.1, 3, 0), repair=3)
    keys = [{"focal", "focal_r2", "focal_frames", "cam"}, {"x2d", "conf", "lost", "status"},
            {"bone_length", "bone_length_gt", "bone_dev_free", "bone_dev"}, set(harness.GROUND_KEYS)]
    restart()
    public = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, left, right, **options)
    assert isinstance(public, tuple) and len(public) == 2 + 4
    assert [set(d) for d in public[2:]] == keys                                         # estimate, seen, held, found
    assert set(public[0]) == set(public[1]) and "abs_mpjpe" in public[0]
    restart()
    named = harness._evaluate_frames(model, ds, seq_2d, seq_3d, cam, left, right, **options)
    assert named.maps is None
    for got, want in zip(public, (named.sums, named.counts, named.estimate, named.seen, named.held, named.found)):
        assert set(got) == set(want) and all(same_bits(got[k], want[k]) for k in got)

"""The aggregates as poses: pose_partials_kernel / pose_combine_kernel (pafuse_pose_partials, pafuse_pose_combine),
torch.ops.pafuse.aggregate_poses, evaluate.accumulate_poses / aggregate_poses_sharded and infer_sequence(aggregate=...).

What is asserted and why it can be asserted:
  * J-Agg index and pose: a first minimum does not depend on the order or grouping of its operands, and e2 is
    metrics_kernel's fp32 expression -> idx is torch.equal to pafuse_procrustes_errors' pick and to the index in
    pafuse_hypothesis_partials' state, for every split; the pose is a copy of the winner's whole-body joint -> torch.equal
    to a gather of harness.wb_pose_from_parts at idx.
  * P-Agg mean: fp64 sums of fp32 values in a stated order, one fp64 divide, one rounding to fp32 - every step is an
    IEEE operation torch performs identically on the host -> torch.equal to the host statement of the SAME grouping.
    Two groupings of the same <= 5 values differ by a few fp64 roundings (relative 2^-52), which can move the fp32
    result only when the quotient sits on a rounding boundary, and then by one step: |d| <= |nextafter(x, inf) - x|.
Shapes: B=2, T=2, P=5, F=3, J=134 (1 608 elements: six full 256-thread blocks and a ragged seventh) and B=T=P=F=1 (134
elements, less than one block).
"""
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT
from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, sequence, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG, SMALL = (2, 2, 5, 3), (1, 1, 1, 1)
J = 134


def inputs(B, T, P, F, seed):
    """pred = 0.25 randn, part-centred; x2d uniform in the normalised image; traj with z = 4 (no projected depth near 0);
    a random part-centred target for the evaluation entries the picks are compared with"""
    from pafuse_amd import harness
    g = torch.Generator().manual_seed(seed)
    pred = harness.center_pose_parts(torch.randn(B, T, P, F, J, 3, generator=g) * 0.25, dataset())
    gt = harness.center_pose_parts(torch.randn(B, F, J, 3, generator=g) * 0.25, dataset())
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    traj = torch.randn(B, F, 3, generator=g) * 0.1
    traj[..., 2] = 4.0
    cam = sequence(1)[2]
    return {k: v.contiguous().to(DEV) for k, v in (("pred", pred), ("gt", gt), ("x2d", x2d), ("traj", traj), ("cam", cam))}


def whole_body(pred):
    from pafuse_amd import harness
    return harness.wb_pose_from_parts(pred.cpu(), dataset())


def cuts_of(P, sizes):
    out, lo = [], 0
    for s in sizes:
        out.append((lo, lo + s))
        lo += s
    assert lo == P
    return out


def aggregate(z, sizes, running=False, reproj=True, want=("mean", "pick", "idx")):
    """the P hypotheses cut into shards of `sizes`: one state per shard combined in one call, or (running=True) folded chunk
    after chunk into a running state merged in place"""
    from pafuse_amd import ops
    pred = z["pred"]
    B, T, P, F = pred.shape[:4]
    conn = tables()[0]
    extra = (z["x2d"], z["traj"], z["cam"]) if reproj else ()
    L = ops.pose_partials_bytes(B, T, F, J) // 8
    cuts = cuts_of(P, sizes)
    if not running:
        states = torch.full((len(cuts), L + 3), float("nan"), device=DEV, dtype=torch.float64)     # padded rows
        for r, (lo, hi) in enumerate(cuts):
            ops.pose_partials(pred[:, :, lo:hi].contiguous(), conn, lo, *extra, out=states[r])
        return ops.combine_poses(states, (B, T, F, J), P, want=want)
    slots = torch.full((2, L), float("nan"), device=DEV, dtype=torch.float64)
    for r, (lo, hi) in enumerate(cuts):
        ops.pose_partials(pred[:, :, lo:hi].contiguous(), conn, lo, *extra, out=slots[0 if r == 0 else 1])
        if r:
            ops.combine_poses(slots, (B, T, F, J), 1, merged=slots[0], want=())
    return ops.combine_poses(slots[:1], (B, T, F, J), P, want=want)


def host_mean(wb, sizes):
    """the host statement: every shard summed in fp64 in h order, the shard sums added in shard order, one fp64 divide,
    one rounding"""
    P = wb.shape[2]
    total = torch.zeros(wb[:, :, 0].shape, dtype=torch.float64)
    for lo, hi in cuts_of(P, sizes):
        s = torch.zeros_like(total)
        for h in range(lo, hi):
            s += wb[:, :, h].double()
        total += s
    return (total / P).float()


def equal_or_adjacent(a, b):
    step = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).abs()
    return bool(((a - b).abs() <= step).all())


SPLITS = {"one": (5,), "3+2": (3, 2), "ones": (1, 1, 1, 1, 1)}


@pytest.fixture(scope="module")
def big():
    """inputs, their whole-body poses on the host, and the aggregates of every split (computed once, never modified)"""
    z = inputs(*BIG, seed=11)
    got = {k: aggregate(z, s) for k, s in SPLITS.items()}
    got["running"] = aggregate(z, (2, 2, 1), running=True)
    return z, whole_body(z["pred"]), got


@pytest.fixture(scope="module")
def small():
    z = inputs(*SMALL, seed=12)
    return z, whole_body(z["pred"]), aggregate(z, (1,))


def gather_at(wb, idx):
    B, T, P, F = wb.shape[:4]
    at = idx.cpu().long()[:, :, None, :, :, None].expand(B, T, 1, F, J, 3)
    return torch.gather(wb, 2, at).squeeze(2)


@pytest.mark.parametrize("which", ["big", "small"])
def test_pick_is_the_evaluation_kernels_pick_and_a_gather(big, small, which):
    from pafuse_amd import ops
    z, wb, got = (big[0], big[1], big[2]["one"]) if which == "big" else small
    B, T, P, F = z["pred"].shape[:4]
    conn, pbroot, part = tables()
    idx = got["idx"]
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, T, F, J) and tuple(got["pick"].shape) == (B, T, F, J, 3)
    assert int(idx.min()) >= 0 and int(idx.max()) < P
    pick = ops.procrustes_errors(z["pred"], z["gt"], z["x2d"], z["traj"], z["cam"], conn, pick=True)["pick"]
    assert torch.equal(idx, pick)
    st = ops.hypothesis_partials(z["pred"], z["gt"], z["x2d"], z["traj"], z["cam"], conn, pbroot, part, 4, 0)
    assert torch.equal(idx, ops.partials_views(st, B, T, P, F, J, 4)["idx"])
    assert torch.equal(got["pick"].cpu(), gather_at(wb, idx))
    if which == "big":
        assert len(idx.unique()) == P                      # every hypothesis wins somewhere: the comparison is not vacuous


def test_mean_is_its_host_statement(big, small):
    z, wb, got = big
    for k, sizes in SPLITS.items():
        assert torch.equal(got[k]["mean"].cpu(), host_mean(wb, sizes)), k
    assert torch.equal(got["running"]["mean"].cpu(), host_mean(wb, (2, 2, 1)))
    for k in ("3+2", "ones", "running"):
        assert equal_or_adjacent(got[k]["mean"], got["one"]["mean"]), k
    z1, wb1, got1 = small
    assert torch.equal(got1["mean"].cpu(), host_mean(wb1, (1,))) and torch.equal(got1["mean"].cpu(), wb1[:, :, 0])
    assert (got["one"]["mean"][..., 0, :] == 0).all()      # joint 0 is pinned at the origin


def test_pick_does_not_depend_on_the_split(big):
    _, _, got = big
    for k in ("3+2", "ones", "running"):
        assert torch.equal(got[k]["idx"], got["one"]["idx"]), k
        assert torch.equal(got[k]["pick"], got["one"]["pick"]), k


def test_ties_go_to_the_lowest_hypothesis():
    z = inputs(*BIG, seed=13)
    z["pred"][:, :, 3] = z["pred"][:, :, 1]
    one = aggregate(z, (5,))
    assert (one["idx"] == 1).any() and not (one["idx"] == 3).any()
    for sizes in ((2, 3), (3, 2), (1, 1, 1, 1, 1)):        # hypotheses 1 and 3 in different shards
        got = aggregate(z, sizes)
        assert not (got["idx"] == 3).any()
        assert torch.equal(got["idx"], one["idx"]) and torch.equal(got["pick"], one["pick"])
    got = aggregate(z, (2, 2, 1), running=True)
    assert torch.equal(got["idx"], one["idx"]) and torch.equal(got["pick"], one["pick"])


def test_a_joint_without_a_finite_reprojection_error_has_no_pick(big):
    z, _, got = big
    clean = got["one"]
    b, f, j = 1, 2, 77
    bad = dict(z, x2d=z["x2d"].clone())
    bad["x2d"][b, f, j, 0] = float("nan")
    hit = torch.zeros(BIG[0], BIG[1], BIG[3], J, dtype=torch.bool, device=DEV)
    hit[b, :, f, j] = True
    for sizes in ((5,), (3, 2)):
        out = aggregate(bad, sizes)
        assert (out["idx"][hit] == -1).all() and torch.isnan(out["pick"][hit]).all()
        assert torch.equal(out["idx"][~hit], clean["idx"][~hit]) and torch.equal(out["pick"][~hit], clean["pick"][~hit])
        assert torch.equal(out["mean"], got["one" if sizes == (5,) else "3+2"]["mean"])


def test_mean_only_mode_and_edge_cases(big):
    from pafuse_amd import _lib, ops
    z, wb, got = big
    B, T, P, F = BIG
    conn = tables()[0]
    for sizes in ((5,), (3, 2)):
        out = aggregate(z, sizes, reproj=False, want=("mean",))
        assert set(out) == {"mean"} and torch.equal(out["mean"].cpu(), host_mean(wb, sizes))
    state = ops.pose_partials(z["pred"], conn, 0)
    v = ops.pose_views(state, B, T, F, J)
    assert (v["idx"] == -1).all() and (v["e2"] == float("inf")).all() and torch.isnan(v["sel"]).all()
    for want in (("pick",), ("idx",), ("mean", "pick", "idx")):
        with pytest.raises(_lib.PafuseError):
            ops.combine_poses(state.view(1, -1), (B, T, F, J), P, want=want)
    for some in ({"x2d": z["x2d"]}, {"traj": z["traj"], "cam": z["cam"]}, {"x2d": z["x2d"], "traj": z["traj"]}):
        with pytest.raises(_lib.PafuseError):
            ops.pose_partials(z["pred"], conn, 0, **some)
    # an empty shard: the neutral state, written over whatever the buffer held, and it leaves a combination unchanged
    L = ops.pose_partials_bytes(B, T, F, J) // 8
    buf = torch.full((L,), 7.0, device=DEV, dtype=torch.float64)
    empty = ops.pose_partials(z["pred"][:, :, :0].contiguous(), conn, 5, z["x2d"], z["traj"], z["cam"], out=buf)
    v = ops.pose_views(empty, B, T, F, J)
    assert (v["sum"] == 0).all() and (v["e2"] == float("inf")).all() and (v["idx"] == -1).all() and torch.isnan(v["sel"]).all()
    full = ops.pose_partials(z["pred"], conn, 0, z["x2d"], z["traj"], z["cam"])
    for order in ((empty, full), (full, empty), (empty, full, empty)):
        out = ops.combine_poses(torch.stack(order), (B, T, F, J), P)
        for k in ("mean", "pick", "idx"):
            assert torch.equal(out[k], got["one"][k]), k
    with pytest.raises(ValueError):                       # a merged state over an operand other than the first
        two = torch.stack((full, empty))
        ops.combine_poses(two, (B, T, F, J), P, merged=two[1])
    with pytest.raises(ValueError):
        ops.pose_partials(z["pred"], conn, -1)
    with pytest.raises(ValueError):
        ops.pose_partials(z["pred"], conn, 0, out=torch.empty(3, device=DEV, dtype=torch.float64))
    # an odd element count (44 * 5 = 220 bytes, padded to 224) with a connection table of its own
    g = torch.Generator().manual_seed(5)
    pose = torch.randn(1, 1, 3, 1, 5, 3, generator=g)
    c5 = torch.tensor([0, 0, 1, 1, 2], dtype=torch.int32)
    w5 = pose + pose[..., c5.long(), :]
    w5[..., 0, :] = 0
    assert ops.pose_partials_bytes(1, 1, 1, 5) == 224
    s5 = ops.pose_partials(pose.to(DEV), c5.to(DEV), 0)
    m5 = ops.combine_poses(s5.view(1, -1), (1, 1, 1, 5), 3, want=("mean",))["mean"]
    assert torch.equal(m5.cpu(), host_mean(w5, (3,)))


def test_torch_op_is_the_ops_pair(big):
    from pafuse_amd import torch_ops  # noqa: F401
    z, wb, got = big
    conn = tables()[0]
    mean, pick, idx = torch.ops.pafuse.aggregate_poses(z["pred"], conn, z["x2d"], z["traj"], z["cam"])
    assert torch.equal(mean, got["one"]["mean"]) and torch.equal(pick, got["one"]["pick"]) and torch.equal(idx, got["one"]["idx"])
    mean, pick, idx = torch.ops.pafuse.aggregate_poses(z["pred"], conn)
    assert torch.equal(mean, got["one"]["mean"]) and torch.isnan(pick).all() and (idx == -1).all()
    s = str(torch.ops.pafuse.aggregate_poses.default._schema)
    assert "Tensor? x2d=None, Tensor? traj=None, Tensor? cam=None" in s and s.endswith("-> Tensor[]")


def test_every_picking_kernel_agrees_on_one_hostile_input():
    """One input (tools/eval_bits.hostile_inputs: an exact tie across the shard border, Z = 0, a projection that clamps in
    every hypothesis, a NaN detection) through the six paths that form the J-Agg index; they all call reproj_error and
    candidate_wins, so the indices are torch.equal.  B=1, T=2, P=6 cut 4+2, F=2, J=134: F*J = 268 > 256 (partials_kernel runs
    two blocks per (b, t)), 128 < J <= 256 (three rounds in the wave kernels, within Protocol #2's limit)."""
    from pafuse_amd import ops
    from tests.test_hip_partials import unsharded
    from tools.eval_bits import HOSTILE, hostile_inputs
    z = hostile_inputs(DEV)
    pred, gt, x2d, traj, cam = (z[k] for k in ("pred", "gt", "x2d", "traj", "cam"))
    (B, T, P, F), sizes = HOSTILE["shape"], HOSTILE["cut"]
    shape, cuts = (B, T, F, J), cuts_of(P, sizes)
    conn, pbroot, part = tables()
    shard = lambda lo, hi: pred[:, :, lo:hi].contiguous()
    picks = {"procrustes_errors": ops.procrustes_errors(pred, gt, x2d, traj, cam, conn, pick=True)["pick"],
             "pose_partials": aggregate(z, sizes, want=("idx",))["idx"]}
    p1 = torch.zeros(len(cuts), ops.partials_bytes(B, T, max(sizes), F, J, 4) // 8, device=DEV, dtype=torch.float64)
    p2 = torch.zeros(len(cuts), ops.procrustes_partials_bytes(B, T, max(sizes), F, J) // 8, device=DEV, dtype=torch.float64)
    fit = torch.zeros(len(cuts), ops.pose_partials_bytes(B, T, F, J) // 8, device=DEV, dtype=torch.float64)
    ones, tfit = torch.ones(B, F, J, device=DEV), []
    for r, (lo, hi) in enumerate(cuts):
        ops.hypothesis_partials(shard(lo, hi), gt, x2d, traj, cam, conn, pbroot, part, 4, lo, out=p1[r])
        ops.procrustes_partials(shard(lo, hi), gt, x2d, traj, cam, conn, lo, out=p2[r])
        tfit.append(torch.full((B, T, hi - lo, F, 3), 7.0, device=DEV))
        ops.pose_partials_fit(shard(lo, hi), conn, lo, x2d, cam, conf=ones, out=fit[r], tfit=tfit[-1])
    merged = torch.empty(5 * B * T * F * J, device=DEV, dtype=torch.float64)
    ops.combine_partials(p1, gt, conn, pbroot, shape, P, merged=merged, maps=False)
    picks["hypothesis_partials"] = ops.partials_views(merged, B, T, 0, F, J, 4)["idx"]
    picks["procrustes_partials"] = ops.combine_procrustes(p2, shape, P, want=("pick",))["pick"]
    want = picks["procrustes_errors"]
    for k, got in picks.items():
        assert got.dtype == torch.int32 and torch.equal(got, want), k
    # what was planted is there: the tie goes to the lower hypothesis, equal clamped errors to the first, NaN to nobody
    (lo, hi), (f, j) = HOSTILE["tie"], HOSTILE["nan"]
    assert (want == lo).any() and not (want == hi).any() and (want[..., HOSTILE["clamped"]] == 0).all()
    assert (want[:, :, f, j] == -1).all() and int((want < 0).sum()) == B * T
    # pafuse_hypothesis_errors keeps no index: its jagg is its e3 at that pick (0 where there is none)
    old, valid = unsharded(pred, gt, x2d, traj, cam), want >= 0
    at_pick = old["e3"].gather(2, want.clamp(min=0).long().unsqueeze(2)).squeeze(2)
    assert torch.equal(at_pick[valid], old["jagg"][valid]) and (old["jagg"][~valid] == 0).all()
    # pose_partials_fit: the pick of pose_partials_kernel on the roots it fitted, one hypothesis at a time
    tfit = torch.cat(tfit, dim=2)
    got = ops.combine_poses(fit, shape, P, want=("idx",), no_pick_ok=True)["idx"]
    x2d_bt = x2d[:, None].expand(B, T, F, J, 2).reshape(B * T, F, J, 2).contiguous()
    best = torch.full(shape, float("inf"), device=DEV)
    idx = torch.full(shape, -1, device=DEV, dtype=torch.int32)
    for h in range(P):
        one = pred[:, :, h].reshape(B * T, 1, 1, F, J, 3).contiguous()
        s = ops.pose_views(ops.pose_partials(one, conn, h, x2d_bt, tfit[:, :, h].reshape(B * T, F, 3).contiguous(), cam), B * T, 1, F, J)
        fitted = ~torch.isnan(tfit[:, :, h]).any(dim=-1)
        better = (s["e2"].view(shape) < best) & fitted[..., None]       # strict: the first minimum wins
        best, idx = torch.where(better, s["e2"].view(shape), best), torch.where(better, s["idx"].view(shape), idx)
    assert torch.equal(got, idx)
    assert (got[:, :, 1 - f] >= 0).all() and (got[:, :, f] == -1).all() and not (got == hi).any()    # the NaN detection leaves frame f without a fit


# ---------------------------------------------------------------------------------------------------- end to end
SEED, FRAMES = 3, 30


def e2e_inputs():
    """a 30-frame sequence (two overlapping 27-frame clips): 2-D input, root trajectory (z near 4), intrinsics"""
    seq_2d, seq_3d, cam = sequence(FRAMES)
    return seq_2d, seq_3d[:, 0].contiguous(), cam


def infer(model, **kw):
    """one infer_sequence call from the start of noise stream (SEED, call 0)"""
    from pafuse_amd import harness
    seq_2d, traj, cam = e2e_inputs()
    model.noise, model.noise_seed = "device", SEED
    if kw.get("aggregate") == "reproj":
        kw.update(cam=cam, traj=traj)
    return harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, **kw)


def aggregates_of_whole_body(wb, sizes=(5,)):
    """the ops pair on the WHOLE-BODY hypotheses infer_sequence(aggregate=None) returns: with a connection table of zeros
    wb_joint adds joint 0, which a whole-body pose pins at 0, so every joint goes through unchanged"""
    from pafuse_amd import harness, ops
    seq_2d, traj, cam = e2e_inputs()
    x2d = harness.cut_clips(seq_2d, 27).contiguous().to(DEV)
    tr = harness.cut_clips(traj.unsqueeze(1), 27).squeeze(2).contiguous().to(DEV)
    assert (wb[..., 0, :] == 0).all()
    B, T, P, F = wb.shape[:4]
    conn = torch.zeros(J, dtype=torch.int32, device=DEV)
    states = torch.stack([ops.pose_partials(wb[:, :, lo:hi].contiguous().to(DEV), conn, lo, x2d, tr, cam.to(DEV))
                          for lo, hi in cuts_of(P, sizes)])
    return ops.combine_poses(states, (B, T, F, J), P)


@pytest.fixture(scope="module")
def model():
    from __graft_entry__ import make_model
    return make_model(5, 2, depth=2)[0]


@pytest.fixture(scope="module")
def hypotheses(model):
    wb = infer(model)
    assert tuple(wb.shape) == (2, 2, 5, 27, J, 3) and not wb.is_cuda
    return wb, aggregates_of_whole_body(wb)


def test_infer_sequence_returns_the_aggregates_of_its_hypotheses(model, hypotheses):
    wb, want = hypotheses
    mean = infer(model, aggregate="mean")
    assert not mean.is_cuda and torch.equal(mean, want["mean"].cpu())
    assert torch.equal(mean, host_mean(wb, (5,)))
    pose, idx = infer(model, aggregate="reproj")
    assert not pose.is_cuda and torch.equal(pose, want["pick"].cpu()) and torch.equal(idx, want["idx"].cpu())
    assert torch.equal(pose, gather_at(wb, idx)) and len(idx.unique()) == 5
    assert torch.equal(infer(model), wb)                   # the default call did not change and is repeatable
    # hypotheses sampled and reduced two at a time
    pose2, idx2 = infer(model, aggregate="reproj", hypothesis_chunk=2)
    assert torch.equal(idx2, idx) and torch.equal(pose2, pose)
    mean2 = infer(model, aggregate="mean", hypothesis_chunk=2)
    assert torch.equal(mean2, host_mean(wb, (2, 2, 1))) and equal_or_adjacent(mean2, mean)


def test_chunked_inference_never_holds_all_hypotheses(model, hypotheses):
    """hypothesis_chunk=1 against the default call, both warm: the peak allocation above the resident set is lower by at
    least the [B,T,P,F,J,3] tensor minus one chunk of it"""
    wb, _ = hypotheses
    full_bytes = wb.numel() * 4
    chunk_bytes = full_bytes // wb.shape[2]
    peaks = {}
    for name, kw in (("all", {}), ("chunked", {"aggregate": "mean", "hypothesis_chunk": 1})):
        infer(model, **kw)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = infer(model, **kw)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        del out
    print(f"peak above the resident set: all hypotheses {peaks['all'] / 1e6:.2f} MB, chunks of 1 {peaks['chunked'] / 1e6:.2f} MB; "
          f"the full tensor {full_bytes / 1e6:.2f} MB, one chunk {chunk_bytes / 1e6:.2f} MB")
    assert peaks["all"] - peaks["chunked"] >= full_bytes - chunk_bytes, peaks


def test_two_rank_pose_aggregation_on_one_gpu(tmp_path, model, hypotheses):
    """Two real ranks sharing one GPU over gloo (the states travel through the host), P = 5: a ragged 3 + 2 split.  Both
    ranks must return the aggregates of a single process: the same pick, and the mean of the 3 + 2 grouping."""
    import socket
    wb, want = hypotheses
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "pose_rank_worker.py"),
                                       str(tmp_path / f"rank{r}.pt")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    r0, r1 = (torch.load(str(tmp_path / f"rank{r}.pt")) for r in range(2))
    assert r0["world"] == 2 and r0["local"] == [0, 3] and r1["local"] == [3, 5]
    for r in (r0, r1):
        assert torch.equal(r["idx"], want["idx"].cpu()) and torch.equal(r["pick"], want["pick"].cpu())
        assert torch.equal(r["mean"], host_mean(wb, (3, 2)))

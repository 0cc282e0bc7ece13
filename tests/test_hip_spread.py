"""The spread of the hypotheses beside the mean pose: spread_partials_kernel / spread_combine_kernel (pafuse_spread_partials,
pafuse_spread_combine), torch.ops.pafuse.hypothesis_spread, evaluate.accumulate_spread / aggregate_poses_sharded(spread_state=)
and infer_sequence(spread=...).

What is asserted and why it can be asserted:
  * mean: the state's `sum` is the pose state's sum (same values, same order, fp64), divided by the same count in fp64 and
    rounded once -> torch.equal to combine_poses' mean of the SAME split.
  * covariance and std against fp64 on the host (harness.wb_pose_from_parts(pred).double(), mean and population covariance
    by torch): the kernels' arithmetic is fp64 (Welford per hypothesis, Chan per shard), relative error of order P * 2^-52,
    about 2^-28 of an fp32 step - it can move the fp32 result only when the exact value sits on a rounding boundary.
    std and the diagonal of cov: equal to the reference rounded to fp32, or adjacent to it (one nextafter step).
    Off-diagonal: one step plus 2^-40 * sqrt(c_ii c_jj) - a small covariance is a cancelled sum of terms of that size.
    Worst observed distance on the MI355X, in steps of the reference: 0 for std, for the
    diagonal and for the off-diagonal entries (without the slack term too), for every split and end to end:
    every value equal to the reference rounded to fp32.  check_against_fp64 prints the figures before it asserts.
  * exact cases (torch.equal to a constant): identical hypotheses and a single hypothesis have cov == 0 and std == 0 (k
    copies of an fp32 value sum and divide exactly in fp64, so Welford's d and Chan's delta are exactly 0 - raw sums of
    squares could not promise that); joint 0 is pinned; two integer hypotheses c + d, c - d give mean c and cov d (x) d.
Shapes: B=2, T=2, P=5, F=3, J=134 (1 608 elements: six full 256-thread blocks and a ragged seventh) and B=T=P=F=1 (134
elements, less than one block).
"""
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT
from tests.test_hip_partials import dataset, same_bits, tables
from tests.test_hip_pose_aggregate import BIG, J, SMALL, cuts_of, e2e_inputs, infer, inputs, whole_body

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("mean", "cov", "std")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))              # the order of m2 and cov: xx, xy, xz, yy, yz, zz
DIAG, OFF = (0, 3, 5), (1, 2, 4)
SPLITS = {"one": (5,), "3+2": (3, 2), "ones": (1, 1, 1, 1, 1), "2+0+3": (2, 0, 3)}
RUNNING = (2, 2, 1)
PAD = 3


def spread(pred, sizes, conn=None, running=False, want=NAMES, merged=False):
    """the P hypotheses cut into shards of `sizes`: one state per shard (rows padded and NaN-filled beforehand) combined in
    one call, or (running=True) folded chunk after chunk into a running state merged in place.  merged=True: also the
    merged state, under "state"."""
    from pafuse_amd import ops
    B, T, P, F = pred.shape[:4]
    conn = tables()[0] if conn is None else conn
    L = ops.spread_partials_bytes(B, T, F, J) // 8
    cuts = cuts_of(P, sizes)
    shard = lambda lo, hi: pred[:, :, lo:hi].contiguous()
    if not running:
        states = torch.full((len(cuts), L + PAD), float("nan"), device=DEV, dtype=torch.float64)
        for r, (lo, hi) in enumerate(cuts):
            ops.spread_partials(shard(lo, hi), conn, lo, out=states[r])
        assert torch.isnan(states[:, L:]).all()                   # nothing is written behind a state
        into = torch.full((L + PAD,), float("nan"), device=DEV, dtype=torch.float64) if merged else None
        out = ops.combine_spread(states, (B, T, F, J), merged=into, want=want)
        if merged:
            assert torch.isnan(into[L:]).all()
            out["state"] = into[:L]
        return out
    slots = torch.full((2, L), float("nan"), device=DEV, dtype=torch.float64)
    for r, (lo, hi) in enumerate(cuts):
        ops.spread_partials(shard(lo, hi), conn, lo, out=slots[0 if r == 0 else 1])
        if r:
            ops.combine_spread(slots, (B, T, F, J), merged=slots[0], want=())
    out = ops.combine_spread(slots[:1], (B, T, F, J), want=want)
    if merged:
        out["state"] = slots[0].clone()
    return out


def reference(wb):
    """wb [B,T,P,F,J,3] whole-body hypotheses on the host -> fp64 mean [B,T,F,J,3], population covariance [B,T,F,J,6], std"""
    x = wb.double()
    mean = x.mean(dim=2)
    c = x - mean[:, :, None]
    cov = torch.stack([(c[..., a] * c[..., b]).mean(dim=2) for a, b in PAIRS], dim=-1)
    return {"mean": mean, "cov": cov, "std": (cov[..., 0] + cov[..., 3] + cov[..., 5]).sqrt()}


def steps_from(got, ref64, slack=None):
    """distance of the fp32 result `got` from the fp64 reference rounded to fp32, in nextafter steps of that value, after
    taking `slack` (fp64, absolute) off"""
    r32 = ref64.float()
    step = (torch.nextafter(r32.abs(), torch.full_like(r32, float("inf"))) - r32.abs()).double()
    dist = (got.cpu().double() - r32.double()).abs()
    if slack is not None:
        dist = (dist - slack).clamp_min(0)
    return dist / step


def check_against_fp64(got, ref, what):
    """the bounds of the module docstring; prints the worst distances before it asserts"""
    cov, rc = got["cov"].cpu(), ref["cov"]
    worst = {"std": float(steps_from(got["std"], ref["std"]).max()),
             "diag": float(steps_from(cov[..., DIAG], rc[..., DIAG]).max())}
    slack = torch.stack([2.0 ** -40 * (rc[..., DIAG[PAIRS[k][0]]] * rc[..., DIAG[PAIRS[k][1]]]).sqrt() for k in OFF], dim=-1)
    worst["off_no_slack"] = float(steps_from(cov[..., OFF], rc[..., OFF]).max())
    worst["off"] = float(steps_from(cov[..., OFF], rc[..., OFF], slack).max())
    print(f"{what}: worst distance from the fp64 reference in fp32 steps: {worst}")
    assert worst["std"] <= 1.0 and worst["diag"] <= 1.0 and worst["off"] <= 1.0, (what, worst)
    assert (cov[..., DIAG] >= 0).all() and (got["std"] >= 0).all()


@pytest.fixture(scope="module")
def big():
    """inputs, their whole-body poses on the host, the fp64 reference, and the spread of every split (computed once, never
    modified)"""
    z = inputs(*BIG, seed=21)
    wb = whole_body(z["pred"])
    got = {k: spread(z["pred"], s) for k, s in SPLITS.items()}
    got["running"] = spread(z["pred"], RUNNING, running=True)
    return z, wb, reference(wb), got


@pytest.fixture(scope="module")
def small():
    z = inputs(*SMALL, seed=22)
    wb = whole_body(z["pred"])
    return z, wb, reference(wb), spread(z["pred"], (1,))


def test_outputs_have_their_shapes(big):
    _, _, _, got = big
    B, T, P, F = BIG
    for out in got.values():
        assert tuple(out["mean"].shape) == (B, T, F, J, 3) and tuple(out["cov"].shape) == (B, T, F, J, 6)
        assert tuple(out["std"].shape) == (B, T, F, J) and all(out[k].dtype == torch.float32 and out[k].is_cuda for k in NAMES)


@pytest.mark.parametrize("split", list(SPLITS) + ["running"])
def test_mean_is_the_pose_mean_of_the_same_split(big, split):
    from tests.test_hip_pose_aggregate import aggregate
    z, _, ref, got = big
    if split == "running":
        pose = aggregate(z, RUNNING, running=True, reproj=False, want=("mean",))
    else:
        pose = aggregate(z, SPLITS[split], reproj=False, want=("mean",))
    assert torch.equal(got[split]["mean"], pose["mean"])
    assert float(steps_from(got[split]["mean"], ref["mean"]).max()) <= 1.0


@pytest.mark.parametrize("split", list(SPLITS) + ["running"])
def test_covariance_and_std_against_fp64(big, split):
    _, _, ref, got = big
    check_against_fp64(got[split], ref, split)
    assert float(got[split]["std"].max()) > 0.1                    # 0.25 randn hypotheses: the comparison is not vacuous


def test_one_hypothesis_and_identical_hypotheses_have_no_spread(big, small):
    z, wb, ref, got = small
    assert torch.equal(got["mean"].cpu(), wb[:, :, 0]) and (got["cov"] == 0).all() and (got["std"] == 0).all()
    zb = big[0]
    one = zb["pred"][:, :, 2:3]
    assert float(one.abs().max()) > 0.1
    same = one.expand(-1, -1, 5, -1, -1, -1).contiguous()
    for sizes in list(SPLITS.values()) + [RUNNING]:
        out = spread(same, sizes, running=sizes == RUNNING)
        assert torch.equal(out["cov"], torch.zeros_like(out["cov"])), sizes
        assert torch.equal(out["std"], torch.zeros_like(out["std"])), sizes
        assert torch.equal(out["mean"].cpu(), whole_body(one)[:, :, 0]), sizes


def test_joint_0_is_pinned(big):
    _, _, _, got = big
    for k, out in got.items():
        assert (out["std"][..., 0] == 0).all() and (out["cov"][..., 0, :] == 0).all() and (out["mean"][..., 0, :] == 0).all(), k
        assert (out["std"][..., 1:] > 0).all(), k


def test_two_integer_hypotheses_give_their_outer_product():
    from pafuse_amd import harness
    B, T, F = 2, 2, 3
    conn = tables()[0]
    g = torch.Generator().manual_seed(23)
    c = torch.randint(-4, 5, (B, T, F, J, 3), generator=g).float()
    d = torch.randint(-4, 5, (B, T, F, J, 3), generator=g).float()
    joints = sorted(set(conn.cpu().tolist()) | {0})                # the connection joints: their own offsets are zero,
    assert joints == [0, 1, 10, 11]                                # so every whole-body joint is the part-centred one
    c[..., joints, :] = 0
    d[..., joints, :] = 0
    pred = torch.stack((c + d, c - d), dim=2)
    assert float(pred.abs().max()) <= 8 and torch.equal(harness.wb_pose_from_parts(pred, dataset()), pred)
    want = torch.stack([d[..., a] * d[..., b] for a, b in PAIRS], dim=-1)
    assert len(want.unique()) == 19                               # every product of two integers in [-4, 4] occurs
    for sizes in ((2,), (1, 1)):
        out = spread(pred.to(DEV), sizes)
        assert torch.equal(out["cov"].cpu(), want), sizes
        assert torch.equal(out["mean"].cpu(), c), sizes
        assert torch.equal(out["std"].cpu(), d.double().pow(2).sum(-1).sqrt().float()), sizes    # a correctly rounded fp64 sqrt


def test_running_state_is_the_one_call_combine(big):
    z = big[0]
    one = spread(z["pred"], RUNNING, merged=True)
    run = spread(z["pred"], RUNNING, running=True, merged=True)
    assert same_bits(run["state"], one["state"])
    for k in NAMES:
        assert torch.equal(run[k], one[k]) and torch.equal(run[k], big[3]["running"][k]), k
    from pafuse_amd import ops
    v = ops.spread_views(run["state"], BIG[0], BIG[1], BIG[3], J)
    assert float(v["count"]) == 5.0 and float(ops.spread_views(one["state"], BIG[0], BIG[1], BIG[3], J)["count"]) == 5.0


def test_state_holds_the_pose_sums_and_the_count(big):
    from pafuse_amd import ops
    z = big[0]
    B, T, P, F = BIG
    conn = tables()[0]
    st = ops.spread_partials(z["pred"][:, :, 1:4].contiguous(), conn, 1)
    assert st.numel() * 8 == ops.spread_partials_bytes(B, T, F, J)
    v = ops.spread_views(st, B, T, F, J)
    pose = ops.pose_views(ops.pose_partials(z["pred"][:, :, 1:4].contiguous(), conn, 1), B, T, F, J)
    assert same_bits(v["sum"], pose["sum"]) and float(v["count"]) == 3.0
    wb = whole_body(z["pred"][:, :, 1:4]).double()
    c = wb - wb.mean(dim=2, keepdim=True)
    m2 = torch.stack([(c[..., a] * c[..., b]).sum(dim=2) for a, b in PAIRS], dim=-1)
    assert torch.allclose(v["m2"].cpu(), m2, rtol=1e-12, atol=1e-14)   # fp64 on both sides, three hypotheses


def test_empty_shards_are_neutral(big):
    from pafuse_amd import ops
    z, _, _, got = big
    B, T, P, F = BIG
    conn = tables()[0]
    L = ops.spread_partials_bytes(B, T, F, J) // 8
    buf = torch.full((L + PAD,), 7.0, device=DEV, dtype=torch.float64)
    empty = ops.spread_partials(z["pred"][:, :, :0].contiguous(), conn, 2, out=buf)
    assert empty.data_ptr() == buf.data_ptr() and (buf[:L] == 0).all() and (buf[L:] == 7.0).all()
    for k in NAMES:                                               # the skipped state leaves the merge as it is, bit for bit
        assert torch.equal(got["2+0+3"][k], spread(z["pred"], (2, 3))[k]), k
    into = torch.full((L,), 7.0, device=DEV, dtype=torch.float64)
    out = ops.combine_spread(torch.stack((buf, buf)), (B, T, F, J), merged=into)      # only empty states: NaN, and a neutral union
    assert all(torch.isnan(out[k]).all() for k in NAMES) and (into == 0).all()
    full = ops.spread_partials(z["pred"], conn, 0)
    for order in ((buf[:L], full), (full, buf[:L]), (buf[:L], full, buf[:L])):
        out = ops.combine_spread(torch.stack(order), (B, T, F, J))
        for k in NAMES:
            assert torch.equal(out[k], got["one"][k]), k
    with pytest.raises(ValueError):                               # a merged state over an operand other than the first
        two = torch.stack((full, buf[:L]))
        ops.combine_spread(two, (B, T, F, J), merged=two[1])
    with pytest.raises(ValueError):
        ops.spread_partials(z["pred"], conn, 0, out=torch.empty(3, device=DEV, dtype=torch.float64))
    e = ops.spread_partials(z["pred"][:0].contiguous(), conn, 0)   # B == 0: an empty state and empty outputs
    assert e.numel() == 0 and tuple(ops.combine_spread(e.view(1, 0), (0, T, F, J))["cov"].shape) == (0, T, F, J, 6)


@pytest.mark.parametrize("sizes", [(5,), (3, 2)])
def test_a_non_finite_hypothesis_stays_in_its_element(big, sizes):
    z, _, _, got = big
    B, T, P, F = BIG
    conn = tables()[0].cpu()
    b, t, h, f, j = 1, 0, 3, 2, 10
    joints = [j] + [k for k in range(1, J) if int(conn[k]) == j]   # joint 10 and the part that hangs on it: the left hand
    assert joints == [10] + list(range(92, 113))
    bad = z["pred"].clone()
    bad[b, t, h, f, j, 1] = float("inf")
    hit = torch.zeros(B, T, F, J, dtype=torch.bool, device=DEV)
    hit[b, t, f, joints] = True
    out = spread(bad, sizes)
    clean = got["one" if sizes == (5,) else "3+2"]
    for k in NAMES:
        assert torch.isnan(out[k][hit]).all(), k
        assert torch.equal(out[k][~hit], clean[k][~hit]), k


def test_torch_op_is_the_ops_pair(big):
    from pafuse_amd import torch_ops  # noqa: F401
    z, _, _, got = big
    mean, cov, std = torch.ops.pafuse.hypothesis_spread(z["pred"], tables()[0])
    assert torch.equal(mean, got["one"]["mean"]) and torch.equal(cov, got["one"]["cov"]) and torch.equal(std, got["one"]["std"])
    s = str(torch.ops.pafuse.hypothesis_spread.default._schema)
    assert "Tensor pred, Tensor conn" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fake = torch.ops.pafuse.hypothesis_spread(torch.empty(2, 3, 5, 4, J, 3, device=DEV), torch.empty(J, device=DEV, dtype=torch.int32))
        assert [tuple(t.shape) for t in fake] == [(2, 3, 4, J, 3), (2, 3, 4, J, 6), (2, 3, 4, J)]
        assert all(t.dtype == torch.float32 for t in fake)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model():
    from __graft_entry__ import make_model
    return make_model(5, 2, depth=2)[0]


@pytest.fixture(scope="module")
def hypotheses(model):
    """the whole-body hypotheses of noise stream (SEED, call 0) on the host, and their fp64 spread"""
    wb = infer(model)
    assert tuple(wb.shape) == (2, 2, 5, 27, J, 3) and not wb.is_cuda
    return wb, reference(wb)


def test_infer_sequence_returns_the_spread_of_its_hypotheses(model, hypotheses):
    from pafuse_amd import harness
    wb, ref = hypotheses
    out = infer(model, aggregate="mean", spread="cov", hypothesis_chunk=2)
    assert sorted(out) == ["cov", "pose", "std"] and not any(v.is_cuda for v in out.values())
    assert tuple(out["std"].shape) == (2, 2, 27, J) and tuple(out["cov"].shape) == (2, 2, 27, J, 6)
    assert torch.equal(out["pose"], infer(model, aggregate="mean", hypothesis_chunk=2))
    check_against_fp64(out, ref, "infer_sequence, chunks of 2")
    assert float(out["std"][..., 1:].min()) > 0
    std_only = infer(model, aggregate="mean", spread="std")
    assert sorted(std_only) == ["pose", "std"]
    check_against_fp64(dict(std_only, cov=out["cov"]), ref, "infer_sequence, one chunk")
    # laid out on the frames of the sequence by the rule of stitch_poses
    frames = e2e_inputs()[0].shape[0]
    flat = harness.stitch_spread(out["std"], frames, 27)
    assert tuple(flat.shape) == (2, frames, J) and tuple(harness.stitch_spread(out["cov"], frames, 27).shape) == (2, frames, J, 6)
    assert torch.equal(flat[:, :27], out["std"][0]) and torch.equal(flat[:, 27:], out["std"][1, :, -(frames - 27):])
    assert torch.equal(flat, harness.stitch_poses(out["std"][..., None].expand(-1, -1, -1, -1, 3).contiguous(), frames, 27)[..., 0])


def test_spread_leaves_the_reprojection_pick_alone(model, hypotheses):
    wb, ref = hypotheses
    pose, idx = infer(model, aggregate="reproj")
    out = infer(model, aggregate="reproj", spread="std", hypothesis_chunk=2)
    assert sorted(out) == ["idx", "pose", "std"]
    assert torch.equal(out["pose"], pose) and torch.equal(out["idx"], idx)
    assert float(steps_from(out["std"], ref["std"]).max()) <= 1.0


def spread_of_whole_body(wb, sizes):
    """the ops pair on the WHOLE-BODY hypotheses infer_sequence(aggregate=None) returns: with a connection table of zeros
    wb_joint adds joint 0, which a whole-body pose pins at 0, so every joint goes through unchanged"""
    assert (wb[..., 0, :] == 0).all()
    return spread(wb.to(DEV), sizes, conn=torch.zeros(J, dtype=torch.int32, device=DEV))


def test_two_rank_spread_on_one_gpu(tmp_path, hypotheses):
    """Two real ranks sharing one GPU over gloo (the states travel through the host), P = 5: a ragged 3 + 2 split.  Both
    ranks must return the mean, covariance and std of the single-process 3 + 2 combine."""
    import socket
    wb, _ = hypotheses
    want = spread_of_whole_body(wb, (3, 2))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "280", sys.executable, os.path.join(ROOT, "tests", "spread_rank_worker.py"),
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
        assert torch.equal(r["pose"], want["mean"].cpu()) and torch.equal(r["cov"], want["cov"].cpu())
        assert torch.equal(r["std"], want["std"].cpu())
        assert torch.equal(r["reproj_std"], r["std"])

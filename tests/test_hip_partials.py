"""Protocol #1 from per-shard partial reductions: partials_kernel / combine_kernel (pafuse_hypothesis_partials,
pafuse_hypothesis_combine), evaluate_accumulators_sharded and evaluate_sequence(gather="partials").

What is asserted and why it can be asserted:
  * j_best / j_agg maps and the J-Agg index: a minimum and a first minimum do not depend on the order or grouping of
    their operands and every per-hypothesis expression is metrics_kernel's -> torch.equal with the unsharded kernel
    for every split, and the index equals pafuse_procrustes_errors' pick.
  * p_agg*, p_best*: fp64 sums of <= 160 fp32 values added in a fixed order; two groupings differ by < 2^-50 relative,
    far below the fp32 rounding of the divide that follows -> bit-identical across all splits and chunk sizes.
  * against the unsharded kernel those values differ in the last bits (it sums in fp32).  Yardstick: the fp64 truth
    below (the reference's formulas on the fp32 whole-body poses).  Requirement: the new path's max |d| to the truth is
    no larger than the unsharded kernel's on the same inputs (tools/partials_bench.py records both distances).
  * end to end the two gather modes see the same hypotheses; the fp32-summed accumulators of the unsharded kernel may
    sit (P - 1) * 2^-24 * max|coordinate| = 159 * 6e-8 * 2 m = 1.9e-5 m from the fp64 mean per coordinate, sqrt(3) times
    that per joint error: E2E_ATOL = 3.3e-5 m (worst case of sequential fp32 summation; measured distances are ~1e-7).
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from pafuse_amd.parallel import shard_range
from tests.conftest import ROOT
from tests.golden import golden_util as gu
from tests.test_p2_report import conn_table, wb

pytestmark = pytest.mark.gpu
DEV = "cuda"
E2E_ATOL = 3.3e-5
PARTS = list(gu.DATASET_PART_JOINTS)
MAPS = ("jbest", "pagg", "jagg", "paggpb")
PBEST = ("p_best", "p_best_pb") + tuple("p_best_pb_" + p for p in PARTS)
FP64_SUMMED = ("p_agg", "p_agg_pb") + tuple("p_agg_pb_" + p for p in PARTS) + PBEST


def dataset():
    return SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                           parts_connection_indices=dict(gu.CONNECTION_INDICES))


def tables():
    from pafuse_amd.evaluate import _part_table, _tables
    conn, pbroot = _tables(dataset(), 134, DEV)
    return conn, pbroot, _part_table(dataset(), 134, DEV)


def same_bits(a, b):
    """torch.equal on the bit patterns (a NaN equals the same NaN)"""
    ints = {torch.float32: torch.int32, torch.float64: torch.int64}
    return a.dtype == b.dtype and torch.equal(a.view(ints.get(a.dtype, a.dtype)), b.view(ints.get(b.dtype, b.dtype)))


def inputs(B, T, P, F, seed, special=True, nan=True):
    """random part-centred predictions around a random target (J = 134).  special=True plants the hard cases: hypotheses
    6|7 and 9|10 identical (exact ties in e2 and e3 across the borders of the 3-, 2- and 4-way splits of P = 20, and
    of the 20-way one); nan=True also makes one joint NaN in hypotheses 0 .. 6 (the whole first shard of the 3-, 4- and
    20-way splits: NaN e3 there, while e2 stays finite - the kernels' clamp of the projected point swallows a NaN, so
    no prediction can make e2 non-finite) and the 2-D input of another joint NaN (e2 NaN in every hypothesis of every
    shard: no candidate anywhere)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(B, F, 134, 3, generator=g) * 0.3
    pred = gt[:, None, None] + torch.randn(B, T, P, F, 134, 3, generator=g) * 0.05
    x2d = torch.rand(B, F, 134, 2, generator=g) * 2 - 1
    traj = torch.randn(B, F, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    if special and P >= 11:
        pred[:, :, 7] = pred[:, :, 6]
        pred[:, :, 10] = pred[:, :, 9]
        if nan:
            pred[:, :, :7, F // 2, 40] = float("nan")
            x2d[:, F // 2, 50] = float("nan")
    return tuple(t.contiguous().to(DEV) for t in (pred, gt, x2d, traj, cam))


def unsharded(pred, gt, x2d, traj, cam):
    """pafuse_hypothesis_errors on all hypotheses: its four maps and the two [B,T,P,F,J] scratch tensors"""
    from pafuse_amd import _lib
    lib = _lib.load()
    conn, pbroot, _ = tables()
    B, T, P, F, J, _ = pred.shape
    o = {k: torch.empty(B, T, P, F, J, device=DEV) for k in ("e3", "epb")}
    o.update({k: torch.empty(B, T, F, J, device=DEV) for k in MAPS})
    _lib.check(lib.pafuse_hypothesis_errors(
        pred.data_ptr(), gt.data_ptr(), x2d.data_ptr(), traj.data_ptr(), cam.data_ptr(), conn.data_ptr(), pbroot.data_ptr(),
        B, T, P, F, J, o["e3"].data_ptr(), o["epb"].data_ptr(), o["jbest"].data_ptr(), o["pagg"].data_ptr(),
        o["jagg"].data_ptr(), o["paggpb"].data_ptr(), torch.cuda.current_stream().cuda_stream))
    return o


def sharded(pred, gt, x2d, traj, cam, world):
    """every shard of shard_range(P, r, world) reduced on its own, the states laid out rank-major and padded to the
    largest shard as the all-gather leaves them, combined -> maps, the J-Agg index, the per-hypothesis sums [P,T,5]"""
    from pafuse_amd import ops
    conn, pbroot, part = tables()
    B, T, P, F, J, _ = pred.shape
    pmax = max(shard_range(P, r, world)[1] - shard_range(P, r, world)[0] for r in range(world))
    L = ops.partials_bytes(B, T, pmax, F, J, 4) // 8
    states = torch.full((world, L), float("nan"), device=DEV, dtype=torch.float64)
    hs = []
    for r in range(world):
        lo, hi = shard_range(P, r, world)
        ops.hypothesis_partials(pred[:, :, lo:hi].contiguous(), gt, x2d, traj, cam, conn, pbroot, part, 4, lo, out=states[r])
        hs.append(ops.partials_views(states[r], B, T, hi - lo, F, J, 4)["hsum"])
    merged = torch.empty(5 * B * T * F * J, device=DEV, dtype=torch.float64)
    out = ops.combine_partials(states, gt, conn, pbroot, (B, T, F, J), P, merged=merged)
    out["idx"] = ops.partials_views(merged, B, T, 0, F, J, 4)["idx"]
    out["hsum"] = torch.cat(hs)
    return out


def accumulators_chunked(pred, gt, x2d, traj, cam, chunk):
    from pafuse_amd.evaluate import accumulate_partials, evaluate_accumulators_sharded
    P = pred.shape[2]
    state = None
    for lo in range(0, P, chunk):
        state = accumulate_partials(state, pred[:, :, lo:lo + chunk], lo, gt, x2d, traj, cam, dataset())
    return evaluate_accumulators_sharded(None, None, P, gt, x2d, traj, cam, dataset(), state=state)


def truth64(pred, gt):
    """fp64 Protocol #1 of the order-dependent accumulators: the reference's formulas (main_h3wb.py:327-362 with
    common/loss.py:36-168) on the fp32 whole-body poses, every sum and mean in fp64 -> pagg, paggpb maps [B,T,F,J] and
    the per-hypothesis means e3 [T,P], epb [T,P], epb per part {part: [T,P]}"""
    pred, gt = pred.cpu().float(), gt.cpu().float()
    conn = conn_table(134)
    root = torch.zeros(134, dtype=torch.long)
    for p, idx in gu.DATASET_PART_JOINTS.items():
        root[list(idx)] = gu.ROOT_INDICES[p]
    w, g = wb(pred, conn), wb(gt, conn)                                   # fp32, as the reference forms them
    wc, gc = (w - w[..., root, :]).double(), (g - g[..., root, :]).double()   # center_pose_parts in fp32
    w, g = w.double(), g.double()
    e3 = (w - g[:, None, None]).norm(dim=-1)                               # [B,T,P,F,J]
    epb = (wc - gc[:, None, None]).norm(dim=-1)
    T, P = pred.shape[1], pred.shape[2]
    out = {"pagg": (w.mean(dim=2) - g[:, None]).norm(dim=-1),
           "paggpb": ((w.mean(dim=2) - w.mean(dim=2)[..., root, :]) - gc[:, None]).norm(dim=-1),
           "e3": e3.permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1),
           "epb": epb.permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1)}
    for p, idx in gu.DATASET_PART_JOINTS.items():
        out["epb_" + p] = epb[..., list(idx)].permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1)
    return out


def distances_to_truth(pred, gt, x2d, traj, cam):
    """max |d| to the fp64 truth of the fp32-order accumulators, for the unsharded kernel ("old": fp32 sums, fp32 torch
    means as evaluate_accumulators forms them) and the partial path ("new"), on inputs without NaN"""
    B, T, P, F, J, _ = pred.shape
    tr = truth64(pred, gt)
    old, new = unsharded(pred, gt, x2d, traj, cam), sharded(pred, gt, x2d, traj, cam, 1)
    d = {"old": {}, "new": {}}
    for k in ("pagg", "paggpb"):
        for name, got in (("old", old), ("new", new)):
            d[name][k] = (got[k].cpu().double() - tr[k]).abs().max().item()
    hs = new["hsum"].permute(1, 0, 2).cpu()                                 # [T,P,5]
    n = B * F * J
    per_h = {"old": {"e3": old["e3"].permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1),
                     "epb": old["epb"].permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1)},
             "new": {"e3": (hs[..., 0] / n).float(), "epb": (hs[..., 1:].sum(-1) / n).float()}}
    for i, (p, idx) in enumerate(gu.DATASET_PART_JOINTS.items()):
        per_h["old"]["epb_" + p] = old["epb"][..., list(idx)].permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1)
        per_h["new"]["epb_" + p] = (hs[..., 1 + i] / (B * F * len(idx))).float()
    for name in ("old", "new"):
        for k, v in per_h[name].items():
            d[name]["per_hypothesis_mean_" + k] = (v.cpu().double() - tr[k]).abs().max().item()
    return d


# ---------------------------------------------------------------------------------------------------- kernel level
SPLITS = [(20, 1), (20, 2), (20, 3), (20, 4), (20, 20), (160, 8)]


@pytest.fixture(scope="module")
def cases():
    """P -> (inputs, unsharded result, {world: sharded result}); F*J = 5*134 = 670 = 10 waves + 30 lanes"""
    out = {}
    for P in (20, 160):
        z = inputs(2, 2, P, 5, seed=300 + P)
        out[P] = (z, unsharded(*z), {w: sharded(*z, w) for p, w in SPLITS if p == P})
    return out


@pytest.mark.parametrize("P,world", SPLITS)
def test_order_free_accumulators_are_exact(cases, P, world):
    from pafuse_amd import ops
    z, ref, by_world = cases[P]
    got = by_world[world]
    assert same_bits(got["jbest"], ref["jbest"]) and same_bits(got["jagg"], ref["jagg"])
    assert torch.isfinite(got["jbest"]).all()                    # fminf drops the NaN e3 of hypotheses 0 .. 6 on both paths
    conn, _, _ = tables()
    pick = ops.procrustes_errors(*z, conn, pick=True)["pick"]
    assert torch.equal(got["idx"][pick >= 0], pick[pick >= 0]) and (pick >= 0).sum() == pick.numel() - 4
    # the joint without a finite e2: no candidate in any shard -> index -1 and 0, as the unsharded kernel leaves it
    assert (pick[:, :, 2, 50] == -1).all() and (got["idx"][pick < 0] == -1).all() and (got["jagg"][pick < 0] == 0).all()
    if (P, world) == (20, 3):
        pred, gt, x2d, traj, cam = z
        conn, pbroot, part = tables()
        s0 = ops.partials_views(ops.hypothesis_partials(pred[:, :, :7].contiguous(), gt, x2d, traj, cam, conn, pbroot, part, 4, 0),
                                2, 2, 7, 5, 134, 4)
        assert (s0["idx"][:, :, 2, 50] == -1).all() and (s0["e2"][:, :, 2, 50] == float("inf")).all()
        assert (s0["sel3"][:, :, 2, 50] == 0).all() and (s0["idx"] == -1).sum() == 4
        assert torch.isnan(s0["sum"][:, :, 2, 40]).all() and (s0["jbest"][:, :, 2, 40] == float("inf")).all()
    # the planted ties were met: where hypothesis 6 (or 9) is picked, its twin 7 (10) has the same e2 and lost
    assert (got["idx"] == 6).any() and not (got["idx"] == 7).any() and not (got["idx"] == 10).any()


@pytest.mark.parametrize("P", [20, 160])
def test_split_independence_of_the_fp64_summed_accumulators(cases, P):
    z, _, by_world = cases[P]
    worlds = sorted(by_world)
    first = by_world[worlds[0]]
    for w in worlds[1:]:                       # P = 20: 1 (the 1-shard case), 2, 3, 4, 20 shards; P = 160: 8
        for k in ("pagg", "paggpb", "hsum", "jbest", "jagg", "idx"):
            assert same_bits(by_world[w][k], first[k]), (k, w)
    # the 14 vectors: the shard splits (states laid out as the all-gather leaves them) and chunked accumulation on one
    # device, chunk 5 vs 20 vs 160 (one chunk when chunk >= P), on the same inputs without the NaN joint
    z = inputs(2, 2, P, 5, seed=300 + P, nan=False)
    accs = [accumulators_chunked(*z, c) for c in (5, 20, 160)]
    assert set(accs[0]) == set(FP64_SUMMED) | {"j_best", "j_agg"} and len(accs[0]) == 14
    assert all(torch.isfinite(v).all() for v in accs[0].values())
    for a in accs[1:]:
        for k in accs[0]:
            assert torch.equal(a[k], accs[0][k]), k
    one = sharded(*z, 1)
    for w in ((2, 3, 4, 20) if P == 20 else (8,)):
        got = sharded(*z, w)
        for k in MAPS + ("hsum", "idx"):
            assert torch.equal(got[k], one[k]), (k, w)
    # ... and the chunked running state ends where the combination of shards ends
    per_t = lambda x: x.permute(1, 0, 2, 3).reshape(x.shape[1], -1).mean(dim=-1)
    assert torch.equal(accs[0]["p_agg"], per_t(one["pagg"])) and torch.equal(accs[0]["p_agg_pb"], per_t(one["paggpb"]))
    assert torch.equal(accs[0]["p_best"], (one["hsum"].permute(1, 0, 2)[..., 0] / (2 * 5 * 134)).float().min(dim=1).values)


def test_two_calls_same_bits(cases):
    z, _, by_world = cases[20]
    again = sharded(*z, 3)
    for k, v in by_world[3].items():
        assert same_bits(v, again[k]), k


def test_single_hypothesis_and_empty_shard():
    """P = 1: minimum, pick and mean pose are that one pose; an empty shard (P_r = 0) is the neutral state and leaves
    the combination unchanged"""
    from pafuse_amd import ops
    z = inputs(1, 2, 1, 3, seed=5, special=False)
    pred, gt, x2d, traj, cam = z
    ref, got = unsharded(*z), sharded(*z, 1)
    assert torch.equal(got["jbest"], ref["jbest"]) and torch.equal(got["jagg"], ref["jagg"]) and (got["idx"] == 0).all()
    assert torch.equal(got["jbest"], got["jagg"])
    conn, pbroot, part = tables()
    B, T, P, F, J, _ = pred.shape
    s1 = ops.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, 4, 0)
    s0 = ops.hypothesis_partials(pred[:, :, :0].contiguous(), gt, x2d, traj, cam, conn, pbroot, part, 4, 1)
    v = ops.partials_views(s0, B, T, 0, F, J, 4)
    assert (v["jbest"] == float("inf")).all() and (v["e2"] == float("inf")).all() and (v["idx"] == -1).all()
    assert (v["sum"] == 0).all() and (v["sel3"] == 0).all() and v["hsum"].numel() == 0
    both = torch.stack([s1[:5 * B * T * F * J], s0])
    again = ops.combine_partials(both, gt, conn, pbroot, (B, T, F, J), 1)
    for k in MAPS:
        assert torch.equal(again[k], got[k]), k


def test_shards_without_a_candidate_in_first_and_middle_position():
    """combine_kernel's candidate rule with "no candidate" states anywhere in the order.  Two kinds: the neutral state of an
    empty shard (every joint without a candidate, zero sums), and a real shard's state with hand-erased candidates on half
    of the joints ((+inf, 0, -1) there, as a shard whose every e2 is non-finite would leave them - no prediction can do
    that through the kernel, whose clamp swallows a NaN).  The result must be what the shards WITH candidates give."""
    from pafuse_amd import ops
    from pafuse_amd.evaluate import accumulate_partials, evaluate_accumulators_sharded
    z = inputs(2, 2, 9, 3, seed=21, special=False)
    pred, gt, x2d, traj, cam = z
    conn, pbroot, part = tables()
    B, T, P, F, J, _ = pred.shape
    n5 = 5 * B * T * F * J
    st = [ops.hypothesis_partials(pred[:, :, lo:lo + 3].contiguous(), gt, x2d, traj, cam, conn, pbroot, part, 4, lo)[:n5] for lo in (0, 3, 6)]
    empty = lambda h0: ops.hypothesis_partials(pred[:, :, :0].contiguous(), gt, x2d, traj, cam, conn, pbroot, part, 4, h0)

    def combined(states):
        merged = torch.empty(n5, device=DEV, dtype=torch.float64)
        out = ops.combine_partials(torch.stack(states), gt, conn, pbroot, (B, T, F, J), P, merged=merged)
        out["idx"] = ops.partials_views(merged, B, T, 0, F, J, 4)["idx"].clone()
        return out

    want = combined(st)
    ref = unsharded(*z)
    assert torch.equal(want["jagg"], ref["jagg"]) and torch.equal(want["jbest"], ref["jbest"])
    for states in ([empty(0)] + st, [st[0], empty(3), st[1], st[2]], [empty(0), st[0], empty(3), empty(3), st[1], st[2], empty(9)]):
        got = combined(states)
        for k in MAPS + ("idx",):
            assert torch.equal(got[k], want[k]), (k, len(states))
    # erased candidates: on even joints in the FIRST shard, on joints 0 mod 3 in the MIDDLE one
    def erased(state, keep):
        state = state.clone()
        v = ops.partials_views(state, B, T, 0, F, J, 4)
        v["e2"][..., ~keep] = float("inf")
        v["sel3"][..., ~keep] = 0
        v["idx"][..., ~keep] = -1
        return state

    j = torch.arange(J, device=DEV)
    got = combined([erased(st[0], j % 2 == 1), erased(st[1], j % 3 != 0), st[2]])
    v = [ops.partials_views(s.clone(), B, T, 0, F, J, 4) for s in st]
    e2 = torch.stack([torch.where(j % 2 == 1, v[0]["e2"], torch.full_like(v[0]["e2"], float("inf"))),
                      torch.where(j % 3 != 0, v[1]["e2"], torch.full_like(v[1]["e2"], float("inf"))), v[2]["e2"]])
    win = e2.argmin(dim=0)                                           # first minimum = lowest shard among equal ones
    assert (win == 0).any() and (win == 1).any() and (win == 2).any()
    for k, key in (("idx", "idx"), ("jagg", "sel3")):
        pick = torch.stack([x[key] for x in v]).gather(0, win.unsqueeze(0)).squeeze(0)
        assert torch.equal(got[k], pick), k
    assert torch.equal(got["jbest"], want["jbest"]) and torch.equal(got["pagg"], want["pagg"])
    # the running state of chunked evaluation starting from an empty chunk (a rank that owns nothing yet) ends where it ends without
    accs = []
    for first in (False, True):
        state = accumulate_partials(None, pred[:, :, :0], 0, gt, x2d, traj, cam, dataset()) if first else None
        for lo in (0, 3, 6):
            state = accumulate_partials(state, pred[:, :, lo:lo + 3], lo, gt, x2d, traj, cam, dataset())
        accs.append(evaluate_accumulators_sharded(None, None, P, gt, x2d, traj, cam, dataset(), state=state))
    for k in accs[0]:
        assert torch.equal(accs[0][k], accs[1][k]), k


def unique_minimum(per_h, rel=1e-5):
    """[T,P] fp64 means: the smallest is at least `rel` below the runner-up in every step"""
    s = per_h.sort(dim=1).values
    return bool(((s[:, 1] - s[:, 0]) > rel * s[:, 0]).all())


def test_same_p_best_pick_and_accuracy_against_fp64():
    """inputs whose per-hypothesis means have a unique minimum in fp64 (checked): the sharded path picks the hypothesis
    the unsharded one picks, and its fp64-summed accumulators are no farther from the fp64 truth than the unsharded
    kernel's fp32-summed ones"""
    from pafuse_amd.evaluate import evaluate_accumulators
    z = inputs(2, 2, 20, 5, seed=77, special=False)
    pred, gt, x2d, traj, cam = z
    tr = truth64(pred, gt)
    assert unique_minimum(tr["e3"]) and unique_minimum(tr["epb"])
    old = evaluate_accumulators(pred, gt, x2d, traj.reshape(2, 5, 1, 3), cam, dataset())
    scratch = unsharded(*z)                                  # the unsharded path's own pick, formed as evaluate_accumulators forms it
    old_pick = {k: scratch[k].permute(1, 2, 0, 3, 4).reshape(2, 20, -1).mean(dim=-1).argmin(dim=1) for k in ("e3", "epb")}
    n = 2 * 5 * 134
    for world in (1, 3):
        new = sharded(*z, world)
        hs = new["hsum"].permute(1, 0, 2)
        new_pick = {"e3": (hs[..., 0] / n).float().argmin(dim=1), "epb": (hs[..., 1:].sum(-1) / n).float().argmin(dim=1)}
        for k in ("e3", "epb"):
            assert torch.equal(new_pick[k], old_pick[k]), (k, world)
            assert torch.equal(new_pick[k].cpu(), tr[k].argmin(dim=1)), (k, world)
    acc = accumulators_chunked(*z, 7)
    best = tr["epb"].argmin(dim=1)
    want = {"p_best": tr["e3"].min(dim=1).values, "p_best_pb": tr["epb"].min(dim=1).values}
    for p in PARTS:
        want["p_best_pb_" + p] = tr["epb_" + p].gather(1, best.view(-1, 1)).squeeze(1)
    for k, w in want.items():
        d_new, d_old = (acc[k].cpu().double() - w).abs().max().item(), (old[k].cpu().double() - w).abs().max().item()
        print(f"{k}: max|new - fp64| = {d_new:.3e}  max|old - fp64| = {d_old:.3e}")
        assert d_new <= d_old, (k, d_new, d_old)
    d = distances_to_truth(*z)
    for k in d["new"]:
        print(f"{k}: max|new - fp64| = {d['new'][k]:.3e}  max|old - fp64| = {d['old'][k]:.3e}")
        assert d["new"][k] <= d["old"][k], (k, d["new"][k], d["old"][k])


def test_chunked_evaluation_never_holds_the_full_tensor():
    """P = 160 in chunks of 5, every chunk generated when it is needed: the peak allocation of the evaluation stays below
    the bytes of the [B,T,P,F,J,3] tensor alone"""
    from pafuse_amd.evaluate import accumulate_partials, evaluate_accumulators_sharded
    B, T, P, F, J, chunk = 4, 2, 160, 27, 134, 5
    _, gt, x2d, traj, cam = inputs(B, T, 1, F, seed=9, special=False)
    full_bytes = B * T * P * F * J * 3 * 4
    g = torch.Generator(device=DEV).manual_seed(1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    state = None
    for lo in range(0, P, chunk):
        pred = gt[:, None, None] + torch.randn(B, T, chunk, F, J, 3, device=DEV, generator=g) * 0.05
        state = accumulate_partials(state, pred, lo, gt, x2d, traj, cam, dataset())
        del pred
    acc = evaluate_accumulators_sharded(None, None, P, gt, x2d, traj, cam, dataset(), state=state)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak / 1e6:.2f} MB over the evaluation; the full tensor alone: {full_bytes / 1e6:.2f} MB")
    assert len(acc) == 14 and all(torch.isfinite(v).all() for v in acc.values())
    assert peak < full_bytes, (peak, full_bytes)


def test_refusals_on_the_device():
    from pafuse_amd import ops
    pred, gt, x2d, traj, cam = inputs(1, 1, 2, 2, seed=3, special=False)
    conn, pbroot, part = tables()
    with pytest.raises(ValueError):
        ops.hypothesis_partials(pred, gt[:, :1].contiguous(), x2d, traj, cam, conn, pbroot, part, 4, 0)
    with pytest.raises(ValueError):
        ops.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, 4, -1)
    with pytest.raises(ValueError):
        ops.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, 4, 0, out=torch.empty(3, device=DEV, dtype=torch.float64))
    s = ops.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, 4, 0)
    with pytest.raises(ValueError):                       # a merge over its own operand together with the maps
        ops.combine_partials(s.view(1, -1), gt, conn, pbroot, (1, 1, 2, 134), 2, merged=s)
    with pytest.raises(ValueError):
        ops.combine_partials(s.view(1, -1)[:, :10].contiguous(), gt, conn, pbroot, (1, 1, 2, 134), 2)
    from pafuse_amd.evaluate import accumulate_partials, evaluate_accumulators_sharded
    st = accumulate_partials(None, pred, 0, gt, x2d, traj, cam, dataset())
    with pytest.raises(ValueError):                       # a gap: the next chunk must start at hypothesis 2
        accumulate_partials(st, pred, 3, gt, x2d, traj, cam, dataset())
    with pytest.raises(ValueError):                       # 2 of 5 hypotheses seen
        evaluate_accumulators_sharded(None, None, 5, gt, x2d, traj, cam, dataset(), state=st)


def test_torch_ops_are_the_same_entry_points():
    from pafuse_amd import torch_ops  # noqa: F401
    z = inputs(1, 2, 3, 2, seed=4, special=False)
    pred, gt, x2d, traj, cam = z
    conn, pbroot, part = tables()
    s = torch.ops.pafuse.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, 4, 0)
    maps = torch.ops.pafuse.combine_partials(s.view(1, -1), gt, conn, pbroot, 2, 3)
    want = sharded(*z, 1)
    for k, m in zip(MAPS, maps):
        assert torch.equal(m, want[k]), k


# ---------------------------------------------------------------------------------------------------- end to end
def sequence(frames, seed=1):
    g = torch.Generator().manual_seed(seed)
    seq_2d = torch.rand(frames, 134, 2, generator=g) * 2 - 1
    seq_3d = torch.randn(frames, 134, 3, generator=g) * 0.25 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    return seq_2d, seq_3d, cam


def run_sequence(model, frames, **kw):
    from pafuse_amd import harness
    seq_2d, seq_3d, cam = sequence(frames)
    torch.manual_seed(0)
    sums, n = harness.evaluate_sequence(model, dataset(), seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, **kw)
    return {k: v.cpu() for k, v in sums.items()}, n


def compare_modes(got, want, mult):
    """`mult`: the clips x frames multiplier the sums carry"""
    assert set(got) == set(want)
    for k in ("j_best", "j_agg"):
        assert torch.equal(got[k], want[k]), k
    for k in want:
        if k.startswith("p2_"):
            assert torch.equal(got[k], want[k]), k
        else:
            d = (got[k].double() - want[k].double()).abs().max().item() / mult
            print(f"{k}: max |partials - hypotheses| = {d:.3e} m")
            assert d <= E2E_ATOL, (k, d)


def test_evaluate_sequence_partials_p160_in_chunks_of_20():
    """P = 160, T = 2, two clips on one GPU: hypotheses sampled and reduced 20 at a time (torch's generator rewound
    between chunks, so every chunk keeps its slice of the unsharded run's noise) against the one-kernel evaluation"""
    from __graft_entry__ import make_model
    model, _ = make_model(160, 2, depth=2)
    want, n = run_sequence(model, 54)
    got, n2 = run_sequence(model, 54, gather="partials", hypothesis_chunk=20)
    assert n == n2 == 54
    compare_modes(got, want, 54)
    whole, _ = run_sequence(model, 54, gather="partials")
    for k in got:
        assert torch.equal(whole[k], got[k]), k


def test_partials_with_protocol2_keeps_the_full_gather():
    from __graft_entry__ import make_model
    model, _ = make_model(4, 1, depth=2)
    want, _ = run_sequence(model, 27, p2=True)
    got, _ = run_sequence(model, 27, p2=True, gather="partials", hypothesis_chunk=3)
    assert len(got) == 18
    compare_modes(got, want, 27)


def test_two_rank_partials_rehearsal_on_one_gpu(tmp_path):
    """Two real ranks sharing this box's one GPU over gloo (the states travel through the host), P = 5: a ragged 3 + 2
    split.  Both ranks must report the accumulators a single process computes with gather="hypotheses"."""
    import socket
    from __graft_entry__ import make_model
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "partials_rank_worker.py"),
                                       str(tmp_path / f"rank{r}.pt")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    model, _ = make_model(5, 2, depth=2)
    want, n = run_sequence(model, 54)
    r0, r1 = (torch.load(str(tmp_path / f"rank{r}.pt")) for r in range(2))
    assert r0["world"] == 2 and r0["local"] == [0, 3] and r1["local"] == [3, 5] and r0["n"] == n
    for k in want:
        assert torch.equal(r0["sums"][k], r1["sums"][k]), k
    compare_modes(r0["sums"], want, 54)

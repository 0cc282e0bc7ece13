"""The per-frame chain's plan (harness._frame_plan), host side: every option that infer_sequence and evaluate_frames share is
refused by both before the model is touched, in the words recorded before the plan existed (tests/golden/frame_plan_messages.json:
recorded results, one message per entry point and case); the plan of a call with everything on holds what the chain used to
compute inline; ops._index_table through its four thin callers.  No GPU."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_plan_messages.json")
N, J, F = 30, 134, 27
NAN, INF = float("nan"), float("inf")


class Touched(Exception):
    """the stub model was asked for something only a run needs"""


class StubModel:
    frames, num_proposals = F, 2

    def parameters(self):
        raise Touched("parameters()")

    def __call__(self, *args, **kwargs):
        raise Touched("sampled")

    sample_chunks = __call__


def operands():
    from tests.golden import golden_util as gu
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS)
    return ds, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT


DROP = object()      # a base option taken away: the missing companion
# a call that is right in every option: a J-Agg fit per video frame with a smoothed trajectory, confidences given
BASE = dict(aggregate="reproj_fit", stride=9, trajectory=3, conf=torch.ones(N, J))
RADII = ("3", True, 0, 65, 2.5, NAN, INF)       # the wrong type, a bool, below, above, a fraction, NaN, inf
POSITIVE = ("1", True, 0, -1.0, NAN, INF)
BOTH = ("infer_sequence", "evaluate_frames")


def cases():
    """-> [(id, the options laid over BASE, the entry points the case is wrong for)]"""
    out = []

    def bad(option, values, only=BOTH, **context):
        for v in values:
            label = f"tensor{tuple(v.shape)}" if isinstance(v, torch.Tensor) else repr(v)
            tag = "".join(f",{k}={'-' if c is DROP else repr(c)}" for k, c in context.items())
            out.append((f"{option}={label}{tag}", {**context, option: v}, only))

    bad("stride", ("9", True, 0, 28, 65, 2.5, NAN))
    bad("trajectory", ("3", False, 0, 65, 2.5, NAN, INF))
    bad("focal", ("guess", True, 0, 1.0), trajectory=3)
    bad("focal", ("estimate",), trajectory=DROP)
    bad("repair", RADII)
    bad("repair", (3,), conf=DROP)
    bad("repair_threshold", ("0", True, -1.0, NAN, INF), repair=3)
    bad("repair_threshold", (-1.0,), screen=3)
    bad("screen", RADII)
    bad("screen", (3,), conf=DROP)
    bad("screen_gate", POSITIVE, screen=3)
    bad("screen_floor", POSITIVE, screen=3)
    bad("path_weight", ("1", True, -1.0, NAN, INF), stride=F)
    bad("path_weight", (1.0,), stride=F, aggregate="mean")
    bad("path_weight", (1.0,), stride=F, hypothesis_chunk=1)
    bad("path_weight", (1.0,), stride=9)
    bad("path_scope", ("frame", 0, True, None), stride=F, path_weight=1.0)
    bad("path_scope", ("video",))
    bad("pose_smooth", RADII)
    bad("pose_smooth", (4,), only=("infer_sequence",), stride=DROP, trajectory=DROP)
    bad("pose_smooth_floor", POSITIVE, pose_smooth=4)
    bad("bone_lengths", ("both", True, 0, torch.ones(J - 1), torch.ones(0), torch.ones(2, 3, J)))
    bad("bone_lengths", ("video",), only=("infer_sequence",), stride=DROP, trajectory=DROP)
    bad("bone_iterations", ("16", True, -1, 65, 2.5, NAN, INF), bone_lengths="video")
    bad("ground", ("3", False, 0, 65, 2.5, NAN, INF))
    bad("ground", (True,), trajectory=DROP)
    bad("ground_speed", POSITIVE, ground=True)
    bad("hypothesis_chunk", (0, -1, False, NAN))
    bad("aggregate", ("best", 0, True, None))
    return out


def call(entry, options, model=None):
    from pafuse_amd import harness
    ds, left, right = operands()
    kw = {k: v for k, v in {**BASE, **options}.items() if v is not DROP}
    model = StubModel() if model is None else model
    if entry == "infer_sequence":
        return harness.infer_sequence(model, ds, torch.zeros(N, J, 2), left, right, cam=torch.ones(9), **kw)
    return harness.evaluate_frames(model, ds, torch.zeros(N, J, 2), torch.zeros(N, J, 3), torch.ones(9), left, right, **kw)


def test_the_base_call_is_right_in_every_option():
    for entry in BOTH:
        with pytest.raises(Touched):
            call(entry, {})


def test_every_shared_option_is_refused_by_both_entry_points_in_the_recorded_words():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    table = cases()
    assert sorted(recorded) == sorted(name for name, _, _ in table) and len(recorded) == len(table)
    for name, options, only in table:
        assert sorted(recorded[name]) == sorted(only), name
        for entry in only:
            with pytest.raises(ValueError) as caught:       # a Touched stub would not be a ValueError
                call(entry, options)
            assert str(caught.value) == recorded[name][entry], (name, entry)


def test_the_plan_of_a_call_with_everything_on():
    from pafuse_amd import harness
    ds, left, right = operands()
    lengths = torch.full((J,), 0.25)
    plan = harness._frame_plan(F, ds, left, right, cam=torch.ones(9), traj=None, conf=torch.ones(N, J), aggregate="reproj_fit",
                               stride=9, hypothesis_chunk=2, spread=None, trajectory=5, focal="estimate", repair=7,
                               repair_threshold=0.25, pose_smooth=4, pose_smooth_floor=0.002, bone_lengths=lengths, bone_iterations=8,
                               screen=6, screen_gate=3.0, screen_floor=0.01, ground=True, ground_speed=0.02, ground_points=[1, 2])
    assert (plan.aggregate, plan.stride, plan.hypothesis_chunk) == ("reproj_fit", 9, 2)
    assert (plan.spread, plan.fold_spread) == (None, "cov")                     # the smoother and the bones need the covariance
    assert (plan.path_weight, plan.path_scope) == (None, "clip")
    assert (plan.trajectory, plan.smooth, plan.focal) == (True, 5, "estimate")
    assert plan.pose_smooth == (4, 0.002)
    assert plan.screen == (6, 3.0, 0.01) and (plan.repair, plan.threshold) == (7, 0.25)
    assert plan.ground == dict(points=[1, 2], radius=3, speed=0.02, passes=3, gate=2.5, floor=0.005, spread=0.03)
    assert sorted(plan.bones) == ["floor", "iterations", "lengths", "snap", "tables"]
    assert plan.bones["lengths"].dtype == torch.float32 and torch.equal(plan.bones["lengths"], lengths)
    assert (plan.bones["iterations"], plan.bones["snap"], plan.bones["floor"]) == (8, True, harness.BONE_FLOOR)
    for got, want in zip(plan.bones["tables"], harness._bone_tables(None, ds, left, right)):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    with pytest.raises(Exception):                                              # frozen
        plan.stride = 3
    # the switches that are off, and the defaults each entry point fills in
    off = harness._frame_plan(F, ds, left, right, cam=None, traj=None, conf=None, aggregate=None)
    assert (off.stride, off.trajectory, off.smooth, off.pose_smooth, off.bones, off.ground, off.screen, off.repair) == (None, False) + (None,) * 6
    assert harness._frame_plan(F, ds, left, right, cam=torch.ones(9), traj=None, conf=None, aggregate="mean", stride=9, trajectory=True,
                               spread="std").smooth is None
    video = harness._frame_plan(F, ds, left, right, cam=torch.ones(9), traj=None, conf=None, aggregate="reproj_fit", path_weight=2,
                                path_scope="video")
    assert (video.stride, video.path_weight, video.path_scope) == (F, 2.0, "video") and isinstance(video.path_weight, float)
    scored = harness._frame_plan(F, ds, left, right, cam=torch.ones(9), traj=None, conf=None, aggregate="mean", frames_only=True)
    assert scored.stride == F
    std = harness._frame_plan(F, ds, left, right, cam=None, traj=None, conf=None, aggregate="mean", stride=F, spread="std", pose_smooth=2)
    assert (std.spread, std.fold_spread) == ("std", "cov") and std.pose_smooth == (2, 1e-3)


# ------------------------------------------------------------------------------------- ops._index_table, through its callers
def tables():
    """-> [(the thin caller as f(table, J, device), a valid table, an invalid one, the words of the dtype refusal)]"""
    from pafuse_amd import ops
    return [(ops.bone_table, [-1, 0, 1, 2], [-1, 2, 0, 1], "bones: parent must be an integer table"),
            (lambda t, J, device=None: ops.bone_table(t, J, device, mirror=True), [-1, 2, 1, -1], [-1, 4, 1, -1],
             "bones: mirror must be an integer table"),
            (ops.repair_anchor_table, [-1, 0, 0, -1], [-1, 0, 1, -1], "repair_detections: anchor must be an integer table"),
            (ops.screen_mirror_table, [-1, 2, 1, -1], [-1, 2, 3, -1], "screen_detections: mirror must be an integer table"),
            (ops.ground_points, [1, 2, 3], [1, 4], "ground: points must be integers")]


def test_index_tables_are_validated_on_the_host():
    for make, good, bad, words in tables():
        for dtype in (torch.float32, torch.float64, torch.bool):
            with pytest.raises(ValueError) as caught:
                make(torch.tensor(good).to(dtype), 4)
            assert str(caught.value) == words
        with pytest.raises(ValueError):
            make(bad, 4)
        with pytest.raises(ValueError):
            make(torch.tensor(bad), 4)
        for given in (good, np.array(good, dtype=np.int64), torch.tensor(good), torch.tensor(good, dtype=torch.int16)):
            got = make(given, 4)
            assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == good


def test_index_tables_share_one_cache_of_sixteen_that_drops_the_oldest():
    from pafuse_amd import ops
    ops._table_cache.clear()
    anchors = [[-1] * k + [0] * (20 - k) for k in range(1, 19)]       # 18 different valid anchor tables
    first = ops.repair_anchor_table(anchors[0], 20, "cpu")
    assert isinstance(first, torch.Tensor) and first.dtype == torch.int32 and first.tolist() == anchors[0]
    assert ops.repair_anchor_table(torch.tensor(anchors[0]), 20, "cpu") is first and len(ops._table_cache) == 1      # a hit adds nothing
    # the same bytes under another tag are another entry: a mirror table of all -1 and an anchor table of all -1
    none = [-1] * 20
    a, m, b = ops.repair_anchor_table(none, 20, "cpu"), ops.screen_mirror_table(none, 20, "cpu"), ops.bone_table(none, 20, "cpu", mirror=True)
    assert a is not m and m is not b and a.tolist() == m.tolist() == b.tolist() == none and len(ops._table_cache) == 4
    feet = ops.ground_points([3, 4], 20, "cpu")
    assert feet.tolist() == [3, 4] and len(ops._table_cache) == 5
    for table in anchors[1:12]:                                       # 11 more: the cache is full
        ops.repair_anchor_table(table, 20, "cpu")
    assert len(ops._table_cache) == 16 and ops.repair_anchor_table(anchors[0], 20, "cpu") is first
    ops.repair_anchor_table(anchors[12], 20, "cpu")                   # the 17th drops the oldest, and only that
    assert len(ops._table_cache) == 16
    assert ops.repair_anchor_table(none, 20, "cpu") is a and ops.ground_points([3, 4], 20, "cpu") is feet
    again = ops.repair_anchor_table(anchors[0], 20, "cpu")            # gone: made anew, which drops the next oldest - `a`
    assert again is not first and again.tolist() == anchors[0] and len(ops._table_cache) == 16
    assert ops.repair_anchor_table(none, 20, "cpu") is not a

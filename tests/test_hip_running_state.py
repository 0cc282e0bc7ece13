"""The running state the three families of partial reductions share (evaluate._RunningState.fold behind
accumulate_partials, accumulate_procrustes and accumulate_poses): B=2, T=2, P=7, F=3, J=17 with three parts of 9, 5 and 3
joints, folded in chunks of 1, 3, 0 and 3 hypotheses - the slots grow after the first chunk and an empty chunk is folded -
against one fold of all seven.

Bit-equal: every entry the docstrings call independent of the cut.  The two that add per-chunk fp64 sums get the criterion
the families' own tests apply to a change of cut: p2_p_agg equal or adjacent in fp32 (test_hip_p2_partials.adjacent_count),
the pose mean equal or adjacent in fp32 (test_hip_pose_aggregate.equal_or_adjacent)."""
from types import SimpleNamespace

import pytest
import torch

from tests.test_hip_p2_partials import adjacent_count
from tests.test_hip_partials import same_bits
from tests.test_hip_pose_aggregate import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, P, F, J = 2, 2, 7, 3, 17
CHUNKS = (1, 3, 0, 3)


def dataset():
    parts = {"body": list(range(9)), "left": list(range(9, 14)), "right": list(range(14, 17))}
    return SimpleNamespace(parts_joint_indices=parts, root_indices={"body": 0, "left": 9, "right": 14},
                           parts_connection_indices={"left": 7, "right": 8})


@pytest.fixture(scope="module")
def z():
    g = torch.Generator().manual_seed(7)
    gt = torch.randn(B, F, J, 3, generator=g) * 0.3
    pred = gt[:, None, None] + torch.randn(B, T, P, F, J, 3, generator=g) * 0.05
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    traj = torch.randn(B, F, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    return tuple(t.contiguous().to(DEV) for t in (pred, gt, x2d, traj, cam))


def folds(z, family):
    """-> (fold(state, lo, hi) for hypotheses [lo, hi), the function's name, whether the family keeps a tail)"""
    from pafuse_amd import evaluate
    pred, gt, x2d, traj, cam = z
    if family == "poses":
        return (lambda s, lo, hi, at=None: evaluate.accumulate_poses(s, pred[:, :, lo:hi], lo if at is None else at, dataset(),
                                                                      x2d, traj, cam)), "accumulate_poses", False
    fn = evaluate.accumulate_partials if family == "partials" else evaluate.accumulate_procrustes
    return (lambda s, lo, hi, at=None: fn(s, pred[:, :, lo:hi], lo if at is None else at, gt, x2d, traj, cam, dataset())), \
        fn.__name__, True


def results(z, family, state):
    from pafuse_amd import evaluate
    pred, gt, x2d, traj, cam = z
    if family == "partials":
        return evaluate.evaluate_accumulators_sharded(None, None, P, gt, x2d, traj, cam, dataset(), state=state)
    if family == "poses":
        return evaluate.aggregate_poses_sharded(None, None, P, dataset(), state=state)
    p1 = evaluate.accumulate_partials(None, pred, 0, gt, x2d, traj, cam, dataset())      # the sums of the mean pose
    return evaluate.protocol2_accumulators_sharded(state, p1, P, gt, dataset())


@pytest.mark.parametrize("family", ["partials", "procrustes", "poses"])
def test_ragged_chunks_fold_like_one(z, family):
    fold, name, has_tail = folds(z, family)
    state, lo = None, 0
    for k, c in enumerate(CHUNKS):
        state = fold(state, lo, lo + c)
        lo += c
        assert (state.h0, state.count, len(state.tails)) == (0, lo, k + 1 if has_tail else 0), (k, c)
        if has_tail:
            assert [(h, t.shape[0]) for h, t in state.tails] == [(sum(CHUNKS[:i]), CHUNKS[i]) for i in range(k + 1)]
    assert lo == P
    whole = fold(None, 0, P)
    assert (whole.h0, whole.count, len(whole.tails)) == (0, P, 1 if has_tail else 0)
    got, want = results(z, family, state), results(z, family, whole)
    assert set(got) == set(want) and len(want) == {"partials": 6 + 2 * 3, "procrustes": 4, "poses": 3}[family]
    for k in want:
        if k == "p2_p_agg":
            print(f"p2_p_agg: steps adjacent rather than equal to the single fold: {adjacent_count(got[k], want[k])}")
        elif k == "mean":
            assert equal_or_adjacent(got[k], want[k])
            print(f"pose mean: elements that differ from the single fold: {int((got[k] != want[k]).sum())}")
        else:
            assert same_bits(got[k], want[k]), k
    with pytest.raises(ValueError, match=name):                  # a gap: the next chunk starts at P
        fold(state, 0, 1, at=P + 1)
    assert (state.h0, state.count) == (0, P)

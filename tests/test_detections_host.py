"""Host side of the repair of missing 2-D detections (no GPU): the numpy statement pafuse_amd/detections.py, its helpers, and the
refusals of pafuse_detections_repair and of the Python layers, which happen before the first HIP call.

Why the exact cases can be exact.  r = 3: (r+1)^2 = 16, so the taper g = (1 - d*d/16)^2 is dyadic (a multiple of 2^-8).  The planted
coordinates are multiples of 2^-6 below 32 and the confidences 1 or 0.5, so every product and sum of the walk is exact in fp64
(well below 2^53 units of 2^-20).  A series a + b*d gives Q0 = a*S0 + b*S1 and Q1 = a*S1 + b*S2, so S2*Q0 - S1*Q1 = a*D exactly
and the divide returns a, bit for bit.  The hand's OFFSET from its wrist is linear in the frame; the hand itself is not (the
wrist moves on a parabola), so the anchored fill is the truth and the absolute fill is not.

The dropout cap (unfilled share below 2 % at rate 0.2, run 10, radius 13 on 300 x 134) is a condition on the INPUT of the
comparisons elsewhere, not on the code: a joint is unfilled only if a stretch of 2*13 + 1 frames holds no observation of it
(or of its anchor), which runs of 10 starting with probability 0.02 per frame rarely build.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pafuse_amd import synthetic

E_ARG = -1


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def dataset():
    return SimpleNamespace(parts_joint_indices=synthetic.DATASET_PART_JOINTS, root_indices=synthetic.ROOT_INDICES,
                           parts_connection_indices=dict(synthetic.CONNECTION_INDICES))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def walk(N, J, seed, lost_share=0.3):
    """a smooth random walk per joint with random confidences; a share of the joints lost: confidence 0, coordinates 0"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((N, J, 2)) * 0.02, axis=0).astype(np.float32) + rng.uniform(-0.5, 0.5, (1, J, 2)).astype(np.float32)
    conf = rng.uniform(0.1, 1.0, (N, J)).astype(np.float32)
    lost = rng.random((N, J)) < lost_share
    x[lost] = 0
    conf[lost] = 0
    return x, conf, lost


def planted():
    """-> (x2d with the hand lost, conf, truth, lost frames): joint 0 the wrist, joint 1 the hand (see the module docstring)"""
    t = np.arange(40, dtype=np.float64)
    wrist = np.stack([t * t / 64, 3 - t / 8], axis=-1)
    hand = wrist + np.stack([t / 16 + 0.5, -t / 32], axis=-1)
    truth = np.stack([wrist, hand], axis=1).astype(np.float32)
    assert np.array_equal(truth.astype(np.float64), np.stack([wrist, hand], axis=1))       # exact in fp32
    conf = np.where((np.arange(80).reshape(40, 2) % 3) == 0, np.float32(0.5), np.float32(1)).astype(np.float32)
    lost = np.array([0, 5, 6, 7, 20, 38, 39])
    x = truth.copy()
    x[lost, 1] = 0
    conf[lost, 1] = 0
    return x, conf, truth, lost


# ------------------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("r", [1, 3, 13, 64])
def test_level_0_fills_are_the_smoother_bit_for_bit(r):
    from pafuse_amd import detections, trajectory
    x, conf, lost = walk(50, 7, seed=r)
    out, conf_out, status = detections.repair(x, conf, None, r)
    series = np.concatenate([x, np.zeros((50, 7, 1), np.float32)], axis=-1).transpose(1, 0, 2)     # [J,N,3]: x, y, 0
    smooth = trajectory.smooth(series, conf.T, r).transpose(1, 0, 2)[..., :2]                       # [N,J,2]
    filled = (status == 1) | (status == 2)
    assert filled.any() and np.array_equal(status != 0, lost)
    assert np.array_equal(bits(out[filled]), bits(smooth[filled]))
    assert np.isnan(smooth[status == 3]).all()                       # where the smoother has nothing, the repair has nothing
    assert np.array_equal(bits(out[~filled]), bits(x[~filled]))      # observed and unfilled joints: the same bits
    assert out.dtype == conf_out.dtype == np.float32 and status.dtype == np.uint8


def test_planted_hand_moves_with_its_wrist_exactly():
    from pafuse_amd import detections
    x, conf, truth, lost = planted()
    out, _, status = detections.repair(x, conf, [-1, 0], 3)
    assert np.array_equal(out, truth)
    assert (status[lost, 1] == 1).all() and int((status != 0).sum()) == len(lost)
    absolute, _, status0 = detections.repair(x, conf, [-1, -1], 3)
    off = np.abs(absolute.astype(np.float64) - truth).max()
    print(f"the absolute fill of the planted hand is off by {off:.3g}; the anchored fill by 0")
    assert not np.array_equal(absolute, truth) and np.array_equal(status0, status) and off > 0.05


def test_statuses():
    from pafuse_amd import detections
    N, r = 30, 2
    x = np.random.default_rng(0).uniform(-1, 1, (N, 3, 2)).astype(np.float32)
    conf = np.ones((N, 3), np.float32)
    conf[3:8, 0] = 0                 # a gap of five: frames 3, 4 and 6, 7 see one or two neighbours, frame 5 none
    conf[:, 1] = 0
    conf[10, 1] = 0.7                # a single observation: held within the radius, unfilled beyond
    x[~(conf > 0)] = 0
    out, conf_out, status = detections.repair(x, conf, None, r)
    assert status[3:8, 0].tolist() == [1, 2, 3, 2, 1]
    assert np.array_equal(out[4, 0], x[2, 0]) and np.array_equal(out[6, 0], x[8, 0])          # one neighbour: its value
    assert np.array_equal(bits(out[5, 0]), bits(x[5, 0]))                                     # no neighbour: the input's bits
    assert status[:, 1].tolist() == [3] * 8 + [2, 2, 0, 2, 2] + [3] * 17
    assert np.array_equal(out[[8, 9, 11, 12], 1], np.broadcast_to(x[10, 1], (4, 2)))
    # an anchor at status 3 takes its level-1 joint to status 3, although the joint has neighbours of its own
    conf2 = np.ones((N, 2), np.float32)
    conf2[3:8, 0] = 0
    conf2[5, 1] = 0
    x2 = x[:, :2].copy()
    x2[~(conf2 > 0)] = 0
    out2, _, status2 = detections.repair(x2, conf2, [-1, 0], r)
    assert status2[5, 0] == 3 and status2[5, 1] == 3 and np.array_equal(bits(out2[5, 1]), bits(x2[5, 1]))
    assert detections.repair(x2, conf2, None, r)[2][5, 1] == 1
    conf2[5, 1], conf2[4, 1] = 1, 0          # frame 4: the anchor is held (status 2), the joint is filled from frames 2, 3 and 6
    x2[4, 1] = 0                             # (frame 5 takes no part: the anchor has no value there)
    assert detections.repair(x2, conf2, [-1, 0], r)[2][4].tolist() == [2, 1]


def test_conf_out_is_zero_exactly_where_status_is_not_zero():
    from pafuse_amd import detections
    x, conf, _ = walk(40, 9, seed=3)
    conf[5, 5] = np.nan
    conf[20:31, 7] = 0               # a stretch without the joint, but for frame 25: held next to it, unfilled beyond
    conf[25, 7] = 0.5
    anchor = [-1, -1, 0, 0, 1, 1, 1, -1, 7]
    _, conf_out, status = detections.repair(x, conf, anchor, 2)
    assert set(np.unique(status)) == {0, 1, 2, 3}
    assert np.array_equal(conf_out == 0, status != 0) and np.array_equal(bits(conf_out[status == 0]), bits(conf[status == 0]))
    assert status[5, 5] != 0


@pytest.mark.parametrize("junk", [1e30, np.inf, np.nan, 12345.0])
def test_garbage_in_missing_joints_does_not_leak(junk):
    from pafuse_amd import detections
    x, conf, lost = walk(40, 9, seed=4)
    anchor = [-1, -1, 0, 0, 1, 1, 1, -1, 7]
    base = detections.repair(x, conf, anchor, 3)
    y = x.copy()
    y[lost] = np.float32(junk)
    y[lost & (np.arange(40)[:, None] % 2 == 0), 1] = -np.float32(junk)
    out, conf_out, status = detections.repair(y, conf, anchor, 3)
    assert np.array_equal(status, base[2]) and np.array_equal(conf_out, base[1])
    keep = status != 3
    assert np.array_equal(bits(out[keep]), bits(base[0][keep])) and np.isfinite(out[keep]).all()
    assert np.array_equal(bits(out[~keep]), bits(y[~keep]))          # unfilled: the input's bits, whatever they are
    z = x.copy()                                                      # a NaN coordinate under a positive confidence is missing
    seen = np.argwhere(~lost)[7]
    z[seen[0], seen[1], 1] = np.nan
    assert detections.repair(z, conf, anchor, 3)[2][seen[0], seen[1]] != 0


def test_idempotent():
    from pafuse_amd import detections
    x, conf, _ = walk(60, 9, seed=5)
    anchor = [-1, -1, 0, 0, 1, 1, 1, -1, 7]
    for r in (2, 13):
        out, conf_out, status = detections.repair(x, conf, anchor, r)
        again = detections.repair(out, conf_out, anchor, r)
        assert np.array_equal(bits(again[0]), bits(out)) and np.array_equal(again[2], status) and np.array_equal(again[1], conf_out)


def test_threshold():
    from pafuse_amd import detections
    x, conf, lost = walk(40, 5, seed=6)
    out, conf_out, status = detections.repair(x, conf, None, 3, threshold=0.4)
    assert np.array_equal(status != 0, ~(conf > np.float32(0.4))) and (conf_out[status != 0] == 0).all()
    assert int((status != 0).sum()) > int(lost.sum())
    conf[0, 0] = 0.4                                                # conf <= threshold is missing
    assert detections.repair(x, conf, None, 3, threshold=float(np.float32(0.4)))[2][0, 0] != 0
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="threshold"):
            detections.repair(x, conf, None, 3, threshold=bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="radius"):
            detections.repair(x, conf, None, bad)


def test_level_rule():
    from pafuse_amd import detections, ops
    J = 6
    assert detections.levels(None, J).tolist() == [False] * J
    assert detections.levels([-1, 0, 0, -7, 3, 3], J).tolist() == [False, True, True, False, True, True]
    table = [-1, 0, 1, 3, 6, 100]     # 2: nested (its anchor is anchored); 3: itself; 4, 5: out of range
    assert detections.levels(table, J).tolist() == [False, True, False, False, False, False]
    x, conf, _ = walk(30, J, seed=7)
    demoted = detections.repair(x, conf, table, 3)
    plain = detections.repair(x, conf, [-1, 0, -1, -1, -1, -1], 3)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(demoted, plain))
    lib()
    z = torch.zeros
    for bad in ([-1, 0, 1, -1, -1, -1], [-1, 0, -1, 3, -1, -1], [-1, 0, -1, -1, 6, -1], [-1, 0, -1, -1, -1, 100]):
        with pytest.raises(ValueError, match="anchor"):
            ops.repair_detections(z(30, J, 2), z(30, J), anchor=bad)
    with pytest.raises(ValueError, match="anchor"):
        ops.repair_detections(z(30, J, 2), z(30, J), anchor=[-1, 0])          # not [J]
    with pytest.raises(ValueError, match="anchor"):
        ops.repair_detections(z(30, J, 2), z(30, J), anchor=torch.zeros(J))   # not integers
    assert ops.repair_anchor_table([-1, 0, 0, -7, 3, 3], J).tolist() == [-1, 0, 0, -7, 3, 3]


def test_repair_anchors_and_plant_dropouts():
    from pafuse_amd import detections
    a = detections.repair_anchors(dataset())
    assert a.dtype == np.int32 and a.shape == (134,)
    assert (a[:24] == -1).all() and (a[24:92] == 1).all() and (a[92:113] == 10).all() and (a[113:] == 11).all()
    assert detections.levels(a, 134).tolist() == [False] * 24 + [True] * 110
    lost = detections.plant_dropouts(300, 134, 0.2, 10, 5)
    assert lost.dtype == bool and lost.shape == (300, 134)
    assert np.array_equal(lost, detections.plant_dropouts(300, 134, 0.2, 10, 5))
    assert not np.array_equal(lost, detections.plant_dropouts(300, 134, 0.2, 10, 6))
    share = lost.mean()
    print(f"plant_dropouts(0.2, 10) on 300 x 134 loses {share:.4f} of the joints")
    assert 0.15 <= share <= 0.20
    assert detections.plant_dropouts(5, 3, 0.0, 10, 0).sum() == 0
    x, conf = detections.drop(np.ones((300, 134, 2), np.float32), lost)
    assert (x[lost] == np.float32(detections.DROPPED_XY)).all() and (x[~lost] == 1).all()
    assert np.array_equal(conf, np.where(lost, 0, 1).astype(np.float32))


def test_planted_dropouts_are_nearly_all_filled_at_radius_13():
    """a condition on the input of the dropout comparisons: they do not run on nothing"""
    from pafuse_amd import detections
    rng = np.random.default_rng(11)
    truth = np.cumsum(rng.standard_normal((300, 134, 2)) * 0.01, axis=0).astype(np.float32)
    lost = detections.plant_dropouts(300, 134, 0.2, 10, 11)
    x, conf = detections.drop(truth, lost)
    out, _, status = detections.repair(x, conf, detections.repair_anchors(dataset()), 13)
    unfilled = (status[lost] == 3).mean()
    err = detections.repair_error(truth, out, lost, status, parts=dataset().parts_joint_indices)
    print(f"unfilled share of the lost joints at radius 13: {unfilled:.4f}; RMS error filled {err['filled']:.4g}, unfilled {err['unfilled']:.4g}")
    assert unfilled < 0.02
    assert np.array_equal(status != 0, lost) and np.array_equal(detections.counts(status), np.bincount(status.reshape(-1), minlength=4))
    assert err["n_filled"] + err["n_unfilled"] == int(lost.sum()) and set(err["parts"]) == set(dataset().parts_joint_indices)
    assert sum(p["n_filled"] for p in err["parts"].values()) == err["n_filled"]
    assert err["filled"] < err["unfilled"]         # a filled joint is nearer the truth than DROPPED_XY is


# ------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    assert L.pafuse_abi_version() == 8
    buf = (C.c_float * 256)()
    p = C.addressof(buf)
    q, c, cq, s = p + 256, p + 512, p + 640, p + 768
    ok = [p, c, None, 2, 3, 13, 0.0, q, cq, s, None]     # x2d, conf, anchor, N, J, radius, threshold, out, conf_out, status, stream
    cases = [(0, None), (1, None), (7, None), (9, None), (3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, 65), (5, -1),
             (6, -0.5), (6, float("nan")), (6, float("inf")), (7, p), (8, c)]
    for i, v in cases:
        a = list(ok)
        a[i] = v
        assert L.pafuse_detections_repair(*a) == E_ARG, (i, v)
        assert b"detections_repair" in L.pafuse_last_error(), (i, v)
    a = list(ok)
    a[3], a[4] = 2 ** 31 - 1, 2 ** 31 - 1                # N*J / 256 workgroups do not fit a grid
    assert L.pafuse_detections_repair(*a) == E_ARG and b"grid" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    lib()
    from pafuse_amd import harness, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.repair_detections(z(4, 3, 2), z(4, 3))
    with pytest.raises(ValueError, match="conf must be"):
        ops.repair_detections(z(4, 3, 2), z(4, 2))
    with pytest.raises(ValueError, match="x2d must be"):
        ops.repair_detections(z(4, 3, 3), z(4, 3))
    for r in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="radius"):
            ops.repair_detections(z(4, 3, 2), z(4, 3), radius=r)
    for t in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            ops.repair_detections(z(4, 3, 2), z(4, 3), threshold=t)
    with pytest.raises(ValueError, match="want"):
        ops.repair_detections(z(4, 3, 2), z(4, 3), want=("x2d", "mean"))
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    seq, conf = z(60, 134, 2), z(60, 134)
    args = (model, dataset(), seq, [], [])
    with pytest.raises(ValueError, match="repair needs conf"):
        harness.infer_sequence(*args, repair=13)
    with pytest.raises(ValueError, match="repair needs conf"):
        harness.infer_sequence(*args, aggregate="mean", stride=9, repair=13)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="repair"):
            harness.infer_sequence(*args, conf=conf, repair=bad)
    with pytest.raises(ValueError, match="repair_threshold"):
        harness.infer_sequence(*args, conf=conf, repair=13, repair_threshold=-1.0)
    with pytest.raises(ValueError, match="conf must be"):
        harness.infer_sequence(*args, conf=z(60, 133), repair=13)
    with pytest.raises(ValueError, match="conf belongs"):               # unchanged without a repair
        harness.infer_sequence(*args, conf=conf)
    ev = (model, dataset(), seq, z(60, 134, 3), z(9), [], [])
    with pytest.raises(ValueError, match="repair needs conf"):
        harness.evaluate_frames(*ev, repair=13)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="repair"):
            harness.evaluate_frames(*ev, conf=conf, repair=bad)
    for bad in ((0.2, 10), (1.5, 10, 0), (0.2, 0, 0), 0.2):
        with pytest.raises(ValueError, match="drop"):
            harness.evaluate_frames(*ev, drop=bad)
    with pytest.raises(ValueError, match="radius"):
        harness.repair_detections(seq, conf, radius=0)
    with pytest.raises(ValueError, match="seq_2d must be"):
        harness.repair_detections(seq, z(60, 133))


def test_torch_op_has_a_schema_and_a_fake():
    import pafuse_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.pafuse.repair_detections.default._schema)
    assert "Tensor x2d, Tensor conf" in s and "[]? anchor=None" in s and "radius=13" in s and "float threshold=0." in s
    assert s.endswith("-> Tensor[]")
    with FakeTensorMode():
        x, conf, status = torch.ops.pafuse.repair_detections(torch.empty(5, 7, 2, device="cuda"), torch.empty(5, 7, device="cuda"),
                                                            [-1, 0, 0, 0, 0, 0, 0], 3)
        assert x.shape == (5, 7, 2) and conf.shape == status.shape == (5, 7) and x.device.type == "cuda"
        assert x.dtype == conf.dtype == torch.float32 and status.dtype == torch.uint8

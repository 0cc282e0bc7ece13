"""Host side of the frame-level evaluation (no GPU): the numpy statement pafuse_amd/framemetrics.py against the reference's
fp64 numbers (tests/golden/g23_frame_metrics.npz, written by tests/golden/make_golden_frames.py), its closed forms, its counting
rules, the host helpers of the harness and the refusals of pafuse_frame_errors / pafuse_frame_errors_reduce, which happen
before the first HIP call.

G23 tolerance: both sides are fp64 (eps 1.1e-16) over about 1e3 operations per number -> rtol 1e-12 leaves a margin of ~10x.
The closed forms use dyadic numbers (multiples of 2^-6 below 2^4): pose = gt + c(n) is exactly representable in fp32, every
difference, product, sum and square root (of 25 * 2^-12 and its like) is exact in fp64, the sums of equal terms k * v are exact,
and so is the final divide by the count -> compared with ==.
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.golden import golden_util as gu

E_ARG, E_SHAPE = -1, -2
PARTS = list(gu.DATASET_PART_JOINTS)
J = 134
Q = 2.0 ** -6


def dataset():
    return SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                           parts_connection_indices=dict(gu.CONNECTION_INDICES))


def tables(J_=J):
    """pbroot, part as numpy int32 [J_]: the real tables at J = 134; elsewhere parts of (up to) 32 consecutive joints, rooted at
    their first joint, numbered 0 .. 3 in turn"""
    if J_ == J:
        from pafuse_amd.evaluate import _part_table, _tables
        return _tables(dataset(), J, "cpu")[1].numpy(), _part_table(dataset(), J, "cpu").numpy()
    j = np.arange(J_)
    return ((j // 32) * 32).astype(np.int32), ((j // 32) % 4).astype(np.int32)


def metric(err_or_sums, cnt, k):
    """sum of sums / sum of counts of slot k over every leading axis but the first -> [T]"""
    s = err_or_sums[..., k].reshape(err_or_sums.shape[0], -1).sum(axis=1)
    c = cnt[..., k].reshape(cnt.shape[0], -1).sum(axis=1)
    return s / c


def dyadic_gt(N, J_=J, seed=0):
    """gt [N,J_,3] fp32: multiples of 2^-6 in [-2, 2), joint 0 at 0"""
    g = np.random.default_rng(seed)
    gt = (g.integers(-128, 128, size=(N, J_, 3)) * Q).astype(np.float32)
    gt[:, 0] = 0
    return gt


# ------------------------------------------------------------------------------------------------------- G23
def test_statement_matches_the_reference_in_fp64():
    from pafuse_amd import framemetrics as fm
    z = np.load(os.path.join(ROOT, "tests", "golden", "g23_frame_metrics.npz"))
    pose, gt = z["pose"], z["gt"]
    assert pose.dtype == gt.dtype == np.float32 and pose.shape == (2, 9, J, 3) and gt.shape == (9, J, 3)
    pbroot, part = tables()
    err, cnt = fm.frame_errors(pose, gt, None, None, pbroot, part, 4)
    sums, counts = fm.reduce(err, cnt)
    assert err.shape == cnt.shape == (2, 9, 10) and err.dtype == np.float64 and cnt.dtype == np.int32
    assert sums.shape == counts.shape == (2, 10) and counts.dtype == np.int64
    got = {"mpjpe": sums[:, 0] / counts[:, 0], "mpjve": sums[:, 1] / counts[:, 1], "accel": sums[:, 2] / counts[:, 2],
           "mpjpe_pb": sums[:, 6:].sum(axis=1) / counts[:, 6:].sum(axis=1)}
    got.update({"mpjpe_pb_" + p: sums[:, 6 + i] / counts[:, 6 + i] for i, p in enumerate(PARTS)})
    for k, v in got.items():
        rel = np.abs(v / z[k] - 1).max()
        print(f"{k}: statement {v.tolist()} reference {z[k].tolist()} rel {rel:.2g}")
        np.testing.assert_allclose(v, z[k], rtol=1e-12, atol=0)
    assert (counts[:, 0] == 9 * J).all() and (counts[:, 1] == 8 * J).all() and (counts[:, 2] == 7 * J).all()
    assert (counts[:, 6:].sum(axis=1) == 9 * J).all() and not err[..., 3:6].any() and not cnt[..., 3:6].any()


# ---------------------------------------------------------------------------------------------------- closed forms
def closed_form_cases(N=6, J_=J, T=2):
    """name -> (pose, gt, traj, gt_root, {slot: value expected of sum / count}), all exact"""
    gt = dyadic_gt(N, J_)
    n = np.arange(N, dtype=np.float64)[:, None]
    c0 = np.array([3, 4, 0]) * Q
    slope = np.array([0, 3, 4]) * Q
    a = np.array([4, 0, 3]) * Q
    root = (np.random.default_rng(1).integers(-64, 64, size=(N, 3)) * Q + np.array([0, 0, 4.0])).astype(np.float32)
    out = {}

    def pose_of(c):                                                  # c [N,3] -> pose [T,N,J_,3] = gt + c(n), exactly
        p = (gt.astype(np.float64) + c[:, None, :]).astype(np.float32)
        assert np.array_equal(p.astype(np.float64), gt.astype(np.float64) + c[:, None, :])
        return np.repeat(p[None], T, axis=0)

    const = np.broadcast_to(c0, (N, 3))
    out["constant"] = (pose_of(const), gt, None, None, {0: 5 * Q, 1: 0.0, 2: 0.0, 6: 0.0, 7: 0.0, 8: 0.0, 9: 0.0})
    out["linear"] = (pose_of(c0 + slope * n), gt, None, None, {1: 5 * Q, 2: 0.0})
    out["quadratic"] = (pose_of(c0 + slope * n + a * n * n), gt, None, None, {2: 10 * Q})
    traj = np.repeat((root.astype(np.float64) + c0).astype(np.float32)[None], T, axis=0)
    out["root"] = (pose_of(const), gt, traj, root, {0: 5 * Q, 3: 5 * Q, 4: 0.0, 5: 10 * Q})
    return out


@pytest.mark.parametrize("name", ["constant", "linear", "quadratic", "root"])
def test_closed_forms_are_exact(name):
    from pafuse_amd import framemetrics as fm
    pose, gt, traj, gt_root, want = closed_form_cases()[name]
    pbroot, part = tables()
    err, cnt = fm.frame_errors(pose, gt, traj, gt_root, pbroot, part, 4)
    sums, counts = fm.reduce(err, cnt)
    for k, v in want.items():
        assert (counts[:, k] > 0).all()
        assert (sums[:, k] / counts[:, k] == v).all(), (name, k, sums[:, k] / counts[:, k], v)
        defined = cnt[..., k] > 0                                    # and frame by frame
        assert (err[..., k][defined] / cnt[..., k][defined] == v).all()


# ---------------------------------------------------------------------------------------------------------- counts
def random_case(T, N, J_, seed, with_traj=True):
    g = np.random.default_rng(seed)
    gt = (g.standard_normal((N, J_, 3)) * 0.3).astype(np.float32)
    gt[:, 0] = 0
    pose = (gt[None] + g.standard_normal((T, N, J_, 3)) * 0.05).astype(np.float32)
    pose[:, :, 0] = 0
    if not with_traj:
        return pose, gt, None, None
    root = (g.standard_normal((N, 3)) * 0.1 + np.array([0, 0, 4.0])).astype(np.float32)
    traj = (root[None] + g.standard_normal((T, N, 3)) * 0.02).astype(np.float32)
    return pose, gt, traj, root


def test_short_videos_have_no_differences():
    from pafuse_amd import framemetrics as fm
    pbroot, part = tables()
    err, cnt = fm.frame_errors(*random_case(2, 1, J, 3), pbroot, part, 4)
    assert not cnt[..., 1].any() and not cnt[..., 2].any() and not cnt[..., 4].any() and (cnt[..., 0] == J).all() and (cnt[..., 3] == 1).all()
    assert not err[..., 1].any() and not err[..., 2].any() and not err[..., 4].any()
    err, cnt = fm.frame_errors(*random_case(2, 2, J, 4), pbroot, part, 4)
    assert not cnt[..., 2].any() and not err[..., 2].any()
    assert (cnt[:, 0, 1] == 0).all() and (cnt[:, 1, 1] == J).all() and (cnt[:, 1, 4] == 1).all()


def test_a_nan_joint_leaves_its_own_terms_only():
    from pafuse_amd import framemetrics as fm
    pbroot, part = tables()
    N, m, j = 7, 3, 40
    assert pbroot[j] != j
    pose, gt, traj, root = random_case(2, N, J, 5)
    base_err, base_cnt = fm.frame_errors(pose, gt, traj, root, pbroot, part, 4)
    hurt = pose.copy()
    hurt[0, m, j, 1] = np.nan                                         # one component is enough
    err, cnt = fm.frame_errors(hurt, gt, traj, root, pbroot, part, 4)
    d = base_cnt.astype(np.int64) - cnt
    want = np.zeros_like(d)
    want[0, m, 0] = want[0, m, 5] = want[0, m, 6 + part[j]] = 1
    want[0, m, 1] = want[0, m + 1, 1] = 1
    want[0, m - 1, 2] = want[0, m, 2] = want[0, m + 1, 2] = 1
    assert np.array_equal(d, want)
    assert np.isfinite(err).all() and np.array_equal(err[1], base_err[1])
    # ... for that joint only: the same video without joint j's terms, recomputed on a gt that is NaN there in all those frames
    gone = gt.copy()
    gone[m, j] = np.nan                                               # a NaN in the gt counts like one in the pose - in every step
    err_gt, cnt_gt = fm.frame_errors(pose, gone, traj, root, pbroot, part, 4)
    assert np.array_equal(cnt_gt[0], cnt[0]) and np.array_equal(err_gt[0], err[0]) and np.array_equal(cnt_gt[1], cnt[0])


def test_a_nan_part_root_takes_its_part_out_of_the_part_slot():
    from pafuse_amd import framemetrics as fm
    pbroot, part = tables()
    face = PARTS.index("face")
    jr = gu.ROOT_INDICES["face"]
    members = int((part == face).sum())
    pose, gt, traj, root = random_case(1, 5, J, 6)
    base_err, base_cnt = fm.frame_errors(pose, gt, traj, root, pbroot, part, 4)
    pose[0, 2, jr] = np.nan
    err, cnt = fm.frame_errors(pose, gt, traj, root, pbroot, part, 4)
    assert base_cnt[0, 2, 6 + face] == members and cnt[0, 2, 6 + face] == 0 and err[0, 2, 6 + face] == 0.0
    for i in range(4):                                                # the other parts keep their joints (the root joint itself is the face's)
        if i != face:
            assert cnt[0, 2, 6 + i] == base_cnt[0, 2, 6 + i] and err[0, 2, 6 + i] == base_err[0, 2, 6 + i]
    assert part[jr] == face
    assert cnt[0, 2, 0] == J - 1 and np.array_equal(cnt[0, [0, 4]], base_cnt[0, [0, 4]])


def test_an_all_nan_frame_and_a_nan_traj_row():
    from pafuse_amd import framemetrics as fm
    pbroot, part = tables()
    N = 6
    pose, gt, traj, root = random_case(2, N, J, 7)
    pose[1, 2] = np.nan
    traj[0, 4, 2] = np.nan
    err, cnt = fm.frame_errors(pose, gt, traj, root, pbroot, part, 4)
    assert np.isfinite(err).all()
    joints = [0, 1, 2, 5, 6, 7, 8, 9]                                 # every slot summed over joints; the root's two see traj only
    assert not cnt[1, 2, joints].any() and not err[1, 2, joints].any() and cnt[1, 2, 3] == 1 and cnt[1, 2, 4] == 1
    assert cnt[1, 3, 1] == 0 and cnt[1, 1, 2] == 0 and cnt[1, 3, 2] == 0 and cnt[1, 4, 1] == J and cnt[1, 4, 2] == J
    assert cnt[0, 4, 3] == 0 and cnt[0, 4, 4] == 0 and cnt[0, 5, 4] == 0 and cnt[0, 4, 5] == 0 and err[0, 4, 3] == 0.0
    assert cnt[0, 4, 0] == J and cnt[0, 3, 4] == 1 and cnt[0, 3, 5] == J and cnt[1, 4, 3] == 1
    nt_err, nt_cnt = fm.frame_errors(pose, gt, None, None, pbroot, part, 4)
    assert not nt_err[..., 3:6].any() and not nt_cnt[..., 3:6].any()
    keep = [0, 1, 2, 6, 7, 8, 9]
    assert np.array_equal(nt_err[..., keep], err[..., keep]) and np.array_equal(nt_cnt[..., keep], cnt[..., keep])


# -------------------------------------------------------------------------------------------------- host interface
def test_reduce_is_the_ordered_sum():
    from pafuse_amd import framemetrics as fm
    g = np.random.default_rng(8)
    for N in (1, 5, 64, 70, 200):
        err = g.uniform(0, 3, (2, N, 7))
        cnt = g.integers(0, 135, (2, N, 7)).astype(np.int32)
        sums, counts = fm.reduce(err, cnt)
        want = np.zeros((2, 7))
        for t in range(2):
            for k in range(7):
                lanes = [0.0] * 64
                for n in range(N):                                    # lane n % 64 adds its frames in ascending order
                    lanes[n % 64] = lanes[n % 64] + err[t, n, k]
                for o in (32, 16, 8, 4, 2, 1):
                    lanes = [lanes[i] + lanes[i ^ o] for i in range(64)]
                want[t, k] = lanes[0]
        assert np.array_equal(sums, want) and np.array_equal(counts, cnt.astype(np.int64).sum(axis=1))


def test_seam_profile_on_a_hand_made_map():
    from pafuse_amd import harness
    err = torch.zeros(1, 7, 2, dtype=torch.float64)
    cnt = torch.zeros(1, 7, 2, dtype=torch.int32)
    err[0, :, 0] = torch.tensor([1.0, 2.0, 3.0, 5.0, 7.0, 0.0, 13.0])      # frame 5: no participant, sum 0.0
    cnt[0, :, 0] = torch.tensor([1, 2, 1, 1, 2, 0, 1])
    got = harness.seam_profile(err, cnt, 3)
    assert got.shape == (1, 3) and got.dtype == torch.float64
    assert got[0].tolist() == [(1.0 + 5.0 + 13.0) / 3, (2.0 + 7.0) / 4, 3.0 / 1]
    assert torch.isnan(harness.seam_profile(err, cnt, 3, slot=1)).all()                  # nothing counted
    assert harness.seam_profile(err, cnt, 27).shape == (1, 27)
    with pytest.raises(ValueError):
        harness.seam_profile(err, cnt, 3, slot=2)
    rep = harness.frame_report({"mpjpe": torch.tensor([0.5, 1.0], dtype=torch.float64), "mpjve": torch.tensor([0.0, 3.0], dtype=torch.float64)},
                               {"mpjpe": torch.tensor([5, 4]), "mpjve": torch.tensor([0, 4])})
    assert rep["mpjpe"] == [100.0, 250.0] and np.isnan(rep["mpjve"][0]) and rep["mpjve"][1] == 750.0
    lines = harness.format_frame_report(rep)
    assert "step 1 : Frame Error (MPJPE): 250.000000 mm" in lines and "step 1 : Frame Error (MPJVE): 750.000000 mm/frame" in lines


def test_evaluate_frames_refuses_before_the_library_loads():
    from pafuse_amd import harness
    z = torch.zeros
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    seq2, seq3 = z(60, J, 2), z(60, J, 3)
    call = lambda **kw: harness.evaluate_frames(model, None, kw.pop("seq2", seq2), kw.pop("seq3", seq3), kw.pop("cam", z(9)), [], [], **kw)
    with pytest.raises(ValueError, match="aggregate"):
        call(aggregate=None)
    with pytest.raises(ValueError, match="aggregate"):
        call(aggregate="best")
    for bad in (0, 28, 2.5, True):
        with pytest.raises(ValueError, match="stride"):
            call(stride=bad)
    for bad in (0, 65, 2.5, False):
        with pytest.raises(ValueError, match="trajectory"):
            call(trajectory=bad)
    with pytest.raises(ValueError, match="cam"):
        call(cam=None)
    with pytest.raises(ValueError, match="seq_3d"):
        call(seq3=z(61, J, 3))
    with pytest.raises(ValueError, match="conf belongs"):
        call(conf=z(60, J))
    with pytest.raises(ValueError, match="conf must be"):
        call(conf=z(60, J - 1), trajectory=3)
    with pytest.raises(ValueError, match="hypothesis_chunk"):
        call(hypothesis_chunk=0)


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import evaluate, ops
    from pafuse_amd._lib import PafuseError
    z = torch.zeros
    i32 = lambda n: z(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.frame_errors(z(1, 2, 3, 3), z(2, 3, 3), i32(3), i32(3), 1)
    with pytest.raises(ValueError, match="must match"):
        ops.frame_errors(z(1, 2, 3, 3), z(2, 4, 3), i32(3), i32(3), 1)
    with pytest.raises(ValueError, match="must match"):
        ops.frame_errors(z(1, 2, 3, 3), z(2, 3, 3), i32(3), i32(3), 1, traj=z(1, 3, 3), gt_root=z(2, 3))
    with pytest.raises(ValueError, match="come together"):
        ops.frame_errors(z(1, 2, 3, 3), z(2, 3, 3), i32(3), i32(3), 1, traj=z(1, 2, 3))
    for bad in (0, 5, 1.5, True):
        with pytest.raises(ValueError, match="num_parts"):
            ops.frame_errors(z(1, 2, 3, 3), z(2, 3, 3), i32(3), i32(3), bad)
    with pytest.raises(PafuseError, match="no CPU fallback"):
        evaluate.frame_metrics(z(1, 2, J, 3), z(2, J, 3), dataset())


def test_header_and_bindings_name_the_entries():
    from pafuse_amd import _lib
    with open(os.path.join(ROOT, "include", "pafuse_hip.h")) as f:
        header = f.read()
    for name in ("pafuse_frame_errors", "pafuse_frame_errors_reduce"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pafuse_frame_errors"][1]) == 13 and len(_lib.SIGNATURES["pafuse_frame_errors_reduce"][1]) == 8
    assert _lib.ABI_VERSION == 8 and re.search(r"#define PAFUSE_ABI_VERSION 8\b", header)


def test_torch_op_has_a_schema_and_a_fake():
    import pafuse_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.pafuse.frame_errors.default._schema)
    assert "Tensor? traj=None" in s and "Tensor? gt_root=None" in s and "num_parts" in s
    with FakeTensorMode():
        pose = torch.empty(2, 5, 7, 3, device="cuda")
        tab = torch.empty(7, device="cuda", dtype=torch.int32)
        sums, counts, err, cnt = torch.ops.pafuse.frame_errors(pose, torch.empty(5, 7, 3, device="cuda"), tab, tab, 4)
        assert sums.shape == counts.shape == (2, 10) and err.shape == cnt.shape == (2, 5, 10)
        assert (sums.dtype, counts.dtype, err.dtype, cnt.dtype) == (torch.float64, torch.int64, torch.float64, torch.int32)


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    L = _lib.load()
    assert L.pafuse_abi_version() == 8
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    # pose, gt, traj, gt_root, pbroot, part, num_parts, T, N, J, err, cnt, stream
    ok = [p, p, p, p, p, p, 4, 1, 1, 1, p, p, None]
    for i in (0, 1, 4, 5, 10, 11):
        a = list(ok)
        a[i] = None
        assert L.pafuse_frame_errors(*a) == E_ARG, i
    for i in (2, 3):                                                 # traj without gt_root, and the reverse
        a = list(ok)
        a[i] = None
        assert L.pafuse_frame_errors(*a) == E_ARG, i
    for i in (7, 8, 9):
        for v in (0, -1):
            a = list(ok)
            a[i] = v
            assert L.pafuse_frame_errors(*a) == E_ARG, (i, v)
    for v in (0, -1, 5):
        a = list(ok)
        a[6] = v
        assert L.pafuse_frame_errors(*a) == E_SHAPE, v
    assert b"frame_errors" in L.pafuse_last_error()
    ok = [p, p, 1, 1, 10, p, p, None]                                # err, cnt, T, N, K, sums, counts, stream
    for i in (0, 1, 5, 6):
        a = list(ok)
        a[i] = None
        assert L.pafuse_frame_errors_reduce(*a) == E_ARG, i
    for i in (2, 3):
        for v in (0, -1):
            a = list(ok)
            a[i] = v
            assert L.pafuse_frame_errors_reduce(*a) == E_ARG, (i, v)
    for v in (6, 11, 0):
        a = list(ok)
        a[4] = v
        assert L.pafuse_frame_errors_reduce(*a) == E_SHAPE, v
    assert b"frame_errors_reduce" in L.pafuse_last_error()

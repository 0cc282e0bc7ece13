"""Host side of J-Agg without a trajectory (no GPU): the numpy statement of the root fit (pafuse_amd/rootfit.py), the
refusals of pafuse_pose_partials_fit that happen before the first HIP call, the argument checks of
infer_sequence(aggregate="reproj_fit"), the detector confidences of load_pifpaf_keypoints and the example's options.

The recovery bound: on exact pinhole data the fit is exact up to the rounding of the detections to fp32 (relative 6e-8 of a
coordinate of size <= 1, seen through a depth of 4.5 m: a few 1e-8 m when 134 joints average it out, observed 7e-9 m for
J = 134 and 1.1e-7 m for J = 5) - the bound is 1e-6 m, 1/1000 of the millimetre the project reports in.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

E_ARG = -1
T_TRUE = np.array([0.3, -0.2, 4.5])
CAM = np.array([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001], dtype=np.float32)


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def planted(J, seed):
    """a pose with |X/Z| < 1 and Z + tz > 0, and its exact pinhole detections rounded to fp32"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((J, 3)) * 0.3).astype(np.float32)
    w[0] = 0
    X = w.astype(np.float64) + T_TRUE
    assert (X[:, 2] > 0).all() and (np.abs(X[:, :2] / X[:, 2:]) < 1).all()
    fx, fy, cx, cy = (np.float64(v) for v in CAM[:4])
    uv = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], axis=-1).astype(np.float32)
    return w, uv


@pytest.mark.parametrize("J", [134, 5])
def test_statement_recovers_a_planted_root(J):
    from pafuse_amd import rootfit
    w, uv = planted(J, seed=J)
    t = rootfit.fit_root(w, uv, None, CAM)
    err = np.abs(t - T_TRUE).max()
    print(f"J = {J}: |t - t_true| = {err:.3g} m")
    assert err <= 1e-6
    t32 = rootfit.fit_roots(w[None, None, None, None], uv[None, None], None, CAM)[0, 0, 0, 0]
    assert np.array_equal(t32, t.astype(np.float32))                    # the two spellings of the statement agree


def test_statement_ignores_zero_weight_joints_whatever_they_hold():
    from pafuse_amd import rootfit
    w, uv = planted(134, seed=7)
    lost = np.random.default_rng(8).permutation(134)[:40]
    c = np.ones(134, dtype=np.float32)
    c[lost] = 0
    uv0 = uv.copy()
    uv0[lost] = 0                                                       # what OpenPifPaf writes for a keypoint it did not find
    t = rootfit.fit_root(w, uv0, c, CAM)
    err = np.abs(t - T_TRUE).max()
    print(f"40 of 134 joints lost: |t - t_true| = {err:.3g} m")
    assert err <= 1e-6
    unweighted = rootfit.fit_root(w, uv0, None, CAM)                    # the same data without the weights: far off
    assert np.abs(unweighted - T_TRUE).max() > 0.1
    uv_nan = uv.copy()
    uv_nan[lost] = np.nan
    c_neg = c.copy()
    c_neg[lost[:20]], c_neg[lost[20:]] = -1.0, np.nan                   # negative and NaN weights count as 0
    assert np.array_equal(rootfit.fit_root(w, uv_nan, c_neg, CAM), t)


def test_statement_has_no_fit():
    from pafuse_amd import rootfit
    w, uv = planted(134, seed=9)
    one = np.zeros(134, dtype=np.float32)
    one[17] = 1
    assert rootfit.fit_root(w, uv, one, CAM) is None                    # one positive weight
    two = one.copy()
    two[50] = 0.5
    assert rootfit.fit_root(w, uv, two, CAM) is not None                # two are enough for three unknowns (four equations)
    same = np.tile(np.array([[0.25, -0.5]], dtype=np.float32), (134, 1))
    cam = np.array([2, 2, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)      # dyadic: den is exactly 0
    assert rootfit.fit_root(w, same, None, cam) is None                 # all detections coincident: one direction of sight
    assert rootfit.fit_root(w, uv, np.full(134, np.nan, dtype=np.float32), CAM) is None      # NaN weights
    t = rootfit.fit_roots(w[None, None, None, None], uv[None, None], one[None, None], CAM)
    assert t.shape == (1, 1, 1, 1, 3) and np.isnan(t).all()
    w_nan = w.copy()
    w_nan[3, 1] = np.nan
    assert rootfit.fit_root(w_nan, uv, None, CAM) is None               # t is not finite


def test_statement_sum_order_and_pick():
    from pafuse_amd import rootfit
    rng = np.random.default_rng(3)
    x = rng.standard_normal(134)
    lanes = np.zeros(64)
    for j in range(134):                                                # lane l: joints l, l + 64, l + 128 in ascending order
        lanes[j % 64] = lanes[j % 64] + x[j]
    for o in (32, 16, 8, 4, 2, 1):
        lanes = np.array([lanes[l] + lanes[l ^ o] for l in range(64)])
    assert (lanes == lanes[0]).all() and rootfit.lane_sum(x) == lanes[0]
    # the pick: hypothesis 1 is the pose that was projected, hypothesis 0 and 2 are 5 cm off; zero-weight joints have none
    w, uv = planted(134, seed=4)
    wb = np.stack([w + np.float32(0.05) * rng.standard_normal(w.shape).astype(np.float32), w,
                   w + np.float32(0.05) * rng.standard_normal(w.shape).astype(np.float32)])[None, None, :, None]
    c = np.ones((1, 1, 134), dtype=np.float32)
    c[0, 0, 100:] = 0
    cam = CAM.copy()
    cam[4:] = 0
    got = rootfit.pick(wb, uv[None, None], c, cam, h0=4)
    assert (got["idx"][0, 0, 0, 1:100] == 5).all() and (got["idx"][0, 0, 0, 100:] == -1).all()
    assert np.isinf(got["e2"][0, 0, 0, 100:]).all() and np.isnan(got["sel"][0, 0, 0, 100:]).all()
    assert np.array_equal(got["sel"][0, 0, 0, 1:100], w[1:100])
    assert np.abs(got["tfit"][0, 0, 1, 0] - T_TRUE).max() <= 1e-5


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    assert L.pafuse_abi_version() == 8
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    # pred, x2d, conf, cam, conn, B, T, P_r, F, J, h0, state, state_bytes, tfit, stream; B = T = P_r = F = J = 1: a 48-byte state
    ok = [p, p, p, p, p, 1, 1, 1, 1, 1, 0, p, 512, p, None]

    def fit(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_pose_partials_fit(*a)

    for i in (5, 6, 7, 8, 9, 10):                                      # B, T, P_r, F, J, h0 negative
        assert fit(**{f"a{i}": -1}) == E_ARG, i
    assert fit(a6=0) == E_ARG and fit(a8=0) == E_ARG and fit(a9=0) == E_ARG            # T, F, J zero
    assert fit(a1=None) == E_ARG and fit(a3=None) == E_ARG                               # x2d, cam: there is no mean-only fit
    assert fit(a1=None, a3=None) == E_ARG and fit(a1=None, a5=0) == E_ARG
    assert fit(a0=None) == E_ARG and fit(a4=None) == E_ARG                               # pred, conn
    assert fit(a0=None, a2=None, a13=None) == E_ARG                                      # conf and tfit are optional, pred is not
    assert fit(a11=None) == E_ARG and fit(a12=47) == E_ARG and fit(a11=p + 4) == E_ARG   # state: none, short, misaligned
    assert b"pose_partials_fit" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import evaluate, ops
    z = torch.zeros
    conn = z(3, dtype=torch.int32)
    with pytest.raises(ValueError):                                     # CPU tensors: no fallback
        ops.pose_partials_fit(z(1, 1, 2, 2, 3, 3), conn, 0, z(1, 2, 3, 2), z(9))
    with pytest.raises(ValueError, match="do not match"):
        ops.pose_partials_fit(z(1, 1, 2, 2, 3, 3), conn, 0, z(1, 2, 3, 2), z(9), conf=z(1, 2, 4))
    with pytest.raises(ValueError, match="do not match"):
        ops.pose_partials_fit(z(1, 1, 2, 2, 3, 3), conn, 0, z(1, 2, 3, 2), z(9), tfit=z(1, 1, 2, 2, 2))
    with pytest.raises(ValueError, match="x2d and cam"):
        ops.pose_partials_fit(z(1, 1, 2, 2, 3, 3), conn, 0, None, z(9))
    with pytest.raises(ValueError, match="fit=True"):
        evaluate.accumulate_poses(None, z(1, 1, 2, 2, 3, 3), 0, None, z(1, 2, 3, 2), z(1, 2, 3), z(9), fit=True)
    with pytest.raises(ValueError, match="fit=True"):
        evaluate.accumulate_poses(None, z(1, 1, 2, 2, 3, 3), 0, None, None, None, z(9), fit=True)
    with pytest.raises(ValueError, match="fit=True"):
        evaluate.accumulate_poses(None, z(1, 1, 2, 2, 3, 3), 0, None, conf=z(1, 2, 3))
    state = evaluate.PoseState((1, 1, 2, 3), "cpu", True, fit=True)
    assert state.reproj and state.fit and not evaluate.PoseState((1, 1, 2, 3), "cpu", True).fit


def test_infer_sequence_refuses_before_touching_the_model():
    from pafuse_amd import harness
    seq = torch.zeros(30, 134, 2)
    cam, traj = torch.zeros(9), torch.zeros(30, 3)
    call = lambda **kw: harness.infer_sequence(None, None, seq, [], [], **kw)
    with pytest.raises(ValueError, match="reproj_fit"):
        call(aggregate="reproj_fit")                                    # no cam
    with pytest.raises(ValueError, match="reproj_fit"):
        call(aggregate="reproj_fit", cam=cam, traj=traj)                # a trajectory is what it does not take
    for bad in (torch.zeros(30, 133), torch.zeros(29, 134), torch.zeros(30, 134, 1), torch.zeros(134)):
        with pytest.raises(ValueError, match="conf"):
            call(aggregate="reproj_fit", cam=cam, conf=bad)
    with pytest.raises(ValueError, match="conf"):
        call(aggregate="mean", conf=torch.zeros(30, 134))               # the weights belong to the fit
    with pytest.raises(ValueError, match="reproj"):
        call(aggregate="reproj", cam=cam)                               # "reproj" keeps demanding its trajectory


def test_load_pifpaf_keypoints_with_conf(tmp_path):
    from pafuse_amd import harness
    rng = np.random.default_rng(5)
    path = tmp_path / "three.openpifpaf.json"
    rows = []
    with open(path, "w") as f:
        for i in range(3):
            flat = rng.uniform(0, 1000, (133, 3)).astype(np.float32)
            flat[:, 2] = rng.uniform(0.1, 1, 133)
            flat[40 + i] = 0                                            # a keypoint the detector did not find
            flat[11 if i == 1 else 12, 2] = 0.05                        # joints 12 / 13 after the shift: the hips
            rows.append(flat)
            f.write(json.dumps({"predictions": [{"keypoints": flat.reshape(-1).tolist()}]}) + "\n")
    plain = harness.load_pifpaf_keypoints(str(path))
    kps, conf = harness.load_pifpaf_keypoints(str(path), with_conf=True)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, kps)      # the default return value is unchanged
    assert kps.shape == (3, 134, 2) and conf.shape == (3, 134) and conf.dtype == np.float32
    for i, flat in enumerate(rows):
        assert np.array_equal(conf[i, 1:], flat[:, 2]) and np.array_equal(kps[i, 1:], flat[:, :2])
        assert conf[i, 0] == np.float32(0.05) == min(conf[i, 12], conf[i, 13])
        assert conf[i, 41 + i] == 0 and (kps[i, 41 + i] == 0).all()


def test_example_options():
    script = os.path.join(ROOT, "examples", "infer_in_the_wild.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "--reproj-fit FOCAL_PX" in out.stdout and "--aggregate {none,mean}" in out.stdout
    out = subprocess.run([sys.executable, script, "--reproj-fit", "0"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 2 and "--reproj-fit" in out.stderr


def test_torch_op_schema_and_fake():
    from pafuse_amd import torch_ops  # noqa: F401
    s = str(torch.ops.pafuse.aggregate_poses_fit.default._schema)
    assert "Tensor pred, Tensor conn, Tensor x2d, Tensor cam, Tensor? conf=None" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *shape, **kw: torch.empty(*shape, device="cuda", **kw)
        mean, pick, idx, tfit = torch.ops.pafuse.aggregate_poses_fit(e(2, 3, 5, 4, 134, 3), e(134, dtype=torch.int32),
                                                                     e(2, 4, 134, 2), e(9))
        assert tuple(mean.shape) == tuple(pick.shape) == (2, 3, 4, 134, 3) and tuple(idx.shape) == (2, 3, 4, 134)
        assert idx.dtype == torch.int32 and tuple(tfit.shape) == (2, 3, 5, 4, 3)

"""Host side of the covariance-weighted pose smoother (no GPU): the numpy statement
pafuse_amd/posesmooth.py against independent solvers, its degenerate cases, and the refusals of pafuse_pose_smooth and the
Python layers, which happen before the first HIP call.

Bounds.  Against np.linalg.lstsq on the whitened stacked system and against trajectory.local_line: 1e-12 m (a prototype of the
statement measured 3.4e-15 and 2.8e-16; the margin covers another, equally valid loop order).  A noiseless line: 2 fp32
steps of the largest coordinate - the inputs are rounded to fp32 and the output is rounded once.  The planted case is a relation
(weighted better than unweighted), not a number.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
FLOOR = 1e-3


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def pack(S):
    """[...,3,3] symmetric -> [...,6] xx xy xz yy yz zz"""
    return np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2], S[..., 2, 2]], axis=-1)


def unpack(c):
    c = np.asarray(c, dtype=np.float64)
    return np.stack([np.stack([c[..., 0], c[..., 1], c[..., 2]], -1), np.stack([c[..., 1], c[..., 3], c[..., 4]], -1),
                     np.stack([c[..., 2], c[..., 4], c[..., 5]], -1)], -2)


def random_cov(rng, shape):
    """random rotations of covariances with standard deviations 1 - 10 cm x (1, 0.3, 0.1) -> fp32 [*shape, 6]"""
    Q, _ = np.linalg.qr(rng.standard_normal(shape + (3, 3)))
    sd = rng.uniform(0.01, 0.10, shape)[..., None] * np.array([1.0, 0.3, 0.1])
    S = np.einsum("...ik,...k,...jk->...ij", Q, sd * sd, Q)
    return pack(0.5 * (S + np.swapaxes(S, -1, -2))).astype(np.float32)


def weights(cov32, floor=FLOOR):
    """fp32 cov [...,6] (None rows: zeros) -> W = inv(Sigma + floor^2 I) [...,3,3] fp64 by np.linalg.inv: NOT the statement's cofactors"""
    s2 = np.float64(np.float32(floor)) ** 2
    return np.linalg.inv(unpack(cov32) + s2 * np.eye(3))


def taper(d, r):
    return (1.0 - (d * d) / float((r + 1) * (r + 1))) ** 2


def lstsq_value(y, W, part, n, r):
    """the local line's value at frame n of one joint's track y [N,3] with precisions W [N,3,3] over the frames in `part`:
    np.linalg.lstsq on the whitened stacked system, one block R_m [d*I, I] per frame with R_m^T R_m = g*W_m"""
    N = y.shape[0]
    rows, rhs = [], []
    for m in range(max(0, n - r), min(N - 1, n + r) + 1):
        if not part[m]:
            continue
        d = float(m - n)
        R = np.linalg.cholesky(taper(d, r) * W[m]).T
        rows.append(R @ np.concatenate([d * np.eye(3), np.eye(3)], axis=1))
        rhs.append(R @ y[m])
    x = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    return x[3:]


# ------------------------------------------------------------------------------------------- 1. against np.linalg.lstsq
@pytest.mark.parametrize("N,r", [(9, 3), (40, 13), (70, 64), (30, 1)])
def test_statement_is_the_whitened_least_squares_line(N, r):
    from pafuse_amd import posesmooth
    rng = np.random.default_rng(100 + N)
    T, J = 1, 3
    pose = (rng.standard_normal((T, N, J, 3)) * 0.3).astype(np.float32)
    cov = random_cov(rng, (T, N, J))
    value, code = posesmooth.smooth_f64(pose, cov, r, np.float32(FLOOR))
    assert (code == posesmooth.LINE).all()
    W = weights(cov)
    y = pose.astype(np.float64)
    worst = 0.0
    for j in range(J):
        for n in range(N):
            want = lstsq_value(y[0, :, j], W[0, :, j], np.ones(N, bool), n, r)
            worst = max(worst, float(np.abs(value[0, n, j] - want).max()))
    print(f"N={N} r={r}: max |statement - lstsq| = {worst:.3e} m")
    assert worst <= 1e-12
    out, code32 = posesmooth.smooth(pose, cov, r, FLOOR)
    assert out.dtype == np.float32 and np.array_equal(out, value.astype(np.float32)) and np.array_equal(code32, code)


# ------------------------------------------------------------------------------------------- 2. equal covariances cancel
@pytest.mark.parametrize("N,r", [(9, 3), (40, 13), (70, 64), (30, 1), (2, 5)])
def test_equal_isotropic_covariances_give_the_line_filter(N, r):
    from pafuse_amd import posesmooth, trajectory
    rng = np.random.default_rng(7 * N + r)
    T, J = 2, 4
    pose = (rng.standard_normal((T, N, J, 3)) * 0.3).astype(np.float32)
    y = np.moveaxis(pose.astype(np.float64), 1, 0)                             # local_line walks axis 0
    want, kind = trajectory.local_line(y, np.ones((N, T, J), bool), np.ones((N, T, J)), r)
    want = np.moveaxis(want, 0, 1)
    assert (kind == trajectory.LINE).all()
    none, code = posesmooth.smooth_f64(pose, None, r, np.float32(FLOOR))
    iso = np.zeros((T, N, J, 6), np.float32)
    iso[..., [0, 3, 5]] = np.float32(0.02 ** 2)
    same, code_iso = posesmooth.smooth_f64(pose, iso, r, np.float32(FLOOR))
    worst = max(float(np.abs(none - want).max()), float(np.abs(same - want).max()))
    print(f"N={N} r={r}: max |statement - local_line| = {worst:.3e} m")
    assert worst <= 1e-12 and (code == posesmooth.LINE).all() and (code_iso == posesmooth.LINE).all()
    zero = posesmooth.smooth_f64(pose, np.zeros((T, N, J, 6), np.float32), r, np.float32(FLOOR))
    assert np.array_equal(zero[0], none) and np.array_equal(zero[1], code)      # cov=None IS an all-zero cov, bit for bit
    a, b = posesmooth.smooth(pose, None, r, FLOOR), posesmooth.smooth(pose, np.zeros((T, N, J, 6), np.float32), r, FLOOR)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------- 3. constant velocity passes
@pytest.mark.parametrize("N,r", [(9, 3), (40, 13), (70, 64), (30, 1)])
def test_constant_velocity_comes_through_without_lag_or_end_shrinkage(N, r):
    from pafuse_amd import posesmooth
    rng = np.random.default_rng(N + r)
    T, J = 1, 5
    start, vel = rng.standard_normal((T, 1, J, 3)) * 0.3, rng.standard_normal((T, 1, J, 3)) * 0.02
    pose = (start + vel * np.arange(N)[None, :, None, None]).astype(np.float32)
    out, code = posesmooth.smooth(pose, random_cov(rng, (T, N, J)), r, FLOOR)
    step = np.spacing(np.float32(np.abs(pose).max()))
    assert (code == posesmooth.LINE).all()
    err = np.abs(out.astype(np.float64) - pose.astype(np.float64))
    print(f"N={N} r={r}: max error {err.max():.3e}, at the ends {err[:, [0, -1]].max():.3e}, fp32 step {step:.3e}")
    assert err.max() <= 2 * step                                              # frames 0 and N - 1 included


# ------------------------------------------------------------------------------------------- 4. the planted case
def planted(seed=0, N=60):
    """constant velocity, 5 mm noise, every 7th frame 8 cm uncertain in z - and the covariance that says so"""
    rng = np.random.default_rng(seed)
    J = 8
    truth = rng.standard_normal((1, 1, J, 3)) * 0.3 + rng.standard_normal((1, 1, J, 3)) * 0.01 * np.arange(N)[None, :, None, None]
    noise = rng.standard_normal((1, N, J, 3)) * 0.005
    cov = np.zeros((1, N, J, 6))
    cov[..., [0, 3, 5]] = 0.005 ** 2
    wide = np.arange(N) % 7 == 3
    noise[0, wide, :, 2] = rng.standard_normal((int(wide.sum()), J)) * 0.08
    cov[0, wide, :, 5] = 0.08 ** 2
    return truth, (truth + noise).astype(np.float32), cov.astype(np.float32)


@pytest.mark.parametrize("r", [3, 13])
def test_planted_uncertain_frames_are_carried_by_their_neighbours(r):
    from pafuse_amd import posesmooth
    truth, pose, cov = planted()
    rms = lambda a: float(np.sqrt(((a.astype(np.float64) - truth) ** 2).sum(-1).mean()))
    weighted, plain = posesmooth.smooth(pose, cov, r, FLOOR)[0], posesmooth.smooth(pose, None, r, FLOOR)[0]
    print(f"r={r}: raw {rms(pose) * 1e3:.2f} mm, plain line {rms(plain) * 1e3:.2f} mm, weighted {rms(weighted) * 1e3:.2f} mm")
    assert rms(weighted) < rms(plain) < rms(pose)


# ------------------------------------------------------------------------------------------- 5. degenerate cases
def test_one_frame_is_its_own_mean_and_two_frames_make_a_line():
    from pafuse_amd import posesmooth
    rng = np.random.default_rng(3)
    pose = (rng.standard_normal((2, 1, 5, 3)) * 0.3).astype(np.float32)
    for cov in (None, random_cov(rng, (2, 1, 5))):
        out, code = posesmooth.smooth(pose, cov, 4, FLOOR)
        assert (code == posesmooth.MEAN).all()
        assert np.abs(out.astype(np.float64) - pose).max() <= np.spacing(np.float32(np.abs(pose).max()))
    assert np.array_equal(posesmooth.smooth(pose, None, 4, FLOOR)[0], pose)    # W = I/s2 is diagonal: the solve returns y
    pose = (rng.standard_normal((1, 2, 5, 3)) * 0.3).astype(np.float32)
    out, code = posesmooth.smooth(pose, random_cov(rng, (1, 2, 5)), 1, FLOOR)
    assert (code == posesmooth.LINE).all()
    assert np.abs(out.astype(np.float64) - pose).max() <= 2 * np.spacing(np.float32(np.abs(pose).max()))   # a line through two points


def dense_value(y, W, part, n, r):
    """the same line by np.linalg.solve on the dense normal equations over the frames in `part`"""
    A, b = np.zeros((6, 6)), np.zeros(6)
    for m in range(max(0, n - r), min(len(y) - 1, n + r) + 1):
        if part[m]:
            d = float(m - n)
            X = np.concatenate([d * np.eye(3), np.eye(3)], axis=1)
            A += taper(d, r) * X.T @ W[m] @ X
            b += taper(d, r) * X.T @ W[m] @ y[m]
    return np.linalg.solve(A, b)[3:]


def test_a_missing_row_is_a_deleted_frame_and_stays_in_its_own_track():
    from pafuse_amd import posesmooth
    rng = np.random.default_rng(11)
    T, N, J, r = 2, 24, 4, 3
    pose = (rng.standard_normal((T, N, J, 3)) * 0.3).astype(np.float32)
    cov = random_cov(rng, (T, N, J))
    base, base_code = posesmooth.smooth(pose, cov, r, FLOOR)
    t0, n0, j0 = 1, 10, 2
    spoiled = []
    for what in ("pose", "cov", "indefinite"):
        p, c = pose.copy(), cov.copy()
        if what == "pose":
            p[t0, n0, j0, 1] = np.nan
        elif what == "cov":
            c[t0, n0, j0, 4] = np.nan
        else:
            c[t0, n0, j0] = pack(np.diag([1e-2, -1e-2, 1e-2]))                 # indefinite however small the floor
        spoiled.append(posesmooth.smooth(p, c, r, FLOOR))
    for out, code in spoiled[1:]:
        assert out.tobytes() == spoiled[0][0].tobytes() and np.array_equal(code, spoiled[0][1])
    out, code = spoiled[0]
    touched = np.zeros((T, N, J), bool)
    touched[t0, max(0, n0 - r):n0 + r + 1, j0] = True
    assert np.array_equal(out[~touched], base[~touched]) and np.array_equal(code[~touched], base_code[~touched])
    assert (out[touched] != base[touched]).any(axis=-1).all() and not np.isnan(out).any() and (code == posesmooth.LINE).all()
    part = np.ones(N, bool)
    part[n0] = False
    W = weights(cov)
    for n in range(n0 - r, n0 + r + 1):                                       # frame n0 itself is filled from its neighbours
        want = dense_value(pose[t0, :, j0].astype(np.float64), W[t0, :, j0], part, n, r)
        assert np.abs(out[t0, n, j0] - want).max() <= 2 * np.spacing(np.float32(1.0)), n


def test_nothing_in_reach_is_nan_and_a_lone_neighbour_is_held():
    from pafuse_amd import posesmooth
    rng = np.random.default_rng(12)
    T, N, J, r = 1, 12, 3, 2
    pose = (rng.standard_normal((T, N, J, 3)) * 0.3).astype(np.float32)
    cov = random_cov(rng, (T, N, J))
    pose[0, 2:9, 1] = np.nan                                                   # frames 2 .. 8 of joint 1
    pose[0, 5, 1] = (0.1, -0.2, 0.3)                                           # ... except frame 5: 4, 5, 6 see only it
    pose[0, :, 2] = np.nan
    cov[0, :, 2] = np.nan
    out, code = posesmooth.smooth(pose, cov, r, FLOOR)
    assert (code[0, :, 0] == posesmooth.LINE).all()
    assert (code[0, :, 2] == posesmooth.NONE).all() and np.isnan(out[0, :, 2]).all()
    assert code[0, :, 1].tolist() == [1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1]      # 3 sees 1 and 5, 7 sees 5 and 9: lines
    for n in (4, 5, 6):
        assert np.abs(out[0, n, 1] - pose[0, 5, 1]).max() <= np.spacing(np.float32(0.3)), n
    pose[0, 5, 1] = np.nan
    out, code = posesmooth.smooth(pose, cov, r, FLOOR)
    assert code[0, :, 1].tolist() == [1, 1, 1, 2, 3, 3, 3, 2, 1, 1, 1, 1]
    assert np.isnan(out[0, 4:7, 1]).all() and not np.isnan(out[0, [3, 7], 1]).any()
    big = np.full((1, 3, 1, 3), 3.3e38, np.float32)                            # the line through (a, a, -a) is about 1.2 a at frame 0:
    big[0, 2] = -3.3e38                                                        # finite in fp64, not in fp32
    out, code = posesmooth.smooth(big, None, 2, FLOOR)
    assert code[0, 0, 0] == posesmooth.NONE and code[0, 1, 0] == posesmooth.LINE
    assert np.isnan(out[code == posesmooth.NONE]).all() and np.isfinite(out[code != posesmooth.NONE]).all()


def test_statement_refuses_bad_arguments():
    from pafuse_amd import posesmooth
    pose = np.zeros((1, 4, 2, 3), np.float32)
    for r in (0, 65, -1, True, 2.5, None):
        with pytest.raises(ValueError, match="1 .. 64"):
            posesmooth.smooth(pose, None, r, FLOOR)
    for f in (0.0, -1e-3, float("nan"), float("inf"), 1e-60, True, None):
        with pytest.raises(ValueError, match="floor"):
            posesmooth.smooth(pose, None, 3, f)
    with pytest.raises(ValueError, match="cov"):
        posesmooth.smooth(pose, np.zeros((1, 4, 2, 5), np.float32), 3, FLOOR)
    with pytest.raises(ValueError, match="pose"):
        posesmooth.smooth(pose[0], None, 3, FLOOR)


# ------------------------------------------------------------------------------------------- the C ABI, no device
CTYPES = {"const float *": C.c_void_p, "float *": C.c_void_p, "uint8_t *": C.c_void_p, "void *": C.c_void_p,
          "int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t}


def test_the_entry_is_declared_exported_and_bound_as_the_header_says():
    from pafuse_amd import _lib, ops, torch_ops  # noqa: F401
    L = lib()
    with open(os.path.join(ROOT, "include", "pafuse_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint pafuse_pose_smooth\(([^;]*)\);", header)
    assert m and hasattr(L, "pafuse_pose_smooth")
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = [re.sub(r"\s*\w+$", "", p).strip() for p in params]     # drop the parameter's name
    restype, argtypes = _lib.SIGNATURES["pafuse_pose_smooth"]
    assert restype is C.c_int and argtypes == [CTYPES[k] for k in kinds], kinds
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == ["pose", "cov", "T", "N", "J", "radius", "floor", "out", "code",
                                                                      "workspace", "workspace_bytes", "stream"]
    assert _lib.ABI_VERSION == 8 and L.pafuse_abi_version() == 8              # a new entry only: no struct changed
    assert re.search(r"\bsize_t pafuse_pose_smooth_workspace_bytes\(int32_t T, int32_t N, int32_t J\);", header)
    assert _lib.SIGNATURES["pafuse_pose_smooth_workspace_bytes"] == (C.c_size_t, [C.c_int32] * 3)
    assert L.pafuse_pose_smooth_workspace_bytes(10, 594, 134) == 10 * 594 * 134 * 48 == ops.smooth_poses_workspace_bytes(10, 594, 134)
    assert L.pafuse_pose_smooth_workspace_bytes(0, 5, 5) == L.pafuse_pose_smooth_workspace_bytes(5, -1, 5) == 0
    assert L.pafuse_pose_smooth_workspace_bytes(2000, 5000, 134) == 2000 * 5000 * 134 * 48      # past 2^32: no int overflow
    assert callable(ops.smooth_poses)


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    assert L.pafuse_abi_version() == 8
    buf = (C.c_float * 256)()
    p = C.addressof(buf)
    q, w = p + 512, p + 768
    ok = [p, p, 1, 1, 1, 3, 1e-3, q, q, w, 48, None]     # pose, cov, T, N, J, radius, floor, out, code, workspace, its bytes, stream
    bad = [(0, None), (7, None), (7, p)] + [(i, v) for i in (2, 3, 4) for v in (0, -1)] + [(5, 0), (5, 65), (5, -1)]
    bad += [(6, v) for v in (0.0, -1e-3, float("nan"), float("inf"), -float("inf"))]
    bad += [(9, None), (9, w + 4), (10, 47), (10, 0), (3, 2)]                   # no, a misaligned, a short workspace (N = 2 needs 96)
    for i, v in bad:
        a = list(ok)
        a[i] = v
        assert L.pafuse_pose_smooth(*a) == E_ARG, (i, v)
        assert b"pose_smooth" in L.pafuse_last_error()
    a = list(ok)
    a[1] = a[8] = None                             # a null cov and a null code are accepted: with a bad radius the refusal names it
    a[5] = 0
    assert L.pafuse_pose_smooth(*a) == E_ARG and b"radius" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import harness, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.smooth_poses(z(1, 4, 2, 3), None, 3)
    for r in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="1 .. 64"):
            ops.smooth_poses(z(1, 4, 2, 3), None, r)
    for f in (0.0, -1.0, float("nan"), float("inf"), 1e-60, True, "1"):
        with pytest.raises(ValueError, match="floor"):
            ops.smooth_poses(z(1, 4, 2, 3), None, 3, floor=f)
    with pytest.raises(ValueError, match="cov"):
        ops.smooth_poses(z(1, 4, 2, 3), z(1, 4, 2, 3), 3)
    with pytest.raises(ValueError, match="pose must be"):
        ops.smooth_poses(z(4, 2, 3), None, 3)
    t = z(1, 4, 2, 3)
    with pytest.raises(ValueError, match="alias"):
        ops.smooth_poses(t, None, 3, out=t)
    for r in (0, 65, 2.5, True, None):
        with pytest.raises(ValueError, match="1 .. 64"):
            harness.smooth_poses(t, None, radius=r)
    for f in (0.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="floor"):
            harness.smooth_poses(t, None, radius=3, floor=f)
    with pytest.raises(ValueError, match="cov must be"):
        harness.smooth_poses(t, z(1, 4, 2, 5), radius=3)
    with pytest.raises(ValueError, match="poses must be"):
        harness.smooth_poses(z(4, 2, 3), None, radius=3)
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    seq = z(60, 134, 2)
    with pytest.raises(ValueError, match="harness.smooth_poses"):               # no stride
        harness.infer_sequence(model, None, seq, [], [], aggregate="mean", pose_smooth=3)
    with pytest.raises(ValueError, match="pose_smooth needs aggregate"):
        harness.infer_sequence(model, None, seq, [], [], stride=9, pose_smooth=3)
    for bad in (0, 65, 2.5, True, False):
        with pytest.raises(ValueError, match="1 .. 64"):
            harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, pose_smooth=bad)
        with pytest.raises(ValueError, match="1 .. 64"):
            harness.evaluate_frames(model, None, seq, z(60, 134, 3), z(9), [], [], pose_smooth=bad)
    for f in (0.0, -1e-3, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="finite number > 0"):
            harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, pose_smooth=3, pose_smooth_floor=f)
        with pytest.raises(ValueError, match="finite number > 0"):
            harness.evaluate_frames(model, None, seq, z(60, 134, 3), z(9), [], [], pose_smooth=3, pose_smooth_floor=f)


def test_torch_op_has_a_schema_and_a_fake():
    import pafuse_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.pafuse.pose_smooth.default._schema)
    assert "Tensor? cov" in s and re.search(r"[Ii]nt radius", s) and "float floor=0.001" in s and s.endswith("-> Tensor[]")
    with FakeTensorMode():
        pose = torch.empty(2, 5, 7, 3, device="cuda")
        out, code = torch.ops.pafuse.pose_smooth(pose, torch.empty(2, 5, 7, 6, device="cuda"), 3)
        assert out.shape == (2, 5, 7, 3) and out.dtype == torch.float32 and code.shape == (2, 5, 7) and code.dtype == torch.uint8
        out, code = torch.ops.pafuse.pose_smooth(pose, None, 13, 2e-3)
        assert out.device.type == "cuda" and code.device.type == "cuda"

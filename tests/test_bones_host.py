"""Bone lengths held constant along a video, on the host: the numpy statement pafuse_amd/bones.py (what bone_lengths_kernel and
bone_project_kernel are compared with on the device, tests/test_hip_bones.py), h3wb.bone_tables, and what the C ABI and the
Python layers refuse before anything touches the device.

The planted case (planted()): the H3WB tables, 60 frames, constant true bone lengths, directions that drift slowly, the root
exact (the poses of this project are root-relative: joint 0 is 0 with a zero covariance), every other joint with independent
Gaussian noise of 5 mm x U(0.5, 1.5) x (0.3, 0.3, 1.2) along x, y, z - four times wider along the viewing ray, the shape a
monocular lifter's hypotheses have - and that noise's covariance as `cov`.  The projection with the TRUE lengths must bring
the mean joint error of body and hands each below 0.8 x the raw error; the top-down snap alone must make both worse than raw.

Why the root is exact: every pose this project returns has joint 0 at 0 exactly (the evaluation subtracts it from the ground
truth as well), so noise on the root is not a case the product meets.  It is also not a case the method can help: the root is
pinned, so noise planted on it cannot be corrected and passes to the five bones that hang on it - measured with this statement
the body then ends at 0.86 - 0.89 x raw, converged or not (hands 0.69 - 0.76 x), which is above the bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pafuse_amd import bones, h3wb
from tests.conftest import ROOT

FLOOR = 1e-3
BODY, FACE, HANDS = np.arange(0, 24), np.arange(24, 92), np.arange(92, 134)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def packed(S):
    return np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2], S[..., 2, 2]], axis=-1).astype(np.float32)


def random_cov(rng, shape, lo=0.002, hi=0.02):
    Q, _ = np.linalg.qr(rng.standard_normal(shape + (3, 3)))
    sd = rng.uniform(lo, hi, shape)[..., None] * np.array([1.0, 0.4, 0.15])
    return np.einsum("...ik,...k,...jk->...ij", Q, sd * sd, Q)


def full(c6, floor=FLOOR):
    c = c6.astype(np.float64)
    s2 = float(np.float32(floor)) ** 2
    return np.array([[c[0] + s2, c[1], c[2]], [c[1], c[3] + s2, c[4]], [c[2], c[4], c[5] + s2]])


def planted(seed, N=60, sigma=0.005):
    rng = np.random.default_rng(seed)
    parent, mirror = h3wb.bone_tables(68)
    J = len(parent)
    L = np.where(parent >= 0, np.where(np.arange(J) >= 92, rng.uniform(0.02, 0.05, J), rng.uniform(0.1, 0.45, J)), np.nan)
    for j in range(J):
        if mirror[j] > j and parent[j] >= 0:
            L[mirror[j]] = L[j]
    u = rng.standard_normal((1, J, 3)) + np.cumsum(rng.standard_normal((N, J, 3)) * 0.05, axis=0)
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    x = np.zeros((N, J, 3))
    x[:, FACE] = rng.standard_normal((1, 68, 3)) * 0.05 + np.array([0, 0.5, 0])
    for j in range(1, J):
        if parent[j] >= 0:
            x[:, j] = x[:, parent[j]] + u[:, j] * L[j]
    sd = sigma * rng.uniform(0.5, 1.5, (N, J, 1)) * np.array([0.3, 0.3, 1.2])
    sd[:, 0] = 0.0                                                                 # root-relative poses: the root is exact
    pose = (x + rng.standard_normal((N, J, 3)) * sd).astype(np.float32)[None]
    cov = np.zeros((1, N, J, 6), dtype=np.float32)
    cov[0, ..., 0], cov[0, ..., 3], cov[0, ..., 5] = sd[..., 0] ** 2, sd[..., 1] ** 2, sd[..., 2] ** 2
    return pose, cov, parent, mirror, L.astype(np.float32)[None], x


@pytest.fixture(scope="module")
def plant():
    return planted(20261020)


def error_mm(p, x, sel):
    return float(np.linalg.norm(p[0][:, sel].astype(np.float64) - x[:, sel], axis=-1).mean() * 1000)


# --------------------------------------------------------------------------------------------------- the statement
def test_one_bone_with_a_pinned_parent_lands_on_the_length_in_one_sweep():
    rng = np.random.default_rng(1)
    pose = rng.standard_normal((1, 7, 2, 3)).astype(np.float32)
    cov = np.zeros((1, 7, 2, 6), dtype=np.float32)
    cov[..., [0, 3, 5]] = 4e-4                                                     # isotropic
    L = np.array([[np.nan, 0.3]], dtype=np.float32)
    y, fr = bones.project_f64(pose, cov, [-1, 0], L, 1, False, np.float32(FLOOR))
    l = np.linalg.norm(y[:, :, 1] - y[:, :, 0], axis=-1)
    assert np.abs(l - np.float64(L[0, 1])).max() < 1e-12
    assert np.array_equal(y[:, :, 0], pose[:, :, 0].astype(np.float64))             # the pinned end did not move
    assert fr.active[:, :, 1].all() and not fr.active[:, :, 0].any()


def test_first_sweep_is_the_kkt_solution_when_both_ends_are_free():
    """chain 0 -> 1 -> 2 with no length for bone 1: joint 1 is free (it has a bone) and bone 2 is its only active bone, so
    n = 1 at both ends and the sweep's displacements are the minimiser of dc' Ec^-1 dc + dp' Ep^-1 dp under
    u'(dc - dp) = -(l - L)"""
    rng = np.random.default_rng(2)
    for _ in range(8):
        pose = rng.standard_normal((1, 1, 3, 3)).astype(np.float32)
        cov = packed(random_cov(rng, (1, 1, 3), 0.5, 1.0))                         # of the size of the pose: a well-conditioned system
        L = np.array([[np.nan, np.nan, 0.4]], dtype=np.float32)
        y, _ = bones.project_f64(pose, cov, [-1, 0, 1], L, 1, False, np.float32(FLOOR))
        x = pose.astype(np.float64)[0, 0]
        d = x[2] - x[1]
        l = np.linalg.norm(d)
        u = d / l
        Ec, Ep = full(cov[0, 0, 2]), full(cov[0, 0, 1])
        K = np.zeros((7, 7))
        K[:3, :3], K[3:6, 3:6] = 2 * np.linalg.inv(Ec), 2 * np.linalg.inv(Ep)
        K[:3, 6], K[3:6, 6], K[6, :3], K[6, 3:6] = u, -u, u, -u
        sol = np.linalg.solve(K, np.array([0, 0, 0, 0, 0, 0, -(l - np.float64(L[0, 2]))]))
        assert np.abs((y[0, 0, 2] - x[2]) - sol[:3]).max() < 1e-12
        assert np.abs((y[0, 0, 1] - x[1]) - sol[3:6]).max() < 1e-12
        assert np.array_equal(y[0, 0, 0], x[0])


def test_no_sweep_and_no_snap_is_the_input(plant):
    pose, cov, parent, _, L, _ = plant
    pose = pose.copy()
    pose[0, 3, 5] = np.nan
    pose[0, 4, 30, 1] = -0.0
    out, code, resid = bones.project(pose, cov, parent, L, 0, False)
    assert same_bits(out, pose)
    assert same_bits(resid[..., 0], resid[..., 1])


def test_snap_makes_every_active_bone_exact_in_fp32(plant):
    pose, cov, parent, _, L, _ = plant
    assert np.abs(pose).max() < 2.0
    for it in (0, 3, 16):
        out, code, resid = bones.project(pose, cov, parent, L, it, True)
        o = out.astype(np.float64)
        has = parent >= 0
        l = np.linalg.norm(o[:, :, has] - o[:, :, parent[has]], axis=-1)
        assert np.abs(l - L[:, None, has].astype(np.float64)).max() <= 1e-6
        assert float(resid[..., 1].max()) <= 1e-6 and float(resid[..., 0].min()) > 1e-4
        assert same_bits(out[:, :, FACE], pose[:, :, FACE]) and same_bits(out[:, :, 0], pose[:, :, 0])
        assert (code[:, :, FACE] == 0).all() and (code[:, :, has] == 1).all() and (code[:, :, 0] == 1).all()


def test_mirror_partners_get_identical_bits(plant):
    pose, cov, parent, mirror, _, _ = plant
    length, dev, frames = bones.lengths(pose, cov, parent, mirror)
    alone, _, alone_frames = bones.lengths(pose, cov, parent, None)
    pairs = [j for j in range(134) if mirror[j] >= 0 and parent[j] >= 0]
    assert len(pairs) == 2 * (8 + 3 + 21)
    for j in pairs:
        m = mirror[j]
        assert bits(length)[0, j] == bits(length)[0, m] and bits(dev)[0, j] == bits(dev)[0, m]
        assert frames[0, j] == frames[0, m] == alone_frames[0, j] + alone_frames[0, m] == 120
    assert any(bits(alone)[0, j] != bits(alone)[0, mirror[j]] for j in pairs)
    assert np.isnan(length[0, FACE]).all() and (frames[0, FACE] == 0).all() and np.isnan(length[0, 0])


def test_no_covariance_is_an_all_zero_covariance(plant):
    pose, cov, parent, mirror, L, _ = plant
    zero = np.zeros_like(cov)
    for a, b in zip(bones.lengths(pose, None, parent, mirror), bones.lengths(pose, zero, parent, mirror)):
        assert same_bits(a, b)
    for a, b in zip(bones.project(pose, None, parent, L, 2, True), bones.project(pose, zero, parent, L, 2, True)):
        assert same_bits(a, b)


@pytest.mark.parametrize("N", [1, 64, 65, 130])
def test_lengths_are_the_weighted_mean_at_the_lane_boundaries(N):
    rng = np.random.default_rng(N)
    J = 6
    parent = np.array([-1, 0, 0, 1, 2, 2])
    mirror = np.array([-1, 2, 1, -1, 5, 4])
    pose = rng.standard_normal((2, N, J, 3)).astype(np.float32)
    cov = packed(random_cov(rng, (2, N, J)))
    pose[0, 0, 3] = np.nan                                                         # that frame takes no part in bone 3
    length, dev, frames = bones.lengths(pose, cov, parent, mirror)
    w, wl, wll, part = bones.bone_sums(pose, cov, parent, np.float32(FLOOR))
    for t in range(2):
        for j in range(1, J):
            both = [j] + ([int(mirror[j])] if mirror[j] >= 0 else [])
            S0, S1, S2 = (sum(a[t, :, k].sum() for k in both) for a in (w, wl, wll))
            cnt = sum(int(part[t, :, k].sum()) for k in both)
            assert frames[t, j] == cnt
            if cnt == 0:
                assert np.isnan(length[t, j]) and np.isnan(dev[t, j])
                continue
            assert abs(np.float64(length[t, j]) - S1 / S0) <= np.spacing(np.float32(S1 / S0))      # the one rounding to fp32
            want = np.sqrt(max(S2 / S0 - (S1 / S0) ** 2, 0.0))
            assert abs(np.float64(dev[t, j]) - want) <= 1e-6 * max(want, 1e-3)
    assert frames[0, 3] == N - 1 and frames[1, 3] == N
    # the fp64 length before its rounding, against the closed form
    pair = bones.partners(bones.table(parent, J), mirror)
    S0, S1 = bones._frames_sum(w, pair), bones._frames_sum(wl, pair)
    worst = 0.0
    for t in range(2):
        for j in range(1, J):
            both = [j] + ([int(pair[j])] if pair[j] >= 0 else [])
            if part[t][:, both].any():
                closed = sum(wl[t, :, k].sum() for k in both) / sum(w[t, :, k].sum() for k in both)
                gap = abs(S1[t, j] / S0[t, j] - closed) / closed
                worst = max(worst, gap)
                assert gap <= 1e-15, (t, j, gap)
    print(f"N = {N}: the lane-ordered length is within {worst:.1e} (relative) of the closed form")


def test_a_nan_joint_disables_exactly_its_bones_and_stays_in_its_frame(plant):
    pose, cov, parent, _, L, _ = plant
    want = bones.project(pose, cov, parent, L, 4, True)
    bad, bad_cov = pose.copy(), cov.copy()
    bad[0, 7, 10, 1] = np.nan                                                       # the left wrist of frame 7
    bad_cov[0, 9, 14, 2] = np.nan                                                   # the covariance of the left knee of frame 9
    bad_cov[0, 11, 0, 3] = -1.0                                                     # an indefinite root covariance in frame 11
    out, code, resid = bones.project(bad, bad_cov, parent, L, 4, True)
    kids = bones.children(bones.table(parent, 134))
    others = np.ones(60, dtype=bool)
    others[[7, 9, 11]] = False
    for a, b in zip((out, code, resid), want):                                     # every other frame: the same bits
        assert same_bits(a[:, others], b[:, others])
    assert np.isnan(out).sum() == 1 and same_bits(out[0, 7, 10], bad[0, 7, 10])     # no NaN created, its own bits kept
    fr = bones.Frame(bad, bad_cov, parent, L, np.float32(FLOOR))
    for n, j in ((7, 10), (9, 14), (11, 0)):
        off = [j] + kids[j]
        assert not fr.active[0, n, off].any()
        rest = np.ones(134, dtype=bool)
        rest[off] = False
        assert np.array_equal(fr.active[0, n, rest], fr.active[0, 0, rest])
        assert code[0, n, j] == 3 and same_bits(out[0, n, j], bad[0, n, j])
    assert (code == 3).sum() == 3                                                   # the elbow still has its shoulder, the ankle its feet
    assert code[0, 7, 8] == 1 and code[0, 7, 92] == 1 and code[0, 9, 16] == 1
    assert (code[0, 11, [1, 6, 7, 12, 13]] == 1).all()                             # nose, shoulders, hips: moved by their children
    assert (code[:, :, FACE] == 0).all()
    missing = L.copy()
    missing[0, [8, 10]] = np.nan                                                    # no length for the left forearm and upper arm
    out2, code2, _ = bones.project(bad, bad_cov, parent, missing, 1, False)
    assert (code2[:, :, 8] == 0).all() and same_bits(out2[:, :, 8], bad[:, :, 8])   # nothing is asked of the elbow: not a failure
    assert code2[0, 7, 10] == 3 and (np.delete(code2[0, :, 10], 7) == 1).all()      # the wrist still carries the hand


def test_the_projection_beats_raw_and_the_snap_alone_does_not(plant):
    pose, cov, parent, _, L, x = plant
    out, _, resid = bones.project(pose, cov, parent, L, 16, True)
    snap, _, _ = bones.project(pose, cov, parent, L, 0, True)
    for name, sel in (("body", BODY), ("hands", HANDS)):
        raw, got, top_down = error_mm(pose, x, sel), error_mm(out, x, sel), error_mm(snap, x, sel)
        print(f"{name}: raw {raw:.2f} mm, 16 sweeps + snap {got:.2f} mm ({got / raw:.2f} x), snap alone {top_down:.2f} mm")
        assert got < 0.8 * raw
        assert top_down > raw
    assert error_mm(out, x, FACE) == error_mm(pose, x, FACE)
    _, _, free = bones.project(pose, cov, parent, L, 16, False)
    print(f"worst bone of 60 frames: {resid[0, :, 0].max() * 1000:.1f} mm -> {free[0, :, 1].max() * 1000:.2f} mm in 16 sweeps")
    assert free[0, :, 1].max() < resid[0, :, 0].max() / 4


def test_statement_refuses_bad_arguments(plant):
    pose, cov, parent, mirror, L, _ = plant
    for kw in (dict(iterations=-1), dict(iterations=65), dict(iterations=True), dict(iterations=1.5), dict(snap=2), dict(snap="yes"),
               dict(floor=0.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=True), dict(floor=1e-60)):
        with pytest.raises(ValueError):
            bones.project(pose, cov, parent, L, **kw)
    for bad in (dict(floor=-1.0), dict(floor=None)):
        with pytest.raises(ValueError):
            bones.lengths(pose, cov, parent, mirror, **bad)
    with pytest.raises(ValueError, match="pose"):
        bones.project(pose[0], cov, parent, L)
    with pytest.raises(ValueError, match="cov"):
        bones.project(pose, cov[..., :3], parent, L)
    with pytest.raises(ValueError, match="length"):
        bones.project(pose, cov, parent, L[0])
    with pytest.raises(ValueError, match="parent"):
        bones.project(pose, cov, parent[:-1], L)
    with pytest.raises(ValueError, match="parent"):
        bones.lengths(pose, cov, parent.astype(np.float32), mirror)
    with pytest.raises(ValueError, match="mirror"):
        bones.lengths(pose, cov, parent, mirror[:-1])
    with pytest.raises(ValueError, match="256"):
        bones.lengths(np.zeros((1, 1, 257, 3), dtype=np.float32), None, np.full(257, -1))
    with pytest.raises(ValueError, match="smaller"):
        bones.table([-1, 1, 0], 3, strict=True)
    assert bones.table([5, 1, 0, -7, 3], 5).tolist() == [-1, -1, 0, -1, 3]          # what the kernels read


# --------------------------------------------------------------------------------------------------- the tables
def test_bone_tables_are_the_body_s_forest():
    parent, mirror = h3wb.bone_tables(68)
    assert parent.dtype == mirror.dtype == np.int32 and parent.shape == mirror.shape == (134,)
    assert all(-1 <= parent[j] < j for j in range(134))
    assert (parent[FACE] == -1).all() and parent[0] == -1 and (parent >= 0).sum() == 134 - 68 - 1
    depth = np.zeros(134, dtype=int)
    for j in range(134):
        depth[j] = 0 if parent[j] < 0 else depth[parent[j]] + 1
    assert depth.max() == 8 and depth[[96, 133]].tolist() == [8, 8]                 # root, shoulder, elbow, wrist, hand, four finger joints
    assert parent[1] == 0 and parent[2:6].tolist() == [1] * 4                       # unlike skeleton_parents: the head has bones
    assert h3wb.skeleton_parents(68, True)[1:6] == [-1] * 5
    assert parent[6:18].tolist() == [0, 0, 6, 7, 8, 9, 0, 0, 12, 13, 14, 15] and parent[18:24].tolist() == [16] * 3 + [17] * 3
    assert parent[92:].tolist() == h3wb.skeleton_parents(68, True)[92:]
    from tests.golden import golden_util as gu
    for a, b in zip(gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT):
        assert mirror[a] == b and mirror[b] == a
    assert (mirror >= 0).sum() == 2 * len(gu.SYN_JOINTS_LEFT) and (mirror[FACE] == -1).all() and mirror[0] == mirror[1] == -1
    paired = np.flatnonzero(mirror >= 0)
    assert all(mirror[parent[j]] == parent[mirror[j]] or parent[j] == parent[mirror[j]] for j in paired)   # partners hang on partners
    from types import SimpleNamespace
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS)
    p2, m2 = h3wb.bone_tables(ds, True, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT)
    assert np.array_equal(p2, parent) and np.array_equal(m2, mirror)
    # a dataset with a skeleton(): its joints_left() / joints_right(), paired by position - what the harness reaches with a real dataset
    real = h3wb.Human3WBDataset(os.path.join(ROOT, "tests", "golden", "h3wb_synth", "train_h3wb.npz"))
    p3, m3 = h3wb.bone_tables(real)
    assert np.array_equal(p3, parent) and len(real.skeleton().joints_left()) == 32
    for a, b in zip(real.skeleton().joints_left(), real.skeleton().joints_right()):
        assert m3[a] == b and m3[b] == a
    assert (m3 >= 0).sum() == 64 and np.array_equal(m3, mirror)
    from pafuse_amd import harness
    for got in harness._bone_tables(None, real, [1, 2], [3, 4]), harness._bone_tables(None, real):     # the skeleton comes before the caller's lists
        assert np.array_equal(got[0], parent) and np.array_equal(got[1], mirror)
    assert harness._bone_tables(None, ds, [2], [3])[1].tolist().count(-1) == 132                          # no skeleton: the caller's lists
    flat, _ = h3wb.bone_tables(68, root_added=False)
    assert flat.shape == (133,) and all(-1 <= flat[j] < j for j in range(133)) and (flat[23:91] == -1).all()
    with pytest.raises(ValueError):
        h3wb.bone_tables(68, True, [1, 2], [3])


# --------------------------------------------------------------------------------------------------- the interface
def built():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib, _lib.load()


def test_entries_are_declared_exported_and_bound_as_the_header_says():
    _lib, lib = built()
    header = open(os.path.join(ROOT, "include", "pafuse_hip.h")).read()
    C = ctypes
    kinds = {"float": C.c_float, "int32_t": C.c_int32}
    for name in ("pafuse_bone_lengths", "pafuse_bone_project"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        want = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
        assert _lib.SIGNATURES[name] == (C.c_int, want), name
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["pafuse_bone_lengths"][1]) == 12 and len(_lib.SIGNATURES["pafuse_bone_project"][1]) == 14


def test_the_c_abi_refuses_before_any_hip_call():
    """host memory stands in for the operands: a call that got as far as a launch could not succeed here, and -1 is
    PAFUSE_E_ARG, not the HIP error a launch without a device returns"""
    _lib, lib = built()
    J, N = 5, 4
    pose = np.zeros((1, N, J, 3), dtype=np.float32)
    out = np.full((1, N, J, 3), 7.0, dtype=np.float32)
    parent = np.array([-1, 0, 1, 2, 3], dtype=np.int32)
    length = np.ones((1, J), dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data

    def lengths(pose=pose, parent=parent, length=length, T=1, N=N, J=J, floor=FLOOR):
        return lib.pafuse_bone_lengths(p(pose), None, p(parent), None, T, N, J, floor, p(length), None, None, None)

    def project(pose=pose, parent=parent, length=length, out=out, T=1, N=N, J=J, it=16, snap=1, floor=FLOOR):
        return lib.pafuse_bone_project(p(pose), None, p(parent), p(length), T, N, J, it, snap, floor, p(out), None, None, None)

    for bad in (dict(pose=None), dict(parent=None), dict(length=None), dict(T=0), dict(N=0), dict(J=0), dict(J=-3), dict(J=257),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf"))):
        assert lengths(**bad) == -1, bad
        assert b"bone_lengths" in lib.pafuse_last_error()
        assert project(**bad) == -1, bad
        assert b"bone_project" in lib.pafuse_last_error()
    for bad in (dict(out=None), dict(it=-1), dict(it=65), dict(snap=2), dict(snap=-1), dict(out=pose)):
        assert project(**bad) == -1, bad
    assert (out == 7.0).all()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import harness, ops
    pose = torch.zeros(1, 4, 3, 3)
    L = torch.ones(1, 3)
    with pytest.raises(ValueError, match="smaller"):
        ops.bone_lengths(pose, None, [-1, 2, 0])
    with pytest.raises(ValueError, match="smaller"):
        ops.project_bones(pose, None, [-1, 1, 0], L)
    with pytest.raises(ValueError, match="smaller"):
        ops.project_bones(pose, None, torch.tensor([0, 0, 1]), L)
    with pytest.raises(ValueError, match="mirror"):
        ops.bone_lengths(pose, None, [-1, 0, 0], mirror=[-1, 3, 1])
    with pytest.raises(ValueError, match="length"):
        ops.project_bones(pose, None, [-1, 0, 1], torch.ones(1, 4))
    with pytest.raises(ValueError, match="length"):
        ops.project_bones(pose, None, [-1, 0, 1], torch.ones(2, 3))
    for kw in (dict(iterations=65), dict(iterations=-1), dict(iterations=True), dict(snap=2), dict(floor=0.0), dict(floor=float("nan"))):
        with pytest.raises(ValueError):
            ops.project_bones(pose, None, [-1, 0, 1], L, **kw)
    with pytest.raises(ValueError, match="HIP device"):
        ops.project_bones(pose, None, [-1, 0, 1], L)                               # a CPU tensor: no fallback
    with pytest.raises(ValueError, match="smaller"):
        harness.constrain_bones(pose, tables=([-1, 2, 0], None))
    with pytest.raises(ValueError, match="lengths"):
        harness.constrain_bones(pose, tables=([-1, 0, 1], None), lengths=torch.ones(4))
    with pytest.raises(ValueError, match="lengths"):
        harness.constrain_bones(pose, tables=([-1, 0, 1], None), lengths="left")
    with pytest.raises(ValueError, match="joints"):
        harness.constrain_bones(pose)                                              # the H3WB tables hold 134 joints
    with pytest.raises(ValueError, match="iterations"):
        harness.constrain_bones(pose, tables=([-1, 0, 1], None), iterations=70)
    from types import SimpleNamespace
    from tests.golden import golden_util as gu
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS)
    model = SimpleNamespace(frames=27)
    seq = torch.zeros(30, 134, 2)
    call = lambda **kw: harness.infer_sequence(model, ds, seq, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, **kw)
    with pytest.raises(ValueError, match="bone_lengths needs stride"):
        call(bone_lengths="video", aggregate="mean")
    with pytest.raises(ValueError, match="bone_lengths needs aggregate"):
        call(bone_lengths="video", stride=9)
    with pytest.raises(ValueError, match="bone_lengths must be"):
        call(bone_lengths="both", stride=9, aggregate="mean")
    with pytest.raises(ValueError, match="J = 134"):
        call(bone_lengths=torch.ones(133), stride=9, aggregate="mean")
    with pytest.raises(ValueError, match="bone_iterations"):
        call(bone_lengths="video", bone_iterations=65, stride=9, aggregate="mean")
    with pytest.raises(ValueError, match="bone_iterations"):
        harness.evaluate_frames(model, ds, seq, torch.zeros(30, 134, 3), torch.zeros(9), gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                                bone_lengths="symmetric", bone_iterations=-1)


def test_torch_ops_have_a_schema_and_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import pafuse_amd.torch_ops  # noqa: F401
    schema = str(torch.ops.pafuse.bone_lengths.default._schema)
    assert "Tensor pose, Tensor? cov" in schema and re.search(r"[Ii]nt\[\] parent", schema) and re.search(r"[Ii]nt\[\]\? mirror=None", schema)
    assert "float floor=0.001" in schema and schema.endswith("-> Tensor[]")
    schema = str(torch.ops.pafuse.bone_project.default._schema)
    assert "Tensor length" in schema and re.search(r"[Ii]nt iterations=16", schema) and "bool snap=True" in schema and schema.endswith("-> Tensor[]")
    with FakeTensorMode():
        pose, cov = torch.empty(2, 9, 134, 3, device="cuda"), torch.empty(2, 9, 134, 6, device="cuda")
        length, dev, frames = torch.ops.pafuse.bone_lengths(pose, cov, [-1] * 134, None, 1e-3)
        assert length.shape == dev.shape == frames.shape == (2, 134) and frames.dtype == torch.int32 and length.dtype == torch.float32
        out, code, resid = torch.ops.pafuse.bone_project(pose, None, [-1] * 134, length, 16, True, 1e-3)
        assert out.shape == pose.shape and code.shape == (2, 9, 134) and code.dtype == torch.uint8 and resid.shape == (2, 9, 2)
    with pytest.raises(NotImplementedError):
        torch.ops.pafuse.bone_project(torch.zeros(1, 1, 2, 3), None, [-1, 0], torch.ones(1, 2))

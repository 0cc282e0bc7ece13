"""Bone lengths held constant along a video, on the device: bone_lengths_kernel (pafuse_bone_lengths), bone_project_kernel
(pafuse_bone_project), ops.bone_lengths / ops.project_bones, torch.ops.pafuse.bone_lengths / bone_project,
harness.constrain_bones, infer_sequence(bone_lengths=...) and evaluate_frames(bone_lengths=...).

What is asserted and why it can be asserted:
  * kernel vs statement: the kernels and pafuse_amd/bones.py perform the same IEEE fp64 operations in the same order
    (contraction off, correctly rounded sqrt and divide; the sums over the frames in the lane-then-butterfly order), then round
    once to fp32 -> the design goal is equal bits; the test accepts equal or ADJACENT fp32 values with NaN in the same places -
    the acceptance rule of tests/test_hip_rootfit.py - on EVERY value of out, length, dev and resid, and prints how many
    differ.  code and frames are integers -> torch.equal.
  * everything else is same bits: guard rows around every output, two calls, optional outputs NULL, a side stream, a frame
    alone against the same frame in a batch, iterations = 0 without snap against the input, the Python layers over the entry.
Shapes: J in {2, 5, 64, 65, 134, 256} - one bone, part of a wave, exactly a wave, a wave and a lane, three slots with the last
one partly filled, the most a wave holds - under random forests (parent uniform in -1 .. j-1), the chain parent = j - 1 (the
longest snap walk), the star parent = 0 (one joint with J - 1 children: the longest child list) and the H3WB tables at 134.
Projection: N in {1, 9} (a workgroup partly filled, three workgroups) x iterations in {0, 1, 16} x snap in {0, 1}; lengths: N in
{1, 2, 65, 130} (the lane boundaries of the frame loop); T in {1, 2}; with a covariance and without.  About 5 % of the rows
have a NaN pose or covariance, a few are indefinite, a few lengths are missing, zero, negative or infinite.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1e-3
PAD = 7
TABLES = [(J, kind) for J in (2, 5, 64, 65, 134, 256) for kind in ("forest", "chain", "star")] + [(134, "h3wb")]


def tables(J, kind, seed=0):
    """-> (parent, mirror) int32 [J]; the mirror of the made-up tables pairs random joints: partners that name each other,
    one-sided entries, an entry naming itself and -1"""
    rng = np.random.default_rng(1000 * J + seed)
    if kind == "h3wb":
        from pafuse_amd import h3wb
        return h3wb.bone_tables(68)
    j = np.arange(J)
    parent = {"forest": rng.integers(-1, np.maximum(j, 1)), "chain": j - 1, "star": np.where(j > 0, 0, -1)}[kind]
    parent[0] = -1
    order = rng.permutation(J)
    mirror = np.full(J, -1)
    for a, b in zip(order[0:J // 2:2], order[1:J // 2:2]):
        mirror[a], mirror[b] = b, a
    mirror[order[-1]] = order[-1]                                     # itself: read as no partner
    if J > 4:
        mirror[order[-2]] = order[0]                                  # one-sided
    return parent.astype(np.int32), mirror.astype(np.int32)


def inputs(T, N, J, seed):
    """a random pose per (t, frame) with random anisotropic covariances (standard deviations 2 - 20 mm x (1, 0.4, 0.15),
    rotated) and lengths 5 - 50 cm; about 5 % of the rows without a pose or without a covariance, a few indefinite, an infinite
    coordinate, a row the floor alone carries, and lengths that are missing, zero, negative and infinite"""
    rng = np.random.default_rng(seed)
    pose = (rng.standard_normal((T, N, J, 3)) * 0.3).astype(np.float32)
    Q, _ = np.linalg.qr(rng.standard_normal((T, N, J, 3, 3)))
    sd = rng.uniform(0.002, 0.02, (T, N, J))[..., None] * np.array([1.0, 0.4, 0.15])
    S = np.einsum("...ik,...k,...jk->...ij", Q, sd * sd, Q)
    cov = np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2], S[..., 2, 2]], axis=-1).astype(np.float32)
    pose[rng.random((T, N, J)) < 0.03] = np.nan
    cov[rng.random((T, N, J)) < 0.02, rng.integers(0, 6)] = np.nan
    bad = rng.random((T, N, J)) < 0.02
    cov[bad, 3] = -cov[bad, 3]                                        # yy < 0: indefinite whatever the floor
    length = rng.uniform(0.05, 0.5, (T, J)).astype(np.float32)
    length[rng.random((T, J)) < 0.05] = np.nan
    if J > 4:
        pose[0, 0, 3, 1] = np.inf
        cov[T - 1, N - 1, J - 1] = 0
        length[0, 2], length[T - 1, 3], length[0, 4] = 0.0, -0.2, np.inf
    return pose, cov, length


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------------------------------- kernel vs statement
@pytest.mark.parametrize("case", TABLES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_projection_kernel_is_the_statement(case):
    from pafuse_amd import bones, ops
    J, kind = case
    parent, _ = tables(J, kind)
    differ = total = 0
    for T, N in ((1, 1), (2, 9)):
        pose, cov, length = inputs(T, N, J, seed=100 * J + N)
        for c in (cov, None):
            for it in (0, 1, 16):
                for snap in (False, True):
                    out, code, resid = ops.project_bones(dev(pose), dev(c), parent, dev(length), iterations=it, snap=snap, floor=FLOOR,
                                                         want_code=True, want_resid=True)
                    w_out, w_code, w_resid = bones.project(pose, c, parent, length, it, snap, FLOOR)
                    assert tuple(out.shape) == (T, N, J, 3) and out.dtype == torch.float32 and code.dtype == torch.uint8
                    assert tuple(resid.shape) == (T, N, 2) and resid.dtype == torch.float32
                    assert torch.equal(code.cpu(), torch.from_numpy(w_code)), (T, N, c is None, it, snap)
                    differ += equal_or_adjacent(out.cpu(), torch.from_numpy(w_out))
                    differ += equal_or_adjacent(resid.cpu(), torch.from_numpy(w_resid))
                    total += out.numel() + resid.numel()
                    keep = torch.from_numpy(w_code != 1)              # a joint outside every active bone: the input's bits
                    assert same_bits(out.cpu()[keep], torch.from_numpy(pose)[keep])
                    assert torch.equal(torch.isnan(out.cpu()), torch.isnan(torch.from_numpy(pose)))     # no NaN created
                    if it == 0 and not snap:
                        assert same_bits(out.cpu(), torch.from_numpy(pose))
    print(f"(J, table) = {case}: {differ} of {total} values of out and resid differ from the statement (by one fp32 step)")


@pytest.mark.parametrize("case", TABLES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_lengths_kernel_is_the_statement(case):
    from pafuse_amd import bones, ops
    J, kind = case
    parent, mirror = tables(J, kind)
    differ = total = 0
    for T, N in ((1, 1), (2, 2), (2, 65), (1, 130)):
        pose, cov, _ = inputs(T, N, J, seed=200 * J + N)
        for c in (cov, None):
            for m in (mirror, None):
                length, sd, frames = ops.bone_lengths(dev(pose), dev(c), parent, m, floor=FLOOR, want_dev=True, want_frames=True)
                w_length, w_sd, w_frames = bones.lengths(pose, c, parent, m, FLOOR)
                assert tuple(length.shape) == tuple(sd.shape) == tuple(frames.shape) == (T, J) and frames.dtype == torch.int32
                assert torch.equal(frames.cpu(), torch.from_numpy(w_frames)), (T, N, c is None, m is None)
                differ += equal_or_adjacent(length.cpu(), torch.from_numpy(w_length)) + equal_or_adjacent(sd.cpu(), torch.from_numpy(w_sd))
                total += 2 * length.numel()
                if m is not None:                                     # partners that name each other: the same bits
                    for j in range(J):
                        k = int(m[j])
                        if 0 <= k < J and k != j and m[k] == j and parent[j] >= 0 and parent[k] >= 0:
                            assert same_bits(length[:, j], length[:, k]) and same_bits(sd[:, j], sd[:, k])
    print(f"(J, table) = {case}: {differ} of {total} values of length and dev differ from the statement (by one fp32 step)")


def test_the_kernels_read_a_bad_table_entry_as_no_bone():
    """the raw entries take any table: an entry outside 0 .. j-1 is -1, as the statement's table() reads it"""
    from pafuse_amd import _lib, bones
    lib = _lib.load()
    T, N, J = 1, 3, 9
    pose, cov, length = inputs(T, N, J, seed=9)
    parent = np.array([5, 0, 2, 7, -9, 4, 300, 3, 8], dtype=np.int32)
    mirror = np.array([1, 0, 900, -5, 5, 4, 7, 6, 8], dtype=np.int32)
    p, c, par, mir, L = dev(pose), dev(cov), dev(parent), dev(mirror), dev(length)
    out, code, resid = torch.full_like(p, 7.0), torch.full((T, N, J), 9, dtype=torch.uint8, device=DEV), torch.full((T, N, 2), 7.0, device=DEV)
    got_len, got_dev, got_frames = torch.full((T, J), 7.0, device=DEV), torch.full((T, J), 7.0, device=DEV), torch.full((T, J), 9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    assert lib.pafuse_bone_project(p.data_ptr(), c.data_ptr(), par.data_ptr(), L.data_ptr(), T, N, J, 3, 1, FLOOR, out.data_ptr(),
                                   code.data_ptr(), resid.data_ptr(), None) == 0
    assert lib.pafuse_bone_lengths(p.data_ptr(), c.data_ptr(), par.data_ptr(), mir.data_ptr(), T, N, J, FLOOR, got_len.data_ptr(),
                                   got_dev.data_ptr(), got_frames.data_ptr(), None) == 0
    torch.cuda.synchronize()
    w_out, w_code, w_resid = bones.project(pose, cov, parent, length, 3, True, FLOOR)
    assert torch.equal(code.cpu(), torch.from_numpy(w_code))
    differ = equal_or_adjacent(out.cpu(), torch.from_numpy(w_out))
    differ += equal_or_adjacent(resid.cpu(), torch.from_numpy(w_resid))
    w_len, w_dev, w_frames = bones.lengths(pose, cov, parent, mirror, FLOOR)
    assert torch.equal(got_frames.cpu(), torch.from_numpy(w_frames))
    differ += equal_or_adjacent(got_len.cpu(), torch.from_numpy(w_len))
    differ += equal_or_adjacent(got_dev.cpu(), torch.from_numpy(w_dev))
    print(f"tables with entries out of range: {differ} of {out.numel() + resid.numel() + 2 * got_len.numel()} values differ from the statement")


# --------------------------------------------------------------------------------------------------- same bits
def raw_project(lib, pose, cov, par, length, T, N, J, it, snap, out, code, resid, stream=None):
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.pafuse_bone_project(ptr(pose), ptr(cov), ptr(par), ptr(length), T, N, J, it, snap, FLOOR, ptr(out), ptr(code), ptr(resid), stream)
    torch.cuda.synchronize()
    return rc


def raw_lengths(lib, pose, cov, par, mir, T, N, J, length, sd, frames, stream=None):
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.pafuse_bone_lengths(ptr(pose), ptr(cov), ptr(par), ptr(mir), T, N, J, FLOOR, ptr(length), ptr(sd), ptr(frames), stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, "h3wb", 9), (256, "chain", 5), (65, "forest", 1), (2, "star", 2)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_guard_rows_repeat_calls_null_outputs_a_side_stream_and_the_python_layers(case):
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import _lib, ops
    lib = _lib.load()
    J, kind, N = case
    T = 2
    parent, mirror = tables(J, kind)
    pose, cov, length = inputs(T, N, J, seed=77)
    p, c, L, par, mir = dev(pose), dev(cov), dev(length), dev(parent), dev(mirror)
    n = T * N * J
    # ---- the projection
    want, want_code, want_resid = ops.project_bones(p, c, parent, L, want_code=True, want_resid=True)
    out = torch.full((PAD + n * 3 + PAD,), 7.0, device=DEV)
    code = torch.full((PAD + n + PAD,), 9, dtype=torch.uint8, device=DEV)
    resid = torch.full((PAD + T * N * 2 + PAD,), 7.0, device=DEV)
    torch.cuda.synchronize()
    assert raw_project(lib, p, c, par, L, T, N, J, 16, 1, out[PAD:], code[PAD:], resid[PAD:]) == 0
    for buf, size, fill in ((out, n * 3, 7.0), (code, n, 9), (resid, T * N * 2, 7.0)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + size:] == fill).all())
    assert same_bits(out[PAD:PAD + n * 3], want.reshape(-1)) and torch.equal(code[PAD:PAD + n], want_code.reshape(-1))
    assert same_bits(resid[PAD:PAD + T * N * 2], want_resid.reshape(-1))
    again = torch.full((n * 3 + PAD,), 7.0, device=DEV)
    torch.cuda.synchronize()
    assert raw_project(lib, p, c, par, L, T, N, J, 16, 1, again, None, None) == 0           # code and resid NULL: the same out
    assert bool((again[n * 3:] == 7.0).all()) and same_bits(again[:n * 3], want.reshape(-1))
    assert same_bits(ops.project_bones(p, c, parent, L), want)                                # two calls, the same bits
    given = torch.full((T, N, J, 3), 7.0, device=DEV)
    assert ops.project_bones(p, c, parent, L, out=given) is given and same_bits(given, want)
    t_out, t_code, t_resid = torch.ops.pafuse.bone_project(p, c, parent.tolist(), L, 16, True, FLOOR)
    assert same_bits(t_out, want) and torch.equal(t_code, want_code) and same_bits(t_resid, want_resid)
    assert same_bits(ops.project_bones(p, c, torch.from_numpy(parent), L[0] if T == 1 else L), want)
    for t in range(T):                                                                        # a frame alone: the same bits as in the batch
        f = N // 2
        one = ops.project_bones(p[t:t + 1, f:f + 1].contiguous(), c[t:t + 1, f:f + 1].contiguous(), parent, L[t:t + 1].contiguous())
        assert same_bits(one[0, 0], want[t, f])
    assert same_bits(ops.project_bones(p, c, parent, L, iterations=0, snap=False), p)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, code_side, resid_side = ops.project_bones(p, c, parent, L, want_code=True, want_resid=True)
        len_side = ops.bone_lengths(p, c, parent, mirror)
    side.synchronize()
    assert same_bits(on_side, want) and torch.equal(code_side, want_code) and same_bits(resid_side, want_resid)
    other = torch.full((n * 3,), 7.0, device=DEV)
    torch.cuda.synchronize()
    assert raw_project(lib, p, c, par, L, T, N, J, 16, 1, other, None, None, stream=side.cuda_stream) == 0
    assert same_bits(other, want.reshape(-1))
    # ---- the lengths
    w_len, w_sd, w_frames = ops.bone_lengths(p, c, parent, mirror, want_dev=True, want_frames=True)
    assert same_bits(len_side, w_len)
    g_len, g_sd = torch.full((PAD + T * J + PAD,), 7.0, device=DEV), torch.full((PAD + T * J + PAD,), 7.0, device=DEV)
    g_frames = torch.full((PAD + T * J + PAD,), 9, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    assert raw_lengths(lib, p, c, par, mir, T, N, J, g_len[PAD:], g_sd[PAD:], g_frames[PAD:]) == 0
    for buf, fill in ((g_len, 7.0), (g_sd, 7.0), (g_frames, 9)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + T * J:] == fill).all())
    assert same_bits(g_len[PAD:PAD + T * J], w_len.reshape(-1)) and same_bits(g_sd[PAD:PAD + T * J], w_sd.reshape(-1))
    assert torch.equal(g_frames[PAD:PAD + T * J], w_frames.reshape(-1))
    alone = torch.full((T * J + PAD,), 7.0, device=DEV)
    torch.cuda.synchronize()
    assert raw_lengths(lib, p, c, par, mir, T, N, J, alone, None, None) == 0                 # dev and frames NULL: the same length
    assert bool((alone[T * J:] == 7.0).all()) and same_bits(alone[:T * J], w_len.reshape(-1))
    t_len, t_sd, t_frames = torch.ops.pafuse.bone_lengths(p, c, parent.tolist(), mirror.tolist(), FLOOR)
    assert same_bits(t_len, w_len) and same_bits(t_sd, w_sd) and torch.equal(t_frames, w_frames)
    for t in range(T):                                                                        # a step alone
        assert same_bits(ops.bone_lengths(p[t:t + 1].contiguous(), c[t:t + 1].contiguous(), parent, mirror)[0], w_len[t])
    assert same_bits(ops.bone_lengths(p, None, parent, mirror), ops.bone_lengths(p, torch.zeros_like(c), parent, mirror))
    assert same_bits(ops.project_bones(p, None, parent, L), ops.project_bones(p, torch.zeros_like(c), parent, L))


def test_refusals_on_the_device_launch_nothing():
    from pafuse_amd import _lib, harness, ops
    lib = _lib.load()
    pose = torch.zeros(1, 4, 5, 3, device=DEV)
    out = torch.full((1, 4, 5, 3), 7.0, device=DEV)
    par, L = torch.tensor([-1, 0, 1, 2, 3], dtype=torch.int32, device=DEV), torch.ones(1, 5, device=DEV)
    torch.cuda.synchronize()
    for bad in (dict(T=0), dict(J=257), dict(it=65), dict(it=-1), dict(snap=2)):
        a = dict(T=1, N=4, J=5, it=3, snap=1)
        a.update(bad)
        assert raw_project(lib, pose, None, par, L, a["T"], a["N"], a["J"], a["it"], a["snap"], out, None, None) == -1, bad
    assert raw_project(lib, pose, None, par, L, 1, 4, 5, 3, 1, pose, None, None) == -1
    assert raw_project(lib, pose, None, par, None, 1, 4, 5, 3, 1, out, None, None) == -1
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="alias"):
        ops.project_bones(pose, None, [-1, 0, 1, 2, 3], L, out=pose)
    with pytest.raises(ValueError, match="smaller"):
        ops.project_bones(pose, None, [-1, 0, 1, 4, 3], L)
    with pytest.raises(ValueError, match="dtypes"):
        ops.project_bones(pose.double(), None, [-1, 0, 1, 2, 3], L)
    with pytest.raises(ValueError, match="cov"):
        ops.bone_lengths(pose, torch.zeros(1, 4, 5, 3, device=DEV), [-1, 0, 1, 2, 3])


def test_constrain_bones_on_poses_a_caller_has():
    from pafuse_amd import harness, ops
    parent, mirror = tables(134, "h3wb")
    pose, cov, _ = inputs(2, 9, 134, seed=5)
    got = harness.constrain_bones(pose, cov, lengths="symmetric")
    assert set(got) == {"pose", "pose_free", "bone_length", "bone_dev", "bone_frames", "bone_code", "bone_resid"}
    assert all(not v.is_cuda for v in got.values()) and same_bits(got["pose_free"], torch.from_numpy(pose))
    length, sd, frames = ops.bone_lengths(dev(pose), dev(cov), parent, mirror, want_dev=True, want_frames=True)
    assert same_bits(got["bone_length"], length.cpu()) and same_bits(got["bone_dev"], sd.cpu()) and torch.equal(got["bone_frames"], frames.cpu())
    want, code, resid = ops.project_bones(dev(pose), dev(cov), parent, length, want_code=True, want_resid=True)
    assert same_bits(got["pose"], want.cpu()) and torch.equal(got["bone_code"], code.cpu()) and same_bits(got["bone_resid"], resid.cpu())
    own = torch.full((134,), 0.1)
    own[40] = float("nan")
    mine = harness.constrain_bones(pose, None, tables=(parent, None), lengths=own, iterations=2, snap=False, floor=2e-3)
    assert same_bits(mine["bone_length"], own.expand(2, 134)) and tuple(mine["bone_dev"].shape) == (2, 134)
    assert same_bits(mine["pose"], ops.project_bones(dev(pose), None, parent, dev(own.numpy()), iterations=2, snap=False, floor=2e-3).cpu())
    assert not same_bits(mine["bone_dev"], got["bone_dev"])                                   # no mirror, no covariance: other weights


# --------------------------------------------------------------------------------------------------- the harness
SEED = 9753
N_VIDEO = 30


@pytest.fixture(scope="module")
def runs():
    """infer_sequence(stride = 9, aggregate = "mean") on a 30-frame video, from the same start of the noise stream: without the
    keyword, with bone_lengths = None, "video" (alone; with spread = "cov"; behind pose_smooth; with a trajectory), "symmetric"
    and a tensor; computed once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, seq_3d, cam = sequence(N_VIDEO)
    own = torch.full((134,), 0.2)
    out = {}
    for name, kw in (("plain", dict()), ("none", dict(bone_lengths=None)), ("video", dict(bone_lengths="video")),
                     ("cov", dict(bone_lengths="video", spread="cov")), ("plain_cov", dict(spread="cov")),
                     ("smooth", dict(bone_lengths="video", pose_smooth=3)), ("smooth_only", dict(pose_smooth=3)),
                     ("symmetric", dict(bone_lengths="symmetric", bone_iterations=4)), ("own", dict(bone_lengths=own)),
                     ("traj", dict(bone_lengths="video", trajectory=3, cam=cam))):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        out[name] = harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2,
                                           aggregate="mean", stride=9, **kw)
    return out, model, seq_2d, seq_3d, cam, own


def snap_bound(pose):
    """metres: what the rounding of the returned coordinates to fp32 can leave of |l - L| - half a step of the largest
    coordinate at each of the six coordinates of a bone (1e-6 m below 2 m)"""
    return 6 * 0.5 * float(torch.finfo(torch.float32).eps) * max(2.0, float(pose.abs().max()))


BONE_KEYS = {"pose_free", "bone_length", "bone_dev", "bone_frames", "bone_code", "bone_resid"}


def test_infer_sequence_without_bone_lengths_is_unchanged(runs):
    out = runs[0]
    assert set(out["plain"]) == set(out["none"]) == {"pose", "count"}
    assert all(same_bits(out["plain"][k], out["none"][k]) for k in out["plain"])
    assert not BONE_KEYS & set(out["smooth_only"])


def test_infer_sequence_projects_the_returned_pose_onto_the_video_s_lengths(runs):
    from pafuse_amd import h3wb, ops
    out = runs[0]
    got, cov = out["video"], out["cov"]
    parent, mirror = h3wb.bone_tables(68)
    assert set(got) == {"pose", "count"} | BONE_KEYS and set(cov) == set(got) | {"std", "cov"}
    assert all(not v.is_cuda for v in cov.values())
    assert tuple(got["pose"].shape) == (2, N_VIDEO, 134, 3) and tuple(got["bone_length"].shape) == (2, 134)
    assert tuple(got["bone_code"].shape) == (2, N_VIDEO, 134) and tuple(got["bone_resid"].shape) == (2, N_VIDEO, 2)
    assert same_bits(got["pose_free"], out["plain"]["pose"]) and same_bits(got["count"], out["plain"]["count"])
    for k in ("std", "cov"):                                                                  # the covariance is not updated
        assert same_bits(cov[k], out["plain_cov"][k]), k
    assert all(same_bits(got[k], cov[k]) for k in got)
    length, sd, frames = ops.bone_lengths(cov["pose_free"].to(DEV), cov["cov"].to(DEV), parent, None, want_dev=True, want_frames=True)
    assert same_bits(cov["bone_length"], length.cpu()) and same_bits(cov["bone_dev"], sd.cpu()) and torch.equal(cov["bone_frames"], frames.cpu())
    want, code, resid = ops.project_bones(cov["pose_free"].to(DEV), cov["cov"].to(DEV), parent, cov["bone_length"].to(DEV),
                                          want_code=True, want_resid=True)
    assert same_bits(cov["pose"], want.cpu()) and torch.equal(cov["bone_code"], code.cpu()) and same_bits(cov["bone_resid"], resid.cpu())
    has = torch.from_numpy(parent >= 0)
    assert bool((got["bone_code"][:, :, has] == 1).all()) and bool((got["bone_code"][:, :, 24:92] == 0).all())
    assert same_bits(got["pose"][:, :, 24:92], got["pose_free"][:, :, 24:92]) and same_bits(got["pose"][:, :, 0], got["pose_free"][:, :, 0])
    # the snap: exact up to the two fp32 roundings of each of the six coordinates of a bone
    assert float(got["bone_resid"][..., 1].max()) <= snap_bound(got["pose"]) < float(got["bone_resid"][..., 0].min())
    assert bool((got["bone_frames"][:, has] == N_VIDEO).all()) and bool(torch.isfinite(got["pose"]).all())
    sym = out["symmetric"]
    length_sym = ops.bone_lengths(sym["pose_free"].to(DEV), cov["cov"].to(DEV), parent, mirror)
    assert same_bits(sym["bone_length"], length_sym.cpu()) and bool((sym["bone_frames"][:, 6:24] == 2 * N_VIDEO).all())
    assert same_bits(sym["bone_length"][:, gu.SYN_JOINTS_LEFT], sym["bone_length"][:, gu.SYN_JOINTS_RIGHT])
    assert same_bits(sym["pose"], ops.project_bones(sym["pose_free"].to(DEV), cov["cov"].to(DEV), parent, length_sym, iterations=4).cpu())
    own = out["own"]
    assert same_bits(own["bone_length"], runs[5].expand(2, 134)) and same_bits(own["bone_dev"], got["bone_dev"])
    assert same_bits(own["pose"], ops.project_bones(own["pose_free"].to(DEV), cov["cov"].to(DEV), parent, runs[5].to(DEV)).cpu())


def test_bones_run_behind_the_smoother_and_before_the_trajectory(runs):
    from pafuse_amd import harness
    out, _, seq_2d, _, cam, _ = runs
    got = out["smooth"]
    assert set(got) == {"pose", "count", "pose_raw", "pose_smooth_code"} | BONE_KEYS
    assert same_bits(got["pose_free"], out["smooth_only"]["pose"]) and same_bits(got["pose_raw"], out["plain"]["pose"])
    assert not same_bits(got["pose"], out["video"]["pose"])
    traj = out["traj"]
    assert set(traj) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"} | BONE_KEYS
    assert same_bits(traj["pose"], out["video"]["pose"])
    want = harness.fit_trajectory(traj["pose"], seq_2d, cam, smooth=3)
    assert all(same_bits(want[k], traj[k]) for k in want)
    assert not same_bits(harness.fit_trajectory(traj["pose_free"], seq_2d, cam, smooth=3)["traj"], traj["traj"])


def test_evaluate_frames_scores_the_constrained_pose(runs):
    from pafuse_amd import evaluate, h3wb, harness, ops
    out, model, seq_2d, seq_3d, cam, _ = runs
    ds = dataset()
    model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
    sums, counts, held = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="mean",
                                                 stride=9, trajectory=3, bone_lengths="video", bone_iterations=16)
    got = out["traj"]
    gt_wb = (seq_3d - seq_3d[:, :1]).to(DEV)
    m = evaluate.frame_metrics(got["pose"].to(DEV), gt_wb, ds, traj=got["traj"].to(DEV), gt_root=seq_3d[:, 0].contiguous().to(DEV))
    assert set(m) == set(sums)
    for k in m:
        assert same_bits(m[k][0].cpu(), sums[k]) and torch.equal(m[k][1].cpu(), counts[k]), k
    parent, _ = h3wb.bone_tables(68)
    assert set(held) == {"bone_length", "bone_length_gt", "bone_dev_free", "bone_dev"}
    assert same_bits(held["bone_length"], got["bone_length"][-1])
    assert same_bits(held["bone_length_gt"], ops.bone_lengths(gt_wb.unsqueeze(0).contiguous(), None, parent).cpu()[0])
    assert tuple(held["bone_dev"].shape) == tuple(held["bone_dev_free"].shape) == (2,)
    assert torch.equal(held["bone_dev_free"], got["bone_dev"].double().nanmean(dim=1) * 1000.0)
    print("bone-length std, mm (synthetic weights: the sizes mean nothing): free", held["bone_dev_free"].tolist(), "constrained",
          held["bone_dev"].tolist())
    assert bool((held["bone_dev"] <= snap_bound(got["pose"]) * 1000.0).all())                 # held constant: the rounding is what is left
    assert bool((held["bone_dev_free"] > 100 * held["bone_dev"]).all())
    model.noise_seed = SEED
    raw_sums, _ = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="mean",
                                          stride=9, trajectory=3)
    assert not same_bits(raw_sums["mpjpe"], sums["mpjpe"])

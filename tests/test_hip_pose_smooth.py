"""The covariance-weighted pose smoother on the device: pose_smooth_kernel (pafuse_pose_smooth), ops.smooth_poses,
torch.ops.pafuse.pose_smooth, harness.smooth_poses, infer_sequence(pose_smooth=...) and evaluate_frames(pose_smooth=...).

What is asserted and why it can be asserted:
  * kernel vs statement: the kernel and pafuse_amd/posesmooth.py perform the same IEEE fp64 operations in the same order
    (contraction off, correctly rounded divides; the LDL^T loops are unrolled in the statement's order), then round once to
    fp32 -> the design goal is equal bits; the test accepts equal or ADJACENT fp32 values with NaN in the same places - the
    acceptance rule of tests/test_hip_rootfit.py - on EVERY value, and prints how many differ.  The codes are integers ->
    torch.equal.
  * everything else is same bits: guard rows (out, code and the workspace), two calls, code = NULL, a side stream, the Python
    layers over the entry.
Shapes: J in {1, 5, 64, 65, 134} - one lane, part of a wave, exactly a wave, a wave and a lane, a frame that is no multiple of
the wave or the workgroup - N in {1, 2, 9, 70} x r in {1, 3, 64} (r >= N: every frame sees every frame; r = 1 at N = 70: gaps
nothing reaches across), T in {1, 2}, with a covariance and without.  About 5 % of the rows NaN (pose or covariance), a few
indefinite.
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
CASES = [(J, N, r) for J in (1, 5, 64, 65, 134) for N in (1, 2, 9, 70) for r in (1, 3, 64)]
PAD = 7


def smooth_inputs(T, N, J, r, seed):
    """a noisy walk per joint with random anisotropic covariances (standard deviations 1 - 10 cm x (1, 0.3, 0.1), rotated);
    about 5 % of the rows without a pose or without a covariance, a few indefinite, an infinite coordinate, and - N
    permitting - a stretch longer than 2r + 1 frames without a pose"""
    rng = np.random.default_rng(seed)
    pose = (np.cumsum(rng.standard_normal((T, N, J, 3)) * 0.02, axis=1) + rng.standard_normal((T, 1, J, 3)) * 0.3).astype(np.float32)
    Q, _ = np.linalg.qr(rng.standard_normal((T, N, J, 3, 3)))
    sd = rng.uniform(0.01, 0.10, (T, N, J))[..., None] * np.array([1.0, 0.3, 0.1])
    S = np.einsum("...ik,...k,...jk->...ij", Q, sd * sd, Q)
    cov = np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2], S[..., 2, 2]], axis=-1).astype(np.float32)
    pose[rng.random((T, N, J)) < 0.03] = np.nan
    cov[rng.random((T, N, J)) < 0.02, rng.integers(0, 6)] = np.nan
    bad = rng.random((T, N, J)) < 0.02
    cov[bad, 3] = -cov[bad, 3]                                        # yy < 0: indefinite whatever the floor
    if N > 4:
        pose[0, 3, 0, 1] = np.inf
        cov[T - 1, 2, J - 1] = 0                                      # a row the floor alone carries
    if N == 70:
        pose[T - 1, 20:20 + min(2 * r + 4, 40), J // 2] = np.nan
    return pose, cov


def statement(pose, cov, r, floor=FLOOR):
    from pafuse_amd import posesmooth
    out, code = posesmooth.smooth(pose, cov, r, floor)
    return torch.from_numpy(out), torch.from_numpy(code)


# --------------------------------------------------------------------------------------------------- 6. kernel vs statement
@pytest.mark.parametrize("case", CASES)
def test_kernel_is_the_statement(case):
    from pafuse_amd import ops
    J, N, r = case
    differ = total = 0
    for T in (1, 2):
        pose, cov = smooth_inputs(T, N, J, r, seed=1000 * J + 10 * N + r + T)
        for c in (cov, None):
            got, code = ops.smooth_poses(torch.from_numpy(pose).to(DEV), None if c is None else torch.from_numpy(c).to(DEV), r,
                                         floor=FLOOR, want_code=True)
            want, want_code = statement(pose, c, r)
            assert tuple(got.shape) == (T, N, J, 3) and got.dtype == torch.float32 and code.dtype == torch.uint8
            assert torch.equal(code.cpu(), want_code), (T, c is None)
            differ += equal_or_adjacent(got.cpu(), want)              # every value; the same NaN pattern
            total += got.numel()
            assert torch.equal(torch.isnan(got.cpu()).any(-1), want_code == 3)
        if N == 70 and r == 1:
            assert bool((want_code[T - 1, 22:25, J // 2] == 3).all())   # the middle of a stretch without a pose stays NaN
    print(f"(J, N, r) = {case}: {differ} of {total} values differ from the statement (by one fp32 step)")


def test_floor_and_equal_covariances():
    """another floor is another result; cov = None is an all-zero cov, bit for bit; without a covariance the filter is the
    trajectory smoother's, joint by joint (equal or adjacent: two routes to one line)"""
    from pafuse_amd import ops
    pose, cov = smooth_inputs(2, 9, 65, 3, seed=5)
    p, c = torch.from_numpy(pose).to(DEV), torch.from_numpy(cov).to(DEV)
    a, b = ops.smooth_poses(p, c, 3, floor=1e-3), ops.smooth_poses(p, c, 3, floor=2e-2)
    assert not same_bits(a, b)
    want, _ = statement(pose, cov, 3, 2e-2)
    equal_or_adjacent(b.cpu(), want)
    none, zero = ops.smooth_poses(p, None, 3), ops.smooth_poses(p, torch.zeros_like(c), 3)
    assert same_bits(none, zero)
    tracks = p.permute(0, 2, 1, 3).reshape(2 * 65, 9, 3).contiguous()                # [T*J, N, 3]
    line = ops.smooth_trajectory(tracks, None, 3).view(2, 65, 9, 3).permute(0, 2, 1, 3)
    assert torch.equal(torch.isnan(line), torch.isnan(none))
    assert float(p[torch.isfinite(p)].abs().max()) < 2.0                              # so one fp32 step is at most eps
    assert bool(((torch.nan_to_num(line) - torch.nan_to_num(none)).abs() <= torch.finfo(torch.float32).eps).all())


# --------------------------------------------------------------------------------------------------- 7. other properties
def raw(pose, cov, T, N, J, r, floor, out, code, stream=None, workspace=None):
    """the bare entry on the null stream (or `stream`); workspace: a float64 tensor, or None: one of exactly the size asked for"""
    from pafuse_amd import _lib
    lib = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()
    if workspace is None:
        workspace = torch.empty(max(lib.pafuse_pose_smooth_workspace_bytes(T, N, J) // 8, 1), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
    rc = lib.pafuse_pose_smooth(ptr(pose), ptr(cov), T, N, J, r, floor, ptr(out), ptr(code), ptr(workspace), workspace.numel() * 8, stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 70, 64), (65, 9, 3), (1, 1, 1), (5, 2, 13)])
def test_guard_rows_repeat_calls_null_code_and_a_side_stream(case):
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import ops
    J, N, r = case
    T = 2
    pose, cov = (torch.from_numpy(a).to(DEV) for a in smooth_inputs(T, N, J, r, seed=77))
    n = T * N * J
    want, want_code = ops.smooth_poses(pose, cov, r, want_code=True)
    out = torch.full((PAD + n * 3 + PAD,), 7.0, device=DEV)
    code = torch.full((PAD + n + PAD,), 9, dtype=torch.uint8, device=DEV)
    ws = torch.full((PAD + n * 6 + PAD,), 7.0, dtype=torch.float64, device=DEV)
    assert ops.smooth_poses_workspace_bytes(T, N, J) == n * 48
    assert raw(pose, cov, T, N, J, r, FLOOR, out[PAD:], code[PAD:], workspace=ws[PAD:PAD + n * 6]) == 0
    assert bool((ws[:PAD] == 7.0).all()) and bool((ws[PAD + n * 6:] == 7.0).all())
    assert bool((out[:PAD] == 7.0).all()) and bool((out[PAD + n * 3:] == 7.0).all())
    assert bool((code[:PAD] == 9).all()) and bool((code[PAD + n:] == 9).all())
    assert same_bits(out[PAD:PAD + n * 3], want.reshape(-1)) and torch.equal(code[PAD:PAD + n], want_code.reshape(-1))
    again = torch.full((n * 3 + PAD,), 7.0, device=DEV)
    assert raw(pose, cov, T, N, J, r, FLOOR, again, None) == 0                       # code = NULL: the same out
    assert bool((again[n * 3:] == 7.0).all()) and same_bits(again[:n * 3], want.reshape(-1))
    assert same_bits(ops.smooth_poses(pose, cov, r), want)                           # two calls, the same bits
    given = torch.full((T, N, J, 3), 7.0, device=DEV)
    assert ops.smooth_poses(pose, cov, r, out=given, workspace=ws) is given and same_bits(given, want)   # a larger, reused workspace
    t_out, t_code = torch.ops.pafuse.pose_smooth(pose, cov, r, FLOOR)
    assert same_bits(t_out, want) and torch.equal(t_code, want_code)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, code_side = ops.smooth_poses(pose, cov, r, want_code=True)
    side.synchronize()
    assert same_bits(on_side, want) and torch.equal(code_side, want_code)
    other = torch.full((n * 3,), 7.0, device=DEV)
    torch.cuda.synchronize()                                                         # the fill is on another stream
    assert raw(pose, cov, T, N, J, r, FLOOR, other, None, stream=side.cuda_stream) == 0
    assert same_bits(other, want.reshape(-1))


def test_refusals_come_before_any_launch():
    from pafuse_amd import harness, ops
    pose = torch.zeros(1, 4, 5, 3, device=DEV)
    out = torch.full((1, 4, 5, 3), 7.0, device=DEV)
    for bad in (dict(r=0), dict(r=65), dict(floor=0.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(T=0), dict(J=-1)):
        a = dict(T=1, N=4, J=5, r=3, floor=FLOOR)
        a.update(bad)
        assert raw(pose, None, a["T"], a["N"], a["J"], a["r"], a["floor"], out, None) == -1, bad
    assert raw(pose, None, 1, 4, 5, 3, FLOOR, pose, None) == -1 and raw(None, None, 1, 4, 5, 3, FLOOR, out, None) == -1
    short = torch.empty(4 * 5 * 6 - 1, dtype=torch.float64, device=DEV)
    assert raw(pose, None, 1, 4, 5, 3, FLOOR, out, None, workspace=short) == -1
    with pytest.raises(ValueError, match="workspace"):
        ops.smooth_poses(pose, None, 3, workspace=short)
    with pytest.raises(ValueError, match="workspace"):
        ops.smooth_poses(pose, None, 3, workspace=torch.empty(4 * 5 * 6, device=DEV))          # fp32
    assert bool((out == 7.0).all())                                                  # nothing was launched on it
    with pytest.raises(ValueError, match="alias"):
        ops.smooth_poses(pose, None, 3, out=pose)
    with pytest.raises(ValueError, match="cov"):
        ops.smooth_poses(pose, torch.zeros(1, 4, 5, 3, device=DEV), 3)
    with pytest.raises(ValueError, match="dtypes"):
        ops.smooth_poses(pose.double(), None, 3)
    got = harness.smooth_poses(pose.cpu() + 1.0, None, radius=2)
    assert set(got) == {"pose", "pose_raw", "pose_smooth_code"} and all(not v.is_cuda for v in got.values())
    assert torch.equal(got["pose"], got["pose_raw"]) and bool((got["pose_smooth_code"] == 1).all())    # a constant is a line


# --------------------------------------------------------------------------------------------------- 8. integration
SEED = 9753
N_VIDEO = 30


@pytest.fixture(scope="module")
def runs():
    """infer_sequence(stride = 9, aggregate = "mean") on a 30-frame video, from the same start of the noise stream: without the
    keyword, with pose_smooth = None, with pose_smooth = 3 (alone; with spread = "cov"; with a smoothed trajectory); computed
    once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, seq_3d, cam = sequence(N_VIDEO)
    out = {}
    for name, kw in (("plain", dict()), ("none", dict(pose_smooth=None)), ("smooth", dict(pose_smooth=3)),
                     ("cov", dict(pose_smooth=3, spread="cov")), ("plain_cov", dict(spread="cov")),
                     ("traj", dict(pose_smooth=3, pose_smooth_floor=1e-3, trajectory=3, cam=cam))):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        out[name] = harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2,
                                           aggregate="mean", stride=9, **kw)
    return out, model, seq_2d, seq_3d, cam


def test_infer_sequence_without_pose_smooth_is_unchanged(runs):
    out = runs[0]
    assert set(out["plain"]) == set(out["none"]) == {"pose", "count"}
    assert all(same_bits(out["plain"][k], out["none"][k]) for k in out["plain"])


def test_infer_sequence_smooths_the_returned_pose_with_the_pooled_covariance(runs):
    from pafuse_amd import ops
    out = runs[0]
    got, cov = out["smooth"], out["cov"]
    assert set(got) == {"pose", "count", "pose_raw", "pose_smooth_code"}
    assert set(cov) == set(got) | {"std", "cov"} and all(not v.is_cuda for v in cov.values())
    assert tuple(got["pose"].shape) == (2, N_VIDEO, 134, 3) and tuple(got["pose_smooth_code"].shape) == (2, N_VIDEO, 134)
    assert got["pose_smooth_code"].dtype == torch.uint8 and bool((got["pose_smooth_code"] == 1).all())
    assert torch.equal(got["pose_raw"], out["plain"]["pose"]) and same_bits(got["count"], out["plain"]["count"])
    for k in ("std", "cov"):                                                        # the spread describes the hypotheses: unchanged
        assert same_bits(cov[k], out["plain_cov"][k]), k
    want, code = ops.smooth_poses(cov["pose_raw"].to(DEV), cov["cov"].to(DEV), 3, want_code=True)
    assert same_bits(cov["pose"], want.cpu()) and torch.equal(cov["pose_smooth_code"], code.cpu())
    assert all(same_bits(got[k], cov[k]) for k in got)                               # folding the spread for it alone is the same fold
    assert not torch.equal(got["pose"], got["pose_raw"]) and bool(torch.isfinite(got["pose"]).all())


def test_everything_downstream_sees_the_smoothed_pose(runs):
    from pafuse_amd import harness
    out, _, seq_2d, _, cam = runs
    got = out["traj"]
    assert set(got) == {"pose", "count", "pose_raw", "pose_smooth_code", "traj", "traj_raw", "traj_weight", "traj_resid"}
    assert same_bits(got["pose"], out["smooth"]["pose"]) and same_bits(got["pose_raw"], out["plain"]["pose"])
    want = harness.fit_trajectory(got["pose"], seq_2d, cam, smooth=3)
    assert all(same_bits(want[k], got[k]) for k in want)
    on_raw = harness.fit_trajectory(got["pose_raw"], seq_2d, cam, smooth=3)
    assert not same_bits(on_raw["traj"], got["traj"])


def test_batching_does_not_matter(runs):
    from pafuse_amd import harness
    from tests.test_hip_windows import noise_per_window
    _, model, seq_2d, _, _ = runs
    got = []
    for batch_size in (1, 4):
        noise_per_window(model)
        try:
            got.append(harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=batch_size,
                                              aggregate="mean", stride=9, pose_smooth=3))
        finally:
            model.noise_fn = None
    a, b = got
    assert set(a) == set(b) == {"pose", "count", "pose_raw", "pose_smooth_code"}
    assert all(same_bits(a[k], b[k]) for k in a)


def test_pick_is_smoothed_with_the_mean_filled_in(runs):
    """with "reproj_fit" the smoothed pose is the pick with the pooled mean where idx is -1; idx and window still name the pick"""
    from pafuse_amd import harness, ops
    _, model, seq_2d, _, cam = runs
    conf = torch.ones(N_VIDEO, 134)
    conf[4:7, 20] = 0                                                                # no weight: no pick, the mean is filled in
    res = {}
    for name, kw in (("plain", dict(spread="cov")), ("smooth", dict(spread="cov", pose_smooth=3, pose_smooth_floor=5e-3))):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        res[name] = harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2,
                                           aggregate="reproj_fit", cam=cam, conf=conf, stride=9, **kw)
    plain, got = res["plain"], res["smooth"]
    assert set(got) == set(plain) | {"pose_raw", "pose_smooth_code"}
    for k in plain:
        assert same_bits(plain[k], got["pose_raw"] if k == "pose" else got[k]), k
    assert bool((got["idx"][:, 4:7, 20] == -1).all()) and bool(torch.isfinite(got["pose_raw"][:, 4:7, 20]).all())
    want = ops.smooth_poses(got["pose_raw"].to(DEV), got["cov"].to(DEV), 3, floor=5e-3)
    assert same_bits(got["pose"], want.cpu())


def test_evaluate_frames_scores_the_smoothed_pose(runs):
    from pafuse_amd import evaluate, harness
    out, model, seq_2d, seq_3d, cam = runs
    ds = dataset()
    model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
    sums, counts = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="mean",
                                           stride=9, trajectory=3, pose_smooth=3)
    got = out["traj"]
    gt_root = seq_3d[:, 0].contiguous()
    m = evaluate.frame_metrics(got["pose"].to(DEV), (seq_3d - seq_3d[:, :1]).to(DEV), ds, traj=got["traj"].to(DEV), gt_root=gt_root.to(DEV))
    assert set(m) == set(sums)
    for k in m:
        assert same_bits(m[k][0].cpu(), sums[k]) and torch.equal(m[k][1].cpu(), counts[k]), k
    model.noise_seed = SEED
    raw_sums, _ = harness.evaluate_frames(model, ds, seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="mean",
                                          stride=9, trajectory=3)
    print("accel sums (synthetic weights: the sizes mean nothing): per-frame mean", raw_sums["accel"].tolist(), "smoothed, r = 3",
          sums["accel"].tolist())
    assert not same_bits(raw_sums["mpjpe"], sums["mpjpe"])

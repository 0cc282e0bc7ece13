"""The camera-space root trajectory on the device: frames_root_fit_kernel (pafuse_frames_root_fit), trajectory_smooth_kernel
(pafuse_trajectory_smooth), ops.fit_trajectory / smooth_trajectory, torch.ops.pafuse.fit_trajectory / smooth_trajectory and
infer_sequence(stride=..., trajectory=...).

What is asserted and why it can be asserted:
  * fit vs statement: the kernel and pafuse_amd/trajectory.py perform the same IEEE fp64 operations in the same order (every sum
    over the joints in the pinned lane order, contraction off, correctly rounded divides and square root), then round once to
    fp32 -> the design goal is equal bits; the test accepts equal or ADJACENT fp32 values with NaN in the same places - the
    acceptance rule of tests/test_hip_rootfit.py - and prints how many differ.
  * fit vs the existing kernel: on a finite pose run as a single hypothesis (B = 1, P_r = 1, F = N, a connection table of zeros:
    wb_joint adds joint 0, which a whole-body pose pins at 0) pafuse_pose_partials_fit's tfit is the same arithmetic ->
    torch.equal.
  * smoother vs statement: the same rule; a line with integer values, unit weights and r = 3 is exact in fp64 -> torch.equal.
Shapes: J in {5, 64, 65, 134} - lanes without a joint, exactly one round, one joint in a second round, the real three rounds
with a ragged third - and 200, 300 for the four-slot kernel and the round-by-round kernel behind J = 256; N in {1, 2, 7} and T in
{1, 2}: one wave, less than a workgroup of four waves, up to four workgroups with a ragged last one.  Smoother: N in
{1, 2, 9, 70} x r in {1, 3, 64} (r >= N; T = 4 at N = 70: 280 threads, two workgroups with a ragged second).
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT_TRUE = (0.3, -0.2, 4.5)
CAM = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
FIT_CASES = [(J, N, T) for J in (5, 64, 65, 134) for N in (1, 2, 7) for T in (1, 2)] + [(200, 7, 2), (300, 7, 2)]
SMOOTH_CASES = [(N, r) for N in (1, 2, 9, 70) for r in (1, 3, 64)]
PAD = 5


def fit_inputs(J, N, T, seed, planted_nan=True, nan_frame=True):
    """poses scattered 5 cm per step about a pose seen from a root that walks away from ROOT_TRUE, its detections with 2 %
    noise; a fifth of the weights 0 (detection (0, 0)); planted_nan: one joint's pose NaN, and (nan_frame) one frame
    entirely NaN"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(N, J, 3, generator=g) * 0.2
    base[:, 0] = 0
    root = torch.tensor(ROOT_TRUE, dtype=torch.float64) + torch.arange(N, dtype=torch.float64)[:, None] * torch.tensor([0.05, 0.0, 0.02], dtype=torch.float64)
    X = base.double() + root[:, None]
    fx, fy, cx, cy = (float(v) for v in CAM[:4])
    x2d = torch.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], dim=-1).float()
    x2d = x2d + torch.randn(N, J, 2, generator=g) * 0.02
    pose = (base[None] + torch.randn(T, N, J, 3, generator=g) * 0.05).contiguous()
    pose[:, :, 0] = 0
    conf = torch.rand(N, J, generator=g) * 0.9 + 0.1
    lost = torch.rand(N, J, generator=g) < 0.2
    lost[:, :3] = False                                          # joints 0 .. 2 stay: a frame with a pose has a fit
    conf[lost] = 0
    x2d[lost] = 0
    if planted_nan:
        pose[0, 0, min(3, J - 1), 1] = float("nan")
        if nan_frame:
            pose[T - 1, N - 1] = float("nan")
    return {"pose": pose.to(DEV), "x2d": x2d.contiguous().to(DEV), "conf": conf.to(DEV), "cam": CAM.to(DEV)}


def statement(z):
    from pafuse_amd import trajectory
    return [torch.from_numpy(v) for v in trajectory.fit_frames(z["pose"].cpu().numpy(), z["x2d"].cpu().numpy(),
                                                               z["conf"].cpu().numpy(), z["cam"].cpu().numpy())]


def check_fit(z, case, note=""):
    from pafuse_amd import ops
    got = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    want = statement(z)
    T, N = z["pose"].shape[:2]
    assert tuple(got["traj"].shape) == (T, N, 3) and tuple(got["wsum"].shape) == tuple(got["resid"].shape) == (T, N)
    differ = {k: equal_or_adjacent(got[k].cpu(), w) for k, w in zip(("traj", "wsum", "resid"), want)}
    print(f"(J, N, T) = {case}{note}: values that differ from the statement (by one fp32 step): {differ} of {got['traj'].numel()} / "
          f"{got['wsum'].numel()} / {got['resid'].numel()}")
    return got, want


@pytest.mark.parametrize("case", FIT_CASES)
def test_fit_is_the_statement(case):
    J, N, T = case
    z = fit_inputs(J, N, T, seed=100 + 7 * J + 3 * N + T)
    got, want = check_fit(z, case)
    nofit = torch.isnan(want[0]).any(-1)
    assert bool(nofit[T - 1, N - 1]) and int(nofit.sum()) == 1      # the all-NaN frame and nothing else
    assert bool((got["wsum"].cpu()[nofit] == 0).all()) and bool((got["wsum"].cpu()[~nofit] > 0).all())
    if T * N == 1:      # the only frame is the NaN frame: the fit itself runs on the same inputs without it
        got, want = check_fit(fit_inputs(J, N, T, seed=100 + 7 * J + 3 * N + T, nan_frame=False), case, " without the NaN frame")
        assert not bool(torch.isnan(want[0]).any())
    if J >= 134:        # and it is a root, not just a number (tests/test_hip_rootfit.py: the depth within 1 m of the truth)
        fitted = ~torch.isnan(got["traj"][..., 2])
        assert bool(((got["traj"][..., 2] - ROOT_TRUE[2]).abs()[fitted] < 1.0).all())


@pytest.mark.parametrize("case", [(5, 7, 2), (64, 2, 1), (65, 7, 2), (134, 7, 2), (134, 1, 1), (300, 2, 2)])
def test_fit_is_the_existing_kernels_fit_of_one_hypothesis(case):
    from pafuse_amd import ops
    J, N, T = case
    z = fit_inputs(J, N, T, seed=500 + J + N + T, planted_nan=False)
    traj = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"], conf=z["conf"], want=("traj",))["traj"]
    cam9 = z["cam"]
    tfit = torch.full((1, T, 1, N, 3), 7.0, device=DEV)
    ops.pose_partials_fit(z["pose"].view(1, T, 1, N, J, 3), torch.zeros(J, dtype=torch.int32, device=DEV), 0, z["x2d"].view(1, N, J, 2),
                          cam9, conf=z["conf"].view(1, N, J), tfit=tfit)
    assert not bool(torch.isnan(tfit).any())
    assert torch.equal(traj, tfit.view(T, N, 3))


def test_fit_outputs_are_optional_and_the_torch_op_is_the_op():
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import ops
    z = fit_inputs(134, 7, 2, seed=9)
    full = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    only = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"], conf=z["conf"], want=("traj",))
    assert set(only) == {"traj"} and same_bits(only["traj"], full["traj"])
    t, w, r = torch.ops.pafuse.fit_trajectory(z["pose"], z["x2d"], z["cam"], z["conf"])
    assert same_bits(t, full["traj"]) and same_bits(w, full["wsum"]) and same_bits(r, full["resid"])
    ones = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"], conf=torch.ones_like(z["conf"]))
    none = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"])         # conf=None is every weight 1
    assert all(same_bits(none[k], ones[k]) for k in none)


def raw(name, *args):
    from pafuse_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 7, 2), (65, 1, 1), (300, 2, 1)])
def test_fit_canaries(case):
    from pafuse_amd import ops
    J, N, T = case
    z = fit_inputs(J, N, T, seed=77)
    bufs = {k: torch.full((n + PAD,), 7.0, device=DEV) for k, n in (("traj", T * N * 3), ("wsum", T * N), ("resid", T * N))}
    assert raw("pafuse_frames_root_fit", z["pose"], z["x2d"], z["conf"], z["cam"], T, N, J, bufs["traj"], bufs["wsum"], bufs["resid"]) == 0
    want = ops.fit_trajectory(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    for k, n in (("traj", T * N * 3), ("wsum", T * N), ("resid", T * N)):
        assert bool((bufs[k][n:] == 7.0).all()), k
        assert same_bits(bufs[k][:n], want[k].reshape(-1)), k


# ------------------------------------------------------------------------------------------------------------ smoother
def smooth_inputs(N, r, seed):
    """a noisy walk with random weights; zero weights, a NaN weight, NaN frames and (N permitting) a gap longer than 2r + 1"""
    T = 4 if N == 70 else 2
    g = torch.Generator().manual_seed(seed)
    traj = torch.cumsum(torch.randn(T, N, 3, generator=g) * 0.05, dim=1) + torch.tensor(ROOT_TRUE)
    weight = torch.rand(T, N, generator=g) * 50 + 1
    weight[torch.rand(T, N, generator=g) < 0.15] = 0
    nan = torch.rand(T, N, generator=g) < 0.15
    traj[nan] = float("nan")
    if N > 4:
        traj[0, 3, 1] = float("inf")
        weight[1, 2] = float("nan")
        weight[1, 4] = -1.0
    if N == 70:
        traj[2, 20:20 + min(2 * r + 4, 40)] = float("nan")
    return traj.contiguous().to(DEV), weight.contiguous().to(DEV)


@pytest.mark.parametrize("case", SMOOTH_CASES)
def test_smooth_is_the_statement(case):
    from pafuse_amd import ops, trajectory
    N, r = case
    traj, weight = smooth_inputs(N, r, seed=31 * N + r)
    got = ops.smooth_trajectory(traj, weight, r)
    want = torch.from_numpy(trajectory.smooth(traj.cpu().numpy(), weight.cpu().numpy(), r))
    differ = equal_or_adjacent(got.cpu(), want)
    print(f"(N, r) = {case}: {differ} of {got.numel()} values differ from the statement (by one fp32 step); {int(torch.isnan(want).sum())} NaN")
    unweighted = ops.smooth_trajectory(traj, None, r)
    want = torch.from_numpy(trajectory.smooth(traj.cpu().numpy(), None, r))
    equal_or_adjacent(unweighted.cpu(), want)
    if N == 70 and r == 1:
        assert bool(torch.isnan(got[2, 22:25]).all())               # the middle of a stretch without fits stays NaN


def test_smooth_returns_a_line_exactly():
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import ops
    n = torch.arange(70, dtype=torch.float32)
    y = torch.stack([3 * n - 7, -2 * n + 40, n + 4000], dim=-1)
    y = torch.stack([y, y + 5]).contiguous().to(DEV)
    assert torch.equal(ops.smooth_trajectory(y, None, 3), y)
    w = torch.ones(2, 70, device=DEV)
    hole = y.clone()
    w[0, 5] = 0
    hole[0, 5] = 123.0
    hole[1, 7] = float("nan")
    hole[1, 69, 2] = float("nan")
    assert torch.equal(ops.smooth_trajectory(hole, w, 3), y)
    assert torch.equal(torch.ops.pafuse.smooth_trajectory(hole, w, 3), y)


@pytest.mark.parametrize("case", [(70, 64), (9, 3), (1, 1)])
def test_smooth_canaries(case):
    from pafuse_amd import ops
    N, r = case
    traj, weight = smooth_inputs(N, r, seed=5)
    T = traj.shape[0]
    buf = torch.full((T * N * 3 + PAD,), 7.0, device=DEV)
    assert raw("pafuse_trajectory_smooth", traj, weight, T, N, r, buf) == 0
    assert bool((buf[T * N * 3:] == 7.0).all())
    assert same_bits(buf[:T * N * 3], ops.smooth_trajectory(traj, weight, r).reshape(-1))
    out = torch.full((T, N, 3), 7.0, device=DEV)
    assert ops.smooth_trajectory(traj, weight, r, out=out) is out and same_bits(out.reshape(-1), buf[:T * N * 3])


# --------------------------------------------------------------------------------------------------------- infer_sequence
SEED = 4321
F27 = 27
N_VIDEO = 2 * F27 + 1


@pytest.fixture(scope="module")
def runs():
    """infer_sequence(stride = F - 1, aggregate = "mean") on the seeded video with trajectory = 3 and without, from the same
    start of the noise stream; computed once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, _, cam = sequence(N_VIDEO)
    out = {}
    for name, kw in (("traj", dict(trajectory=3, cam=cam)), ("plain", dict())):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        out[name] = harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2,
                                           aggregate="mean", stride=F27 - 1, **kw)
    return out, seq_2d, cam


def test_infer_sequence_trajectory_is_the_ops_pair_on_the_returned_pose(runs):
    from pafuse_amd import harness, ops
    (out, seq_2d, cam) = runs
    got = out["traj"]
    assert set(got) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"}
    assert all(not v.is_cuda for v in got.values())
    assert tuple(got["traj"].shape) == tuple(got["traj_raw"].shape) == (2, N_VIDEO, 3)
    assert tuple(got["traj_weight"].shape) == tuple(got["traj_resid"].shape) == (2, N_VIDEO)
    want = ops.fit_trajectory(got["pose"].to(DEV), seq_2d.to(DEV), cam.to(DEV))
    assert same_bits(got["traj_raw"], want["traj"].cpu()) and same_bits(got["traj_weight"], want["wsum"].cpu())
    assert same_bits(got["traj_resid"], want["resid"].cpu())
    assert same_bits(got["traj"], ops.smooth_trajectory(want["traj"], want["wsum"], 3).cpu())
    assert bool(torch.isfinite(got["traj"]).all()) and bool((got["traj_weight"] == 134).all())
    again = harness.fit_trajectory(got["pose"], seq_2d, cam, smooth=3)      # the same keys from the per-frame array
    assert set(again) == {"traj", "traj_raw", "traj_weight", "traj_resid"} and all(same_bits(again[k], got[k]) for k in again)
    raw_only = harness.fit_trajectory(got["pose"], seq_2d, cam)
    assert set(raw_only) == {"traj", "traj_weight", "traj_resid"} and same_bits(raw_only["traj"], got["traj_raw"])


def test_infer_sequence_without_trajectory_is_unchanged(runs):
    out = runs[0]
    assert set(out["plain"]) == {"pose", "count"}
    for k, v in out["plain"].items():
        assert same_bits(v, out["traj"][k]), k


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch():
    from pafuse_amd import _lib, harness, ops
    lib = _lib.load()
    z = fit_inputs(5, 2, 1, seed=1)
    traj = torch.full((1, 2, 3), 7.0, device=DEV)
    out = torch.full((1, 2, 3), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    E_ARG = -1
    ok = [p(z["pose"]), p(z["x2d"]), p(z["conf"]), p(z["cam"]), 1, 2, 5, p(traj), None, None, None]
    for i in (0, 1, 3, 7):
        a = list(ok)
        a[i] = None
        assert lib.pafuse_frames_root_fit(*a) == E_ARG, i
    ok = [p(traj), None, 1, 2, 3, p(out), None]
    for i, v in ((0, None), (5, None), (4, 0), (4, 65), (5, p(traj))):
        a = list(ok)
        a[i] = v
        assert lib.pafuse_trajectory_smooth(*a) == E_ARG, (i, v)
    with pytest.raises(ValueError, match="radius"):
        ops.smooth_trajectory(traj, None, 0)
    with pytest.raises(ValueError, match="radius"):
        ops.smooth_trajectory(traj, None, 65)
    with pytest.raises(ValueError, match="alias"):
        ops.smooth_trajectory(traj, None, 3, out=traj)
    with pytest.raises(ValueError, match="x2d and cam"):
        ops.fit_trajectory(z["pose"], None, z["cam"])
    with pytest.raises(ValueError, match="x2d and cam"):
        ops.fit_trajectory(z["pose"], z["x2d"], None)
    torch.cuda.synchronize()
    assert bool((traj == 7.0).all()) and bool((out == 7.0).all())    # nothing was launched on them
    model = torch.nn.Linear(1, 1).to(DEV)
    model.frames = F27
    seq_2d, _, cam = sequence(N_VIDEO)
    with pytest.raises(ValueError, match="harness.fit_trajectory"):
        harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="mean", cam=cam, trajectory=3)
    with pytest.raises(ValueError, match="cam"):
        harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="mean", stride=9, trajectory=3)

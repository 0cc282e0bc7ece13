"""The focal-length estimate on the device: frames_focal_sums_kernel (pafuse_frames_focal_sums), focal_solve_kernel
(pafuse_focal_solve), ops.focal_sums / focal_solve / estimate_focal, torch.ops.pafuse.focal_sums / focal_solve and
infer_sequence(trajectory=..., focal="estimate").

What is asserted and why it can be asserted:
  * state vs statement: the kernel and pafuse_amd/focal.py perform the same IEEE fp64 operations in the same order (every sum over
    the joints in the pinned lane order, contraction off, correctly rounded divides) -> the design goal is equal bits; the test
    accepts equal or ADJACENT fp64 values - the acceptance rule of tests/test_hip_rootfit.py - and prints how many differ.  The
    participation slot is 0.0 or 1.0 and compared with torch.equal.
  * solve vs statement on the kernel's own state: the same, in fp32 after the one rounding, NaN in the same places; the frame count
    and the copied slots of cam_out are integers and copies -> torch.equal.
  * planted focal length: the bound of tests/test_focal_host.py, 1e-5 relative (the fp32 rounding of the detections limits it);
    the root fit with the returned intrinsics recovers the planted roots within 1e-5 m (3e-7 relative in f at 4 m is about 1.2e-6 m)
    with a residual below 1e-5 m.
Shapes: those of tests/test_hip_trajectory.py for the sums - J in {5, 64, 65, 134} (lanes without a joint, exactly one round, one
joint in a second round, three rounds with a ragged third), 200 and 300 (the four-slot kernel and the round-by-round kernel
behind J = 256), N in {1, 2, 7}, T in {1, 2} - and N in {1, 2, 63, 64, 65, 130} for the solve: fewer frames than lanes, exactly
one round, one frame in a second round, a ragged third.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_focal_host import CAM_TRUE, F_TRUE, guess, planted
from tests.test_hip_partials import dataset, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent
from tests.test_hip_trajectory import FIT_CASES, fit_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 5
E_ARG = -1
SOLVE_CASES = (1, 2, 63, 64, 65, 130)


def on_device(pose, uv, c, cam):
    return [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (pose, uv, c, cam)]


def state_statement(z):
    from pafuse_amd import focal
    return torch.from_numpy(focal.focal_sums(z["pose"].cpu().numpy(), z["x2d"].cpu().numpy(), z["conf"].cpu().numpy(), z["cam"].cpu().numpy()))


@pytest.mark.parametrize("case", FIT_CASES)
def test_state_is_the_statement(case):
    from pafuse_amd import ops
    J, N, T = case
    z = fit_inputs(J, N, T, seed=300 + 7 * J + 3 * N + T)
    got = ops.focal_sums(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    want = state_statement(z)
    assert tuple(got.shape) == (T, N, 4) and got.dtype == torch.float64
    differ = equal_or_adjacent(got.cpu(), want)
    print(f"(J, N, T) = {case}: {differ} of {got.numel()} state values differ from the statement (by one fp64 step)")
    assert torch.equal(got.cpu()[..., 3], want[..., 3])
    assert not bool(got[T - 1, N - 1].any())                         # the all-NaN frame: exactly (0, 0, 0, 0)
    joints = ((z["conf"] > 0)[None] & torch.isfinite(z["pose"]).all(-1)).sum(-1).cpu()      # [T,N]: at J = 5 a frame can fall below 4
    assert torch.equal(got.cpu()[..., 3], (joints >= 4).double())
    none = ops.focal_sums(z["pose"], z["x2d"], z["cam"])             # conf=None is every weight 1
    ones = ops.focal_sums(z["pose"], z["x2d"], z["cam"], conf=torch.ones_like(z["conf"]))
    assert same_bits(none, ones)


@pytest.mark.parametrize("N", SOLVE_CASES)
def test_solve_is_the_statement_on_the_kernels_state(N):
    from pafuse_amd import focal, ops
    T, J = 2, 134
    z = fit_inputs(J, N, T, seed=700 + N)
    state = ops.focal_sums(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    got = ops.focal_solve(state, z["cam"])
    f, r2, frames, cam_out = (torch.from_numpy(v) for v in focal.focal_solve(state.cpu().numpy(), z["cam"].cpu().numpy()))
    differ = (equal_or_adjacent(got["focal"].cpu(), f), equal_or_adjacent(got["r2"].cpu(), r2),
              equal_or_adjacent(got["cam"].cpu()[:, :2], cam_out[:, :2]))
    print(f"N = {N}: focal {got['focal'].tolist()}, r2 {got['r2'].tolist()}, frames {got['frames'].tolist()}; values that differ "
          f"from the statement (by one fp32 step) in focal / r2 / cam[:, :2]: {differ}")
    assert got["frames"].dtype == torch.int32 and torch.equal(got["frames"].cpu(), frames)
    assert frames.tolist() == [N, N - 1]
    assert torch.equal(got["cam"].cpu()[:, 2:], cam_out[:, 2:]) and torch.equal(cam_out[:, 2:], z["cam"].cpu()[2:].expand(T, 7))
    assert same_bits(got["cam"][:, 0], got["focal"])
    if N == 1:                                                      # step 1 holds the NaN frame alone: no estimate
        assert bool(torch.isnan(got["focal"][1])) and bool(torch.isnan(got["r2"][1])) and bool(torch.isnan(got["cam"][1, :2]).all())
    both = ops.estimate_focal(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    assert set(both) == {"focal", "r2", "frames", "cam"} and all(same_bits(both[k], got[k]) for k in got)
    # the states of two videos concatenate along N
    z2 = fit_inputs(J, 7, T, seed=5)
    s2 = ops.focal_sums(z2["pose"], z2["x2d"], z2["cam"], conf=z2["conf"])
    joint = ops.focal_solve(torch.cat([state, s2], dim=1).contiguous(), z["cam"], want=("focal", "frames"))
    assert joint["frames"].tolist() == [N + 7, N + 5]


@pytest.mark.parametrize("case", [(5, 1), (65, 2), (134, 70), (300, 7)])
def test_planted_focal_length_and_roots_are_recovered(case):
    from pafuse_amd import ops
    J, N = case
    pose, uv, c, root = planted(J, N, seed=10 + 3 * J + N)
    pose, uv, c, cam = on_device(pose, uv, c, guess())
    state = ops.focal_sums(pose, uv, cam, conf=c)
    tot = state.sum(dim=1)[0].cpu()
    est = ops.focal_solve(state, cam)
    f = float(est["focal"][0])
    print(f"(J, N) = {case}: focal {f!r}, relative error {abs(f / F_TRUE - 1):.3g} (fp64 sums: {abs(float(tot[0] / tot[1]) / F_TRUE - 1):.3g}), "
          f"1 - r2 = {1 - float(est['r2'][0]):.3g}")
    assert int(est["frames"][0]) == N
    assert abs(f / float(CAM_TRUE[0]) - 1) <= 1e-5
    assert abs(float(est["r2"][0]) - 1) <= 1e-6
    fit = ops.fit_trajectory(pose, uv, est["cam"][0], conf=c)
    err = float((fit["traj"][0].double().cpu() - torch.from_numpy(root)).abs().max())
    print(f"    roots fitted with the estimated intrinsics: |t - t_true| = {err:.3g} m, resid {float(fit['resid'].max()):.3g} m")
    assert err <= 1e-5 and float(fit["resid"].max()) < 1e-5


def raw(name, *args):
    from pafuse_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 7, 2), (65, 1, 1), (300, 2, 1)])
def test_canaries_optional_outputs_and_the_torch_op(case):
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import ops
    J, N, T = case
    z = fit_inputs(J, N, T, seed=77, nan_frame=False)
    want = ops.focal_sums(z["pose"], z["x2d"], z["cam"], conf=z["conf"])
    state = torch.full((T * N * 4 + PAD,), 7.0, device=DEV, dtype=torch.float64)
    assert raw("pafuse_frames_focal_sums", z["pose"], z["x2d"], z["conf"], z["cam"], T, N, J, state) == 0
    assert bool((state[T * N * 4:] == 7.0).all()) and same_bits(state[:T * N * 4], want.reshape(-1))
    assert same_bits(torch.ops.pafuse.focal_sums(z["pose"], z["x2d"], z["cam"], z["conf"]), want)
    for L in (9, 4):
        cam = z["cam"][:L].contiguous()
        full = ops.focal_solve(want, cam)
        sizes = (("focal", T, torch.float32), ("r2", T, torch.float32), ("frames", T, torch.int32), ("cam", T * L, torch.float32))
        bufs = {k: torch.full((n + PAD,), 7, device=DEV, dtype=dt) for k, n, dt in sizes}
        assert raw("pafuse_focal_solve", want, T, N, cam, L, bufs["focal"], bufs["r2"], bufs["frames"], bufs["cam"]) == 0
        for k, n, _ in sizes:
            assert bool((bufs[k][n:] == 7).all()), (k, L)
            assert same_bits(bufs[k][:n], full[k].reshape(-1)), (k, L)
        lone = torch.full((T + PAD,), 7.0, device=DEV)
        assert raw("pafuse_focal_solve", want, T, N, cam, L, lone, None, None, None) == 0      # the optional outputs may be NULL
        assert bool((lone[T:] == 7.0).all()) and same_bits(lone[:T], full["focal"])
        only = ops.focal_solve(want, cam, want=("focal",))
        assert set(only) == {"focal"} and same_bits(only["focal"], full["focal"])
        assert tuple(full["cam"].shape) == (T, L)
    f, r2, frames, cam_out = torch.ops.pafuse.focal_solve(want, z["cam"])
    full = ops.focal_solve(want, z["cam"])
    assert same_bits(f, full["focal"]) and same_bits(r2, full["r2"]) and same_bits(frames, full["frames"]) and same_bits(cam_out, full["cam"])


def test_refusals_come_before_any_launch():
    from pafuse_amd import _lib, ops
    lib = _lib.load()
    z = fit_inputs(5, 2, 1, seed=1)
    p = lambda t: t.data_ptr()
    state = torch.full((1, 2, 4), 7.0, device=DEV, dtype=torch.float64)
    outs = {k: torch.full((9,), 7, device=DEV, dtype=dt) for k, dt in (("focal", torch.float32), ("r2", torch.float32),
                                                                       ("frames", torch.int32), ("cam", torch.float32))}
    ok = [p(z["pose"]), p(z["x2d"]), p(z["conf"]), p(z["cam"]), 1, 2, 5, p(state), None]
    for i, v in ((0, None), (1, None), (3, None), (7, None), (4, 0), (5, 0), (6, 0)):
        a = list(ok)
        a[i] = v
        assert lib.pafuse_frames_focal_sums(*a) == E_ARG, (i, v)
    ok = [p(state), 1, 2, p(z["cam"]), 9, p(outs["focal"]), p(outs["r2"]), p(outs["frames"]), p(outs["cam"]), None]
    for i, v in ((0, None), (3, None), (5, None), (1, 0), (2, 0), (4, 3), (4, 10)):
        a = list(ok)
        a[i] = v
        assert lib.pafuse_focal_solve(*a) == E_ARG, (i, v)
    with pytest.raises(ValueError, match="x2d and cam"):
        ops.focal_sums(z["pose"], z["x2d"], None)
    with pytest.raises(ValueError, match=r"4 \.\. 9"):
        ops.focal_solve(state, z["cam"][:3].contiguous())
    with pytest.raises(ValueError, match=r"4 \.\. 9"):
        ops.focal_solve(state, torch.zeros(10, device=DEV))
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and all(bool((v == 7).all()) for v in outs.values())      # nothing was launched on them


# --------------------------------------------------------------------------------------------------------- infer_sequence
SEED = 4321
F27 = 27
N_VIDEO = 2 * F27 + 1
FOCAL_KEYS = {"focal", "focal_r2", "focal_frames", "cam"}


@pytest.fixture(scope="module")
def runs():
    """infer_sequence(stride = F - 1, aggregate = "mean", trajectory = 3) on the seeded video with focal = "estimate" and no cam, and
    with focal = None and a given cam, from the same start of the noise stream; computed once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, _, cam = sequence(N_VIDEO)
    out = {}
    for name, kw in (("estimate", dict(focal="estimate")), ("given", dict(cam=cam))):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        out[name] = harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2,
                                           aggregate="mean", stride=F27 - 1, trajectory=3, **kw)
    return out, seq_2d, cam


def test_infer_sequence_fits_the_root_with_the_estimate_of_the_last_step(runs):
    from pafuse_amd import harness, ops
    out, seq_2d, cam = runs
    got = out["estimate"]
    assert set(got) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"} | FOCAL_KEYS
    assert all(not v.is_cuda for v in got.values())
    T = got["pose"].shape[0]
    assert T == 2 and tuple(got["focal"].shape) == tuple(got["focal_r2"].shape) == tuple(got["focal_frames"].shape) == (T,)
    assert tuple(got["cam"].shape) == (T, 9) and got["focal_frames"].dtype == torch.int32
    print(f"focal {got['focal'].tolist()}, r2 {got['focal_r2'].tolist()}, frames {got['focal_frames'].tolist()} (synthetic weights: the numbers mean nothing)")
    pose, x2d = got["pose"].to(DEV), seq_2d.to(DEV)
    square = torch.tensor([1.0, 1, 0, 0, 0, 0, 0, 0, 0], device=DEV)
    est = ops.estimate_focal(pose, x2d, square)
    for k, name in (("focal", "focal"), ("r2", "focal_r2"), ("frames", "focal_frames"), ("cam", "cam")):
        assert same_bits(got[name], est[k].cpu()), name
    want = ops.fit_trajectory(pose, x2d, got["cam"][T - 1].to(DEV))
    assert same_bits(got["traj_raw"], want["traj"].cpu()) and same_bits(got["traj_weight"], want["wsum"].cpu())
    assert same_bits(got["traj_resid"], want["resid"].cpu())
    assert same_bits(got["traj"], ops.smooth_trajectory(want["traj"], want["wsum"], 3).cpu())
    if bool(torch.isnan(got["focal"][T - 1])):                       # no estimate: a NaN trajectory, not a guessed one
        assert bool(torch.isnan(got["traj_raw"]).all())
    again = harness.fit_trajectory(got["pose"], seq_2d, smooth=3, focal="estimate")      # the same keys from the per-frame array
    assert set(again) == {"traj", "traj_raw", "traj_weight", "traj_resid"} | FOCAL_KEYS and all(same_bits(again[k], got[k]) for k in again)
    alone = harness.estimate_focal(got["pose"], seq_2d)
    assert set(alone) == FOCAL_KEYS and all(same_bits(alone[k], got[k]) for k in alone)
    kept = harness.estimate_focal(got["pose"], seq_2d, cam=cam)      # a given cam keeps its principal point, aspect and distortion
    assert torch.equal(kept["cam"][:, 2:], cam[2:].expand(T, 7))


def test_infer_sequence_with_a_given_cam_is_unchanged(runs):
    from pafuse_amd import ops
    out, seq_2d, cam = runs
    got = out["given"]
    assert set(got) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"}
    for k in ("pose", "count"):
        assert same_bits(got[k], out["estimate"][k]), k
    want = ops.fit_trajectory(got["pose"].to(DEV), seq_2d.to(DEV), cam.to(DEV))
    assert same_bits(got["traj_raw"], want["traj"].cpu()) and same_bits(got["traj_weight"], want["wsum"].cpu())
    assert same_bits(got["traj_resid"], want["resid"].cpu())
    assert same_bits(got["traj"], ops.smooth_trajectory(want["traj"], want["wsum"], 3).cpu())

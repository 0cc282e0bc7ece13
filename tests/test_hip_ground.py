"""The ground-plane estimate on the device: foot_contacts_kernel (pafuse_foot_contacts), ground_sums_kernel (pafuse_ground_sums),
ground_solve_kernel (pafuse_ground_solve), frames_to_world_kernel (pafuse_frames_to_world), ops.foot_contacts / ground_sums /
ground_solve / frames_to_world / estimate_ground, torch.ops.pafuse.*, harness.estimate_ground and infer_sequence(trajectory=...,
ground=...).

What is asserted and why it can be asserted:
  * every kernel vs the statement pafuse_amd/ground.py: both perform the same IEEE fp64 operations in the same order (contraction
    off, correctly rounded divides and square roots, the frames of the solve in the pinned lane order) -> the design goal is equal
    bits; the test accepts equal or ADJACENT values - the acceptance rule of tests/test_hip_rootfit.py - and prints how many
    differ.  Zero contacts, counts and codes are exact: torch.equal.
  * the solve is compared on the KERNEL'S OWN state, the world on the kernel's own plane: an adjacent value upstream would
    otherwise be conditioned through the Jacobi.
  * the chain on the planted walk of tests/test_ground_host.py: the bound fixed there from the statement (WALK_BOUND_DEG), the
    camera height within `floor`.
Shapes: J in {5, 134} x K in {1, 2, 6, 16} x N in {1, 2, 3, 9, 70} x r in {1, 3, 64}, T in {1, 2} for the contacts and the sums (N = 1, 2:
no line through three frames; r = 64 > N: every window clipped at both ends; N = 70 at K = 16: more than one workgroup);
N in {1, 2, 63, 64, 65, 130} for the solve: fewer frames than lanes, exactly one round, one frame in a second round, a ragged third.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_ground_host import CAM_HEIGHT, POINTS, SEEDS, WALK_BOUND_DEG, angle, standing, walk
from tests.test_hip_partials import dataset, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 5
E_ARG = -1
GRID = [(J, K, N) for J in (5, 134) for K in (1, 2, 6, 16) for N in (1, 2, 3, 9, 70)]
RADII = (1, 3, 64)
SOLVE_CASES = (1, 2, 63, 64, 65, 130)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def video(J, K, N, T, seed):
    """joints that drift at 0 .. 0.03 m/frame (on both sides of the default speed gate) with 1 mm of noise around a moving root; 5 %
    of the pose rows and of the roots NaN -> pose [T,N,J,3], traj [T,N,3] fp32, points [K] (repeats where K > J)"""
    g = np.random.default_rng(seed)
    n = np.arange(N, dtype=np.float64)[None, :, None, None]
    drift = g.uniform(0.0, 0.03, (T, 1, J, 1)) * g.standard_normal((T, 1, J, 3)) / np.sqrt(3)
    pose = g.standard_normal((T, 1, J, 3)) * 0.4 + drift * n + 1e-3 * g.standard_normal((T, N, J, 3))
    traj = np.array([0.2, 0.1, 4.5]) + 0.01 * n[:, :, 0] * np.array([1.0, 0.0, 0.3]) + 1e-3 * g.standard_normal((T, N, 3))
    pose, traj = pose.astype(np.float32), traj.astype(np.float32)
    pose[g.uniform(size=(T, N, J)) < 0.05, 1] = np.nan
    traj[g.uniform(size=(T, N)) < 0.05] = np.nan
    if N >= 3:
        traj[T - 1, N // 2] = np.nan                                           # at least one frame without a root
    return pose, traj, g.integers(0, J, K).astype(np.int32)


def given_plane(foot, T, seed):
    """a plane through the middle of the finite foot points of every step and a scale that leaves about half of them inside the
    gate: what a later pass reads"""
    g = np.random.default_rng(seed)
    plane, scale = np.zeros((T, 4)), np.zeros(T)
    for t in range(T):
        nrm = g.standard_normal(3)
        nrm /= np.linalg.norm(nrm)
        p = foot[t].reshape(-1, 3).astype(np.float64)
        p = p[np.isfinite(p).all(axis=-1)]
        h = p @ nrm if len(p) else np.zeros(1)
        plane[t] = (*nrm, np.median(h))
        scale[t] = max(float(np.abs(h - np.median(h)).mean()) / 2.5, 1e-3)
    return plane, scale


@pytest.mark.parametrize("case", GRID)
def test_contacts_and_sums_are_the_statement(case):
    from pafuse_amd import ground, ops
    J, K, N = case
    differ = {"foot": 0, "foot_speed": 0, "contact": 0, "state": 0, "state_later": 0}
    total = dict(differ)
    for r in RADII:
        for T in (1, 2):
            pose, traj, points = video(J, K, N, T, seed=1000 * J + 100 * K + 10 * N + r + T)
            got = ops.foot_contacts(dev(pose), dev(traj), points, radius=r, speed=0.015)
            foot, foot_speed, contact = ground.contacts(pose, traj, points, radius=r, speed=0.015)
            want = {"foot": foot, "foot_speed": foot_speed, "contact": contact}
            assert set(got) == set(want) and tuple(got["foot"].shape) == (T, N, K, 3)
            for k in want:
                differ[k] += equal_or_adjacent(got[k].cpu(), torch.from_numpy(want[k]))
                total[k] += want[k].size
            assert torch.equal(got["contact"].cpu() == 0, torch.from_numpy(contact) == 0)       # exactly 0 in the same places
            if N < 3:                                                                          # no line through three frames
                assert bool(torch.isnan(got["foot"]).all()) and bool(torch.isnan(got["foot_speed"]).all()) and not bool(got["contact"].any())
            lone = ops.foot_contacts(dev(pose), dev(traj), points, radius=r, speed=0.015, want_speed=False)
            assert set(lone) == {"foot", "contact"} and same_bits(lone["foot"], got["foot"]) and same_bits(lone["contact"], got["contact"])
            # the sums on the kernel's own foot points: the first pass, and a later one that reads a plane and a scale
            f, c = got["foot"].cpu().numpy(), got["contact"].cpu().numpy()
            plane, scale = given_plane(f, T, seed=N + K)
            for name, pl, sc in (("state", None, None), ("state_later", plane, scale)):
                state = ops.ground_sums(got["foot"], got["contact"], dev(traj), None if pl is None else dev(pl), None if sc is None else dev(sc),
                                        gate=2.5)
                ref = torch.from_numpy(ground.sums(f, c, traj, pl, sc, gate=2.5))
                assert tuple(state.shape) == (T, N, 14) and state.dtype == torch.float64
                differ[name] += equal_or_adjacent(state.cpu(), ref)
                total[name] += ref.numel()
                assert torch.equal(state.cpu()[..., 13], ref[..., 13])                        # the number of points: exact
                empty = ref[..., 13] == 0
                assert same_bits(state.cpu()[empty], torch.zeros_like(ref[empty]))            # every weight 0: exactly 14 zeros (+0.0)
                if N >= 3:
                    assert bool(empty.any())                                                   # the frame without a root is one of them
    print(f"(J, K, N) = {case}: values that differ from the statement (by one step) / compared: "
          + ", ".join(f"{k} {differ[k]}/{total[k]}" for k in differ))


def planted_feet(N, T, seed, K=6):
    """foot points on a tilted plane 5 m away, 1.2 m wide, with 3 mm of noise and random contact weights (a third of them 0); the last
    step's points within 2 mm of one spot (no plane, no line: the body's up); a root 0.9 m above"""
    g = np.random.default_rng(seed)
    nrm = np.array([0.05, -0.95, -0.3])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [1.0, 0, 0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    uv = g.uniform(-0.6, 0.6, (T, N, K, 2))
    uv[T - 1] *= 1e-3 / 0.6
    foot = np.array([0.1, 1.2, 5.0]) + uv[..., :1] * a + uv[..., 1:] * b + 3e-3 * g.standard_normal((T, N, K, 1)) * nrm
    traj = foot.mean(axis=2) + 0.9 * nrm + 0.02 * g.standard_normal((T, N, 3))
    contact = g.uniform(0.05, 1.0, (T, N, K))
    contact[g.uniform(size=contact.shape) < 0.33] = 0
    return foot.astype(np.float32), contact.astype(np.float32), traj.astype(np.float32)


def check_solve(got, want, T):
    """got: ops.ground_solve's dict (device), want: the statement's on the same state -> the number of values that differ by one step"""
    assert torch.equal(got["ground_code"].cpu(), torch.from_numpy(want["ground_code"])) and got["ground_code"].dtype == torch.uint8
    assert torch.equal(got["ground_points"].cpu(), torch.from_numpy(want["ground_points"])) and got["ground_points"].dtype == torch.int32
    assert tuple(got["plane"].shape) == (T, 4) and got["plane"].dtype == got["scale"].dtype == torch.float64
    return {k: equal_or_adjacent(got[k].cpu(), torch.from_numpy(want[k])) for k in ("plane", "scale", "up", "camera_height", "ground_rms", "ground_eig")}


@pytest.mark.parametrize("N", SOLVE_CASES)
def test_solve_is_the_statement_on_the_kernels_state(N):
    from pafuse_amd import ground, ops
    T = 2
    foot, contact, traj = planted_feet(N, T, seed=40 + N)
    state = ops.ground_sums(dev(foot), dev(contact), dev(traj))
    got = ops.ground_solve(state)
    want = ground.solve(state.cpu().numpy())
    differ = check_solve(got, want, T)
    print(f"N = {N}: codes {got['ground_code'].tolist()}, points {got['ground_points'].tolist()}, up {got['up'].tolist()}; values that "
          f"differ from the statement (by one step): {differ}")
    assert int(got["ground_points"][0]) == int((contact[0] > 0).sum())
    assert got["ground_code"].tolist() == ([1, 3] if N > 1 else [int(want["ground_code"][0]), 3])
    # a later pass on the plane the kernel wrote, read on the device
    later = ops.ground_sums(dev(foot), dev(contact), dev(traj), got["plane"], got["scale"])
    ref = ground.sums(foot, contact, traj, got["plane"].cpu().numpy(), got["scale"].cpu().numpy())
    equal_or_adjacent(later.cpu(), torch.from_numpy(ref))
    check_solve(ops.ground_solve(later), ground.solve(later.cpu().numpy()), T)
    # the states of two videos concatenate along N
    f2, c2, t2 = planted_feet(7, T, seed=5)
    s2 = ops.ground_sums(dev(f2), dev(c2), dev(t2))
    both = torch.cat([state, s2], dim=1).contiguous()
    joint = ops.ground_solve(both)
    check_solve(joint, ground.solve(both.cpu().numpy()), T)
    assert joint["ground_points"].tolist() == [int((contact[t] > 0).sum() + (c2[t] > 0).sum()) for t in range(T)]
    only = ops.ground_solve(state, want=("up", "ground_code"))
    assert set(only) == {"up", "ground_code"} and same_bits(only["up"], got["up"])


def four_codes(N=65):
    """one step per code, by construction: the planted walk (1 plane), a person standing (2 line), coincident feet (3 body), no root (0)"""
    w, s, c = walk(0, N=N), standing(0.0, N=N), standing(3.0, feet_apart=0.0, N=N)
    pose = np.concatenate([w[0], s[0], c[0], w[0]])
    traj = np.concatenate([w[1], s[1], c[1], np.full_like(w[1], np.nan)])
    return pose, traj, w[2]


def test_every_code_is_reached_and_the_chain_is_the_statement():
    from pafuse_amd import ground, ops
    pose, traj, up = four_codes()
    got = ops.estimate_ground(dev(pose), dev(traj), POINTS)
    assert set(got) == set(ops.GROUND_OUTPUTS)
    assert got["ground_code"].tolist() == [1, 2, 3, 0]
    want = ground.estimate(pose, traj, POINTS)
    assert torch.equal(got["ground_code"].cpu(), torch.from_numpy(want["ground_code"]))
    assert torch.equal(got["ground_points"].cpu(), torch.from_numpy(want["ground_points"]))
    differ = {k: equal_or_adjacent(got[k].cpu(), torch.from_numpy(want[k])) for k in ("foot", "foot_speed", "contact", "plane", "scale", "up",
                                                                                      "camera_height", "ground_rms", "ground_eig")}
    # the world on the kernel's own plane
    pw, tw = ground.to_world(pose, traj, got["plane"].cpu().numpy())
    differ["pose_world"] = equal_or_adjacent(got["pose_world"].cpu(), torch.from_numpy(pw))
    differ["traj_world"] = equal_or_adjacent(got["traj_world"].cpu(), torch.from_numpy(tw))
    print(f"codes {got['ground_code'].tolist()}, camera height {got['camera_height'].tolist()}; values that differ from the statement "
          f"(by one step): {differ}")
    assert bool(torch.isnan(got["pose_world"][3]).all()) and bool(torch.isnan(got["up"][3]).all()) and int(got["ground_points"][3]) == 0
    assert angle(got["up"][1].cpu().numpy(), up) <= 1e-3 and abs(angle(got["up"][2].cpu().numpy(), up) - 3.0) <= 1e-3


@pytest.mark.parametrize("seed", SEEDS)
def test_planted_walk_on_the_device(seed):
    """the bound of tests/test_ground_host.py::test_planted_walk_noise_free, fixed there from the statement"""
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import harness, ops
    pose, traj, up, stance = walk(seed)
    got = ops.estimate_ground(dev(pose), dev(traj), POINTS)
    a, h = angle(got["up"][0].cpu().numpy(), up), float(got["camera_height"][0])
    print(f"seed {seed}: code {int(got['ground_code'][0])}, angle {a:.5f} deg (bound {WALK_BOUND_DEG}), camera height {h:.5f} m, rms "
          f"{float(got['ground_rms'][0]) * 1e3:.3f} mm, points {int(got['ground_points'][0])}")
    assert int(got["ground_code"][0]) == 1 and a <= WALK_BOUND_DEG and abs(h - CAM_HEIGHT) <= 0.005
    feet = got["pose_world"][0][:, list(POINTS), 2].cpu().numpy()
    assert np.abs(feet[stance]).max() <= 0.005
    alone = harness.estimate_ground(pose, traj, POINTS)
    assert set(alone) == set(harness.GROUND_KEYS) and all(not v.is_cuda for v in alone.values())
    names = {"ground_plane": "plane"}
    assert all(same_bits(alone[k], got[names.get(k, k)].cpu()) for k in alone)
    op = torch.ops.pafuse.estimate_ground(dev(pose), dev(traj), list(POINTS))
    assert len(op) == len(ops.GROUND_OUTPUTS) and all(same_bits(v, got[k]) for k, v in zip(ops.GROUND_OUTPUTS, op))
    if seed == 0:                                                     # the ops one by one, through torch.ops
        foot, speed, contact = torch.ops.pafuse.foot_contacts(dev(pose), dev(traj), list(POINTS))
        assert same_bits(foot, got["foot"]) and same_bits(speed, got["foot_speed"]) and same_bits(contact, got["contact"])
        plane = scale = None
        for _ in range(3):
            sol = torch.ops.pafuse.ground_solve(torch.ops.pafuse.ground_sums(foot, contact, dev(traj), plane, scale))
            plane, scale = sol[0], sol[1]
        assert all(same_bits(v, got[k]) for k, v in zip(ops.GROUND_SOLVE_OUTPUTS, sol))
        pw, tw = torch.ops.pafuse.frames_to_world(dev(pose), dev(traj), plane)
        assert same_bits(pw, got["pose_world"]) and same_bits(tw, got["traj_world"])
        one = ops.estimate_ground(dev(pose), dev(traj), POINTS, passes=1, want=("up", "ground_points"))
        assert set(one) == {"up", "ground_points"} and int(one["ground_points"][0]) >= int(got["ground_points"][0])


def raw(name, *args):
    from pafuse_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 6, 9, 2), (5, 16, 70, 1), (5, 1, 1, 1)])
def test_guard_rows_behind_every_output_keep_their_bits(case):
    from pafuse_amd import ops
    J, K, N, T = case
    pose, traj, points = video(J, K, N, T, seed=77)
    pose, traj, pts = dev(pose), dev(traj), dev(points)
    want = ops.estimate_ground(pose, traj, points, passes=1)
    full = lambda n, dt=torch.float32: torch.full((n + PAD,), 7, device=DEV, dtype=dt)
    foot, speed, contact = full(T * N * K * 3), full(T * N * K), full(T * N * K)
    assert raw("pafuse_foot_contacts", pose, traj, pts, T, N, J, K, 3, 0.015, foot, speed, contact) == 0
    for buf, k in ((foot, "foot"), (speed, "foot_speed"), (contact, "contact")):
        n = want[k].numel()
        assert bool((buf[n:] == 7).all()) and same_bits(buf[:n], want[k].reshape(-1)), k
    lone = full(T * N * K * 3)
    assert raw("pafuse_foot_contacts", pose, traj, pts, T, N, J, K, 3, 0.015, lone, None, contact) == 0      # foot_speed may be NULL
    assert bool((lone[T * N * K * 3:] == 7).all()) and same_bits(lone[:T * N * K * 3], want["foot"].reshape(-1))
    state = full(T * N * 14, torch.float64)
    assert raw("pafuse_ground_sums", want["foot"], want["contact"], traj, None, None, T, N, K, 2.5, state) == 0
    assert bool((state[T * N * 14:] == 7).all())
    assert same_bits(state[:T * N * 14], ops.ground_sums(want["foot"], want["contact"], traj).reshape(-1))
    sizes = (("plane", T * 4, torch.float64), ("scale", T, torch.float64), ("up", T * 3, torch.float32), ("camera_height", T, torch.float32),
             ("ground_rms", T, torch.float32), ("ground_eig", T * 3, torch.float32), ("ground_points", T, torch.int32), ("ground_code", T, torch.uint8))
    bufs = {k: full(n, dt) for k, n, dt in sizes}
    st = state[:T * N * 14].clone()
    assert raw("pafuse_ground_solve", st, T, N, 0.005, 0.03, *[bufs[k] for k, _, _ in sizes]) == 0
    for k, n, _ in sizes:
        assert bool((bufs[k][n:] == 7).all()), k
        assert same_bits(bufs[k][:n], want[k].reshape(-1)), k
    pl, sc = full(T * 4, torch.float64), full(T, torch.float64)
    assert raw("pafuse_ground_solve", st, T, N, 0.005, 0.03, pl, sc, None, None, None, None, None, None) == 0  # the optional outputs may be NULL
    assert bool((pl[T * 4:] == 7).all()) and bool((sc[T:] == 7).all()) and same_bits(pl[:T * 4], want["plane"].reshape(-1))
    pw, tw = full(T * N * J * 3), full(T * N * 3)
    assert raw("pafuse_frames_to_world", pose, traj, want["plane"], T, N, J, pw, tw) == 0
    assert bool((pw[T * N * J * 3:] == 7).all()) and bool((tw[T * N * 3:] == 7).all())
    assert same_bits(pw[:T * N * J * 3], want["pose_world"].reshape(-1)) and same_bits(tw[:T * N * 3], want["traj_world"].reshape(-1))
    pw2 = full(T * N * J * 3)
    assert raw("pafuse_frames_to_world", pose, traj, want["plane"], T, N, J, pw2, None) == 0                  # traj_world may be NULL
    assert same_bits(pw2, pw)


def test_refusals_come_before_any_launch():
    from pafuse_amd import _lib, ops
    lib = _lib.load()
    pose, traj, points = video(5, 2, 4, 1, seed=1)
    pose, traj, pts = dev(pose), dev(traj), dev(points)
    p = lambda t: t.data_ptr()
    outs = [torch.full((64,), 7.0, device=DEV) for _ in range(3)]
    ok = [p(pose), p(traj), p(pts), 1, 4, 5, 2, 3, 0.015, p(outs[0]), p(outs[1]), p(outs[2]), None]
    for i, v in ((0, None), (2, None), (9, None), (11, None), (4, 0), (6, 17), (7, 65), (8, 0.0), (8, float("nan"))):
        a = list(ok)
        a[i] = v
        assert lib.pafuse_foot_contacts(*a) == E_ARG, (i, v)
    with pytest.raises(ValueError, match="ground: "):
        ops.foot_contacts(pose, traj, [5])
    with pytest.raises(ValueError, match="speed"):
        ops.foot_contacts(pose, traj, [1, 2], speed=-1.0)
    with pytest.raises(ValueError, match="radius"):
        ops.foot_contacts(pose, traj, [1, 2], radius=0)
    with pytest.raises(ValueError, match="plane"):
        ops.frames_to_world(pose, traj, torch.zeros(1, 4, device=DEV))
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in outs)                  # nothing was launched on them


# --------------------------------------------------------------------------------------------------------- infer_sequence
SEED = 4321
F27 = 27
N_VIDEO = 2 * F27 + 1


@pytest.fixture(scope="module")
def runs():
    """infer_sequence(stride = F - 1, aggregate = "mean", trajectory = 3) on the seeded video with ground = True and with ground = None,
    from the same start of the noise stream; computed once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, _, cam = sequence(N_VIDEO)
    out = {}
    for name, kw in (("ground", dict(ground=True)), ("none", dict(ground=None)), ("plain", dict())):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        out[name] = harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2,
                                           aggregate="mean", stride=F27 - 1, trajectory=3, cam=cam, **kw)
    return out


def test_infer_sequence_adds_the_ground_of_the_pose_it_returns(runs):
    from pafuse_amd import h3wb, harness, ops
    got = runs["ground"]
    assert set(got) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"} | set(harness.GROUND_KEYS)
    assert all(not v.is_cuda for v in got.values())
    T = got["pose"].shape[0]
    assert T == 2 and tuple(got["up"].shape) == (T, 3) and tuple(got["pose_world"].shape) == tuple(got["pose"].shape)
    assert tuple(got["foot"].shape) == (T, N_VIDEO, 6, 3) and got["ground_code"].dtype == torch.uint8
    print(f"code {got['ground_code'].tolist()}, up {got['up'].tolist()}, camera height {got['camera_height'].tolist()}, points "
          f"{got['ground_points'].tolist()} (synthetic weights: the numbers mean nothing)")
    want = ops.estimate_ground(got["pose"].to(DEV), got["traj"].to(DEV), h3wb.foot_points(True))
    names = {"ground_plane": "plane"}
    for k in harness.GROUND_KEYS:
        assert same_bits(got[k], want[names.get(k, k)].cpu()), k
    alone = harness.estimate_ground(got["pose"], got["traj"])          # the same keys from the arrays a caller has
    assert set(alone) == set(harness.GROUND_KEYS) and all(same_bits(alone[k], got[k]) for k in alone)


def test_infer_sequence_without_ground_is_unchanged(runs):
    for name in ("none", "plain"):
        got = runs[name]
        assert set(got) == {"pose", "count", "traj", "traj_raw", "traj_weight", "traj_resid"}
        for k in got:                                                 # key for key the output without the feature, and the shared keys with it
            assert same_bits(got[k], runs["plain"][k]), (name, k)
            assert same_bits(got[k], runs["ground"][k]), (name, k)

"""Host side of the ground-plane estimate (no GPU): the numpy statement pafuse_amd/ground.py - foot contacts from the local line's
slope, fourteen sums per (t, frame), a cyclic Jacobi on a 3x3, the plane or its degenerate stand-ins, the world axes - and the
refusals of pafuse_foot_contacts / pafuse_ground_sums / pafuse_ground_solve / pafuse_frames_to_world, which happen before the
first HIP call.

What is asserted and why it can be asserted:
  * the Jacobi against np.linalg.eigh: both are backward-stable fp64 decompositions of one symmetric matrix -> eigenvalues within
    1e-12 of the largest; an eigenvector is determined to about eps / gap, so where the gap to both neighbours is at least 1e-3 of
    the largest eigenvalue it agrees up to sign within 1e-10.
  * the slope member: on exact data y = a + b*m a weighted line fit returns b whatever the weights -> 1e-12 relative, and
    np.polyfit with w = sqrt(taper) is the same least-squares problem.
  * the planted walk (200 frames, camera tilted 18 degrees and rolled 3, stance 24 of a 40-frame cycle, feet 0.2 m apart, the body
    at 0.02 m/frame, the swing at constant velocity with a 0.1 m lift, the video beginning and ending in double support, radius 3,
    speed 0.015 m/frame; a seed draws the heading, the start and the phase): see test_planted_walk_noise_free for the bound and
    how it was fixed.  The camera height: within `floor` (5 mm), the resolution the estimator itself claims.
  * codes 2 and 3: the normal is built from the body's own up, root - feet, so its angle to the planted up is bounded by the planted
    lean; the inputs are fp32 (2^-23 * 6 m = 7e-7 m per coordinate, over the 0.2 m between the feet: 2e-4 degrees) -> 1e-3 degrees
    on top.
  * the sign: a camera with y up and z backward (the other common convention: a half turn about x, a proper rotation) sees the
    same world - up turns with the camera and pose_world keeps its values to fp32 rounding (4.8e-7 m at 5 m -> 1e-6 m).  A
    MIRRORED y alone is no rotation: up_y flips, every height stays, and the world comes out mirrored in y, as it must.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLE, STANCE, STEP, SIDE, LIFT, HIP = 40, 24, 0.02, 0.1, 0.1, 0.9
CAM_HEIGHT, TILT, ROLL = 1.5, 18.0, 3.0
POINTS = (1, 2)                      # the two feet of the five-joint figure below
WALK_BOUND_DEG = 0.0069              # 3 x the worst of seeds 0 .. 5 (0.00229 degrees): test_planted_walk_noise_free
SEEDS = tuple(range(6))


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def camera(tilt=TILT, roll=ROLL):
    """world (z up) -> camera (x right, y down, z forward): looking along world +y, tilted down by `tilt`, rolled by `roll` degrees"""
    a, b = np.deg2rad(tilt), np.deg2rad(roll)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return Rz @ Rx @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])


def to_camera(J, R):
    """world joints [N,5,3] (joint 0 the root) -> (pose [1,N,5,3] root-relative, traj [1,N,3]) fp32 as a camera at CAM_HEIGHT sees them"""
    Jc = (J - np.array([0.0, 0.0, CAM_HEIGHT])) @ R.T
    return (Jc - Jc[:, :1]).astype(np.float32)[None], Jc[:, 0].astype(np.float32)[None]


def walk(seed, N=200, noise=0.0, R=None):
    """the planted walk -> pose [1,N,5,3], traj [1,N,3] fp32, up [3] (the planted up in camera space), stance [N,2] bool"""
    g = np.random.default_rng(seed)
    R = camera() if R is None else R
    head = np.deg2rad(g.uniform(-30, 30))
    h, s = np.array([np.cos(head), np.sin(head), 0.0]), np.array([-np.sin(head), np.cos(head), 0.0])
    start = np.array([-2.0 + g.uniform(-0.3, 0.3), 5.0 + g.uniform(-0.5, 0.5), 0.0])
    phase0 = int(g.choice([1, 2, 3, 21, 22, 23]))                       # both feet down in the first and in the last frame
    n = np.arange(N)
    stride = STEP * CYCLE
    feet, stance = [], []
    for k, off in enumerate((0, CYCLE // 2)):
        ph = (n + phase0 + off) % CYCLE
        cyc = (n + phase0 + off) // CYCLE
        sw = np.clip((ph - STANCE + 0.5) / (CYCLE - STANCE), 0.0, 1.0)  # 0 in stance, 1/32 .. 31/32 through the 16 swing frames
        along = stride * (cyc + sw) - STEP * (phase0 + off) + stride / 2
        lift = LIFT * np.sin(np.pi * sw)
        feet.append(start + along[:, None] * h + (SIDE if k == 0 else -SIDE) * s + lift[:, None] * np.array([0, 0, 1.0]))
        stance.append(ph < STANCE)
    root = start + (STEP * n)[:, None] * h + np.array([0, 0, HIP])
    J = np.stack([root, feet[0], feet[1], root + np.array([0, 0, 0.7]), root + 0.3 * s], axis=1)        # [N,5,3] world
    J = J + noise * g.standard_normal(J.shape) * (np.arange(5) != 0)[None, :, None]
    pose, traj = to_camera(J, R)
    return pose, traj, R @ np.array([0, 0, 1.0]), np.stack(stance, axis=1)


def standing(lean_deg=0.0, feet_apart=2 * SIDE, N=50, R=None, lean_along=False):
    """a person standing still: the feet two fixed spots `feet_apart` apart (0: coincident), the root HIP above their midpoint,
    displaced by tan(lean)*HIP across the line of the feet (lean_along: along it) -> pose, traj, up"""
    R = camera() if R is None else R
    mid = np.array([0.3, 5.0, 0.0])
    s, across = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    root = mid + np.array([0, 0, HIP]) + np.tan(np.deg2rad(lean_deg)) * HIP * (s if lean_along else across)
    one = np.stack([root, mid + feet_apart / 2 * s, mid - feet_apart / 2 * s, root + np.array([0, 0, 0.7]), root + 0.3 * s])
    pose, traj = to_camera(np.repeat(one[None], N, axis=0), R)
    return pose, traj, R @ np.array([0, 0, 1.0])


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.rad2deg(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))))


def kept_weights(out, traj):
    """the weight of every point under the plane that is returned: what one more pass would sum"""
    from pafuse_amd import ground
    return ground.weights(out["foot"], out["contact"], traj, out["plane"], out["scale"])[0]


# --------------------------------------------------------------------------------------------------------------- the Jacobi
def sym(A):
    from pafuse_amd import ground
    return [A[..., a, b] for a, b in ground.SYM]


def jacobi_cases():
    g = np.random.default_rng(0)
    A = g.standard_normal((200, 3, 3))
    A = A + A.transpose(0, 2, 1)
    Q = np.linalg.qr(g.standard_normal((50, 3, 3)))[0]
    twice = Q @ np.diag([1.0, 1.0, 3.0]) @ Q.transpose(0, 2, 1)                 # equal eigenvalues, rotated
    v = g.standard_normal((50, 3))
    rank1 = v[:, :, None] * v[:, None, :]
    diag = np.stack([np.diag(d) for d in ([3.0, 1.0, 2.0], [2.0, 2.0, 5.0], [5.0, 2.0, 2.0], [0.0, 0.0, 0.0], [1e-6, 1e-2, 1.3])])
    cov = np.stack([np.cov(g.standard_normal((3, 40)) * np.array([[1e-3], [0.1], [1.0]])) for _ in range(50)])   # what the solve sees
    return np.concatenate([A, twice, rank1, diag, cov])


def test_jacobi_is_an_eigen_decomposition():
    from pafuse_amd import ground
    A = jacobi_cases()
    lam, vec = ground.jacobi_eigen(sym(A))
    lam = np.stack(lam, axis=-1)
    V = np.stack([np.stack(vec[k], axis=-1) for k in range(3)], axis=-1)         # [n, component, k]
    w, v = np.linalg.eigh(A)
    top = np.abs(w).max(axis=-1, keepdims=True)
    top[top == 0] = 1.0
    err = np.abs(lam - w) / top
    print(f"eigenvalues: worst |jacobi - eigh| / largest = {err.max():.3g} over {len(A)} matrices")
    assert err.max() <= 1e-12 and (np.diff(lam, axis=-1) >= 0).all()
    gap = np.full(w.shape, np.inf)
    gap[:, :-1] = np.minimum(gap[:, :-1], np.diff(w, axis=-1))
    gap[:, 1:] = np.minimum(gap[:, 1:], np.diff(w, axis=-1))
    clear = gap >= 1e-3 * top
    dots = np.abs(np.einsum("nik,nik->nk", V, v))
    print(f"eigenvectors: worst 1 - |v.v_eigh| where the gap allows = {(1 - dots[clear]).max():.3g} ({clear.sum()} of {clear.size})")
    assert (1 - dots[clear]).max() <= 1e-10
    assert np.abs(np.einsum("nik,nil->nkl", V, V) - np.eye(3)).max() <= 1e-14   # orthonormal, equal eigenvalues or not
    resid = np.abs(np.einsum("nij,njk->nik", A, V) - V * lam[:, None, :]).max(axis=(1, 2)) / top[:, 0]
    assert resid.max() <= 1e-12                                                  # A v = lambda v, for the repeated ones too


def test_jacobi_pinned_details():
    from pafuse_amd import ground
    one = lambda M: ground.jacobi_eigen(sym(np.asarray(M, dtype=np.float64)[None]))
    lam, vec = one(np.diag([5.0, 2.0, 2.0]))                                      # the tie rule: equal eigenvalues keep their order
    assert [float(v[0]) for v in lam] == [2.0, 2.0, 5.0]
    assert [[float(c[0]) for c in v] for v in vec] == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]
    lam, vec = one(np.diag([3.0, 1.0, 2.0]))                                      # exactly zero off-diagonals: every rotation skipped
    assert [float(v[0]) for v in lam] == [1.0, 2.0, 3.0] and [float(c[0]) for c in vec[0]] == [0, 1, 0]
    M = np.diag([1.0, 2.0, 3.0])
    M[0, 1] = M[1, 0] = 1e-200                                                   # theta*theta overflows: t = 0, the diagonal keeps its bits
    lam, vec = one(M)
    assert [float(v[0]) for v in lam] == [1.0, 2.0, 3.0] and all(np.isfinite(c).all() for v in vec for c in v)
    M[0, 1] = M[1, 0] = 5e-324                                                   # theta itself is infinite
    lam, vec = one(M)
    assert [float(v[0]) for v in lam] == [1.0, 2.0, 3.0] and all(np.isfinite(c).all() for v in vec for c in v)
    lam, vec = one(np.full((3, 3), np.nan))                                      # NaN spreads, nothing raises
    assert all(np.isnan(v).all() for v in lam)


def test_slope_is_the_weighted_line_fit():
    from pafuse_amd import trajectory
    N, r = 23, 4
    m = np.arange(N, dtype=np.float64)
    a, b = np.array([0.3, -1.2, 4.0]), np.array([0.0125, -0.004, 0.03])
    y = a + b * m[:, None]                                                       # exact data
    part = np.ones(N, dtype=bool)
    part[[5, 6, 17]] = False
    value, slope, code, cnt = trajectory.local_line_slope(y, part, np.ones(N), r)
    assert (code == trajectory.LINE).all()
    assert np.abs(slope / b - 1).max() <= 1e-12 and np.abs(value - y).max() <= 1e-12
    v2, c2 = trajectory.local_line(y, part, np.ones(N), r)                       # the existing members keep their bits
    assert np.array_equal(v2, value) and np.array_equal(c2, code)
    rng = np.random.default_rng(3)
    yn = y + 0.01 * rng.standard_normal(y.shape)
    value, slope, code, cnt = trajectory.local_line_slope(yn, part, np.ones(N), r)
    for n in (0, 7, 12, N - 1):
        ms = np.array([k for k in range(max(0, n - r), min(N - 1, n + r) + 1) if part[k]])
        d = (ms - n).astype(np.float64)
        g = (1.0 - d * d / (r + 1) ** 2) ** 2
        assert cnt[n] == len(ms)
        for k in range(3):
            fit = np.polyfit(d, yn[ms, k], 1, w=np.sqrt(g))
            assert abs(slope[n, k] - fit[0]) <= 1e-12 and abs(value[n, k] - fit[1]) <= 1e-12


# --------------------------------------------------------------------------------------------------------- the planted walk
@pytest.fixture(scope="module")
def walks():
    """the statement on the planted walk, seeds 0 .. 5, noise-free and with 5 mm of noise; computed once and never modified"""
    from pafuse_amd import ground
    out = {}
    for noise in (0.0, 0.005):
        for seed in SEEDS:
            pose, traj, up, stance = walk(seed, noise=noise)
            out[noise, seed] = (pose, traj, up, stance, ground.estimate(pose, traj, POINTS))
    return out


def test_planted_walk_noise_free(walks):
    """MEASURED FROM THE STATEMENT FIRST, then fixed: on seeds 0 .. 5 the angle between the estimated and the planted up is at worst
    0.00229 degrees (seeds 0, 2 .. 5 alike; seed 1: below 1e-5); WALK_BOUND_DEG = 0.0069 = 3 x that.  The
    residue comes from the stance frames next to a swing, whose local line leans into the first lifted frames (a few tenths of a
    millimetre; ground_rms 0.5 mm).  The camera height comes back within 0.3 mm of 1.5 m; the bound is `floor`, 5 mm."""
    worst = 0.0
    for seed in SEEDS:
        pose, traj, up, stance, out = walks[0.0, seed]
        a, h = angle(out["up"][0], up), float(out["camera_height"][0])
        kept = kept_weights(out, traj) > 0
        print(f"seed {seed}: angle {a:.5f} deg, camera height {h:.5f} m, rms {float(out['ground_rms'][0]) * 1e3:.3f} mm, eig "
              f"{out['ground_eig'][0].tolist()}, points {int(out['ground_points'][0])}, kept {int(kept.sum())} of which not in stance "
              f"{int((kept & ~stance).sum())}")
        worst = max(worst, a)
        assert int(out["ground_code"][0]) == 1
        assert kept.sum() >= 100 and not (kept & ~stance).any()                   # every point the re-weighting keeps is a stance point
        assert a <= WALK_BOUND_DEG
        assert abs(h - CAM_HEIGHT) <= 0.005
        assert abs(float(np.linalg.norm(out["up"][0].astype(np.float64))) - 1) <= 1e-6
        feet_height = out["pose_world"][0][:, list(POINTS), 2]
        assert np.abs(feet_height[stance]).max() <= 0.005                         # the resting feet are on the ground, in world space
        assert abs(float(np.median(out["traj_world"][0, :, 2])) - HIP) <= 0.005
    print(f"worst angle over seeds 0 .. 5: {worst:.5f} deg (bound {WALK_BOUND_DEG})")


def test_planted_walk_with_5mm_noise(walks):
    """reported, and asserted only to stay below the noise-free bound + 2 degrees; seen: 0.01 .. 0.25 degrees"""
    for seed in SEEDS:
        pose, traj, up, stance, out = walks[0.005, seed]
        a = angle(out["up"][0], up)
        print(f"seed {seed}, 5 mm noise: angle {a:.4f} deg, camera height {float(out['camera_height'][0]):.4f} m, rms "
              f"{float(out['ground_rms'][0]) * 1e3:.2f} mm, code {int(out['ground_code'][0])}")
        assert int(out["ground_code"][0]) == 1 and a <= WALK_BOUND_DEG + 2.0


# --------------------------------------------------------------------------------------------------- the degenerate cases
@pytest.mark.parametrize("lean", [0.0, 4.0])
def test_standing_still_is_a_line(lean):
    from pafuse_amd import ground
    pose, traj, up = standing(lean)
    out = ground.estimate(pose, traj, POINTS)
    a = angle(out["up"][0], up)
    print(f"standing, lean {lean}: code {int(out['ground_code'][0])}, angle {a:.6f} deg, eig {out['ground_eig'][0].tolist()}")
    assert int(out["ground_code"][0]) == 2 and int(out["ground_points"][0]) == 2 * pose.shape[1]
    assert a <= lean + 1e-3
    # the leaning plane passes through the feet, 5.01 m from the point below the camera: that far it carries its tilt
    assert abs(float(out["camera_height"][0]) - CAM_HEIGHT) <= 0.005 + 5.01 * np.tan(np.deg2rad(lean))
    along = ground.estimate(*standing(lean, lean_along=True)[:2], POINTS)        # a lean along the line of the feet is projected out
    assert int(along["ground_code"][0]) == 2 and angle(along["up"][0], up) <= 1e-3


@pytest.mark.parametrize("lean", [0.0, 4.0])
def test_coincident_feet_fall_back_to_the_bodys_up(lean):
    from pafuse_amd import ground
    pose, traj, up = standing(lean, feet_apart=0.0)
    out = ground.estimate(pose, traj, POINTS)
    a = angle(out["up"][0], up)
    print(f"coincident feet, lean {lean}: code {int(out['ground_code'][0])}, angle {a:.6f} deg")
    assert int(out["ground_code"][0]) == 3 and a <= lean + 1e-3 and a >= lean - 1e-3


def test_no_finite_trajectory_is_code_0_and_all_nan():
    from pafuse_amd import ground
    pose, traj, up, _ = walk(0, N=40)
    out = ground.estimate(pose, np.full_like(traj, np.nan), POINTS)
    assert int(out["ground_code"][0]) == 0 and int(out["ground_points"][0]) == 0
    for k in ("plane", "scale", "up", "camera_height", "ground_rms", "ground_eig", "foot", "foot_speed", "pose_world", "traj_world"):
        assert np.isnan(out[k]).all(), k
    assert (out["contact"] == 0).all()
    short = ground.estimate(pose[:, :2], traj[:, :2], POINTS)                    # two frames: no line through three
    assert int(short["ground_code"][0]) == 0 and np.isnan(short["foot"]).all() and (short["contact"] == 0).all()
    state = ground.sums(out["foot"], out["contact"], traj)
    assert not state.any()                                                       # every weight 0: exactly 14 zeros per frame


def test_the_sign_follows_the_body_not_the_cameras_y_axis():
    from pafuse_amd import ground
    pose, traj, up, _ = walk(3, N=120)
    base = ground.estimate(pose, traj, POINTS)
    turn = np.array([1.0, -1.0, -1.0], dtype=np.float32)                         # y up, z backward: a half turn about x
    other = ground.estimate(pose * turn, traj * turn, POINTS)
    assert int(other["ground_code"][0]) == 1
    assert np.abs(other["up"][0] - base["up"][0] * turn).max() <= 1e-6 and base["up"][0][1] * other["up"][0][1] < 0
    assert abs(float(other["camera_height"][0] - base["camera_height"][0])) <= 1e-6
    assert np.abs(other["pose_world"] - base["pose_world"]).max() <= 1e-6
    assert np.abs(other["traj_world"] - base["traj_world"]).max() <= 1e-6
    mirror = np.array([1.0, -1.0, 1.0], dtype=np.float32)                        # y mirrored alone: not a rotation
    m = ground.estimate(pose * mirror, traj * mirror, POINTS)
    assert np.abs(m["up"][0] - base["up"][0] * mirror).max() <= 1e-6
    assert np.abs(m["pose_world"] - base["pose_world"] * mirror).max() <= 1e-6   # x and the heights stay, the world's y is mirrored
    assert float((base["pose_world"][0, :, 0, 2]).min()) > 0.8                   # the root is above the ground either way


def quaternion(Rm):
    """rotation matrix -> unit quaternion (w, x, y, z), fp64"""
    w = np.sqrt(max(0.0, 1 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + Rm[0, 0] - Rm[1, 1] - Rm[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - Rm[0, 0] + Rm[1, 1] - Rm[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - Rm[0, 0] - Rm[1, 1] + Rm[2, 2])) / 2
    q = np.array([w, np.copysign(x, Rm[2, 1] - Rm[1, 2]), np.copysign(y, Rm[0, 2] - Rm[2, 0]), np.copysign(z, Rm[1, 0] - Rm[0, 1])])
    return q / np.linalg.norm(q)


def test_to_world_is_camera_to_world_with_the_equivalent_quaternion():
    from pafuse_amd import ground, harness
    rng = np.random.default_rng(5)
    normals = [camera() @ np.array([0, 0, 1.0]), [0.995, 0.05, -0.0866], [-0.999, 0.03, 0.0], [0.0, -1.0, 0.0], [0.3, -0.5, 0.81]]
    T, N, J = len(normals), 7, 5
    plane = np.array([np.append(np.asarray(n) / np.linalg.norm(n), d) for n, d in zip(normals, (-1.5, 0.7, -2.0, -1.2, 0.0))])
    pose = (rng.standard_normal((T, N, J, 3)) * 0.4).astype(np.float32)
    traj = (rng.standard_normal((T, N, 3)) + np.array([0, 0, 5.0])).astype(np.float32)
    pose[1, 2, 3, 0] = np.nan
    traj[2, 4] = np.nan
    pw, tw = ground.to_world(pose, traj, plane)
    assert pw.dtype == tw.dtype == np.float32
    x, y, z = ground.world_axes(plane)
    for t in range(T):
        Rm = np.array([[x[a][t] for a in range(3)], [y[a][t] for a in range(3)], [z[a][t] for a in range(3)]])
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rm) - 1) <= 1e-14          # a proper rotation
        e = np.array([0.0, 0.0, 1.0]) if abs(plane[t, 0]) > 0.99 else np.array([1.0, 0.0, 0.0])
        assert abs(Rm[0] @ np.cross(plane[t, :3], e)) <= 1e-15 and Rm[0] @ e > 0                             # x: the camera's right, levelled
        shift = torch.tensor([0.0, 0.0, -plane[t, 3]], dtype=torch.float64)
        cam = torch.from_numpy(pose[t].astype(np.float64) + traj[t].astype(np.float64)[:, None])
        want = harness.camera_to_world(cam, quaternion(Rm), shift).numpy()
        assert np.array_equal(np.isnan(want), np.isnan(pw[t]))
        ok = ~np.isnan(want)
        assert (np.abs(pw[t][ok] - want[ok]) <= 2.0 ** -23 * np.abs(want[ok]) + 1e-9).all()               # one fp32 rounding
        wroot = harness.camera_to_world(torch.from_numpy(traj[t].astype(np.float64)), quaternion(Rm), shift).numpy()
        ok = ~np.isnan(wroot)
        assert np.array_equal(np.isnan(wroot), np.isnan(tw[t])) and (np.abs(tw[t][ok] - wroot[ok]) <= 2.0 ** -23 * np.abs(wroot[ok]) + 1e-9).all()
    nowhere = ground.to_world(pose, traj, np.full((T, 4), np.nan))
    assert np.isnan(nowhere[0]).all() and np.isnan(nowhere[1]).all()              # code 0 gives NaN


def test_states_of_two_videos_concatenate():
    from pafuse_amd import ground
    a, b = walk(0, N=90), walk(0, N=200)
    fa, fb = ground.contacts(a[0], a[1], POINTS), ground.contacts(b[0][:, 110:], b[1][:, 110:], POINTS)
    sa, sb = ground.sums(fa[0], fa[2], a[1]), ground.sums(fb[0], fb[2], b[1][:, 110:])
    both = ground.solve(np.concatenate([sa, sb], axis=1))
    assert int(both["ground_points"][0]) == int(ground.solve(sa)["ground_points"][0]) + int(ground.solve(sb)["ground_points"][0])
    assert int(both["ground_code"][0]) == 1 and angle(both["up"][0], a[2]) <= WALK_BOUND_DEG


# ------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    from pafuse_amd import _lib
    assert L.pafuse_abi_version() == 8 and _lib.ABI_VERSION == 8        # new entries only: no struct changed
    with open(os.path.join(ROOT, "include", "pafuse_hip.h")) as f:
        header = f.read()
    names = ("pafuse_foot_contacts", "pafuse_ground_sums", "pafuse_ground_solve", "pafuse_frames_to_world")
    assert all(f"int {n}(" in header and n in _lib.SIGNATURES for n in names) and "#define PAFUSE_ABI_VERSION 8" in header
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    inf, nan = float("inf"), float("nan")
    ok = [p, p, p, 1, 3, 5, 2, 3, 0.015, p, p, p, None]     # pose, traj, points, T, N, J, K, radius, speed, foot, foot_speed, contact
    bad = [(0, None), (1, None), (2, None), (9, None), (11, None), (3, 0), (4, 0), (5, 0), (3, -1), (6, 0), (6, 17), (7, 0), (7, 65),
           (8, 0.0), (8, -1.0), (8, inf), (8, nan)]
    for i, v in bad:
        a = list(ok)
        a[i] = v
        assert L.pafuse_foot_contacts(*a) == E_ARG, (i, v)
    assert b"foot_contacts" in L.pafuse_last_error()
    ok = [p, p, p, p, p, 1, 3, 2, 2.5, p, None]             # foot, contact, traj, plane, scale, T, N, K, gate, state
    bad = [(0, None), (1, None), (2, None), (9, None), (3, None), (4, None), (5, 0), (6, 0), (7, 0), (7, 17), (8, 0.0), (8, nan), (8, inf),
           (9, p + 4), (3, p + 4), (4, p + 4)]
    for i, v in bad:
        a = list(ok)
        a[i] = v
        assert L.pafuse_ground_sums(*a) == E_ARG, (i, v)
    assert b"ground_sums" in L.pafuse_last_error()
    ok = [p, 1, 3, 0.005, 0.03, p, p, p, p, p, p, p, p, None]   # state, T, N, floor, spread, plane, scale, up, height, rms, eig, points, code
    bad = [(0, None), (5, None), (6, None), (1, 0), (2, 0), (2, -1), (3, 0.0), (3, nan), (4, -0.03), (4, inf), (0, p + 4), (5, p + 4), (6, p + 4)]
    for i, v in bad:
        a = list(ok)
        a[i] = v
        assert L.pafuse_ground_solve(*a) == E_ARG, (i, v)
    assert b"ground_solve" in L.pafuse_last_error()
    ok = [p, p, p, 1, 3, 5, p, p, None]                     # pose, traj, plane, T, N, J, pose_world, traj_world
    for i, v in ((0, None), (1, None), (2, None), (6, None), (3, 0), (4, 0), (5, 0), (2, p + 4)):
        a = list(ok)
        a[i] = v
        assert L.pafuse_frames_to_world(*a) == E_ARG, (i, v)
    assert b"frames_to_world" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import ground, h3wb, harness, ops
    z = torch.zeros
    assert h3wb.foot_points().tolist() == [18, 19, 20, 21, 22, 23] and h3wb.foot_points(False).tolist() == [17, 18, 19, 20, 21, 22]
    assert h3wb.foot_points(True).dtype == np.int32
    parent = h3wb.bone_tables(68, True)[0]
    assert [int(parent[j]) for j in h3wb.foot_points()] == [16, 16, 16, 17, 17, 17]       # the toe and heel points hang on the ankles
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.foot_contacts(z(1, 4, 5, 3), z(1, 4, 3), [1, 2])
    with pytest.raises(ValueError, match=r"traj must be \[T,N,3\]"):
        ops.foot_contacts(z(1, 4, 5, 3), z(1, 3, 3), [1, 2])
    for points in ([], list(range(17)), [5], [-1], [1.5]):
        with pytest.raises(ValueError, match="ground: "):
            ops.ground_points(points, 5)
    with pytest.raises(ValueError, match="plane and scale come together"):
        ops.ground_sums(z(1, 4, 2, 3), z(1, 4, 2), z(1, 4, 3), plane=z(1, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="must match"):
        ops.ground_sums(z(1, 4, 2, 3), z(1, 4, 3), z(1, 4, 3))
    with pytest.raises(ValueError, match="HIP device"):
        ops.ground_solve(z(1, 4, 14, dtype=torch.float64))
    with pytest.raises(ValueError, match="want"):
        ops.ground_solve(z(1, 4, 14, dtype=torch.float64), want=("height",))
    with pytest.raises(ValueError, match="passes"):
        ops.estimate_ground(z(1, 4, 5, 3), z(1, 4, 3), [1, 2], passes=0)
    with pytest.raises(ValueError, match="passes"):
        ground.estimate(np.zeros((1, 4, 5, 3)), np.zeros((1, 4, 3)), [1, 2], passes=9)
    with pytest.raises(ValueError, match="speed"):
        ground.contacts(np.zeros((1, 4, 5, 3)), np.zeros((1, 4, 3)), [1, 2], speed=0.0)
    with pytest.raises(ValueError, match="radius"):
        harness.estimate_ground(z(1, 4, 5, 3), z(1, 4, 3), [1, 2], radius=65)
    with pytest.raises(ValueError, match="ground_speed"):
        harness.estimate_ground(z(1, 4, 5, 3), z(1, 4, 3), [1, 2], speed=float("nan"))
    with pytest.raises(ValueError, match=r"\[T,N,J,3\]"):
        harness.estimate_ground(z(4, 5, 3), z(4, 3), [1, 2])
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    with pytest.raises(ValueError, match="ground needs a trajectory"):
        harness.infer_sequence(model, None, z(30, 5, 2), [], [], aggregate="mean", stride=9, ground=True)
    with pytest.raises(ValueError, match="ground must be"):
        harness.infer_sequence(model, None, z(30, 5, 2), [], [], aggregate="mean", stride=9, trajectory=3, cam=z(9), ground=0)
    with pytest.raises(ValueError, match="ground_passes"):
        harness.infer_sequence(model, None, z(30, 5, 2), [], [], aggregate="mean", stride=9, trajectory=3, cam=z(9), ground=3, ground_passes=9)
    with pytest.raises(ValueError, match="ground needs a trajectory"):
        harness.evaluate_frames(model, None, z(30, 5, 2), z(30, 5, 3), z(9), [], [], ground=True)


def test_torch_ops_have_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import pafuse_amd.torch_ops  # noqa: F401
    with FakeTensorMode():
        pose, traj = torch.empty(2, 7, 134, 3, device="cuda"), torch.empty(2, 7, 3, device="cuda")
        foot, speed, contact = torch.ops.pafuse.foot_contacts(pose, traj, [18, 19, 20])
        assert foot.shape == (2, 7, 3, 3) and speed.shape == contact.shape == (2, 7, 3)
        state = torch.ops.pafuse.ground_sums(foot, contact, traj)
        assert state.shape == (2, 7, 14) and state.dtype == torch.float64
        sol = torch.ops.pafuse.ground_solve(state)
        assert [tuple(v.shape) for v in sol] == [(2, 4), (2,), (2, 3), (2,), (2,), (2, 3), (2,), (2,)]
        assert sol[0].dtype == torch.float64 and sol[6].dtype == torch.int32 and sol[7].dtype == torch.uint8
        pw, tw = torch.ops.pafuse.frames_to_world(pose, traj, sol[0])
        assert pw.shape == pose.shape and tw.shape == traj.shape
        assert len(torch.ops.pafuse.estimate_ground(pose, traj, [18, 19, 20, 21, 22, 23])) == 13

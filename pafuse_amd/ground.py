"""Which way is up: the ground plane of a video from its foot contacts, and the poses in world space -
the host statement, in numpy, of what foot_contacts_kernel, ground_sums_kernel, ground_solve_kernel and
frames_to_world_kernel (csrc/kernels.hpp; pafuse_foot_contacts, pafuse_ground_sums, pafuse_ground_solve,
pafuse_frames_to_world) compute.  fp64 throughout, every product rounded before it is added (no fused multiply-add), the
parentheses the order of the operations, every output rounded once.

A foot that is not moving is on the ground, and the ground is the plane through those points.

Contacts.  pose [T,N,J,3] fp32 root-relative, traj [T,N,3] fp32 the camera-space root (NaN: none), points int32 [K] the foot
points (1 <= K <= 16, each in [0, J)), radius r in 1 .. 64, speed in metres per FRAME (finite, > 0).  For every (t, n, k) the
camera-space position of the point in frame m is y[m] = double(pose[t,m,points[k]]) + double(traj[t,m]); it goes through the
walk of pafuse_amd.trajectory (line_sums: m = n - r .. n + r ascending, the biweight taper, weight 1.0); a frame takes part
if all six values are finite.  Only a LINE fit (two frames or more, D finite and > 0) with AT LEAST 3 FRAMES counts:
  foot  = (S2*Q0 - S1*Q1)/D per component      the line's value at d = 0
  slope = (S0*Q1 - S1*Q0)/D per component      its change per frame: the foot's velocity
  v = sqrt((sx*sx + sy*sy) + sz*sz)            a correctly rounded sqrt
  w = (1 - (v/speed)*(v/speed))^2  if v < speed, else 0          q = v/speed; h = 1 - q*q; w = h*h
-> foot [T,N,K,3], foot_speed [T,N,K], contact [T,N,K] fp32.  Without such a line: foot and foot_speed NaN, contact 0.

Per-frame sums.  For every (t, n), over k ascending, p = double(foot[t,n,k]), c = double(contact[t,n,k]), root =
double(traj[t,n]).  A point takes part if c > 0 and the three components of p AND of root are finite (a frame without a root of
its own has no body-up term to give, and its world-space pose is NaN anyway).  Its weight is omega = c * rho:
  first pass (no plane):  rho = 1
  later:  z = (((nx*px + ny*py) + nz*pz) - d) / (gate * sigma);  rho = (1 - z*z)^2 if |z| < 1, else 0
          with (nx, ny, nz, d) = plane[t] and sigma = scale[t] of the previous pass.  A NaN plane (code 0) gives rho = 0:
          a step without a plane stays without one.
A point with omega > 0 adds, everyone else adds nothing (the running sums start at +0.0, so a frame whose every weight is 0
is exactly 14 zeros):
  slot 0        omega
  slots 1..3    omega*p_a
  slots 4..9    (omega*p_a)*p_b   for (a,b) = xx xy xz yy yz zz
  slots 10..12  omega*(root_a - p_a)         the body's own up: the root is above the feet
  slot 13       1.0                          the number of points
-> state double [T,N,14].  States of several videos of one scene concatenate along N, as the focal states do.
The second moments are taken ABOUT THE CAMERA ORIGIN, deliberately: a centred form would need the mean before the sums, a
second walk.  In fp64 the cancellation in M/W - mu*mu^T for points 5 m away costs about 25 m^2 * 2^-53 = 3e-15 m^2 absolute,
that is 1e-9 relative on an eigenvalue of a square millimetre - far below everything this estimate is asked for.

Solve, per t.  The 14 slots are summed over the frames in rootfit.lane_sum's order (lane l adds frames l, l + 64, ...
ascending, then the butterfly).  W = slot 0, mu_a = S_a/W, C_ab = M_ab/W - mu_a*mu_b, u = slots 10..12.
The eigen decomposition of C is CYCLIC JACOBI (jacobi_eigen below): 8 sweeps, fixed, over (p,q) = (0,1), (0,2), (1,2); V = I
at the start; for each pair, with r the third index,
  a_pq == 0 exactly: skipped (nothing changes)
  theta = (a_qq - a_pp)/(2*a_pq);  t = sgn(theta)/(|theta| + sqrt(theta*theta + 1)),  sgn = -1 if theta < 0 else +1
  c = 1/sqrt(t*t + 1);  s = t*c
  a_pp' = a_pp - t*a_pq;  a_qq' = a_qq + t*a_pq;  a_pq' = 0
  a_rp' = c*a_rp - s*a_rq;  a_rq' = s*a_rp + c*a_rq
  v_ip' = c*v_ip - s*v_iq;  v_iq' = s*v_ip + c*v_iq   for the rows i = 0, 1, 2
Only + - * / sqrt.  WHEN theta*theta OVERFLOWS (an off-diagonal below 1e-154 of the diagonal's gap; theta itself may already be
infinite) the formulas are evaluated as they stand in IEEE arithmetic: sqrt(+inf) = +inf, t = +-0, c = 1, s = +-0 - the diagonal
and the vectors keep their bits and a_pq becomes 0.  No special case, on the host or on the device.  A NaN in C (W = 0) spreads
to everything, and every comparison below then fails: code 0.
The eigenvalues are the diagonal, the eigenvectors the columns of V (unit to rounding; not normalised again).  They are sorted
ascending by the compare-and-swap network (0,1), (1,2), (0,1), each swapping only on a strict >: equal eigenvalues keep their
order (the lower index first).  lambda0 <= lambda1 <= lambda2.
With |x| = sqrt((x0*x0 + x1*x1) + x2*x2), x.y = (x0*y0 + x1*y1) + x2*y2 and normalize(x) = x_a / |x|:
  code 1 plane:  lambda1 >= spread^2 and lambda1 >= 9*max(lambda0, floor^2)      n = the eigenvector of lambda0
  code 2 line:   otherwise, if lambda2 >= spread^2: the contacts lie on a line a (the eigenvector of lambda2; a person standing),
                 w = u - (u.a)*a, n = normalize(w): the plane through that line closest to the body's own up.
                 |w| not > 0 (the body's up along the line, or none): code 0 - it does not fall through to code 3
  code 3 body:   otherwise, if W > 0 and |u| > 0:  n = normalize(u)
  code 0 none:   NaN in every floating-point output, never a guess
  sign:   n is negated iff n.u < 0 - the root is above the feet, whichever way the camera's y axis points
  d = n.mu
  q = n.(C n) with (C n)_a = (C_a0*n0 + C_a1*n1) + C_a2*n2 on C as it was before the rotations: the weighted mean of the squared
      distance to the plane through the moments;  rms = sqrt(q) if q > 0 else 0;  sigma = rms if rms > floor else floor
-> plane [T,4] fp64 (n, d) and scale [T] fp64 (sigma) for the next pass; fp32, rounded once: up [T,3] (n), camera_height [T]
(-d), ground_rms [T] (rms), ground_eig [T,3]; ground_points [T] int32 (slot 13, whatever the code); ground_code [T] uint8.
`passes` repetitions of sums + solve, each re-weighting with the plane of the one before.

Defaults: speed 0.015 m/frame, gate 2.5, floor 0.005 m, spread 0.03 m, radius 3, 3 passes.  DEFAULTS, NOT TUNED VALUES.

World.  Per t from plane[t]: z = n;  e = (1,0,0), the camera's right - if |n0| > 0.99, e = (0,0,1);  x = normalize(e - (e.n)*n)
(e.n is n0 or n2 itself);  y = z cross x = (n1*x2 - n2*x1, n2*x0 - n0*x2, n0*x1 - n1*x0).  Every camera-space point
p = double(pose[t,n,j]) + double(traj[t,n]) becomes (x.p, y.p, n.p - d): pose_world [T,N,J,3]; the root double(traj[t,n])
likewise: traj_world [T,N,3]; fp32, rounded once.  NaN in gives NaN out, code 0 gives NaN.  The height of a joint above the
ground is its third component.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

from . import rootfit, trajectory

SLOTS = 14
MAX_POINTS = 16
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (1, 2))
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                 # the order of slots 4..9
NONE, PLANE, LINE, BODY = 0, 1, 2, 3                                    # ground_code
DEFAULTS = dict(radius=3, speed=0.015, passes=3, gate=2.5, floor=0.005, spread=0.03)   # defaults, not tuned values
MIN_FRAMES = 3


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _norm(x):
    return np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])


def _need_points(points, J):
    points = np.asarray(points, dtype=np.int64).reshape(-1)
    if not 1 <= points.size <= MAX_POINTS or points.min() < 0 or points.max() >= J:
        raise ValueError(f"points: 1 .. {MAX_POINTS} joints, each in [0, {J}), got {points.tolist()}")
    return points


def _need_positive(name, v):
    v = float(v)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be finite and > 0, got {v!r}")
    return np.float64(v)


def contacts(pose, traj, points, radius=3, speed=0.015):
    """pose [T,N,J,3] fp32, traj [T,N,3] fp32, points [K] -> (foot [T,N,K,3], foot_speed [T,N,K], contact [T,N,K]) fp32: what
    pafuse_foot_contacts writes."""
    pose, traj = np.asarray(pose, dtype=np.float32), np.asarray(traj, dtype=np.float32)
    T, N, J, _ = pose.shape
    assert pose.shape == (T, N, J, 3) and traj.shape == (T, N, 3)
    points = _need_points(points, J)
    r = int(radius)
    if not 1 <= r <= 64:
        raise ValueError(f"contacts: radius must lie in 1 .. 64, got {radius!r}")
    speed = _need_positive("speed", speed)
    with np.errstate(all="ignore"):
        pk = pose[:, :, points]                                        # [T,N,K,3]
        y = pk.astype(np.float64) + traj.astype(np.float64)[:, :, None]
        part = np.isfinite(pk).all(axis=-1) & np.isfinite(traj).all(axis=-1)[:, :, None]
        first = lambda a: np.moveaxis(a, 1, 0)                         # line_sums walks axis 0; elementwise, so no bit moves
        value, slope, code, cnt = trajectory.local_line_slope(first(y), first(part), np.ones(first(part).shape), r)
        has = first((code == trajectory.LINE) & (cnt >= MIN_FRAMES))   # [T,N,K]
        value, slope = first(value), first(slope)
        v = _norm([slope[..., a] for a in range(3)])
        q = v / speed
        h = 1.0 - q * q
        w = np.where(has & (v < speed), h * h, 0.0)
        nan = np.float32(np.nan)
        foot = np.where(has[..., None], value.astype(np.float32), nan)
        foot_speed = np.where(has, v.astype(np.float32), nan)
    return foot.astype(np.float32), foot_speed.astype(np.float32), w.astype(np.float32)


def weights(foot, contact, traj, plane=None, scale=None, gate=2.5):
    """-> omega [T,N,K] fp64: the weight contact * rho of every point in a pass that reads `plane` and `scale` (None: the first),
    0.0 for a point that takes no part"""
    foot, contact, traj = (np.asarray(v, dtype=np.float32) for v in (foot, contact, traj))
    gate = _need_positive("gate", gate)
    with np.errstate(all="ignore"):
        p = [foot[..., a].astype(np.float64) for a in range(3)]
        c = contact.astype(np.float64)
        on = (contact > 0) & np.isfinite(foot).all(axis=-1) & np.isfinite(traj).all(axis=-1)[:, :, None]
        if plane is None:
            om = c
        else:
            plane, scale = np.asarray(plane, dtype=np.float64), np.asarray(scale, dtype=np.float64)
            assert plane.shape == (foot.shape[0], 4) and scale.shape == (foot.shape[0],)
            nx, ny, nz, d = (plane[:, a][:, None, None] for a in range(4))
            z = (((nx * p[0] + ny * p[1]) + nz * p[2]) - d) / (gate * scale)[:, None, None]
            g = 1.0 - z * z
            om = c * np.where(np.abs(z) < 1.0, g * g, 0.0)
        return np.where(on & (om > 0), om, 0.0)


def sums(foot, contact, traj, plane=None, scale=None, gate=2.5):
    """foot [T,N,K,3], contact [T,N,K], traj [T,N,3] fp32; plane [T,4], scale [T] fp64 of the previous pass or both None ->
    state [T,N,14] float64: what pafuse_ground_sums writes."""
    foot, contact, traj = (np.asarray(v, dtype=np.float32) for v in (foot, contact, traj))
    T, N, K, _ = foot.shape
    assert foot.shape == (T, N, K, 3) and contact.shape == (T, N, K) and traj.shape == (T, N, 3)
    assert (plane is None) == (scale is None)
    gate = _need_positive("gate", gate)
    state = np.zeros((T, N, SLOTS))
    omega = weights(foot, contact, traj, plane, scale, gate)
    with np.errstate(all="ignore"):
        root = traj.astype(np.float64)
        for k in range(K):                                             # ascending
            p = [foot[:, :, k, a].astype(np.float64) for a in range(3)]
            om = omega[:, :, k]
            on = om > 0
            add = lambda i, v: state.__setitem__((..., i), state[..., i] + np.where(on, v, 0.0))
            add(0, om)
            op = [om * p[a] for a in range(3)]
            for a in range(3):
                add(1 + a, op[a])
            for i, (a, b) in enumerate(SYM):
                add(4 + i, op[a] * p[b])
            for a in range(3):
                add(10 + a, om * (root[..., a] - p[a]))
            add(13, np.ones_like(om))
    return state


def jacobi_eigen(C):
    """C: the six entries xx xy xz yy yz zz of symmetric 3x3 matrices, arrays of one shape (or a [...,6] array) ->
    (lam: three arrays ascending, vec: vec[k] = the three components of the eigenvector of lam[k]).  THE decomposition of the
    solve: 8 cyclic sweeps, then the sort; see the module text."""
    if isinstance(C, np.ndarray):
        C = [C[..., i] for i in range(6)]
    a = {ab: np.asarray(C[i], dtype=np.float64) for i, ab in enumerate(SYM)}
    one, zero = np.ones_like(a[0, 0]), np.zeros_like(a[0, 0])
    V = [[one if i == j else zero for j in range(3)] for i in range(3)]     # V[i][j]: row i, column j
    key = lambda i, j: (i, j) if i <= j else (j, i)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                r = 3 - p - q
                apq, app, aqq, arp, arq = a[p, q], a[p, p], a[q, q], a[key(r, p)], a[key(r, q)]
                skip = apq == 0
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                keep = lambda old, new: np.where(skip, old, new)
                a[p, p], a[q, q], a[p, q] = keep(app, app - t * apq), keep(aqq, aqq + t * apq), keep(apq, zero)
                a[key(r, p)], a[key(r, q)] = keep(arp, c * arp - s * arq), keep(arq, s * arp + c * arq)
                for i in range(3):
                    vp, vq = V[i][p], V[i][q]
                    V[i][p], V[i][q] = keep(vp, c * vp - s * vq), keep(vq, s * vp + c * vq)
        lam = [a[0, 0], a[1, 1], a[2, 2]]
        vec = [[V[i][k] for i in range(3)] for k in range(3)]
        for i, j in ((0, 1), (1, 2), (0, 1)):                          # strict >: equal eigenvalues keep their order
            sw = lam[i] > lam[j]
            lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
            vi, vj = vec[i], vec[j]
            vec[i] = [np.where(sw, vj[k], vi[k]) for k in range(3)]
            vec[j] = [np.where(sw, vi[k], vj[k]) for k in range(3)]
    return lam, vec


def totals(state):
    """state [T,N,14] -> [T,14]: the slots summed over the frames in the order of the solve"""
    state = np.asarray(state, dtype=np.float64)
    assert state.ndim == 3 and state.shape[-1] == SLOTS
    return rootfit.lane_sum(np.moveaxis(state, 1, -1))


OUTPUTS = ("plane", "scale", "up", "camera_height", "ground_rms", "ground_eig", "ground_points", "ground_code")


def solve(state, floor=0.005, spread=0.03):
    """state [T,N,14] float64 -> dict: plane [T,4], scale [T] fp64; up [T,3], camera_height, ground_rms [T], ground_eig [T,3]
    fp32; ground_points [T] int32; ground_code [T] uint8: what pafuse_ground_solve writes."""
    floor, spread = _need_positive("floor", floor), _need_positive("spread", spread)
    tot = totals(state)
    with np.errstate(all="ignore"):
        W = tot[:, 0]
        mu = [tot[:, 1 + a] / W for a in range(3)]
        C = [tot[:, 4 + i] / W - mu[a] * mu[b] for i, (a, b) in enumerate(SYM)]
        u = [tot[:, 10 + a] for a in range(3)]
        lam, vec = jacobi_eigen(C)
        floor2, spread2 = floor * floor, spread * spread
        is_plane = (lam[1] >= spread2) & (lam[1] >= 9.0 * np.where(lam[0] > floor2, lam[0], floor2))
        is_line = ~is_plane & (lam[2] >= spread2)
        ua = _dot(u, vec[2])
        w = [u[a] - ua * vec[2][a] for a in range(3)]
        wn, un = _norm(w), _norm(u)
        is_body = ~is_plane & ~is_line & (W > 0) & (un > 0)
        code = np.where(is_plane, PLANE, np.where(is_line, np.where(wn > 0, LINE, NONE), np.where(is_body, BODY, NONE)))
        n = [np.where(code == PLANE, vec[0][a], np.where(code == LINE, w[a] / wn, u[a] / un)) for a in range(3)]
        flip = _dot(n, u) < 0
        n = [np.where(flip, -n[a], n[a]) for a in range(3)]
        d = _dot(n, mu)
        Cm = [[C[SYM.index((min(a, b), max(a, b)))] for b in range(3)] for a in range(3)]
        g = [(Cm[a][0] * n[0] + Cm[a][1] * n[1]) + Cm[a][2] * n[2] for a in range(3)]
        q = _dot(n, g)
        rms = np.where(q > 0, np.sqrt(q), 0.0)
        sigma = np.where(rms > floor, rms, floor)
        ok = code != NONE
        nan = np.float64(np.nan)
        plane = np.stack([np.where(ok, v, nan) for v in (n[0], n[1], n[2], d)], axis=-1)
        scale = np.where(ok, sigma, nan)
        f32 = lambda v: np.where(ok, v, nan).astype(np.float32)
        return {"plane": plane, "scale": scale, "up": np.stack([f32(n[a]) for a in range(3)], axis=-1),
                "camera_height": f32(-d), "ground_rms": f32(rms), "ground_eig": np.stack([f32(lam[a]) for a in range(3)], axis=-1),
                "ground_points": tot[:, 13].astype(np.int32), "ground_code": code.astype(np.uint8)}


def world_axes(plane):
    """plane [T,4] fp64 -> (x, y, z): three lists of three [T] arrays, the rows of the camera-to-world rotation"""
    plane = np.asarray(plane, dtype=np.float64)
    n = [plane[:, a] for a in range(3)]
    with np.errstate(all="ignore"):
        alt = np.abs(n[0]) > 0.99
        e = [np.where(alt, 0.0, 1.0), np.zeros_like(n[0]), np.where(alt, 1.0, 0.0)]
        en = np.where(alt, n[2], n[0])
        w = [e[a] - en * n[a] for a in range(3)]
        wn = _norm(w)
        x = [w[a] / wn for a in range(3)]
        y = [n[1] * x[2] - n[2] * x[1], n[2] * x[0] - n[0] * x[2], n[0] * x[1] - n[1] * x[0]]
    return x, y, n


def to_world(pose, traj, plane):
    """pose [T,N,J,3], traj [T,N,3] fp32, plane [T,4] fp64 -> (pose_world [T,N,J,3], traj_world [T,N,3]) fp32: what
    pafuse_frames_to_world writes."""
    pose, traj = np.asarray(pose, dtype=np.float32), np.asarray(traj, dtype=np.float32)
    plane = np.asarray(plane, dtype=np.float64)
    T, N, J, _ = pose.shape
    assert traj.shape == (T, N, 3) and plane.shape == (T, 4)
    x, y, n = world_axes(plane)
    d = plane[:, 3]
    with np.errstate(all="ignore"):
        root = traj.astype(np.float64)
        cam = pose.astype(np.float64) + root[:, :, None]

        def turn(p, shape):
            ax = lambda v: [v[a].reshape(shape) for a in range(3)]
            q = [p[..., a] for a in range(3)]
            return np.stack([_dot(ax(x), q), _dot(ax(y), q), _dot(ax(n), q) - d.reshape(shape)], axis=-1).astype(np.float32)
        return turn(cam, (T, 1, 1)), turn(root, (T, 1))


def estimate(pose, traj, points, radius=3, speed=0.015, passes=3, gate=2.5, floor=0.005, spread=0.03):
    """The chain: contacts, `passes` times sums + solve, world -> the dict of solve plus foot, foot_speed, contact, pose_world and
    traj_world: what ops.estimate_ground returns."""
    if isinstance(passes, bool) or int(passes) != passes or not 1 <= int(passes) <= 8:
        raise ValueError(f"passes must be an integer in 1 .. 8, got {passes!r}")
    foot, foot_speed, contact = contacts(pose, traj, points, radius, speed)
    out = {"plane": None, "scale": None}
    for _ in range(int(passes)):
        out = solve(sums(foot, contact, traj, out["plane"], out["scale"], gate), floor, spread)
    pose_world, traj_world = to_world(pose, traj, out["plane"])
    return {**out, "foot": foot, "foot_speed": foot_speed, "contact": contact, "pose_world": pose_world, "traj_world": traj_world}

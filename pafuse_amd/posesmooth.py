"""The per-frame pose smoothed along the frames, every frame weighted by the inverse of its hypothesis covariance (DESIGN.md
section 6m) - the host statement, in numpy, of what pose_precision_kernel and pose_smooth_kernel (csrc/kernels.hpp;
pafuse_pose_smooth) compute.

pose [T,N,J,3] fp32, cov [T,N,J,6] fp32 in the order xx, xy, xz, yy, yz, zz (finish_frames' "cov") or None, radius r in
1 .. 64, floor in metres (fp32, finite and > 0).  Everything below is fp64, one rounded operation after the other, no fused
multiply-add; a sum written  (a + b) + c  is added in that order.

Per row (t, m, j) - precision():

  s2 = double(floor)*double(floor)
  xx = cov0 + s2   yy = cov3 + s2   zz = cov5 + s2     xy = cov1  xz = cov2  yz = cov4      (cov None: the six entries are 0)
  c00 = yy*zz - yz*yz    c01 = xz*yz - xy*zz    c02 = xy*yz - xz*yy
  c11 = xx*zz - xz*xz    c12 = xy*xz - xx*yz    c22 = xx*yy - xy*xy
  det = (xx*c00 + xy*c01) + xz*c02
  the row TAKES PART iff its three pose components are finite, det is finite, xx > 0, c22 > 0 and det > 0 (the three leading
  minors: Sylvester's criterion for a positive definite matrix) - a NaN anywhere in its cov removes it
  W = (c00, c01, c02, c11, c12, c22) / det              six divisions: the inverse of Sigma + floor^2*I, symmetric, packed

Per output (t, n, j) the frames m = max(0, n - r) .. min(N - 1, n + r) are walked in ascending order, d = m - n; a row that
takes no part is skipped:

  q = double(d*d) / double((r+1)*(r+1));  h = 1.0 - q;  g = h*h        LineFilter's taper (pafuse_amd.trajectory)
  G = g*W    Gd = G*double(d)    Gdd = Gd*double(d)                    six values each
  z_k = (G_k0*y0 + G_k1*y1) + G_k2*y2    zd_k = z_k*double(d)          k = 0, 1, 2;  G_kl the symmetric matrix G
  A0 += G   A1 += Gd   A2 += Gdd   b0 += z   b1 += zd   cnt += 1       24 sums and a count

  LINE (code 1): cnt >= 2, the 6x6 system  [[A2, A1], [A1, A0]] * [slope; value] = [b1; b0]  factors by ldl_solve with six
     pivots finite and > 0, and the three components of value are finite.
  MEAN (code 2): otherwise, cnt >= 1 and the 3x3 system  A0 * value = b0  factors by ldl_solve, three pivots finite and > 0.
  NONE (code 3): otherwise; NaN.

The value is rounded once to fp32; a value any component of which is not finite in fp32 is code 3, NaN in all three.  The
codes are LineKind's and the repair's 1, 2, 3.

ldl_solve(M, b, tail) - LDL^T without a square root and without pivoting, on the lower triangle M[i][j], i >= j, of a
symmetric n x n matrix; only the last `tail` unknowns are back-substituted:

  for j = 0 .. n-1:
      for i = j .. n-1:   u[i][j] = M[i][j];  for k = 0 .. j-1 ascending:  u[i][j] = u[i][j] - u[i][k]*l[j][k]
      D[j] = u[j][j]                                                     the pivot: finite and > 0, or the system does not factor
      for i = j+1 .. n-1: l[i][j] = u[i][j] / D[j]
  for i = 0 .. n-1:       w[i] = b[i];        for k = 0 .. i-1 ascending:  w[i] = w[i] - l[i][k]*w[k]
  for i = n-1 down to n-tail:  x[i] = w[i] / D[i];  for k = i+1 .. n-1 ascending:  x[i] = x[i] - l[k][i]*x[k]

With equal covariances W cancels and the result is trajectory.local_line per joint: constant velocity comes through without
lag and without shrinking at the ends.  Slope first and value last halves the back-substitution.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

LINE, MEAN, NONE = 1, 2, 3
SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))     # the packed index of entry (k, l) of a symmetric 3x3: xx xy xz yy yz zz


def check(radius, floor):
    """-> (r, floor as fp32); ValueError for a radius outside 1 .. 64 (or a bool) and a floor that is not finite and > 0"""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 64:
        raise ValueError(f"pose_smooth: radius must be an integer in 1 .. 64, got {radius!r}")
    if isinstance(floor, (bool, np.bool_)) or not isinstance(floor, (int, float, np.floating, np.integer)):
        raise ValueError(f"pose_smooth: floor must be a finite number > 0 (metres), got {floor!r}")
    with np.errstate(all="ignore"):
        f = np.float32(floor)
    if not (np.isfinite(f) and f > 0):
        raise ValueError(f"pose_smooth: floor must be finite and > 0 in fp32 (metres), got {floor!r}")
    return int(radius), f


def precision(pose, cov, floor):
    """pose [...,3] fp32, cov [...,6] fp32 or None, floor fp32 -> (W [...,6] fp64, part [...] bool)"""
    pose = np.asarray(pose, dtype=np.float32)
    s2 = np.float64(np.float32(floor)) * np.float64(np.float32(floor))
    c = np.zeros(pose.shape[:-1] + (6,)) if cov is None else np.asarray(cov, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        xx, xy, xz, yy, yz, zz = c[..., 0] + s2, c[..., 1], c[..., 2], c[..., 3] + s2, c[..., 4], c[..., 5] + s2
        c00 = yy * zz - yz * yz
        c01 = xz * yz - xy * zz
        c02 = xy * yz - xz * yy
        c11 = xx * zz - xz * xz
        c12 = xy * xz - xx * yz
        c22 = xx * yy - xy * xy
        det = (xx * c00 + xy * c01) + xz * c02
        part = np.isfinite(pose).all(axis=-1) & np.isfinite(det) & (xx > 0) & (c22 > 0) & (det > 0)
        W = np.stack([c00, c01, c02, c11, c12, c22], axis=-1) / det[..., None]
    return W, part


def ldl_solve(M, b, tail):
    """THE factorisation above, elementwise on arrays: M[i][j] (i >= j) and b[i] fp64 arrays of one shape ->
    (the last `tail` unknowns, ok: every pivot finite and > 0)"""
    n = len(b)
    u = [[None] * n for _ in range(n)]
    l = [[None] * n for _ in range(n)]
    D = [None] * n
    ok = np.ones(np.shape(b[0]), dtype=bool)
    for j in range(n):
        for i in range(j, n):
            v = M[i][j]
            for k in range(j):
                v = v - u[i][k] * l[j][k]
            u[i][j] = v
        D[j] = u[j][j]
        ok = ok & np.isfinite(D[j]) & (D[j] > 0)
        for i in range(j + 1, n):
            l[i][j] = u[i][j] / D[j]
    w = []
    for i in range(n):
        v = b[i]
        for k in range(i):
            v = v - l[i][k] * w[k]
        w.append(v)
    x = [None] * n
    for i in range(n - 1, n - 1 - tail, -1):
        v = w[i] / D[i]
        for k in range(i + 1, n):
            v = v - l[k][i] * x[k]
        x[i] = v
    return x[n - tail:], ok


def sums(pose, cov, radius, floor):
    """-> (A0, A1, A2 [T,N,J,6], b0, b1 [T,N,J,3] fp64, cnt [T,N,J] int64): the 24 sums and the count of every output"""
    pose = np.asarray(pose, dtype=np.float32)
    T, N, J, _ = pose.shape
    r = int(radius)
    W, part = precision(pose, cov, floor)
    y = pose.astype(np.float64)
    A0, A1, A2 = np.zeros((T, N, J, 6)), np.zeros((T, N, J, 6)), np.zeros((T, N, J, 6))
    b0, b1 = np.zeros((T, N, J, 3)), np.zeros((T, N, J, 3))
    cnt = np.zeros((T, N, J), dtype=np.int64)
    n = np.arange(N)
    span = np.float64((r + 1) * (r + 1))
    with np.errstate(all="ignore"):
        for d in range(-r, r + 1):                                    # ascending m = n + d
            m = n + d
            inside = (m >= 0) & (m < N)
            mc = np.clip(m, 0, N - 1)
            take = part[:, mc] & inside[None, :, None]
            q = np.float64(d * d) / span
            h = 1.0 - q
            g = h * h
            dd = np.float64(d)
            G = g * W[:, mc]
            Gd = G * dd
            Gdd = Gd * dd
            ym = y[:, mc]
            z = np.stack([(G[..., SYM[k][0]] * ym[..., 0] + G[..., SYM[k][1]] * ym[..., 1]) + G[..., SYM[k][2]] * ym[..., 2]
                          for k in range(3)], axis=-1)
            zd = z * dd
            t6, t3 = take[..., None], take[..., None]
            A0 = A0 + np.where(t6, G, 0.0)
            A1 = A1 + np.where(t6, Gd, 0.0)
            A2 = A2 + np.where(t6, Gdd, 0.0)
            b0 = b0 + np.where(t3, z, 0.0)
            b1 = b1 + np.where(t3, zd, 0.0)
            cnt = cnt + take
    return A0, A1, A2, b0, b1, cnt


def smooth_f64(pose, cov, radius, floor):
    """-> (value [T,N,J,3] fp64 BEFORE its rounding - NaN where neither system factors - and code [T,N,J] uint8 before the
    fp32 test)"""
    A0, A1, A2, b0, b1, cnt = sums(pose, cov, radius, floor)
    blocks = ((A2, A1), (A1, A0))
    M = [[blocks[i // 3][j // 3][..., SYM[i % 3][j % 3]] for j in range(6)] for i in range(6)]
    rhs = [b1[..., k] for k in range(3)] + [b0[..., k] for k in range(3)]
    with np.errstate(all="ignore"):
        v6, ok6 = ldl_solve(M, rhs, 3)
        v6 = np.stack(v6, axis=-1)
        line = (cnt >= 2) & ok6 & np.isfinite(v6).all(axis=-1)
        v3, ok3 = ldl_solve([[A0[..., SYM[i][j]] for j in range(3)] for i in range(3)], [b0[..., k] for k in range(3)], 3)
        v3 = np.stack(v3, axis=-1)
        mean = ~line & (cnt >= 1) & ok3
    value = np.where(line[..., None], v6, np.where(mean[..., None], v3, np.nan))
    code = np.where(line, LINE, np.where(mean, MEAN, NONE)).astype(np.uint8)
    return value, code


def smooth(pose, cov, radius, floor=1e-3):
    """pose [T,N,J,3] fp32, cov [T,N,J,6] fp32 or None, radius 1 .. 64, floor > 0 in metres -> (out [T,N,J,3] fp32, code
    [T,N,J] uint8): what pafuse_pose_smooth writes, one rounded operation after the other."""
    r, f = check(radius, floor)
    pose = np.asarray(pose, dtype=np.float32)
    if pose.ndim != 4 or pose.shape[-1] != 3 or 0 in pose.shape:
        raise ValueError(f"pose_smooth: pose must be [T,N,J,3] with T, N, J >= 1, got {pose.shape}")
    if cov is not None:
        cov = np.asarray(cov, dtype=np.float32)
        if cov.shape != pose.shape[:3] + (6,):
            raise ValueError(f"pose_smooth: cov must be [T,N,J,6] = {pose.shape[:3] + (6,)}, got {cov.shape}")
    value, code = smooth_f64(pose, cov, r, f)
    with np.errstate(all="ignore"):
        out = value.astype(np.float32)
    bad = ~np.isfinite(out).all(axis=-1)
    out = np.where(bad[..., None], np.float32(np.nan), out).astype(np.float32)
    code = np.where(bad, NONE, code).astype(np.uint8)
    return out, code

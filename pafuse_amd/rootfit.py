"""The root fit of J-Agg without a trajectory - the host statement, in numpy, of what
pose_fit_partials_kernel (csrc/kernels.hpp, pafuse_pose_partials_fit) computes.

The hypotheses are root-relative; the reprojection error of J-Agg needs absolute points.  With the intrinsics known, the
root position t of one hypothesis in one frame is a linear least-squares problem in three unknowns: for the whole-body
joint w_j (fp32, as wb_joint gives it), its screen-normalised detection (u_j, v_j) with weight c_j >= 0, and
fx, fy, cx, cy = cam[0:4], everything in fp64,

  a_j = (u_j - cx) / fx          b_j = (v_j - cy) / fy
  rx_j = a_j*w_jz - w_jx         ry_j = b_j*w_jz - w_jy            (pinhole: tx - a*tz = rx, ty - b*tz = ry)
  W = sum c    Sa = sum c*a    Sb = sum c*b    Sq = sum c*(a*a + b*b)          per (b, f): no hypothesis in them
  Srx = sum c*rx    Sry = sum c*ry    Sm = sum c*(a*rx + b*ry)                 per hypothesis
  den = Sq - (Sa*Sa + Sb*Sb)/W
  tz = (-Sm + (Sa*Srx + Sb*Sry)/W) / den
  tx = (Srx + Sa*tz)/W           ty = (Sry + Sb*tz)/W

Every product is rounded before it is added (no fused multiply-add: the kernel pins contraction off), and the
parentheses above are the order of the operations.  The distortion terms cam[4:9] take no part in the fit; they do in
the error below.

Weights.  A weight that is not > 0 (zero, negative, NaN) takes its joint out of every sum - the term is 0.0 whatever the
joint's coordinates hold, NaN included - and out of the pick.  conf=None is every weight 1.

No fit.  A (hypothesis, frame) has no fit if fewer than two joints have a positive weight, if den is not finite and > 0
(one direction of sight: nothing fixes the depth), or if t, rounded to fp32, is not finite.  Its t is NaN.

The order of every sum over j (SUM_ORDER).  Lane l of 64 adds the terms of its joints l, l + 64, l + 128, ... in ascending
order, starting from 0.0; then v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1, after which all 64 lanes hold the same
bits (a + b == b + a) - lane 0 is taken.  A lane without a joint contributes its 0.0.  (A running sum that starts at
+0.0 never becomes -0.0, so "adds 0.0" and "adds nothing" are the same bits.)

The pick.  t is rounded to fp32; e2 is the fp32 reprojection error of pose_partials_kernel with t in the place of traj;
per joint the first minimum over the hypotheses wins; a joint without a positive weight, and a hypothesis without a
fit, offer no candidate: (e2, idx, sel) = (+inf, -1, NaN NaN NaN).  reproj_error states e2 one rounded operation after
the other; the kernel's e2 is compiled like pose_partials_kernel's (the compiler may fuse there), which is why the GPU
tests compare the pick with THAT kernel's on the fitted roots and only tfit with this module.

This module is test infrastructure and the documentation of the fit.  The product path never calls it.
"""
import numpy as np

LANES = 64
SUM_ORDER = (32, 16, 8, 4, 2, 1)


def whole_body(pred, conn):
    """wb_joint in numpy: pred [...,J,3] fp32 part-centred, conn int [J] -> pred[j] + pred[conn[j]] in fp32, joint 0 at 0."""
    pred = np.asarray(pred, dtype=np.float32)
    out = pred + pred[..., np.asarray(conn, dtype=np.int64), :]
    out[..., 0, :] = 0
    return out


def lane_sum(terms):
    """[...,J] fp64 -> [...]: the sum over the last axis in SUM_ORDER."""
    terms = np.asarray(terms, dtype=np.float64)
    J = terms.shape[-1]
    rounds = -(-J // LANES)
    pad = np.zeros(terms.shape[:-1] + (rounds * LANES - J,))
    x = np.concatenate([terms, pad], axis=-1).reshape(terms.shape[:-1] + (rounds, LANES))
    acc = np.zeros(terms.shape[:-1] + (LANES,))
    for r in range(rounds):
        acc = acc + x[..., r, :]
    lane = np.arange(LANES)
    for o in SUM_ORDER:
        acc = acc + acc[..., lane ^ o]
    return acc[..., 0]


def _fit(wb, x2d, conf, cam):
    """-> (t [B,T,P,F,3] fp64, fit [B,T,P,F] bool): the fit before its rounding to fp32, and where there is one"""
    wb = np.asarray(wb, dtype=np.float32)
    x2d = np.asarray(x2d, dtype=np.float32)
    cam = np.asarray(cam, dtype=np.float32).reshape(-1)
    B, T, P, F, J, _ = wb.shape
    assert x2d.shape == (B, F, J, 2) and cam.size >= 4
    c32 = np.ones((B, F, J), dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)
    assert c32.shape == (B, F, J)
    fx, fy, cx, cy = (np.float64(v) for v in cam[:4])
    with np.errstate(all="ignore"):
        pos = c32 > 0                                               # False for NaN
        c = c32.astype(np.float64)
        a = (x2d[..., 0].astype(np.float64) - cx) / fx
        b = (x2d[..., 1].astype(np.float64) - cy) / fy
        term = lambda v: np.where(pos, v, 0.0)
        W, Sa, Sb = lane_sum(term(c)), lane_sum(term(c * a)), lane_sum(term(c * b))
        Sq = lane_sum(term(c * (a * a + b * b)))
        den = Sq - (Sa * Sa + Sb * Sb) / W                          # [B,F]
        can = (pos.sum(axis=-1) >= 2) & np.isfinite(den) & (den > 0)
        w = wb.astype(np.float64)                                   # [B,T,P,F,J,3]
        a6, b6, c6, pos6 = (v[:, None, None] for v in (a, b, c, pos))
        rx = a6 * w[..., 2] - w[..., 0]
        ry = b6 * w[..., 2] - w[..., 1]
        term6 = lambda v: np.where(pos6, v, 0.0)
        Srx, Sry = lane_sum(term6(c6 * rx)), lane_sum(term6(c6 * ry))
        Sm = lane_sum(term6(c6 * (a6 * rx + b6 * ry)))              # [B,T,P,F]
        W4, Sa4, Sb4, den4 = (v[:, None, None] for v in (W, Sa, Sb, den))
        tz = (-Sm + (Sa4 * Srx + Sb4 * Sry) / W4) / den4
        tx = (Srx + Sa4 * tz) / W4
        ty = (Sry + Sb4 * tz) / W4
        t = np.stack([tx, ty, tz], axis=-1)
        return t, can[:, None, None] & np.isfinite(t.astype(np.float32)).all(axis=-1)


def fit_roots(wb, x2d, conf, cam):
    """wb [B,T,P,F,J,3] fp32 whole-body hypotheses, x2d [B,F,J,2] fp32, conf [B,F,J] fp32 or None, cam [>=4] fp32 ->
    t [B,T,P,F,3] fp32, NaN where there is no fit: what the kernel writes to tfit."""
    t, fit = _fit(wb, x2d, conf, cam)
    with np.errstate(all="ignore"):
        t = t.astype(np.float32)
    t[~fit] = np.nan
    return t


def fit_root(w, uv, c, cam):
    """One hypothesis in one frame: w [J,3], uv [J,2], c [J] or None, cam -> t [3] in fp64, BEFORE the rounding to fp32 hides
    the error of the fit (the recovery tests), or None where there is no fit."""
    t, fit = _fit(np.asarray(w)[None, None, None, None], np.asarray(uv)[None, None], None if c is None else np.asarray(c)[None, None], cam)
    return t[0, 0, 0, 0] if fit.all() else None


def reproj_error(wb, t, x2d, cam):
    """The fp32 reprojection error of pose_partials_kernel, one rounded operation after the other: wb [B,T,P,F,J,3],
    t [B,T,P,F,3] fp32 (the root), x2d [B,F,J,2], cam [9] -> e2 [B,T,P,F,J] fp32."""
    f = np.float32
    wb, t, x2d = np.asarray(wb, dtype=f), np.asarray(t, dtype=f), np.asarray(x2d, dtype=f)
    fx, fy, cx, cy, k1, k2, k3, p1, p2 = (f(v) for v in np.asarray(cam, dtype=f).reshape(-1)[:9])
    with np.errstate(all="ignore"):
        X, Y, Z = (wb[..., k] + t[..., None, k] for k in range(3))
        xx = np.minimum(np.maximum(X / Z, f(-1)), f(1))
        yy = np.minimum(np.maximum(Y / Z, f(-1)), f(1))
        r2 = xx * xx + yy * yy
        radial = f(1) + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2))
        tan = p1 * xx + p2 * yy
        u = fx * (xx * (radial + tan) + p1 * r2) + cx
        v = fy * (yy * (radial + tan) + p2 * r2) + cy
        q0, q1 = u - x2d[:, None, None, :, :, 0], v - x2d[:, None, None, :, :, 1]
        return np.sqrt(q0 * q0 + q1 * q1).astype(f)


def pick(wb, x2d, conf, cam, h0=0):
    """The fit and the pick of one shard: -> dict tfit [B,T,P,F,3], e2 [B,T,F,J], idx [B,T,F,J] int32 (global: h0 + h),
    sel [B,T,F,J,3]; (+inf, -1, NaN) where a joint has no candidate."""
    wb = np.asarray(wb, dtype=np.float32)
    B, T, P, F, J, _ = wb.shape
    t = fit_roots(wb, x2d, conf, cam)
    e2 = reproj_error(wb, t, x2d, cam)                               # NaN where there is no fit: never a minimum
    pos = np.ones((B, F, J), dtype=bool) if conf is None else np.asarray(conf, dtype=np.float32) > 0
    best = np.full((B, T, F, J), np.inf, dtype=np.float32)
    idx = np.full((B, T, F, J), -1, dtype=np.int32)
    sel = np.full((B, T, F, J, 3), np.nan, dtype=np.float32)
    for h in range(P):
        better = (e2[:, :, h] < best) & pos[:, None]                 # strict: the first minimum wins
        best = np.where(better, e2[:, :, h], best)
        idx = np.where(better, np.int32(h0 + h), idx)
        sel = np.where(better[..., None], wb[:, :, h], sel)
    return {"tfit": t, "e2": best, "idx": idx, "sel": sel}

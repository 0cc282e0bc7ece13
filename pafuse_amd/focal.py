"""The focal length of a video's camera, estimated from the per-frame pose and its detections - the
host statement, in numpy, of what frames_focal_sums_kernel and focal_solve_kernel (csrc/kernels.hpp; pafuse_frames_focal_sums,
pafuse_focal_solve) compute.

Unknown are ONE focal length f for the whole video and the root (tx, ty, tz) of every (t, frame).  Known are the principal point
cx, cy = cam[2:4] and the pixel aspect rho = cam[1] / cam[0] - only the RATIO of cam[0:2] is read: cam and cam with fx, fy doubled
give the same bits.  For joint j with the root-relative pose (X, Y, Z) (fp32, whole-body), its screen-normalised detection (u, v)
and weight c, everything in fp64,

  p = u - cx        q = (v - cy) / rho        hx = p*Z        hy = q*Z

With phi = 1/f and gamma = phi*tz the pinhole is LINEAR in (phi; tx, ty, gamma):

  X + tx = phi*hx + gamma*p        Y + ty = phi*hy + gamma*q

g = (X, Y) is the observation and h = (hx, hy) the regressor.  The per-frame nuisance directions e_x, e_y and (p, q) are projected
out of both with the weights c (the roots are eliminated, not estimated), and what is left of h is regressed ON g:
f = sum K / sum H, the errors-in-variables direction.  The other one, sum H / sum G, divides by the energy of the noisy pose and
collapses with pose noise (tests/test_focal_host.py pins the choice).

Per (t, frame): thirteen sums over the joints that take part - weight > 0 and the three components of the pose finite, the rule of
pafuse_amd.trajectory - each in rootfit.SUM_ORDER, every product rounded before it is added (no fused multiply-add), the
parentheses the order of the operations:

  W   = sum c        Sp  = sum c*p        Sq = sum c*q              Spp = sum c*(p*p + q*q)
  gx  = sum c*X      gy  = sum c*Y        gp = sum c*(p*X + q*Y)    gg  = sum c*(X*X + Y*Y)
  hxs = sum c*hx     hys = sum c*hy       hp = sum c*(p*hx + q*hy)  hh  = sum c*(hx*hx + hy*hy)      hg = sum c*(hx*X + hy*Y)
  den = Spp - (Sp*Sp + Sq*Sq)/W
  rg  = gp - (Sp*gx + Sq*gy)/W            rh = hp - (Sp*hxs + Sq*hys)/W
  K   = (hh - (hxs*hxs + hys*hys)/W) - (rh*rh)/den          <h_perp, h_perp>
  H   = (hg - (hxs*gx + hys*gy)/W) - (rh*rg)/den            <h_perp, g_perp>
  G   = (gg - (gx*gx + gy*gy)/W) - (rg*rg)/den              <g_perp, g_perp>

A frame takes part if at least 4 joints are in the sums (three nuisance directions and the focal length), den is finite and > 0,
and K, H, G are finite.  Its state row is (K, H, G, 1.0), otherwise (0, 0, 0, 0): the state is double [T,N,4], and the states of
several videos of one camera concatenate along N.

The solve, per t.  The four slots are summed over n in the order of pafuse_frame_errors_reduce - rootfit.lane_sum along the frames:
lane l adds frames l, l + 64, ... in ascending order, then the butterfly.  There is an estimate if the count is >= 1, K > 0 and
H > 0:

  focal = K/H  and  r2 = (H*H)/(G*K),  each rounded once to fp32        (otherwise both NaN)
  frames  = the count, int32
  cam_out = (focal, rho*(K/H) in fp64 rounded once to fp32, cam[2], cam[3], ...)     NaN in the first two slots without an estimate

r2 is the fraction of the perspective signal h_perp that the line explains: 1 on exact data, small where the person is far away
or the pose is noisy.  It is a diagnostic, not a confidence interval.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

from . import rootfit

MIN_JOINTS = 4


def focal_sums(pose, x2d, conf, cam):
    """pose [T,N,J,3] fp32 whole-body, root-relative; x2d [N,J,2] fp32 screen-normalised; conf [N,J] fp32 or None; cam [>= 4]
    -> state [T,N,4] float64: what pafuse_frames_focal_sums writes."""
    pose = np.asarray(pose, dtype=np.float32)
    x2d = np.asarray(x2d, dtype=np.float32)
    cam = np.asarray(cam, dtype=np.float32).reshape(-1)
    T, N, J, _ = pose.shape
    assert pose.shape == (T, N, J, 3) and x2d.shape == (N, J, 2) and cam.size >= 4
    c32 = np.ones((N, J), dtype=np.float32) if conf is None else np.asarray(conf, dtype=np.float32)
    assert c32.shape == (N, J)
    lane_sum = rootfit.lane_sum
    with np.errstate(all="ignore"):
        on = (c32 > 0)[None] & np.isfinite(pose).all(axis=-1)          # [T,N,J]; False for a NaN weight
        rho = np.float64(cam[1]) / np.float64(cam[0])
        cx, cy = np.float64(cam[2]), np.float64(cam[3])
        c = np.broadcast_to(c32.astype(np.float64), (T, N, J))
        p = np.broadcast_to(x2d[..., 0].astype(np.float64) - cx, (T, N, J))
        q = np.broadcast_to((x2d[..., 1].astype(np.float64) - cy) / rho, (T, N, J))
        w = pose.astype(np.float64)
        X, Y, Z = w[..., 0], w[..., 1], w[..., 2]
        hx, hy = p * Z, q * Z
        S = lambda v: lane_sum(np.where(on, v, 0.0))
        W, Sp, Sq, Spp = S(c), S(c * p), S(c * q), S(c * (p * p + q * q))
        gx, gy, gp, gg = S(c * X), S(c * Y), S(c * (p * X + q * Y)), S(c * (X * X + Y * Y))
        hxs, hys, hp = S(c * hx), S(c * hy), S(c * (p * hx + q * hy))
        hh, hg = S(c * (hx * hx + hy * hy)), S(c * (hx * X + hy * Y))
        den = Spp - (Sp * Sp + Sq * Sq) / W
        rg = gp - (Sp * gx + Sq * gy) / W
        rh = hp - (Sp * hxs + Sq * hys) / W
        K = (hh - (hxs * hxs + hys * hys) / W) - (rh * rh) / den
        H = (hg - (hxs * gx + hys * gy) / W) - (rh * rg) / den
        G = (gg - (gx * gx + gy * gy) / W) - (rg * rg) / den
        part = (on.sum(axis=-1) >= MIN_JOINTS) & np.isfinite(den) & (den > 0) & np.isfinite(K) & np.isfinite(H) & np.isfinite(G)
        state = np.stack([K, H, G, np.ones_like(K)], axis=-1)
    return np.where(part[..., None], state, 0.0)


def totals(state):
    """state [T,N,4] -> [T,4]: K, H, G and the frame count summed over the frames in the order of the solve"""
    state = np.asarray(state, dtype=np.float64)
    assert state.ndim == 3 and state.shape[-1] == 4
    return rootfit.lane_sum(np.moveaxis(state, 1, -1))


def focal_solve(state, cam):
    """state [T,N,4] float64, cam [4 .. 9] fp32 -> (focal [T] fp32, r2 [T] fp32, frames [T] int32, cam_out [T,len(cam)] fp32):
    what pafuse_focal_solve writes."""
    cam = np.asarray(cam, dtype=np.float32).reshape(-1)
    assert 4 <= cam.size <= 9
    tot = totals(state)
    K, H, G, cnt = (tot[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        rho = np.float64(cam[1]) / np.float64(cam[0])
        ok = (cnt >= 1) & (K > 0) & (H > 0)
        f64 = K / H
        nan = np.float32(np.nan)
        focal = np.where(ok, f64.astype(np.float32), nan)
        r2 = np.where(ok, ((H * H) / (G * K)).astype(np.float32), nan)
        fy = np.where(ok, (rho * f64).astype(np.float32), nan)
    cam_out = np.broadcast_to(cam, (tot.shape[0], cam.size)).copy()
    cam_out[:, 0], cam_out[:, 1] = focal, fy
    return focal.astype(np.float32), r2.astype(np.float32), cnt.astype(np.int32), cam_out

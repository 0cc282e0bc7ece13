"""Repair of missing 2-D detections before lifting - the host statement, in numpy, of what
detections_repair_kernel (csrc/kernels.hpp; pafuse_detections_repair) computes, and the helpers that plant dropouts into clean
detections and measure what the repair makes of them.

A detector that loses a keypoint writes (0, 0) with confidence 0 (OpenPifPaf's "not found").  Unrepaired, that point enters the
denoisers as the image corner.  The repair fills it along the frames with the confidence-weighted local-linear filter of
pafuse_amd.trajectory.smooth, per joint, from the OBSERVED frames within `radius`; observed detections pass through untouched.

  observed(n, j)   conf[n,j] > threshold and both coordinates finite (a NaN confidence is not observed)

Levels.  `anchor` [J] names, for a joint that hangs on another (a finger on its wrist, a face point on the nose), that other
joint; -1 for a joint that hangs on nothing.  Joint j is LEVEL 1 iff 0 <= anchor[j] < J and anchor[anchor[j]] < 0; every other
joint is LEVEL 0 - anchor[j] < 0, out of range, anchored on itself or on an anchored joint, and anchor=None.  (The rule reads
anchor[anchor[j]] only for an in-range anchor[j]: no table can cause a read out of bounds.)

Level 0, a missing (n, j): the frames m = max(0, n - r) .. min(N - 1, n + r) are walked in ascending order, d = m - n, all in
fp64, no fused multiply-add; a frame takes part if observed(m, j):

  q = double(d*d) / double((r+1)*(r+1));  h = 1.0 - q;  g = h*h            the biweight taper of the smoother
  omega = g * double(conf[m,j])
  S0 = sum omega;  S1 = sum omega*d;  S2 = sum (omega*d)*d;  per coordinate  Q0 = sum omega*y;  Q1 = sum (omega*d)*y
  D = S0*S2 - S1*S1
  two frames or more and D finite and > 0:   (S2*Q0 - S1*Q1)/D     the local line's value at d = 0      status 1, filled
  else S0 > 0:                               Q0/S0                                                      status 2, held
  else:                                                                                                 status 3, unfilled

with y = double(x2d[m,j]).  The value is rounded once to fp32; a value that is not finite in fp32 is status 3.  Status 3 keeps
the input's bits: the repair never makes an input worse than it is and creates no NaN.  An observed joint is status 0 and keeps
its bits.

Level 1, with a = anchor[j]: the same steps on y[m] = double(x2d[m,j]) - double(out[m,a]), out[., a] being level 0's finished
output.  A frame takes part if observed(m, j) and status[m,a] != 3; the target needs status[n,a] != 3, otherwise the joint is
status 3; the value is float(double(out[n,a]) + line).  So a hand lost for five frames moves with its wrist.

conf_out = conf where status is 0 and 0 elsewhere: a filled joint carries no measurement, and the root fit, the focal estimate and
the reprojection pick go on ignoring it.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

from .trajectory import LINE, MEAN, NONE, local_line      # the smoother's filter: x2d [N,J,2] has its frames on axis 0 already

OBSERVED, FILLED, HELD, UNFILLED = 0, LINE, MEAN, NONE
STATUS_NAMES = ("observed", "filled", "held", "unfilled")
DROPPED_XY = (-1.0, -1.0)      # what a planted dropout holds: about what pixel (0, 0) normalises to on the H3WB cameras


def levels(anchor, J):
    """anchor [J] int or None -> bool [J]: True for the level-1 joints (the rule above)"""
    if anchor is None:
        return np.zeros(J, dtype=bool)
    a = np.asarray(anchor).astype(np.int64).reshape(-1)
    assert a.shape == (J,)
    inside = (a >= 0) & (a < J)
    return inside & (a[np.where(inside, a, 0)] < 0)


def check_anchor(anchor, J):
    """the table as the Python layers take it: int [J], every entry negative (level 0) or a level-1 entry - an entry that the
    level rule would demote silently (out of range, anchored on itself or on an anchored joint) is a ValueError.  -> int32 [J]"""
    a = np.asarray(anchor)
    if a.ndim != 1 or a.shape[0] != J or a.dtype.kind not in "iu":
        raise ValueError(f"anchor must be an integer table [J] = [{J}], got {a.dtype} {tuple(a.shape)}")
    a = a.astype(np.int64)
    bad = np.nonzero((a >= 0) & ~levels(a, J))[0]
    if bad.size:
        j = int(bad[0])
        raise ValueError(f"anchor[{j}] = {int(a[j])} is out of range, the joint itself or an anchored joint (one anchor level only): "
                         f"the repair would treat joint {j} as unanchored")
    return a.astype(np.int32)


def repair(x2d, conf, anchor=None, radius=13, threshold=0.0):
    """x2d [N,J,2] fp32, conf [N,J] fp32, anchor [J] int or None, radius 1 .. 64, threshold >= 0 ->
    (out [N,J,2] fp32, conf_out [N,J] fp32, status [N,J] uint8): what pafuse_detections_repair writes, one rounded operation
    after the other."""
    x2d = np.asarray(x2d, dtype=np.float32)
    conf = np.asarray(conf, dtype=np.float32)
    N, J, _ = x2d.shape
    r = int(radius)
    if not 1 <= r <= 64:
        raise ValueError(f"repair: radius must lie in 1 .. 64, got {radius!r}")
    thr = np.float32(threshold)
    if not (np.isfinite(thr) and thr >= 0):
        raise ValueError(f"repair: threshold must be finite and >= 0, got {threshold!r}")
    assert x2d.shape == (N, J, 2) and conf.shape == (N, J) and N >= 1 and J >= 1
    lvl1 = levels(anchor, J)
    out = x2d.copy()
    status = np.zeros((N, J), dtype=np.uint8)
    with np.errstate(all="ignore"):
        observed = (conf > thr) & np.isfinite(x2d).all(axis=-1)          # False for a NaN confidence
        x64, w64 = x2d.astype(np.float64), conf.astype(np.float64)

        def settle(cols, value32, code, able):
            """write the missing joints of the columns `cols`: the value where there is one and it is finite, status 3 otherwise"""
            miss = ~observed[:, cols]
            code = np.where(able & np.isfinite(value32).all(axis=-1), code, UNFILLED).astype(np.uint8)
            st = np.where(miss, code, OBSERVED).astype(np.uint8)
            write = miss & (st != UNFILLED)
            out[:, cols] = np.where(write[..., None], value32, x2d[:, cols])
            status[:, cols] = st

        j0 = np.nonzero(~lvl1)[0]
        value, code = local_line(x64[:, j0], observed[:, j0], w64[:, j0], r)
        settle(j0, value.astype(np.float32), code, np.ones((N, j0.size), dtype=bool))
        j1 = np.nonzero(lvl1)[0]
        if j1.size:
            a = np.asarray(anchor).astype(np.int64)[j1]
            base = out[:, a].astype(np.float64)                          # level 0's finished output
            able = status[:, a] != UNFILLED
            value, code = local_line(x64[:, j1] - base, observed[:, j1] & able, w64[:, j1], r)
            settle(j1, (base + value).astype(np.float32), code, able)
    conf_out = np.where(status == OBSERVED, conf, np.float32(0)).astype(np.float32)
    return out, conf_out, status


def counts(status):
    """status [N,J] -> int64 [4]: the joints observed, filled, held and unfilled"""
    return np.bincount(np.asarray(status, dtype=np.uint8).reshape(-1), minlength=4)[:4].astype(np.int64)


def repair_anchors(dataset):
    """The anchor table of a whole-body dataset, int32 [J]: -1 for the joints of parts_joint_indices["body"]; for every other
    part (face, left hand, right hand) the joint the part hangs on, parts_connection_indices[part] - the nose for the face,
    the wrists for the hands."""
    J = sum(len(idx) for idx in dataset.parts_joint_indices.values())
    anchor = np.full(J, -1, dtype=np.int32)
    for part, idx in dataset.parts_joint_indices.items():
        if part != "body":
            anchor[np.asarray(list(idx), dtype=np.int64)] = int(dataset.parts_connection_indices[part])
    return anchor


def plant_dropouts(N, J, rate, run, seed):
    """-> bool [N,J], True where a detection is to be lost: at every (n, j) a run of `run` frames starts with probability
    rate / run (np.random.default_rng(seed)), clipped at the end of the video; overlapping runs merge, so the lost share is a
    little below `rate`."""
    N, J, run = int(N), int(J), int(run)
    if N < 1 or J < 1 or run < 1 or not 0.0 <= float(rate) <= run:
        raise ValueError(f"plant_dropouts: N, J, run >= 1 and 0 <= rate <= run, got {(N, J, rate, run)!r}")
    start = np.random.default_rng(seed).random((N, J)) < float(rate) / run
    lost = np.zeros((N, J), dtype=bool)
    for k in range(min(run, N)):
        lost[k:] |= start[:N - k]
    return lost


def drop(x2d, lost):
    """x2d [N,J,2] with the planted dropouts `lost` [N,J] -> (x2d with DROPPED_XY there, conf: 0 there, else 1), fp32"""
    x = np.array(x2d, dtype=np.float32, copy=True)
    lost = np.asarray(lost, dtype=bool)
    x[lost] = np.asarray(DROPPED_XY, dtype=np.float32)
    return x, np.where(lost, np.float32(0), np.float32(1)).astype(np.float32)


def repair_error(x_true, x_out, lost, status, parts=None):
    """How far the repaired detections are from the truth at the joints that were lost: x_true, x_out [N,J,2], lost [N,J]
    bool, status [N,J] -> {"filled": RMS 2-D distance over the lost joints at status 1 or 2, "unfilled": over those at status
    3, "n_filled", "n_unfilled"}; with `parts` ({name: joint indices}) also "parts": {name: the same four}.  NaN where
    nothing was counted.  Needs no checkpoint."""
    x_true, x_out = np.asarray(x_true, dtype=np.float64), np.asarray(x_out, dtype=np.float64)
    lost, status = np.asarray(lost, dtype=bool), np.asarray(status)
    d2 = ((x_out - x_true) ** 2).sum(axis=-1)

    def rms(sel):
        k = int(sel.sum())
        return (float(np.sqrt(d2[sel].mean())) if k else float("nan")), k

    def over(cols):
        sel = np.zeros_like(lost)
        sel[:, cols] = lost[:, cols]
        f, nf = rms(sel & (status != UNFILLED))
        u, nu = rms(sel & (status == UNFILLED))
        return {"filled": f, "unfilled": u, "n_filled": nf, "n_unfilled": nu}

    res = over(np.arange(lost.shape[1]))
    if parts is not None:
        res["parts"] = {name: over(np.asarray(list(idx), dtype=np.int64)) for name, idx in parts.items()}
    return res

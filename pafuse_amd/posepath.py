"""J-Agg coherent in time - the host statement, in numpy, of what pose_path_kernel (csrc/kernels.hpp,
pafuse_pose_path) computes: the recursion path_forward / path_backtrace on the candidates of a clip.

J-Agg picks, per joint and per frame, the hypothesis whose reprojection is closest to the detection; every frame on its
own, so the winner changes on sub-pixel differences of e2 and the joint jumps between hypotheses centimetres apart.  Here
one line (b, t, j) of a clip chooses a PATH h(f) through its P hypotheses that minimises the reprojection error plus a
penalty for jumping - a Viterbi recursion along the frames, everything in fp64, every product rounded before it is added
(the kernel pins contraction off), np.sqrt and the kernel's sqrt both correctly rounded.

Operands of one line: e2 [P,F] fp32 unary costs, off [P,F,3] offsets, lam >= 0 a double.

Availability and observation.  Hypothesis h is AVAILABLE at frame f if its three offsets are finite.  A frame is OBSERVED
if at least one available hypothesis has a finite e2.  The unary cost u_f(h) at an observed frame is (double)e2, +inf for a
non-finite e2 or an unavailable hypothesis; at an unobserved frame (a NaN detection, a confidence not > 0: `unary` gives
+inf there) it is 0 for every available hypothesis and +inf for the others - the joint is carried through the gap by
smoothness alone.  If some frame has no available hypothesis, or no frame is observed, the line has no path: idx -1 at all
its frames and a NaN total.

Transition.  From h' at f - 1 to h at f:  lam * sqrt((dx*dx + dy*dy) + dz*dz),  d = off[h,f] - off[h',f-1], in this order.

Recursion.  c_0 = u_0;  c_f(h) = u_f(h) + min_h' (c_f-1(h') + transition), the minimum being the FIRST in ascending h' under
strict < starting from +inf with back-pointer 0 (a NaN - an unavailable h' - never wins).  After every frame
m_f = min_h c_f(h) is subtracted from all c_f and added to total.  The subtraction is part of the statement, not an
optimisation: with lam == 0 the minimum of the previous costs is an exact 0, c_f(h) == u_f(h) exactly, and the path is
J-Agg's first minimum frame by frame whatever the magnitudes are; and it keeps the resolution of the costs at F = 243.

Backtrace.  From the first minimum of the last frame's costs along the back-pointers.  Outputs: idx [F], total.

Offsets.  off = (double)w - (double)mean, w the fp32 whole-body joint of the hypothesis (rootfit.whole_body) and mean the
fp32 P-Agg pose of the same (b, t, f, j) as pafuse_pose_combine writes it; mean=None: absolute offsets.  Subtracting the
mean removes the motion all hypotheses share: staying on a hypothesis that moves like the mean costs nothing, and real
motion is not penalised.

The weight.  lam has the unit of normalised screen length per metre.  fx / Z (cam[0] over the depth of the subject) is the
weight at which a jump costs as much as its own projection onto the screen.  The library chooses no default.

What this is not: `path` / `pick` work per clip and cross neither clip seams nor pooled windows, and it is not a smoother of
the pose values - every returned joint is still some hypothesis's joint.

The path of a whole VIDEO (frames_path_kernel, pafuse_frames_path: the same device recursion) is the
same statement on more candidates: at video frame n the candidates are the pairs (window, hypothesis) of ALL windows that cover n.  Number them
g = w * P + h and give a window that does not cover a frame NaN offsets - unavailable -: `path` on that dense [W*P, N] array
(frames_dense) is the wanted recursion along the N frames.  An unavailable candidate never wins under strict <, and ties
go to the lower (w, h): the order in which the fold of the windows (windows.fold_pose) keeps its candidate, so weight 0 is
the pooled per-frame pick.  frames_path does that per line (t, j) and takes the offsets against the pooled per-frame mean.
Its limits: A LINE DIES WHOLE - one frame at which no candidate is available, or a line that is never observed, has no
path at any frame of the video; segments that restart are not built -, the dense form and the device's workspace grow with
the length of the video, and it still is no smoother of the pose values.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import itertools

import numpy as np

from . import rootfit


def unary(wb, root, x2d, cam, conf=None):
    """e2 of every (hypothesis, frame, joint) by rootfit.reproj_error (the fp32 expression of the kernels' reproj_error, one
    rounded operation after the other): wb [B,T,P,F,J,3] fp32 whole-body hypotheses, root [B,F,3] (one trajectory) or
    [B,T,P,F,3] (one root per hypothesis: tfit), x2d [B,F,J,2], cam [9], conf [B,F,J] or None -> e2 [B,T,P,F,J] fp32, +inf
    where the confidence is not > 0."""
    wb = np.asarray(wb, dtype=np.float32)
    B, T, P, F, J, _ = wb.shape
    root = np.asarray(root, dtype=np.float32)
    if root.size == B * F * 3:
        root = np.broadcast_to(root.reshape(B, 1, 1, F, 3), (B, T, P, F, 3))
    assert root.shape == (B, T, P, F, 3)
    e2 = rootfit.reproj_error(wb, root, x2d, cam)
    return gate(e2, conf)


def gate(e2, conf):
    """e2 [B,T,P,F,J] with +inf where conf [B,F,J] is not > 0 (None: unchanged)"""
    if conf is None:
        return e2
    seen = np.asarray(conf, dtype=np.float32) > 0                      # False for NaN
    return np.where(seen[:, None, None], e2, np.float32(np.inf)).astype(np.float32)


def offsets(wb, mean=None):
    """wb [B,T,P,F,J,3] fp32, mean [B,T,F,J,3] fp32 or None -> off [B,T,P,F,J,3] fp64 = (double)w - (double)mean"""
    w = np.asarray(wb, dtype=np.float32).astype(np.float64)
    if mean is None:
        return w
    with np.errstate(all="ignore"):
        return w - np.asarray(mean, dtype=np.float32).astype(np.float64)[:, :, None]


def transition(a, b, lam):
    """lam * |a - b| for offsets a (at f), b (at f - 1) [...,3] fp64, in the statement's order of operations"""
    with np.errstate(all="ignore"):
        d = a - b
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return np.float64(lam) * np.sqrt((dx * dx + dy * dy) + dz * dz)


def path(e2, off, lam):
    """The statement for any number of lines at once: e2 [...,P,F] fp32, off [...,P,F,3], lam >= 0 ->
    (idx [...,F] int32, total [...] fp64); a line without a path: -1 throughout and NaN."""
    e2 = np.asarray(e2, dtype=np.float32)
    off = np.asarray(off).astype(np.float64)
    lam = float(lam)
    assert lam >= 0 and np.isfinite(lam) and off.shape == e2.shape + (3,)
    lead, (P, F) = e2.shape[:-2], e2.shape[-2:]
    e2 = e2.reshape((-1, P, F))
    off = off.reshape((-1, P, F, 3))
    L = e2.shape[0]
    inf = np.float64(np.inf)
    with np.errstate(all="ignore"):
        avail = np.isfinite(off).all(axis=-1)                          # [L,P,F]
        fin = avail & np.isfinite(e2)
        observed = fin.any(axis=1)                                     # [L,F]
        alive = avail.any(axis=1).all(axis=1) & observed.any(axis=1)   # [L]
        u = np.where(observed[:, None], np.where(fin, e2.astype(np.float64), inf), np.where(avail, 0.0, inf))
        back = np.zeros((L, F, P), dtype=np.int64)
        total = np.zeros(L)
        c = u[:, :, 0].copy()
        some = avail.any(axis=0)                                       # [P,F]: available on any line at all
        for f in range(F):
            if f:
                best = np.full((L, P), inf)
                # an h or h' that no line has available gives NaN transitions only, and a NaN never wins: leaving those
                # columns and rounds out changes no bit (frames_path's dense form is mostly such candidates)
                cols = np.flatnonzero(some[:, f])
                for hp in np.flatnonzero(some[:, f - 1]):
                    v = c[:, hp, None] + transition(off[:, cols, f], off[:, hp, None, f - 1], lam)
                    better = v < best[:, cols]                         # strict: the first minimum wins, a NaN never
                    best[:, cols] = np.where(better, v, best[:, cols])
                    back[:, f, cols] = np.where(better, hp, back[:, f, cols])
                c = u[:, :, f] + best
            m = np.min(np.where(np.isnan(c), inf, c), axis=1)
            total = total + m
            c = c - m[:, None]
        idx = np.full((L, F), -1, dtype=np.int32)
        h = np.argmin(np.where(np.isnan(c), inf, c), axis=1)           # argmin returns the first minimum
        rows = np.arange(L)
        for f in range(F - 1, -1, -1):
            idx[:, f] = h
            h = back[rows, f, h]
    idx[~alive] = -1
    total[~alive] = np.nan
    return idx.reshape(lead + (F,)), total.reshape(lead)


def lines(x):
    """[B,T,P,F,J,...] -> [B,T,J,P,F,...]: the hypotheses and frames of every line (b, t, j) last, as `path` takes them"""
    return np.moveaxis(np.asarray(x), 4, 2)


def pick(wb, e2, lam, mean=None):
    """The path of every line of a batch: wb [B,T,P,F,J,3], e2 [B,T,P,F,J] (unary), mean [B,T,F,J,3] or None ->
    dict idx [B,T,F,J] int32, cost [B,T,J] fp64, pick [B,T,F,J,3] fp32 and e2 [B,T,F,J] fp32 (the chosen hypothesis's joint
    and e2; +inf at an unobserved frame; NaN / +inf where there is no path)."""
    wb = np.asarray(wb, dtype=np.float32)
    e2 = np.asarray(e2, dtype=np.float32)
    off = offsets(wb, mean)
    idx, cost = path(lines(e2), lines(off), lam)                       # [B,T,J,F], [B,T,J]
    idx = np.ascontiguousarray(np.moveaxis(idx, 2, 3))                 # [B,T,F,J]
    at = np.maximum(idx, 0).astype(np.int64)[:, :, None]
    sel = np.take_along_axis(wb, at[..., None], axis=2)[:, :, 0]
    with np.errstate(all="ignore"):
        fin = np.isfinite(off).all(axis=-1) & np.isfinite(e2)
    observed = fin.any(axis=2)                                         # [B,T,F,J]
    e2_at = np.where(observed, np.take_along_axis(e2, at, axis=2)[:, :, 0], np.float32(np.inf))
    none = idx < 0
    sel = np.where(none[..., None], np.float32(np.nan), sel).astype(np.float32)
    e2_at = np.where(none, np.float32(np.inf), e2_at).astype(np.float32)
    return {"idx": idx, "cost": cost, "pick": sel, "e2": e2_at}


def path_cost(e2, off, lam, idx):
    """The cost of path idx [F] of ONE line, added up plainly (no normalisation): sum of the unary costs along it plus
    lam times the jumps; e2 [P,F], off [P,F,3].  Exact where every term is (the brute-force tests)."""
    e2 = np.asarray(e2, dtype=np.float32)
    off = np.asarray(off).astype(np.float64)
    P, F = e2.shape
    with np.errstate(all="ignore"):
        avail = np.isfinite(off).all(axis=-1)
        fin = avail & np.isfinite(e2)
        observed = fin.any(axis=0)
        u = np.where(observed[None], np.where(fin, e2.astype(np.float64), np.inf), np.where(avail, 0.0, np.inf))
        total = np.float64(0.0)
        for f in range(F):
            total = total + u[idx[f], f]
            if f:
                total = total + transition(off[idx[f], f], off[idx[f - 1], f - 1], lam)
    return total


def brute_force(e2, off, lam):
    """The minimum of path_cost over all P**F paths of one tiny line -> (cost, a path that attains it).  Ties between paths
    are broken differently from the recursion: compare the costs, not the paths.  A path through an unavailable hypothesis
    costs +inf or NaN and never is the minimum, so only the available ones of every frame are walked (the dense form of
    frames_path is mostly unavailable candidates)."""
    P, F = np.asarray(e2).shape
    best, arg = np.inf, None
    with np.errstate(all="ignore"):
        avail = np.isfinite(np.asarray(off).astype(np.float64)).all(axis=-1)
    for hs in itertools.product(*(np.flatnonzero(avail[:, f]).tolist() for f in range(F))):
        v = path_cost(e2, off, lam, hs)
        if v < best:
            best, arg = v, hs
    return best, arg


# --------------------------------------------------------------------------------- the path of a whole video (section 6l)
def frames_dense(e2, wb, mean, starts, valid, N):
    """The candidates of a video in dense form.  e2 [W,T,P,F,J] fp32 (gated), wb [W,T,P,F,J,3] fp32: the hypotheses of the W
    windows of one video, window w covering the frames [starts[w], starts[w] + valid[w]); mean [T,N,J,3] fp32 or None.
    Candidate g = w * P + h.  -> (e2 [T,J,W*P,N] fp32, off [T,J,W*P,N,3] fp64): off = (double)w - (double)mean[t,n,j] where
    window w covers frame n, NaN - unavailable - elsewhere (the padding f >= valid[w] of a short video included)."""
    e2 = np.asarray(e2, dtype=np.float32)
    wb = np.asarray(wb, dtype=np.float32)
    W, T, P, F, J = e2.shape
    N = int(N)
    assert wb.shape == (W, T, P, F, J, 3) and len(starts) == W and len(valid) == W
    m = np.zeros((T, N, J, 3)) if mean is None else np.asarray(mean, dtype=np.float32).astype(np.float64)
    assert m.shape == (T, N, J, 3)
    de = np.full((T, J, W * P, N), np.nan, dtype=np.float32)
    do = np.full((T, J, W * P, N, 3), np.nan)
    for w in range(W):
        s, v = int(starts[w]), int(valid[w])
        assert 1 <= v <= F and 0 <= s and s + v <= N
        de[:, :, w * P:(w + 1) * P, s:s + v] = e2[w, :, :, :v].transpose(0, 3, 1, 2)                      # [T,J,P,v]
        with np.errstate(all="ignore"):
            do[:, :, w * P:(w + 1) * P, s:s + v] = (wb[w, :, :, :v].astype(np.float64).transpose(0, 3, 1, 2, 4)
                                                    - m[:, s:s + v].transpose(0, 2, 1, 3)[:, :, None])    # [T,J,P,v,3]
    return de, do


def frames_path(e2, wb, mean, starts, valid, N, lam):
    """The path of every line (t, j) of a VIDEO: at frame n the candidates are the pairs (window, hypothesis) of all windows
    that cover n, and `path` runs on their dense form (frames_dense) along the N frames - an unavailable candidate never
    wins, ties go to the lower (window, hypothesis).  e2 [W,T,P,F,J] fp32 unary (gated), wb [W,T,P,F,J,3] fp32, mean
    [T,N,J,3] fp32 as the pooled finish writes it (None: absolute offsets), starts / valid as windows.window_starts gives them.
    -> dict idx [T,N,J] int32 (the hypothesis), window [T,N,J] int32, pick [T,N,J,3] fp32, e2 [T,N,J] fp32 (+inf at an
    unobserved frame), cost [T,J] fp64; -1 / -1 / NaN / +inf / NaN on a line without a path - one frame without an
    available candidate, or no observed frame at all, removes the path of the line at EVERY frame."""
    e2 = np.asarray(e2, dtype=np.float32)
    wb = np.asarray(wb, dtype=np.float32)
    W, T, P, F, J = e2.shape
    N = int(N)
    de, do = frames_dense(e2, wb, mean, starts, valid, N)
    g, cost = path(de, do, lam)                                        # [T,J,N], [T,J]
    g = np.ascontiguousarray(np.moveaxis(g, 1, 2))                     # [T,N,J]
    none = g < 0
    at = np.maximum(g, 0).astype(np.int64)
    win, idx = at // P, at % P
    f = np.clip(np.arange(N)[None, :, None] - np.asarray(starts, dtype=np.int64)[win], 0, F - 1)
    tt, jj = np.arange(T)[:, None, None], np.arange(J)[None, None, :]
    sel = wb[win, tt, idx, f, jj]                                      # [T,N,J,3]
    e2_at = e2[win, tt, idx, f, jj]
    with np.errstate(all="ignore"):
        fin = np.isfinite(do).all(axis=-1) & np.isfinite(de)           # [T,J,G,N]
    observed = np.moveaxis(fin.any(axis=2), 1, 2)                      # [T,N,J]
    e2_at = np.where(observed & ~none, e2_at, np.float32(np.inf)).astype(np.float32)
    sel = np.where(none[..., None], np.float32(np.nan), sel).astype(np.float32)
    return {"idx": np.where(none, -1, idx).astype(np.int32), "window": np.where(none, -1, win).astype(np.int32),
            "pick": sel, "e2": e2_at, "cost": cost}

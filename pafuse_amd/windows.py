"""Overlapping windows pooled into one pose per video frame - the host statement, in numpy, of what
pose_windows_fold_kernel, spread_windows_fold_kernel and frames_finish_kernel (csrc/kernels.hpp; pafuse_pose_windows_fold,
pafuse_spread_windows_fold, pafuse_frames_finish) compute.

A seq2seq lifter sees F frames at a time.  Cut into consecutive clips (harness.cut_clips) a frame at a clip border has
temporal context on one side only; with a sliding window of stride s < F every frame is seen by about F/s windows at
different positions.  The hypotheses of one window are reduced on the device to a pose state (44 bytes per (b,t,f,j):
fp64 sums and the J-Agg candidate) and a spread state (72 bytes: fp64 sums and centred second moments); the fold maps
(window b, local frame f) to the global frame n = start_b + f and merges the row into a FRAME state with rows (t, n, j):

  pose     sum += state.sum                               one fp64 add per component and window
           count[n] += P                                  the hypotheses of the window
           if state.e2 < e2: (e2, idx, win, sel) = (state.e2, state.idx, w0 + b, state.sel)
                                                          strict: among equal errors the lowest window keeps the candidate,
                                                          and within it the lowest hypothesis (the state's first minimum)
  spread   Chan's pairwise rule, the operations of spread_combine_kernel in its order (na = count[n], nb = the window's):
           na == 0: the window's sums and moments go through as they are; else
           fac = na*nb/(na + nb);  dl = sum_b/nb - sum/na;  m2 = (m2 + m2_b) + dl (x) dl * fac;  sum += sum_b;  count[n] += nb

The windows that cover a frame are visited in ascending order, whether they arrive in one batch or in several: the frame
state does not depend on how the windows are batched.  The finish divides in fp64 and rounds once: mean = sum / count[n],
cov = m2 / count[n], std = sqrt(((m2_xx + m2_yy) + m2_zz) / count[n]); a frame no window covered is NaN.

Every product is rounded before it is added (numpy does not fuse; the kernels pin contraction off).

This module is test infrastructure and the documentation of the arithmetic.  The product path calls window_starts only.
"""
import numpy as np


def window_starts(N, frames, stride):
    """The windows of a video of N frames: -> (starts, valid), int32 [W] each.  starts = 0, s, 2s, ... while start + frames
    <= N, and one last window at N - frames if the last frame is not covered yet.  N < frames: one window at 0 with
    valid = N real frames (the clip is padded by repeating its last frame, as harness.cut_clips does; the padding is never
    folded); otherwise valid = frames throughout.  stride = frames gives exactly the clips of cut_clips."""
    N, F, s = int(N), int(frames), int(stride)
    if N < 1 or F < 1:
        raise ValueError(f"window_starts: N and frames must be positive, got {N}, {F}")
    if not 1 <= s <= F:
        raise ValueError(f"window_starts: stride must lie in 1 .. frames = {F}, got {stride!r}")
    if N < F:
        return np.zeros(1, dtype=np.int32), np.full(1, N, dtype=np.int32)
    starts = list(range(0, N - F + 1, s))
    if starts[-1] + F < N:
        starts.append(N - F)
    return np.asarray(starts, dtype=np.int32), np.full(len(starts), F, dtype=np.int32)


def coverage(N, starts, valid):
    """-> int64 [N]: the number of windows that cover every frame"""
    c = np.zeros(int(N), dtype=np.int64)
    for s, v in zip(starts, valid):
        c[int(s):int(s) + int(v)] += 1
    return c


def _check(N, F, starts, valid):
    starts, valid = np.asarray(starts, dtype=np.int64), np.asarray(valid, dtype=np.int64)
    if starts.shape != valid.shape or starts.ndim != 1:
        raise ValueError("windows: starts and valid are two vectors of one length")
    if ((valid < 1) | (valid > F)).any() or (starts < 0).any() or (starts + valid > N).any() or (np.diff(starts) <= 0).any():
        raise ValueError("windows: valid in 1 .. F, windows inside [0, N), starts strictly ascending")
    return starts, valid


def frame_pose_state(N, T, J):
    """the neutral frame pose state: zero sums and counts, no candidate (+inf, -1, -1, NaN NaN NaN)"""
    return {"sum": np.zeros((T, N, J, 3)), "e2": np.full((T, N, J), np.inf, dtype=np.float32),
            "idx": np.full((T, N, J), -1, dtype=np.int32), "win": np.full((T, N, J), -1, dtype=np.int32),
            "sel": np.full((T, N, J, 3), np.nan, dtype=np.float32), "count": np.zeros(N, dtype=np.int32)}


def frame_spread_state(N, T, J):
    """the neutral frame spread state: all zeros"""
    return {"sum": np.zeros((T, N, J, 3)), "m2": np.zeros((T, N, J, 6)), "count": np.zeros(N)}


def fold_pose(frame, state, starts, valid, w0, P_total):
    """Fold the pose state of B windows (sum [B,T,F,J,3] f64, e2 [B,T,F,J] f32, idx i32, sel [B,T,F,J,3] f32: the union
    of P_total hypotheses per window) into `frame` in place, window after window in ascending order; -> frame."""
    B, T, F, J = state["e2"].shape
    N = frame["count"].shape[0]
    starts, valid = _check(N, F, starts, valid)
    assert len(starts) == B and frame["e2"].shape == (T, N, J)
    for b in range(B):
        s, v = int(starts[b]), int(valid[b])
        at = slice(s, s + v)
        frame["sum"][:, at] += np.asarray(state["sum"], dtype=np.float64)[b, :, :v]
        frame["count"][at] += np.int32(P_total)
        e2 = np.asarray(state["e2"], dtype=np.float32)[b, :, :v]
        better = e2 < frame["e2"][:, at]
        frame["e2"][:, at] = np.where(better, e2, frame["e2"][:, at])
        frame["idx"][:, at] = np.where(better, state["idx"][b, :, :v], frame["idx"][:, at])
        frame["win"][:, at] = np.where(better, np.int32(int(w0) + b), frame["win"][:, at])
        frame["sel"][:, at] = np.where(better[..., None], state["sel"][b, :, :v], frame["sel"][:, at])
    return frame


PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # the order of m2 and cov: xx, xy, xz, yy, yz, zz


def fold_spread(frame, state, starts, valid):
    """Fold the spread state of B windows (sum [B,T,F,J,3], m2 [B,T,F,J,6], count: a scalar - every window holds as many
    hypotheses) into `frame` in place by Chan's rule, window after window in ascending order; -> frame."""
    B, T, F, J, _ = state["sum"].shape
    N = frame["count"].shape[0]
    starts, valid = _check(N, F, starts, valid)
    assert len(starts) == B
    nb = float(np.asarray(state["count"]).reshape(-1)[0])
    if nb == 0.0:
        return frame
    for b in range(B):
        s, v = int(starts[b]), int(valid[b])
        at = slice(s, s + v)
        sb, mb = np.asarray(state["sum"], dtype=np.float64)[b, :, :v], np.asarray(state["m2"], dtype=np.float64)[b, :, :v]
        na = frame["count"][at][None, :, None]                   # [1,v,1] against [T,v,J]
        first = np.broadcast_to(na == 0.0, sb.shape[:-1])
        with np.errstate(all="ignore"):
            fac = na * nb / (na + nb)
            dl = sb / nb - frame["sum"][:, at] / na[..., None]
            m = np.stack([(frame["m2"][:, at][..., k] + mb[..., k]) + dl[..., a] * dl[..., c] * fac
                          for k, (a, c) in enumerate(PAIRS)], axis=-1)
            sm = frame["sum"][:, at] + sb
        frame["m2"][:, at] = np.where(first[..., None], mb, m)
        frame["sum"][:, at] = np.where(first[..., None], sb, sm)
        frame["count"][at] += nb
    return frame


def finish(frame=None, spread=None):
    """-> dict: from a frame pose state "mean" [T,N,J,3] f32 (sum / count[n] in fp64, rounded once), "pick" [T,N,J,3],
    "idx", "window" [T,N,J]; from a frame spread state "std" [T,N,J] and "cov" [T,N,J,6] f32 (NaN where count is 0 or a sum
    or moment is not finite)."""
    out = {}
    with np.errstate(all="ignore"):
        if frame is not None:
            out["mean"] = (frame["sum"] / frame["count"].astype(np.float64)[None, :, None, None]).astype(np.float32)
            out["pick"], out["idx"], out["window"] = frame["sel"].copy(), frame["idx"].copy(), frame["win"].copy()
        if spread is not None:
            na = spread["count"][None, :, None]
            fine = (na > 0) & np.isfinite(spread["sum"]).all(-1) & np.isfinite(spread["m2"]).all(-1)
            m = spread["m2"]
            cov = (m / na[..., None]).astype(np.float32)
            std = np.sqrt(((m[..., 0] + m[..., 3]) + m[..., 5]) / na).astype(np.float32)
            out["cov"] = np.where(fine[..., None], cov, np.float32(np.nan))
            out["std"] = np.where(fine, std, np.float32(np.nan))
    return out

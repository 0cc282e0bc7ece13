"""People followed through a video - the host statement, in numpy, of what track_nodes_kernel,
track_links_kernel, track_path_kernel and track_gather_kernel (csrc/kernels.hpp; pafuse_tracks_links, pafuse_tracks_path,
pafuse_tracks_gather) compute, and the helpers that plant distractor people into a one-person video and count what the
tracker makes of them.

A detector lists the people of a frame in no stable order.  The tracker turns x2d [N,K,J,2] (screen-normalised, fp32) and
conf [N,K,J] (fp32) - K candidate detections per frame, an all-zero slot being "nobody" - into M per-person videos.  All
arithmetic is fp64, no fused multiply-add, every product rounded before it is added; every sum over the joints is
rootfit.lane_sum (SUM_ORDER).  Limits: K <= 64, max_gap G in 1 .. 8, tracks M in 1 .. 64.

Nodes.  Joint j of candidate (n, k) is OBSERVED iff conf > threshold and both coordinates are finite.  Over the observed
joints  size(n, k) = sqrt((xmax - xmin) * (ymax - ymin)).  The candidate is PRESENT iff it has at least `support` observed
joints and size is finite and > 0; size is NaN where it is absent.

Links.  a = (n - g, ka) and b = (n, kb), lag g = 1 .. G, both present, sharing c >= support observed joints:

  w_j = double(min(conf_a, conf_b)),  dx = double(xb) - double(xa), dy alike      over the common joints, every other term 0.0
  d = lane_sum(w * sqrt(dx*dx + dy*dy)) / lane_sum(w)
  cost = d / (0.5 * (size_a + size_b))            how far the person moved, in units of their own size
  gain[n, g, ka, kb] = (gate - cost) - skip * (g - 1)   iff cost <= gate (a NaN cost is not), else -inf

The cost is symmetric in a and b, bit for bit.  A link that reaches in front of frame 0 is -inf.

One track: the path that maximises the summed gain.  In ascending n, per node b of frame n that is present and not used

  S[n, b] = max(0.0, max over g ascending, a ascending of S[n - g, a] + gain[n, g, a, b])

under strict >, so ties go to "start here" first and then to the lower (g, a); a NaN never wins.  Every other node has
S = -inf and is nobody's predecessor.  The track ends at the first maximum of S in (n, b) order and its nodes come from the
back-pointers; score = that S.  With seed = (n0, k0) only the seed may start a path (every other node starts from -inf) and the
frames before n0 are ignored; the half before the seed is the same recursion, seeded at (N - 1 - n0, k0), on the
frame-reversed video (gain recomputed on the flipped input: the Python layer does exactly that), and the track is the union of
the halves, its score the sum of theirs.  A seed names one person: it goes with tracks = 1.

Several tracks.  Greedy: M rounds of the same recursion, each marking its nodes used.  A round whose best path has fewer than
min_frames nodes ends the extraction: that track and all later ones are -1 everywhere, score NaN, 0 frames.

Outputs.  assign [M,N] int32 (the candidate, or -1), score [M] fp64, frames [M] int32, and the gather: x2d [M,N,J,2] and
conf [M,N,J] carry the bits of the chosen candidate; a frame without one is zeros with confidence 0 - the detector's own
encoding of "not found", which the repair fills and every fit ignores.

gate = 0.5, skip = 0.05, max_gap = 4, support = 5, min_frames = 5 and threshold = 0 are defaults, not tuned values.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

from .rootfit import lane_sum

MAX_K, MAX_GAP, MAX_TRACKS = 64, 8, 64


def check(N, K, tracks, seed, gate, skip, max_gap, support, min_frames, threshold):
    """the refusals of the Python layers (the C entries repeat them) -> (M, G, support, min_frames, seed or None)"""
    M, G, s, mf = int(tracks), int(max_gap), int(support), int(min_frames)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"tracks: K must lie in 1 .. {MAX_K}, got {K} (pass the largest number of people in any frame)")
    if N < 1:
        raise ValueError(f"tracks: N must be >= 1, got {N}")
    if M != tracks or not 1 <= M <= MAX_TRACKS:
        raise ValueError(f"tracks: tracks must lie in 1 .. {MAX_TRACKS}, got {tracks!r}")
    if G != max_gap or not 1 <= G <= MAX_GAP:
        raise ValueError(f"tracks: max_gap must lie in 1 .. {MAX_GAP}, got {max_gap!r}")
    if s != support or not 1 <= s <= 65535:
        raise ValueError(f"tracks: support must lie in 1 .. 65535, got {support!r}")
    if mf != min_frames or mf < 1:
        raise ValueError(f"tracks: min_frames must be >= 1, got {min_frames!r}")
    if not (np.isfinite(gate) and gate > 0):
        raise ValueError(f"tracks: gate must be finite and > 0, got {gate!r}")
    if not (np.isfinite(skip) and skip >= 0):
        raise ValueError(f"tracks: skip must be finite and >= 0, got {skip!r}")
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError(f"tracks: threshold must be finite and >= 0, got {threshold!r}")
    if seed is not None:
        n0, k0 = (int(v) for v in seed)
        if not (0 <= n0 < N and 0 <= k0 < K):
            raise ValueError(f"tracks: seed {seed!r} outside [0, {N}) x [0, {K})")
        if M != 1:
            raise ValueError("tracks: a seed names one person, it goes with tracks=1")
        seed = (n0, k0)
    return M, G, s, mf, seed


def nodes(x2d, conf, support=5, threshold=0.0):
    """x2d [N,K,J,2], conf [N,K,J] -> (observed [N,K,J] bool, size [N,K] fp64, NaN where the candidate is absent)"""
    x2d, conf = np.asarray(x2d, dtype=np.float32), np.asarray(conf, dtype=np.float32)
    with np.errstate(all="ignore"):
        obs = (conf > np.float32(threshold)) & np.isfinite(x2d).all(axis=-1)
        x64 = x2d.astype(np.float64)
        lo = np.where(obs[..., None], x64, np.inf).min(axis=2)
        hi = np.where(obs[..., None], x64, -np.inf).max(axis=2)
        size = np.sqrt((hi[..., 0] - lo[..., 0]) * (hi[..., 1] - lo[..., 1]))
        present = (obs.sum(axis=2) >= support) & np.isfinite(size) & (size > 0)
    return obs, np.where(present, size, np.nan)


def links(x2d, conf, gate=0.5, skip=0.05, max_gap=4, support=5, threshold=0.0):
    """-> (gain [N,G,K,K] fp64 indexed [n, g - 1, ka, kb], size [N,K] fp64): what pafuse_tracks_links writes"""
    x2d, conf = np.asarray(x2d, dtype=np.float32), np.asarray(conf, dtype=np.float32)
    N, K, J, _ = x2d.shape
    G = int(max_gap)
    obs, size = nodes(x2d, conf, support, threshold)
    x64 = x2d.astype(np.float64)
    gain = np.full((N, G, K, K), -np.inf)
    gate, skip = np.float64(gate), np.float64(skip)
    present = ~np.isnan(size)
    with np.errstate(all="ignore"):
        for g in range(1, min(G, N - 1) + 1):
            n, ka, kb = np.nonzero(present[:-g, :, None] & present[g:, None, :])          # the pairs with both ends present
            xa, xb = x64[n, ka], x64[n + g, kb]                                           # [pairs, J, 2]
            common = obs[n, ka] & obs[n + g, kb]
            w = np.where(common, np.minimum(conf[n, ka], conf[n + g, kb]).astype(np.float64), 0.0)
            dx, dy = xb[..., 0] - xa[..., 0], xb[..., 1] - xa[..., 1]
            dist = np.sqrt(dx * dx + dy * dy)
            num = lane_sum(np.where(common, w * dist, 0.0))
            den = lane_sum(w)
            cost = (num / den) / (0.5 * (size[n, ka] + size[n + g, kb]))
            ok = (common.sum(axis=-1) >= support) & (cost <= gate)
            gain[n + g, g - 1, ka, kb] = np.where(ok, (gate - cost) - skip * np.float64(g - 1), -np.inf)
    return gain, size


def one_track(gain, alive, seed=None):
    """gain [N,G,K,K], alive [N,K] bool (present and not used) -> (nodes [N] int, -1 where the track has none; score; count).
    Without a node that may start a path: all -1, -inf, 0."""
    N, G, K, _ = gain.shape
    S = np.full((N, K), -np.inf)
    back = np.zeros((N, K, 2), dtype=np.int64)                       # (g, a); g = 0: the path starts here
    n0 = 0 if seed is None else seed[0]
    best, end = -np.inf, None
    with np.errstate(all="ignore"):
        for n in range(n0, N):                                       # all b of a frame at once; (g, a) in the stated order
            v = np.zeros(K) if seed is None else np.full(K, -np.inf)
            if seed is not None and n == seed[0]:
                v[seed[1]] = 0.0
            for g in range(1, min(G, n - n0) + 1):
                c = S[n - g][:, None] + gain[n, g - 1]               # [a, b]
                c = np.where(np.isnan(c), -np.inf, c)                # a NaN never wins
                a = np.argmax(c, axis=0)                             # the first maximum over a: the lower a at a tie
                top = c[a, np.arange(K)]
                win = top > v                                        # strict: the earlier (start, lower g) keeps a tie
                v = np.where(win, top, v)
                back[n][win] = np.stack([np.full(K, g), a], axis=-1)[win]
            S[n] = np.where(alive[n], v, -np.inf)
            if S[n].max() > best:
                best, end = S[n].max(), (n, int(np.argmax(S[n])))
    out = np.full(N, -1, dtype=np.int64)
    if end is None:
        return out, -np.inf, 0
    n, b = end
    count = 0
    while True:
        out[n] = b
        count += 1
        g, a = back[n, b]
        if g == 0:
            break
        n, b = n - g, a
    return out, np.float64(best), count


def path(gain, size, tracks=1, min_frames=5, seed=None):
    """What pafuse_tracks_path writes from a gain table and the sizes (present = not NaN): (assign [M,N] int32, score [M]
    fp64, frames [M] int32).  With a seed: the half from the seed on, nothing else."""
    gain, size = np.asarray(gain, dtype=np.float64), np.asarray(size, dtype=np.float64)
    N, K = size.shape
    M = int(tracks)
    assign = np.full((M, N), -1, dtype=np.int32)
    score = np.full(M, np.nan)
    frames = np.zeros(M, dtype=np.int32)
    used = np.zeros((N, K), dtype=bool)
    present = ~np.isnan(size)
    for m in range(M):
        row, s, c = one_track(gain, present & ~used, seed)
        if c < min_frames:
            break
        assign[m], score[m], frames[m] = row, s, c
        on = row >= 0
        used[np.nonzero(on)[0], row[on]] = True
    return assign, score, frames


def join_halves(fwd, bwd, min_frames):
    """(assign [1,N], score [1], frames [1]) of the half from the seed on and of the half on the flipped video -> the track"""
    (fa, fs, ff), (ba, bs, bf) = fwd, bwd
    assign = np.where(fa >= 0, fa, ba[:, ::-1]).astype(np.int32)
    count = int(ff[0]) + int(bf[0]) - 1
    if ff[0] < 1 or bf[0] < 1 or count < min_frames:                  # an absent seed has neither half
        return np.full_like(assign, -1), np.full(1, np.nan), np.zeros(1, dtype=np.int32)
    return assign, np.asarray(fs, dtype=np.float64) + np.asarray(bs, dtype=np.float64), np.array([count], dtype=np.int32)


def gather(x2d, conf, assign):
    """-> (x2d [M,N,J,2], conf [M,N,J]): the chosen candidates' bits, zeros with confidence 0 where there is none"""
    x2d, conf = np.asarray(x2d, dtype=np.float32), np.asarray(conf, dtype=np.float32)
    assign = np.asarray(assign)
    n = np.arange(x2d.shape[0])[None, :]
    k = np.where(assign >= 0, assign, 0)
    on = assign >= 0
    return (np.where(on[..., None, None], x2d[n, k], np.float32(0)).astype(np.float32),
            np.where(on[..., None], conf[n, k], np.float32(0)).astype(np.float32))


def track(x2d, conf, tracks=1, seed=None, gate=0.5, skip=0.05, max_gap=4, support=5, min_frames=5, threshold=0.0):
    """-> {"x2d" [M,N,J,2], "conf" [M,N,J], "assign" [M,N] int32, "score" [M] fp64, "frames" [M] int32, "gain", "size"}"""
    x2d, conf = np.asarray(x2d, dtype=np.float32), np.asarray(conf, dtype=np.float32)
    N, K, J, _ = x2d.shape
    assert x2d.shape == (N, K, J, 2) and conf.shape == (N, K, J) and J >= 1
    M, G, s, mf, seed = check(N, K, tracks, seed, gate, skip, max_gap, support, min_frames, threshold)
    gain, size = links(x2d, conf, gate, skip, G, s, threshold)
    if seed is None:
        assign, score, frames = path(gain, size, M, mf)
    else:
        rgain, rsize = links(x2d[::-1], conf[::-1], gate, skip, G, s, threshold)
        assign, score, frames = join_halves(path(gain, size, 1, 1, seed), path(rgain, rsize, 1, 1, (N - 1 - seed[0], seed[1])), mf)
    gx, gc = gather(x2d, conf, assign)
    return {"x2d": gx, "conf": gc, "assign": assign, "score": score, "frames": frames, "gain": gain, "size": size}


# ------------------------------------------------------------------------------------------------------------ planting
def plant_video(people_x2d, people_conf, slots=None, seed=0, drop=None, ghost=None):
    """people_x2d [P,N,J,2], people_conf [P,N,J]: P people, each with one detection per frame -> {"x2d" [N,K,J,2], "conf"
    [N,K,J] (fp32), "truth" [P,N] int32: the slot that holds person p at frame n, -1 where the detector lost them}.
    K = slots (default P) >= P; every frame draws its own order of the K slots (np.random.default_rng(seed)); the slots
    left over are all-zero.  drop = (rate, run): at every (person, frame) a run of `run` lost frames starts with probability
    rate / run and a length drawn in 1 .. run; runs that would touch or overlap an earlier one are not planted, so no person is
    gone for more than `run` frames.  ghost = (rate, y): with probability `rate` a frame gets one more detection in a free slot (if there is one) -
    person 0's of that frame moved to a random x in (-1, 1) and to height y - which belongs to nobody."""
    px, pc = np.asarray(people_x2d, dtype=np.float32), np.asarray(people_conf, dtype=np.float32)
    P, N, J, _ = px.shape
    K = P if slots is None else int(slots)
    if K < P or pc.shape != (P, N, J):
        raise ValueError(f"plant_video: slots must be >= the {P} people and conf [P,N,J], got {K} and {pc.shape}")
    rng = np.random.default_rng(seed)
    lost = np.zeros((P, N), dtype=bool)
    if drop is not None:
        rate, run = float(drop[0]), int(drop[1])
        start = rng.random((P, N)) < rate / max(run, 1)
        length = rng.integers(1, max(run, 1) + 1, (P, N))              # every run draws its length in 1 .. run
        for p in range(P):
            for n in range(1, N - run):                                # the first and the last frames stay
                if start[p, n] and not lost[p, n - 1:n + length[p, n] + 1].any():
                    lost[p, n:n + length[p, n]] = True
    x = np.zeros((N, K, J, 2), dtype=np.float32)
    c = np.zeros((N, K, J), dtype=np.float32)
    truth = np.full((P, N), -1, dtype=np.int32)
    for n in range(N):
        order = rng.permutation(K)
        for p in range(P):
            if not lost[p, n]:
                x[n, order[p]], c[n, order[p]], truth[p, n] = px[p, n], pc[p, n], order[p]
        if ghost is not None and K > P and rng.random() < float(ghost[0]):
            centre = px[0, n].mean(axis=0)
            to = np.array([rng.uniform(-1.0, 1.0), float(ghost[1])], dtype=np.float32)
            x[n, order[P]], c[n, order[P]] = px[0, n] - centre + to, pc[0, n]
    return {"x2d": x, "conf": c, "truth": truth}


def plant_people(x2d, conf, people, seed=0, slots=None, spacing=1.5, others=None, drop=None, ghost=None):
    """A one-person video x2d [N,J,2], conf [N,J] -> plant_video of `people` people: person 0 is the input, person p >= 1 a
    copy shifted along x by spacing * its own width * (+1, -1, +2, -2, ...), or - with others = [(x2d, conf), ...] - another
    sequence's detections, repeated to N frames."""
    x2d, conf = np.asarray(x2d, dtype=np.float32), np.asarray(conf, dtype=np.float32)
    N, J, _ = x2d.shape
    P = int(people)
    if P < 1 or conf.shape != (N, J):
        raise ValueError(f"plant_people: people >= 1 and conf [N,J], got {people!r} and {conf.shape}")
    px, pc = [x2d], [conf]
    on = conf > 0
    width = float(np.ptp(x2d[..., 0][on])) if on.any() else 1.0
    for p in range(1, P):
        if others is not None:
            ox, oc = (np.asarray(v, dtype=np.float32) for v in others[(p - 1) % len(others)])
            idx = np.arange(N) % ox.shape[0]
            px.append(ox[idx]), pc.append(oc[idx])
        else:
            step = ((p + 1) // 2) * (1 if p % 2 else -1)
            px.append(x2d + np.array([spacing * width * step, 0.0], dtype=np.float32)), pc.append(conf)
    return plant_video(np.stack(px), np.stack(pc), slots, seed, drop, ghost)


def track_error(assign, truth):
    """assign [N] (one track) against truth [N] (one person's slots, -1 where lost) -> {"right": frames with the person's
    slot, "wrong": frames with another slot (the person present or not), "missed": frames where the person is present and
    the track has nobody, "switches": the times the track goes from right to wrong or back between consecutive frames it
    has somebody in}.  For assign [M,N] and truth [P,N]: a list, track m against the person it shares most frames with
    (entry "person", -1 for an empty track)."""
    assign, truth = np.asarray(assign), np.asarray(truth)
    if assign.ndim == 2:
        out = []
        for row in assign:
            hits = [int(((row == t) & (t >= 0)).sum()) for t in truth]
            p = int(np.argmax(hits)) if (row >= 0).any() else -1
            out.append(dict(track_error(row, truth[max(p, 0)]), person=p))
        return out
    has = assign >= 0
    right = has & (assign == truth)
    wrong = has & ~right
    state = right[has]
    return {"right": int(right.sum()), "wrong": int(wrong.sum()), "missed": int((~has & (truth >= 0)).sum()),
            "switches": int((state[1:] != state[:-1]).sum())}

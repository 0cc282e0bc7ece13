"""The J-Agg path of a whole video on the device: frames_path_kernel (pafuse_frames_path), ops.frames_path,
torch.ops.pafuse.frames_path, evaluate.path_frames, infer_sequence(path_scope="video") and evaluate_frames(path_scope="video").

What is asserted and why it can be asserted: as in tests/test_hip_pose_path.py.  The kernel and posepath.frames_path (= the
per-clip statement on the dense [W*P, N] form) perform the same IEEE operations in the same order on the same operands,
so idx and window are torch.equal and cost is the same double (an adjacent one would be accepted, and is printed).  The
statement is fed the e2 the DEVICE computes for every hypothesis of every window (`device_e2` on the windows cut from the
video), because reproj_error is an fp32 expression the device compiler may contract.

Shapes (W,T,P,F,J; N, stride): (17,1,20,9,134; 70, 4) K = 60, 134 lines, windows entering and leaving every four frames, the
shifted last window; (3,2,2,3,5; 7, 2) the brute-forceable one, T = 2; (8,1,64,4,5; 11, 1) K = 256, four slots per lane, the set
changes at every frame; (2,1,65,2,5; 4, 2) disjoint clips and the first size with two slots per lane; (5,1,13,5,5; 9, 1) K = 65
reached by overlap; (2,1,5,27,5; 30, 27) the shifted last window, 24 frames of overlap; (1,1,3,3,5; 2) one padded window;
W = P = F = N = 1.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, same_bits, sequence, tables
from tests.test_hip_pose_aggregate import DEV, J, inputs
from tests.test_hip_pose_path import C5, WEIGHTS, adjacent64, device_e2, wb_of

pytestmark = pytest.mark.gpu
BIG = (1, 20, 9, 134, 70, 4)         # T, P, F, J; N, stride
SMALL = [(2, 2, 3, 5, 7, 2), (1, 64, 4, 5, 11, 1), (1, 65, 2, 5, 4, 2), (1, 13, 5, 5, 9, 1), (1, 5, 27, 5, 30, 27), (1, 3, 3, 5, 2, 3),
         (1, 1, 1, 5, 1, 1)]
WINDOWS = {BIG: 17, SMALL[0]: 3, SMALL[1]: 8, SMALL[2]: 2, SMALL[3]: 5, SMALL[4]: 2, SMALL[5]: 1, SMALL[6]: 1}


def cut(seq, starts, F):
    from pafuse_amd import harness
    return harness.cut_windows(seq, starts, F).contiguous()


class Video:
    """one video with everything both sides need, computed once: the windows, the pooled mean, fitted roots, device e2"""

    def __init__(self, T, P, F, Jn, N, stride, seed, conn=None):
        from pafuse_amd.windows import window_starts
        self.starts, self.valid = window_starts(N, F, stride)
        W = len(self.starts)
        self.W, self.T, self.P, self.F, self.J, self.N = W, T, P, F, Jn, N
        g = torch.Generator().manual_seed(seed)
        if Jn == J:
            pred, self.conn = inputs(W, T, P, F, seed)["pred"], tables()[0]
        else:
            pred = (torch.randn(W, T, P, F, Jn, 3, generator=g) * 0.25).to(DEV)
            self.conn = torch.tensor(C5 if conn is None else conn, dtype=torch.int32, device=DEV)
        x2d = torch.rand(N, Jn, 2, generator=g) * 2 - 1
        traj = torch.randn(N, 3, generator=g) * 0.1
        traj[:, 2] = 4.0
        self.pred, self.x2d, self.traj, self.cam = pred.contiguous(), x2d.to(DEV), traj.to(DEV), sequence(1)[2].to(DEV)
        self.conf = (torch.rand(N, Jn, generator=g) >= 0.2).float().to(DEV)                 # a fifth of (frame, joint) off
        self.prepare()

    def prepare(self):
        from pafuse_amd import ops
        W, T, P, F, Jn, N = self.W, self.T, self.P, self.F, self.J, self.N
        # what the per-clip helpers take: the windows as a batch of clips
        self.z = {"pred": self.pred, "x2d": cut(self.x2d, self.starts, F), "traj": cut(self.traj, self.starts, F), "cam": self.cam}
        self.conf_w = cut(self.conf, self.starts, F)
        self.wb = wb_of(self.z) if (Jn == J or self.conn.cpu().tolist() == C5) else self.pred.cpu().clone()
        self.tfit = torch.full((W, T, P, F, 3), 7.0, device=DEV)
        self.fit_state = ops.pose_partials_fit(self.pred, self.conn, 0, self.z["x2d"], self.cam, conf=self.conf_w, tfit=self.tfit)
        self.state = ops.pose_partials(self.pred, self.conn, 0, self.z["x2d"], self.z["traj"], self.cam)
        self.frame = ops.fold_windows(ops.frame_state(N, T, Jn, DEV), N, self.state, (W, T, F, Jn), self.starts, self.valid, 0, P)
        self.fold = ops.finish_frames(N, T, Jn, frame=self.frame)
        self.mean = self.fold["mean"]
        self.e2 = {}

    def root(self, kind):
        return self.traj if kind == "traj" else self.tfit

    def unary(self, kind, gated):
        from pafuse_amd import posepath
        if kind not in self.e2:
            self.e2[kind] = device_e2(self.z, self.conn, self.z["traj"] if kind == "traj" else self.tfit).cpu().numpy()
        return posepath.gate(self.e2[kind], self.conf_w.cpu().numpy()) if gated else self.e2[kind]

    def run(self, kind, weight, gated, mean=True, **kw):
        from pafuse_amd import ops
        return ops.frames_path(self.pred, self.conn, self.x2d, self.root(kind), self.cam, weight, self.starts, self.valid,
                               conf=self.conf if gated else None, mean=self.mean if mean else None, want=ops.FRAMES_PATH_OUTPUTS, **kw)

    def want(self, kind, weight, gated, mean=True):
        from pafuse_amd import posepath
        return posepath.frames_path(self.unary(kind, gated), self.wb.numpy(), self.mean.cpu().numpy() if mean else None,
                                    self.starts, self.valid, self.N, weight)

    def gather(self, idx, window):
        """wb at (window, idx, the window's local frame) [T,N,J,3]; rows with idx < 0 are not meant"""
        T, N, Jn = idx.shape
        w, h = window.clamp(min=0).long(), idx.clamp(min=0).long()
        f = (torch.arange(N)[None, :, None] - torch.from_numpy(self.starts).long()[w]).clamp(0, self.F - 1)
        return self.wb[w, torch.arange(T)[:, None, None], h, f, torch.arange(Jn)[None, None, :]]


def compare(v, kind, weight, gated, mean=True):
    got, want = v.run(kind, weight, gated, mean), v.want(kind, weight, gated, mean)
    tag = (kind, weight, gated, mean)
    idx, win = got["idx"].cpu(), got["window"].cpu()
    assert idx.dtype == torch.int32 and win.dtype == torch.int32 and tuple(idx.shape) == (v.T, v.N, v.J) == tuple(win.shape)
    assert torch.equal(idx, torch.from_numpy(want["idx"])), tag
    assert torch.equal(win, torch.from_numpy(want["window"])), tag
    cost = got["cost"].cpu().numpy()
    same = np.array_equal(cost, want["cost"], equal_nan=True)
    print(f"{tag}: cost {'equal' if same else 'ADJACENT'}; lines without a path {int((idx[:, 0] < 0).sum())} of {v.T * v.J}")
    assert adjacent64(cost, want["cost"]), tag
    assert np.array_equal(got["pick"].cpu().numpy(), want["pick"], equal_nan=True), tag
    assert np.array_equal(got["e2"].cpu().numpy(), want["e2"]), tag
    alive = idx >= 0
    assert torch.equal(alive, win >= 0)
    assert torch.equal(got["pick"].cpu()[alive], v.gather(idx, win)[alive]) and torch.isnan(got["pick"].cpu()[~alive]).all(), tag
    return got


def sweep(v, kind, gated, mean=True):
    """the three weights of one (root kind, conf) setting -> (the last result, picks a weight moved, steps of a path from
    one window into another)"""
    moved = switched = 0
    for weight in WEIGHTS:
        got = compare(v, kind, weight, gated, mean)
        if weight == 0.0:
            free = got
        else:
            moved += int((got["idx"] != free["idx"]).sum() + (got["window"] != free["window"]).sum())
            w = got["window"]
            switched += int(((w[:, 1:] != w[:, :-1]) & (w[:, 1:] >= 0)).sum())
    return got, moved, switched


@pytest.fixture(scope="module")
def big():
    v = Video(*BIG, seed=41)
    assert v.W == WINDOWS[BIG]
    return v


@pytest.mark.parametrize("kind,gated", [("traj", False), ("traj", True), ("fit", False), ("fit", True)])
def test_path_is_the_statement(big, kind, gated):
    got, moved, switched = sweep(big, kind, gated)
    assert moved > 0          # the penalty changed picks: the comparison is not the weight = 0 case three times
    assert switched > 0       # some path goes from one window into another
    if gated:                 # an unobserved (frame, joint) reports no error, and on a line with a path it still gets a hypothesis
        off = ~(big.conf > 0)[None].expand(big.T, big.N, big.J)
        assert off.any() and (got["idx"][off] >= 0).any() and torch.isinf(got["e2"][off]).all()


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "-".join(map(str, s)))
def test_small_shapes(shape):
    v = Video(*shape, seed=50 + shape[1])
    assert v.W == WINDOWS[shape]
    moved = switched = 0
    for kind in ("traj", "fit"):
        for gated in (False, True):
            _, m, s = sweep(v, kind, gated)
            moved, switched = moved + m, switched + s
    assert moved > 0 or v.P == 1 or v.N == 1      # (two frames of three hypotheses: not in every setting, but in the case)
    assert switched > 0 or v.W == 1
    compare(v, "traj", 0.5, False, mean=False)


def test_one_window_is_pose_path():
    """One clip call on a batch of B = 2 clips against two video calls of one window each: the same bits per clip in every
    output, at one and at two slots per lane - the video stride of every operand and the decode of the line (v, t, j)."""
    from pafuse_amd import ops
    for P in (5, 65):
        vs = [Video(2, P, 3, J, 3, 3, seed=61 + b) for b in range(2)]
        assert all(v.W == 1 for v in vs)
        batch = lambda pick: torch.cat([pick(v) for v in vs]).contiguous()
        for kind in ("traj", "fit"):
            for gated in (False, True):
                root = batch(lambda v: v.z["traj"] if kind == "traj" else v.tfit)
                clip = ops.pose_path(batch(lambda v: v.pred), vs[0].conn, batch(lambda v: v.z["x2d"]), root, vs[0].cam, 0.5,
                                     conf=batch(lambda v: v.conf_w) if gated else None, mean=batch(lambda v: v.mean[None]),
                                     want=ops.PATH_OUTPUTS)
                for b, v in enumerate(vs):
                    got, tag = v.run(kind, 0.5, gated), (P, kind, gated, b)
                    assert torch.equal(got["idx"], clip["idx"][b]) and same_bits(got["pick"], clip["pick"][b]), tag   # (NaN on a line without a path)
                    assert torch.equal(got["window"], torch.where(got["idx"] >= 0, 0, -1).int()) and (got["idx"] >= 0).any(), tag
                    assert same_bits(got["e2"], clip["e2"][b]) and same_bits(got["cost"], clip["cost"][b]), tag
        assert not torch.equal(vs[0].pred, vs[1].pred) and not torch.equal(clip["idx"][0], clip["idx"][1])   # two clips, not one twice


@pytest.mark.parametrize("entry", ["clip", "video"])
def test_without_e2_the_path_is_the_same(entry):
    """want without "e2": pick_e2 is null - in the video kernel the observed mark of the forward pass then has nowhere to live
    and the backtrace forms no e2 - and pick and idx keep the bits of the call that asks for e2 (conf gated, so that there
    are unobserved frames)."""
    from pafuse_amd import ops
    if entry == "clip":                                  # (B,T,P,F) = (2,2,65,3), J = 5
        g = torch.Generator().manual_seed(91)
        pred = (torch.randn(2, 2, 65, 3, 5, 3, generator=g) * 0.25).to(DEV)
        x2d = (torch.rand(2, 3, 5, 2, generator=g) * 2 - 1).to(DEV)
        traj = torch.randn(2, 3, 3, generator=g) * 0.1
        traj[..., 2] = 4.0
        conf = (torch.rand(2, 3, 5, generator=g) >= 0.2).float().to(DEV)
        conn = torch.tensor(C5, dtype=torch.int32, device=DEV)
        run = lambda want: ops.pose_path(pred, conn, x2d, traj.to(DEV), sequence(1)[2].to(DEV), 0.5, conf=conf, want=want)
        names = ops.PATH_OUTPUTS
    else:
        v = Video(*SMALL[2], seed=92)
        run = lambda want: ops.frames_path(v.pred, v.conn, v.x2d, v.traj, v.cam, 0.5, v.starts, v.valid, conf=v.conf, mean=v.mean, want=want)
        names = ops.FRAMES_PATH_OUTPUTS
    full, bare = run(names), run(("pick", "idx"))
    assert set(bare) == {"pick", "idx"} and (full["idx"] >= 0).any() and torch.isinf(full["e2"]).any()
    assert torch.equal(bare["idx"], full["idx"]) and same_bits(bare["pick"], full["pick"])


def test_zero_weight_is_the_pick_of_the_fold(big):
    from pafuse_amd import ops
    got, fold = big.run("traj", 0.0, False), big.fold
    assert (fold["idx"] >= 0).all()
    assert torch.equal(got["idx"], fold["idx"]) and torch.equal(got["window"], fold["window"]) and torch.equal(got["pick"], fold["pick"])
    # on the fitted roots with the weights: wherever the fold has a pick it is the path's; where it has none (a weight not
    # > 0: unobserved) the path still carries a hypothesis through and reports e2 = +inf
    frame = ops.fold_windows(ops.frame_state(big.N, big.T, big.J, DEV), big.N, big.fit_state, (big.W, big.T, big.F, big.J), big.starts,
                             big.valid, 0, big.P)
    fit, got = ops.finish_frames(big.N, big.T, big.J, frame=frame), big.run("fit", 0.0, True)
    has = fit["idx"] >= 0
    alive = (got["idx"] >= 0).all(dim=1)[:, None].expand_as(has)
    assert has.any() and (~has & alive).any()
    assert torch.equal(got["idx"][has & alive], fit["idx"][has & alive]) and torch.equal(got["window"][has & alive], fit["window"][has & alive])
    assert torch.equal(got["pick"][has & alive], fit["pick"][has & alive])
    off = ~(big.conf > 0)[None].expand_as(has) & alive
    assert (got["idx"][off] >= 0).all() and torch.isinf(got["e2"][off]).all()


def seam_video(F=4):
    """Two clips at stride = F, P = 3, J = 5 with a connection table of zeros (joint 0 at 0: wb = pred, the joints independent).
    Clip 1 holds clip 0's hypotheses - constant along the frames, 0.5 m and 0.75 m apart - under the permutation (0,1,2) ->
    (2,0,1).  The detections of clip 0 are the same point at every frame and those of clip 1 another one, so the unaries are
    constant inside a clip and a per-clip pick knows nothing of the other clip."""
    v = Video.__new__(Video)
    g = torch.Generator().manual_seed(71)
    P, T, Jn, N = 3, 1, 5, 2 * F
    from pafuse_amd.windows import window_starts
    v.starts, v.valid = window_starts(N, F, F)
    v.W, v.T, v.P, v.F, v.J, v.N = 2, T, P, F, Jn, N
    base = torch.randn(Jn, 3, generator=g) * 0.1
    hyp = torch.stack([base, base + torch.tensor([0.5, 0.0, 0.0]), base - torch.tensor([0.0, 0.75, 0.0])])      # [P,J,3]
    hyp[:, 0] = 0
    pred = torch.empty(2, T, P, F, Jn, 3)
    pred[0] = hyp[None, :, None]
    pred[1] = hyp[[2, 0, 1]][None, :, None]
    a, b = torch.rand(Jn, 2, generator=g) * 0.4 - 0.2, torch.rand(Jn, 2, generator=g) * 0.4 - 0.2
    x2d = torch.cat([a[None].expand(F, Jn, 2), b[None].expand(F, Jn, 2)])
    traj = torch.zeros(N, 3)
    traj[:, 2] = 4.0
    v.conn = torch.zeros(Jn, dtype=torch.int32, device=DEV)
    v.pred, v.x2d, v.traj, v.cam = pred.contiguous().to(DEV), x2d.contiguous().to(DEV), traj.to(DEV), sequence(1)[2].to(DEV)
    v.conf = torch.ones(N, Jn, device=DEV)
    v.prepare()
    return v


def test_the_path_keeps_the_geometric_hypothesis_across_a_seam():
    from pafuse_amd import ops
    v, lam = seam_video(), 8.0
    F, geo = v.F, torch.tensor([1, 2, 0])                    # geometric hypothesis g sits at index geo[g] in clip 1
    got = compare(v, "traj", lam, False, mean=False)
    e2 = torch.from_numpy(v.unary("traj", False))            # [2,1,3,F,J]
    alone = ops.pose_path(v.pred, v.conn, v.z["x2d"], v.z["traj"], v.cam, lam, want=("idx",))["idx"].cpu()    # per clip
    idx, win = got["idx"].cpu(), got["window"].cpu()
    held = 0
    for j in range(1, v.J):
        # a path that never jumps stays on one geometric hypothesis g: index g in clip 0, geo[g] in clip 1
        stay = e2[0, 0, :, :, j].double().sum(dim=1) + e2[1, 0, geo, :, j].double().sum(dim=1)               # [3]
        g = int(stay.argmin())
        floor = float(e2[0, 0, :, :, j].double().min(dim=0).values.sum() + e2[1, 0, :, :, j].double().min(dim=0).values.sum())
        own = int(e2[1, 0, :, :, j].double().sum(dim=1).argmin())                                             # clip 1's own best
        if float(stay[g]) - floor < lam * 0.5 and own != int(geo[g]):
            # no jump (>= 0.5 m, at weight 8) can pay for itself, and the hypothesis held is not what clip 1 alone prefers
            assert (idx[0, :F, j] == g).all() and (win[0, :F, j] == 0).all()
            assert (idx[0, F:, j] == geo[g]).all() and (win[0, F:, j] == 1).all()                             # the video path holds it
            assert torch.equal(got["pick"].cpu()[0, F:, j], got["pick"].cpu()[0, :F, j])                      # no jump at the seam
            assert (alone[1, 0, :, j] == own).all() and own != int(geo[g])                                    # the clip path does not
            held += 1
    print("joints whose geometric hypothesis is held across the seam against clip 1's own preference:", held)
    assert held > 0


def raw_call(v, weight, pred=None, x2d=None, pad=5):
    """the C entry itself on buffers with guard rows (absolute offsets): -> (pick, idx, window, e2, cost, guards intact?)"""
    from pafuse_amd import _lib, ops
    lib = _lib.load()
    pred = v.pred if pred is None else pred
    x2d = v.x2d if x2d is None else x2d
    W, T, P, F, Jn, N = v.W, v.T, v.P, v.F, v.J, v.N
    n, lines = T * N * Jn, T * Jn
    pick = torch.full((pad + n * 3 + pad,), 7.0, device=DEV)
    idx = torch.full((pad + n + pad,), 77, device=DEV, dtype=torch.int32)
    win = torch.full((pad + n + pad,), 77, device=DEV, dtype=torch.int32)
    e2 = torch.full((pad + n + pad,), 7.0, device=DEV)
    cost = torch.full((pad + lines + pad,), 7.0, device=DEV, dtype=torch.float64)
    need = ops.frames_path_workspace_bytes(N, T, Jn, P, v.starts, v.valid)
    assert need == lib.pafuse_frames_path_workspace_bytes(N, T, Jn, P, W, v.starts.ctypes.data, v.valid.ctypes.data) > 0
    ws = torch.full((8 + need + 64,), 0xAB, device=DEV, dtype=torch.uint8)
    tab = torch.from_numpy(np.stack([v.starts, v.valid])).to(DEV)
    _lib.check(lib.pafuse_frames_path(
        pred.data_ptr(), x2d.data_ptr(), v.traj.data_ptr(), 0, v.cam.data_ptr(), None, v.conn.data_ptr(), None, float(weight),
        W, T, P, F, Jn, N, tab[0].data_ptr(), tab[1].data_ptr(), v.starts.ctypes.data, v.valid.ctypes.data,
        pick[pad:].data_ptr(), idx[pad:].data_ptr(), win[pad:].data_ptr(), e2[pad:].data_ptr(), cost[pad:].data_ptr(),
        ws[8:].data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    used = need // 8 * 8
    edge = lambda t, val: bool((t[:pad] == val).all() and (t[-pad:] == val).all())
    intact = (edge(pick, 7) and edge(idx, 77) and edge(win, 77) and edge(e2, 7) and edge(cost, 7)
              and bool((ws[:8] == 0xAB).all() and (ws[8 + used:] == 0xAB).all()))
    return (pick[pad:pad + n * 3].view(T, N, Jn, 3), idx[pad:pad + n].view(T, N, Jn), win[pad:pad + n].view(T, N, Jn),
            e2[pad:pad + n].view(T, N, Jn), cost[pad:pad + lines].view(T, Jn), intact)


def test_planted_nans_touch_only_their_lines_and_guards_stay():
    from pafuse_amd import posepath
    v, weight = Video(*SMALL[0], seed=81), 0.5               # W = 3 windows at 0, 2, 4 of N = 7; C5: joints 2, 3 hang on 1
    T, N, Jn = v.T, v.N, v.J
    clean = raw_call(v, weight)
    assert clean[5]
    want = v.run("traj", weight, False, mean=False)
    for got, k in zip(clean, ("pick", "idx", "window", "e2", "cost")):
        assert same_bits(got, want[k]), k
    again = raw_call(v, weight)                              # two calls give the same bits
    assert all(same_bits(a, b) for a, b in zip(clean[:5], again[:5]))
    t, j, n = 1, 1, 2                                        # frame 2 lies in windows 0 (f = 2) and 1 (f = 0)
    hit_j = [1, 2, 3]
    e2_clean = v.unary("traj", False)

    def same_elsewhere(out, js, ts):
        keep = torch.ones(T, Jn, dtype=torch.bool, device=DEV)
        for tt in ts:
            keep[tt, js] = False
        k3 = keep[:, None].expand(T, N, Jn)
        return all(torch.equal(out[i][k3], clean[i][k3]) for i in range(4)) and torch.equal(out[4][keep], clean[4][keep])

    def statement(pred, e2):
        z = {"pred": pred}
        return posepath.frames_path(e2, wb_of(z).numpy(), None, v.starts, v.valid, N, weight)

    # (a) one candidate at one frame: only that (window, hypothesis) leaves its lines, there
    pred = v.pred.clone()
    pred[0, t, 1, 2, j] = float("nan")
    out = raw_call(v, weight, pred=pred)
    assert out[5] and same_elsewhere(out, hit_j, [t])
    assert (out[1][t, :, hit_j] >= 0).all() and not ((out[2][t, n, hit_j] == 0) & (out[1][t, n, hit_j] == 1)).any()
    st = statement(pred, e2_clean)          # (the availability mask hides whatever e2 the NaN pose has)
    assert torch.equal(out[1].cpu(), torch.from_numpy(st["idx"])) and torch.equal(out[2].cpu(), torch.from_numpy(st["window"]))
    assert np.array_equal(out[4].cpu().numpy(), st["cost"], equal_nan=True)
    # (b) a NaN detection: the frame is unobserved for that joint at every t, and is carried through
    x2d = v.x2d.clone()
    x2d[n, j, 1] = float("nan")
    out = raw_call(v, weight, x2d=x2d)
    assert out[5] and same_elsewhere(out, [j], range(T))
    assert (out[1][:, :, j] >= 0).all() and torch.isinf(out[3][:, n, j]).all() and torch.isfinite(out[4][:, j]).all()
    # (c) every candidate of one frame of one joint: its lines have no path at any frame
    pred = v.pred.clone()
    pred[0, t, :, 2, j] = float("nan")
    pred[1, t, :, 0, j] = float("nan")
    out = raw_call(v, weight, pred=pred)
    assert out[5] and same_elsewhere(out, hit_j, [t])
    assert (out[1][t, :, hit_j] == -1).all() and (out[2][t, :, hit_j] == -1).all() and torch.isnan(out[0][t, :, hit_j]).all()
    assert torch.isinf(out[3][t, :, hit_j]).all() and torch.isnan(out[4][t, hit_j]).all()


def test_refusals_and_the_torch_op(big):
    from pafuse_amd import _lib, ops, torch_ops  # noqa: F401
    v = big
    args = (v.pred, v.conn, v.x2d, v.traj, v.cam)
    with pytest.raises(ValueError, match="256"):            # K = 3 * 86 = 258
        ops.frames_path(torch.zeros(v.W, 1, 86, v.F, J, 3, device=DEV), *args[1:], 0.5, v.starts, v.valid)
    with pytest.raises(_lib.PafuseError, match="workspace"):
        ops.frames_path(*args, 0.5, v.starts, v.valid, workspace=torch.empty(8, device=DEV, dtype=torch.uint8))
    for weight in (-0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.PafuseError, match="weight"):
            ops.frames_path(*args, weight, v.starts, v.valid)
    with pytest.raises(ValueError):
        ops.frames_path(*args, 0.5, v.starts[:-1], v.valid[:-1])                # not the whole video
    with pytest.raises(ValueError):
        ops.frames_path(*args, 0.5, v.starts, v.valid, mean=v.mean[:, :-1])
    want = v.run("traj", 0.5, False)
    got = torch.ops.pafuse.frames_path(*args, 0.5, v.starts.tolist(), v.valid.tolist(), None, v.mean)
    assert all(same_bits(g, want[k]) for g, k in zip(got, ops.FRAMES_PATH_OUTPUTS))


# ---------------------------------------------------------------------------------------------------- end to end
SEED, FRAMES = 3, 30


@pytest.fixture(scope="module")
def model():
    from __graft_entry__ import make_model
    return make_model(5, 2, depth=2)[0]


def infer(model, **kw):
    """one infer_sequence call on the 30-frame video from the start of noise stream (SEED, call 0)"""
    from pafuse_amd import harness
    seq_2d, seq_3d, cam = sequence(FRAMES)
    model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
    if kw.get("aggregate") == "reproj":
        kw.update(traj=seq_3d[:, 0].contiguous())
    return harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, cam=cam, **kw)


def test_path_frames_is_the_kernel_on_the_folded_mean(big):
    from pafuse_amd import evaluate
    v = big
    frames = evaluate.FrameState(v.N, v.T, v.J, torch.device(DEV))
    frames.pose, frames.windows = v.frame, v.W
    out = evaluate.path_frames(v.pred, dataset(), v.x2d, v.cam, 0.5, v.starts, v.valid, v.N, frames, traj=v.traj)
    want = v.run("traj", 0.5, False)
    assert torch.equal(out["mean"], v.mean) and all(same_bits(out[k], want[k]) for k in want)
    out = evaluate.path_frames(v.pred, dataset(), v.x2d, v.cam, 0.5, v.starts, v.valid, v.N, frames, conf=v.conf, fit=True)
    want = v.run("fit", 0.5, True)
    assert all(same_bits(out[k], want[k]) for k in want)
    with pytest.raises(ValueError):
        evaluate.path_frames(v.pred, dataset(), v.x2d, v.cam, 0.5, v.starts, v.valid, v.N, None, traj=v.traj)


def test_infer_sequence_along_the_video(model):
    plain = infer(model, aggregate="reproj")
    same = infer(model, aggregate="reproj", path_scope="clip")
    assert torch.equal(same[0], plain[0]) and torch.equal(same[1], plain[1])
    clip8, same8 = infer(model, aggregate="reproj", path_weight=8.0), infer(model, aggregate="reproj", path_weight=8.0, path_scope="clip")
    assert torch.equal(clip8[0], same8[0]) and torch.equal(clip8[1], same8[1])
    pooled = infer(model, aggregate="reproj", stride=9, spread="std", trajectory=True)
    zero = infer(model, aggregate="reproj", stride=9, path_weight=0.0, path_scope="video", spread="std", trajectory=True)
    assert set(zero) == set(pooled) | {"path_cost"} and {"pose", "idx", "window", "count", "std", "traj"} <= set(pooled)
    assert not zero["pose"].is_cuda
    for k in pooled:          # weight 0 is the pooled per-frame pick: the pose, and with it the trajectory fitted to it, keep their bits
        assert same_bits(zero[k], pooled[k]), k
    bare = infer(model, aggregate="reproj", stride=9, path_weight=0.0, path_scope="video")
    assert set(bare) == {"pose", "idx", "window", "count", "path_cost"} and torch.equal(bare["pose"], zero["pose"])
    assert tuple(zero["path_cost"].shape) == (2, J) and zero["path_cost"].dtype == torch.float64
    held = infer(model, aggregate="reproj", stride=9, path_weight=8.0, path_scope="video", spread="std", trajectory=True)
    assert torch.isfinite(held["pose"]).all() and torch.isfinite(held["path_cost"]).all() and not torch.equal(held["pose"], zero["pose"])
    for k in ("std", "count"):
        assert torch.equal(held[k], pooled[k]), k
    assert set(held) == set(pooled) | {"path_cost"}
    # the pose is a gather of the hypotheses at (window, idx): the hypotheses of the same windows, from the same noise
    from pafuse_amd import harness
    from pafuse_amd.windows import window_starts
    seq_2d, _, cam = sequence(FRAMES)
    starts, _ = window_starts(FRAMES, 27, 9)
    model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
    wb = torch.cat([harness.wb_pose_from_parts(model(harness.cut_windows(seq_2d, starts[lo:lo + 2], 27).to(DEV), None,
                                                     input_2d_flip=harness.cut_windows(harness.flip_2d(seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT),
                                                                                       starts[lo:lo + 2], 27).to(DEV)), dataset()).cpu()
                    for lo in range(0, len(starts), 2)])                                    # [W,T,P,F,J,3]
    w, h = held["window"].long(), held["idx"].long()
    f = torch.arange(FRAMES)[None, :, None] - torch.from_numpy(starts).long()[w]
    assert (w >= 0).all() and (f >= 0).all() and (f < 27).all()
    assert torch.equal(held["pose"], wb[w, torch.arange(2)[:, None, None], h, f, torch.arange(J)[None, None, :]])
    assert ((w[:, 1:] != w[:, :-1]).any())                                                # paths cross from window to window
    un = infer(model, aggregate="reproj", path_weight=8.0, path_scope="video")             # stride None means F: the clips
    assert tuple(un["pose"].shape) == (2, FRAMES, J, 3) and torch.isfinite(un["pose"]).all() and int(un["window"].max()) == 1
    fit = infer(model, aggregate="reproj_fit", stride=9, path_weight=8.0, path_scope="video")
    assert torch.isfinite(fit["pose"]).all() and set(fit) == {"pose", "idx", "window", "count", "path_cost"}
    for kw in ({"hypothesis_chunk": 2}, {"aggregate": "mean"}, {"aggregate": None}, {"path_weight": None}, {"path_scope": "frame"},
               {"path_weight": -1.0}):
        with pytest.raises(ValueError):
            infer(model, **{"aggregate": "reproj", "stride": 9, "path_weight": 1.0, "path_scope": "video", **kw})
    with pytest.raises(ValueError):                           # the clip scope keeps its refusal
        infer(model, aggregate="reproj", stride=9, path_weight=1.0)
    model.num_proposals, keep = 65, model.num_proposals       # the 4 windows of stride 1 all cover frame 3: 260 candidates
    try:
        with pytest.raises(ValueError, match="256"):
            infer(model, aggregate="reproj", stride=1, path_weight=1.0, path_scope="video")
    finally:
        model.num_proposals = keep


def test_batching_does_not_matter(model):
    from pafuse_amd import harness
    from tests.test_hip_windows import noise_per_window
    seq_2d, seq_3d, cam = sequence(FRAMES)
    runs = []
    for batch_size in (1, 4):
        noise_per_window(model)
        try:
            runs.append(harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=batch_size,
                                               aggregate="reproj", cam=cam, traj=seq_3d[:, 0].contiguous(), stride=9, path_weight=8.0,
                                               path_scope="video", spread="std"))
        finally:
            model.noise_fn = None
    a, b = runs
    assert set(a) == set(b) == {"pose", "idx", "window", "count", "std", "path_cost"}
    for k in a:
        assert same_bits(a[k], b[k]), k


def test_evaluate_frames_along_the_video(model):
    from pafuse_amd import harness
    seq_2d, seq_3d, cam = sequence(FRAMES)

    def run(**kw):
        model.noise_fn, model.noise, model.noise_seed = None, "device", SEED
        return harness.evaluate_frames(model, dataset(), seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="reproj",
                                       stride=9, **kw)

    plain, zero, held = run(), run(path_weight=0.0, path_scope="video"), run(path_weight=8.0, path_scope="video")
    for k in plain[0]:
        assert torch.equal(zero[0][k], plain[0][k]) and torch.equal(zero[1][k], plain[1][k]), k
    print("accel sums (synthetic weights: the sizes mean nothing): per-frame pick", plain[0]["accel"].tolist(),
          "video path, weight 8", held[0]["accel"].tolist())
    assert torch.isfinite(held[0]["mpjpe"]).all() and torch.isfinite(held[0]["accel"]).all()
    assert torch.equal(held[1]["accel"], plain[1]["accel"])
    with pytest.raises(ValueError):
        run(path_weight=1.0)                                  # the clip scope takes no stride

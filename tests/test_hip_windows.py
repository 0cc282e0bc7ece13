"""Overlapping windows pooled into one pose per video frame: pose_windows_fold_kernel, spread_windows_fold_kernel and
frames_finish_kernel (pafuse_pose_windows_fold, pafuse_spread_windows_fold, pafuse_frames_finish), torch.ops.pafuse.fold_windows
/ finish_frames, evaluate.accumulate_frames and infer_sequence(stride=...).

What is asserted and why it can be asserted:
  * fold and finish against pafuse_amd.windows, the numpy statement of the same fp64 / fp32 operations in the same order, on
    the SAME batch states (made on the device by pafuse_pose_partials / pafuse_spread_partials, copied to the host): every
    step is an IEEE operation numpy performs identically (the kernels pin contraction off in the fp64 blocks) -> equal bits
    in every field of the frame states and in every output.
  * batching: the windows that cover a frame are visited in ascending order however they are cut into batches -> equal bytes.
    Two hypothesis shards merged by pafuse_pose_combine: the candidate does not depend on the cut; the sums do only through
    fp64 roundings, and on inputs of a 2^-16 grid there are none -> equal bytes too.
  * the kernels that exist: a frame covered by m windows is one clip of m*P hypotheses in (window, hypothesis) order; on grid
    inputs pafuse_pose_partials + pafuse_pose_combine on that clip give the pooled mean, pick and - decoded - (window, hypothesis).
  * infer_sequence: stride = F visits the clips of cut_clips, so with the same noise the per-frame output is today's output
    laid end to end; with stride < F the result is the same for two batch sizes once the noise is a function of the window.
Shapes: P = 3 hypotheses; N just above 2F so that several blocks, a ragged last block and the irregular last window occur.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, same_bits, sequence, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 3
PAD = 5
CAM = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])


def frames_for(F, stride):
    """the smallest N > 2F whose last window is irregular (stride 1 has none)"""
    N = 2 * F + 1
    while stride > 1 and (N - F) % stride == 0:
        N += 1
    return N


def batches_of(W, sizes):
    """W windows cut into batches of `sizes`, repeated as often as needed"""
    out, lo, k = [], 0, 0
    while lo < W:
        hi = min(W, lo + sizes[k % len(sizes)])
        out.append((lo, hi))
        lo, k = hi, k + 1
    return out


class Case:
    """a seeded video of N frames cut into windows: per-window hypotheses on the device, their states there and on the host"""

    def __init__(self, T, F, J, stride, N=None, seed=0, on_grid=False):
        from pafuse_amd import ops
        from pafuse_amd.windows import window_starts
        self.T, self.F, self.J, self.stride = T, F, J, stride
        self.N = N = frames_for(F, stride) if N is None else N
        self.starts, self.valid = window_starts(N, F, stride)
        self.W = W = len(self.starts)
        g = torch.Generator().manual_seed(1000 * seed + 97 * F + 7 * J + stride + T)
        rnd = lambda *s: torch.randn(*s, generator=g)
        if on_grid:
            rnd = lambda *s: torch.randint(-2 ** 15, 2 ** 15, s, generator=g).float() / 2.0 ** 16
        self.pred = (rnd(W, T, P, F, J, 3) * (1.0 if on_grid else 0.25)).contiguous().to(DEV)
        from pafuse_amd.harness import cut_windows
        seq2d = torch.rand(N, J, 2, generator=g) * 2 - 1
        traj = torch.randn(N, 3, generator=g) * 0.1
        traj[:, 2] = 4.0
        self.seq2d, self.seqtraj = seq2d, traj
        self.x2d = cut_windows(seq2d, self.starts, F).contiguous().to(DEV)
        self.traj = cut_windows(traj, self.starts, F).contiguous().to(DEV)
        self.cam = CAM.to(DEV)
        self.conn = tables()[0] if J == 134 else (torch.arange(J, dtype=torch.int32) // 3).to(DEV)
        self.ops = ops

    def pose_state(self, lo, hi, reproj=True, hyp=(0, P)):
        extra = (self.x2d[lo:hi], self.traj[lo:hi], self.cam) if reproj else ()
        return self.ops.pose_partials(self.pred[lo:hi, :, hyp[0]:hyp[1]].contiguous(), self.conn, hyp[0], *extra)

    def spread_state(self, lo, hi):
        return self.ops.spread_partials(self.pred[lo:hi].contiguous(), self.conn, 0)

    def host_states(self, reproj=True):
        """the states of all W windows as numpy arrays (what the device wrote, copied)"""
        a = lambda t: t.cpu().numpy()
        pose = {k: a(v) for k, v in self.ops.pose_views(self.pose_state(0, self.W, reproj), self.W, self.T, self.F, self.J).items()}
        spread = {k: a(v) for k, v in self.ops.spread_views(self.spread_state(0, self.W), self.W, self.T, self.F, self.J).items()}
        return pose, spread

    def device_fold(self, batches, reproj=True, merged_shards=None):
        """-> (frame pose state, frame spread state) as flat buffers with PAD canary doubles behind each"""
        ops, N, T, F, J = self.ops, self.N, self.T, self.F, self.J
        bufs = []
        for spread in (False, True):
            L = ops.frame_state_bytes(N, T, J, spread) // 8
            buf = torch.full((L + PAD,), float("nan"), device=DEV, dtype=torch.float64)
            ops.frame_state(N, T, J, spread=spread, out=buf)
            bufs.append(buf)
        for lo, hi in batches:
            if merged_shards is None:
                st = self.pose_state(lo, hi, reproj)
            else:       # the hypotheses cut into shards, merged by pafuse_pose_combine
                cuts = [(0, merged_shards), (merged_shards, P)]
                rows = torch.stack([self.pose_state(lo, hi, reproj, hyp=c) for c in cuts])
                st = torch.empty_like(rows[0])
                ops.combine_poses(rows, (hi - lo, T, F, J), P, merged=st, want=())
            ops.fold_windows(bufs[0], N, st, (hi - lo, T, F, J), self.starts[lo:hi], self.valid[lo:hi], lo, P)
            ops.fold_spread_windows(bufs[1], N, self.spread_state(lo, hi), (hi - lo, T, F, J), self.starts[lo:hi], self.valid[lo:hi])
        return bufs

    def host_fold(self, batches, reproj=True):
        from pafuse_amd import windows as w
        pose, spread = self.host_states(reproj)
        fp, fs = w.frame_pose_state(self.N, self.T, self.J), w.frame_spread_state(self.N, self.T, self.J)
        for lo, hi in batches:
            w.fold_pose(fp, {k: v[lo:hi] for k, v in pose.items()}, self.starts[lo:hi], self.valid[lo:hi], lo, P)
            w.fold_spread(fs, {k: (v if k == "count" else v[lo:hi]) for k, v in spread.items()}, self.starts[lo:hi], self.valid[lo:hi])
        return fp, fs


def canaries_intact(case, bufs):
    for buf, spread in zip(bufs, (False, True)):
        L = case.ops.frame_state_bytes(case.N, case.T, case.J, spread) // 8
        if not torch.isnan(buf[L:]).all():
            return False
    return True


def assert_state_equals_host(case, bufs, fp, fs, what):
    ops, N, T, J = case.ops, case.N, case.T, case.J
    for k, v in ops.frame_views(bufs[0], N, T, J).items():
        assert same_bits(v.cpu(), torch.from_numpy(fp[k])), (what, "pose", k)
    for k, v in ops.frame_views(bufs[1], N, T, J, spread=True).items():
        assert same_bits(v.cpu(), torch.from_numpy(fs[k])), (what, "spread", k)


# ------------------------------------------------------------------------------------- fold and finish vs the host statement
@pytest.mark.parametrize("stride_of", ["1", "3", "F-1", "F"])
@pytest.mark.parametrize("J", [5, 65, 134])
@pytest.mark.parametrize("F", [5, 27])
@pytest.mark.parametrize("T", [1, 2])
def test_fold_and_finish_equal_the_host_statement(T, F, J, stride_of):
    from pafuse_amd import windows as w
    stride = {"1": 1, "3": 3, "F-1": F - 1, "F": F}[stride_of]
    case = Case(T, F, J, stride, seed=1)
    assert case.N > 2 * F and (stride == 1 or case.starts[-1] - case.starts[-2] != stride)       # the irregular last window
    batches = batches_of(case.W, (2, 3))
    for reproj in (True, False):
        bufs = case.device_fold(batches, reproj)
        assert canaries_intact(case, bufs)
        fp, fs = case.host_fold(batches, reproj)
        assert_state_equals_host(case, bufs, fp, fs, (T, F, J, stride, reproj))
        got = case.ops.finish_frames(case.N, T, J, frame=bufs[0], spread=bufs[1], want=("mean", "pick", "idx", "window", "std", "cov", "count"))
        ref = w.finish(fp, fs)
        for k in ("mean", "pick", "idx", "window", "std", "cov"):
            assert tuple(got[k].shape)[:3] == (T, case.N, J)
            assert same_bits(got[k].cpu(), torch.from_numpy(np.ascontiguousarray(ref[k]))), (T, F, J, stride, reproj, k)
        assert torch.equal(got["count"].cpu(), torch.from_numpy(P * w.coverage(case.N, case.starts, case.valid)))
        assert torch.isfinite(got["mean"]).all() and torch.isfinite(got["std"]).all() and torch.isfinite(got["cov"]).all()
        if reproj:
            assert (got["idx"][:, :, 1:] >= 0).all() and (got["window"][:, :, 1:] >= 0).all()
        else:       # mean-only states hold no candidate: the frame state stays neutral there
            assert (got["idx"] == -1).all() and (got["window"] == -1).all() and torch.isnan(got["pick"]).all()


def test_a_video_shorter_than_a_window_folds_its_real_frames_only():
    from pafuse_amd import windows as w
    case = Case(2, 27, 134, 9, N=11, seed=2)
    assert case.W == 1 and case.valid[0] == 11
    bufs = case.device_fold([(0, 1)])
    fp, fs = case.host_fold([(0, 1)])
    assert_state_equals_host(case, bufs, fp, fs, "N < F")
    assert canaries_intact(case, bufs)
    got = case.ops.finish_frames(case.N, 2, 134, frame=bufs[0], spread=bufs[1], want=("mean", "count"))
    assert tuple(got["mean"].shape) == (2, 11, 134, 3) and (got["count"] == P).all()
    one = case.ops.combine_poses(case.pose_state(0, 1).view(1, -1), (1, 2, 27, 134), P, want=("mean",))["mean"]
    assert torch.equal(got["mean"], one[0, :, :11])


# ------------------------------------------------------------------------------------------------- batching invariance
@pytest.fixture(scope="module")
def grid_case():
    return Case(2, 5, 134, 2, N=14, seed=3, on_grid=True)       # windows 0, 2, 4, 6, 8 and the irregular 9


def test_the_result_does_not_depend_on_the_batching(grid_case):
    case = grid_case
    assert case.W == 6
    whole = case.device_fold([(0, case.W)])
    for sizes in ((1,), (2,), (3,), (1, 2, 3), (4, 2)):
        got = case.device_fold(batches_of(case.W, sizes))
        assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]), sizes
    for cut in (1, 2):        # the merged state of two hypothesis shards folds like the unsharded one (grid inputs: exact sums)
        got = case.device_fold(batches_of(case.W, (2, 3)), merged_shards=cut)
        assert same_bits(got[0], whole[0]), cut


def test_random_inputs_batch_invariant_too():
    case = Case(2, 27, 65, 3, seed=4)
    whole = case.device_fold([(0, case.W)])
    for sizes in ((1,), (5, 2), (7,)):
        got = case.device_fold(batches_of(case.W, sizes))
        assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]), sizes


# ------------------------------------------------------------------------------------- agreement with the kernels that exist
def test_pooling_equals_the_existing_kernels_on_the_concatenated_hypotheses(grid_case):
    from pafuse_amd import ops
    case = grid_case
    T, F, J, N = case.T, case.F, case.J, case.N
    pred = case.pred.clone()
    pred[1, :, :, 0] = pred[0, :, :, 2]            # frame 2 as windows 0 (f = 2) and 1 (f = 0) see it: the same hypotheses, so
    tied = Case.__new__(Case)                      # every error of window 1 ties with one of window 0
    tied.__dict__.update(case.__dict__)
    tied.pred = pred.contiguous()
    bufs = tied.device_fold(batches_of(case.W, (2, 3)))
    got = ops.finish_frames(N, T, J, frame=bufs[0])
    for n in range(N):
        cover = [(b, n - int(s)) for b, (s, v) in enumerate(zip(case.starts, case.valid)) if s <= n < s + v]
        clip = torch.cat([tied.pred[b, :, :, f] for b, f in cover], dim=1)[None, :, :, None].contiguous()   # [1,T,m*P,1,J,3]
        m = len(cover)
        st = ops.pose_partials(clip, case.conn, 0, case.seq2d[n][None, None].contiguous().to(DEV),
                               case.seqtraj[n][None, None].contiguous().to(DEV), case.cam)
        ref = ops.combine_poses(st.view(1, -1), (1, T, 1, J), m * P)
        assert torch.equal(got["mean"][:, n], ref["mean"][0, :, 0]), n
        assert same_bits(got["pick"][:, n], ref["pick"][0, :, 0]), n
        k = ref["idx"][0, :, 0].long()
        has = k >= 0
        win = torch.tensor([b for b, _ in cover], device=DEV)[k.clamp_min(0) // P]
        assert torch.equal(got["idx"][:, n].long(), torch.where(has, k % P, k)), n
        assert torch.equal(got["window"][:, n].long(), torch.where(has, win, k)), n
    assert [b for b, (s, v) in enumerate(zip(case.starts, case.valid)) if s <= 2 < s + v] == [0, 1]
    assert (got["window"][:, 2, 1:] == 0).all()    # the planted tie: the lower window wins
    assert (got["idx"][:, :, 1:] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- bounds
def test_neutral_state_and_untouched_rows(grid_case):
    case = grid_case
    ops, N, T, F, J = case.ops, case.N, case.T, case.F, case.J
    L = ops.frame_state_bytes(N, T, J) // 8
    buf = torch.full((L + PAD,), float("nan"), device=DEV, dtype=torch.float64)
    assert ops.frame_state(N, T, J, out=buf) is buf
    v = ops.frame_views(buf, N, T, J)
    assert (v["sum"] == 0).all() and (v["count"] == 0).all() and torch.isinf(v["e2"]).all() and (v["e2"] > 0).all()
    assert (v["idx"] == -1).all() and (v["win"] == -1).all() and torch.isnan(v["sel"]).all() and torch.isnan(buf[L:]).all()
    sp = ops.frame_state(N, T, J, DEV, spread=True)
    assert sp.numel() * 8 == ops.frame_state_bytes(N, T, J, spread=True) and (sp == 0).all()
    # a batch in the middle of the video: windows 2 and 3 cover frames [4, 11) - nothing else changes, in either state
    before = case.device_fold([(0, 2)])
    after = [b.clone() for b in before]
    lo, hi = 2, 4
    state_p, state_s = case.pose_state(lo, hi), case.spread_state(lo, hi)
    keep_p, keep_s = state_p.clone(), state_s.clone()
    ops.fold_windows(after[0], N, state_p, (2, T, F, J), case.starts[lo:hi], case.valid[lo:hi], lo, P)
    ops.fold_spread_windows(after[1], N, state_s, (2, T, F, J), case.starts[lo:hi], case.valid[lo:hi])
    assert same_bits(state_p, keep_p) and same_bits(state_s, keep_s) and canaries_intact(case, after)
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[4:11] = True
    for spread in (False, True):
        a, b = ops.frame_views(after[spread], N, T, J, spread=spread), ops.frame_views(before[spread], N, T, J, spread=spread)
        for k in a:
            rows = (lambda t: t) if k == "count" else (lambda t: t.transpose(0, 1))     # frames first
            assert same_bits(rows(a[k])[~touched].contiguous(), rows(b[k])[~touched].contiguous()), (spread, k)
        assert not same_bits(a["sum"].transpose(0, 1)[touched].contiguous(), b["sum"].transpose(0, 1)[touched].contiguous())
    from pafuse_amd.windows import coverage
    want = P * coverage(N, case.starts[:4], case.valid[:4])
    assert want.tolist() == [P, P, 2 * P, 2 * P, 3 * P, 2 * P, 3 * P, 2 * P, 2 * P, P, P, 0, 0, 0]
    assert ops.frame_views(after[0], N, T, J)["count"].cpu().tolist() == want.tolist()
    assert ops.frame_views(after[1], N, T, J, spread=True)["count"].cpu().tolist() == want.tolist()


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(grid_case):
    from pafuse_amd import torch_ops  # noqa: F401  (registers torch.ops.pafuse.*)
    case = grid_case
    ops, N, T, F, J = case.ops, case.N, case.T, case.F, case.J
    frame, sframe = ops.frame_state(N, T, J, DEV), ops.frame_state(N, T, J, DEV, spread=True)
    st, ss = case.pose_state(0, 2), case.spread_state(0, 2)
    keep = frame.clone()
    shape = (2, T, F, J)
    bad = [dict(starts=[0, 10], valid=[5, 5]),            # a window reaching past N = 14
           dict(starts=[-1, 2], valid=[5, 5]),
           dict(starts=[0, 2], valid=[5, 6]),             # valid outside 1 .. F
           dict(starts=[0, 2], valid=[0, 5]),
           dict(starts=[2, 0], valid=[5, 5]),             # not strictly ascending
           dict(starts=[2, 2], valid=[5, 5]),
           dict(starts=[0], valid=[5])]                   # not B windows
    for kw in bad:
        with pytest.raises(ValueError):
            ops.fold_windows(frame, N, st, shape, kw["starts"], kw["valid"], 0, P)
        with pytest.raises(ValueError):
            ops.fold_spread_windows(sframe, N, ss, shape, kw["starts"], kw["valid"])
    with pytest.raises(ValueError):                       # short states
        ops.fold_windows(frame[:-1], N, st, shape, [0, 2], [5, 5], 0, P)
    with pytest.raises(ValueError):
        ops.fold_windows(frame, N, st[:-1], shape, [0, 2], [5, 5], 0, P)
    with pytest.raises(ValueError):
        ops.fold_spread_windows(sframe, N, ss[:-1], shape, [0, 2], [5, 5])
    with pytest.raises(ValueError):
        ops.fold_windows(frame, N, st, shape, [0, 2], [5, 5], -1, P)
    with pytest.raises(ValueError):                       # CPU tensors: no fallback
        ops.fold_windows(frame.cpu(), N, st, shape, [0, 2], [5, 5], 0, P)
    with pytest.raises(ValueError):
        ops.fold_windows(frame, N, st.cpu(), shape, [0, 2], [5, 5], 0, P)
    with pytest.raises(ValueError):
        ops.finish_frames(N, T, J, frame=frame.cpu())
    with pytest.raises(ValueError):
        ops.finish_frames(N, T, J, frame=frame, want=("std",))
    with pytest.raises(NotImplementedError):
        torch.ops.pafuse.finish_frames(frame.cpu(), N, T, J)
    assert same_bits(frame, keep) and (sframe == 0).all()    # a refused call wrote nothing
    assert ops.fold_windows(frame, N, st[:0], (0, T, F, J), [], [], 0, P) is frame and same_bits(frame, keep)     # B == 0
    # the library's own refusal, behind the Python checks: the device tables are fine, the host copy is not
    from pafuse_amd import _lib
    lib = _lib.load()
    tab = torch.tensor([[0, 2], [5, 5]], dtype=torch.int32, device=DEV)
    hs, hv = np.array([2, 0], dtype=np.int32), np.array([5, 5], dtype=np.int32)
    rc = lib.pafuse_pose_windows_fold(frame.data_ptr(), frame.numel() * 8, N, st.data_ptr(), st.numel() * 8, 2, T, F, J,
                                      tab[0].data_ptr(), tab[1].data_ptr(), hs.ctypes.data, hv.ctypes.data, 0, P, None)
    assert rc == -1 and b"ascend" in lib.pafuse_last_error()
    torch.cuda.synchronize()
    assert same_bits(frame, keep)
    # an uncovered frame is NaN through the bare entries
    out = ops.finish_frames(N, T, J, frame=frame, spread=sframe)
    assert torch.isnan(out["mean"]).all() and torch.isnan(out["std"]).all() and (out["window"] == -1).all()


def test_torch_ops_are_the_same_entries(grid_case):
    from pafuse_amd import torch_ops  # noqa: F401
    case = grid_case
    ops, N, T, F, J = case.ops, case.N, case.T, case.F, case.J
    want = case.device_fold([(0, case.W)])
    frame = ops.frame_state(N, T, J, DEV)
    assert torch.ops.pafuse.fold_windows(frame, N, case.pose_state(0, case.W), [case.W, T, F, J], case.starts.tolist(),
                                         case.valid.tolist(), 0, P) is None
    L = frame.numel()
    assert same_bits(frame, want[0][:L])
    mean, pick, idx, win, std, cov = torch.ops.pafuse.finish_frames(frame, N, T, J, want[1][:ops.frame_state_bytes(N, T, J, True) // 8].clone())
    ref = ops.finish_frames(N, T, J, frame=want[0], spread=want[1])
    for a, k in ((mean, "mean"), (pick, "pick"), (idx, "idx"), (win, "window"), (std, "std"), (cov, "cov")):
        assert same_bits(a, ref[k]), k
    assert len(torch.ops.pafuse.finish_frames(frame, N, T, J)) == 4


# --------------------------------------------------------------------------------------------------------- infer_sequence
SEED = 4321
F27 = 27


@pytest.fixture(scope="module")
def model():
    from __graft_entry__ import make_model
    return make_model(5, 2, depth=2)[0]


def infer(model, frames, noise="device", **kw):
    """one infer_sequence call on the seeded `frames`-frame video.  noise="device": noise stream v1 from (SEED, call 0) -
    setting noise_seed restarts the call counter, so two runs that cut the video into the same batches draw the same noise"""
    from pafuse_amd import harness
    seq_2d, seq_3d, cam = sequence(frames)
    model.noise_fn = None
    model.noise = noise
    if noise == "device":
        model.noise_seed = SEED
    if kw.get("aggregate") in ("reproj", "reproj_fit"):
        kw.update(cam=cam)
    try:
        return harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, **kw)
    finally:
        model.noise_fn = None


def noise_per_window(model):
    """Injected noise that is a function of the GLOBAL window index.  The device stream cannot be pinned per window with the
    attributes the model has: its key is (noise_seed, noise_call, clip index INSIDE the call), and noise_call advances once
    per batch, so the same window gets other draws when batch_size changes.  noise_fn(k, shape, device) is called for draw
    k = 0, 1, ... of every sampling call (one call per batch here: no hypothesis chunks); draw 0 opens a new batch, whose
    first window is the number of windows drawn before."""
    seen = {"lo": 0, "next": 0}

    def fn(k, shape, device):
        if k == 0:
            seen["lo"], seen["next"] = seen["next"], seen["next"] + shape[0]
        rows = [torch.randn(shape[1:], generator=torch.Generator().manual_seed(7919 * (seen["lo"] + b) + k)) for b in range(shape[0])]
        return torch.stack(rows).to(device)

    model.noise = "torch"
    model.noise_fn = fn


@pytest.mark.parametrize("aggregate", ["mean", "reproj_fit"])
def test_stride_f_is_todays_output_laid_end_to_end(model, aggregate):
    N = 2 * F27
    today = infer(model, N, aggregate=aggregate, batch_size=2)
    got = infer(model, N, aggregate=aggregate, batch_size=2, stride=F27)
    frames = lambda t: t.transpose(0, 1).reshape(t.shape[1], N, *t.shape[3:])       # [clips,T,F,..] -> [T,N,..]
    assert set(got) == {"pose", "count"} | ({"idx", "window"} if aggregate == "reproj_fit" else set())
    pose = today[0] if aggregate == "reproj_fit" else today
    assert tuple(got["pose"].shape) == (2, N, 134, 3) and not got["pose"].is_cuda
    assert torch.equal(got["pose"], frames(pose))
    assert (got["count"] == 5).all() and got["count"].dtype == torch.int64
    if aggregate == "reproj_fit":
        assert torch.equal(got["idx"], frames(today[1]))
        clip = (torch.arange(N) // F27).to(torch.int32)[None, :, None].expand_as(got["window"])
        assert torch.equal(got["window"], torch.where(got["idx"] >= 0, clip, torch.full_like(clip, -1)))
        assert (got["idx"] >= 0).any()


def test_stride_below_f_pools_and_does_not_depend_on_the_batch_size(model):
    from pafuse_amd.windows import coverage, window_starts
    N, stride = 2 * F27 + 3, 13
    starts, valid = window_starts(N, F27, stride)
    assert starts.tolist() == [0, 13, 26, 30]
    runs = []
    for batch_size in (2, 3):
        noise_per_window(model)
        try:
            from pafuse_amd import harness
            seq_2d, _, cam = sequence(N)
            runs.append(harness.infer_sequence(model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=batch_size,
                                               aggregate="reproj_fit", cam=cam, spread="cov", stride=stride))
        finally:
            model.noise_fn = None
    a, b = runs
    assert set(a) == {"pose", "count", "idx", "window", "std", "cov"}
    shapes = {"pose": (2, N, 134, 3), "count": (N,), "idx": (2, N, 134), "window": (2, N, 134), "std": (2, N, 134), "cov": (2, N, 134, 6)}
    for k, shape in shapes.items():
        assert tuple(a[k].shape) == shape and not a[k].is_cuda, k
        assert same_bits(a[k], b[k]), k
    assert torch.equal(a["count"], torch.from_numpy(5 * coverage(N, starts, valid)))
    assert torch.isfinite(a["pose"]).all() and torch.isfinite(a["std"]).all() and torch.isfinite(a["cov"]).all()
    assert (a["window"] < len(starts)).all() and (a["window"] >= -1).all() and (a["idx"] < 5).all()
    picked = a["window"] >= 0
    assert picked.any() and torch.equal(picked, a["idx"] >= 0)
    n = torch.arange(N)[None, :, None].expand_as(a["window"])[picked]
    s = torch.from_numpy(starts).long()[a["window"][picked].long()]
    assert ((s <= n) & (n < s + F27)).all()            # a pick comes from a window that covers its frame


def test_stride_with_the_device_stream_and_mean(model):
    from pafuse_amd.windows import coverage, window_starts
    N = F27 + 22
    starts, valid = window_starts(N, F27, 9)
    assert starts.tolist() == [0, 9, 18, 22]             # two batches of two windows, the last one irregular
    got = infer(model, N, aggregate="mean", batch_size=2, stride=9, spread="std", hypothesis_chunk=2)
    assert set(got) == {"pose", "count", "std"} and tuple(got["pose"].shape) == (2, N, 134, 3)
    assert torch.isfinite(got["pose"]).all() and torch.isfinite(got["std"]).all() and (got["pose"][:, :, 0] == 0).all()
    assert got["count"].tolist() == (5 * coverage(N, starts, valid)).tolist()

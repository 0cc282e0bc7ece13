"""Host side of the per-frame pooling of overlapping windows (no GPU): pafuse_amd.windows - the window table against
harness.cut_clips, and the numpy fold and finish against a brute-force statement -, the refusals of the C ABI that happen
before the first HIP call, and the argument checks of the Python layers.

The brute force gathers, per frame, ALL hypotheses of ALL windows that cover it (in window order, and within a window in
hypothesis order) and takes their fp64 mean, the first minimum of the reprojection errors and the fp64 population
covariance.  Inputs lie on a 2^-16 grid with |x| < 4, so every fp64 sum of them is exact: the pooled mean must be EQUAL
whatever the grouping.  std and cov are compared as tests/test_hip_spread.py compares the spread kernels with fp64: the
fold's arithmetic is fp64 (Chan's rule, relative error of order windows * 2^-52, about 2^-28 of an fp32 step), so std and
the diagonal are equal to the reference rounded to fp32 or adjacent to it, the off-diagonal entries within one step plus
2^-40 * sqrt(c_ii c_jj) (a small covariance is a cancelled sum of terms of that size).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

E_ARG = -1
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
DIAG, OFF = (0, 3, 5), (1, 2, 4)


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------- window_starts
@pytest.mark.parametrize("F", [5, 27])
def test_stride_f_reproduces_cut_clips(F):
    from pafuse_amd import harness
    from pafuse_amd.windows import window_starts
    for N in (1, F - 1, F, F + 1, 2 * F, 2 * F + 5):
        seq = torch.arange(N, dtype=torch.float32).view(N, 1, 1).expand(N, 2, 2).contiguous()
        clips = harness.cut_clips(seq, F)
        starts, valid = window_starts(N, F, F)
        assert starts.dtype == np.int32 and valid.dtype == np.int32
        assert len(starts) == clips.shape[0]
        assert torch.equal(harness.cut_windows(seq, starts, F), clips)
        assert (valid == min(N, F)).all()


@pytest.mark.parametrize("F,stride", [(5, 1), (5, 3), (5, 4), (5, 5), (27, 1), (27, 9), (27, 26), (27, 27)])
def test_every_frame_is_covered_and_counts_are_those_of_the_table(F, stride):
    from pafuse_amd.windows import coverage, window_starts
    for N in (1, F - 1, F, F + 1, 2 * F, 2 * F + 5, 3 * F + 2):
        starts, valid = window_starts(N, F, stride)
        assert (np.diff(starts) > 0).all() and starts[0] == 0
        assert (starts + valid <= N).all() and starts[-1] + valid[-1] == N
        c = coverage(N, starts, valid)
        brute = np.array([sum(1 for s, v in zip(starts, valid) if s <= n < s + v) for n in range(N)])
        assert (c == brute).all() and (c >= 1).all() and c.max() <= -(-F // stride) + 1
        if N >= F:       # regular starts, and at most one irregular last window
            assert (np.diff(starts)[:-1] == stride).all() and (valid == F).all()
        else:
            assert len(starts) == 1 and valid[0] == N


def test_window_starts_refuses():
    from pafuse_amd.windows import window_starts
    for bad in (0, -1, 28, 100):
        with pytest.raises(ValueError):
            window_starts(60, 27, bad)
    with pytest.raises(ValueError):
        window_starts(0, 27, 9)
    with pytest.raises(ValueError):
        window_starts(10, 0, 1)


# ------------------------------------------------------------------------------------ fold and finish, numpy vs brute force
def grid(rng, *shape):
    return (rng.integers(-2 ** 17, 2 ** 17, size=shape) / 2.0 ** 16).astype(np.float32)


def window_states(wb, e2):
    """wb [W,T,P,F,J,3] f32 whole-body hypotheses, e2 [W,T,P,F,J] f32 -> the pose and spread states of the W windows"""
    W, T, P, F, J, _ = wb.shape
    x = wb.astype(np.float64)
    sm = np.zeros((W, T, F, J, 3))
    for h in range(P):
        sm += x[:, :, h]
    first = np.argmin(e2, axis=2)                                      # numpy's argmin is the first minimum
    has = np.isfinite(np.take_along_axis(e2, first[:, :, None], 2)[:, :, 0])
    best = np.where(has, np.take_along_axis(e2, first[:, :, None], 2)[:, :, 0], np.float32(np.inf)).astype(np.float32)
    sel = np.take_along_axis(wb, first[:, :, None, :, :, None].repeat(3, -1), 2)[:, :, 0]
    pose = {"sum": sm, "e2": best, "idx": np.where(has, first, -1).astype(np.int32),
            "sel": np.where(has[..., None], sel, np.float32(np.nan)).astype(np.float32)}
    c = x - (sm / P)[:, :, None]
    m2 = np.stack([(c[..., a] * c[..., b]).sum(axis=2) for a, b in PAIRS], axis=-1)
    return pose, {"sum": sm.copy(), "m2": m2, "count": np.array([float(P)])}


def brute_force(wb, e2, starts, valid, N):
    W, T, P, F, J, _ = wb.shape
    out = {"mean": np.zeros((T, N, J, 3), np.float32), "pick": np.full((T, N, J, 3), np.nan, np.float32),
           "idx": np.full((T, N, J), -1, np.int32), "window": np.full((T, N, J), -1, np.int32),
           "cov": np.zeros((T, N, J, 6)), "std": np.zeros((T, N, J)), "count": np.zeros(N, np.int64)}
    for n in range(N):
        cover = [(w, n - int(s)) for w, (s, v) in enumerate(zip(starts, valid)) if s <= n < s + v]
        hyp = np.concatenate([wb[w, :, :, f] for w, f in cover], axis=1).astype(np.float64)     # [T, m*P, J, 3]
        err = np.concatenate([e2[w, :, :, f] for w, f in cover], axis=1)                        # [T, m*P, J]
        out["count"][n] = hyp.shape[1]
        mean = hyp.mean(axis=1)
        out["mean"][:, n] = mean.astype(np.float32)
        c = hyp - mean[:, None]
        cov = np.stack([(c[..., a] * c[..., b]).mean(axis=1) for a, b in PAIRS], axis=-1)
        out["cov"][:, n], out["std"][:, n] = cov, np.sqrt(cov[..., 0] + cov[..., 3] + cov[..., 5])
        k = np.argmin(err, axis=1)                                                              # first minimum in (window, hypothesis) order
        has = np.isfinite(np.take_along_axis(err, k[:, None], 1)[:, 0])
        win = np.array([w for w, _ in cover])[k // P]
        out["idx"][:, n] = np.where(has, k % P, -1)
        out["window"][:, n] = np.where(has, win, -1)
        sel = np.take_along_axis(hyp, k[:, None, :, None].repeat(3, -1), 1)[:, 0].astype(np.float32)
        out["pick"][:, n] = np.where(has[..., None], sel, np.float32(np.nan))
    return out


def steps_from(got, ref64, slack=None):
    r32 = ref64.astype(np.float32)
    step = (np.nextafter(np.abs(r32), np.float32(np.inf)) - np.abs(r32)).astype(np.float64)
    dist = np.abs(got.astype(np.float64) - r32.astype(np.float64))
    if slack is not None:
        dist = np.clip(dist - slack, 0, None)
    return dist / step


def check_spread(got, ref, what):
    cov, rc = got["cov"], ref["cov"]
    worst = {"std": steps_from(got["std"], ref["std"]).max(), "diag": steps_from(cov[..., DIAG], rc[..., DIAG]).max()}
    slack = np.stack([2.0 ** -40 * np.sqrt(rc[..., DIAG[PAIRS[k][0]]] * rc[..., DIAG[PAIRS[k][1]]]) for k in OFF], axis=-1)
    worst["off"] = steps_from(cov[..., OFF], rc[..., OFF], slack).max()
    print(f"{what}: worst distance from the fp64 brute force in fp32 steps: {worst}")
    assert worst["std"] <= 1.0 and worst["diag"] <= 1.0 and worst["off"] <= 1.0, (what, worst)


@pytest.mark.parametrize("N,F,stride,batches", [(14, 5, 2, (1, 2, 3)), (11, 5, 4, (3,)), (3, 5, 1, (1,)), (12, 5, 5, (2, 1)),
                                                (9, 5, 1, (2, 3))])
def test_numpy_fold_and_finish_equal_the_brute_force(N, F, stride, batches):
    from pafuse_amd import windows as w
    rng = np.random.default_rng(100 * N + stride)
    T, P, J = 2, 3, 4
    starts, valid = w.window_starts(N, F, stride)
    W = len(starts)
    assert sum(batches) == W, (W, batches)
    wb = grid(rng, W, T, P, F, J, 3)
    e2 = rng.integers(0, 6, size=(W, T, P, F, J)).astype(np.float32)     # few values: ties within and across windows
    e2[:, :, :, :, 0] = np.inf                                           # a joint without any candidate
    pose, spread = window_states(wb, e2)
    fp, fs = w.frame_pose_state(N, T, J), w.frame_spread_state(N, T, J)
    lo = 0
    for b in batches:
        cut = lambda s: {k: (v if k == "count" else v[lo:lo + b]) for k, v in s.items()}
        w.fold_pose(fp, cut(pose), starts[lo:lo + b], valid[lo:lo + b], lo, P)
        w.fold_spread(fs, cut(spread), starts[lo:lo + b], valid[lo:lo + b])
        lo += b
    got = w.finish(fp, fs)
    ref = brute_force(wb, e2, starts, valid, N)
    assert (fp["count"] == ref["count"]).all() and (fs["count"] == ref["count"]).all()
    assert (fp["count"] == P * w.coverage(N, starts, valid)).all()
    assert np.array_equal(got["mean"], ref["mean"])
    assert np.array_equal(got["idx"], ref["idx"]) and np.array_equal(got["window"], ref["window"])
    assert np.array_equal(got["pick"], ref["pick"], equal_nan=True)
    assert (got["idx"][..., 0] == -1).all() and np.isnan(got["pick"][..., 0, :]).all()
    check_spread(got, ref, f"N={N} F={F} stride={stride}")
    # the batching does not matter: one window at a time gives the same bytes
    fp1, fs1 = w.frame_pose_state(N, T, J), w.frame_spread_state(N, T, J)
    for b in range(W):
        cut = lambda s: {k: (v if k == "count" else v[b:b + 1]) for k, v in s.items()}
        w.fold_pose(fp1, cut(pose), starts[b:b + 1], valid[b:b + 1], b, P)
        w.fold_spread(fs1, cut(spread), starts[b:b + 1], valid[b:b + 1])
    for k in fp:
        assert fp[k].tobytes() == fp1[k].tobytes(), k
    for k in fs:
        assert fs[k].tobytes() == fs1[k].tobytes(), k


def test_a_tie_across_two_windows_keeps_the_lower_window():
    from pafuse_amd import windows as w
    T, P, F, J, N = 1, 2, 4, 2, 6
    starts, valid = w.window_starts(N, F, 2)                              # 0, 2: frames 2 and 3 are covered twice
    rng = np.random.default_rng(5)
    wb = grid(rng, 2, T, P, F, J, 3)
    e2 = np.full((2, T, P, F, J), 3.0, dtype=np.float32)
    e2[0, 0, 1, 2, 1] = 1.0                                              # frame 2 in window 0 (f = 2), hypothesis 1
    e2[1, 0, 0, 0, 1] = 1.0                                              # frame 2 in window 1 (f = 0), hypothesis 0: a tie
    pose, _ = window_states(wb, e2)
    fp = w.fold_pose(w.frame_pose_state(N, T, J), pose, starts, valid, 0, P)
    got = w.finish(fp)
    assert got["window"][0, 2, 1] == 0 and got["idx"][0, 2, 1] == 1
    assert np.array_equal(got["pick"][0, 2, 1], wb[0, 0, 1, 2, 1])
    assert fp["count"].tolist() == [2, 2, 4, 4, 2, 2]


def test_an_uncovered_frame_is_nan():
    from pafuse_amd import windows as w
    got = w.finish(w.frame_pose_state(3, 1, 2), w.frame_spread_state(3, 1, 2))
    assert np.isnan(got["mean"]).all() and np.isnan(got["std"]).all() and np.isnan(got["cov"]).all()
    assert (got["idx"] == -1).all() and (got["window"] == -1).all()


# --------------------------------------------------------------------------------------------------- the C ABI, no device
def test_state_size_formulas():
    from pafuse_amd import _lib, ops
    L = lib()
    assert _lib.ABI_VERSION == 8 and L.pafuse_abi_version() == 8          # new entries only: no struct changed
    for N, T, J in ((1, 1, 1), (3, 1, 5), (60, 10, 134), (7, 2, 65), (5, 1, 134)):
        r = N * T * J
        assert ops.frame_state_bytes(N, T, J) == (48 * r + 4 * N + 7) // 8 * 8 == L.pafuse_frame_pose_state_bytes(N, T, J)
        assert ops.frame_state_bytes(N, T, J, spread=True) == (9 * r + N) * 8 == L.pafuse_frame_spread_state_bytes(N, T, J)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, -1)):
        assert L.pafuse_frame_pose_state_bytes(*bad) == 0 == L.pafuse_frame_spread_state_bytes(*bad)
        assert ops.frame_state_bytes(*bad) == 0 == ops.frame_state_bytes(*bad, spread=True)


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call: host pointers are never followed as device pointers"""
    L = lib()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    alive = []                                                           # the tables must outlive the calls that read them

    def i32(*v):
        alive.append((C.c_int32 * len(v))(*v))
        return alive[-1]

    s2, v2 = i32(0, 2), i32(3, 3)                                        # N = 5, F = 3: windows [0,3) and [2,5)
    ptr = lambda a: C.addressof(a)
    # frame, frame_bytes, N, state, state_bytes, B, T, F, J, starts, valid, starts_host, valid_host, w0, P_total, stream
    ok = [p, 4096, 5, p + 2048, 2048, 2, 1, 3, 2, p, p, ptr(s2), ptr(v2), 0, 4, None]

    def refused(rc, entry, word=None):
        assert rc == E_ARG
        assert entry in L.pafuse_last_error(), L.pafuse_last_error()
        assert word is None or word in L.pafuse_last_error(), L.pafuse_last_error()

    def both(word=None, **kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        refused(L.pafuse_pose_windows_fold(*a), b"pose_windows_fold", word)
        refused(L.pafuse_spread_windows_fold(*(a[:13] + a[15:])), b"spread_windows_fold", word)

    for i in (2, 5, 6, 7, 8):                                            # N, B, T, F, J negative
        both(**{f"a{i}": -1})
    for i in (2, 6, 7, 8):                                               # N, T, F, J zero
        both(**{f"a{i}": 0})
    for i in (0, 3, 9, 10, 11, 12):                                      # null operands
        both(**{f"a{i}": None})
    both(a1=8)                                                           # short frame state
    both(a4=8)                                                           # short batch state
    both(a0=p + 4)                                                       # misaligned
    both(a3=p + 2052)
    both(b"valid", a12=ptr(i32(3, 0)))                                   # valid outside 1 .. F
    both(b"valid", a12=ptr(i32(4, 3)))
    both(b"covers", a11=ptr(i32(0, 3)))                                  # a window reaching past N
    both(b"covers", a11=ptr(i32(-1, 2)))
    both(b"ascend", a11=ptr(i32(2, 0)))                                  # starts not strictly ascending
    both(b"ascend", a11=ptr(i32(2, 2)))
    a = list(ok)
    a[13] = -1
    refused(L.pafuse_pose_windows_fold(*a), b"pose_windows_fold")        # w0, P_total negative
    a = list(ok)
    a[14] = -1
    refused(L.pafuse_pose_windows_fold(*a), b"pose_windows_fold")
    a = list(ok)
    a[5] = 0                                                             # B == 0 launches nothing (and reads no table)
    a[9] = a[10] = a[11] = a[12] = a[3] = None
    assert L.pafuse_pose_windows_fold(*a) == 0 and L.pafuse_spread_windows_fold(*(a[:13] + a[15:])) == 0

    for init, name in ((L.pafuse_frame_pose_state_init, b"frame_pose_state_init"),
                       (L.pafuse_frame_spread_state_init, b"frame_spread_state_init")):
        refused(init(None, 4096, 5, 1, 2, None), name)
        refused(init(p, 8, 5, 1, 2, None), name)
        refused(init(p + 4, 4096, 5, 1, 2, None), name)
        refused(init(p, 4096, -1, 1, 2, None), name)
        refused(init(p, 4096, 5, 0, 2, None), name)
        refused(init(p, 4096, 5, 1, 0, None), name)

    # frame_state, frame_spread, N, T, J, mean, pick, pick_idx, pick_win, std, cov, stream
    fin = lambda *a: L.pafuse_frames_finish(*a)
    refused(fin(p, p, 5, 1, 2, None, None, None, None, None, None, None), b"frames_finish", b"nothing to write")
    refused(fin(None, p, 5, 1, 2, p, None, None, None, None, None, None), b"frames_finish")        # mean without its state
    refused(fin(p, None, 5, 1, 2, None, None, None, None, p, None, None), b"frames_finish")        # std without its state
    refused(fin(p + 4, None, 5, 1, 2, p, None, None, None, None, None, None), b"frames_finish")
    refused(fin(p, None, -1, 1, 2, p, None, None, None, None, None, None), b"frames_finish")
    refused(fin(p, None, 5, 0, 2, p, None, None, None, None, None, None), b"frames_finish")
    big = 1 << 14
    refused(fin(p, None, big, big, big, p, None, None, None, None, None, None), b"frames_finish", b"grid")


# ----------------------------------------------------------------------------------------------------- the Python layers
def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import evaluate, ops
    z = lambda n: torch.zeros(n, dtype=torch.float64)
    with pytest.raises(ValueError):                                      # CPU tensors: no fallback
        ops.fold_windows(z(1000), 5, z(1000), (2, 1, 3, 2), [0, 2], [3, 3], 0, 4)
    with pytest.raises(ValueError):
        ops.fold_spread_windows(z(1000), 5, z(1000), (2, 1, 3, 2), [0, 2], [3, 3])
    with pytest.raises(ValueError):
        ops.finish_frames(5, 1, 2, frame=z(1000))
    with pytest.raises(ValueError):
        ops.finish_frames(5, 1, 2)
    with pytest.raises(ValueError):
        ops.frame_state(5, 1, 2, device="cpu")
    with pytest.raises(ValueError):
        ops.frame_views(z(10), 5, 1, 2)
    v = ops.frame_views(z(63), 5, 1, 2)                                  # 48 * 10 + 4 * 5 = 500 -> 504 bytes = 63 doubles
    assert tuple(v["sum"].shape) == (1, 5, 2, 3) and tuple(v["win"].shape) == (1, 5, 2) and tuple(v["count"].shape) == (5,)
    assert v["idx"].dtype == torch.int32 and v["e2"].dtype == torch.float32 and tuple(v["sel"].shape) == (1, 5, 2, 3)
    v = ops.frame_views(z(95), 5, 1, 2, spread=True)
    assert tuple(v["m2"].shape) == (1, 5, 2, 6) and tuple(v["count"].shape) == (5,)
    with pytest.raises(ValueError):
        evaluate.accumulate_frames(None, {"mean": z(3)}, [0], [3], 5, 4)


def test_infer_sequence_checks_stride_before_anything_runs():
    from pafuse_amd import harness
    model = types.SimpleNamespace(frames=27)
    seq = torch.zeros(60, 134, 2)
    for bad in (0, -3, 28, 2.5, True):
        with pytest.raises(ValueError, match="stride"):
            harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=bad)
    with pytest.raises(ValueError, match="ragged"):
        harness.infer_sequence(model, None, seq, [], [], aggregate=None, stride=9)
    with pytest.raises(ValueError):
        harness.infer_sequence(model, None, seq, [], [], aggregate="reproj", stride=9)       # no cam / traj
    with pytest.raises(ValueError):
        harness.infer_sequence(model, None, seq, [], [], aggregate="mean", stride=9, conf=torch.ones(60, 134))


def test_torch_op_schemas():
    from pafuse_amd import torch_ops  # noqa: F401  (registers torch.ops.pafuse.*)
    s = str(torch.ops.pafuse.fold_windows.default._schema)
    assert "Tensor(a0!) frame" in s and "[] starts" in s and "num_proposals" in s and s.endswith("-> ()")
    s = str(torch.ops.pafuse.finish_frames.default._schema)
    assert "Tensor? spread=None" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        frame = torch.empty(1000, device="cuda", dtype=torch.float64)
        assert torch.ops.pafuse.fold_windows(frame, 5, torch.empty(100, device="cuda", dtype=torch.float64), [2, 1, 3, 2], [0, 2],
                                             [3, 3], 0, 4) is None
        out = torch.ops.pafuse.finish_frames(frame, 5, 1, 2)
        assert [tuple(t.shape) for t in out] == [(1, 5, 2, 3), (1, 5, 2, 3), (1, 5, 2), (1, 5, 2)]
        assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.int32]
        out = torch.ops.pafuse.finish_frames(frame, 5, 1, 2, frame)
        assert [tuple(t.shape) for t in out[4:]] == [(1, 5, 2), (1, 5, 2, 6)]

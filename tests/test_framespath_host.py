"""posepath.frames_path, the numpy statement of the J-Agg path of a whole video (frames_path_kernel),
and the refusals of pafuse_frames_path that happen before the first HIP call - on the CPU.

At video frame n the candidates are the pairs (window, hypothesis) of all windows that cover n; frames_path scatters them
into the dense [W*P, N] form (a window that does not cover a frame is unavailable there) and calls posepath.path.  The
brute-force cases lie on grids - offsets on quarter-steps, e2 in eighths, weights 0, 1/2 and 8 -, so the sums are exact and
only the square root of a transition rounds: the recursion's normalised total is the plainly added minimum over all paths,
or the double next to it.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pafuse_amd import posepath, windows

INF, NAN = np.float32(np.inf), np.float32(np.nan)
E_ARG, E_SHAPE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def video(N, F, stride, P, T=1, J=2, seed=0, grid=True):
    """-> (e2 [W,T,P,F,J], wb [W,T,P,F,J,3], mean [T,N,J,3], starts, valid): unrelated hypotheses in every window"""
    g = np.random.default_rng(seed)
    starts, valid = windows.window_starts(N, F, stride)
    W = len(starts)
    if grid:
        wb = (g.integers(-8, 9, size=(W, T, P, F, J, 3)) / 4).astype(np.float32)
        mean = (g.integers(-4, 5, size=(T, N, J, 3)) / 4).astype(np.float32)
        e2 = (g.integers(0, 64, size=(W, T, P, F, J)) / 8).astype(np.float32)
    else:
        wb = (g.standard_normal((W, T, P, F, J, 3)) * 0.05).astype(np.float32)
        mean = (g.standard_normal((T, N, J, 3)) * 0.05).astype(np.float32)
        e2 = (g.random((W, T, P, F, J)) * 0.02).astype(np.float32)
    return e2, wb, mean, starts, valid


def covers(window, n, starts, valid):
    s, v = np.asarray(starts)[window], np.asarray(valid)[window]
    return (s <= n) & (n < s + v)


@pytest.mark.parametrize("N,F,stride,P", [(7, 3, 2, 2), (6, 3, 3, 2), (2, 3, 3, 3)])
def test_statement_is_the_brute_force_minimum_on_the_dense_form(N, F, stride, P):
    T, J = 2, 2
    e2, wb, mean, starts, valid = video(N, F, stride, P, T, J, seed=N)
    de, do = posepath.frames_dense(e2, wb, mean, starts, valid, N)
    assert de.shape == (T, J, len(starts) * P, N) and do.shape == de.shape + (3,)
    per_frame = None
    for lam in (0.0, 0.5, 8.0):
        out = posepath.frames_path(e2, wb, mean, starts, valid, N, lam)
        assert out["idx"].shape == (T, N, J) and out["idx"].dtype == np.int32 and out["window"].dtype == np.int32
        assert (out["idx"] >= 0).all() and (out["idx"] < P).all()
        assert covers(out["window"], np.arange(N)[None, :, None], starts, valid).all()     # every pick lies in a covering window
        for t in range(T):
            for j in range(J):
                best, _ = posepath.brute_force(de[t, j], do[t, j], lam)
                g = out["window"][t, :, j] * P + out["idx"][t, :, j]
                plain = posepath.path_cost(de[t, j], do[t, j], lam, g)
                total = out["cost"][t, j]
                assert plain == best, (lam, t, j)                                           # the path attains the minimum
                assert total == best or abs(total - best) <= np.spacing(best), (lam, t, j, total, best)
        if lam == 0.0:
            per_frame = out
            first = np.nanargmin(np.where(np.isfinite(do).all(-1), de, INF), axis=2)         # [T,J,N] the first minimum per frame
            assert np.array_equal(np.moveaxis(first, 1, 2), out["window"] * P + out["idx"])
    if N > 2:
        assert (out["idx"] != per_frame["idx"]).any() or (out["window"] != per_frame["window"]).any()   # the weight moved a pick


def test_one_window_is_the_per_clip_statement():
    N = F = 6
    e2, wb, mean, starts, valid = video(N, F, F, 4, T=2, J=3, seed=11, grid=False)
    e2[0, 1, :, 2, 1] = INF                                                # an unobserved (frame, joint)
    assert len(starts) == 1
    for lam in (0.0, 0.5, 8.0):
        got = posepath.frames_path(e2, wb, mean, starts, valid, N, lam)
        want = posepath.pick(wb, e2, lam, mean[None])
        assert np.array_equal(got["idx"], want["idx"][0]) and (got["window"] == 0).all()
        assert np.array_equal(got["pick"], want["pick"][0]) and np.array_equal(got["e2"], want["e2"][0])
        assert np.array_equal(got["cost"], want["cost"][0])
    assert got["e2"][1, 2, 1] == INF and got["idx"][1, 2, 1] >= 0


def test_a_short_video_ignores_the_padding():
    N, F, P = 2, 3, 3
    e2, wb, mean, starts, valid = video(N, F, 3, P, seed=5)
    assert list(valid) == [2]
    a = posepath.frames_path(e2, wb, mean, starts, valid, N, 0.5)
    e2[:, :, :, 2:], wb[:, :, :, 2:] = NAN, NAN                            # what lies in the padded frame is never read
    b = posepath.frames_path(e2, wb, mean, starts, valid, N, 0.5)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("N,F,stride,P", [(30, 27, 27, 5), (70, 9, 4, 20)])
def test_zero_weight_is_the_fold_of_the_windows(N, F, stride, P):
    T, J = 1, 3
    e2, wb, mean, starts, valid = video(N, F, stride, P, T, J, seed=N, grid=False)
    W = len(starts)
    s0, s1 = int(starts[0]), int(starts[1])
    tie = e2[0, :, :, s1 - s0].min(axis=1)                                 # [T,J]
    e2[1, :, :, 0] = np.maximum(e2[1, :, :, 0], tie[:, None] * 2)
    e2[1, :, 2, 0] = tie                                                   # a tie across two windows: the lower window keeps it
    at = np.argmin(e2, axis=2)                                             # [W,T,F,J] the first minimum within a window
    state = {"sum": np.zeros((W, T, F, J, 3)), "e2": np.take_along_axis(e2, at[:, :, None], axis=2)[:, :, 0],
             "idx": at.astype(np.int32), "sel": np.take_along_axis(wb, at[:, :, None, ..., None], axis=2)[:, :, 0]}
    fin = windows.finish(windows.fold_pose(windows.frame_pose_state(N, T, J), state, starts, valid, 0, P))
    got = posepath.frames_path(e2, wb, mean, starts, valid, N, 0.0)
    assert (fin["idx"] >= 0).all()
    assert np.array_equal(got["idx"], fin["idx"]) and np.array_equal(got["window"], fin["window"])
    assert np.array_equal(got["pick"], fin["pick"])
    assert (got["window"][:, s1] == 0).all()
    moved = posepath.frames_path(e2, wb, mean, starts, valid, N, 8.0)
    assert (moved["idx"] != got["idx"]).any() and (np.diff(moved["window"], axis=1) != 0).any()


def seam(F=4):
    """two clips at stride = F, P = 3: clip 1 holds clip 0's constant offsets under the permutation (0,1,2) -> (2,0,1); all e2
    equal, except that frame 0 prefers hypothesis 1"""
    g = np.random.default_rng(21)
    P, T, J, N = 3, 1, 2, 2 * F
    base = (g.integers(-8, 9, size=(P, J, 3)) / 4).astype(np.float32)
    base[1], base[2] = base[0] + np.float32(0.5), base[0] - np.float32(0.75)          # three distinct offsets per joint
    wb = np.empty((2, T, P, F, J, 3), dtype=np.float32)
    wb[0] = base[None, :, None]
    wb[1] = base[[2, 0, 1]][None, :, None]
    e2 = np.ones((2, T, P, F, J), dtype=np.float32)
    e2[0, :, 1, 0] = 0.5
    starts, valid = windows.window_starts(N, F, F)
    return e2, wb, starts, valid, N


def test_the_path_keeps_the_geometric_hypothesis_across_a_seam():
    e2, wb, starts, valid, N = seam()
    F = e2.shape[3]
    for lam in (0.5, 8.0):
        out = posepath.frames_path(e2, wb, None, starts, valid, N, lam)
        assert (out["window"][:, :F] == 0).all() and (out["window"][:, F:] == 1).all()
        assert (out["idx"][:, :F] == 1).all() and (out["idx"][:, F:] == 2).all()
        assert (out["cost"] == 0.5 + (N - 1) * 1.0).all()                  # no jump: exactly the sum of the unaries
        assert np.array_equal(out["pick"][:, F:], np.broadcast_to(out["pick"][:, :1], out["pick"][:, F:].shape))
        alone = posepath.pick(wb[1:], e2[1:], lam)                         # the per-clip statement knows nothing of clip 0
        assert (alone["idx"] == 0).all()


def test_a_nan_removes_only_its_candidate_and_frame():
    N, F, stride, P = 6, 4, 2, 3
    e2, wb, mean, starts, valid = video(N, F, stride, P, T=1, J=2, seed=31, grid=False)
    e2[:, :, 2], wb[:, :, 2] = 0, 0                                        # hypothesis 2 of every window rests at 0 and fits
    clean = posepath.frames_path(e2, wb, None, starts, valid, N, 0.01)
    assert (clean["idx"] == 2).all()
    n = 3
    assert clean["window"][0, n, 0] == 0 and list(starts) == [0, 2]
    for plant in ("wb", "e2"):
        w2, v2 = wb.copy(), e2.copy()
        if plant == "wb":
            w2[0, 0, 2, n, 0, 1] = NAN
        else:
            v2[0, 0, 2, n, 0] = NAN
        out = posepath.frames_path(v2, w2, None, starts, valid, N, 0.01)
        assert out["window"][0, n, 0] == 1 and out["idx"][0, n, 0] == 2, plant      # the next window's candidate, there only
        keep = np.ones((1, N, 2), dtype=bool)
        keep[0, n, 0] = False
        for k in ("idx", "window", "e2"):
            assert np.array_equal(out[k][keep], clean[k][keep]), (plant, k)
        assert np.isfinite(out["cost"]).all()


def test_a_frame_without_a_candidate_kills_its_lines_and_no_others():
    N, F, stride, P = 7, 3, 2, 2
    e2, wb, mean, starts, valid = video(N, F, stride, P, T=2, J=3, seed=41, grid=False)
    clean = posepath.frames_path(e2, wb, mean, starts, valid, N, 0.5)
    n, j = 2, 1                                                            # frame 2 lies in windows 0 and 1
    for w in range(len(starts)):
        if covers(w, n, starts, valid):
            wb[w, :, :, n - int(starts[w]), j, 0] = NAN
    out = posepath.frames_path(e2, wb, mean, starts, valid, N, 0.5)
    assert (out["idx"][:, :, j] == -1).all() and (out["window"][:, :, j] == -1).all() and np.isnan(out["pick"][:, :, j]).all()
    assert np.isinf(out["e2"][:, :, j]).all() and np.isnan(out["cost"][:, j]).all()
    others = [k for k in range(3) if k != j]
    for k in ("idx", "window", "pick", "e2"):
        assert np.array_equal(out[k][:, :, others], clean[k][:, :, others]), k
    assert np.array_equal(out["cost"][:, others], clean["cost"][:, others])
    e2[:, :, :, :, 0] = INF                                                # a line that is never observed has no path either
    out = posepath.frames_path(e2, wb, mean, starts, valid, N, 0.5)
    assert (out["idx"][:, :, 0] == -1).all() and np.isnan(out["cost"][:, 0]).all() and (out["idx"][:, :, 2] >= 0).all()


# --------------------------------------------------------------------------------------------------- the C ABI, no device
def test_the_entry_is_declared_exported_and_bound():
    from pafuse_amd import _lib, ops, torch_ops  # noqa: F401
    L = lib()
    with open(os.path.join(ROOT, "include", "pafuse_hip.h")) as f:
        header = f.read()
    for name in ("pafuse_frames_path", "pafuse_frames_path_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES and hasattr(L, name)
    assert _lib.ABI_VERSION == 8 and L.pafuse_abi_version() == 8          # new entries only: no struct changed
    assert callable(ops.frames_path) and callable(ops.frames_path_workspace_bytes)
    import torch
    s = str(torch.ops.pafuse.frames_path.default._schema)
    assert "[] starts" in s and "[] valid" in s and "Tensor? mean=None" in s and s.endswith("-> Tensor[]")


def tables(*rows):
    keep = [(C.c_int32 * len(r))(*r) for r in rows]
    return keep, [C.addressof(k) for k in keep]


def test_workspace_formula():
    from pafuse_amd import ops
    L = lib()
    up8 = lambda n: (n + 7) // 8 * 8
    # N, T, J, P, (F, stride) -> coverage
    for N, T, J, P, F, stride, cover in ((70, 1, 134, 20, 9, 4, 3), (7, 2, 5, 2, 3, 2, 2), (11, 1, 5, 64, 4, 1, 4),
                                         (30, 1, 5, 5, 27, 27, 2), (2, 3, 5, 3, 3, 3, 1)):
        starts, valid = windows.window_starts(N, F, stride)
        assert int(windows.coverage(N, starts, valid).max()) == cover
        keep, (s, v) = tables(starts.tolist(), valid.tolist())
        want = up8(T * J * N * cover * P)
        assert L.pafuse_frames_path_workspace_bytes(N, T, J, P, len(starts), s, v) == want
        assert ops.frames_path_workspace_bytes(N, T, J, P, starts, valid) == want
    keep, (s, v, gap, late, down, same, short, zero) = tables([0, 2], [3, 3], [0, 4], [1, 2], [0, 1], [0, 0], [3, 1], [3, 0])
    ok = (5, 1, 2, 4, 2, s, v)
    assert L.pafuse_frames_path_workspace_bytes(*ok) == up8(5 * 2 * 2 * 4)
    for i in range(5):                                                    # N, T, J, P, W zero or negative
        for bad in (0, -1):
            a = list(ok)
            a[i] = bad
            assert L.pafuse_frames_path_workspace_bytes(*a) == 0, (i, bad)
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, None, v) == 0 == L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, s, None)
    assert L.pafuse_frames_path_workspace_bytes(7, 1, 2, 4, 2, gap, v) == 0           # a gap
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, late, v) == 0          # does not start at 0
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, same, v) == 0          # starts not strictly ascending
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, down, short) == 0      # ends descend
    assert L.pafuse_frames_path_workspace_bytes(6, 1, 2, 4, 2, s, v) == 0             # the last window ends before N
    assert L.pafuse_frames_path_workspace_bytes(4, 1, 2, 4, 2, s, v) == 0             # ... or behind it
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, s, zero) == 0          # valid < 1
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 129, 2, s, v) == 0           # K = 258 > 256
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 128, 2, s, v) == up8(5 * 2 * 256)
    assert ops.frames_path_workspace_bytes(5, 1, 2, 129, [0, 2], [3, 3]) == 0 == ops.frames_path_workspace_bytes(7, 1, 2, 4, [0, 4], [3, 3])


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call: host pointers are never followed as device pointers"""
    L = lib()
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    keep, (s, v, gap, late, down, same, short, zero, four) = tables([0, 2], [3, 3], [0, 4], [1, 2], [0, 1], [0, 0], [3, 1], [3, 0], [4, 3])
    # 0 pred, 1 x2d, 2 root, 3 per_h, 4 cam, 5 conf, 6 conn, 7 mean, 8 weight, 9 W, 10 T, 11 P, 12 F, 13 J, 14 N, 15 starts, 16 valid,
    # 17 starts_host, 18 valid_host, 19 pick, 20 pick_idx, 21 pick_win, 22 pick_e2, 23 cost, 24 workspace, 25 workspace_bytes, 26 stream
    ok = [p, p, p, 0, p, None, p, None, 0.5, 2, 1, 4, 3, 2, 5, p, p, s, v, p, p, p, None, None, p, 4096, None]
    assert L.pafuse_frames_path_workspace_bytes(5, 1, 2, 4, 2, s, v) == 80 <= 4096

    def refused(word=None, rc=E_ARG, **kw):
        a = list(ok)
        for i, val in kw.items():
            a[int(i[1:])] = val
        assert L.pafuse_frames_path(*a) == rc, kw
        assert b"frames_path" in L.pafuse_last_error(), L.pafuse_last_error()
        assert word is None or word in L.pafuse_last_error(), L.pafuse_last_error()

    for i in (9, 10, 11, 12, 13, 14):                                     # W, T, P, F, J, N zero (W == 0: no video) or negative
        refused(**{f"a{i}": 0})
        refused(**{f"a{i}": -1})
    for i in (0, 1, 2, 4, 6, 15, 16, 17, 18, 19, 20, 21):                 # null required operands
        refused(**{f"a{i}": None})
    for bad in (-0.5, float("inf"), float("nan")):
        refused(b"weight", a8=bad)
    refused(b"workspace", a24=None)
    refused(b"workspace", a25=72)                                         # short
    refused(b"workspace", a24=p + 4)                                      # misaligned
    refused(b"cost", a23=p + 4)
    refused(b"gap", a14=7, a17=gap)
    refused(b"frame 0", a17=late)
    refused(b"ascend", a17=same)
    refused(b"descend", a17=down, a18=short)
    refused(b"end at frame N", a14=6)
    refused(b"past", a14=4)
    refused(b"valid", a18=zero)
    refused(b"valid", a14=6, a18=four)                                    # valid > F
    refused(b"256", rc=E_SHAPE, a11=129)                                  # K = 2 * 129
    refused(b"256", rc=E_SHAPE, a11=257, a9=1, a14=3, a17=s, a18=v)       # one window of 257 hypotheses


def test_python_layers_refuse_before_touching_the_device():
    import torch
    from pafuse_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError):                                       # CPU tensors: no fallback
        ops.frames_path(z(2, 1, 4, 3, 2, 3), z(2, dtype=torch.int32), z(5, 2, 2), z(5, 3), z(9), 0.5, [0, 2], [3, 3])
    with pytest.raises(ValueError, match="want"):
        ops.frames_path(z(2, 1, 4, 3, 2, 3), z(2, dtype=torch.int32), z(5, 2, 2), z(5, 3), z(9), 0.5, [0, 2], [3, 3], want=("mean",))

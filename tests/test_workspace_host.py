"""The workspace helper (pafuse_amd._lib.workspace / workspace_policy), the guarded-arena policy of the tests
(tests/workspace_policy.py) and the size functions of the C ABI, on the host: no device is touched.

The size functions (`pafuse_*_bytes`) are plain host arithmetic.  Each is held to two properties over a small lattice around a
base point: it does not decrease when one size argument grows (a carve that shrinks while its kernels' rows grow is a carve
that is too small somewhere), and it returns 0 where the header says it refuses - a size below the smallest it accepts - instead
of a wrapped product."""
import ctypes as C

import numpy as np
import pytest
import torch

from pafuse_amd import _lib
from tests.workspace_policy import FILLS, GUARD, SENTINEL, GuardedArenas


# ------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("nbytes,dtype,numel", [(1000, None, 1000), (0, None, 1), (1, torch.uint8, 1), (48, torch.float64, 6),
                                                (0, torch.float64, 1), (13, torch.float64, 2)])
def test_without_a_policy_the_helper_is_torch_empty(nbytes, dtype, numel, monkeypatch):
    assert _lib._workspace_policy is None
    calls = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    t = _lib.workspace(nbytes, "cpu", "test") if dtype is None else _lib.workspace(nbytes, "cpu", "test", dtype)
    want = torch.uint8 if dtype is None else dtype
    assert calls == [((numel,), {"dtype": want, "device": "cpu"})]        # one plain torch.empty, nothing else
    assert t.dtype == want and t.dim() == 1 and t.is_contiguous() and t.numel() == numel
    assert t.numel() * t.element_size() == (max(nbytes, 1) if want == torch.uint8 else (max(nbytes, 1) + 7) // 8 * 8)


def test_the_helper_takes_two_dtypes_only():
    with pytest.raises(ValueError):
        _lib.workspace(16, "cpu", "test", torch.float32)


def test_policy_is_restored_on_exit_and_on_exception():
    outer, inner = GuardedArenas("zeros"), GuardedArenas("ones")
    assert _lib._workspace_policy is None
    with _lib.workspace_policy(outer) as got:
        assert got is outer and _lib._workspace_policy is outer
        with _lib.workspace_policy(inner):
            assert _lib._workspace_policy is inner
            _lib.workspace(8, "cpu", "inner")
        assert _lib._workspace_policy is outer                     # the PREVIOUS policy, not none
        with pytest.raises(RuntimeError, match="boom"):
            with _lib.workspace_policy(inner):
                raise RuntimeError("boom")
        assert _lib._workspace_policy is outer
        _lib.workspace(8, "cpu", "outer")
    assert _lib._workspace_policy is None
    assert outer.names() == ["outer"] and inner.names() == ["inner"]
    with pytest.raises(ValueError, match="boom"):
        with _lib.workspace_policy(outer):
            raise ValueError("boom")
    assert _lib._workspace_policy is None


def test_a_policy_must_return_the_bytes_asked_for():
    with _lib.workspace_policy(lambda nbytes, device, what, dtype: torch.empty(nbytes + 1, dtype=torch.uint8)):
        with pytest.raises(_lib.PafuseError, match="'short'"):
            _lib.workspace(16, "cpu", "short")


# ------------------------------------------------------------------------------------------------ the policy
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes,dtype", [(1, torch.uint8), (1000, torch.uint8), (4096, torch.uint8), (48, torch.float64)])
def test_view_is_exact_aligned_and_filled(fill, nbytes, dtype):
    arenas = GuardedArenas(fill)
    with _lib.workspace_policy(arenas):
        t = _lib.workspace(nbytes, "cpu", "site", dtype)
    assert t.numel() * t.element_size() == nbytes and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 256 == 0
    (what, whole, n), = arenas.arenas
    assert (what, n) == ("site", nbytes) and whole.numel() == GUARD + nbytes + GUARD and whole.dtype == torch.uint8
    assert t.data_ptr() == whole.data_ptr() + GUARD                       # a view INTO the remembered tensor
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + nbytes:] == SENTINEL).all())
    inner = whole[GUARD:GUARD + nbytes]
    if fill == "zeros":
        assert bool((inner == 0).all())
    elif fill == "ones":
        assert bool((inner == 0xFF).all())
        if dtype == torch.float64:
            assert bool(torch.isnan(t).all())
    else:
        again = GuardedArenas(fill)
        with _lib.workspace_policy(again):
            _lib.workspace(nbytes, "cpu", "site", dtype)
        assert torch.equal(again.arenas[0][1], whole)                     # seeded: the same bytes every time
        assert nbytes < 1000 or len(inner.unique()) > 200                 # ... and really bytes of every kind
    arenas.check()
    assert arenas.names() == ["site"]


def test_random_fill_holds_the_values_it_promises():
    arenas = GuardedArenas("random")
    with _lib.workspace_policy(arenas):
        t = _lib.workspace(1 << 16, "cpu", "site")
    f = t.view(torch.float32)
    assert bool(torch.isnan(f).any()) and bool(torch.isinf(f.view(torch.float16)).any())
    assert bool(((f != 0) & (f.abs() < 1.1754944e-38)).any())           # denormals
    assert int(t.view(torch.int32).abs().max()) > 1 << 30


@pytest.mark.parametrize("side,offset", [("below", -1), ("above", 0), ("below", -GUARD), ("above", GUARD - 1)])
def test_the_detector_detects(side, offset):
    """one byte written just outside the view - through the remembered whole tensor, as a kernel's stray store would land -
    fails check() with the arena's name, the side and the offset; the last interior byte is the library's to write"""
    nbytes = 1000
    arenas = GuardedArenas("zeros")
    with _lib.workspace_policy(arenas):
        _lib.workspace(64, "cpu", "first")
        view = _lib.workspace(nbytes, "cpu", "second")
    _, whole, _ = arenas.arenas[1]
    view[nbytes - 1] = 0x5A                                               # the last interior byte: allowed
    view[0] = 0x5A
    arenas.check()
    at = offset if side == "below" else nbytes + offset                   # relative to the view
    whole[GUARD + at] = 0x5A
    with pytest.raises(AssertionError) as err:
        arenas.check()
    msg = str(err.value)
    assert "'second'" in msg and f"guard {side} the view" in msg and f"offset {at} of the view" in msg, msg
    whole[GUARD + at] = SENTINEL
    arenas.check()


def test_a_stray_store_of_the_sentinel_byte_itself_is_not_seen():
    """what the guard cannot see is stated, not hidden: a stray store of the byte 0xA5 itself leaves no trace (1 value in 256)"""
    arenas = GuardedArenas("ones")
    with _lib.workspace_policy(arenas):
        _lib.workspace(8, "cpu", "site")
    arenas.arenas[0][1][GUARD + 8] = SENTINEL
    arenas.check()


# ------------------------------------------------------------------------------------------------ the size functions
def _weights(F=27, J=24, Cw=384, depth=2, heads=8, mode=0):
    w = _lib.MixSTE2Weights()
    w.frames, w.joints, w.channels, w.depth, w.heads, w.in_chans, w.operand_bf16 = F, J, Cw, depth, heads, 5, mode
    return w


def _config(F=27, flip=1, mode=0):
    cfg = _lib.D3DPConfig()
    parts = ((24, 384), (68, 224), (42, 256))
    cfg.num_parts, cfg.num_kps, cfg.frames, cfg.flip = len(parts), sum(j for j, _ in parts), F, flip
    for i, (J, Cw) in enumerate(parts):
        w = _weights(F, J, Cw, 1, 8, mode)
        C.memmove(C.byref(cfg.part[i]), C.byref(w), C.sizeof(w))
    return cfg


def _windows(N, W):
    """W windows of equal stride over N frames, each reaching its successor's start or beyond"""
    starts = np.linspace(0, max(N - 1, 0), W, endpoint=False).astype(np.int32) if W > 0 else np.zeros(0, np.int32)
    starts = np.unique(starts)
    ends = np.append(starts[1:] + 1, N).clip(max=N) if len(starts) else starts
    ends[-1:] = N
    return starts, (ends - starts).astype(np.int32)


def _frames_path_bytes(lib, N, T, J, P, W):
    if min(N, W) < 1:
        return lib.pafuse_frames_path_workspace_bytes(N, T, J, P, W, None, None)
    s, v = _windows(N, min(W, N))
    return lib.pafuse_frames_path_workspace_bytes(N, T, J, P, len(s), s.ctypes.data, v.ctypes.data)


# name -> (callable(lib, *sizes), base sizes, per size: the largest value at which the function returns 0 - None: the argument is
#          a mode or has no refusal -, per size: the lattice it is monotone over)
UP = (1, 2, 3, 5, 8, 27, 64)
SIZE_FUNCTIONS = {
    "split_weights": (lambda lib, N, K: lib.pafuse_split_weights_bytes(N, K), (384, 384), (0, 0), ((32, 64, 224, 384, 768), (32, 64, 224, 384, 768))),
    "split_image_f16x2": (lambda lib, N, K: lib.pafuse_split_image_bytes(N, K, 4), (384, 384), (0, 0), ((32, 64, 224, 384, 768), (32, 64, 224, 384, 768))),
    "split_image_x": (lambda lib, N, K: lib.pafuse_split_image_bytes(N, K, 8), (384, 384), (0, 0), ((32, 64, 224, 384, 768), (32, 64, 224, 384, 768))),
    "train_unit": (lambda lib, M, N, K: lib.pafuse_train_unit_bytes(M, N, K), (105, 256, 128), (-1, -1, -1),
                   ((0, 1, 31, 32, 33, 105, 127, 128, 129, 1000), (0, 64, 128, 384), (0, 64, 128, 384))),
    "train_head_grad": (lambda lib, M, Cw: lib.pafuse_train_head_grad_bytes(M, Cw), (105, 128), (-1, 0), ((0, 1, 63, 64, 65, 105, 1000, 5000), (64, 128, 224, 384))),
    "train_patch_grad": (lambda lib, B, F, J, Cw: lib.pafuse_train_patch_grad_bytes(B, F, J, Cw), (2, 5, 7, 128), (-1, -1, -1, 0),
                         ((0,) + UP, (0,) + UP, (0,) + UP, (64, 128, 224, 384))),
    **{f"train_group_sum_{m}": (lambda lib, B, F, J, Cw, m=m: lib.pafuse_train_group_sum_bytes(m, B, F, J, Cw), (2, 5, 7, 128), (-1, -1, -1, 0),
                                ((0,) + UP, (0,) + UP, (0,) + UP, (64, 128, 224, 384))) for m in (0, 1, 2)},
    "block_workspace": (lambda lib, rows, Cw: lib.pafuse_block_workspace_bytes(rows, Cw), (243, 384), (0, 0), ((1, 2, 7, 8, 9, 243, 1836), (64, 128, 224, 256, 384))),
    **{f"mixste2_workspace_mode{mode}": (lambda lib, B, P, F, J, Cw, mode=mode: lib.pafuse_mixste2_workspace_bytes(C.byref(_weights(F, J, Cw, 1, 8, mode)), B, P),
                                         (1, 3, 27, 24, 384), (0, 0, 0, 0, 0), (UP, UP, UP, UP, (64, 128, 224, 256, 384))) for mode in (0, 2, 3, 4)},
    **{f"d3dp_workspace_mode{mode}_flip{flip}": (lambda lib, B, P, F, mode=mode, flip=flip: lib.pafuse_d3dp_workspace_bytes(C.byref(_config(F, flip, mode)), B, P),
                                                 (2, 3, 27), (0, 0, 0), (UP, UP, UP)) for mode in (0, 3, 4) for flip in (0, 1)},
    "mixste2_train": (lambda lib, B, F, J, Cw, depth: lib.pafuse_mixste2_train_bytes(C.byref(_weights(F, J, Cw, depth, 8, 0)), B),
                      (2, 5, 7, 128, 1), (0, 0, 0, None, 0), (UP, UP, UP, (64, 128, 224, 256, 384), (1, 2, 8))),
    "hypothesis_partials": (lambda lib, *a: lib.pafuse_hypothesis_partials_bytes(*a), (2, 2, 5, 5, 134, 3), (-1, 0, -1, 0, 0, 0),
                            ((0,) + UP, UP, (0,) + UP, UP, UP + (134,), (1, 2, 3, 4))),
    "hypothesis_partials_workspace": (lambda lib, *a: lib.pafuse_hypothesis_partials_workspace_bytes(*a), (2, 2, 5, 5, 134, 3), (-1, 0, -1, 0, 0, 0),
                                      ((0,) + UP, UP, (0,) + UP, UP, UP + (134,), (1, 2, 3, 4))),
    "procrustes_partials": (lambda lib, *a: lib.pafuse_procrustes_partials_bytes(*a), (2, 2, 5, 5, 134), (-1, 0, -1, 0, 0),
                            ((0,) + UP, UP, (0,) + UP, UP, UP + (134,))),
    "procrustes_partials_workspace": (lambda lib, *a: lib.pafuse_procrustes_partials_workspace_bytes(*a), (2, 2, 5, 5, 134), (-1, 0, -1, 0, 0),
                                      ((0,) + UP, UP, (0,) + UP, UP, UP + (134,))),
    "pose_partials": (lambda lib, *a: lib.pafuse_pose_partials_bytes(*a), (2, 2, 5, 134), (-1, 0, 0, 0), ((0,) + UP, UP, UP, UP + (134,))),
    "spread_partials": (lambda lib, *a: lib.pafuse_spread_partials_bytes(*a), (2, 2, 5, 134), (0, 0, 0, 0), (UP, UP, UP, UP + (134,))),
    "frame_pose_state": (lambda lib, *a: lib.pafuse_frame_pose_state_bytes(*a), (9, 2, 5), (0, 0, 0), (UP, UP, UP)),
    "frame_spread_state": (lambda lib, *a: lib.pafuse_frame_spread_state_bytes(*a), (9, 2, 5), (0, 0, 0), (UP, UP, UP)),
    "pose_path_workspace": (lambda lib, *a: lib.pafuse_pose_path_workspace_bytes(*a), (2, 2, 5, 5, 134), (-1, 0, 0, 0, 0),
                            ((0,) + UP, UP, UP + (65, 256), UP + (256,), UP + (134,))),
    "frames_path_workspace": (_frames_path_bytes, (9, 2, 5, 5, 3), (0, 0, 0, 0, 0), ((3, 5, 8, 9, 27, 64), UP, UP, (1, 2, 3, 5, 8, 27), (1, 2, 3))),
    "detections_screen_workspace": (lambda lib, *a: lib.pafuse_detections_screen_workspace_bytes(*a), (9, 5), (0, 0), (UP, UP + (134,))),
    "tracks_workspace": (lambda lib, *a: lib.pafuse_tracks_workspace_bytes(*a), (9, 7, 5, 3), (0, 0, 0, 0), (UP, UP, UP, (1, 2, 3, 4, 8))),
    "pose_smooth_workspace": (lambda lib, *a: lib.pafuse_pose_smooth_workspace_bytes(*a), (2, 9, 5), (0, 0, 0), (UP, UP, UP)),
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_every_size_function_of_the_abi_is_covered():
    """a `*_bytes` entry added to the C ABI must be added to the table above (pafuse_linear_weight_grad_bytes takes no size)"""
    named = {n for n in _lib.SIGNATURES if n.endswith("_bytes")} - {"pafuse_linear_weight_grad_bytes"}
    covered = {"pafuse_split_weights_bytes", "pafuse_split_image_bytes", "pafuse_train_unit_bytes", "pafuse_train_head_grad_bytes",
               "pafuse_train_patch_grad_bytes", "pafuse_train_group_sum_bytes", "pafuse_block_workspace_bytes", "pafuse_mixste2_workspace_bytes",
               "pafuse_d3dp_workspace_bytes", "pafuse_mixste2_train_bytes", "pafuse_hypothesis_partials_bytes",
               "pafuse_hypothesis_partials_workspace_bytes", "pafuse_procrustes_partials_bytes", "pafuse_procrustes_partials_workspace_bytes",
               "pafuse_pose_partials_bytes", "pafuse_spread_partials_bytes", "pafuse_frame_pose_state_bytes", "pafuse_frame_spread_state_bytes",
               "pafuse_pose_path_workspace_bytes", "pafuse_frames_path_workspace_bytes", "pafuse_detections_screen_workspace_bytes",
               "pafuse_tracks_workspace_bytes", "pafuse_pose_smooth_workspace_bytes"}
    assert named == covered, named ^ covered


@pytest.mark.parametrize("name", sorted(SIZE_FUNCTIONS))
def test_size_functions_are_monotone_and_refuse_with_zero(lib, name):
    fn, base, floors, lattices = SIZE_FUNCTIONS[name]
    at_base = int(fn(lib, *base))
    assert 0 < at_base < 1 << 40, (name, at_base)
    for k, (floor, lattice) in enumerate(zip(floors, lattices)):
        sizes = [int(fn(lib, *base[:k], v, *base[k + 1:])) for v in lattice]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (name, k, list(zip(lattice, sizes)))
        assert all(s < 1 << 40 for s in sizes), (name, k, sizes)           # (a wrapped product would be astronomically large)
        if floor is None:
            continue
        assert sizes[0] > 0 or lattice[0] <= floor + 1, (name, k, lattice[0], sizes[0])
        for v in (floor, floor - 1, -(1 << 20)):
            got = int(fn(lib, *base[:k], v, *base[k + 1:]))
            assert got == 0, f"{name}: size argument {k} = {v} gives {got} bytes, not the refusal 0"


def test_weight_grad_partials_have_one_size(lib):
    assert 0 < lib.pafuse_linear_weight_grad_bytes() < 1 << 30


@pytest.mark.parametrize("mode", [0, 3, 4])
@pytest.mark.parametrize("B,P,F,J,Cw", [(1, 3, 27, 68, 224), (1, 1, 27, 68, 224), (1, 3, 27, 24, 384), (2, 3, 27, 42, 256), (1, 3, 5, 7, 128), (1, 1, 2, 1, 64),
                                        (1, 1, 1, 7, 224)])
def test_denoiser_arena_is_its_carve(lib, B, P, F, J, Cw, mode):
    """the size pafuse_mixste2_workspace_bytes returns IS the sum of the sub-buffers of carve_part (x | xn | o | wide | temb | pred
    | stats, each rounded up to 256 bytes), restated here: not a byte of slack that would hide a tile tail, and none missing"""
    up = lambda n: (n + 255) // 256 * 256
    eb, rows = (6 if mode == 4 else 4), B * P * F * J
    want = up(rows * Cw * 4) + 2 * up(rows * Cw * eb) + up(rows * 3 * Cw * 4) + up(B * Cw * 4) + up(rows * 12) + up(rows * 8)
    got = lib.pafuse_mixste2_workspace_bytes(C.byref(_weights(F, J, Cw, 1, 8, mode)), B, P)
    assert got == want, (got, want)

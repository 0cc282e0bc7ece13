"""Every composite entry point of the C ABI works inside a caller-owned byte arena (pafuse_amd._lib.workspace).  Each flow below
runs once as the library runs it (torch.empty: the reference bits) and once under each fill of tests/workspace_policy.py -
zeros, every byte 0xFF (NaN as fp32 / fp16 / bf16 / fp64, -1 as an integer), seeded random bytes - inside 4096-byte guard bands:

  * names():  the flow asked the helper for the arenas expected of it (a flow that allocates nothing fails),
  * check():  no guard byte changed - no tile tail, lane offset or image row was written outside the bytes `*_bytes()` asked for,
  * every output has the reference's bits under every fill - no byte of an arena is read before the call wrote it,
  * in 'f16x2' no range error is raised over a dirty arena (the flag word lives in the arena; the library clears it),
  * where a flow can repeat on the SAME, now dirty, arena (graph replay, the unit entries) it gives the same bits again.

The shapes are the smallest at which the tile tails exist: row counts no tile of 16 .. 128 rows divides, at the part widths
384 / 224 / 256 and at 128, through the carve x | xn | o | wide | temb | pred | stats (no slack between neighbours at these widths).

A (shape, mode) pair the library has no kernels for is refused loudly by design (pafuse_mode_supported == 0: 'f16x2' outside the
widths 224 / 256 / 384; 'bf16x3_images' falls back to 'bf16x3' in images.effective_mode before that): such a pair asserts the
refusal, with and without a policy, and nothing else.

THE INDEX-HOLDING WORKSPACES, read kernel by kernel before the first run (pafuse_amd/csrc/kernels.hpp) - every word is written by
the call before it is read or used as an index; none needed a fix:

  pose_path_kernel / frames_path_kernel: one recursion, path_forward and path_backtrace, on two candidate sources
                      back[line, n, s], one byte (the clip kernel: n = f, s = h, k_n = K = P at every frame; the video kernel:
                      k_n = P * the windows covering n).  Forward pass: at every frame n >= 1 lane l stores
                      back[n*K + r*64 + l] for every slot s = r*64 + l < k_n (R = ceil(K / 64) rounds cover K <= 256) - the value in
                      [0, k_(n-1)), 0 when no predecessor wins.  Backtrace: s is the exact-zero slot of the last frame (< k_(N-1)),
                      then the byte back[n*K + s] for n >= 1 only (n == 0 takes 0), which is < k_(n-1): a slot stored at n - 1 (or of
                      frame 0, whose row is neither stored nor read).  A dead line returns before the backtrace.  A workgroup fence
                      stands between the wave's stores and its loads.  The "observed" marks the backtrace reads are not in the arena:
                      the clip kernel keeps them in registers, the video kernel in the OUTPUT pick_e2 - written for every n in the
                      forward pass before they are read, and neither written nor read when pick_e2 is null.
  track_nodes_kernel  size[n, k]: every (n, k) stored (NaN: absent) before track_links / track_path read it (stream order).
  track_links_kernel  gain[n, g, ka, kb]: every element stored - the absent branch stores the whole column over its lanes, the
                      other branch stores each ka from lane 0.
  track_path_kernel   used[n, k]: cleared for all N*K at entry, fence, then read.  back[n, k, 2] (lag g, predecessor a): per round
                      every node of the frames n0 .. N-1 is stored (g = 0 for a node that is not alive) before the fence; both walks
                      start at (endn, endb) with endn >= n0 and stop where g == 0 or g > n - n0, so a node before n0 (not stored
                      with a seed) is never read; a is a set bit of the live mask, < K.  The score ring s_S is LDS, not arena: row
                      (n - g) & 7 is read for g <= min(G, n - n0) only, at the set bits of live[g-1] - rows and lanes stored before.
  detections_residual_kernel / _scale_kernel / _screen_finish_kernel
                      tau[j]: stored for every j by the scale kernel before the first SCREEN_FIRST / acc_next launch reads it
                      (pass 1 reads neither).  e_1, e_self, e_cross: stored for every (n, j) by the launch that names them (e_cross
                      only with a mirror table, and read only then).  The acc double buffer: a pass stores acc_next[e] for EVERY e
                      unconditionally; pass p reads acc[(p-1) & 1] (SCREEN_STORED from pass 3 on; pass 2 forms acc_1 from e_1 and
                      tau) and writes acc[p & 1] - never the buffer it reads; the evaluation and the finish read the last one
                      written (passes = 1: none, acc_1 is formed again).  A byte is tested != 0 only, never used as an index.
  pose_precision_kernel  W[row, 6] fp64: a row that takes no part stores a NaN in W[0] only; pose_smooth_kernel tests W[0] before
                      it reads the other five.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pafuse_amd import _lib
from pafuse_amd._lib import PRECISIONS
from tests.golden import golden_util as gu
from tests.test_hip_partials import same_bits
from tests.workspace_policy import FILLS, GuardedArenas

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("f32", "bf16x3", "bf16x3_images", "f16x2")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _normal(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(DEV)


def tensors(out):
    """the output tensors of a flow, by name"""
    if isinstance(out, torch.Tensor):
        return {"out": out}
    if isinstance(out, dict):
        return {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}
    return {str(i): v for i, v in enumerate(out) if isinstance(v, torch.Tensor)}


def assert_same(got, ref, label):
    got, ref = tensors(got), tensors(ref)
    assert got.keys() == ref.keys() and ref, (label, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape and same_bits(got[k].contiguous(), ref[k].contiguous()), \
            f"{label}: output '{k}' depends on what the arena held ({int((got[k] != ref[k]).sum())} of {ref[k].numel()} values differ)"


def guarded(flow, names, label, repeat=False, between=None):
    """flow() with no policy, then under each fill: the arenas asked for, the guards, the bits; repeat=True: a second call that
    gets the first call's arenas back as they were left (between(): run between the fills, e.g. to drop a captured graph)"""
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in tensors(flow()).items()}
    for fill in FILLS:
        if between:
            between()
        arenas = GuardedArenas(fill, reuse=repeat)
        with _lib.workspace_policy(arenas):
            got = flow()
            assert arenas.names() == list(names), (label, fill, arenas.names())
            arenas.check()
            assert_same(got, ref, (label, fill))
            if repeat:
                made = len(arenas.arenas)
                again = flow()
                assert arenas.names() == list(names) * 2 and len(arenas.arenas) == made, (label, fill, arenas.names())
                arenas.check()
                assert_same(again, ref, (label, fill, "second call on the dirty arena"))
    if between:
        between()
    assert _lib._workspace_policy is None


def refused(flow, label):
    """a (shape, mode) without kernels: the same loud refusal whatever the arenas hold"""
    for fill in (None,) + FILLS:
        arenas = GuardedArenas(fill or "zeros")
        with pytest.raises(_lib.PafuseError):
            if fill is None:
                flow()
            else:
                with _lib.workspace_policy(arenas):
                    flow()
        arenas.check()


# ------------------------------------------------------------------------------------------------ denoiser forward
def denoiser(F, J, Cw, depth=1, heads=8, seed=91, train=False):
    import pafuse_amd
    m = pafuse_amd.MixSTE2(num_frame=F, num_joints=J, in_chans=5, embed_dim_ratio=Cw, depth=depth, num_heads=heads,
                           drop_path_rate=0.0, is_train=train)
    sd = {k: gu.seeded_tensor(k, v.shape, seed) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    m = m.to(DEV)
    return (m.train() if train else m.eval()), sd


def ran_mode(precision, Cw, heads, J, F):
    """(the mode images.effective_mode hands the library, whether the library has kernels for it at this shape)"""
    from pafuse_amd.images import effective_mode
    mode = effective_mode(PRECISIONS[precision], Cw, 2 * Cw, heads, J, F)
    return mode, bool(_lib.load().pafuse_mode_supported(mode, Cw, 2 * Cw, heads, J, F))


@pytest.mark.parametrize("F,J,Cw", [(27, 24, 384), (27, 68, 224), (27, 42, 256), (5, 7, 128)])
def test_denoiser_forward(F, J, Cw):
    """MixSTE2 in eval, depth 1, B = 1, P = 3, in the four modes, through the module and through torch.ops.pafuse.mixste_eval.
    At width 224 M = 5508: M C eb is a multiple of 256 for eb = 4 and 6 and M is no multiple of 8."""
    from pafuse_amd import torch_ops  # noqa: F401  (registers torch.ops.pafuse)
    B, P = 1, 3
    m, _ = denoiser(F, J, Cw)
    x2d, x3d = _normal((B, F, J, 2), 1, 0.5), _normal((B, P, F, J, 3), 2).clamp(-1.1, 1.1)
    t = torch.tensor([499], device=DEV)
    ran = {}
    for precision in MODES:
        m.operand_bf16 = PRECISIONS[precision]
        mode, ok = ran_mode(precision, Cw, 8, J, F)
        ran[precision] = (mode, ok)
        op = lambda: torch.ops.pafuse.mixste_eval(x2d, x3d, t, list(m.parameters()), 1, 8, precision)
        if not ok:
            refused(lambda: m(x2d, x3d, t), (F, J, Cw, precision))
            refused(op, (F, J, Cw, precision, "op"))
            continue
        guarded(lambda: m(x2d, x3d, t), ["mixste2_forward"], (F, J, Cw, precision))
        guarded(op, ["mixste2_forward"], (F, J, Cw, precision, "op"))
        assert same_bits(op(), m(x2d, x3d, t))
    wide = Cw in (224, 256, 384)
    assert ran["f32"] == (0, True) and ran["bf16x3"] == (2, True) and ran["f16x2"] == (3, wide), ran
    assert ran["bf16x3_images"][1] and ran["bf16x3_images"][0] in ((4, 2) if wide else (2,)), ran
    print(f"denoiser forward (F, J, C) = {(F, J, Cw)}: modes handed to the library {ran}")


# ------------------------------------------------------------------------------------------------ block forward
@pytest.mark.parametrize("S,L,Cw", [(9, 27, 384), (3, 68, 224)])
def test_block_forward(S, L, Cw):
    from pafuse_amd import ops
    m, _ = denoiser(L, L, Cw)
    blk = m.STEblocks[0]
    x = _normal((S, L, Cw), 3)
    for precision in MODES:
        guarded(lambda: ops.block_forward(blk, x, heads=8, precision=precision), ["block_forward"], (S, L, Cw, precision))
        guarded(lambda: torch.ops.pafuse.block(x, list(blk.parameters()), 8, precision), ["block_forward"], (S, L, Cw, precision, "op"))


# ------------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def loop_models():
    from __graft_entry__ import make_model
    return {flip: make_model(3, 2, seed=77, flip=flip)[0] for flip in (True, False)}


def loop_flow(model, B, flip, noises=None):
    x2d, x2f = gu.synthetic_inputs_2d(B=B, seed=1234)
    x2d, x2f = x2d.to(DEV), x2f.to(DEV)
    if noises is not None:
        noises = [n.to(DEV) for n in noises]
        model.noise_fn = lambda k, shape, device: noises[k]

    def flow():
        if noises is None:
            model.noise_seed = 5          # (also rewinds noise_call: the same draws in every run)
        return model(x2d, None, input_2d_flip=x2f if flip else None)
    return flow


@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
@pytest.mark.parametrize("precision", MODES)
def test_loop(loop_models, precision, flip):
    """make_model(P = 3, T = 2), B = 2: the (part, hypothesis-group) lanes on the side streams, everything on one stream, and the
    part-by-part schedule - row offsets of the lanes into the shared sub-buffers; 'f16x2' raises no range error over 0xFF bytes"""
    model = loop_models[flip]
    model.precision = precision
    flow = loop_flow(model, 2, flip, gu.synthetic_noises(B=2, P=3, n=2, seed=3))
    try:
        for n_aux, part_by_part in ((2, False), (0, False), (0, True)):
            model.n_aux_streams, model.part_by_part_launches = n_aux, part_by_part
            guarded(flow, ["d3dp_sample"], (precision, flip, n_aux, part_by_part))
    finally:
        model.n_aux_streams, model.part_by_part_launches, model.noise_fn = 2, False, None


def test_loop_graph_replayed_twice(loop_models):
    """use_graph in 'bf16x3': the static arena is filled before the capture begins; the second replay runs on the arena the first
    one left"""
    model = loop_models[True]
    model.precision = "bf16x3"
    flow = loop_flow(model, 2, True, gu.synthetic_noises(B=2, P=3, n=2, seed=3))
    eager = flow().clone()
    model.use_graph = True
    try:
        for fill in FILLS:
            model._graphs.clear()
            arenas = GuardedArenas(fill)
            with _lib.workspace_policy(arenas):
                first = flow()
                second = flow()
            assert arenas.names() == ["d3dp_sample_graph"], arenas.names()      # one static arena, asked for once
            arenas.check()
            assert same_bits(first, eager) and same_bits(second, eager), fill
    finally:
        model._graphs.clear()
        model.use_graph, model.noise_fn = False, None


def test_loop_device_noise(loop_models):
    model = loop_models[True]
    model.precision = "bf16x3"
    model.noise = "device"
    try:
        guarded(loop_flow(model, 2, True), ["d3dp_sample"], "device noise")
    finally:
        model.noise = "torch"


def test_loop_through_the_torch_op(loop_models):
    from pafuse_amd import torch_ops as to
    model = loop_models[True]
    model.precision = "bf16x3_images"
    noises = [n.to(DEV) for n in gu.synthetic_noises(B=1, P=3, n=2, seed=12)]
    i2d, i2f = (v.to(DEV) for v in gu.synthetic_inputs_2d(B=1))
    args = to.ddim_loop_args(model)
    guarded(lambda: torch.ops.pafuse.ddim_loop(i2d, i2f, torch.stack(noises), *args, "bf16x3_images"), ["d3dp_sample"], "ddim_loop op")


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("F,J,Cw,depth,B,with_drop", [(5, 7, 128, 1, 2, True), (27, 68, 224, 1, 1, False)])
def test_training_forward_and_backward(F, J, Cw, depth, B, with_drop, precision):
    """one forward and backward through the `saved` arena: the output and every gradient.  with_drop: a DropPath table
    [2 depth, 2, B max(F, J)] is handed to the step (at depth 1 the module's own rates are all 0 and it draws none, so the
    table is made here: factors 0 or 1 / keep, keep = 0.5)"""
    from pafuse_amd.mixste2 import _TrainFunction
    m, _ = denoiser(F, J, Cw, depth=depth, train=True, seed=93)
    m.operand_bf16 = PRECISIONS[precision]
    x2d, x3d = _normal((B, F, J, 2), 4, 0.5), _normal((B, F, J, 3), 5)
    t = torch.tensor([17, 803][:B], device=DEV)
    dout = _normal((B, F, J, 3), 6)
    drop = None
    if with_drop:
        drop = ((torch.rand(2 * depth, 2, B * max(F, J), generator=_gen(7)) < 0.5).float() * 2.0).to(DEV)
    params = list(m.parameters())

    def flow():
        for p in params:
            p.grad = None
        out = _TrainFunction.apply(m, x2d, x3d, t, drop, *params) if with_drop else m(x2d, x3d, t)
        out.backward(dout)
        res = {"out": out.detach()}
        res.update({n: p.grad for n, p in m.named_parameters()})
        assert all(g is not None for g in res.values())
        return res
    guarded(flow, ["mixste2_train"], (F, J, Cw, depth, B, precision))


# ------------------------------------------------------------------------------------------------ unit training entries
def _lnb():
    from pafuse_amd import ops
    M, Cw = 9, 64
    dy, x, w, add = _normal((M, Cw), 10), _normal((M, Cw), 11), _normal((Cw,), 12), _normal((M, Cw), 13)
    drop = (torch.rand(3, generator=_gen(14)) < 0.5).float().to(DEV) * 2
    return lambda: ops.layer_norm_backward(dy, x, w, 1e-6, add=add, drop=drop, seq_map=(0, 1, 3), scaled=True, branch=True), ["train_unit"]


def _dx():
    from pafuse_amd import ops
    M, N, K = 129, 192, 64      # qkv of width 64; M >= 128: the split products on the M16 image of W^T, one row past the tile
    dy, w, u = _normal((M, N), 15), _normal((N, K), 16), _normal((M, K), 17)
    return lambda: {p + str(s): ops.linear_input_grad(dy, w, u, p, s) for p, s in (("bf16x3", 0), ("bf16x3", 1), ("f32", 0))}, ["train_unit"] * 3


def _fwd():
    from pafuse_amd import ops
    M, N, K = 129, 128, 64      # fc1 of width 64
    x, w, b = _normal((M, K), 18), _normal((N, K), 19), _normal((N,), 20)

    def flow():
        out = {}
        for p in ("bf16x3", "f32"):
            out[p + "_u"], out[p + "_h"] = ops.linear_train(x, w, b, True, p)
        return out
    return flow, ["train_unit"] * 2


def _gelu():
    from pafuse_amd import ops
    M, N = 37, 448
    u, dh = _normal((M, N), 21, 1.5), _normal((M, N), 22)
    return lambda: dict(zip(("du", "db"), ops.gelu_backward(u, dh))), ["train_unit"]


def _dw():
    from pafuse_amd import ops
    M, N, K = 389, 768, 256
    dy, x = _normal((M, N), 23), _normal((M, K), 24)

    def flow():
        out = {}
        for p in ("bf16x3", "f32"):
            out[p + "_dw"], out[p + "_db"] = ops.linear_weight_grad(dy, x, p)
        return out
    return flow, ["linear_weight_grad"] * 2


def _head():
    from pafuse_amd import ops
    M, Cw = 65, 64
    dout, hn, hw = _normal((M, 3), 25), _normal((M, Cw), 26), _normal((3, Cw), 27)
    return lambda: ops.train_head_grad(dout, hn, hw), ["train_rim"]


def _patch():
    from pafuse_amd import ops
    B, F, J, Cw = 3, 5, 7, 64
    x2d, x3d, g = _normal((B, F, J, 2), 28), _normal((B, F, J, 3), 29), _normal((B, F, J, Cw), 30)
    return lambda: ops.train_patch_grad(x2d, x3d, g), ["train_rim"]


def _group():
    from pafuse_amd import ops
    x = _normal((2, 3, 5, 64), 31)
    return lambda: {str(mode): ops.train_group_sum(x, mode) for mode in (0, 1, 2)}, ["train_rim"] * 3


UNITS = {"layer_norm_backward": _lnb, "linear_input_grad": _dx, "linear_train": _fwd, "gelu_backward": _gelu, "linear_weight_grad": _dw,
         "train_head_grad": _head, "train_patch_grad": _patch, "train_group_sum": _group}


@pytest.mark.parametrize("name", list(UNITS))
def test_unit_training_entries(name):
    """one shape each from the smallest parametrisation of the entry's own tests; the second call gets the first call's arena
    back dirty (partial sums a call adds into without clearing them would double there)"""
    flow, names = UNITS[name]()
    guarded(flow, names, name, repeat=True)


# ------------------------------------------------------------------------------------------------ evaluation, per-frame
def _eval_inputs(B, T, P, F, seed):
    from tests.test_hip_partials import inputs, tables
    pred, gt, x2d, traj, cam = inputs(B, T, P, F, seed, special=False)
    return pred, gt, x2d, traj, cam, tables()


def _partials():
    from pafuse_amd import ops
    B, T, P, F, J = 2, 2, 5, 5, 134
    pred, gt, x2d, traj, cam, (conn, pbroot, part) = _eval_inputs(B, T, P, F, 40)

    def flow():
        state = ops.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, 4, 0)
        merged = torch.empty(5 * B * T * F * J, device=DEV, dtype=torch.float64)
        out = ops.combine_partials(state[None], gt, conn, pbroot, (B, T, F, J), P, merged=merged)
        out["state"], out["merged"] = state, merged
        return out
    return flow, ["hypothesis_partials"]


def _procrustes():
    from pafuse_amd import ops
    B, T, P, F, J = 2, 2, 5, 5, 134
    pred, gt, x2d, traj, cam, (conn, _, _) = _eval_inputs(B, T, P, F, 41)

    def flow():
        state = ops.procrustes_partials(pred, gt, x2d, traj, cam, conn, 0)
        sums = ops.pose_partials(pred, conn, 0)
        out = ops.combine_procrustes(state[None], (B, T, F, J), P, sums=sums[None], gt=gt, conn=conn)
        out["state"] = state
        return out
    return flow, ["procrustes_partials"]


def _pose_path(P):
    def make():
        from pafuse_amd import ops
        pred, gt, x2d, traj, cam, (conn, _, _) = _eval_inputs(1, 2, P, 5, 42 + P)
        return lambda: ops.pose_path(pred, conn, x2d, traj, cam, 0.5, want=("pick", "idx", "e2", "cost")), ["pose_path"]
    return make


def _frames_path():
    from pafuse_amd import ops
    from tests.test_hip_partials import tables
    W, T, P, F, J = 3, 2, 5, 5, 134
    starts, valid = [0, 3, 6], [5, 5, 5]                 # three windows, each overlapping the next by two frames: N = 11
    N = 11
    conn = tables()[0]
    g = _gen(50)
    base = torch.randn(N, J, 3, generator=g) * 0.3
    pred = torch.stack([base[s:s + F] for s in starts])[:, None, None] + torch.randn(W, T, P, F, J, 3, generator=g) * 0.05
    x2d = torch.rand(N, J, 2, generator=g) * 2 - 1
    root = torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    pred, x2d, root, cam = (v.contiguous().to(DEV) for v in (pred, x2d, root, cam))
    return lambda: ops.frames_path(pred, conn, x2d, root, cam, 0.5, starts, valid, want=("pick", "idx", "window", "e2", "cost")), ["frames_path"]


def _smooth():
    from pafuse_amd import ops
    from tests.test_hip_pose_smooth import smooth_inputs
    pose, cov = (torch.from_numpy(v).to(DEV) for v in smooth_inputs(2, 9, 5, 3, seed=60))
    return lambda: dict(zip(("out", "code"), ops.smooth_poses(pose, cov, 3, want_code=True))), ["smooth_poses"]


def _screen():
    from pafuse_amd import ops
    from tests.test_hip_detections_screen import inputs
    x, conf, mirror = inputs(5, 9, seed=61)
    x, conf = x.to(DEV), conf.to(DEV)
    return lambda: ops.screen_detections(x, conf, mirror=mirror, radius=3), ["screen_detections"]


def _tracks():
    from pafuse_amd import ops
    from tests.test_hip_tracks import inputs
    x, c = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in inputs(5, 9, 7, seed=62))
    want = ("x2d", "conf", "assign", "score", "frames", "gain", "size")
    return lambda: ops.track_people(x, c, tracks=3, max_gap=3, support=2, min_frames=2, want=want), ["track_people"]


def _tracks_seeded():
    from pafuse_amd import ops
    from tests.test_hip_tracks import inputs
    hx, hc = inputs(5, 9, 7, seed=62)
    seed = tuple(int(v) for v in np.argwhere((hc > 0).sum(-1) >= 2)[5])       # a present candidate in the middle of the video
    x, c = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (hx, hc))
    return lambda: ops.track_people(x, c, tracks=1, seed=seed, max_gap=3, support=2, min_frames=2), ["track_people"] * 2


FRAME_FLOWS = {"hypothesis_partials": _partials, "procrustes_partials": _procrustes, "pose_path_P5": _pose_path(5), "pose_path_P65": _pose_path(65),
               "frames_path": _frames_path, "smooth_poses": _smooth, "screen_detections": _screen, "track_people": _tracks,
               "track_people_seeded": _tracks_seeded}


@pytest.mark.parametrize("name", list(FRAME_FLOWS))
def test_evaluation_and_per_frame_workspaces(name):
    """B = 2, T = 2, P = 5, F = 5, J = 134 for the partials; pose_path at P = 5 and 65 (one and two hypotheses per lane);
    frames_path on three overlapping windows; smooth_poses N = 9, J = 5, r = 3; screen_detections N = 9, J = 5; track_people
    (N, K, G) = (9, 7, 3), and with a seed (two halves, the second on the reversed video: back-pointers before the seed's
    frame are never stored).  Back-pointers, counters and flags of 0xFF / random bytes: see the module docstring."""
    flow, names = FRAME_FLOWS[name]()
    guarded(flow, names, name, repeat=True)


def test_caller_supplied_workspaces_are_used_as_given():
    """a `workspace=` argument does not go through the helper"""
    from pafuse_amd import ops
    pred, gt, x2d, traj, cam, (conn, _, _) = _eval_inputs(1, 1, 5, 5, 70)
    ref = ops.pose_path(pred, conn, x2d, traj, cam, 0.5)
    mine = torch.full((ops.pose_path_workspace_bytes(1, 1, 5, 5, 134) + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    arenas = GuardedArenas("ones")
    with _lib.workspace_policy(arenas):
        got = ops.pose_path(pred, conn, x2d, traj, cam, 0.5, workspace=mine)
    assert arenas.names() == [] and bool((mine[-64:] == 0xFF).all())
    assert_same(got, ref, "caller's workspace")

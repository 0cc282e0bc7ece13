"""PyTorch-ROCm custom ops over the C ABI: ``torch.ops.pafuse.*`` ("native surface").

Importing this module registers, for the HIP device only (a CPU tensor gets torch's "no kernel for backend" error -
there is no fallback), with fake-tensor shape functions so the ops trace under ``torch.export`` / ``torch.compile``:

  pafuse::linear(x, weight, bias, gelu)                    nn.Linear (+ exact GELU)       common/mixste.py:30-43,54,57
  pafuse::layer_norm(x, weight, bias, eps)                 nn.LayerNorm                   common/mixste.py:96,101
  pafuse::attention(qkv, heads, seq_len, joints)           softmax(q k^T d^-1/2) v        common/mixste.py:65-79
  pafuse::block(x, weights[12], heads, precision)          Block.forward on [S,L,C]       common/mixste.py:113-116
  pafuse::mixste_eval(x2d, x3d, t, weights, depth, heads, precision)  MixSTE2.forward, eval  common/mixste.py:278-298
  pafuse::ddim_loop(..., precision)                        D3DP.ddim_sample[_flip]        common/diffusionpose.py:227-316
  pafuse::hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, num_parts, h0)   one shard's partial reductions
  pafuse::combine_partials(states, gt, conn, pbroot, T, num_proposals)   jbest, pagg, jagg, paggpb from W states   main_h3wb.py:327-362
  pafuse::procrustes_partials(pred, gt, x2d, traj, cam, conn, h0)   one shard's Protocol #2 state
  pafuse::procrustes_combine(states, sums, gt, conn, T, num_proposals)   jbest, pagg, jagg, pick from W states   main_h3wb.py:381-395
  pafuse::aggregate_poses(pred, conn, x2d?, traj?, cam?)  P-Agg mean pose, J-Agg pose and its hypothesis index, one shard
  pafuse::aggregate_poses_fit(pred, conn, x2d, cam, conf?)  the same without a trajectory: roots fitted on the device; + tfit
  pafuse::pose_path(pred, conn, x2d, root, cam, weight, conf?, mean?)   J-Agg coherent in time: per joint a path through the hypotheses
  pafuse::frames_path(pred, conn, x2d, root, cam, weight, starts, valid, conf?, mean?)   that path along a whole video, across its windows
  pafuse::fold_windows(frame!, N, state, shape, starts, valid, w0, num_proposals)   a batch of overlapping windows into the frame state
  pafuse::finish_frames(frame, N, T, J, spread?)          one pose per video frame: mean, pick, idx, window (+ std, cov)
  pafuse::fit_trajectory(pose, x2d, cam, conf?)           the camera-space root of that pose: traj, wsum, resid per (t, frame)
  pafuse::smooth_trajectory(traj, weight?, radius)        a confidence-weighted local-linear filter along the frames
  pafuse::pose_smooth(pose, cov?, radius, floor)          that pose smoothed along the frames, weighted by the hypothesis covariance
  pafuse::bone_lengths(pose, cov?, parent, mirror?, floor)   one length per bone from the whole video: length, dev, frames
  pafuse::bone_project(pose, cov?, parent, length, iterations, snap, floor)   every frame moved onto those lengths: out, code, resid
  pafuse::repair_detections(x2d, conf, anchor?, radius, threshold)   missing 2-D detections filled along the frames, per joint
  pafuse::screen_detections(x2d, conf, mirror?, radius, gate, floor, passes, support, threshold)   observed detections screened first
  pafuse::track_people(x2d, conf, tracks, seed?, gate, skip, max_gap, support, min_frames, threshold)   [N,K] candidates -> per-person videos
  pafuse::focal_sums(pose, x2d, cam, conf?)               the focal-length sums of that pose: (K, H, G, 1) per (t, frame)
  pafuse::focal_solve(state, cam)                         the focal length from them: focal, r2, frames, cam per t
  pafuse::foot_contacts(pose, traj, points, radius, speed)   the foot points on their local line and the weight of one that rests
  pafuse::ground_sums(foot, contact, traj, plane?, scale?, gate) / pafuse::ground_solve(state, floor, spread)   the ground plane per t
  pafuse::frames_to_world(pose, traj, plane)              pose + traj in world space: z up, the ground at z = 0
  pafuse::estimate_ground(pose, traj, points, ...)        that chain in one call: the tensors of ops.GROUND_OUTPUTS
  pafuse::frame_errors(pose, gt, pbroot, part, num_parts, traj?, gt_root?)   that pose (and root) scored against ground truth
  pafuse::noise_fill(key, draw, B, P, F, J)               one draw of noise stream v1 as a tensor

``precision`` ('bf16x3' = the modules' default; 'bf16x3_images', 'f16x2', 'f32', 'bf16': pafuse_amd.D3DP.precision) is the
matrix-product mode of the linear layers; in the split modes the ops build and cache the pre-split weight images themselves: the
modules' plan with the modules' default options (images.py: plan_images, make_images, cached), so the ops return the modules' bits.

``weights`` lists are in ``named_parameters()`` order of the corresponding module (= the reference's state-dict
order), so ``list(model.parameters())`` is the argument.  The modules in pafuse_amd call the C ABI directly; these ops
are the same entry points for callers that want schema'd operators instead of nn.Modules.
"""
import ctypes as C
from functools import lru_cache
from typing import List, Optional

import torch

from . import _lib
from ._lib import PRECISIONS      # (as pafuse_amd.D3DP.PRECISIONS)
from .images import (BLOCK_PARAMS, _IMAGE_CACHE_MAX, _image_cache, _ptr, block_images, cached, cached_split_image,  # noqa: F401
                     effective_mode, fill_block_struct, make_images, plan_images, resolve_options)   # (the cache: importable from here)
from .ops import _need, _stream
from .mixste2 import MixSTE2, fill_weights_struct, sinusoid_frequencies

BLOCK_KEYS = tuple(key for _, key in BLOCK_PARAMS)


@lru_cache(maxsize=None)
def mixste_param_names(frames, joints, channels, depth, heads):
    """named_parameters() order of a MixSTE2 of these dimensions (built on the meta device: no storage)."""
    with torch.device("meta"):
        m = MixSTE2(num_frame=frames, num_joints=joints, in_chans=5, embed_dim_ratio=channels, depth=depth,
                    num_heads=heads, is_train=False)
    return tuple(n for n, _ in m.named_parameters())


@lru_cache(maxsize=None)
def mixste_param_shapes(frames, joints, channels, depth, heads):
    with torch.device("meta"):
        m = MixSTE2(num_frame=frames, num_joints=joints, in_chans=5, embed_dim_ratio=channels, depth=depth,
                    num_heads=heads, is_train=False)
    return tuple(tuple(p.shape) for _, p in m.named_parameters())


_freq_cache = {}


def _freqs(channels, device):
    key = (channels, device)
    if key not in _freq_cache:
        _freq_cache[key] = sinusoid_frequencies(channels).to(device)
    return _freq_cache[key]


def _mode(precision):
    if precision not in PRECISIONS:
        raise _lib.PafuseError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
    return PRECISIONS[precision]


def mixste_struct(weights, frames, joints, depth, heads, precision="f32"):
    """pafuse_mixste2_weights from a flat parameter list; returns (struct, keep-alive)."""
    channels = weights[0].shape[-1]                           # Spatial_pos_embed [1,J,C] comes first
    mode = effective_mode(_mode(precision), channels, 0, heads, joints, frames)
    names = mixste_param_names(frames, joints, channels, depth, heads)
    if len(weights) != len(names):
        raise _lib.PafuseError(f"expected {len(names)} weight tensors (named_parameters() order), got {len(weights)}")
    table = dict(zip(names, weights))
    for (n, t), shape in zip(table.items(), mixste_param_shapes(frames, joints, channels, depth, heads)):
        _need(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
        _ptr(t, n)
    fr = _freqs(channels, weights[0].device)
    w = _lib.MixSTE2Weights()
    # the modules' default options (the shapes checked above are those of mlp_ratio 2)
    plan = plan_images(names, mode, resolve_options(mode, channels, 2 * channels))
    images = make_images(plan, table.__getitem__, mode, heads, cache=cached) if plan else None
    fill_weights_struct(w, table.__getitem__, fr, frames, joints, channels, depth, heads, 5, mode, images)
    return w, (table, fr, images)


# ------------------------------------------------------------------------------------------------ unit ops
@torch.library.custom_op("pafuse::linear", mutates_args=(), device_types="cuda")
def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    lib = _lib.load()
    K, N = x.shape[-1], weight.shape[0]
    _need(tuple(weight.shape) == (N, K) and bias.numel() == N, f"linear: x [..,{K}] needs weight [N,{K}] and bias [N]")
    x2 = x.contiguous().view(-1, K)
    out = torch.empty(x2.shape[0], N, device=x.device, dtype=torch.float32)
    _lib.check(lib.pafuse_linear(_ptr(x2, "x"), _ptr(weight, "weight"), _ptr(bias, "bias"), out.data_ptr(),
                                 x2.shape[0], N, K, int(gelu), _stream(x)))
    return out.view(*x.shape[:-1], N)


@linear.register_fake
def _(x, weight, bias, gelu=False):
    return x.new_empty(*x.shape[:-1], weight.shape[0])


@torch.library.custom_op("pafuse::layer_norm", mutates_args=(), device_types="cuda")
def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    lib = _lib.load()
    Cc = x.shape[-1]
    _need(weight.numel() == Cc and bias.numel() == Cc, f"layer_norm: weight and bias must have {Cc} elements")
    x2 = x.contiguous().view(-1, Cc)
    out = torch.empty_like(x2)
    _lib.check(lib.pafuse_layernorm(_ptr(x2, "x"), _ptr(weight, "weight"), _ptr(bias, "bias"), out.data_ptr(),
                                    x2.shape[0], Cc, eps, _stream(x)))
    return out.view(x.shape)


@layer_norm.register_fake
def _(x, weight, bias, eps):
    return torch.empty_like(x)


@torch.library.custom_op("pafuse::attention", mutates_args=(), device_types="cuda")
def attention(qkv: torch.Tensor, heads: int, seq_len: int, joints: int = 0) -> torch.Tensor:
    """qkv [M,3C] in the fixed (r,f,j) token order.  joints == 0: M/seq_len contiguous sequences (spatial,
    seq_len = J); joints > 0: temporal sequences of seq_len = F tokens at stride `joints`."""
    lib = _lib.load()
    M, C3 = qkv.shape
    Cc = C3 // 3
    _need(C3 % 3 == 0 and heads > 0 and Cc % heads == 0 and seq_len > 0 and joints >= 0,
          "attention: qkv must be [M, 3*heads*d]")
    if M % seq_len or (joints and M % (seq_len * joints)):
        raise _lib.PafuseError(f"attention: {M} rows do not split into sequences of {seq_len}")
    o = torch.empty(M, Cc, device=qkv.device, dtype=torch.float32)
    if joints:
        args = (M // seq_len, seq_len, Cc, heads, joints, seq_len * joints, 1, joints)
    else:
        args = (M // seq_len, seq_len, Cc, heads, 1, seq_len, 0, 1)
    _lib.check(lib.pafuse_attention(_ptr(qkv, "qkv"), o.data_ptr(), *args, _stream(qkv)))
    return o


@attention.register_fake
def _(qkv, heads, seq_len, joints=0):
    return qkv.new_empty(qkv.shape[0], qkv.shape[1] // 3)


@torch.library.custom_op("pafuse::block", mutates_args=(), device_types="cuda")
def block(x: torch.Tensor, weights: List[torch.Tensor], heads: int, precision: str = "bf16x3") -> torch.Tensor:
    """Block.forward on [S,L,C]: S sequences of L tokens (spatial: L = J; temporal: the caller passes [.., F, C]).
    precision: matrix-product mode of the linear layers, as pafuse_amd.D3DP.precision (default: the inference default)."""
    lib = _lib.load()
    mode = _mode(precision)
    if len(weights) != len(BLOCK_KEYS):
        raise _lib.PafuseError(f"block: expected {len(BLOCK_KEYS)} tensors in order {BLOCK_KEYS}")
    S, L, Cc = x.shape
    shapes = ((Cc,), (Cc,), (3 * Cc, Cc), (3 * Cc,), (Cc, Cc), (Cc,), (Cc,), (Cc,), (2 * Cc, Cc), (2 * Cc,), (Cc, 2 * Cc), (Cc,))
    for t, shape, name in zip(weights, shapes, BLOCK_KEYS):
        _need(tuple(t.shape) == shape, f"block: {name} must be {shape}, got {tuple(t.shape)}")
    _need(heads > 0 and Cc % heads == 0, "block: heads must divide the width")
    y = x.contiguous().clone()
    w = _lib.BlockWeights()
    mode = effective_mode(mode, Cc, 0, heads, L, L)
    get = dict(zip(BLOCK_KEYS, weights)).__getitem__
    images = block_images(get, mode, heads, cache=cached)
    fill_block_struct(w, get, images=images)
    nbytes = lib.pafuse_block_workspace_bytes(S * L, Cc)
    ws = _lib.workspace(nbytes, x.device, "block_forward")
    _lib.check(lib.pafuse_block_forward(C.byref(w), _ptr(y, "x"), S, L, Cc, heads, mode, ws.data_ptr(), nbytes, _stream(x)))
    return y


@block.register_fake
def _(x, weights, heads, precision="bf16x3"):
    return torch.empty_like(x)


# ------------------------------------------------------------------------------------------- model-level ops
@torch.library.custom_op("pafuse::mixste_eval", mutates_args=(), device_types="cuda")
def mixste_eval(x2d: torch.Tensor, x3d: torch.Tensor, t: torch.Tensor, weights: List[torch.Tensor], depth: int,
                heads: int, precision: str = "bf16x3") -> torch.Tensor:
    lib = _lib.load()
    _need(x3d.dim() == 5 and x3d.shape[-1] == 3, "mixste_eval: x3d must be [B,P,F,J,3]")
    B, P, F, J, _ = x3d.shape
    _need(tuple(x2d.shape) == (B, F, J, 2) and tuple(t.shape) == (B,), "mixste_eval: x2d must be [B,F,J,2], t [B]")
    w, keep = mixste_struct(weights, F, J, depth, heads, precision)
    x2d, x3d, t = x2d.contiguous().float(), x3d.contiguous().float(), t.contiguous().long()
    out = torch.empty(B, P, F, J, 3, device=x3d.device, dtype=torch.float32)
    nbytes = lib.pafuse_mixste2_workspace_bytes(C.byref(w), B, P)
    ws = _lib.workspace(nbytes, x3d.device, "mixste2_forward")
    _lib.check(lib.pafuse_mixste2_forward(C.byref(w), _ptr(x2d, "x2d"), _ptr(x3d, "x3d"), t.data_ptr(), B, P,
                                          out.data_ptr(), ws.data_ptr(), nbytes, _stream(x3d)))
    return out


@mixste_eval.register_fake
def _(x2d, x3d, t, weights, depth, heads, precision="bf16x3"):
    return torch.empty_like(x3d)


@torch.library.custom_op("pafuse::ddim_loop", mutates_args=(), device_types="cuda")
def ddim_loop(x2d: torch.Tensor, x2d_flip: torch.Tensor, noise: torch.Tensor, weights: List[torch.Tensor],
              part_joints: List[torch.Tensor], flip_perm: torch.Tensor, depth: int, heads: int, times: List[int],
              sched: List[float], flip: bool, scale: float, precision: str = "bf16x3") -> torch.Tensor:
    """The whole sampler.  noise [n_draws,B,P,F,J,3] in the reference's draw order; weights = the per-part
    parameter lists concatenated in part order; part_joints[i] int32 joint indices of part i; flip_perm int32 [J];
    times[k] the k-th timestep (the last one is the step whose time_next < 0); sched 5 doubles per step:
    sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t], sqrt(alpha_next), c, sigma.  precision: the
    matrix-product mode of every part's linear layers (default = the modules' inference default).  -> [B,T,P,F,J,3]"""
    lib = _lib.load()
    _mode(precision)
    _need(noise.dim() == 6 and noise.shape[-1] == 3, "ddim_loop: noise must be [n_draws,B,P,F,J,3]")
    n_draws, B, P, F, J, _ = noise.shape
    _need(tuple(x2d.shape) == (B, F, J, 2) and (not flip or tuple(x2d_flip.shape) == (B, F, J, 2)),
          "ddim_loop: x2d / x2d_flip must be [B,F,J,2]")
    _need(flip_perm.numel() == J and int(flip_perm.min()) >= 0 and int(flip_perm.max()) < J, "ddim_loop: flip_perm")
    _need(all(int(i.min()) >= 0 and int(i.max()) < J for i in part_joints), "ddim_loop: joint index out of range")
    T = len(times)
    if len(sched) != 5 * T or len(part_joints) > _lib.MAX_PARTS:
        raise _lib.PafuseError("ddim_loop: sched needs 5 values per step; at most %d parts" % _lib.MAX_PARTS)
    dev = noise.device
    cfg = _lib.D3DPConfig()
    cfg.num_parts, cfg.num_kps, cfg.frames, cfg.flip, cfg.scale = len(part_joints), J, F, int(flip), float(scale)
    keep, at = [], 0
    joint_part = torch.full((J,), -1, dtype=torch.int32)
    joint_local = torch.zeros(J, dtype=torch.int32)
    for i, idx in enumerate(part_joints):
        Jp = idx.numel()
        n = len(mixste_param_names(F, Jp, weights[at].shape[-1], depth, heads))
        w, k = mixste_struct(weights[at:at + n], F, Jp, depth, heads, precision)
        at += n
        idx32 = idx.to(device=dev, dtype=torch.int32).contiguous()
        cfg.part[i], cfg.part_joints[i] = w, idx32.data_ptr()
        host = idx.cpu().long()
        joint_part[host] = i
        joint_local[host] = torch.arange(Jp, dtype=torch.int32)
        keep += [k, idx32]
    if at != len(weights) or int(joint_part.min()) < 0:
        raise _lib.PafuseError("ddim_loop: weights / part_joints do not cover the model")
    joint_part, joint_local = joint_part.to(dev), joint_local.to(dev)
    perm = flip_perm.to(device=dev, dtype=torch.int32).contiguous()
    cfg.joint_part, cfg.joint_local, cfg.flip_perm = joint_part.data_ptr(), joint_local.data_ptr(), perm.data_ptr()
    # one stream, every layer part by part: the launches of the modules' three-stream schedule.  (The shared grids of the library's
    # own single-stream schedule run another whole-row epilogue that gives the same bits: tests/test_hip_rowln.py.)
    cfg.part_by_part_launches = 1
    steps = (_lib.DDIMStep * T)()
    for k in range(T):
        st = steps[k]
        st.time, st.last = int(times[k]), int(k == T - 1)
        st.sqrt_recip_acp, st.sqrt_recipm1_acp, st.sqrt_alpha_next, st.c, st.sigma = sched[5 * k:5 * k + 5]
    if n_draws < T:
        raise _lib.PafuseError(f"ddim_loop: {T} steps need {T} noise draws, got {n_draws}")
    x2d = x2d.contiguous().float()
    x2f = x2d_flip.contiguous().float() if flip else x2d
    noise = noise.contiguous().float()
    out = torch.empty(B, T, P, F, J, 3, device=dev, dtype=torch.float32)
    nbytes = lib.pafuse_d3dp_workspace_bytes(C.byref(cfg), B, P)
    ws = _lib.workspace(nbytes, dev, "d3dp_sample")
    _lib.check(lib.pafuse_d3dp_sample(C.byref(cfg), steps, T, _ptr(x2d, "x2d"), _ptr(x2f, "x2d_flip"),
                                      _ptr(noise, "noise"), n_draws, B, P, out.data_ptr(), ws.data_ptr(), nbytes,
                                      _stream(noise), None, 0))
    return out


@ddim_loop.register_fake
def _(x2d, x2d_flip, noise, weights, part_joints, flip_perm, depth, heads, times, sched, flip, scale, precision="bf16x3"):
    n_draws, B, P, F, J, _ = noise.shape
    return noise.new_empty(B, len(times), P, F, J, 3)


# --------------------------------------------------------------------------------- sharded hypothesis evaluation
@torch.library.custom_op("pafuse::hypothesis_partials", mutates_args=(), device_types="cuda")
def hypothesis_partials(pred: torch.Tensor, gt: torch.Tensor, x2d: torch.Tensor, traj: torch.Tensor, cam: torch.Tensor,
                        conn: torch.Tensor, pbroot: torch.Tensor, part: torch.Tensor, num_parts: int, h0: int) -> torch.Tensor:
    """pafuse_amd.ops.hypothesis_partials: the flat float64 state of the local hypotheses [h0, h0 + P_r)."""
    from . import ops
    return ops.hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, num_parts, h0)


@hypothesis_partials.register_fake
def _(pred, gt, x2d, traj, cam, conn, pbroot, part, num_parts, h0):
    B, T, P_r, F, J, _ = pred.shape
    return pred.new_empty(5 * B * T * F * J + P_r * T * (1 + num_parts), dtype=torch.float64)


@torch.library.custom_op("pafuse::combine_partials", mutates_args=(), device_types="cuda")
def combine_partials(states: torch.Tensor, gt: torch.Tensor, conn: torch.Tensor, pbroot: torch.Tensor, T: int,
                     num_proposals: int) -> List[torch.Tensor]:
    """pafuse_amd.ops.combine_partials on states [W, L]: -> [jbest, pagg, jagg, paggpb], each [B,T,F,J]."""
    from . import ops
    B, F, J, _ = gt.shape
    m = ops.combine_partials(states, gt, conn, pbroot, (B, T, F, J), num_proposals)
    return [m["jbest"], m["pagg"], m["jagg"], m["paggpb"]]


@combine_partials.register_fake
def _(states, gt, conn, pbroot, T, num_proposals):
    B, F, J, _ = gt.shape
    return [gt.new_empty(B, T, F, J) for _ in range(4)]


# ---------------------------------------------------------------------------- Protocol #2 from partial states
@torch.library.custom_op("pafuse::procrustes_partials", mutates_args=(), device_types="cuda")
def procrustes_partials(pred: torch.Tensor, gt: torch.Tensor, x2d: torch.Tensor, traj: torch.Tensor, cam: torch.Tensor,
                        conn: torch.Tensor, h0: int) -> torch.Tensor:
    """pafuse_amd.ops.procrustes_partials: the flat float64 Protocol #2 state of the local hypotheses [h0, h0 + P_r)."""
    from . import ops
    return ops.procrustes_partials(pred, gt, x2d, traj, cam, conn, h0)


@procrustes_partials.register_fake
def _(pred, gt, x2d, traj, cam, conn, h0):
    B, T, P_r, F, J, _ = pred.shape
    return pred.new_empty(2 * B * T * F * J + P_r * T, dtype=torch.float64)


@torch.library.custom_op("pafuse::procrustes_combine", mutates_args=(), device_types="cuda")
def procrustes_combine(states: torch.Tensor, sums: torch.Tensor, gt: torch.Tensor, conn: torch.Tensor, T: int,
                       num_proposals: int) -> List[torch.Tensor]:
    """pafuse_amd.ops.combine_procrustes on states [W, L] and sums [W, >= 3*B*T*F*J] (rows beginning with the fp64 sums of
    the same shards): -> [jbest, pagg, jagg [B,T,F,J] fp32, pick [B,T,F,J] int32]."""
    from . import ops
    B, F, J, _ = gt.shape
    m = ops.combine_procrustes(states, (B, T, F, J), num_proposals, sums=sums, gt=gt, conn=conn)
    return [m["jbest"], m["pagg"], m["jagg"], m["pick"]]


@procrustes_combine.register_fake
def _(states, sums, gt, conn, T, num_proposals):
    B, F, J, _ = gt.shape
    return [gt.new_empty(B, T, F, J) for _ in range(3)] + [gt.new_empty((B, T, F, J), dtype=torch.int32)]


# ------------------------------------------------------------------------------------------ aggregates as poses
@torch.library.custom_op("pafuse::aggregate_poses", mutates_args=(), device_types="cuda")
def aggregate_poses(pred: torch.Tensor, conn: torch.Tensor, x2d: Optional[torch.Tensor] = None,
                    traj: Optional[torch.Tensor] = None, cam: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """The one-shard convenience of pafuse_amd.ops.pose_partials + combine_poses: pred [B,T,P,F,J,3] part-centred ->
    [mean [B,T,F,J,3], pick [B,T,F,J,3], idx [B,T,F,J] int32].  Without x2d / traj / cam (mean-only) there is no pick: it
    comes back as NaN with idx -1, the library's "no candidate"."""
    from . import ops
    B, T, P, F, J, _ = pred.shape
    state = ops.pose_partials(pred, conn, 0, x2d, traj, cam)
    if x2d is None:
        mean = ops.combine_poses(state.view(1, -1), (B, T, F, J), P, want=("mean",))["mean"]
        return [mean, torch.full_like(mean, float("nan")), torch.full((B, T, F, J), -1, device=pred.device, dtype=torch.int32)]
    m = ops.combine_poses(state.view(1, -1), (B, T, F, J), P)
    return [m["mean"], m["pick"], m["idx"]]


@aggregate_poses.register_fake
def _(pred, conn, x2d=None, traj=None, cam=None):
    B, T, P, F, J, _ = pred.shape
    return [pred.new_empty(B, T, F, J, 3), pred.new_empty(B, T, F, J, 3), pred.new_empty((B, T, F, J), dtype=torch.int32)]


@torch.library.custom_op("pafuse::aggregate_poses_fit", mutates_args=(), device_types="cuda")
def aggregate_poses_fit(pred: torch.Tensor, conn: torch.Tensor, x2d: torch.Tensor, cam: torch.Tensor,
                        conf: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """The one-shard convenience of pafuse_amd.ops.pose_partials_fit + combine_poses (J-Agg without a trajectory): pred
    [B,T,P,F,J,3] part-centred, x2d [B,F,J,2], cam [9], conf [B,F,J] or None -> [mean [B,T,F,J,3], pick [B,T,F,J,3], idx
    [B,T,F,J] int32, tfit [B,T,P,F,3]].  Where no hypothesis has a fit, or a joint no positive weight, pick is NaN and
    idx -1; tfit is NaN where there is no fit."""
    from . import ops
    B, T, P, F, J, _ = pred.shape
    tfit = pred.new_empty(B, T, P, F, 3)
    state = ops.pose_partials_fit(pred, conn, 0, x2d, cam, conf=conf, tfit=tfit)
    m = ops.combine_poses(state.view(1, -1), (B, T, F, J), P, no_pick_ok=True)
    return [m["mean"], m["pick"], m["idx"], tfit]


@aggregate_poses_fit.register_fake
def _(pred, conn, x2d, cam, conf=None):
    B, T, P, F, J, _ = pred.shape
    return [pred.new_empty(B, T, F, J, 3), pred.new_empty(B, T, F, J, 3), pred.new_empty((B, T, F, J), dtype=torch.int32),
            pred.new_empty(B, T, P, F, 3)]


@torch.library.custom_op("pafuse::pose_path", mutates_args=(), device_types="cuda")
def pose_path(pred: torch.Tensor, conn: torch.Tensor, x2d: torch.Tensor, root: torch.Tensor, cam: torch.Tensor, weight: float,
              conf: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """pafuse_amd.ops.pose_path (J-Agg coherent in time): pred [B,T,P,F,J,3] ALL part-centred hypotheses, x2d [B,F,J,2], root
    [B,F,3] or [B,T,P,F,3], cam [9], weight >= 0, conf [B,F,J] or None, mean [B,T,F,J,3] or None -> [pick [B,T,F,J,3],
    idx [B,T,F,J] int32, e2 [B,T,F,J], cost [B,T,J] float64]; a line without a path: NaN, -1, +inf, NaN."""
    from . import ops
    m = ops.pose_path(pred, conn, x2d, root, cam, weight, conf=conf, mean=mean, want=ops.PATH_OUTPUTS)
    return [m[k] for k in ops.PATH_OUTPUTS]


@pose_path.register_fake
def _(pred, conn, x2d, root, cam, weight, conf=None, mean=None):
    B, T, P, F, J, _ = pred.shape
    return [pred.new_empty(B, T, F, J, 3), pred.new_empty((B, T, F, J), dtype=torch.int32), pred.new_empty(B, T, F, J),
            pred.new_empty((B, T, J), dtype=torch.float64)]


@torch.library.custom_op("pafuse::frames_path", mutates_args=(), device_types="cuda")
def frames_path(pred: torch.Tensor, conn: torch.Tensor, x2d: torch.Tensor, root: torch.Tensor, cam: torch.Tensor, weight: float,
                starts: List[int], valid: List[int], conf: Optional[torch.Tensor] = None,
                mean: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """pafuse_amd.ops.frames_path (the J-Agg path of a whole video): pred [W,T,P,F,J,3] ALL part-centred hypotheses of the W
    windows, x2d [N,J,2], root [N,3] or [W,T,P,F,3], cam [9], weight >= 0, starts / valid W host integers each (the whole
    video), conf [N,J] or None, mean [T,N,J,3] or None -> [pick [T,N,J,3], idx [T,N,J] int32, window [T,N,J] int32,
    e2 [T,N,J], cost [T,J] float64]; a line without a path: NaN, -1, -1, +inf, NaN."""
    from . import ops
    m = ops.frames_path(pred, conn, x2d, root, cam, weight, starts, valid, conf=conf, mean=mean, want=ops.FRAMES_PATH_OUTPUTS)
    return [m[k] for k in ops.FRAMES_PATH_OUTPUTS]


@frames_path.register_fake
def _(pred, conn, x2d, root, cam, weight, starts, valid, conf=None, mean=None):
    T, J, N = pred.shape[1], pred.shape[4], x2d.shape[0]
    return [pred.new_empty(T, N, J, 3), pred.new_empty((T, N, J), dtype=torch.int32), pred.new_empty((T, N, J), dtype=torch.int32),
            pred.new_empty(T, N, J), pred.new_empty((T, J), dtype=torch.float64)]


# ----------------------------------------------------------------------------------- spread of the hypotheses
@torch.library.custom_op("pafuse::hypothesis_spread", mutates_args=(), device_types="cuda")
def hypothesis_spread(pred: torch.Tensor, conn: torch.Tensor) -> List[torch.Tensor]:
    """The one-shard convenience of pafuse_amd.ops.spread_partials + combine_spread: pred [B,T,P,F,J,3] part-centred ->
    [mean [B,T,F,J,3], cov [B,T,F,J,6] (population covariance: xx, xy, xz, yy, yz, zz), std [B,T,F,J]], fp32."""
    from . import ops
    B, T, P, F, J, _ = pred.shape
    m = ops.combine_spread(ops.spread_partials(pred, conn, 0).view(1, -1), (B, T, F, J))
    return [m["mean"], m["cov"], m["std"]]


@hypothesis_spread.register_fake
def _(pred, conn):
    B, T, P, F, J, _ = pred.shape
    return [pred.new_empty(B, T, F, J, 3), pred.new_empty(B, T, F, J, 6), pred.new_empty(B, T, F, J)]


# ----------------------------------------------------------------- overlapping windows pooled into one pose per frame
@torch.library.custom_op("pafuse::fold_windows", mutates_args=("frame",), device_types="cuda")
def fold_windows(frame: torch.Tensor, N: int, state: torch.Tensor, shape: List[int], starts: List[int], valid: List[int],
                 w0: int, num_proposals: int) -> None:
    """pafuse_amd.ops.fold_windows: the flat pose state of B windows (shape = [B,T,F,J]) folded IN PLACE into the frame pose
    state `frame` (ops.frame_state) of N video frames; window b covers frames [starts[b], starts[b] + valid[b])."""
    from . import ops
    ops.fold_windows(frame, N, state, shape, starts, valid, w0, num_proposals)


@fold_windows.register_fake
def _(frame, N, state, shape, starts, valid, w0, num_proposals):
    return None


@torch.library.custom_op("pafuse::finish_frames", mutates_args=(), device_types="cuda")
def finish_frames(frame: torch.Tensor, N: int, T: int, J: int, spread: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """pafuse_amd.ops.finish_frames: the frame pose state -> [mean [T,N,J,3], pick [T,N,J,3], idx [T,N,J] int32, window
    [T,N,J] int32]; with the frame spread state `spread` also [std [T,N,J], cov [T,N,J,6]]."""
    from . import ops
    m = ops.finish_frames(N, T, J, frame=frame, spread=spread)
    return [m[k] for k in ("mean", "pick", "idx", "window") + (("std", "cov") if spread is not None else ())]


@finish_frames.register_fake
def _(frame, N, T, J, spread=None):
    f32 = lambda *tail: frame.new_empty((T, N, J, *tail), dtype=torch.float32)
    i32 = lambda: frame.new_empty((T, N, J), dtype=torch.int32)
    return [f32(3), f32(3), i32(), i32()] + ([f32(), f32(6)] if spread is not None else [])


# ------------------------------------------------------------------ the camera-space root of the per-frame pose
@torch.library.custom_op("pafuse::fit_trajectory", mutates_args=(), device_types="cuda")
def fit_trajectory(pose: torch.Tensor, x2d: torch.Tensor, cam: torch.Tensor, conf: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """pafuse_amd.ops.fit_trajectory: pose [T,N,J,3] root-relative, x2d [N,J,2], cam [>= 4], conf [N,J] or None -> [traj [T,N,3]
    (NaN where there is no fit), wsum [T,N], resid [T,N]]."""
    from . import ops
    m = ops.fit_trajectory(pose, x2d, cam, conf=conf)
    return [m["traj"], m["wsum"], m["resid"]]


@fit_trajectory.register_fake
def _(pose, x2d, cam, conf=None):
    T, N = pose.shape[0], pose.shape[1]
    return [pose.new_empty((T, N, 3), dtype=torch.float32), pose.new_empty((T, N), dtype=torch.float32),
            pose.new_empty((T, N), dtype=torch.float32)]


@torch.library.custom_op("pafuse::smooth_trajectory", mutates_args=(), device_types="cuda")
def smooth_trajectory(traj: torch.Tensor, weight: Optional[torch.Tensor], radius: int) -> torch.Tensor:
    """pafuse_amd.ops.smooth_trajectory: traj [T,N,3], weight [T,N] or None, radius 1 .. 64 -> the filtered trajectory [T,N,3]."""
    from . import ops
    return ops.smooth_trajectory(traj, weight, radius)


@smooth_trajectory.register_fake
def _(traj, weight, radius):
    return torch.empty_like(traj)


# ------------------------------------------------------------------ the per-frame pose smoothed along the frames
@torch.library.custom_op("pafuse::pose_smooth", mutates_args=(), device_types="cuda")
def pose_smooth(pose: torch.Tensor, cov: Optional[torch.Tensor], radius: int, floor: float = 1e-3) -> List[torch.Tensor]:
    """pafuse_amd.ops.smooth_poses: pose [T,N,J,3], cov [T,N,J,6] or None, radius 1 .. 64, floor > 0 (metres) -> [the smoothed
    pose [T,N,J,3], code [T,N,J] uint8 (1 line, 2 weighted mean, 3 none)]."""
    from . import ops
    return list(ops.smooth_poses(pose, cov, radius, floor=floor, want_code=True))


@pose_smooth.register_fake
def _(pose, cov, radius, floor=1e-3):
    return [torch.empty_like(pose), pose.new_empty(pose.shape[:3], dtype=torch.uint8)]


# ------------------------------------------------------------------ bone lengths held constant along a video
@torch.library.custom_op("pafuse::bone_lengths", mutates_args=(), device_types="cuda")
def bone_lengths(pose: torch.Tensor, cov: Optional[torch.Tensor], parent: List[int], mirror: Optional[List[int]] = None,
                 floor: float = 1e-3) -> List[torch.Tensor]:
    """pafuse_amd.ops.bone_lengths: pose [T,N,J,3], cov [T,N,J,6] or None, parent [J] host integers (-1 or a joint below the
    entry's own), mirror [J] or None, floor > 0 (metres) -> [length [T,J], dev [T,J], frames [T,J] int32]."""
    from . import ops
    return list(ops.bone_lengths(pose, cov, parent, mirror, floor=floor, want_dev=True, want_frames=True))


@bone_lengths.register_fake
def _(pose, cov, parent, mirror=None, floor=1e-3):
    T, J = pose.shape[0], pose.shape[2]
    return [pose.new_empty((T, J)), pose.new_empty((T, J)), pose.new_empty((T, J), dtype=torch.int32)]


@torch.library.custom_op("pafuse::bone_project", mutates_args=(), device_types="cuda")
def bone_project(pose: torch.Tensor, cov: Optional[torch.Tensor], parent: List[int], length: torch.Tensor, iterations: int = 16,
                 snap: bool = True, floor: float = 1e-3) -> List[torch.Tensor]:
    """pafuse_amd.ops.project_bones: pose [T,N,J,3], cov [T,N,J,6] or None, parent [J] host integers, length [T,J], iterations
    0 .. 64, snap, floor > 0 (metres) -> [the constrained pose [T,N,J,3], code [T,N,J] uint8, resid [T,N,2]]."""
    from . import ops
    return list(ops.project_bones(pose, cov, parent, length, iterations=iterations, snap=snap, floor=floor, want_code=True, want_resid=True))


@bone_project.register_fake
def _(pose, cov, parent, length, iterations=16, snap=True, floor=1e-3):
    return [torch.empty_like(pose), pose.new_empty(pose.shape[:3], dtype=torch.uint8), pose.new_empty((*pose.shape[:2], 2))]


# ------------------------------------------------------------------ missing 2-D detections, repaired before lifting
@torch.library.custom_op("pafuse::repair_detections", mutates_args=(), device_types="cuda")
def repair_detections(x2d: torch.Tensor, conf: torch.Tensor, anchor: Optional[List[int]] = None, radius: int = 13,
                      threshold: float = 0.0) -> List[torch.Tensor]:
    """pafuse_amd.ops.repair_detections: x2d [N,J,2], conf [N,J], anchor J host integers or None, radius 1 .. 64, threshold >= 0
    -> [x2d [N,J,2] repaired, conf [N,J] (0 where not observed), status [N,J] uint8]."""
    from . import ops
    m = ops.repair_detections(x2d, conf, anchor=anchor, radius=radius, threshold=threshold)
    return [m["x2d"], m["conf"], m["status"]]


@repair_detections.register_fake
def _(x2d, conf, anchor=None, radius=13, threshold=0.0):
    return [torch.empty_like(x2d), torch.empty_like(conf), conf.new_empty(conf.shape, dtype=torch.uint8)]


# ------------------------------------------------------------------ observed 2-D detections, screened before the repair
@torch.library.custom_op("pafuse::screen_detections", mutates_args=(), device_types="cuda")
def screen_detections(x2d: torch.Tensor, conf: torch.Tensor, mirror: Optional[List[int]] = None, radius: int = 13, gate: float = 4.0,
                      floor: float = 0.005, passes: int = 3, support: int = 3, threshold: float = 0.0) -> List[torch.Tensor]:
    """pafuse_amd.ops.screen_detections: x2d [N,J,2], conf [N,J], mirror J host integers or None ->
    [x2d [N,J,2] screened, conf [N,J] (0 where rejected), status [N,J] uint8, resid [N,J], scale [J]]."""
    from . import ops
    m = ops.screen_detections(x2d, conf, mirror=mirror, radius=radius, gate=gate, floor=floor, passes=passes, support=support,
                              threshold=threshold)
    return [m["x2d"], m["conf"], m["status"], m["resid"], m["scale"]]


@screen_detections.register_fake
def _(x2d, conf, mirror=None, radius=13, gate=4.0, floor=0.005, passes=3, support=3, threshold=0.0):
    return [torch.empty_like(x2d), torch.empty_like(conf), conf.new_empty(conf.shape, dtype=torch.uint8), torch.empty_like(conf),
            conf.new_empty(conf.shape[1:])]


# ------------------------------------------------------------------ people followed through a video: [N,K] candidates -> tracks
@torch.library.custom_op("pafuse::track_people", mutates_args=(), device_types="cuda")
def track_people(x2d: torch.Tensor, conf: torch.Tensor, tracks: int = 1, seed: Optional[List[int]] = None, gate: float = 0.5,
                 skip: float = 0.05, max_gap: int = 4, support: int = 5, min_frames: int = 5, threshold: float = 0.0) -> List[torch.Tensor]:
    """pafuse_amd.ops.track_people: x2d [N,K,J,2], conf [N,K,J], seed (frame, candidate) or None ->
    [x2d [M,N,J,2], conf [M,N,J], assign [M,N] int32, score [M] float64, frames [M] int32]."""
    from . import ops
    m = ops.track_people(x2d, conf, tracks=tracks, seed=None if seed is None else tuple(seed), gate=gate, skip=skip, max_gap=max_gap,
                         support=support, min_frames=min_frames, threshold=threshold)
    return [m["x2d"], m["conf"], m["assign"], m["score"], m["frames"]]


@track_people.register_fake
def _(x2d, conf, tracks=1, seed=None, gate=0.5, skip=0.05, max_gap=4, support=5, min_frames=5, threshold=0.0):
    N, J = x2d.shape[0], x2d.shape[2]
    return [x2d.new_empty((tracks, N, J, 2)), conf.new_empty((tracks, N, J)), x2d.new_empty((tracks, N), dtype=torch.int32),
            x2d.new_empty((tracks,), dtype=torch.float64), x2d.new_empty((tracks,), dtype=torch.int32)]


# ------------------------------------------------------------------ the focal length, estimated from pose and detections
@torch.library.custom_op("pafuse::focal_sums", mutates_args=(), device_types="cuda")
def focal_sums(pose: torch.Tensor, x2d: torch.Tensor, cam: torch.Tensor, conf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pafuse_amd.ops.focal_sums: pose [T,N,J,3] root-relative, x2d [N,J,2], cam [>= 4], conf [N,J] or None -> state [T,N,4] float64."""
    from . import ops
    return ops.focal_sums(pose, x2d, cam, conf=conf)


@focal_sums.register_fake
def _(pose, x2d, cam, conf=None):
    return pose.new_empty((pose.shape[0], pose.shape[1], 4), dtype=torch.float64)


@torch.library.custom_op("pafuse::focal_solve", mutates_args=(), device_types="cuda")
def focal_solve(state: torch.Tensor, cam: torch.Tensor) -> List[torch.Tensor]:
    """pafuse_amd.ops.focal_solve: state [T,N,4] float64, cam [4 .. 9] -> [focal [T], r2 [T], frames [T] int32, cam [T,len(cam)]]."""
    from . import ops
    m = ops.focal_solve(state, cam)
    return [m["focal"], m["r2"], m["frames"], m["cam"]]


@focal_solve.register_fake
def _(state, cam):
    T = state.shape[0]
    return [state.new_empty((T,), dtype=torch.float32), state.new_empty((T,), dtype=torch.float32),
            state.new_empty((T,), dtype=torch.int32), state.new_empty((T, cam.shape[0]), dtype=torch.float32)]


# ------------------------------------------------------------------ which way is up: the ground plane from the foot contacts
def _ground_fake_solve(ref, T):
    f32, f64 = torch.float32, torch.float64
    return [ref.new_empty((T, 4), dtype=f64), ref.new_empty((T,), dtype=f64), ref.new_empty((T, 3), dtype=f32),
            ref.new_empty((T,), dtype=f32), ref.new_empty((T,), dtype=f32), ref.new_empty((T, 3), dtype=f32),
            ref.new_empty((T,), dtype=torch.int32), ref.new_empty((T,), dtype=torch.uint8)]


@torch.library.custom_op("pafuse::foot_contacts", mutates_args=(), device_types="cuda")
def foot_contacts(pose: torch.Tensor, traj: torch.Tensor, points: List[int], radius: int = 3, speed: float = 0.015) -> List[torch.Tensor]:
    """pafuse_amd.ops.foot_contacts: pose [T,N,J,3], traj [T,N,3], points K host integers -> [foot [T,N,K,3], foot_speed [T,N,K],
    contact [T,N,K]]."""
    from . import ops
    m = ops.foot_contacts(pose, traj, list(points), radius=radius, speed=speed)
    return [m["foot"], m["foot_speed"], m["contact"]]


@foot_contacts.register_fake
def _(pose, traj, points, radius=3, speed=0.015):
    T, N, K = pose.shape[0], pose.shape[1], len(points)
    return [pose.new_empty((T, N, K, 3)), pose.new_empty((T, N, K)), pose.new_empty((T, N, K))]


@torch.library.custom_op("pafuse::ground_sums", mutates_args=(), device_types="cuda")
def ground_sums(foot: torch.Tensor, contact: torch.Tensor, traj: torch.Tensor, plane: Optional[torch.Tensor] = None,
                scale: Optional[torch.Tensor] = None, gate: float = 2.5) -> torch.Tensor:
    """pafuse_amd.ops.ground_sums: foot [T,N,K,3], contact [T,N,K], traj [T,N,3], plane [T,4] / scale [T] float64 or neither ->
    state [T,N,14] float64."""
    from . import ops
    return ops.ground_sums(foot, contact, traj, plane, scale, gate=gate)


@ground_sums.register_fake
def _(foot, contact, traj, plane=None, scale=None, gate=2.5):
    return foot.new_empty((foot.shape[0], foot.shape[1], 14), dtype=torch.float64)


@torch.library.custom_op("pafuse::ground_solve", mutates_args=(), device_types="cuda")
def ground_solve(state: torch.Tensor, floor: float = 0.005, spread: float = 0.03) -> List[torch.Tensor]:
    """pafuse_amd.ops.ground_solve: state [T,N,14] float64 -> [plane [T,4] f64, scale [T] f64, up [T,3], camera_height [T],
    ground_rms [T], ground_eig [T,3], ground_points [T] int32, ground_code [T] uint8]."""
    from . import ops
    m = ops.ground_solve(state, floor=floor, spread=spread)
    return [m[k] for k in ops.GROUND_SOLVE_OUTPUTS]


@ground_solve.register_fake
def _(state, floor=0.005, spread=0.03):
    return _ground_fake_solve(state, state.shape[0])


@torch.library.custom_op("pafuse::frames_to_world", mutates_args=(), device_types="cuda")
def frames_to_world(pose: torch.Tensor, traj: torch.Tensor, plane: torch.Tensor) -> List[torch.Tensor]:
    """pafuse_amd.ops.frames_to_world: pose [T,N,J,3], traj [T,N,3], plane [T,4] float64 -> [pose_world [T,N,J,3], traj_world [T,N,3]]."""
    from . import ops
    return list(ops.frames_to_world(pose, traj, plane))


@frames_to_world.register_fake
def _(pose, traj, plane):
    return [torch.empty_like(pose), torch.empty_like(traj)]


@torch.library.custom_op("pafuse::estimate_ground", mutates_args=(), device_types="cuda")
def estimate_ground(pose: torch.Tensor, traj: torch.Tensor, points: List[int], radius: int = 3, speed: float = 0.015, passes: int = 3,
                    gate: float = 2.5, floor: float = 0.005, spread: float = 0.03) -> List[torch.Tensor]:
    """pafuse_amd.ops.estimate_ground: the chain -> the tensors of ops.GROUND_OUTPUTS in that order: plane, scale, up, camera_height,
    ground_rms, ground_eig, ground_points, ground_code, foot, foot_speed, contact, pose_world, traj_world."""
    from . import ops
    m = ops.estimate_ground(pose, traj, list(points), radius=radius, speed=speed, passes=passes, gate=gate, floor=floor, spread=spread)
    return [m[k] for k in ops.GROUND_OUTPUTS]


@estimate_ground.register_fake
def _(pose, traj, points, radius=3, speed=0.015, passes=3, gate=2.5, floor=0.005, spread=0.03):
    T, N, K = pose.shape[0], pose.shape[1], len(points)
    return _ground_fake_solve(pose, T) + [pose.new_empty((T, N, K, 3)), pose.new_empty((T, N, K)), pose.new_empty((T, N, K)),
                                          torch.empty_like(pose), torch.empty_like(traj)]


# ------------------------------------------------------------------ the per-frame pose scored against ground truth
@torch.library.custom_op("pafuse::frame_errors", mutates_args=(), device_types="cuda")
def frame_errors(pose: torch.Tensor, gt: torch.Tensor, pbroot: torch.Tensor, part: torch.Tensor, num_parts: int,
                 traj: Optional[torch.Tensor] = None, gt_root: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """pafuse_amd.ops.frame_errors(per_frame=True): pose [T,N,J,3], gt [N,J,3], pbroot / part int32 [J], num_parts, traj [T,N,3]
    with gt_root [N,3] or neither -> [sums [T,K] float64, counts [T,K] int64, err [T,N,K] float64, cnt [T,N,K] int32], K = 6 + num_parts."""
    from . import ops
    m = ops.frame_errors(pose, gt, pbroot, part, num_parts, traj=traj, gt_root=gt_root, per_frame=True)
    return [m["sums"], m["counts"], m["err"], m["cnt"]]


@frame_errors.register_fake
def _(pose, gt, pbroot, part, num_parts, traj=None, gt_root=None):
    T, N, K = pose.shape[0], pose.shape[1], 6 + num_parts
    return [pose.new_empty((T, K), dtype=torch.float64), pose.new_empty((T, K), dtype=torch.int64),
            pose.new_empty((T, N, K), dtype=torch.float64), pose.new_empty((T, N, K), dtype=torch.int32)]


# ----------------------------------------------------------------------------------------------- noise stream v1
@torch.library.custom_op("pafuse::noise_fill", mutates_args=(), device_types="cuda")
def noise_fill(key: torch.Tensor, draw: int, B: int, P: int, F: int, J: int) -> torch.Tensor:
    """pafuse_amd.ops.noise_fill: draw `draw` of noise stream v1 under key = ops.noise_key(seed, call, b0, p0) -> [B,P,F,J,3]."""
    from . import ops
    return ops.noise_fill(key, draw, B, P, F, J)


@noise_fill.register_fake
def _(key, draw, B, P, F, J):
    return key.new_empty((B, P, F, J, 3), dtype=torch.float32)


def ddim_loop_args(model):
    """The (weights, part_joints, flip_perm, depth, heads, times, sched, flip, scale) tail of pafuse::ddim_loop for a
    pafuse_amd.D3DP instance."""
    weights, joints = [], []
    for part, m in model.denoisers().items():
        weights += list(m.parameters())
        joints.append(getattr(model, f"_joints_{part}"))
    first = next(iter(model.denoisers().values()))
    steps = model.ddim_steps()
    times = [int(s.time) for s in steps]
    sched = [v for s in steps for v in (s.sqrt_recip_acp, s.sqrt_recipm1_acp, s.sqrt_alpha_next, s.c, s.sigma)]
    return (weights, joints, model._flip_perm, first.block_depth, first.num_heads, times, sched, bool(model.flip),
            float(model.scale))

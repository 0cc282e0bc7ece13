"""MixSTE2 - drop-in for the reference denoiser (common/mixste.py:141-298) backed by the HIP library.

The module owns exactly the reference's parameters (same names, shapes, creation order and default init, so
``torch.manual_seed(s); MixSTE2(...)`` yields the reference's weights and ``load_state_dict`` accepts its
checkpoints), but has no per-layer Python forward: ``forward`` hands raw device pointers to
``pafuse_mixste2_forward`` (include/pafuse_hip.h), which runs the fused gfx950 kernels; in train mode it is one
autograd node over ``pafuse_mixste2_train_forward`` / ``_backward`` (DropPath factors drawn here, as timm draws them).
"""
import ctypes as C
import math
from functools import partial
from operator import attrgetter

import torch
import torch.nn as nn

from . import _lib
from ._lib import MODE_BF16, MODE_BF16X3, MODE_F16X2, MODE_F32
from .images import (FOLD_SUFFIXES, SPLIT_SUFFIXES, _ptr, effective_mode, fill_block_struct, make_images,  # noqa: F401  (_ptr: imported from here too)
                     plan_images, resolve_options)


class _AttentionParams(nn.Module):
    """qkv / proj of common/mixste.py:46-61 (parameters only)."""

    def __init__(self, dim, qkv_bias):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class _MlpParams(nn.Module):
    """fc1 / fc2 of common/mixste.py:24-35 (parameters only)."""

    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _BlockParams(nn.Module):
    """norm1, attn, norm2, mlp of common/mixste.py:84-103 (parameters only, in the reference's creation order)."""

    def __init__(self, dim, mlp_ratio, qkv_bias, norm_layer):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = _AttentionParams(dim, qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = _MlpParams(dim, int(dim * mlp_ratio))


def sinusoid_frequencies(dim):
    """omega table of SinusoidalPositionEmbeddings (common/mixste.py:134-136), evaluated by the same CPU ops."""
    half = dim // 2
    step = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half) * -step)


class MixSTE2(nn.Module):
    def __init__(self, num_frame=9, num_joints=17, in_chans=5, embed_dim_ratio=32, depth=4,
                 num_heads=8, mlp_ratio=2., qkv_bias=True, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2, norm_layer=None, is_train=True):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        C_ = embed_dim_ratio
        # Constructor options PAFUSE never sets (it builds qkv_bias=True, qk_scale=None, mlp_ratio=2, no dropout,
        # common/diffusionpose.py:144-147) are inference options here: the training kernels implement the PAFUSE
        # configuration and refuse anything else in forward().
        self.qk_scale = None if qk_scale is None else float(qk_scale)     # common/mixste.py:52: qk_scale or d ** -0.5
        self.mlp_hidden = int(C_ * mlp_ratio)                             # common/mixste.py:101
        self.qkv_bias = bool(qkv_bias)
        self.drop_rate, self.attn_drop_rate = float(drop_rate), float(attn_drop_rate)   # nn.Dropout: identity in eval
        if self.qk_scale is not None and not self.qk_scale > 0:
            # `qk_scale or default` treats 0 as unset in the reference; a negative scale has no kernel here
            self.qk_scale = None if self.qk_scale == 0 else self.qk_scale
            if self.qk_scale is not None:
                raise ValueError("qk_scale must be positive")
        if self.mlp_hidden % 32 or not 0 < self.mlp_hidden <= 3 * C_:
            raise NotImplementedError(f"mlp hidden width int({C_} * {mlp_ratio}) = {self.mlp_hidden}: the kernels need a "
                                      f"multiple of 32, at most 3 * embed_dim_ratio")
        self.is_train = is_train
        self.num_frame, self.num_joints, self.in_chans = num_frame, num_joints, in_chans
        self.embed_dim, self.block_depth, self.num_heads = C_, depth, num_heads
        self.drop_path_rate = drop_path_rate

        self.Spatial_patch_to_embedding = nn.Linear(in_chans, C_)
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, num_joints, C_))
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, num_frame, C_))
        # index 0 stands for the parameter-free sinusoid, 2 for GELU: keys time_mlp.1.* / time_mlp.3.*
        self.time_mlp = nn.Sequential(nn.Identity(), nn.Linear(C_, C_ * 2), nn.GELU(), nn.Linear(C_ * 2, C_))
        self.STEblocks = nn.ModuleList([_BlockParams(C_, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.TTEblocks = nn.ModuleList([_BlockParams(C_, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.Spatial_norm = norm_layer(C_)
        self.Temporal_norm = norm_layer(C_)
        self.head = nn.Sequential(nn.LayerNorm(C_), nn.Linear(C_, 3))
        self.register_buffer("_freqs", sinusoid_frequencies(C_), persistent=False)
        if not self.qkv_bias:        # nn.Linear(bias=False): no key in the state dict; the kernels add these zeros
            self.register_buffer("_zero_qkv_bias", torch.zeros(3 * C_), persistent=False)
        self._wcache_by_device = {}    # device index -> (key, struct, split images, event, stream): shared with DataParallel replicas
        self.split_generation = {}     # device index -> how many times the split images were (re)made (graph caches key on it)
        self._param_names = tuple(n for n, _ in self.named_parameters())
        self.drop_fn = None            # tests: callable(block, branch, nseq, rate) -> DropPath factors [nseq] or None
        self.drop_key = None           # (key4, denoiser index) of the running training forward, set by a D3DP with train_draws =
        #                                "device": the DropPath table comes from noise stream v1 in ONE launch (ops.droppath_fill)
        self._drop_tables = {}         # device index -> (drop_path_rate, depth, keep float64 [2 depth], factor float32 [2 depth])
        self.operand_bf16 = MODE_F32   # matrix-product mode of the linear layers (_lib.PRECISIONS, include/pafuse_hip.h): 'f32' fp32 MFMA,
        #                                'bf16x3' split precision (the D3DP default), 'bf16x3_images' the same products on the image
        #                                pipeline (inference; where its kernels do not exist - training, the single-model variant -
        #                                images.effective_mode runs 'bf16x3'), 'f16x2' split precision (inference only), 'bf16' opt-in bf16
        #                                operands.  Which weight images a mode needs and how they are made: images.py
        self.fold_layernorm = None     # split-precision inference: norm1 / norm2 applied inside the qkv / fc1 GEMMs
        #                                (pafuse_block_weights.qkv_lt ...: g-scaled weight images + a vector per layer) - the producing
        #                                whole-row kernel stores the residual stream CENTRED on its row means and emits (mean, rstd), the
        #                                consumer's epilogue is rstd acc + lt: nothing cancels whatever the row means are (round 5 in mode
        #                                2; the image pipelines since round 4).  None = on; False = the whole-row kernels write the
        #                                normalised rows (same function, one more [M,C] store and normalise pass per whole-row launch)
        self.fuse_qkv_attention = None   # split-precision inference: qkv projection + attention of a block in ONE kernel where the
        #                                sequence length has a fused form (include/pafuse_hip.h pafuse_block_weights.qkv_hs): q, k, v
        #                                never reach memory.  None = on in 'f16x2' (+7 % on the loop), always on in 'bf16x3_images' (its
        #                                only form), off in 'bf16x3' (equal in time)
        self.fuse_mlp = None           # 'f16x2' with the LayerNorm folded and the residual stream as its image only: fc1 -> GELU -> fc2
        #                                of a block in ONE kernel, the hidden activations [M, 2C] stay in registers (include/pafuse_hip.h
        #                                pafuse_block_weights.fc2_hp).  None = on at the widths where it wins in the loop (224 and 256: the face and
        #                                the hands; equal or slower as a launch of its own, faster beside the other parts' kernels because it moves
        #                                8 C bytes per token less); True = wherever the kernel exists (also 384, where its 192 accumulator registers
        #                                leave one workgroup per CU: slower), mlp_ratio 2 only
        self.keep_f32_residual = False  # 'f16x2' with the LayerNorm folded: False keeps the residual stream between the blocks in memory
        #                                only as the two-fp16-slice image the GEMMs read (22-23 significant bits; measured: the loop stays
        #                                closer to an fp64 evaluation than the reference's fp32 arithmetic, tests/test_hip_parity.py);
        #                                True also keeps the fp32 rows (include/pafuse_hip.h pafuse_mixste2_weights.keep_f32_residual)
        self.use_side_stream = False   # training backward: weight-gradient GEMMs on a second stream (identical
        #                                results; measured 3 % slower than one stream per part at B=37, so off)
        self._side_by_device = {}

    # ------------------------------------------------------------------------------------------- C structs
    def weights_struct(self, images=True):
        """pafuse_mixste2_weights pointing at the live parameter storage (cached until a pointer changes).
        images=False (training): no pre-split / folded images - the training entry points split the weight a GEMM is
        about to read themselves (weights change every step)."""
        # attribute access, not named_parameters(): nn.DataParallel replicas keep their copies as plain attributes
        def get(name):
            if name.endswith("attn.qkv.bias") and not self.qkv_bias:
                return self._zero_qkv_bias
            return attrgetter(name)(self)
        mode = effective_mode(int(self.operand_bf16), self.embed_dim, self.mlp_hidden, self.num_heads, self.num_joints, self.num_frame,
                              training=not images)
        key = tuple(get(n).data_ptr() for n in self._param_names) + (self._freqs.data_ptr(), mode, bool(images),
                                                                     bool(self.keep_f32_residual), self.fuse_mlp)
        if not images:
            hit = self._wcache_by_device.get(("train", self._freqs.device.index))
            if hit is not None and hit[0] == key:
                return hit[1]
            w = _lib.MixSTE2Weights()
            fill_weights_struct(w, get, self._freqs, self.num_frame, self.num_joints, self.embed_dim,
                                self.block_depth, self.num_heads, self.in_chans, mode, None)
            w.mlp_hidden = self.mlp_hidden
            w.qk_scale = 0.0 if self.qk_scale is None else self.qk_scale
            self._wcache_by_device[("train", self._freqs.device.index)] = (key, w)
            return w
        split = mode >= MODE_BF16X3
        fold, fuse, fuse_mlp = resolve_options(mode, self.embed_dim, self.mlp_hidden, self.fold_layernorm, self.fuse_qkv_attention,
                                               self.fuse_mlp, self.keep_f32_residual)
        if split:           # the split images are values, not views: an in-place update of a weight must remake them
            key += tuple(get(n)._version for n in self._param_names if n.endswith(SPLIT_SUFFIXES))
        if fold or fuse:    # ... and so are the folded / head-major images and vectors: they also hold LayerNorm and bias values
            key += ("fold", fold, fuse) + tuple(get(n)._version for n in self._param_names if n.endswith(FOLD_SUFFIXES))
        dev = self._freqs.device
        # per device, in a dict the replicas of nn.DataParallel share with their parent (replicate() copies attributes
        # shallowly and makes fresh module objects on every forward: a per-object cache would never hit there, and every
        # replica would re-split all its weights on every call)
        # A replica made by nn.DataParallel never reads the cache: its parameters are fresh broadcast copies on every forward
        # (version 0, and the caching allocator hands out the same addresses again), so pointer + version cannot tell the
        # copies of two different parent states apart - the images (value copies) are remade per forward there, and kept
        # alive on the replica object itself.
        replica = bool(getattr(self, "_is_replica", False))
        hit = None if replica else self._wcache_by_device.get(dev.index)
        if hit is not None and hit[0] == key:
            if split and hit[3] is not None and torch.cuda.current_stream(dev) != hit[4]:
                torch.cuda.current_stream(dev).wait_event(hit[3])     # images were made on another stream
            return hit[1]
        w = _lib.MixSTE2Weights()
        images, event, stream = None, None, None
        if split:
            # one uint8 tensor per image, made on the device and kept until a weight changes (the cache key above)
            images = make_images(plan_images(self._param_names, mode, (fold, fuse, fuse_mlp)), get, mode, self.num_heads)
            stream = torch.cuda.current_stream(dev)
            event = torch.cuda.Event()
            event.record(stream)
            self.split_generation[dev.index] = self.split_generation.get(dev.index, 0) + 1
        fill_weights_struct(w, get, self._freqs, self.num_frame, self.num_joints, self.embed_dim,
                            self.block_depth, self.num_heads, self.in_chans, mode, images)
        w.mlp_hidden = self.mlp_hidden
        w.qk_scale = 0.0 if self.qk_scale is None else self.qk_scale
        w.keep_f32_residual = int(bool(self.keep_f32_residual))
        if replica:
            self._replica_keep = (w, images, event)      # alive as long as the replica (one forward)
        else:
            self._wcache_by_device[dev.index] = (key, w, images, event, stream)   # (images: keeps the storage the struct points into alive)
        return w

    # ---------------------------------------------------------------------------------------------- forward
    def forward(self, x_2d, x_3d, t):
        """eval: x_2d [B,F,J,2], x_3d [B,P,F,J,3], t [B] int64 -> [B,P,F,J,3]  (common/mixste.py:278-298);
        train: x_3d [B,F,J,3] -> [B,F,J,3], differentiable w.r.t. the parameters (common/mixste.py:215-225)."""
        lib = _lib.load()
        if not x_3d.is_cuda:
            raise _lib.PafuseError("MixSTE2 runs on the HIP device only (no CPU fallback)")
        if self.is_train:
            if (self.qk_scale is not None or not self.qkv_bias or self.mlp_hidden != 2 * self.embed_dim or self.drop_rate
                    or self.attn_drop_rate):
                raise NotImplementedError("training implements the PAFUSE configuration: qkv_bias=True, qk_scale=None, "
                                          "mlp_ratio=2, no dropout (common/diffusionpose.py:144-147)")
            if self.operand_bf16 in (MODE_BF16, MODE_F16X2):
                raise NotImplementedError("rounded-bf16 and f16x2 products are inference options; training runs fp32 ('f32') "
                                          "or split-precision ('bf16x3') products")
            return self._forward_train(x_2d, x_3d, t)
        B, P, F, J = self._check_inputs(x_2d, x_3d, t, 5)
        x_2d = x_2d.contiguous().float()
        x_3d = x_3d.contiguous().float()
        t = t.contiguous().long()
        w = self.weights_struct()
        out = torch.empty(B, P, F, J, 3, device=x_3d.device, dtype=torch.float32)
        nbytes = lib.pafuse_mixste2_workspace_bytes(C.byref(w), B, P)
        ws = _lib.workspace(nbytes, x_3d.device, "mixste2_forward")
        stream = torch.cuda.current_stream(x_3d.device).cuda_stream
        _lib.check(lib.pafuse_mixste2_forward(C.byref(w), x_2d.data_ptr(), x_3d.data_ptr(), t.data_ptr(), B, P,
                                              out.data_ptr(), ws.data_ptr(), nbytes, stream))
        return out

    def _check_inputs(self, x_2d, x_3d, t, ndim):
        """The kernels index by (B, P, F, J): refuse anything else on the host instead of faulting on the device."""
        if x_3d.dim() != ndim or x_3d.shape[-1] != 3:
            raise ValueError(f"x_3d must be [B,{'P,' if ndim == 5 else ''}F,J,3], got {tuple(x_3d.shape)}")
        B, P = x_3d.shape[0], (x_3d.shape[1] if ndim == 5 else 1)
        F, J = x_3d.shape[-3], x_3d.shape[-2]
        if (F, J) != (self.num_frame, self.num_joints):
            raise ValueError(f"this MixSTE2 was built for {self.num_frame} frames x {self.num_joints} joints, got {F} x {J}")
        if tuple(x_2d.shape) != (B, F, J, 2) or tuple(t.shape) != (B,):
            raise ValueError(f"x_2d must be [{B},{F},{J},2] and t [{B}], got {tuple(x_2d.shape)} and {tuple(t.shape)}")
        if x_2d.device != x_3d.device or t.device != x_3d.device:
            raise ValueError("x_2d, x_3d and t must live on the same device")
        return B, P, F, J

    # ------------------------------------------------------------------------------------------------ training
    def side_stream(self, device):
        if not self.use_side_stream:
            return None
        if device.index not in self._side_by_device:
            self._side_by_device[device.index] = torch.cuda.Stream(device=device)
        return self._side_by_device[device.index]

    def drop_path_factors(self, B, device):
        """DropPath factors (mask / keep) of one forward, [2*depth, 2, B*max(F,J)] or None, drawn as the reference's
        blocks draw them: execution order STE0 (attn, mlp), TTE0, STE1, ...; one Bernoulli(keep) per sequence of the
        block's batch axis ((b f) spatial, (b n) temporal); rate 0 is nn.Identity and draws nothing
        (common/mixste.py:100,113-116,187; timm.layers.drop_path with scale_by_keep=True)."""
        if self.drop_key is not None:
            return self._drop_path_factors_seeded(B, device)
        rates = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.block_depth)]
        if not self.training or all(r <= 0.0 for r in rates):
            return None
        smax = B * max(self.num_frame, self.num_joints)
        out = torch.ones(2 * self.block_depth, 2, smax, device=device, dtype=torch.float32)
        for i, rate in enumerate(rates):
            for k, nseq in ((2 * i, B * self.num_frame), (2 * i + 1, B * self.num_joints)):
                for branch in range(2):
                    if self.drop_fn is not None:
                        m = self.drop_fn(k, branch, nseq, rate)
                    elif rate > 0.0:
                        keep = 1.0 - rate
                        m = torch.empty((nseq, 1, 1), device=device, dtype=torch.float32).bernoulli_(keep)
                        if keep > 0.0:
                            m.div_(keep)
                    else:
                        m = None
                    if m is not None:
                        out[k, branch, :nseq] = m.reshape(nseq).to(device=device, dtype=torch.float32)
        return out

    def drop_path_tables(self, device):
        """(rates, keep float64 [2 depth], factor float32 [2 depth]) of the seeded DropPath draws, made on the host as the torch
        path makes them - rate = linspace(0, drop_path_rate, depth)[i].item(), keep = 1.0 - rate in double, factor =
        torch.ones(()).div_(keep) - once per module and device; block k of the execution order belongs to layer k // 2."""
        device = torch.device(device)
        hit = self._drop_tables.get(device.index)
        if hit is None or hit[0] != (self.drop_path_rate, self.block_depth):
            rates = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.block_depth)]
            keep = [1.0 - r if r > 0.0 else 1.0 for r in rates]
            factor = [float(torch.ones(()).div_(k)) if k > 0.0 else 1.0 for k in keep]       # keep = 0: nothing is ever kept
            keep2 = torch.tensor([k for k in keep for _ in range(2)], dtype=torch.float64)
            factor2 = torch.tensor([f for f in factor for _ in range(2)], dtype=torch.float32)
            hit = self._drop_tables[device.index] = ((self.drop_path_rate, self.block_depth), rates, keep2.to(device), factor2.to(device))
        return hit[1:]

    def _drop_path_factors_seeded(self, B, device):
        """drop_path_factors from noise stream v1: the same table, in one launch, a pure function of
        (seed, call, denoiser, global clip index)."""
        from . import ops
        if self.drop_fn is not None:
            raise ValueError("drop_fn injects DropPath factors into the torch draws: it cannot be combined with a stream key "
                             "(D3DP.train_draws = 'device')")
        key4, denoiser = self.drop_key
        rates, keep, factor = self.drop_path_tables(device)
        if not self.training or all(r <= 0.0 for r in rates):
            return None
        return ops.droppath_fill(key4, denoiser, self.block_depth, self.num_frame, self.num_joints, B, keep, factor)

    def _forward_train(self, x_2d, x_3d, t):
        B, _, F, J = self._check_inputs(x_2d, x_3d, t, 4)
        drop = self.drop_path_factors(B, x_3d.device)
        params = [attrgetter(n)(self) for n in self._param_names]
        return _TrainFunction.apply(self, x_2d.contiguous().float(), x_3d.contiguous().float(), t.contiguous().long(),
                                    drop, *params)


class _TrainFunction(torch.autograd.Function):
    """pafuse_mixste2_train_forward / _backward (include/pafuse_hip.h) as one autograd node: the forward leaves its
    activations in a library-owned layout inside one byte tensor, the backward fills one gradient per parameter."""

    @staticmethod
    def forward(ctx, module, x_2d, x_3d, t, drop, *params):
        lib = _lib.load()
        w = module.weights_struct(images=False)
        B, F, J, _ = x_3d.shape
        nbytes = lib.pafuse_mixste2_train_bytes(C.byref(w), B)
        if nbytes == 0:
            raise _lib.PafuseError("pafuse_mixste2_train_bytes: unsupported configuration")
        saved = _lib.workspace(nbytes, x_3d.device, "mixste2_train")
        out = torch.empty(B, F, J, 3, device=x_3d.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(x_3d.device).cuda_stream
        _lib.check(lib.pafuse_mixste2_train_forward(C.byref(w), x_2d.data_ptr(), x_3d.data_ptr(), t.data_ptr(), B,
                                                    drop.data_ptr() if drop is not None else None, out.data_ptr(),
                                                    saved.data_ptr(), nbytes, stream))
        ctx.module, ctx.saved, ctx.drop, ctx.B, ctx.nbytes = module, saved, drop, B, nbytes
        ctx.keep = (x_2d, x_3d, t)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        module = ctx.module
        w = module.weights_struct(images=False)
        shapes = [attrgetter(n)(module).shape for n in module._param_names]
        sizes = [(s.numel() + 3) // 4 * 4 for s in shapes]               # keep every gradient 16-byte aligned
        flat = torch.zeros(sum(sizes), device=dout.device, dtype=torch.float32)    # one fill instead of 208
        grads, at = {}, 0
        for n, shape, size in zip(module._param_names, shapes, sizes):
            grads[n] = flat[at:at + shape.numel()].view(shape)
            at += size
        gw = _lib.MixSTE2Weights()
        fill_weights_struct(gw, grads.__getitem__, module._freqs, module.num_frame, module.num_joints,
                            module.embed_dim, module.block_depth, module.num_heads, module.in_chans)
        dout = dout.contiguous().float()
        stream = torch.cuda.current_stream(dout.device)
        side = module.side_stream(dout.device)
        _lib.check(lib.pafuse_mixste2_train_backward(C.byref(w), C.byref(gw), dout.data_ptr(), ctx.B,
                                                     ctx.drop.data_ptr() if ctx.drop is not None else None,
                                                     ctx.saved.data_ptr(), ctx.nbytes, stream.cuda_stream,
                                                     side.cuda_stream if side is not None else None))
        if side is not None:                     # the library joined the streams; tell the allocator about the use
            for tensor in (flat, ctx.saved, dout):
                tensor.record_stream(side)
        ctx.saved = None
        return (None, None, None, None, None) + tuple(grads[n] for n in module._param_names)


MODEL_PARAMS = (("patch_w", "Spatial_patch_to_embedding.weight"), ("patch_b", "Spatial_patch_to_embedding.bias"),
                ("pos_spatial", "Spatial_pos_embed"), ("pos_temporal", "Temporal_pos_embed"),
                ("tm1_w", "time_mlp.1.weight"), ("tm1_b", "time_mlp.1.bias"), ("tm3_w", "time_mlp.3.weight"),
                ("tm3_b", "time_mlp.3.bias"), ("snorm_w", "Spatial_norm.weight"), ("snorm_b", "Spatial_norm.bias"),
                ("tnorm_w", "Temporal_norm.weight"), ("tnorm_b", "Temporal_norm.bias"), ("hnorm_w", "head.0.weight"),
                ("hnorm_b", "head.0.bias"), ("head_w", "head.1.weight"), ("head_b", "head.1.bias"))


def fill_weights_struct(w, get, freqs, frames, joints, channels, depth, heads, in_chans, operand_bf16=0, split=None):
    """Fill a pafuse_mixste2_weights from ``get(state-dict key) -> tensor`` (keys as in common/mixste.py); ``split`` is the
    image dict of the split modes (images.make_images)."""
    if depth > _lib.MAX_DEPTH:
        raise _lib.PafuseError(f"depth {depth} > {_lib.MAX_DEPTH}")
    w.frames, w.joints, w.channels, w.depth, w.heads, w.in_chans = frames, joints, channels, depth, heads, in_chans
    w.operand_bf16 = int(operand_bf16)
    for field, key in MODEL_PARAMS:
        setattr(w, field, _ptr(get(key), key))
    w.freqs = _ptr(freqs, "freqs")
    for dst, prefix in ((w.ste, "STEblocks"), (w.tte, "TTEblocks")):
        for i in range(depth):
            fill_block_struct(dst[i], get, f"{prefix}.{i}.", split)

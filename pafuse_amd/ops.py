"""Thin tensor-level wrappers over the unit entry points of the C ABI (used by the parity tests).

Every wrapper checks operand shapes on the host and launches with the operands' device current."""
import ctypes as C
import math
from operator import attrgetter

import torch

from . import _lib
from ._lib import IMAGE_BYTES, MODE_BF16X3, MODE_F16X2, PRECISIONS, SPLIT_FLAG      # (PRECISIONS: as pafuse_amd.D3DP.PRECISIONS)
from .images import _ptr, block_images, effective_mode, fill_block_struct, fused_mlp_fc2_image, head_major_qkv, split_image


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need(cond, msg):
    """host-side operand check: a kernel launched on mismatched shapes faults on the device"""
    if not cond:
        raise ValueError(msg)


def _data(t):
    return t.data_ptr() if t.numel() else None   # an empty tensor has no storage to point the library at


def _need_pred(who, pred, axis="P_r"):
    _need(pred.dim() == 6 and pred.shape[-1] == 3, f"{who}: pred must be [B,T,{axis},F,J,3], got {tuple(pred.shape)}")
    return pred.shape[:5]


def _need_tensors(who, f32, i32):
    """the fp32 operands `f32` and the int32 tables `i32`: contiguous, all on the HIP device of the first"""
    _need(all(t.is_cuda and t.device == f32[0].device and t.is_contiguous() for t in (*f32, *i32)),
          f"{who}: contiguous tensors on one HIP device (no CPU fallback)")
    _need(all(t.dtype == torch.float32 for t in f32) and all(t.dtype == torch.int32 for t in i32), f"{who}: dtypes")


def _state_out(who, out, need, dev):
    """the flat float64 buffer a partials op writes its `need` bytes of state into: `out`, or a new one"""
    if out is None:
        out = torch.empty(need // 8, device=dev, dtype=torch.float64)
    _need(out.is_cuda and out.device == dev and out.dtype == torch.float64 and out.dim() == 1 and out.is_contiguous()
          and out.numel() * 8 >= need, f"{who}: out must be a float64 buffer of {need} bytes or more on {dev}")
    return out


def _need_rows(t, head, msg, strided=False, like=None):
    """operand rows of a combine op: [W >= 1, >= head] float64 on a HIP device, contiguous or (strided) a column slice of
    a wider buffer with rows `head` or more apart; `like`: on its device and with as many rows"""
    ok = t.dim() == 2 and t.dtype == torch.float64 and t.is_cuda and t.shape[0] >= 1 and t.shape[1] >= head
    ok = ok and (like is None or (t.device == like.device and t.shape[0] == like.shape[0]))
    _need(ok and ((t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= head)) if strided else t.is_contiguous()), msg)


def _need_merged(who, merged, states, head, size, span, over):
    """the buffer a combine op merges into: `head` (in words: `size`) float64 or more on the device of `states`.  `over`:
    what it may lie over of the `span` elements read from there - "first": states[0] alone, "none", None: not checked"""
    _need(merged.is_cuda and merged.device == states.device and merged.dtype == torch.float64 and merged.is_contiguous()
          and merged.numel() >= head, f"{who}: merged must hold {size} float64")
    lo, at = states.data_ptr(), merged.data_ptr()
    overlap = at < lo + 8 * span and at + 8 * head > lo
    if over == "first":
        _need(at == lo or not overlap, f"{who}: of its operands the merged state may only lie over the first")
    elif over == "none":
        _need(not overlap, f"{who}: a merge over its own operands cannot also write the maps")


def linear(x, weight, bias, act=None, bf16=False):
    """nn.Linear (+ exact GELU when act == 'gelu') on the last dim of a contiguous fp32 tensor; bf16=True rounds both
    operands to bf16 in registers (fp32 accumulate)."""
    lib = _lib.load()
    K = x.shape[-1]
    N = weight.shape[0]
    _need(tuple(weight.shape) == (N, K) and bias.numel() == N, f"linear: x [..,{K}] needs weight [N,{K}] and bias [N]")
    x2 = x.contiguous().view(-1, K)
    out = torch.empty(x2.shape[0], N, device=x.device, dtype=torch.float32)
    if x2.shape[0] == 0:      # no rows: nothing to launch (an empty tensor has no storage to point the library at)
        return out.view(*x.shape[:-1], N)
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_linear(_ptr(x2, "x"), _ptr(weight, "weight"), _ptr(bias, "bias"), out.data_ptr(),
                                     x2.shape[0], N, K, (1 if act == "gelu" else 0) | (2 if bf16 else 0), _stream(x)))
    return out.view(*x.shape[:-1], N)


def layer_norm(x, weight, bias, eps):
    lib = _lib.load()
    Cc = x.shape[-1]
    _need(weight.numel() == Cc and bias.numel() == Cc, f"layer_norm: weight and bias must have {Cc} elements")
    x2 = x.contiguous().view(-1, Cc)
    out = torch.empty_like(x2)
    if x2.shape[0] == 0:
        return out.view_as(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_layernorm(_ptr(x2, "x"), _ptr(weight, "w"), _ptr(bias, "b"), out.data_ptr(), x2.shape[0],
                                        Cc, eps, _stream(x)))
    return out.view_as(x)


def attention(qkv, heads, nseq, L, group=1, group_stride=None, seq_stride=0, tok_stride=1):
    """softmax(q k^T d^-1/2) v on a [M,3C] qkv matrix; default addressing = contiguous sequences of L rows."""
    lib = _lib.load()
    M, C3 = qkv.shape
    Cc = C3 // 3
    gs = L if group_stride is None else group_stride
    _need(C3 % 3 == 0 and Cc % heads == 0 and nseq >= 0 and group >= 1, "attention: qkv must be [M, 3*heads*d]")
    if nseq:   # the last row any sequence touches must exist
        last = ((nseq - 1) // group) * gs + ((nseq - 1) % group) * seq_stride + (L - 1) * tok_stride
        _need(0 <= last < M and min(gs, seq_stride, tok_stride) >= 0, f"attention: sequences reach row {last} of {M}")
    o = torch.zeros(M, Cc, device=qkv.device, dtype=torch.float32)
    if M == 0 or nseq == 0:
        return o
    with torch.cuda.device(qkv.device):
        _lib.check(lib.pafuse_attention(_ptr(qkv, "qkv"), o.data_ptr(), nseq, L, Cc, heads, group,
                                        L if group_stride is None else group_stride, seq_stride, tok_stride,
                                        _stream(qkv)))
    return o


def attention_backward(qkv, d_o, heads, nseq, L, group=1, group_stride=None, seq_stride=0, tok_stride=1):
    """dqkv [M,3C] of attention(): the training step's attention backward kernel on its own (rows no sequence touches: 0)."""
    lib = _lib.load()
    M, C3 = qkv.shape
    Cc = C3 // 3
    gs = L if group_stride is None else group_stride
    _need(C3 % 3 == 0 and Cc % heads == 0 and nseq >= 0 and group >= 1 and tuple(d_o.shape) == (M, Cc),
          "attention_backward: qkv must be [M, 3*heads*d] and d_o [M, heads*d]")
    if nseq:
        last = ((nseq - 1) // group) * gs + ((nseq - 1) % group) * seq_stride + (L - 1) * tok_stride
        _need(0 <= last < M and min(gs, seq_stride, tok_stride) >= 0, f"attention_backward: sequences reach row {last} of {M}")
    dqkv = torch.zeros(M, C3, device=qkv.device, dtype=torch.float32)
    with torch.cuda.device(qkv.device):
        _lib.check(lib.pafuse_attention_backward(_ptr(qkv, "qkv"), _ptr(d_o, "d_o"), dqkv.data_ptr(), nseq, L, Cc, heads, group,
                                                 gs, seq_stride, tok_stride, _stream(qkv)))
    return dqkv


def linear_weight_grad(d_y, x, precision="bf16x3", bias=True):
    """(dW [N,K], db [N] or None) = (d_y^T x, column sums of d_y) for d_y [M,N], x [M,K]: the weight / bias gradient kernels of
    the training step on their own; precision 'bf16x3' (split products) or 'f32'."""
    lib = _lib.load()
    _need(precision in ("bf16x3", "f32"), "linear_weight_grad: precision 'bf16x3' or 'f32'")
    M, N = d_y.shape
    K = x.shape[1]
    _need(x.shape[0] == M, "linear_weight_grad: d_y [M,N] and x [M,K]")
    dw = torch.zeros(N, K, device=x.device, dtype=torch.float32)
    db = torch.zeros(N, device=x.device, dtype=torch.float32) if bias else None
    nbytes = lib.pafuse_linear_weight_grad_bytes()
    ws = _lib.workspace(nbytes, x.device, "linear_weight_grad")
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_linear_weight_grad(_ptr(d_y, "d_y"), _ptr(x, "x"), dw.data_ptr(), db.data_ptr() if bias else None, M, N, K,
                                                 PRECISIONS[precision], ws.data_ptr(), nbytes, _stream(x)))
    return dw, db




def _out_buf(out, name, shape, dev, zero=False):
    """a preallocated output from `out` (contiguous, at least as large: nothing past the used part is written) or a new one"""
    n = shape[0] * shape[1] if len(shape) == 2 else shape[0]
    t = out.get(name) if out else None
    if t is None:
        return (torch.zeros if zero else torch.empty)(shape, device=dev, dtype=torch.float32)
    _need(t.is_contiguous() and t.dtype == torch.float32 and t.numel() >= n, f"output '{name}' must be contiguous fp32 of >= {n} elements")
    return t


def _unit_workspace(lib, M, N, K, dev):
    nbytes = lib.pafuse_train_unit_bytes(M, N, K)
    return _lib.workspace(nbytes, dev, "train_unit"), nbytes


def layer_norm_backward(dy, x, weight, eps, add=None, drop=None, seq_map=(0, 1, 1), scaled=False, branch=False, out=None):
    """The training step's LayerNorm backward on its own (pafuse_layernorm_backward -> ln_backward): dx = add + LN'(x)^T dy,
    out_scaled = drop[seq(m)] dx (scaled=True), and dw += sum dy xh, db += sum dy, dbranch += column sums of out_scaled
    (branch=True).  dy, x, add [M,C]; drop [nseq] with seq_map = (temporal, J, FJ).  out: preallocated outputs by name ('dx',
    'out_scaled', 'dw', 'db', 'dbranch'); the gradients are ADDED into the given dw / db / dbranch (new ones start at 0); 'dx'
    may be `add` itself.  Returns a dict of the outputs ('dx', 'dw', 'db', and 'out_scaled' / 'dbranch' when asked for)."""
    lib = _lib.load()
    M, Cc = x.shape
    _need(tuple(dy.shape) == (M, Cc) and weight.numel() == Cc and (add is None or tuple(add.shape) == (M, Cc)),
          "layer_norm_backward: dy, x, add [M,C] and weight [C]")
    _need(not branch or scaled, "layer_norm_backward: the branch's bias gradient is the column sums of out_scaled")
    dev = x.device
    res = {"dx": _out_buf(out, "dx", (M, Cc), dev), "dw": _out_buf(out, "dw", (Cc,), dev, True),
           "db": _out_buf(out, "db", (Cc,), dev, True)}
    if scaled:
        res["out_scaled"] = _out_buf(out, "out_scaled", (M, Cc), dev)
    if branch:
        res["dbranch"] = _out_buf(out, "dbranch", (Cc,), dev, True)
    a = _lib.LnbArgs()
    a.dy, a.x, a.w, a.eps = _ptr(dy, "dy"), _ptr(x, "x"), _ptr(weight, "weight"), float(eps)
    a.add = _ptr(add, "add") if add is not None else None
    a.dx = res["dx"].data_ptr()
    if drop is not None:
        a.drop = _ptr(drop, "drop")
    a.temporal, a.J, a.FJ = (int(v) for v in seq_map)
    a.out_scaled = res["out_scaled"].data_ptr() if scaled else None
    a.dw, a.db = res["dw"].data_ptr(), res["db"].data_ptr()
    a.dbranch = res["dbranch"].data_ptr() if branch else None
    a.M, a.C = M, Cc
    ws, nbytes = _unit_workspace(lib, M, Cc, 0, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_layernorm_backward(C.byref(a), ws.data_ptr(), nbytes, _stream(x)))
    for name in ("dx", "out_scaled"):
        if name in res:
            res[name] = res[name].reshape(-1)[:M * Cc].view(M, Cc)
    for name in ("dw", "db", "dbranch"):
        if name in res:
            res[name] = res[name].reshape(-1)[:Cc]
    return res


def linear_input_grad(d_y, weight, dact_u=None, precision="bf16x3", image_source=0, out=None):
    """The training step's dX GEMM on its own (pafuse_linear_input_grad -> input_grad): dX [M,K] = d_y [M,N] weight [N,K],
    times gelu'(dact_u) [M,K] when given.  precision 'bf16x3' (split products on the M16 image of W^T where the step takes
    them, M >= 128; image_source 0: split_weights_transposed_kernel, 1: the batch kernel the step uses) or 'f32'.
    out: a preallocated [>= M*K] output."""
    lib = _lib.load()
    M, N = d_y.shape
    K = weight.shape[1]
    _need(tuple(weight.shape) == (N, K) and (dact_u is None or tuple(dact_u.shape) == (M, K)),
          "linear_input_grad: d_y [M,N], weight [N,K], dact_u [M,K]")
    dev = d_y.device
    dx = _out_buf({"dx": out} if out is not None else None, "dx", (M, K), dev)
    ws, nbytes = _unit_workspace(lib, M, N, K, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_linear_input_grad(_ptr(d_y, "d_y"), _ptr(weight, "weight"), _ptr(dact_u, "dact_u") if dact_u is not None else None,
                                                dx.data_ptr(), M, N, K, PRECISIONS[precision], int(image_source), ws.data_ptr(), nbytes,
                                                _stream(d_y)))
    return dx.reshape(-1)[:M * K].view(M, K)


def linear_train(x, weight, bias, gelu=True, precision="bf16x3", out=None):
    """The training forward's plain linear layer on its own (pafuse_linear_train -> plain_linear): u = x W^T + b and, with
    gelu=True, h = gelu(u) from the same epilogue (mlp.fc1; the time MLP at M < 128).  out: preallocated 'u' / 'h'.
    Returns (u, h or None)."""
    lib = _lib.load()
    M, K = x.shape
    N = weight.shape[0]
    _need(tuple(weight.shape) == (N, K) and bias.numel() == N, "linear_train: x [M,K], weight [N,K], bias [N]")
    dev = x.device
    u = _out_buf(out, "u", (M, N), dev)
    h = _out_buf(out, "h", (M, N), dev) if gelu else None
    ws, nbytes = _unit_workspace(lib, M, N, K, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_linear_train(_ptr(x, "x"), _ptr(weight, "weight"), _ptr(bias, "bias"), u.data_ptr(),
                                           h.data_ptr() if gelu else None, M, N, K, PRECISIONS[precision], ws.data_ptr(), nbytes,
                                           _stream(x)))
    view = lambda t: t.reshape(-1)[:M * N].view(M, N)
    return view(u), (view(h) if gelu else None)


def gelu_backward(u, dh, db=None, in_place=False):
    """The training step's GELU backward on its own (pafuse_gelu_backward -> gelu_bwd): du = dh gelu'(u) (in_place: written
    over dh) and db += column sums of du (db None: a new zero vector).  Returns (du, db)."""
    lib = _lib.load()
    M, N = u.shape
    _need(tuple(dh.shape) == (M, N), "gelu_backward: u and dh [M,N]")
    dev = u.device
    du = dh if in_place else torch.empty(M, N, device=dev, dtype=torch.float32)
    db = torch.zeros(N, device=dev, dtype=torch.float32) if db is None else db
    _need(db.is_contiguous() and db.numel() == N, "gelu_backward: db [N]")
    ws, nbytes = _unit_workspace(lib, M, N, 0, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_gelu_backward(_ptr(u, "u"), _ptr(dh, "dh"), _ptr(du, "du"), db.data_ptr(), M, N, ws.data_ptr(), nbytes,
                                            _stream(u)))
    return du, db


def _rim_workspace(nbytes, dev):
    """the workspace of a first- / last-layer unit entry, every float a NaN: a partial sum a kernel fails to write shows in the result"""
    ws = _lib.workspace(nbytes, dev, "train_rim")
    return ws if _lib._workspace_policy is not None else ws.fill_(0xFF)     # (an installed policy decides what the arena holds)


def train_head_grad(dout, hn, head_w, out=None):
    """The training step's output-head backward on its own (pafuse_train_head_grad -> head_grad): for out = hn head_w^T + b with
    dout [M,3], hn [M,C], head_w [3,C]: d_head_w [3,C] += dout^T hn, d_head_b [3] += column sums of dout, dhn [M,C] = dout head_w.
    out: preallocated outputs by name; the gradients are ADDED into a given 'd_head_w' / 'd_head_b' (new ones start at 0), 'dhn'
    is overwritten.  Returns a dict of the three."""
    lib = _lib.load()
    M, Cc = hn.shape
    _need(tuple(dout.shape) == (M, 3) and tuple(head_w.shape) == (3, Cc), "train_head_grad: dout [M,3], hn [M,C], head_w [3,C]")
    dev = hn.device
    res = {"d_head_w": _out_buf(out, "d_head_w", (3, Cc), dev, True), "d_head_b": _out_buf(out, "d_head_b", (3,), dev, True),
           "dhn": _out_buf(out, "dhn", (M, Cc), dev)}
    nbytes = lib.pafuse_train_head_grad_bytes(M, Cc)
    ws = _rim_workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_train_head_grad(_ptr(dout, "dout"), _ptr(hn, "hn"), _ptr(head_w, "head_w"), res["d_head_w"].data_ptr(),
                                              res["d_head_b"].data_ptr(), res["dhn"].data_ptr(), M, Cc, ws.data_ptr(), nbytes,
                                              _stream(hn)))
    return {"d_head_w": res["d_head_w"].reshape(-1)[:3 * Cc].view(3, Cc), "d_head_b": res["d_head_b"].reshape(-1)[:3],
            "dhn": res["dhn"].reshape(-1)[:M * Cc].view(M, Cc)}


def train_patch_grad(x2d, x3d, g, out=None):
    """The training step's first-layer backward on its own (pafuse_train_patch_grad -> concat_inputs, patch_grad): for
    x0 = (x2d | x3d) patch_w^T + patch_b + pos_spatial[j] + temb[b] with x2d [B,F,J,2], x3d [B,F,J,3], g = d x0 [B,F,J,C]:
    d_patch_w [C,5] += g^T (x2d | x3d), d_patch_b [C] += column sums of g, d_pos_spatial [J,C] += sums over (b, f),
    dtemb [B,C] = sums over (f, j).  out: preallocated outputs by name; the three gradients are ADDED into given ones (new ones
    start at 0), 'dtemb' is overwritten.  Returns a dict of the four."""
    lib = _lib.load()
    B, F, J, Cc = g.shape
    _need(tuple(x2d.shape) == (B, F, J, 2) and tuple(x3d.shape) == (B, F, J, 3), "train_patch_grad: x2d [B,F,J,2], x3d [B,F,J,3], g [B,F,J,C]")
    dev = g.device
    shapes = {"d_patch_w": (Cc, 5), "d_patch_b": (Cc,), "d_pos_spatial": (J, Cc), "dtemb": (B, Cc)}
    res = {k: _out_buf(out, k, s, dev, k != "dtemb") for k, s in shapes.items()}
    nbytes = lib.pafuse_train_patch_grad_bytes(B, F, J, Cc)
    ws = _rim_workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_train_patch_grad(_ptr(x2d, "x2d"), _ptr(x3d, "x3d"), _ptr(g, "g"), res["d_patch_w"].data_ptr(),
                                               res["d_patch_b"].data_ptr(), res["d_pos_spatial"].data_ptr(), res["dtemb"].data_ptr(),
                                               B, F, J, Cc, ws.data_ptr(), nbytes, _stream(g)))
    return {k: res[k].reshape(-1)[:math.prod(s)].view(s) for k, s in shapes.items()}


def train_group_sum(x, mode, out=None, accumulate=True):
    """The training step's embedding-gradient sums on their own (pafuse_train_group_sum -> group_sum): x [B,F,J,C] summed over the
    rows of each group - mode 0: per joint -> [J,C], 1: per frame -> [F,C], 2: per sample -> [B,C].  accumulate: ADDED into `out`
    (None: a new zero tensor), else `out` is overwritten."""
    lib = _lib.load()
    B, F, J, Cc = x.shape
    _need(mode in (0, 1, 2), "train_group_sum: mode 0, 1 or 2")
    G = (J, F, B)[mode]
    dev = x.device
    res = _out_buf({"out": out} if out is not None else None, "out", (G, Cc), dev, True)
    nbytes = lib.pafuse_train_group_sum_bytes(mode, B, F, J, Cc)
    ws = _rim_workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_train_group_sum(_ptr(x, "x"), res.data_ptr(), mode, 1 if accumulate else 0, B, F, J, Cc, ws.data_ptr(),
                                              nbytes, _stream(x)))
    return res.reshape(-1)[:G * Cc].view(G, Cc)


def train_sinusoid(t, freqs, out=None):
    """The time MLP's input as the training forward forms it (pafuse_train_sinusoid -> sinusoid): t int64 [B], freqs [C/2] ->
    [B,C] = [sin(t freqs) | cos(t freqs)], the argument one fp32 product.  out: a preallocated [>= B*C] output."""
    lib = _lib.load()
    _need(t.dim() == 1 and t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and freqs.dim() == 1, "train_sinusoid: t int64 [B], freqs [C/2]")
    B, Cc = t.shape[0], 2 * freqs.shape[0]
    dev = t.device
    res = _out_buf({"out": out} if out is not None else None, "out", (B, Cc), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_train_sinusoid(_data(t), _ptr(freqs, "freqs"), res.data_ptr(), B, Cc, _stream(t)))
    return res.reshape(-1)[:B * Cc].view(B, Cc)


def block_forward(block_params, x, heads=8, precision="f32"):
    """Block.forward (common/mixste.py:113-116) on [S,L,C]; ``block_params`` is a pafuse_amd.mixste2._BlockParams;
    ``precision`` the matrix-product mode of its four linear layers (the split modes make their weight images here;
    'bf16x3_images' runs the image pipeline where it has kernels for the shape, else the 'bf16x3' kernels)."""
    lib = _lib.load()
    S, L, Cc = x.shape
    _need(block_params.norm1.weight.numel() == Cc and Cc % heads == 0, f"block: parameters are not for width {Cc}")
    _need(precision in PRECISIONS, f"precision must be one of {sorted(PRECISIONS)}")
    y = x.contiguous().clone()
    w = _lib.BlockWeights()
    mode = effective_mode(PRECISIONS[precision], Cc, 0, heads, L, L)
    get = lambda key: attrgetter(key)(block_params)      # noqa: E731
    images = block_images(get, mode, heads)
    fill_block_struct(w, get, images=images, what=lambda key: key.split(".")[-2])
    nbytes = lib.pafuse_block_workspace_bytes(S * L, Cc)
    ws = _lib.workspace(nbytes, x.device, "block_forward")
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_block_forward(C.byref(w), y.data_ptr(), S, L, Cc, heads, mode, ws.data_ptr(),
                                            nbytes, _stream(x)))
    del images      # (stream-ordered: the caching allocator reuses the blocks only for later work on this stream)
    return y


def time_embed(model, t, out=None):
    """MixSTE2.time_mlp(t) for a pafuse_amd.MixSTE2 (into `out` [B,C] when given)."""
    lib = _lib.load()
    w = model.weights_struct()
    _need(t.dim() == 1, "time_embed: t must be [B]")
    t = t.contiguous().long()
    if out is None:
        out = torch.empty(t.shape[0], model.embed_dim, device=t.device, dtype=torch.float32)
    _need(out.is_cuda and out.device == t.device and out.dtype == torch.float32 and out.is_contiguous() and
          tuple(out.shape) == (t.shape[0], model.embed_dim), "time_embed: out must be a contiguous fp32 [B,C] on the device of t")
    hid = torch.empty(t.shape[0], 2 * model.embed_dim, device=t.device, dtype=torch.float32)
    with torch.cuda.device(t.device):
        _lib.check(lib.pafuse_time_embed(C.byref(w), t.data_ptr(), t.shape[0], out.data_ptr(), hid.data_ptr(), _stream(t)))
    return out


def _embed_operands(x3d, x2d, patch_w, patch_b, pos_spatial, temb, norm_w, norm_b, joints, perm, x2d_flip):
    """host checks shared by embed and embed_unit -> (B, P, F, J, J3, C, nflip, {name: pointer of an index table})"""
    B, P, F, J3, _ = x3d.shape
    Cc = patch_w.shape[0]
    nflip = 2 if x2d_flip is not None else 1
    J = J3 if joints is None else int(joints.numel())
    _need(tuple(x3d.shape) == (B, P, F, J3, 3) and tuple(x2d.shape) == (B, F, J3, 2), "embed: x3d [B,P,F,J3,3], x2d [B,F,J3,2]")
    _need(tuple(patch_w.shape) == (Cc, 5) and patch_b.numel() == Cc and tuple(pos_spatial.shape[-2:]) == (J, Cc) and
          tuple(temb.shape) == (B, Cc) and norm_w.numel() == Cc and norm_b.numel() == Cc, "embed: parameter shapes")
    idx = {}
    for name, t, n in (("joints", joints, J), ("perm", perm, J3)):
        if t is not None:
            _need(t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == n, f"embed: {name} int32 [{n}]")
            _need(int(t.min()) >= 0 and int(t.max()) < J3, f"embed: {name} values must index the {J3} joints")
            idx[name] = t.data_ptr()
    if nflip == 2:
        _need(perm is not None and tuple(x2d_flip.shape) == (B, F, J3, 2), "embed: the flipped half needs perm and x2d_flip")
    return B, P, F, J, J3, Cc, nflip, idx


def embed(x3d, x2d, patch_w, patch_b, pos_spatial, temb, norm_w, norm_b, norm_eps=1e-6, joints=None, perm=None,
          x2d_flip=None, do_clamp=False, scale=1.0):
    """Input stage of one body part (pafuse_embed, include/pafuse_hip.h): clamp / scale / flip / part gather of the
    noised 3-D pose, 2-D broadcast over P, Linear(5->C) + pos-embed + time-embed -> x, and LayerNorm(x) -> xn.

    x3d [B,P,F,J3,3], x2d [B,F,J3,2]; ``joints`` = this part's indices into the J3 axis (None: all joints);
    ``x2d_flip`` + ``perm`` switch on the flipped half (rows of the second half).  Returns (x, xn) as
    [nflip, B, P, F, J, C]."""
    lib = _lib.load()
    B, P, F, J, J3, Cc, nflip, idx = _embed_operands(x3d, x2d, patch_w, patch_b, pos_spatial, temb, norm_w, norm_b, joints, perm,
                                                     x2d_flip)
    x = torch.empty(nflip, B, P, F, J, Cc, device=x3d.device, dtype=torch.float32)
    xn = torch.empty_like(x)
    with torch.cuda.device(x3d.device):
        _lib.check(lib.pafuse_embed(_ptr(x3d, "x3d"), _ptr(x2d, "x2d"), _ptr(x2d_flip, "x2d_flip") if nflip == 2 else None,
                                    idx.get("joints"), idx.get("perm"), _ptr(patch_w, "patch_w"), _ptr(patch_b, "patch_b"),
                                    _ptr(pos_spatial, "pos"), _ptr(temb, "temb"), _ptr(norm_w, "norm_w"),
                                    _ptr(norm_b, "norm_b"), float(norm_eps), B, P, F, J, J3, Cc, nflip, int(do_clamp),
                                    float(scale), x.data_ptr(), xn.data_ptr(), _stream(x3d)))
    return x, xn


def embed_unit(x3d, x2d, patch_w, patch_b, pos_spatial, temb, norm_w, norm_b, norm_eps=1e-6, joints=None, perm=None,
               x2d_flip=None, do_clamp=False, scale=1.0, precision="f32", folded=False, h_residual_only=False, window=None,
               out=None):
    """The embed stage in the output form the sampling loop launches for (precision, folded, h_residual_only), over the rows
    ``window`` = (row0, nrows) of the token matrix (None: all M = nflip B P F J rows) - pafuse_embed_unit, which maps the
    three to the kernel's outputs through the loop's own host function.  Operands as :func:`embed`.

    Returns a dict of what the form writes: ``x`` [M,C] (the centred rows in folded 'bf16x3'; absent with h_residual_only),
    ``xn`` [M,C] (unfolded 'f32' / 'bf16' / 'bf16x3'), ``image`` (uint8: the H image in 'f16x2', 4 M C bytes, the X image in
    'bf16x3_images', 6 M C bytes, of the normalised row - folded: of the centred row), ``stats`` [nrows,2] (folded: mean, rstd).
    x, xn and image cover ALL M rows and only the window's rows are written; ``out`` may supply any of the buffers (name ->
    tensor; an ``x`` given with h_residual_only is handed to the library, which must leave it alone)."""
    lib = _lib.load()
    B, P, F, J, J3, Cc, nflip, idx = _embed_operands(x3d, x2d, patch_w, patch_b, pos_spatial, temb, norm_w, norm_b, joints, perm,
                                                     x2d_flip)
    _need(precision in PRECISIONS, f"embed_unit: precision must be one of {sorted(PRECISIONS)}")
    mode = PRECISIONS[precision]
    M = nflip * B * P * F * J
    row0, nrows = (0, M) if window is None else (int(window[0]), int(window[1]))
    _need(0 <= row0 and 1 <= nrows and row0 + nrows <= M, f"embed_unit: window ({row0}, {nrows}) outside the {M} rows")
    images = mode in IMAGE_BYTES
    _need(not folded or mode >= MODE_BF16X3, "embed_unit: the folded LayerNorm exists in 'bf16x3', 'f16x2' and 'bf16x3_images' only")
    _need(not h_residual_only or (images and folded), "embed_unit: h_residual_only is a folded image pipeline's form")
    _need(not images or Cc % (8 if mode == MODE_F16X2 else 32) == 0, f"embed_unit: no {precision} image at C = {Cc}")
    given = dict(out or {})
    _need(set(given) <= {"x", "xn", "image", "stats"}, "embed_unit: out holds x / xn / image / stats")
    dev = x3d.device
    want = {"x": not h_residual_only, "xn": not images and not folded, "image": images, "stats": bool(folded)}
    shapes = {"x": ((M, Cc), torch.float32), "xn": ((M, Cc), torch.float32),
              "image": ((M * Cc * IMAGE_BYTES.get(mode, 0),), torch.uint8), "stats": ((nrows, 2), torch.float32)}
    bufs = {}
    for name, (shape, dtype) in shapes.items():
        t = given.get(name)
        if t is None and want[name]:
            t = torch.empty(shape, device=dev, dtype=dtype)
        if t is not None:
            _need(t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape,
                  f"embed_unit: {name} must be a contiguous {dtype} tensor {shape} on {dev}")
            bufs[name] = t
    a = _lib.EmbedArgs()
    a.x3d, a.x2d, a.x2d_flip = _ptr(x3d, "x3d"), _ptr(x2d, "x2d"), _ptr(x2d_flip, "x2d_flip") if nflip == 2 else None
    a.joints, a.perm = idx.get("joints"), idx.get("perm")
    a.patch_w, a.patch_b, a.pos_spatial, a.temb = _ptr(patch_w, "patch_w"), _ptr(patch_b, "patch_b"), _ptr(pos_spatial, "pos"), _ptr(temb, "temb")
    a.norm_w, a.norm_b, a.norm_eps = _ptr(norm_w, "norm_w"), _ptr(norm_b, "norm_b"), float(norm_eps)
    a.B, a.P, a.F, a.J, a.J3, a.C, a.nflip, a.do_clamp, a.scale = B, P, F, J, J3, Cc, nflip, int(do_clamp), float(scale)
    a.operand_bf16, a.ln_folded, a.h_residual_only = mode, int(bool(folded)), int(bool(h_residual_only))
    for name, t in bufs.items():
        setattr(a, name, t.data_ptr())
    a.row0, a.nrows = row0, nrows
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_embed_unit(C.byref(a), _stream(x3d)))
    return {name: t for name, t in bufs.items() if want[name]}


def ddim_finalize(preds, joint_part, joint_local, img, step_scalars, noise=None, flip_perm=None, scale=1.0, T=1, step=0,
                  out=None):
    """Output stage of one DDIM step (pafuse_ddim_finalize): concat of the parts' predictions, un-flip + TTA mean,
    scale + clamp -> x_start (written to out[:, step]); epsilon in fp64; img update in place.

    preds: list of per-part tensors [nflip,B,P,F,Jp,3]; img [B,P,F,J,3] (updated in place); step_scalars: a
    ``_lib.DDIMStep``.  Returns (out [B,T,P,F,J,3], img)."""
    lib = _lib.load()
    B, P, F, J, _ = img.shape
    flip = flip_perm is not None
    nflip = 2 if flip else 1
    for p in preds:
        _need(tuple(p.shape[:4]) == (nflip, B, P, F) and p.shape[-1] == 3, f"ddim_finalize: prediction {tuple(p.shape)}")
    _need(sum(p.shape[4] for p in preds) == J, "ddim_finalize: the parts must cover every joint")
    for name, t in (("joint_part", joint_part), ("joint_local", joint_local), ("flip_perm", flip_perm)):
        if t is not None:
            _need(t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == J, f"ddim_finalize: {name}")
    _need(int(joint_part.min()) >= 0 and int(joint_part.max()) < len(preds), "ddim_finalize: joint_part range")
    for i, p in enumerate(preds):
        sel = joint_local[joint_part == i]
        _need(sel.numel() == p.shape[4] and int(sel.max()) < p.shape[4] and int(sel.min()) >= 0,
              f"ddim_finalize: joint_local of part {i}")
    if flip:
        _need(int(flip_perm.min()) >= 0 and int(flip_perm.max()) < J, "ddim_finalize: flip_perm range")
    if not step_scalars.last:
        _need(noise is not None and tuple(noise.shape) == tuple(img.shape), "ddim_finalize: an update step needs noise")
    if out is None:
        out = torch.zeros(B, T, P, F, J, 3, device=img.device, dtype=torch.float32)
    _need(tuple(out.shape) == (B, T, P, F, J, 3) and 0 <= step < T, "ddim_finalize: out [B,T,P,F,J,3]")
    n = len(preds)
    ptrs = (C.c_void_p * n)(*[_ptr(p, "pred") for p in preds])
    counts = (C.c_int32 * n)(*[p.shape[4] for p in preds])
    with torch.cuda.device(img.device):
        _lib.check(lib.pafuse_ddim_finalize(ptrs, counts, n, joint_part.data_ptr(), joint_local.data_ptr(),
                                            flip_perm.data_ptr() if flip else None, _ptr(img, "img"),
                                            _ptr(noise, "noise") if noise is not None else None, _ptr(out, "out"),
                                            B, P, F, J, T, step, int(flip), float(scale), C.byref(step_scalars),
                                            _stream(img)))
    return out, img


def hsplit_rows(x):
    """The activation H image of a contiguous fp32 [R,K] tensor (pafuse_hsplit_rows): per sub-block of 8 k the fp16 slices
    hi = f16(a) and lo = f16((a - hi) 2^11), 4 R K bytes.  In the loop every producer writes this form itself; the unit tests
    and pafuse_block_forward's first LayerNorm use this pass."""
    lib = _lib.load()
    _need(x.dim() == 2 and x.shape[1] % 8 == 0, "hsplit_rows: x must be [R, K] with K % 8 == 0")
    R, K = x.shape
    out = torch.empty(R * K * 4, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_hsplit_rows(_ptr(x, "x"), R, K, out.data_ptr(), _stream(x)))
    return out


def xsplit_rows(x):
    """The X image of a contiguous fp32 [R,K] tensor (pafuse_xsplit_rows): [R][K/32][3][32 x bf16], the three exact bf16 slices
    of every element, 6 R K bytes."""
    lib = _lib.load()
    _need(x.dim() == 2 and x.shape[1] % 32 == 0, "xsplit_rows: x must be [R, K] with K % 32 == 0")
    R, K = x.shape
    out = torch.empty(R * K * 6, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_xsplit_rows(_ptr(x, "x"), R, K, out.data_ptr(), _stream(x)))
    return out


def xjoin_rows(image, R, K):
    """fp32 [R,K] tensor an X image stands for: s0 + (s1 + s2), exact in fp32."""
    v = image.view(torch.bfloat16).view(R, K // 32, 3, 32).float()
    return (v[:, :, 0] + (v[:, :, 1] + v[:, :, 2])).reshape(R, K)


def hjoin_rows(image, R, K):
    """fp32 [R,K] tensor an activation H image stands for: hi + 2^-11 lo (exact in fp32)."""
    v = image.view(torch.float16).view(R, K // 8, 2, 8).float()
    return (v[:, :, 0] + v[:, :, 1] * 2.0 ** -11).reshape(R, K)


def qkv_attention_fused(x, qkv_weight, qkv_bias, heads, nseq, L, scheme="bf16x3_images", rstd=None, group=1, group_stride=None,
                        seq_stride=0, tok_stride=1):
    """The fused qkv + attention kernel on its own (pafuse_qkv_attention_image): x [M,C] fp32 (with `rstd` [M]: the centred rows of
    a folded LayerNorm) -> o [M,C] fp32 decoded from the image the kernel writes; q | k | v = rstd (x W^T) + b per head, then
    softmax(q k^T d^-1/2) v per (sequence, head).  scheme 'f16x2' (hfqa_kernel, H images) or 'bf16x3_images' (xfqa_kernel, X
    images).  Sequence map as `attention`."""
    lib = _lib.load()
    M, Cw = x.shape
    _need(scheme in ("f16x2", "bf16x3_images"), "qkv_attention_fused: scheme 'f16x2' or 'bf16x3_images'")
    _need(tuple(qkv_weight.shape) == (3 * Cw, Cw) and qkv_bias.numel() == 3 * Cw and Cw % heads == 0, "qkv_attention_fused: qkv must be [3C, C] + [3C]")
    gs = L if group_stride is None else group_stride
    if nseq:   # the last row any sequence touches must exist
        last = ((nseq - 1) // group) * gs + ((nseq - 1) % group) * seq_stride + (L - 1) * tok_stride
        _need(0 <= last < M and min(gs, seq_stride, tok_stride) >= 0, f"qkv_attention_fused: sequences reach row {last} of {M}")
    mode = PRECISIONS[scheme]
    f16 = mode == MODE_F16X2
    table = {"attn.qkv.weight": qkv_weight.contiguous(), "attn.qkv.bias": qkv_bias.contiguous()}
    hs, hb = head_major_qkv(table.__getitem__, "attn.qkv.weight", heads, False, mode)
    xi = hsplit_rows(x.contiguous()) if f16 else xsplit_rows(x.contiguous())
    stats = None
    if rstd is not None:
        stats = torch.stack([torch.zeros_like(rstd), rstd], dim=1).contiguous()
    oi = torch.zeros(M * Cw * IMAGE_BYTES[mode], dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_qkv_attention_image(SPLIT_FLAG[mode], xi.data_ptr(), stats.data_ptr() if stats is not None else None,
                                                  hs.data_ptr(), _ptr(hb, "qkv_hb"), oi.data_ptr(), M, nseq, L, Cw, heads, group, gs,
                                                  seq_stride, tok_stride, 0.0, _stream(x)))
    return hjoin_rows(oi, M, Cw) if f16 else xjoin_rows(oi, M, Cw)


def mlp_fused(xc, rstd, fc1_weight, fc1_bias, fc2_weight, fc2_bias, eps=1e-6, in_place=False):
    """The fused MLP kernel on its own (pafuse_mlp_h): xc [M,C] = rows of the residual stream centred on their means, rstd [M] or
    None -> (y - mean(y) as fp32 [M,C] decoded from the H image the kernel writes, stats [M,2] = (mean(y), rstd(y))) with
    y = xc + GELU(rstd (xc W1^T) + b1) W2^T + b2."""
    lib = _lib.load()
    M, Cw = xc.shape
    _need(tuple(fc1_weight.shape) == (2 * Cw, Cw) and tuple(fc2_weight.shape) == (Cw, 2 * Cw), "mlp_fused: weights must be [2C,C] and [C,2C]")
    xh = hsplit_rows(xc.contiguous())
    stats_in = None
    if rstd is not None:
        stats_in = torch.stack([torch.zeros_like(rstd), rstd], dim=1).contiguous()
    w1h = split_image(fc1_weight.contiguous(), 0, MODE_F16X2)
    w2hp = fused_mlp_fc2_image(fc2_weight)
    out = xh if in_place else torch.empty(M * Cw * 4, dtype=torch.uint8, device=xc.device)
    stats = stats_in if in_place and stats_in is not None else torch.empty(M, 2, device=xc.device, dtype=torch.float32)
    with torch.cuda.device(xc.device):
        _lib.check(lib.pafuse_mlp_h(xh.data_ptr(), stats_in.data_ptr() if stats_in is not None else None, w1h.data_ptr(),
                                    _ptr(fc1_bias, "fc1_bias"), w2hp.data_ptr(), _ptr(fc2_bias, "fc2_bias"), out.data_ptr(),
                                    stats.data_ptr(), M, Cw, float(eps), _stream(xc)))
    return hjoin_rows(out, M, Cw), stats


SCHEMES = {name: mode for name, mode in PRECISIONS.items() if mode in SPLIT_FLAG}      # the split modes by name


def split_weights(weight, layout=0, scheme="bf16x3"):
    """Pre-split image of a [N,K] fp32 weight for the split-precision products (pafuse_split_weights);
    scheme 'bf16x3_images' (the X image of the image pipeline: three bf16 slices, one geometry for every layer), 'f16x2' (the H image:
    two fp16 slices of the power-of-two-scaled weight) or 'bf16x3' (the round-3 kernels' images; layout 0: the
    32x32x16-MFMA plain kernel (linear_split's layout 0; no layer of the model since ABI 6), 1: the whole-row layers attn.proj
    and mlp.fc2 (linear_rowln), 2: the 16x16x32-MFMA kernels of attn.qkv and mlp.fc1)."""
    _need(weight.dim() == 2 and weight.shape[1] % 32 == 0, "split_weights: weight must be [N, K] with K % 32 == 0")
    _need(layout in (0, 1, 2), "split_weights: layout 0 (plain 32x32x16 kernel), 1 (whole-row layers) or 2 (qkv / fc1 kernels)")
    _need(scheme in SCHEMES, f"split_weights: scheme must be one of {sorted(SCHEMES)}")
    return split_image(weight, layout, SCHEMES[scheme])


def linear_split(x, weight, bias, act=None, image=None, layout=0, scheme="bf16x3", out_image=False):
    """nn.Linear (+ exact GELU) with split-precision products, fp32 accumulation: scheme 'bf16x3_images' / 'bf16x3' - fp32 operands
    as three bf16 slices each, six bf16 MFMA products per pair (on the image pipeline: both operands as X images; on the
    round-3 kernels: A split in registers); 'f16x2' - two fp16 slices of the activation, three of the scaled weight, three
    fp16 MFMA products.  ``image`` = split_weights(weight, layout, scheme) to reuse a cached image; ``layout`` picks the
    round-3 kernel: 0 the 32x32x16-MFMA tiles (no model layer since ABI 6), 2 the 16x16x32-MFMA tiles (attn.qkv and mlp.fc1:
    the persistent strip kernel).  (Layout 1 images belong to the whole-row layers: linear_rowln.)  ``out_image`` (image schemes):
    return the image of the output (what a producer hands its consumer) instead of fp32 rows."""
    lib = _lib.load()
    K = x.shape[-1]
    N = weight.shape[0]
    _need(tuple(weight.shape) == (N, K) and bias.numel() == N, f"linear: x [..,{K}] needs weight [N,{K}] and bias [N]")
    _need(layout in (0, 2), "linear_split: layout 0 or 2 (layout-1 images are the whole-row layers': linear_rowln)")
    img = split_weights(weight, layout, scheme) if image is None else image
    _need(img.numel() == lib.pafuse_split_image_bytes(N, K, layout | SPLIT_FLAG[SCHEMES[scheme]]), "linear_split: image size does not match the weight")
    x2 = x.contiguous().view(-1, K)
    out = torch.empty(x2.shape[0], N, device=x.device, dtype=torch.float32)
    if scheme == "f16x2":      # both operands as H images (pafuse_linear_h)
        _need(N % 128 == 0 or N % 224 == 0, "linear_split: f16x2 serves N that is a multiple of 128 or 224")
        ah = hsplit_rows(x2)
        oh = torch.empty(x2.shape[0] * N * 4, dtype=torch.uint8, device=x.device) if out_image else None
        with torch.cuda.device(x.device):
            _lib.check(lib.pafuse_linear_h(ah.data_ptr(), img.data_ptr(), _ptr(bias, "bias"), None if out_image else out.data_ptr(),
                                           oh.data_ptr() if out_image else None, x2.shape[0], N, K,
                                           1 if act == "gelu" else 0, _stream(x)))
        return oh if out_image else out.view(*x.shape[:-1], N)
    if scheme == "bf16x3_images":     # both operands as X images (pafuse_linear_x)
        _need(N % 128 == 0 or N % 224 == 0 or N % 96 == 0, "linear_split: the image pipeline serves N that is a multiple of 128, 224 or 96")
        ax = xsplit_rows(x2)
        ox = torch.empty(x2.shape[0] * N * 6, dtype=torch.uint8, device=x.device) if out_image else None
        with torch.cuda.device(x.device):
            _lib.check(lib.pafuse_linear_x(ax.data_ptr(), img.data_ptr(), _ptr(bias, "bias"), None if out_image else out.data_ptr(),
                                           ox.data_ptr() if out_image else None, x2.shape[0], N, K,
                                           1 if act == "gelu" else 0, _stream(x)))
        return ox if out_image else out.view(*x.shape[:-1], N)
    _need(not out_image, "linear_split: the round-3 kernels write fp32 rows")
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_linear_split(_ptr(x2, "x"), img.data_ptr(), _ptr(bias, "bias"), out.data_ptr(),
                                           x2.shape[0], N, K,
                                           (1 if act == "gelu" else 0) + (2 if layout == 2 else 0), _stream(x)))
    return out.view(*x.shape[:-1], N)


def rowln_args(x, weight, bias, resid, precision="bf16x3", image=None, post=None, pos=None, next=None, head=None, fold=False,
               in_place=False, resid_image=False, training=False, rowscale=None, rs_map=(0, 1, 1), out=None):
    """One whole-row layer as a pafuse_rowln_args (include/pafuse_hip.h), with the images its mode reads made here.
    Returns (args, keep, finish): ``keep`` holds every tensor the struct points at, ``finish()`` the outputs as a dict.

    x [M,K], weight [N,K], bias [N], resid [M,N] fp32.  post / next: (weight, bias, eps) of a LayerNorm; pos: (table [F',N],
    posJ, posF); head: (weight [3,N], bias [3]) behind `next`; fold: (mean, rstd) of the next LayerNorm to 'stats' and x stored
    centred on that mean instead of the normalised row.  precision: a key of PRECISIONS; 'bf16x3' uses the layout-1 image of
    weight, 'f16x2' / 'bf16x3_images' the H / X images of x and weight (``image``: a cached weight image).  resid_image (image modes): the
    residual goes in as its image and x comes out only as an image ('x' is decoded from it).  in_place: x is written over the
    residual itself (resid, or its image).  training (modes 0 / 2): rowscale [nseq] or None, rs_map = (rs_temporal, rs_J,
    rs_FJ); 'pre' = the pre-norm sum.  out: preallocated outputs by name ('x', 'n', 'head', 'stats', 'pre', 'x_img', 'n_img'),
    at least as large as the layer needs (nothing past row M is written).
    Outputs: 'x', 'n', 'head', 'stats', 'pre' fp32 (those the options produce); in the image modes also 'x_img' / 'n_img', the
    images joined back to fp32."""
    lib = _lib.load()
    _need(precision in PRECISIONS, f"precision must be one of {sorted(PRECISIONS)}")
    mode = PRECISIONS[precision]
    M, K = x.shape
    N = weight.shape[0]
    _need(tuple(weight.shape) == (N, K) and bias.numel() == N and tuple(resid.shape) == (M, N),
          f"linear_rowln: x [M,K], weight [N,{K}], bias [N], resid [{M},{N}]")
    _need(not resid_image or mode >= MODE_F16X2, "linear_rowln: resid_image needs an image mode (f16x2, bf16x3_images)")
    out = dict(out or {})
    a = _lib.RowLNArgs()
    a.M, a.N, a.K, a.operand_bf16, a.training = M, N, K, mode, int(bool(training))
    keep = [x, weight, bias, resid]
    eb = IMAGE_BYTES.get(mode, 4)

    def buf(name, shape, dtype=torch.float32):
        t = out.get(name)
        if t is None:
            t = out[name] = torch.empty(shape, dtype=dtype, device=x.device)
        _need(t.is_contiguous() and t.numel() >= (shape if isinstance(shape, int) else shape[0] * shape[1]),
              f"linear_rowln: output '{name}' is too small")
        keep.append(t)
        return t.data_ptr()

    split = (hsplit_rows if mode == MODE_F16X2 else xsplit_rows) if mode >= MODE_F16X2 else None
    if mode >= MODE_F16X2:
        ximg = split(x)
        wimg = image if image is not None else split_image(weight, 1, mode)
        keep += [ximg, wimg]
        a.A_img, a.Wsplit = ximg.data_ptr(), wimg.data_ptr()
    else:
        a.A = _ptr(x, "x")
        a.W = _ptr(weight, "weight")
        if mode == MODE_BF16X3:
            wimg = image if image is not None else split_image(weight, 1)
            keep.append(wimg)
            a.Wsplit = wimg.data_ptr()
    a.bias = _ptr(bias, "bias")
    rimg = None
    if resid_image:
        rimg = split(resid)
        keep.append(rimg)
        a.resid_img = rimg.data_ptr()
        if in_place:
            out["x_img"] = rimg
        a.out_x_img = buf("x_img", M * N * eb, torch.uint8)
    else:
        a.resid = _ptr(resid, "resid")
        if in_place:
            out["x"] = resid
        a.out_x = buf("x", (M, N))
        if mode >= MODE_F16X2:
            a.out_x_img = buf("x_img", M * N * eb, torch.uint8)
    if post is not None:
        a.post_w, a.post_b, a.post_eps = _ptr(post[0], "post_w"), _ptr(post[1], "post_b"), float(post[2])
    if pos is not None:
        a.pos, a.posJ, a.posF = _ptr(pos[0], "pos"), int(pos[1]), int(pos[2])
    if next is not None:
        a.next_w, a.next_b, a.next_eps = _ptr(next[0], "next_w"), _ptr(next[1], "next_b"), float(next[2])
        if fold:
            a.ln_stats = buf("stats", (M, 2))
        else:
            a.out_n = buf("n", (M, N))
            if mode >= MODE_F16X2:
                a.out_n_img = buf("n_img", M * N * eb, torch.uint8)
    if head is not None:
        a.head_w, a.head_b = _ptr(head[0], "head_w"), _ptr(head[1], "head_b")
        a.out_head = buf("head", (M, 3))
    if training:
        if rowscale is not None:
            a.rowscale = _ptr(rowscale, "rowscale")
        a.rs_temporal, a.rs_J, a.rs_FJ = (int(v) for v in rs_map)
        a.out_pre = buf("pre", (M, N))
    keep += [post, pos, next, head, rowscale]

    def finish():
        join = hjoin_rows if mode == MODE_F16X2 else xjoin_rows
        res = {}
        for name in ("x", "n", "pre"):
            if name in out and out[name] is not None and (name != "x" or not resid_image):
                res[name] = out[name].reshape(-1)[:M * N].view(M, N)
        for name, cols in (("head", 3), ("stats", 2)):
            if name in out:
                res[name] = out[name].reshape(-1)[:M * cols].view(M, cols)
        for name in ("x_img", "n_img"):
            if name in out:
                res[name] = join(out[name].reshape(-1)[:M * N * eb], M, N)
        if resid_image:
            res["x"] = res["x_img"]
        return res

    return a, keep, finish


def linear_rowln(x, weight, bias, resid, precision="bf16x3", **options):
    """One whole-row layer - attn.proj / mlp.fc2 with the residual add and the LayerNorm chain in the epilogue
    (pafuse_linear_rowln, the kernels the denoisers launch): y = x W^T + b + resid, then post-norm, pos, next-norm / its folded
    statistics / the head.  Options and the returned dict of outputs: rowln_args."""
    lib = _lib.load()
    a, keep, finish = rowln_args(x, weight, bias, resid, precision, **options)
    with torch.cuda.device(x.device):
        _lib.check(lib.pafuse_linear_rowln(C.byref(a), _stream(x)))
    del keep      # (stream-ordered: the caching allocator reuses the blocks only for later work on this stream)
    return finish()


def linear_rowln_group(layers, shared_grid=True):
    """Up to four independent whole-row layers in one call (pafuse_linear_rowln_group): ``layers`` is a list of dicts of
    linear_rowln's arguments (x, weight, bias, resid, precision, options); shared_grid=True runs them in ONE grid where the
    grouped kernel has variants for all of them (the single-stream schedule of the denoiser loop), else one launch each.
    Returns the list of output dicts."""
    lib = _lib.load()
    _need(1 <= len(layers) <= _lib.MAX_PARTS, f"linear_rowln_group: 1 .. {_lib.MAX_PARTS} layers")
    built = [rowln_args(**layer) for layer in layers]
    arr = (_lib.RowLNArgs * len(built))(*[b[0] for b in built])
    dev = layers[0]["x"].device
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_linear_rowln_group(arr, len(built), int(bool(shared_grid)), _stream(layers[0]["x"])))
    return [b[2]() for b in built]


def procrustes_errors(pred, gt, x2d, traj, cam, conn, pick=True):
    """Protocol #2 per-joint / per-pose errors (pafuse_procrustes_errors): pred [B,T,P,F,J,3] and gt [B,F,J,3]
    part-centred, x2d [B,F,J,2], traj [B,F,3] (or [B,F,1,3]), cam [9], conn int32 [J] (connection joint of every
    joint) -> dict jbest, pagg, jagg [B,T,F,J] fp32, pbest_sums [B,T,P,F] fp64 and (pick=True) the J-Agg pick [B,T,F,J]
    int32.  fp32 operands on one HIP device, contiguous."""
    lib = _lib.load()
    _need(pred.dim() == 6 and pred.shape[-1] == 3, f"procrustes_errors: pred must be [B,T,P,F,J,3], got {tuple(pred.shape)}")
    B, T, P, F, J, _ = pred.shape
    _need(tuple(gt.shape) == (B, F, J, 3) and tuple(x2d.shape) == (B, F, J, 2) and traj.numel() == B * F * 3
          and cam.numel() == 9 and conn.numel() == J, "procrustes_errors: operands do not match pred")
    _need_tensors("procrustes_errors", (pred, gt, x2d, traj, cam), (conn,))
    dev = pred.device
    out = {k: torch.empty(B, T, F, J, device=dev) for k in ("jbest", "pagg", "jagg")}
    out["pbest_sums"] = torch.empty(B, T, P, F, device=dev, dtype=torch.float64)
    if pick:
        out["pick"] = torch.empty(B, T, F, J, device=dev, dtype=torch.int32)
    _lib.check(lib.pafuse_procrustes_errors(
        pred.data_ptr(), gt.data_ptr(), x2d.data_ptr(), traj.data_ptr(), cam.data_ptr(), conn.data_ptr(), B, T, P, F, J,
        out["jbest"].data_ptr(), out["pbest_sums"].data_ptr(), out["pagg"].data_ptr(), out["jagg"].data_ptr(),
        out["pick"].data_ptr() if pick else None, _stream(pred)))
    return out


# ------------------------------------------------------------------------------------------------ noise stream v1
def noise_key(seed, call, b0=0, p0=0, device="cuda"):
    """The 16-byte device buffer {seed, call, b0, p0} the seeded kernels read (four uint32 behind an int32 tensor: torch
    has no arithmetic on uint32 and none is needed).  seed and call in [0, 2^32); b0 / p0: global index of the first
    clip / first hypothesis of the call."""
    import numpy as np
    for name, v in (("seed", seed), ("call", call), ("b0", b0), ("p0", p0)):
        _need(0 <= int(v) < 2 ** 32, f"noise_key: {name} = {v} is not in [0, 2^32)")
    words = np.array([int(seed), int(call), int(b0), int(p0)], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(words).to(device)


def noise_fill(key, draw, B, P, F, J, out=None):
    """Draw `draw` of noise stream v1 (pafuse_noise_fill; DESIGN.md section 6, host statement pafuse_amd.noise.reference_draw)
    for clips [b0, b0 + B) and hypotheses [p0, p0 + P): key = noise_key(seed, call, b0, p0) -> float32 [B,P,F,J,3] on the
    key's device."""
    lib = _lib.load()
    _need(torch.is_tensor(key) and key.is_cuda and key.dtype == torch.int32 and key.numel() == 4 and key.is_contiguous(),
          "noise_fill: key must be the int32[4] device tensor of noise_key (no CPU fallback)")
    draw, B, P, F, J = (int(v) for v in (draw, B, P, F, J))
    _need(draw >= 0 and min(B, P, F, J) > 0 and F * J < 2 ** 32 and B * P * F * J < 2 ** 31 * 256,
          f"noise_fill: bad size (draw={draw} B={B} P={P} F={F} J={J})")
    if out is None:
        out = torch.empty(B, P, F, J, 3, device=key.device, dtype=torch.float32)
    _need(out.is_cuda and out.device == key.device and out.dtype == torch.float32 and out.is_contiguous()
          and tuple(out.shape) == (B, P, F, J, 3), "noise_fill: out must be a contiguous float32 [B,P,F,J,3] on the key's device")
    with torch.cuda.device(key.device):
        _lib.check(lib.pafuse_noise_fill(key.data_ptr(), draw, B, P, F, J, out.data_ptr(), _stream(key)))
    return out


# --------------------------------------------------------------------- training draws of noise stream v1
def train_key(seed, call, first=0, stride=1, device="cuda", clips=None):
    """The 16-byte device buffer {seed, call, first, stride} the training-draw kernels read: noise_key's layout with the last
    two words saying where the call's clips sit in the GLOBAL batch - local clip i is global clip first + i * stride.  The
    library reads the words on the device and cannot check them, so the checks live here: stride >= 1 and, with `clips`
    (the number of clips of the call), first + (clips - 1) * stride < 2^32.  On a HIP device the words travel through pinned
    memory without a synchronisation (the training step makes one key per forward)."""
    import numpy as np
    for name, v in (("seed", seed), ("call", call), ("first", first), ("stride", stride)):
        _need(not isinstance(v, bool) and int(v) == v and 0 <= int(v) < 2 ** 32, f"train_key: {name} = {v!r} is not an integer in [0, 2^32)")
    _need(int(stride) >= 1, "train_key: stride = 0 would give every clip of the call the same draws")
    if clips is not None:
        _need(int(clips) >= 1 and int(first) + (int(clips) - 1) * int(stride) < 2 ** 32,
              f"train_key: clips {first} + i * {stride}, i < {clips}, leave the 32 bits of the global clip index")
    words = torch.from_numpy(np.array([int(seed), int(call), int(first), int(stride)], dtype=np.uint32).view(np.int32))
    if torch.device(device).type == "cuda":
        return words.pin_memory().to(device, non_blocking=True)
    return words.to(device)


def _need_key(who, key):
    _need(torch.is_tensor(key) and key.is_cuda and key.dtype == torch.int32 and key.numel() == 4 and key.is_contiguous(),
          f"{who}: key must be the int32[4] device tensor of train_key (no CPU fallback)")


def qsample_seeded(x0, key4, sqrt_ac, sqrt_1mac, scale, num_timesteps, want_noise=False):
    """pafuse_d3dp_qsample_seeded: draw (t, noise) for the clips of x0 [B,F,J,3] from the stream (key4 = train_key(...)) and
    apply q_sample + clamp + / scale in the fp64 of the schedule tables -> (x_t float32 [B,F,J,3], t int64 [B], noise
    float32 [B,F,J,3] or None).  Without want_noise the normals are never stored."""
    lib = _lib.load()
    _need_key("qsample_seeded", key4)
    _need(x0.dim() == 4 and x0.shape[-1] == 3 and x0.shape[0] > 0 and x0.is_cuda and x0.device == key4.device and x0.dtype == torch.float32
          and x0.is_contiguous(), f"qsample_seeded: x0 must be a contiguous float32 [B,F,J,3] on the key's device, got {tuple(x0.shape)}")
    B, F, J, _ = x0.shape
    num_timesteps = int(num_timesteps)
    _need(0 < num_timesteps < 2 ** 31 and F * J < 2 ** 32, f"qsample_seeded: bad size (num_timesteps={num_timesteps} F={F} J={J})")
    for name, tab in (("sqrt_ac", sqrt_ac), ("sqrt_1mac", sqrt_1mac)):
        _need(tab.is_cuda and tab.device == x0.device and tab.dtype == torch.float64 and tab.is_contiguous() and tab.numel() >= num_timesteps,
              f"qsample_seeded: {name} must hold num_timesteps float64 on the device of x0")
    out = torch.empty_like(x0)
    t = torch.empty(B, device=x0.device, dtype=torch.int64)
    noise = torch.empty_like(x0) if want_noise else None
    with torch.cuda.device(x0.device):
        _lib.check(lib.pafuse_d3dp_qsample_seeded(x0.data_ptr(), key4.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), float(scale),
                                                  num_timesteps, out.data_ptr(), t.data_ptr(), noise.data_ptr() if want_noise else None,
                                                  B, F, J, _stream(x0)))
    return out, t, noise


def droppath_fill(key4, denoiser, depth, F, J, B, keep, factor):
    """pafuse_train_droppath_fill: one denoiser's DropPath table of one training forward, float32 [2*depth, 2, B*max(F,J)]
    (the drop_path operand of pafuse_mixste2_train_forward), from the stream.  keep: float64 [2*depth], factor: float32
    [2*depth], both on the key's device (MixSTE2.drop_path_tables makes them)."""
    lib = _lib.load()
    _need_key("droppath_fill", key4)
    denoiser, depth, F, J, B = (int(v) for v in (denoiser, depth, F, J, B))
    _need(0 <= denoiser < 2 ** 16 and 0 < depth <= 2 ** 14 and min(F, J, B) > 0 and F * J < 2 ** 32,
          f"droppath_fill: bad argument (denoiser={denoiser} depth={depth} F={F} J={J} B={B})")
    for name, tab, dtype in (("keep", keep, torch.float64), ("factor", factor, torch.float32)):
        _need(torch.is_tensor(tab) and tab.is_cuda and tab.device == key4.device and tab.dtype == dtype and tab.is_contiguous()
              and tab.numel() == 2 * depth, f"droppath_fill: {name} must hold 2 * depth {dtype} on the key's device")
    out = torch.empty(2 * depth, 2, B * max(F, J), device=key4.device, dtype=torch.float32)
    with torch.cuda.device(key4.device):
        _lib.check(lib.pafuse_train_droppath_fill(key4.data_ptr(), denoiser, depth, F, J, B, keep.data_ptr(), factor.data_ptr(),
                                                  out.data_ptr(), out.numel(), _stream(key4)))
    return out


# ------------------------------------------------------------------------------------ sharded hypothesis evaluation
PARTIALS_HEAD_BYTES_PER_ELEMENT = 40   # double sum[3] + float jbest, e2, sel3 + int32 idx per (b, t, f, j)


def partials_bytes(B, T, P_r, F, J, num_parts):
    """Bytes of the state pafuse_hypothesis_partials writes for a shard of P_r hypotheses (the formula of
    pafuse_hypothesis_partials_bytes, restated so that sizes can be planned without the library): the head, independent
    of P_r, then 8 * (1 + num_parts) bytes per local hypothesis and step."""
    return PARTIALS_HEAD_BYTES_PER_ELEMENT * B * T * F * J + 8 * P_r * T * (1 + num_parts)


def partials_views(state, B, T, P_r, F, J, num_parts):
    """Typed views of a flat state (1-D float64 tensor of partials_bytes / 8 elements, or longer: a padded one):
    sum [B,T,F,J,3] f64, jbest / e2 / sel3 [B,T,F,J] f32, idx [B,T,F,J] i32, hsum [P_r,T,1+num_parts] f64."""
    n = B * T * F * J
    _need(state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous()
          and state.numel() * 8 >= partials_bytes(B, T, P_r, F, J, num_parts), "partials_views: not a state of these sizes")
    f32 = state[3 * n:5 * n].view(torch.float32)
    return {"sum": state[:3 * n].view(B, T, F, J, 3), "jbest": f32[:n].view(B, T, F, J), "e2": f32[n:2 * n].view(B, T, F, J),
            "sel3": f32[2 * n:3 * n].view(B, T, F, J), "idx": f32[3 * n:].view(torch.int32).view(B, T, F, J),
            "hsum": state[5 * n:5 * n + P_r * T * (1 + num_parts)].view(P_r, T, 1 + num_parts)}


def hypothesis_partials(pred, gt, x2d, traj, cam, conn, pbroot, part, num_parts, h0, out=None):
    """One shard's partial reductions (pafuse_hypothesis_partials): pred [B,T,P_r,F,J,3] the LOCAL hypotheses
    [h0, h0 + P_r) of the run, gt [B,F,J,3], x2d [B,F,J,2], traj [B,F,3] (or [B,F,1,3]), cam [9], conn / pbroot / part
    int32 [J] (connection joint, part root, part number of every joint) -> the flat state, a 1-D float64 tensor
    (partials_views names its pieces).  `out`: a float64 buffer at least that long to write into (a padded state for
    the collective); the result is then `out` itself.  fp32 operands on one HIP device, contiguous."""
    lib = _lib.load()
    B, T, P_r, F, J = _need_pred("hypothesis_partials", pred)
    _need(tuple(gt.shape) == (B, F, J, 3) and tuple(x2d.shape) == (B, F, J, 2) and traj.numel() == B * F * 3
          and cam.numel() == 9 and conn.numel() == J and pbroot.numel() == J and part.numel() == J,
          "hypothesis_partials: operands do not match pred")
    _need(T > 0 and F > 0 and J > 0 and int(h0) >= 0, "hypothesis_partials: T, F, J > 0 and h0 >= 0")
    _need(1 <= num_parts <= _lib.MAX_PARTS, f"hypothesis_partials: 1 .. {_lib.MAX_PARTS} parts")
    _need_tensors("hypothesis_partials", (pred, gt, x2d, traj, cam), (conn, pbroot, part))
    dev = pred.device
    need = int(lib.pafuse_hypothesis_partials_bytes(B, T, P_r, F, J, num_parts))
    assert need == partials_bytes(B, T, P_r, F, J, num_parts)
    out = _state_out("hypothesis_partials", out, need, dev)
    wbytes = int(lib.pafuse_hypothesis_partials_workspace_bytes(B, T, P_r, F, J, num_parts))
    work = _lib.workspace(wbytes, dev, "hypothesis_partials", torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_hypothesis_partials(
            _data(pred), _data(gt), _data(x2d), _data(traj), _data(cam), _data(conn), _data(pbroot), _data(part), num_parts,
            B, T, P_r, F, J, int(h0), _data(out), out.numel() * 8, work.data_ptr(), work.numel() * 8, _stream(pred)))
    return out


def combine_partials(states, gt, conn, pbroot, shape, num_proposals, merged=None, maps=True):
    """pafuse_hypothesis_combine: `states` [W, L] float64 (W flat states of the same (B,T,F,J) = `shape`, one per row, in
    ascending-h0 order; L * 8 >= the head bytes - rows may carry their per-hypothesis tail and padding, which is not
    read).  maps=True -> dict jbest, pagg, jagg, paggpb [B,T,F,J] (what pafuse_hypothesis_errors gives; the P-Agg mean
    divides by `num_proposals`, the TOTAL hypothesis count).  `merged`: a float64 buffer that receives the head of the
    union's state (5*B*T*F*J elements); it may be states[0] itself when maps=False (a running state)."""
    lib = _lib.load()
    B, T, F, J = (int(v) for v in shape)
    n = B * T * F * J
    _need_rows(states, 5 * n, "combine_partials: states must be [W, >= 5*B*T*F*J] float64")
    _need(T > 0 and F > 0 and J > 0 and B >= 0, "combine_partials: bad shape")
    _need(maps or merged is not None, "combine_partials: nothing to compute")
    _need(not maps or int(num_proposals) >= 1, "combine_partials: num_proposals >= 1")
    dev = states.device
    ops = (gt, conn, pbroot)
    _need(tuple(gt.shape) == (B, F, J, 3) and conn.numel() == J and pbroot.numel() == J
          and all(t.is_cuda and t.device == dev and t.is_contiguous() for t in ops) and gt.dtype == torch.float32
          and conn.dtype == torch.int32 and pbroot.dtype == torch.int32, "combine_partials: gt [B,F,J,3] f32, conn / pbroot "
          "[J] int32, contiguous on the device of the states")
    if merged is not None:
        _need_merged("combine_partials", merged, states, 5 * n, "5*B*T*F*J", states.numel(), "none" if maps else None)
    out = {k: torch.empty(B, T, F, J, device=dev) for k in ("jbest", "pagg", "jagg", "paggpb")} if maps else {}
    if n == 0:
        return out
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_hypothesis_combine(
            states.data_ptr(), states.shape[0], states.shape[1] * 8, gt.data_ptr(), conn.data_ptr(), pbroot.data_ptr(),
            B, T, F, J, int(num_proposals), None if merged is None else merged.data_ptr(),
            *((out[k].data_ptr() for k in ("jbest", "pagg", "jagg", "paggpb")) if maps else (None,) * 4), _stream(states)))
    return out


# --------------------------------------------------------------------------------------- aggregates as poses
POSE_STATE_BYTES_PER_ELEMENT = 44   # double sum[3] + float e2 + int32 idx + float sel[3] per (b, t, f, j)


def pose_partials_bytes(B, T, F, J):
    """Bytes of the state pafuse_pose_partials writes (the formula of pafuse_pose_partials_bytes, restated so that sizes
    can be planned without the library): 44 bytes per (b,t,f,j), rounded up to a multiple of 8.  No P in it."""
    return (POSE_STATE_BYTES_PER_ELEMENT * B * T * F * J + 7) // 8 * 8


def pose_views(state, B, T, F, J):
    """Typed views of a flat pose state (1-D float64 tensor of pose_partials_bytes / 8 elements, or longer):
    sum [B,T,F,J,3] f64, e2 [B,T,F,J] f32, idx [B,T,F,J] i32, sel [B,T,F,J,3] f32."""
    n = B * T * F * J
    _need(state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous()
          and state.numel() * 8 >= pose_partials_bytes(B, T, F, J), "pose_views: not a state of these sizes")
    f32 = state[3 * n:].view(torch.float32)
    return {"sum": state[:3 * n].view(B, T, F, J, 3), "e2": f32[:n].view(B, T, F, J),
            "idx": f32[n:2 * n].view(torch.int32).view(B, T, F, J), "sel": f32[2 * n:5 * n].view(B, T, F, J, 3)}


def pose_partials(pred, conn, h0, x2d=None, traj=None, cam=None, out=None):
    """One shard's pose state (pafuse_pose_partials): pred [B,T,P_r,F,J,3] the LOCAL part-centred hypotheses
    [h0, h0 + P_r) of the run, conn int32 [J]; x2d [B,F,J,2], traj [B,F,3] (or [B,F,1,3]) and cam [9] together, or none of
    them (mean-only: no candidate is kept) -> the flat state, a 1-D float64 tensor (pose_views names its pieces).
    `out`: a float64 buffer at least that long to write into; the result is then `out` itself."""
    lib = _lib.load()
    B, T, P_r, F, J = _need_pred("pose_partials", pred)
    _need(T > 0 and F > 0 and J > 0 and int(h0) >= 0, "pose_partials: T, F, J > 0 and h0 >= 0")
    _need(conn.numel() == J and conn.dtype == torch.int32, "pose_partials: conn must be int32 [J]")
    given = [t for t in (x2d, traj, cam) if t is not None]   # some but not all of them: the library refuses (PafuseError)
    _need((x2d is None or tuple(x2d.shape) == (B, F, J, 2)) and (traj is None or traj.numel() == B * F * 3)
          and (cam is None or cam.numel() == 9), "pose_partials: operands do not match pred")
    _need_tensors("pose_partials", [pred] + given, (conn,))
    dev = pred.device
    need = int(lib.pafuse_pose_partials_bytes(B, T, F, J))
    assert need == pose_partials_bytes(B, T, F, J)
    out = _state_out("pose_partials", out, need, dev)
    ptrs = [None if t is None else t.data_ptr() for t in (x2d, traj, cam)]
    if B == 0 and len(given) == 3:
        ptrs = [None] * 3                    # empty tensors have no storage to point the library at
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_pose_partials(
            _data(pred), *ptrs, _data(conn), B, T, P_r, F, J, int(h0),
            _data(out), out.numel() * 8, _stream(pred)))
    return out


def pose_partials_fit(pred, conn, h0, x2d, cam, conf=None, out=None, tfit=None):
    """One shard's pose state WITHOUT a trajectory (pafuse_pose_partials_fit): pred [B,T,P_r,F,J,3] the LOCAL part-centred
    hypotheses [h0, h0 + P_r), conn int32 [J], x2d [B,F,J,2] screen-normalised detections, cam [9], conf [B,F,J] their
    weights (None: every weight 1; not > 0: the joint takes no part and gets no pick).  The root of every (hypothesis,
    frame) is fitted on the device (pafuse_amd.rootfit states the arithmetic) and stands in for traj -> the flat state of
    pose_partials.  `out`: as there.  `tfit`: a contiguous fp32 [B,T,P_r,F,3] tensor that receives the fitted roots, NaN
    where there is no fit."""
    lib = _lib.load()
    B, T, P_r, F, J = _need_pred("pose_partials_fit", pred)
    _need(T > 0 and F > 0 and J > 0 and int(h0) >= 0, "pose_partials_fit: T, F, J > 0 and h0 >= 0")
    _need(conn.numel() == J and conn.dtype == torch.int32, "pose_partials_fit: conn must be int32 [J]")
    _need(x2d is not None and cam is not None, "pose_partials_fit: x2d and cam are needed")
    _need(tuple(x2d.shape) == (B, F, J, 2) and cam.numel() == 9 and (conf is None or tuple(conf.shape) == (B, F, J))
          and (tfit is None or tuple(tfit.shape) == (B, T, P_r, F, 3)), "pose_partials_fit: operands do not match pred")
    _need_tensors("pose_partials_fit", [pred, x2d, cam] + [t for t in (conf, tfit) if t is not None], (conn,))
    dev = pred.device
    need = int(lib.pafuse_pose_partials_bytes(B, T, F, J))
    assert need == pose_partials_bytes(B, T, F, J)
    out = _state_out("pose_partials_fit", out, need, dev)
    x2d_ptr = x2d.data_ptr() if B else cam.data_ptr()   # B == 0: no storage to point at, and the library reads none of it
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_pose_partials_fit(
            _data(pred), x2d_ptr, None if conf is None else _data(conf), cam.data_ptr(),
            _data(conn), B, T, P_r, F, J, int(h0), _data(out), out.numel() * 8, None if tfit is None else _data(tfit),
            _stream(pred)))
    return out


def combine_poses(states, shape, num_proposals, merged=None, want=("mean", "pick", "idx"), no_pick_ok=False):
    """pafuse_pose_combine: `states` [W, L] float64 (W flat pose states of the same (B,T,F,J) = `shape`, one per row, in
    ascending-h0 order; rows may be padded) -> dict with the entries named in `want`: "mean" [B,T,F,J,3] (the sums
    divided by `num_proposals`, the TOTAL hypothesis count), "pick" [B,T,F,J,3], "idx" [B,T,F,J] int32.  `merged`: a
    float64 buffer that receives the state of the union; of the operands it may only be states[0] (a running state).
    Asking for "pick" or "idx" when no state holds a single candidate (mean-only states) raises - after the launch, at
    the price of one synchronisation.  no_pick_ok=True (states of pose_partials_fit, where a batch without one weighted
    detection is legitimate) skips that check: the pick is then NaN and idx -1 throughout."""
    lib = _lib.load()
    B, T, F, J = (int(v) for v in shape)
    n = B * T * F * J
    L = pose_partials_bytes(B, T, F, J) // 8
    want = tuple(want)
    _need(all(k in ("mean", "pick", "idx") for k in want), f"combine_poses: want holds mean, pick, idx - got {want}")
    _need_rows(states, L, f"combine_poses: states must be [W, >= {L}] float64")
    _need(T > 0 and F > 0 and J > 0 and B >= 0, "combine_poses: bad shape")
    _need(want or merged is not None, "combine_poses: nothing to compute")
    _need("mean" not in want or int(num_proposals) >= 1, "combine_poses: num_proposals >= 1")
    dev = states.device
    if merged is not None:
        _need_merged("combine_poses", merged, states, L, L, states.numel(), "first")
    out = {}
    if "mean" in want:
        out["mean"] = torch.empty(B, T, F, J, 3, device=dev)
    if "pick" in want:
        out["pick"] = torch.empty(B, T, F, J, 3, device=dev)
    if "idx" in want or "pick" in want:
        idx = torch.empty(B, T, F, J, device=dev, dtype=torch.int32)
        if "idx" in want:
            out["idx"] = idx
    if n == 0:
        return out
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_pose_combine(
            states.data_ptr(), states.shape[0], states.shape[1] * 8, B, T, F, J, int(num_proposals),
            None if merged is None else merged.data_ptr(), ptr("mean"), ptr("pick"),
            idx.data_ptr() if ("idx" in want or "pick" in want) else None, _stream(states)))
    if ("idx" in want or "pick" in want) and not no_pick_ok and not bool((idx >= 0).any()):
        raise _lib.PafuseError("combine_poses: no state holds a J-Agg candidate (mean-only states have no pick)")
    return out


PATH_OUTPUTS = ("pick", "idx", "e2", "cost")


def _path_call(who, names, want):
    """What pose_path and frames_path share around their own shape checks.  Now: `want` checked against the outputs `names`
    -> (want, buffers).  Once the shapes are known, buffers(frames, lines, need, workspace, dev) -> (out, workspace, ptr):
    the outputs by name ("pick" [*frames,3], "idx" and - where named - "window" [*frames] int32 always, "e2" [*frames] and
    "cost" [*lines] float64 when wanted), the checked workspace (a new one of `need` bytes for None) and the pointer of a
    tensor that may be None."""
    want = tuple(want)
    _need(all(k in names for k in want) and want, f"{who}: want holds some of {names} - got {want}")

    def buffers(frames, lines, need, workspace, dev):
        out = {"pick": torch.empty(*frames, 3, device=dev)}
        out.update((k, torch.empty(*frames, device=dev, dtype=torch.int32)) for k in ("idx", "window") if k in names)
        if "e2" in want:
            out["e2"] = torch.empty(*frames, device=dev)
        if "cost" in want:
            out["cost"] = torch.empty(*lines, device=dev, dtype=torch.float64)
        if workspace is None:
            workspace = _lib.workspace(need, dev, who)
        _need(workspace.is_cuda and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous(),
              f"{who}: workspace must be a uint8 buffer on {dev}")
        return out, workspace, lambda t: None if t is None else _data(t)
    return want, buffers


def pose_path_workspace_bytes(B, T, P, F, J):
    """Bytes of the workspace pafuse_pose_path needs (the formula of pafuse_pose_path_workspace_bytes): one back-pointer
    byte per (b, t, j, f, h), rounded up to a multiple of 8."""
    return (B * T * J * F * P + 7) // 8 * 8


def pose_path(pred, conn, x2d, root, cam, weight, conf=None, mean=None, want=("pick", "idx"), workspace=None):
    """J-Agg coherent in time (pafuse_pose_path; pafuse_amd.posepath states the arithmetic): pred [B,T,P,F,J,3] ALL P <= 256
    part-centred hypotheses of clips of F <= 256 frames, conn int32 [J], x2d [B,F,J,2], root [B,F,3] (or [B,F,1,3]) one
    trajectory or [B,T,P,F,3] a root per hypothesis (tfit of pose_partials_fit), cam [9], weight >= 0 (normalised screen
    length per metre; 0: the per-frame pick), conf [B,F,J] (None: all observed; not > 0: that frame is unobserved for that
    joint), mean [B,T,F,J,3] the pose the offsets are taken against (None: absolute) -> dict with the entries of `want`:
    "pick" [B,T,F,J,3], "idx" [B,T,F,J] int32, "e2" [B,T,F,J], "cost" [B,T,J] float64.  A line without a path: NaN, -1, +inf,
    NaN.  `workspace`: a uint8 buffer of pose_path_workspace_bytes or more to use instead of a new one."""
    lib = _lib.load()
    B, T, P, F, J = _need_pred("pose_path", pred, axis="P")
    want, buffers = _path_call("pose_path", PATH_OUTPUTS, want)
    _need(T > 0 and P > 0 and F > 0 and J > 0, "pose_path: T, P, F, J > 0")
    _need(conn.numel() == J and conn.dtype == torch.int32, "pose_path: conn must be int32 [J]")
    per_h = root.dim() == 5
    _need(tuple(x2d.shape) == (B, F, J, 2) and cam.numel() == 9 and (conf is None or tuple(conf.shape) == (B, F, J))
          and (mean is None or tuple(mean.shape) == (B, T, F, J, 3))
          and (tuple(root.shape) == (B, T, P, F, 3) if per_h else root.numel() == B * F * 3), "pose_path: operands do not match pred")
    _need_tensors("pose_path", [pred, x2d, root, cam] + [t for t in (conf, mean) if t is not None], (conn,))
    weight = float(weight)
    dev = pred.device
    need = int(lib.pafuse_pose_path_workspace_bytes(B, T, P, F, J)) if P <= 256 and F <= 256 else 0   # beyond: the library refuses
    assert need == (pose_path_workspace_bytes(B, T, P, F, J) if P <= 256 and F <= 256 else 0)
    out, workspace, ptr = buffers((B, T, F, J), (B, T, J), need, workspace, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_pose_path(
            _data(pred), _data(x2d), _data(root), int(per_h), cam.data_ptr(), ptr(conf), _data(conn), ptr(mean), weight,
            B, T, P, F, J, _data(out["pick"]), _data(out["idx"]), ptr(out.get("e2")), ptr(out.get("cost")),
            _data(workspace), workspace.numel(), _stream(pred)))
    return {k: out[k] for k in want}


FRAMES_PATH_OUTPUTS = ("pick", "idx", "window", "e2", "cost")
FRAMES_PATH_MAX_CANDIDATES = 256    # P times the largest number of windows that cover one frame


def _video_windows(who, starts, valid, N, F=None):
    """starts, valid of the windows of a WHOLE video of N frames, as pafuse_frames_path wants them -> (int32 starts, int32
    valid, the largest number of windows that cover one frame), or None where the library would refuse them"""
    import numpy as np
    hs = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1))
    hv = np.ascontiguousarray(np.asarray(valid, dtype=np.int32).reshape(-1))
    _need(hs.shape == hv.shape, f"{who}: starts and valid are two vectors of one length")
    s, e = hs.astype(np.int64), hs.astype(np.int64) + hv
    if (hs.shape[0] < 1 or int(N) < 1 or s[0] != 0 or e[-1] != int(N) or (hv < 1).any() or (F is not None and (hv > F).any())
            or (np.diff(s) <= 0).any() or (np.diff(e) < 0).any() or (s[1:] > e[:-1]).any()):
        return None
    cover = int(max(w - int(np.searchsorted(e, s[w], side="right")) + 1 for w in range(hs.shape[0])))
    return hs, hv, cover


def frames_path_workspace_bytes(N, T, J, P, starts, valid):
    """Bytes of the workspace pafuse_frames_path needs (the formula of pafuse_frames_path_workspace_bytes): one back-pointer
    byte per (t, j, n, slot) with K = P * the largest coverage slots per frame, rounded up to a multiple of 8; 0 for sizes
    and windows the library refuses (K > 256 among them)."""
    if min(int(N), int(T), int(J), int(P)) < 1:
        return 0
    tables = _video_windows("frames_path_workspace_bytes", starts, valid, N)
    if tables is None or tables[2] * int(P) > FRAMES_PATH_MAX_CANDIDATES:
        return 0
    return (int(T) * int(J) * int(N) * tables[2] * int(P) + 7) // 8 * 8


def frames_path(pred, conn, x2d, root, cam, weight, starts, valid, conf=None, mean=None, want=("pick", "idx", "window"),
                workspace=None):
    """The J-Agg path of a whole VIDEO (pafuse_frames_path; pafuse_amd.posepath.frames_path states it): pred [W,T,P,F,J,3] ALL
    part-centred hypotheses of the W windows of one video of N frames, window w covering the frames [starts[w], starts[w] +
    valid[w]) (host integers, pafuse_amd.windows.window_starts: the whole video, no gap); conn int32 [J], x2d [N,J,2], root
    [N,3] one trajectory or [W,T,P,F,3] a root per hypothesis (tfit of pose_partials_fit), cam [9], weight >= 0, conf [N,J]
    (None: all observed), mean [T,N,J,3] the pooled mean the offsets are taken against (finish_frames; None: absolute).  At
    every frame the candidates are the hypotheses of all windows covering it, at most 256 -> dict with the entries of
    `want`: "pick" [T,N,J,3], "idx" and "window" [T,N,J] int32, "e2" [T,N,J], "cost" [T,J] float64.  A line without a path:
    NaN, -1, -1, +inf, NaN at every frame.  `workspace`: a uint8 buffer of frames_path_workspace_bytes or more to use
    instead of a new one."""
    lib = _lib.load()
    W, T, P, F, J = (int(v) for v in _need_pred("frames_path", pred, axis="P"))
    want, buffers = _path_call("frames_path", FRAMES_PATH_OUTPUTS, want)
    _need(W > 0 and T > 0 and P > 0 and F > 0 and J > 0, "frames_path: W, T, P, F, J > 0 (a video has at least one window)")
    _need(x2d.dim() == 3 and x2d.shape[0] > 0, "frames_path: x2d must be [N,J,2]")
    N = int(x2d.shape[0])
    _need(conn.numel() == J and conn.dtype == torch.int32, "frames_path: conn must be int32 [J]")
    per_h = root.dim() == 5
    _need(tuple(x2d.shape) == (N, J, 2) and cam.numel() == 9 and (conf is None or tuple(conf.shape) == (N, J))
          and (mean is None or tuple(mean.shape) == (T, N, J, 3))
          and (tuple(root.shape) == (W, T, P, F, 3) if per_h else root.numel() == N * 3), "frames_path: operands do not match pred")
    _need_tensors("frames_path", [pred, x2d, root, cam] + [t for t in (conf, mean) if t is not None], (conn,))
    tables = _video_windows("frames_path", starts, valid, N, F)
    _need(tables is not None and tables[0].shape[0] == W,
          f"frames_path: starts / valid must be the W = {W} windows of the whole video of N = {N} frames (from 0, no gap, ends ascending, to N)")
    hs, hv, cover = tables
    _need(cover * P <= FRAMES_PATH_MAX_CANDIDATES, f"frames_path: {cover} windows cover one frame with P = {P} hypotheses each: "
          f"at most {FRAMES_PATH_MAX_CANDIDATES} candidates per frame")
    weight = float(weight)
    dev = pred.device
    need = int(lib.pafuse_frames_path_workspace_bytes(N, T, J, P, W, hs.ctypes.data, hv.ctypes.data))
    assert need == frames_path_workspace_bytes(N, T, J, P, hs, hv)
    out, workspace, ptr = buffers((T, N, J), (T, J), need, workspace, dev)
    import numpy as np
    dtab = torch.from_numpy(np.stack([hs, hv])).to(dev)     # the device copies the kernel reads
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_frames_path(
            _data(pred), _data(x2d), _data(root), int(per_h), cam.data_ptr(), ptr(conf), _data(conn), ptr(mean), weight,
            W, T, P, F, J, N, dtab[0].data_ptr(), dtab[1].data_ptr(), hs.ctypes.data, hv.ctypes.data,
            _data(out["pick"]), _data(out["idx"]), _data(out["window"]), ptr(out.get("e2")), ptr(out.get("cost")),
            _data(workspace), workspace.numel(), _stream(pred)))
    return {k: out[k] for k in want}


# ------------------------------------------------------------------------------------- spread of the hypotheses
SPREAD_STATE_DOUBLES_PER_ELEMENT = 9   # double sum[3] + double m2[6] per (b, t, f, j); one more double, the count, ends the state
SPREAD_OUTPUTS = {"mean": (3,), "cov": (6,), "std": ()}   # trailing shape of every output of combine_spread behind [B,T,F,J]


def spread_partials_bytes(B, T, F, J):
    """Bytes of the state pafuse_spread_partials writes (the formula of pafuse_spread_partials_bytes, restated so that sizes
    can be planned without the library): 72 bytes per (b,t,f,j) and 8 for the count, all float64; 0 for an empty shape.
    No P in it."""
    n = B * T * F * J
    return (SPREAD_STATE_DOUBLES_PER_ELEMENT * n + 1) * 8 if min(B, T, F, J) > 0 else 0


def spread_views(state, B, T, F, J):
    """Typed views of a flat spread state (1-D float64 tensor of spread_partials_bytes / 8 elements, or longer):
    sum [B,T,F,J,3], m2 [B,T,F,J,6] (xx, xy, xz, yy, yz, zz), count [1], all f64."""
    n = B * T * F * J
    _need(state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous() and n > 0
          and state.numel() * 8 >= spread_partials_bytes(B, T, F, J), "spread_views: not a state of these sizes")
    return {"sum": state[:3 * n].view(B, T, F, J, 3), "m2": state[3 * n:9 * n].view(B, T, F, J, 6), "count": state[9 * n:9 * n + 1]}


def spread_partials(pred, conn, h0, out=None):
    """One shard's spread state (pafuse_spread_partials): pred [B,T,P_r,F,J,3] the LOCAL part-centred hypotheses
    [h0, h0 + P_r) of the run, conn int32 [J] -> the flat state, a 1-D float64 tensor (spread_views names its pieces).
    `out`: a float64 buffer at least that long to write into; the result is then `out` itself."""
    lib = _lib.load()
    B, T, P_r, F, J = _need_pred("spread_partials", pred)
    _need(T > 0 and F > 0 and J > 0 and int(h0) >= 0, "spread_partials: T, F, J > 0 and h0 >= 0")
    _need(conn.numel() == J and conn.dtype == torch.int32, "spread_partials: conn must be int32 [J]")
    _need_tensors("spread_partials", (pred,), (conn,))
    dev = pred.device
    need = int(lib.pafuse_spread_partials_bytes(B, T, F, J))
    assert need == spread_partials_bytes(B, T, F, J)
    out = _state_out("spread_partials", out, need, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_spread_partials(_data(pred), _data(conn), B, T, P_r, F, J, int(h0), _data(out), out.numel() * 8,
                                              _stream(pred)))
    return out


def combine_spread(states, shape, merged=None, want=("mean", "cov", "std")):
    """pafuse_spread_combine: `states` [W, L] float64 (W flat spread states of the same (B,T,F,J) = `shape`, one per row, in
    ascending-h0 order; rows may be padded) -> dict with the entries named in `want`: "mean" [B,T,F,J,3] (the sums divided
    by the states' total count), "cov" [B,T,F,J,6] (population covariance: xx, xy, xz, yy, yz, zz) and "std" [B,T,F,J] (RMS
    distance from the mean joint), fp32.  `merged`: a float64 buffer that receives the state of the union; of the
    operands it may only be states[0] (a running state)."""
    lib = _lib.load()
    B, T, F, J = (int(v) for v in shape)
    n = B * T * F * J
    L = spread_partials_bytes(B, T, F, J) // 8
    want = tuple(want)
    _need(all(k in SPREAD_OUTPUTS for k in want), f"combine_spread: want holds mean, cov, std - got {want}")
    _need_rows(states, L, f"combine_spread: states must be [W, >= {L}] float64")
    _need(T > 0 and F > 0 and J > 0 and B >= 0, "combine_spread: bad shape")
    _need(want or merged is not None, "combine_spread: nothing to compute")
    dev = states.device
    if merged is not None:
        _need_merged("combine_spread", merged, states, L, L, states.numel(), "first")
    out = {k: torch.empty(B, T, F, J, *SPREAD_OUTPUTS[k], device=dev) for k in want}
    if n == 0:
        return out
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_spread_combine(
            states.data_ptr(), states.shape[0], states.shape[1] * 8, B, T, F, J,
            None if merged is None else merged.data_ptr(), ptr("mean"), ptr("cov"), ptr("std"), _stream(states)))
    return out


# ----------------------------------------------------------------- overlapping windows pooled into one pose per frame
FRAME_POSE_BYTES_PER_ROW = 48   # double sum[3] + float e2 + int32 idx + int32 win + float sel[3] per (t, n, j); + int32 count per frame
FRAME_OUTPUTS = {"mean": ((3,), torch.float32), "pick": ((3,), torch.float32), "idx": ((), torch.int32), "window": ((), torch.int32),
                 "std": ((), torch.float32), "cov": ((6,), torch.float32)}      # trailing shape and dtype behind [T,N,J]


def frame_state_bytes(N, T, J, spread=False):
    """Bytes of a frame state over N video frames (the formulas of pafuse_frame_pose_state_bytes / _spread_state_bytes):
    pose 48 per (t,n,j) + 4 per frame, rounded up to 8; spread 72 per (t,n,j) + 8 per frame."""
    if min(N, T, J) <= 0:
        return 0
    return (9 * N * T * J + N) * 8 if spread else (FRAME_POSE_BYTES_PER_ROW * N * T * J + 4 * N + 7) // 8 * 8


def frame_state(N, T, J, device="cuda", spread=False, out=None):
    """The NEUTRAL frame state of N video frames as a flat float64 tensor (pafuse_frame_pose_state_init /
    pafuse_frame_spread_state_init): zero sums and counts and no candidate (+inf, -1, -1, NaN NaN NaN); spread=True: the
    frame spread state, all zeros.  `out`: a float64 buffer at least that long to write into."""
    lib = _lib.load()
    N, T, J = int(N), int(T), int(J)
    _need(N > 0 and T > 0 and J > 0, "frame_state: N, T, J > 0")
    dev = out.device if out is not None else torch.empty(0, device=device).device
    _need(dev.type == "cuda", "frame_state: a HIP device (no CPU fallback)")
    need = int((lib.pafuse_frame_spread_state_bytes if spread else lib.pafuse_frame_pose_state_bytes)(N, T, J))
    assert need == frame_state_bytes(N, T, J, spread)
    out = _state_out("frame_state", out, need, dev)
    init = lib.pafuse_frame_spread_state_init if spread else lib.pafuse_frame_pose_state_init
    with torch.cuda.device(out.device):
        _lib.check(init(out.data_ptr(), out.numel() * 8, N, T, J, _stream(out)))
    return out


def frame_views(state, N, T, J, spread=False):
    """Typed views of a flat frame state: pose - sum [T,N,J,3] f64, e2 [T,N,J] f32, idx, win [T,N,J] i32, sel [T,N,J,3] f32,
    count [N] i32; spread=True - sum [T,N,J,3], m2 [T,N,J,6], count [N], all f64."""
    r = N * T * J
    _need(state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous() and r > 0
          and state.numel() * 8 >= frame_state_bytes(N, T, J, spread), "frame_views: not a frame state of these sizes")
    if spread:
        return {"sum": state[:3 * r].view(T, N, J, 3), "m2": state[3 * r:9 * r].view(T, N, J, 6), "count": state[9 * r:9 * r + N]}
    f32 = state[3 * r:].view(torch.float32)
    i32 = f32.view(torch.int32)
    return {"sum": state[:3 * r].view(T, N, J, 3), "e2": f32[:r].view(T, N, J), "idx": i32[r:2 * r].view(T, N, J),
            "win": i32[2 * r:3 * r].view(T, N, J), "sel": f32[3 * r:6 * r].view(T, N, J, 3), "count": i32[6 * r:6 * r + N]}


def _fold_operands(who, frame, N, state, shape, starts, valid, spread):
    import numpy as np
    B, T, F, J = (int(v) for v in shape)
    N = int(N)
    _need(B >= 0 and T > 0 and F > 0 and J > 0 and N > 0, f"{who}: bad shape")
    for name, t in (("frame", frame), ("state", state)):
        _need(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous(),
              f"{who}: {name} must be a flat float64 tensor on a HIP device (no CPU fallback)")
    _need(state.device == frame.device, f"{who}: frame and state on one device")
    _need(frame.numel() * 8 >= frame_state_bytes(N, T, J, spread), f"{who}: the frame state needs {frame_state_bytes(N, T, J, spread)} bytes")
    need = spread_partials_bytes(B, T, F, J) if spread else pose_partials_bytes(B, T, F, J)
    _need(state.numel() * 8 >= need, f"{who}: the batch state needs {need} bytes")
    hs = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1))
    hv = np.ascontiguousarray(np.asarray(valid, dtype=np.int32).reshape(-1))
    _need(hs.shape[0] == B and hv.shape[0] == B, f"{who}: starts and valid must hold B = {B} windows")
    _need(bool(((hv >= 1) & (hv <= F)).all()), f"{who}: valid must lie in 1 .. F = {F}")
    _need(bool((hs >= 0).all() and (hs.astype(np.int64) + hv <= N).all()), f"{who}: a window reaches past the N = {N} frames")
    _need(bool((np.diff(hs) > 0).all()), f"{who}: starts must ascend strictly")
    tables = torch.from_numpy(np.stack([hs, hv])).to(frame.device) if B else None     # the device copies the kernels read
    return B, T, F, J, N, hs, hv, tables


def fold_windows(frame, N, state, shape, starts, valid, w0, num_proposals):
    """pafuse_pose_windows_fold: fold `state`, the flat pose state of B windows (`shape` = (B,T,F,J); what pose_partials,
    pose_partials_fit or combine_poses(merged=) wrote for the union of `num_proposals` hypotheses), into the frame pose
    state `frame` of N video frames, in place -> frame.  starts, valid: B host integers each (pafuse_amd.windows.window_starts),
    strictly ascending starts; window b covers frames [starts[b], starts[b] + valid[b]).  w0: the global index of the
    batch's first window (it is what "window" of finish_frames reports).  Batches come in ascending window order; the
    result does not depend on how the windows are cut into batches."""
    lib = _lib.load()
    B, T, F, J, N, hs, hv, tables = _fold_operands("fold_windows", frame, N, state, shape, starts, valid, False)
    _need(int(w0) >= 0 and int(num_proposals) >= 0, "fold_windows: w0 and num_proposals >= 0")
    if B == 0:
        return frame
    dev = frame.device
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_pose_windows_fold(
            frame.data_ptr(), frame.numel() * 8, N, state.data_ptr(), state.numel() * 8, B, T, F, J,
            tables[0].data_ptr(), tables[1].data_ptr(), hs.ctypes.data, hv.ctypes.data, int(w0), int(num_proposals), _stream(frame)))
    return frame


def fold_spread_windows(frame, N, state, shape, starts, valid):
    """pafuse_spread_windows_fold: fold `state`, the flat spread state of B windows (spread_partials, or
    combine_spread(merged=)), into the frame spread state `frame` (frame_state(spread=True)) in place -> frame.  Operands
    as fold_windows; every covering window is merged by Chan's rule and adds its count to the frame's."""
    lib = _lib.load()
    B, T, F, J, N, hs, hv, tables = _fold_operands("fold_spread_windows", frame, N, state, shape, starts, valid, True)
    if B == 0:
        return frame
    dev = frame.device
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_spread_windows_fold(
            frame.data_ptr(), frame.numel() * 8, N, state.data_ptr(), state.numel() * 8, B, T, F, J,
            tables[0].data_ptr(), tables[1].data_ptr(), hs.ctypes.data, hv.ctypes.data, _stream(frame)))
    return frame


def finish_frames(N, T, J, frame=None, spread=None, want=None):
    """pafuse_frames_finish -> dict with the entries named in `want`: from the frame pose state `frame` "mean" [T,N,J,3]
    (sum / count[n]), "pick" [T,N,J,3], "idx" and "window" [T,N,J] int32 (the J-Agg pose, its hypothesis and its window;
    NaN / -1 / -1 without a candidate); from the frame spread state `spread` "std" [T,N,J] and "cov" [T,N,J,6].  Also
    "count" [N]: the hypotheses folded into every frame (int64; from `frame`, else from `spread`).  want=None: everything
    the given states hold except "count"."""
    lib = _lib.load()
    N, T, J = int(N), int(T), int(J)
    _need(N > 0 and T > 0 and J > 0, "finish_frames: N, T, J > 0")
    _need(frame is not None or spread is not None, "finish_frames: no state")
    if want is None:
        want = (("mean", "pick", "idx", "window") if frame is not None else ()) + (("std", "cov") if spread is not None else ())
    want = tuple(want)
    _need(all(k in FRAME_OUTPUTS or k == "count" for k in want), f"finish_frames: want holds {sorted(FRAME_OUTPUTS)} and count - got {want}")
    _need(frame is not None or not any(k in want for k in ("mean", "pick", "idx", "window")), "finish_frames: mean, pick, idx and window need the frame pose state")
    _need(spread is not None or not any(k in want for k in ("std", "cov")), 'finish_frames: "std" and "cov" need the frame spread state')
    for name, t, sp in (("frame", frame, False), ("spread", spread, True)):
        _need(t is None or (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1
                            and t.is_contiguous() and t.numel() * 8 >= frame_state_bytes(N, T, J, sp)),
              f"finish_frames: {name} must be a flat float64 frame state of {frame_state_bytes(N, T, J, sp)} bytes on a HIP device")
    first = frame if frame is not None else spread
    _need(frame is None or spread is None or frame.device == spread.device, "finish_frames: both states on one device")
    dev = first.device
    out = {k: torch.empty(T, N, J, *FRAME_OUTPUTS[k][0], device=dev, dtype=FRAME_OUTPUTS[k][1]) for k in want if k != "count"}
    ptr = lambda k: out[k].data_ptr() if k in out else None
    if out:
        with torch.cuda.device(dev):
            _lib.check(lib.pafuse_frames_finish(
                None if frame is None else frame.data_ptr(), None if spread is None else spread.data_ptr(), N, T, J,
                ptr("mean"), ptr("pick"), ptr("idx"), ptr("window"), ptr("std"), ptr("cov"), _stream(first)))
    if "count" in want:
        out["count"] = (frame_views(frame, N, T, J)["count"] if frame is not None
                        else frame_views(spread, N, T, J, spread=True)["count"]).to(torch.int64)
    return out


# ------------------------------------------------------------------ the camera-space root of the per-frame pose
TRAJECTORY_OUTPUTS = ("traj", "wsum", "resid")


def _frame_pose_operands(who, pose, x2d, cam, conf):
    """pose [T,N,J,3] beside its detections x2d [N,J,2], cam [>= 4] and conf [N,J] or None, as fit_trajectory and focal_sums take them"""
    _need(isinstance(pose, torch.Tensor) and pose.dim() == 4 and pose.shape[-1] == 3, f"{who}: pose must be [T,N,J,3]")
    T, N, J = (int(v) for v in pose.shape[:3])
    _need(T > 0 and N > 0 and J > 0, f"{who}: T, N, J > 0")
    _need(x2d is not None and cam is not None, f"{who}: x2d and cam are needed")
    _need(tuple(x2d.shape) == (N, J, 2) and cam.dim() == 1 and cam.numel() >= 4 and (conf is None or tuple(conf.shape) == (N, J)),
          f"{who}: x2d [N,J,2], cam [>= 4] and conf [N,J] must match pose [T,N,J,3]")
    _need_tensors(who, [pose, x2d, cam] + ([] if conf is None else [conf]), ())
    return T, N, J


def _need_radius(who, radius):
    _need(not isinstance(radius, bool) and int(radius) == radius and 1 <= int(radius) <= 64, f"{who}: radius must be an integer in 1 .. 64, got {radius!r}")


def fit_trajectory(pose, x2d, cam, conf=None, want=TRAJECTORY_OUTPUTS):
    """pafuse_frames_root_fit: pose [T,N,J,3] the finished whole-body, root-relative pose of every (t, frame) (finish_frames'
    "mean" or "pick", or stitched clips), x2d [N,J,2] screen-normalised detections, cam [>= 4] (fx fy cx cy first), conf
    [N,J] their weights (None: every weight 1) -> dict with the entries named in `want`: "traj" [T,N,3] the fitted root
    (NaN where there is no fit), "wsum" [T,N] the weight the fit rests on (0 where none), "resid" [T,N] the weighted
    algebraic residual in metres (NaN where none).  A joint without a positive weight or with a non-finite pose takes no
    part (pafuse_amd.trajectory states the arithmetic).  Camera-space poses are pose + traj[:, :, None]."""
    lib = _lib.load()
    want = tuple(want)
    _need(all(k in TRAJECTORY_OUTPUTS for k in want) and "traj" in want, f'fit_trajectory: want holds "traj" and any of wsum, resid - got {want}')
    T, N, J = _frame_pose_operands("fit_trajectory", pose, x2d, cam, conf)
    dev = pose.device
    out = {k: torch.empty((T, N, 3) if k == "traj" else (T, N), device=dev, dtype=torch.float32) for k in want}
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_frames_root_fit(pose.data_ptr(), x2d.data_ptr(), None if conf is None else conf.data_ptr(),
                                              cam.data_ptr(), T, N, J, ptr("traj"), ptr("wsum"), ptr("resid"), _stream(pose)))
    return out


def smooth_trajectory(traj, weight, radius, out=None):
    """pafuse_trajectory_smooth: traj [T,N,3] (NaN: no fit), weight [T,N] or None (every weight 1), radius 1 .. 64 ->
    [T,N,3]: the confidence-weighted local-linear filter along the frames (pafuse_amd.trajectory.smooth states it); a frame
    takes part if its weight is > 0 and its root finite, a frame without a fit is filled from its neighbours, and a frame
    with nothing within `radius` stays NaN.  `out`: a [T,N,3] tensor to write into that shares no memory with traj."""
    lib = _lib.load()
    _need(isinstance(traj, torch.Tensor) and traj.dim() == 3 and traj.shape[-1] == 3, "smooth_trajectory: traj must be [T,N,3]")
    T, N = int(traj.shape[0]), int(traj.shape[1])
    _need(T > 0 and N > 0, "smooth_trajectory: T, N > 0")
    _need_radius("smooth_trajectory", radius)
    _need(weight is None or tuple(weight.shape) == (T, N), "smooth_trajectory: weight must be [T,N]")
    if out is None:
        out = torch.empty_like(traj)
    _need(tuple(out.shape) == (T, N, 3), "smooth_trajectory: out must be [T,N,3]")
    lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
    _need(hi <= traj.data_ptr() or lo >= traj.data_ptr() + traj.numel() * 4,
          "smooth_trajectory: out may not alias traj (every frame is read by its neighbours)")
    _need_tensors("smooth_trajectory", [traj, out] + ([] if weight is None else [weight]), ())
    with torch.cuda.device(traj.device):
        _lib.check(lib.pafuse_trajectory_smooth(traj.data_ptr(), None if weight is None else weight.data_ptr(), T, N, int(radius),
                                                out.data_ptr(), _stream(traj)))
    return out


# ------------------------------------------------------------------ the per-frame pose smoothed along the frames
def _need_floor(who, floor):
    import struct
    ok = not isinstance(floor, bool) and isinstance(floor, (int, float))
    if ok:
        try:
            f32 = struct.unpack("f", struct.pack("f", float(floor)))[0]       # what the entry will see
        except OverflowError:
            f32 = float("inf")
        ok = 0.0 < f32 < float("inf")
    _need(ok, f"{who}: floor must be a number that is finite and > 0 in fp32 (metres), got {floor!r}")


def smooth_poses_workspace_bytes(T, N, J):
    """pafuse_pose_smooth_workspace_bytes: 48 bytes per (t, frame, joint) - the precision of every row, formed once"""
    return int(_lib.load().pafuse_pose_smooth_workspace_bytes(int(T), int(N), int(J)))


def smooth_poses(pose, cov, radius, floor=1e-3, out=None, want_code=False, workspace=None):
    """pafuse_pose_smooth: pose [T,N,J,3] the finished per-frame pose (NaN: none), cov [T,N,J,6] the covariance of its
    hypotheses (finish_frames' "cov": xx xy xz yy yz zz) or None (zeros: every frame weighs the same in every direction),
    radius 1 .. 64, floor in metres -> [T,N,J,3]: per joint the local-linear filter along the frames in which frame m enters
    with the matrix weight (cov + floor^2 I)^-1 (pafuse_amd.posesmooth states it).  A row with a NaN pose, a NaN or an
    indefinite covariance takes no part and is filled from its neighbours; a (t, frame, joint) with nothing within `radius` is
    NaN.  The floor is a regulariser - it keeps a zero covariance (P = 1, identical hypotheses) solvable - not a tuned value.
    `out`: a [T,N,J,3] tensor to write into that shares no memory with pose.  want_code=True: -> (out, code [T,N,J] uint8:
    1 line, 2 weighted mean, 3 none).  `workspace`: a flat float64 tensor of smooth_poses_workspace_bytes(T, N, J) bytes or more
    to reuse (None: allocated here)."""
    lib = _lib.load()
    _need(isinstance(pose, torch.Tensor) and pose.dim() == 4 and pose.shape[-1] == 3, "smooth_poses: pose must be [T,N,J,3]")
    T, N, J = (int(v) for v in pose.shape[:3])
    _need(T > 0 and N > 0 and J > 0, "smooth_poses: T, N, J > 0")
    _need_radius("smooth_poses", radius)
    _need_floor("smooth_poses", floor)
    _need(cov is None or (isinstance(cov, torch.Tensor) and tuple(cov.shape) == (T, N, J, 6)), "smooth_poses: cov must be [T,N,J,6]")
    if out is None:
        out = torch.empty_like(pose)
    _need(isinstance(out, torch.Tensor) and tuple(out.shape) == (T, N, J, 3), "smooth_poses: out must be [T,N,J,3]")
    lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
    _need(hi <= pose.data_ptr() or lo >= pose.data_ptr() + pose.numel() * 4,
          "smooth_poses: out may not alias pose (every frame is read by its neighbours)")
    _need_tensors("smooth_poses", [pose, out] + ([] if cov is None else [cov]), ())
    need = smooth_poses_workspace_bytes(T, N, J)
    if workspace is None:
        workspace = _lib.workspace(need, pose.device, "smooth_poses", torch.float64)
    _need(isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == pose.device and workspace.dtype == torch.float64
          and workspace.dim() == 1 and workspace.is_contiguous() and workspace.numel() * 8 >= need,
          f"smooth_poses: workspace must be a flat float64 tensor of {need} bytes or more on {pose.device}")
    code = torch.empty((T, N, J), device=pose.device, dtype=torch.uint8) if want_code else None
    with torch.cuda.device(pose.device):
        _lib.check(lib.pafuse_pose_smooth(pose.data_ptr(), None if cov is None else cov.data_ptr(), T, N, J, int(radius), float(floor),
                                          out.data_ptr(), None if code is None else code.data_ptr(), workspace.data_ptr(),
                                          workspace.numel() * 8, _stream(pose)))
    return (out, code) if want_code else out


# ------------------------------------------------------------------ bone lengths held constant along a video
_TABLE_CACHE_MAX = 16
_table_cache = {}   # (tag, the table's bytes, device) -> its int32 device copy; the oldest entry goes first


def _index_table(who, table, J, check, device, tag):
    """An index table of a per-frame kernel, validated on the host: an integer sequence, numpy array or tensor (refused as `who`
    when its dtype is not an integer's); check(table, J) -> int32 contiguous numpy, or a ValueError.  -> that array; with
    `device` its int32 copy there, cached under (tag, bytes, device)."""
    import numpy as np
    if isinstance(table, torch.Tensor):
        _need(not table.dtype.is_floating_point and table.dtype != torch.bool, who)
        table = table.detach().cpu().numpy()
    table = check(np.asarray(table), int(J))
    if device is None:
        return table
    key = (tag, table.tobytes(), str(device))
    hit = _table_cache.get(key)
    if hit is None:
        if len(_table_cache) >= _TABLE_CACHE_MAX:
            _table_cache.pop(next(iter(_table_cache)))
        hit = _table_cache[key] = torch.from_numpy(table).to(device)
    return hit


def bone_table(table, J, device=None, mirror=False):
    """A table of the bone kernels, validated on the host: an integer sequence, numpy array or tensor [J].  The parent table
    (mirror=False): every entry is -1 (no bone) or the index of a joint below the entry's own - the kernels read anything
    else as -1, here it is a ValueError (pafuse_amd.bones.table).  The mirror table: every entry is -1 or a joint of 0 .. J-1.
    -> int32 numpy [J]; with `device` its cached int32 copy there."""
    from . import bones
    import numpy as np
    who = "mirror" if mirror else "parent"

    def check(table, J):
        _need(table.shape == (J,) and table.dtype.kind in "iu", f"bones: {who} must be an integer table [J] = [{J}], got {table.dtype} {table.shape}")
        if mirror:
            _need(bool(((table >= -1) & (table < J)).all()), f"bones: every mirror entry must be -1 or a joint of 0 .. {J - 1}")
        else:
            bones.table(table, J, strict=True)
        return np.ascontiguousarray(table.astype(np.int32))
    return _index_table(f"bones: {who} must be an integer table", table, J, check, device, "bone " + who)


def _bone_operands(who, pose, cov):
    _need(isinstance(pose, torch.Tensor) and pose.dim() == 4 and pose.shape[-1] == 3, f"{who}: pose must be [T,N,J,3]")
    T, N, J = (int(v) for v in pose.shape[:3])
    _need(T > 0 and N > 0 and J > 0, f"{who}: T, N, J > 0")
    _need(J <= 256, f"{who}: J = {J} is more than 256")
    _need(cov is None or (isinstance(cov, torch.Tensor) and tuple(cov.shape) == (T, N, J, 6)), f"{who}: cov must be [T,N,J,6]")
    return T, N, J


def bone_lengths(pose, cov, parent, mirror=None, floor=1e-3, want_dev=False, want_frames=False):
    """pafuse_bone_lengths: pose [T,N,J,3] the finished per-frame pose of a video of N frames, cov [T,N,J,6] the covariance of
    its hypotheses (finish_frames' "cov") or None (zeros), parent [J] the bone table (host integers: -1 or a joint below the
    entry's own; h3wb.bone_tables), mirror [J] the left/right partners or None, floor in metres -> length [T,J]: per bone the
    mean of its per-frame lengths, a frame weighing 1 / (u'E_j u + u'E_p u) - as far as its hypotheses agree ALONG the bone;
    mirror partners pool their frames and get the same bits; NaN where a joint has no bone or no frame takes part
    (pafuse_amd.bones states it).  want_dev / want_frames: -> (length, dev [T,J] the weighted standard deviation of the input's
    bone length, frames [T,J] int32 the frames that took part), in that order, those asked for."""
    lib = _lib.load()
    T, N, J = _bone_operands("bone_lengths", pose, cov)
    _need_floor("bone_lengths", floor)
    par = bone_table(parent, J)                                       # refused on the host, before anything touches the device
    mir = None if mirror is None else bone_table(mirror, J, mirror=True)
    _need_tensors("bone_lengths", [pose] + ([] if cov is None else [cov]), ())
    par = bone_table(par, J, pose.device)
    mir = None if mir is None else bone_table(mir, J, pose.device, mirror=True)
    length = torch.empty((T, J), device=pose.device, dtype=torch.float32)
    dev = torch.empty_like(length) if want_dev else None
    frames = torch.empty((T, J), device=pose.device, dtype=torch.int32) if want_frames else None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(pose.device):
        _lib.check(lib.pafuse_bone_lengths(pose.data_ptr(), ptr(cov), par.data_ptr(), ptr(mir), T, N, J, float(floor), length.data_ptr(),
                                           ptr(dev), ptr(frames), _stream(pose)))
    got = (length,) + ((dev,) if want_dev else ()) + ((frames,) if want_frames else ())
    return got if len(got) > 1 else length


def project_bones(pose, cov, parent, length, iterations=16, snap=True, floor=1e-3, want_code=False, want_resid=False, out=None):
    """pafuse_bone_project: pose [T,N,J,3], cov [T,N,J,6] or None, parent [J] as in bone_lengths, length [T,J] (or [J]: the same
    for every step) the lengths to hold - bone_lengths' or the caller's own, NaN: that bone is left alone - -> [T,N,J,3]: every
    frame moved onto the lengths by `iterations` (0 .. 64) Jacobi sweeps of the covariance-weighted projection - both ends of a
    wrong bone give way by the least Mahalanobis distance - and, with snap, an exact top-down pass behind them
    (pafuse_amd.bones states it).  A joint that is part of no active bone keeps the input's bits; a joint without a bone (the
    root) never moves.  16 sweeps and the 1 mm floor are defaults, not tuned values.  want_code: code [T,N,J] uint8 (1 moved
    with a bone, 0 untouched, 3 untouched although a bone was asked of it); want_resid: resid [T,N,2] the largest |l - L| of
    every frame before, and after on the values returned.  `out`: a [T,N,J,3] tensor to write into that shares no memory
    with pose."""
    lib = _lib.load()
    T, N, J = _bone_operands("project_bones", pose, cov)
    _need(not isinstance(iterations, bool) and isinstance(iterations, int) and 0 <= iterations <= 64,
          f"project_bones: iterations must be an integer in 0 .. 64, got {iterations!r}")
    _need(isinstance(snap, (bool, int)) and snap in (0, 1), f"project_bones: snap must be a bool, got {snap!r}")
    _need_floor("project_bones", floor)
    _need(isinstance(length, torch.Tensor) and tuple(length.shape) in ((T, J), (J,)), f"project_bones: length must be [T,J] = {(T, J)} (or [J]), got "
          f"{tuple(length.shape) if isinstance(length, torch.Tensor) else type(length).__name__}")
    par = bone_table(parent, J)
    if length.dim() == 1:
        length = length.unsqueeze(0).expand(T, J).contiguous()
    if out is None:
        out = torch.empty_like(pose)
    _need(isinstance(out, torch.Tensor) and tuple(out.shape) == (T, N, J, 3), "project_bones: out must be [T,N,J,3]")
    _need_tensors("project_bones", [pose, out, length] + ([] if cov is None else [cov]), ())
    lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
    _need(hi <= pose.data_ptr() or lo >= pose.data_ptr() + pose.numel() * 4, "project_bones: out may not alias pose")
    par = bone_table(par, J, pose.device)
    code = torch.empty((T, N, J), device=pose.device, dtype=torch.uint8) if want_code else None
    resid = torch.empty((T, N, 2), device=pose.device, dtype=torch.float32) if want_resid else None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(pose.device):
        _lib.check(lib.pafuse_bone_project(pose.data_ptr(), ptr(cov), par.data_ptr(), length.data_ptr(), T, N, J, int(iterations), int(snap),
                                           float(floor), out.data_ptr(), ptr(code), ptr(resid), _stream(pose)))
    got = (out,) + ((code,) if want_code else ()) + ((resid,) if want_resid else ())
    return got if len(got) > 1 else out


# ------------------------------------------------------------------ missing 2-D detections, repaired before lifting
REPAIR_OUTPUTS = {"x2d": ((2,), torch.float32), "conf": ((), torch.float32), "status": ((), torch.uint8)}


def repair_anchor_table(anchor, J, device=None):
    """The anchor table of repair_detections, validated on the host: an integer sequence, numpy array or tensor [J], every
    entry negative (the joint hangs on nothing) or the index of a joint whose own entry is negative.  An entry the level rule
    of pafuse_detections_repair would demote silently - out of range, the joint itself, an anchored joint - is a ValueError
    (pafuse_amd.detections.check_anchor).  -> int32 numpy [J]; with `device` its cached int32 copy there."""
    from .detections import check_anchor
    return _index_table("repair_detections: anchor must be an integer table", anchor, J, check_anchor, device, "anchor")


def repair_detections(x2d, conf, anchor=None, radius=13, threshold=0.0, want=("x2d", "conf", "status")):
    """pafuse_detections_repair: x2d [N,J,2] screen-normalised detections, conf [N,J] their confidences, anchor [J] (host
    integers; None: no joint hangs on another), radius 1 .. 64, threshold >= 0 -> dict with the entries named in `want`:
    "x2d" [N,J,2] the detections with every joint that is not observed (conf <= threshold, or not finite) filled along the
    frames from its observed neighbours within `radius` - a joint with an anchor relative to that joint's repaired track -
    "conf" [N,J] the confidences with 0 at every joint that is not observed, "status" [N,J] uint8: 0 observed (the same
    bits), 1 filled (local line), 2 held (one neighbour), 3 unfilled (the input's bits).  pafuse_amd.detections states the
    arithmetic."""
    lib = _lib.load()
    want = tuple(want)
    _need(all(k in REPAIR_OUTPUTS for k in want), f"repair_detections: want holds any of {sorted(REPAIR_OUTPUTS)} - got {want}")
    _need(isinstance(x2d, torch.Tensor) and x2d.dim() == 3 and x2d.shape[-1] == 2, "repair_detections: x2d must be [N,J,2]")
    N, J = int(x2d.shape[0]), int(x2d.shape[1])
    _need(N > 0 and J > 0, "repair_detections: N, J > 0")
    _need(isinstance(conf, torch.Tensor) and tuple(conf.shape) == (N, J), "repair_detections: conf must be [N,J]")
    _need_radius("repair_detections", radius)
    threshold = float(threshold)
    _need(threshold == threshold and 0.0 <= threshold < float("inf"), f"repair_detections: threshold must be finite and >= 0, got {threshold!r}")
    table = None if anchor is None else repair_anchor_table(anchor, J)      # refused here, before anything touches the device
    _need_tensors("repair_detections", [x2d, conf], ())
    dev = x2d.device
    if table is not None:
        table = repair_anchor_table(table, J, dev)
    made = ("x2d", "status") + (("conf",) if "conf" in want else ())     # the kernel needs out and status whatever is wanted
    out = {k: torch.empty((N, J, *REPAIR_OUTPUTS[k][0]), device=dev, dtype=REPAIR_OUTPUTS[k][1]) for k in made}
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_detections_repair(x2d.data_ptr(), conf.data_ptr(), None if table is None else table.data_ptr(), N, J,
                                                int(radius), threshold, out["x2d"].data_ptr(),
                                                out["conf"].data_ptr() if "conf" in out else None, out["status"].data_ptr(),
                                                _stream(x2d)))
    return {k: out[k] for k in want}


# ------------------------------------------------------------------ observed 2-D detections, screened before the repair
SCREEN_OUTPUTS = {"x2d": ("NJ", (2,), torch.float32), "conf": ("NJ", (), torch.float32), "status": ("NJ", (), torch.uint8),
                  "resid": ("NJ", (), torch.float32), "scale": ("J", (), torch.float32)}


def screen_mirror_table(mirror, J, device=None):
    """The mirror table of screen_detections, validated on the host: an integer sequence, numpy array or tensor [J], every
    entry negative (no partner) or the index of the joint whose own entry points back.  An entry the partner rule of
    pafuse_detections_screen would drop silently - out of range, the joint itself, a joint that does not point back - is a
    ValueError (pafuse_amd.detscreen.check_mirror).  -> int32 numpy [J]; with `device` its cached int32 copy there."""
    from .detscreen import check_mirror
    return _index_table("screen_detections: mirror must be an integer table", mirror, J, check_mirror, device, "mirror")


def _need_count(who, name, value, lo, hi):
    _need(not isinstance(value, bool) and isinstance(value, int) and lo <= value <= hi,
          f"{who}: {name} must be an integer in {lo} .. {hi}, got {value!r}")


def _need_positive(who, name, value):
    _need(not isinstance(value, bool) and isinstance(value, (int, float)) and 0.0 < float(value) < float("inf"),
          f"{who}: {name} must be finite and > 0, got {value!r}")


def screen_detections(x2d, conf, mirror=None, radius=13, gate=4.0, floor=0.005, passes=3, support=3, threshold=0.0,
                      want=("x2d", "conf", "status", "resid", "scale")):
    """pafuse_detections_screen: x2d [N,J,2] screen-normalised detections, conf [N,J] their confidences, mirror [J] (host
    integers: every joint's mirror joint, negative for none; None: no pairs), radius 1 .. 64 frames, gate > 0 (scales), floor
    > 0 (the smallest scale, screen units), passes 1 .. 8, support 2 .. 129 (fewest accepted neighbours for a prediction),
    threshold >= 0 as in repair_detections -> dict with the entries named in `want`: "x2d" [N,J,2] and "conf" [N,J] - a
    rejected detection with confidence 0, a swapped pair exchanged, everything else the same bits - "status" [N,J] uint8: 0
    accepted, 1 rejected, 2 swapped, 3 not observed; "resid" [N,J] the distance of every detection from the leave-one-out
    line through its accepted neighbours (NaN where there is none); "scale" [J] the gate of every joint.
    pafuse_amd.detscreen states the arithmetic.  gate, floor, passes and support are defaults, not tuned values."""
    lib = _lib.load()
    who = "screen_detections"
    want = tuple(want)
    _need(all(k in SCREEN_OUTPUTS for k in want), f"{who}: want holds any of {sorted(SCREEN_OUTPUTS)} - got {want}")
    _need(isinstance(x2d, torch.Tensor) and x2d.dim() == 3 and x2d.shape[-1] == 2, f"{who}: x2d must be [N,J,2]")
    N, J = int(x2d.shape[0]), int(x2d.shape[1])
    _need(N > 0 and J > 0, f"{who}: N, J > 0")
    _need(isinstance(conf, torch.Tensor) and tuple(conf.shape) == (N, J), f"{who}: conf must be [N,J]")
    _need_radius(who, radius)
    _need_count(who, "passes", passes, 1, 8)
    _need_count(who, "support", support, 2, 129)
    _need_positive(who, "gate", gate)
    _need_positive(who, "floor", floor)
    threshold = float(threshold)
    _need(threshold == threshold and 0.0 <= threshold < float("inf"), f"{who}: threshold must be finite and >= 0, got {threshold!r}")
    table = None if mirror is None else screen_mirror_table(mirror, J)      # refused here, before anything touches the device
    _need_tensors(who, [x2d, conf], ())
    dev = x2d.device
    if table is not None:
        table = screen_mirror_table(table, J, dev)
    made = ("x2d", "conf", "status") + tuple(k for k in ("resid", "scale") if k in want)   # the finish writes the first three
    out = {k: torch.empty(((N, J) if SCREEN_OUTPUTS[k][0] == "NJ" else (J,)) + SCREEN_OUTPUTS[k][1], device=dev, dtype=SCREEN_OUTPUTS[k][2])
           for k in made}
    need = lib.pafuse_detections_screen_workspace_bytes(N, J)
    work = _lib.workspace(need, dev, "screen_detections", torch.float64)
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_detections_screen(x2d.data_ptr(), conf.data_ptr(), None if table is None else table.data_ptr(), N, J,
                                                int(radius), int(passes), int(support), threshold, float(gate), float(floor),
                                                ptr("x2d"), ptr("conf"), ptr("status"), ptr("resid"), ptr("scale"),
                                                work.data_ptr(), need, _stream(x2d)))
    return {k: out[k] for k in want}


# ------------------------------------------------------------------ people followed through a video, in front of all of it
TRACK_OUTPUTS = ("x2d", "conf", "assign", "score", "frames", "gain", "size")


def tracks_views(work, N, K, G):
    """the float64 workspace of pafuse_tracks_links -> (gain [N,G,K,K], size [N,K]): views, in the layout of include/pafuse_hip.h"""
    n = N * G * K * K
    return work[:n].view(N, G, K, K), work[n:n + N * K].view(N, K)


def _track_half(lib, x2d, conf, N, K, J, G, M, support, threshold, gate, skip, min_frames, seed):
    """links + path on one video -> (assign [M,N] int32, score [M] float64, frames [M] int32, the workspace)"""
    dev = x2d.device
    need = lib.pafuse_tracks_workspace_bytes(N, K, J, G)
    _need(need > 0, "track_people: sizes out of range")
    work = _lib.workspace(need, dev, "track_people", torch.float64)
    assign = torch.empty(M, N, device=dev, dtype=torch.int32)
    score = torch.empty(M, device=dev, dtype=torch.float64)
    frames = torch.empty(M, device=dev, dtype=torch.int32)
    sn, sk = (-1, -1) if seed is None else seed
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_tracks_links(x2d.data_ptr(), conf.data_ptr(), N, K, J, G, support, threshold, gate, skip,
                                           work.data_ptr(), need, _stream(x2d)))
        _lib.check(lib.pafuse_tracks_path(None, None, N, K, G, M, min_frames, sn, sk, assign.data_ptr(), score.data_ptr(),
                                          frames.data_ptr(), work.data_ptr(), need, _stream(x2d)))
    return assign, score, frames, work


def gather_tracks(x2d, conf, assign):
    """pafuse_tracks_gather: x2d [N,K,J,2], conf [N,K,J], assign [M,N] int32 -> (x2d [M,N,J,2], conf [M,N,J]): the bits of the
    chosen candidates, zeros with confidence 0 where assign is -1."""
    lib = _lib.load()
    who = "gather_tracks"
    _need(isinstance(x2d, torch.Tensor) and x2d.dim() == 4 and x2d.shape[-1] == 2, f"{who}: x2d must be [N,K,J,2]")
    N, K, J = (int(v) for v in x2d.shape[:3])
    _need(N > 0 and J > 0 and 1 <= K <= 64, f"{who}: N, J > 0 and K in 1 .. 64")
    _need(isinstance(conf, torch.Tensor) and tuple(conf.shape) == (N, K, J), f"{who}: conf must be [N,K,J]")
    _need(isinstance(assign, torch.Tensor) and assign.dim() == 2 and assign.shape[1] == N and 1 <= assign.shape[0] <= 64,
          f"{who}: assign must be [M,N], M in 1 .. 64")
    _need_tensors(who, [x2d, conf], [assign])
    M = int(assign.shape[0])
    out = torch.empty(M, N, J, 2, device=x2d.device, dtype=torch.float32)
    cout = torch.empty(M, N, J, device=x2d.device, dtype=torch.float32)
    with torch.cuda.device(x2d.device):
        _lib.check(lib.pafuse_tracks_gather(x2d.data_ptr(), conf.data_ptr(), assign.data_ptr(), N, K, J, M, out.data_ptr(),
                                            cout.data_ptr(), _stream(x2d)))
    return out, cout


def track_people(x2d, conf, tracks=1, seed=None, gate=0.5, skip=0.05, max_gap=4, support=5, min_frames=5, threshold=0.0,
                 want=("x2d", "conf", "assign", "score", "frames")):
    """pafuse_tracks_links + pafuse_tracks_path + pafuse_tracks_gather: x2d [N,K,J,2] screen-normalised candidate detections, K
    per frame in no stable order (an all-zero slot is nobody; K <= 64: pass the largest number of people in any frame), conf
    [N,K,J]; tracks 1 .. 64 people to follow, best first; seed (frame, candidate) or None: follow that detection's person
    (tracks = 1); gate > 0: the farthest a person may move between linked frames, in units of their own size; skip >= 0: what
    every frame a link jumps over costs; max_gap 1 .. 8: the longest link, in frames; support: fewest observed (common) joints
    of a candidate (a link); min_frames: the shortest track kept; threshold >= 0 as in repair_detections -> dict with the
    entries named in `want`: "x2d" [M,N,J,2] and "conf" [M,N,J] the per-person videos (a frame without the person is zeros
    with confidence 0, which repair_detections fills), "assign" [M,N] int32 the candidate followed (-1: nobody), "score" [M]
    float64 (NaN: no such track), "frames" [M] int32, "gain" [N,G,K,K] float64 and "size" [N,K] float64 (NaN: absent).
    pafuse_amd.tracks states the arithmetic.  The gain table takes N*G*K*K*8 bytes.  With a seed the half before it is a
    second run on the frame-reversed video.  gate, skip, max_gap, support and min_frames are defaults, not tuned values."""
    from . import tracks as statement
    lib = _lib.load()
    who = "track_people"
    want = tuple(want)
    _need(all(k in TRACK_OUTPUTS for k in want), f"{who}: want holds any of {sorted(TRACK_OUTPUTS)} - got {want}")
    _need(isinstance(x2d, torch.Tensor) and x2d.dim() == 4 and x2d.shape[-1] == 2, f"{who}: x2d must be [N,K,J,2]")
    N, K, J = (int(v) for v in x2d.shape[:3])
    _need(N > 0 and J > 0, f"{who}: N, J > 0")
    _need(isinstance(conf, torch.Tensor) and tuple(conf.shape) == (N, K, J), f"{who}: conf must be [N,K,J]")
    for name, v in (("tracks", tracks), ("max_gap", max_gap), ("support", support), ("min_frames", min_frames)):
        _need(not isinstance(v, bool) and isinstance(v, int), f"{who}: {name} must be an integer, got {v!r}")
    gate, skip, threshold = float(gate), float(skip), float(threshold)
    M, G, support, min_frames, seed = statement.check(N, K, tracks, seed, gate, skip, max_gap, support, min_frames, threshold)
    _need_tensors(who, [x2d, conf], ())
    args = (lib, x2d, conf, N, K, J, G, M, support, threshold, gate, skip)
    if seed is None:
        assign, score, frames, work = _track_half(*args, min_frames, None)
    else:   # the half from the seed on, and the half before it on the flipped video; min_frames holds for their union
        assign, score, frames, work = _track_half(*args, 1, seed)
        back = _track_half(lib, x2d.flip(0).contiguous(), conf.flip(0).contiguous(), *args[3:], 1, (N - 1 - seed[0], seed[1]))
        assign = torch.where(assign >= 0, assign, back[0].flip(1)).contiguous()
        count = frames + back[2] - 1
        keep = (frames >= 1) & (back[2] >= 1) & (count >= min_frames)
        assign = torch.where(keep[:, None], assign, torch.full_like(assign, -1))
        score = torch.where(keep, score + back[1], torch.full_like(score, float("nan")))
        frames = torch.where(keep, count, torch.zeros_like(count)).to(torch.int32)
    out = {"assign": assign, "score": score, "frames": frames}
    if "x2d" in want or "conf" in want:
        out["x2d"], out["conf"] = gather_tracks(x2d, conf, assign)
    if "gain" in want or "size" in want:
        out["gain"], out["size"] = tracks_views(work, N, K, G)
    return {k: out[k] for k in want}


# ------------------------------------------------------------------ the focal length, estimated from pose and detections
FOCAL_OUTPUTS =("focal", "r2", "frames", "cam")


def focal_sums(pose, x2d, cam, conf=None):
    """pafuse_frames_focal_sums: pose [T,N,J,3], x2d [N,J,2], cam [>= 4] and conf [N,J] (None: every weight 1) as fit_trajectory
    takes them - of cam only cx, cy and the ratio cam[1]/cam[0] are read -> state [T,N,4] float64: (K, H, G, 1.0) per (t, frame),
    zeros for a frame that takes no part (pafuse_amd.focal states the arithmetic).  States of several videos of one camera
    concatenate along N."""
    lib = _lib.load()
    T, N, J = _frame_pose_operands("focal_sums", pose, x2d, cam, conf)
    out = torch.empty(T, N, 4, device=pose.device, dtype=torch.float64)
    with torch.cuda.device(pose.device):
        _lib.check(lib.pafuse_frames_focal_sums(pose.data_ptr(), x2d.data_ptr(), None if conf is None else conf.data_ptr(),
                                                cam.data_ptr(), T, N, J, out.data_ptr(), _stream(pose)))
    return out


def focal_solve(state, cam, want=FOCAL_OUTPUTS):
    """pafuse_focal_solve: state [T,N,4] float64 (focal_sums; several concatenated along N), cam [4 .. 9] the intrinsics whose
    principal point, aspect and distortion terms are kept -> dict with the entries named in `want`: "focal" [T] (screen-normalised
    units, NaN without an estimate), "r2" [T] the fraction of the perspective signal the estimate explains, "frames" [T] int32
    the frames it rests on, "cam" [T,len(cam)] the intrinsics with the estimate in the place of fx, fy (NaN without one)."""
    lib = _lib.load()
    want = tuple(want)
    _need(all(k in FOCAL_OUTPUTS for k in want) and "focal" in want, f'focal_solve: want holds "focal" and any of r2, frames, cam - got {want}')
    _need(isinstance(state, torch.Tensor) and state.dim() == 3 and state.shape[-1] == 4 and state.dtype == torch.float64
          and state.is_cuda and state.is_contiguous(), "focal_solve: state must be a contiguous float64 [T,N,4] tensor on a HIP device")
    T, N = int(state.shape[0]), int(state.shape[1])
    _need(T > 0 and N > 0, "focal_solve: T, N > 0")
    _need(cam is not None and cam.dim() == 1 and 4 <= cam.numel() <= 9, "focal_solve: cam must be [4 .. 9]")
    _need_tensors("focal_solve", [cam], ())
    _need(cam.device == state.device, "focal_solve: cam on the device of the state")
    dev, L = state.device, int(cam.numel())
    shapes = {"focal": ((T,), torch.float32), "r2": ((T,), torch.float32), "frames": ((T,), torch.int32), "cam": ((T, L), torch.float32)}
    out = {k: torch.empty(shapes[k][0], device=dev, dtype=shapes[k][1]) for k in want}
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_focal_solve(state.data_ptr(), T, N, cam.data_ptr(), L, ptr("focal"), ptr("r2"), ptr("frames"),
                                          ptr("cam"), _stream(state)))
    return out


def estimate_focal(pose, x2d, cam, conf=None, want=FOCAL_OUTPUTS):
    """focal_sums and focal_solve in one call, for one video: -> the dict of focal_solve."""
    return focal_solve(focal_sums(pose, x2d, cam, conf=conf), cam, want=want)


# ------------------------------------------------------------------ which way is up: the ground plane from the foot contacts
GROUND_SLOTS, GROUND_MAX_POINTS = 14, 16
GROUND_SOLVE_OUTPUTS = ("plane", "scale", "up", "camera_height", "ground_rms", "ground_eig", "ground_points", "ground_code")
GROUND_OUTPUTS = GROUND_SOLVE_OUTPUTS + ("foot", "foot_speed", "contact", "pose_world", "traj_world")


def ground_points(points, J, device=None):
    """The foot points of the ground estimate, validated on the host: an integer sequence, numpy array or tensor of 1 .. 16
    joints, each in [0, J) (h3wb.foot_points gives the six toe and heel points) -> int32 numpy [K]; with `device` its cached
    int32 copy there."""
    import numpy as np

    def check(points, J):
        _need(points.ndim == 1 and points.dtype.kind in "iu" and 1 <= points.size <= GROUND_MAX_POINTS,
              f"ground: points must be 1 .. {GROUND_MAX_POINTS} integers, got {points.dtype} {points.shape}")
        _need(bool(((points >= 0) & (points < J)).all()), f"ground: every point must be a joint of 0 .. {J - 1}, got {points.tolist()}")
        return np.ascontiguousarray(points.astype(np.int32))
    return _index_table("ground: points must be integers", points, J, check, device, "ground")


def _need_metres(who, name, value):
    ok = not isinstance(value, bool) and isinstance(value, (int, float)) and math.isfinite(float(value)) and float(value) > 0.0
    _need(ok, f"{who}: {name} must be a number that is finite and > 0, got {value!r}")
    return float(value)


def _ground_pose_operands(who, pose, traj):
    _need(isinstance(pose, torch.Tensor) and pose.dim() == 4 and pose.shape[-1] == 3, f"{who}: pose must be [T,N,J,3]")
    T, N, J = (int(v) for v in pose.shape[:3])
    _need(T > 0 and N > 0 and J > 0, f"{who}: T, N, J > 0")
    _need(isinstance(traj, torch.Tensor) and tuple(traj.shape) == (T, N, 3), f"{who}: traj must be [T,N,3] = {(T, N, 3)}")
    _need_tensors(who, [pose, traj], ())
    return T, N, J


def _need_plane(who, plane, scale, T, dev):
    _need(isinstance(plane, torch.Tensor) and tuple(plane.shape) == (T, 4) and plane.dtype == torch.float64 and plane.is_cuda
          and plane.device == dev and plane.is_contiguous(), f"{who}: plane must be a contiguous float64 [T,4] = {(T, 4)} tensor on {dev}")
    _need(scale is None or (isinstance(scale, torch.Tensor) and tuple(scale.shape) == (T,) and scale.dtype == torch.float64
                            and scale.device == dev and scale.is_contiguous()), f"{who}: scale must be a contiguous float64 [T] tensor on {dev}")


def foot_contacts(pose, traj, points, radius=3, speed=0.015, want_speed=True):
    """pafuse_foot_contacts: pose [T,N,J,3] root-relative, traj [T,N,3] the camera-space root (NaN: none), points the foot
    joints (ground_points), radius 1 .. 64 frames, speed in metres per FRAME (finite, > 0) -> dict "foot" [T,N,K,3] the foot
    points in camera space on their local line (NaN: no line through 3 frames), "contact" [T,N,K] the weight of a foot that
    is not moving, (1 - (v/speed)^2)^2 below `speed` and 0 from there, and (want_speed) "foot_speed" [T,N,K] v in metres per
    frame.  pafuse_amd.ground states the arithmetic.  0.015 and 3 are defaults, not tuned values."""
    lib = _lib.load()
    T, N, J = _ground_pose_operands("foot_contacts", pose, traj)
    _need_radius("foot_contacts", radius)
    speed = _need_metres("foot_contacts", "speed", speed)
    pts = ground_points(points, J, pose.device)
    K, dev = int(pts.numel()), pose.device
    out = {"foot": torch.empty(T, N, K, 3, device=dev), "contact": torch.empty(T, N, K, device=dev)}
    if want_speed:
        out["foot_speed"] = torch.empty(T, N, K, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_foot_contacts(pose.data_ptr(), traj.data_ptr(), pts.data_ptr(), T, N, J, K, int(radius), speed,
                                            out["foot"].data_ptr(), out["foot_speed"].data_ptr() if want_speed else None,
                                            out["contact"].data_ptr(), _stream(pose)))
    return out


def ground_sums(foot, contact, traj, plane=None, scale=None, gate=2.5, out=None):
    """pafuse_ground_sums: foot [T,N,K,3], contact [T,N,K] (foot_contacts), traj [T,N,3]; plane [T,4] and scale [T] float64 of
    the previous pass's ground_solve (read on the device) or both None: the first pass -> state [T,N,14] float64 (`out`: a
    tensor of that shape to write into).  States of several videos of one scene concatenate along N."""
    lib = _lib.load()
    _need(isinstance(foot, torch.Tensor) and foot.dim() == 4 and foot.shape[-1] == 3, "ground_sums: foot must be [T,N,K,3]")
    T, N, K = (int(v) for v in foot.shape[:3])
    _need(T > 0 and N > 0 and 1 <= K <= GROUND_MAX_POINTS, f"ground_sums: T, N > 0 and K in 1 .. {GROUND_MAX_POINTS}")
    _need(isinstance(contact, torch.Tensor) and tuple(contact.shape) == (T, N, K) and isinstance(traj, torch.Tensor)
          and tuple(traj.shape) == (T, N, 3), "ground_sums: contact [T,N,K] and traj [T,N,3] must match foot [T,N,K,3]")
    _need((plane is None) == (scale is None), "ground_sums: plane and scale come together (or neither: the first pass)")
    _need_tensors("ground_sums", [foot, contact, traj], ())
    gate = _need_metres("ground_sums", "gate", gate)
    dev = foot.device
    if plane is not None:
        _need_plane("ground_sums", plane, scale, T, dev)
    if out is None:
        out = torch.empty(T, N, GROUND_SLOTS, device=dev, dtype=torch.float64)
    _need(tuple(out.shape) == (T, N, GROUND_SLOTS) and out.dtype == torch.float64 and out.device == dev and out.is_contiguous(),
          f"ground_sums: out must be a contiguous float64 [T,N,{GROUND_SLOTS}] tensor on {dev}")
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_ground_sums(foot.data_ptr(), contact.data_ptr(), traj.data_ptr(), None if plane is None else plane.data_ptr(),
                                          None if scale is None else scale.data_ptr(), T, N, K, gate, out.data_ptr(), _stream(foot)))
    return out


def ground_solve(state, floor=0.005, spread=0.03, want=GROUND_SOLVE_OUTPUTS):
    """pafuse_ground_solve: state [T,N,14] float64 (ground_sums; several concatenated along N) -> dict with "plane" [T,4] float64
    (the unit normal pointing up and d: a point p is n.p - d above the ground), "scale" [T] float64 (what the next pass's
    ground_sums reads) and those of "up" [T,3], "camera_height" [T] (= -d), "ground_rms" [T], "ground_eig" [T,3] (ascending),
    "ground_points" [T] int32 and "ground_code" [T] uint8 (1 plane, 2 line: a person standing, 3 body: the lifted body's own up,
    0 none: NaN everywhere) named in `want`.  floor and spread in metres; 0.005 and 0.03 are defaults, not tuned values."""
    lib = _lib.load()
    want = tuple(want)
    _need(all(k in GROUND_SOLVE_OUTPUTS for k in want), f"ground_solve: want holds any of {GROUND_SOLVE_OUTPUTS} - got {want}")
    _need(isinstance(state, torch.Tensor) and state.dim() == 3 and state.shape[-1] == GROUND_SLOTS and state.dtype == torch.float64
          and state.is_cuda and state.is_contiguous(), f"ground_solve: state must be a contiguous float64 [T,N,{GROUND_SLOTS}] tensor on a HIP device")
    T, N = int(state.shape[0]), int(state.shape[1])
    _need(T > 0 and N > 0, "ground_solve: T, N > 0")
    floor, spread = _need_metres("ground_solve", "floor", floor), _need_metres("ground_solve", "spread", spread)
    dev = state.device
    f32, f64 = torch.float32, torch.float64
    shapes = {"plane": ((T, 4), f64), "scale": ((T,), f64), "up": ((T, 3), f32), "camera_height": ((T,), f32), "ground_rms": ((T,), f32),
              "ground_eig": ((T, 3), f32), "ground_points": ((T,), torch.int32), "ground_code": ((T,), torch.uint8)}
    out = {k: torch.empty(shapes[k][0], device=dev, dtype=shapes[k][1]) for k in GROUND_SOLVE_OUTPUTS if k in want or k in ("plane", "scale")}
    ptr = lambda k: out[k].data_ptr() if k in out else None
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_ground_solve(state.data_ptr(), T, N, floor, spread, ptr("plane"), ptr("scale"), ptr("up"), ptr("camera_height"),
                                           ptr("ground_rms"), ptr("ground_eig"), ptr("ground_points"), ptr("ground_code"), _stream(state)))
    return {k: v for k, v in out.items() if k in want}


def frames_to_world(pose, traj, plane, want_traj=True):
    """pafuse_frames_to_world: pose [T,N,J,3] root-relative, traj [T,N,3], plane [T,4] float64 (ground_solve) ->
    (pose_world [T,N,J,3], traj_world [T,N,3] or None): world space with z up and the ground at z = 0, x the camera's right
    projected onto the ground.  The height of a joint above the ground is its third component.  NaN in gives NaN out."""
    lib = _lib.load()
    T, N, J = _ground_pose_operands("frames_to_world", pose, traj)
    _need_plane("frames_to_world", plane, None, T, pose.device)
    pose_world = torch.empty_like(pose)
    traj_world = torch.empty_like(traj) if want_traj else None
    with torch.cuda.device(pose.device):
        _lib.check(lib.pafuse_frames_to_world(pose.data_ptr(), traj.data_ptr(), plane.data_ptr(), T, N, J, pose_world.data_ptr(),
                                              None if traj_world is None else traj_world.data_ptr(), _stream(pose)))
    return pose_world, traj_world


def estimate_ground(pose, traj, points, radius=3, speed=0.015, passes=3, gate=2.5, floor=0.005, spread=0.03, want=GROUND_OUTPUTS):
    """The chain on one stream, nothing crossing to the host: foot_contacts, `passes` (1 .. 8) times ground_sums + ground_solve -
    every later pass re-weighting the contacts with the plane of the one before, read on the device - and frames_to_world
    when "pose_world" or "traj_world" is wanted: 1 + 2*passes + 1 launches.  -> dict with the entries named in `want`
    (GROUND_OUTPUTS).  One plane per step t for the whole video.  Every default is a default, not a tuned value."""
    want = tuple(want)
    _need(all(k in GROUND_OUTPUTS for k in want), f"estimate_ground: want holds any of {GROUND_OUTPUTS} - got {want}")
    _need(not isinstance(passes, bool) and int(passes) == passes and 1 <= int(passes) <= 8, f"estimate_ground: passes must be an integer in 1 .. 8, got {passes!r}")
    feet = foot_contacts(pose, traj, points, radius=radius, speed=speed, want_speed="foot_speed" in want)
    state, sol = None, {"plane": None, "scale": None}
    for i in range(int(passes)):
        last = i == int(passes) - 1
        state = ground_sums(feet["foot"], feet["contact"], traj, sol["plane"], sol["scale"], gate=gate, out=state)
        sol = ground_solve(state, floor=floor, spread=spread, want=GROUND_SOLVE_OUTPUTS if last else ("plane", "scale"))
    out = {**sol, **feet}
    if "pose_world" in want or "traj_world" in want:
        out["pose_world"], out["traj_world"] = frames_to_world(pose, traj, sol["plane"], want_traj="traj_world" in want)
    return {k: out[k] for k in want}


# ------------------------------------------------------------------ the per-frame pose scored against ground truth
FRAME_ERROR_SLOTS = ("mpjpe", "mpjve", "accel", "root", "root_vel", "abs_mpjpe")   # then one slot per part (pafuse_amd.framemetrics)


def frame_errors(pose, gt, pbroot, part, num_parts, traj=None, gt_root=None, per_frame=False):
    """pafuse_frame_errors + pafuse_frame_errors_reduce: pose [T,N,J,3] the per-frame whole-body, root-relative pose (NaN: no
    pose), gt [N,J,3] likewise, pbroot / part int32 [J] (the root joint of every joint's part, the part's number), num_parts
    1 .. 4, traj [T,N,3] with gt_root [N,3] (the camera-space root; both or neither) -> {"sums": [T,K] float64, "counts": [T,K]
    int64}, K = 6 + num_parts in the order of FRAME_ERROR_SLOTS then the parts: the sums over the frames of the position,
    velocity, acceleration, root, root-velocity, camera-space and part-based errors and of the joints (frames) that took part.
    A metric is sums / counts, in metres.  per_frame=True: also "err" [T,N,K] float64 and "cnt" [T,N,K] int32, the same per
    frame.  pafuse_amd.framemetrics states the arithmetic (fp64)."""
    lib = _lib.load()
    _need(isinstance(pose, torch.Tensor) and pose.dim() == 4 and pose.shape[-1] == 3, "frame_errors: pose must be [T,N,J,3]")
    T, N, J = (int(v) for v in pose.shape[:3])
    _need(T > 0 and N > 0 and J > 0, "frame_errors: T, N, J > 0")
    _need(not isinstance(num_parts, bool) and int(num_parts) == num_parts and 1 <= int(num_parts) <= _lib.MAX_PARTS,
          f"frame_errors: num_parts must be an integer in 1 .. {_lib.MAX_PARTS}, got {num_parts!r}")
    _need((traj is None) == (gt_root is None), "frame_errors: traj and gt_root come together (or neither)")
    _need(isinstance(gt, torch.Tensor) and tuple(gt.shape) == (N, J, 3) and tuple(pbroot.shape) == (J,) and tuple(part.shape) == (J,)
          and (traj is None or (tuple(traj.shape) == (T, N, 3) and tuple(gt_root.shape) == (N, 3))),
          "frame_errors: gt [N,J,3], pbroot [J], part [J], traj [T,N,3] and gt_root [N,3] must match pose [T,N,J,3]")
    _need_tensors("frame_errors", [pose, gt] + ([] if traj is None else [traj, gt_root]), (pbroot, part))
    dev, K = pose.device, 6 + int(num_parts)
    out = {"err": torch.empty(T, N, K, device=dev, dtype=torch.float64), "cnt": torch.empty(T, N, K, device=dev, dtype=torch.int32),
           "sums": torch.empty(T, K, device=dev, dtype=torch.float64), "counts": torch.empty(T, K, device=dev, dtype=torch.int64)}
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_frame_errors(pose.data_ptr(), gt.data_ptr(), None if traj is None else traj.data_ptr(),
                                           None if traj is None else gt_root.data_ptr(), pbroot.data_ptr(), part.data_ptr(),
                                           int(num_parts), T, N, J, out["err"].data_ptr(), out["cnt"].data_ptr(), _stream(pose)))
        _lib.check(lib.pafuse_frame_errors_reduce(out["err"].data_ptr(), out["cnt"].data_ptr(), T, N, K, out["sums"].data_ptr(),
                                                  out["counts"].data_ptr(), _stream(pose)))
    return out if per_frame else {k: out[k] for k in ("sums", "counts")}


# ------------------------------------------------------------------------------ Protocol #2 from partial states
PROCRUSTES_HEAD_BYTES_PER_ELEMENT = 16   # float jbest, e2, sel + int32 idx per (b, t, f, j)


def procrustes_partials_bytes(B, T, P_r, F, J):
    """Bytes of the state pafuse_procrustes_partials writes for a shard of P_r hypotheses (the formula of
    pafuse_procrustes_partials_bytes, restated so that sizes can be planned without the library): the head, independent
    of P_r, then 8 bytes per local hypothesis and step."""
    return PROCRUSTES_HEAD_BYTES_PER_ELEMENT * B * T * F * J + 8 * P_r * T


def procrustes_partial_views(state, B, T, P_r, F, J):
    """Typed views of a flat Protocol #2 state (1-D float64 tensor of procrustes_partials_bytes / 8 elements, or longer: a
    padded one): jbest / e2 / sel [B,T,F,J] f32, idx [B,T,F,J] i32, psum [P_r,T] f64."""
    n = B * T * F * J
    _need(state.dim() == 1 and state.dtype == torch.float64 and state.is_contiguous()
          and state.numel() * 8 >= procrustes_partials_bytes(B, T, P_r, F, J), "procrustes_partial_views: not a state of these sizes")
    f32 = state[:2 * n].view(torch.float32)
    return {"jbest": f32[:n].view(B, T, F, J), "e2": f32[n:2 * n].view(B, T, F, J), "sel": f32[2 * n:3 * n].view(B, T, F, J),
            "idx": f32[3 * n:].view(torch.int32).view(B, T, F, J), "psum": state[2 * n:2 * n + P_r * T].view(P_r, T)}


def procrustes_partials(pred, gt, x2d, traj, cam, conn, h0, out=None):
    """One shard's Protocol #2 state (pafuse_procrustes_partials): pred [B,T,P_r,F,J,3] the LOCAL hypotheses
    [h0, h0 + P_r) of the run, gt [B,F,J,3], x2d [B,F,J,2], traj [B,F,3] (or [B,F,1,3]), cam [9], conn int32 [J] -> the flat
    state, a 1-D float64 tensor (procrustes_partial_views names its pieces).  `out`: a float64 buffer at least that long
    to write into; the result is then `out` itself.  fp32 operands on one HIP device, contiguous.  J <= 256."""
    lib = _lib.load()
    B, T, P_r, F, J = _need_pred("procrustes_partials", pred)
    _need(tuple(gt.shape) == (B, F, J, 3) and tuple(x2d.shape) == (B, F, J, 2) and traj.numel() == B * F * 3
          and cam.numel() == 9 and conn.numel() == J, "procrustes_partials: operands do not match pred")
    _need(T > 0 and F > 0 and J > 0 and int(h0) >= 0, "procrustes_partials: T, F, J > 0 and h0 >= 0")
    _need_tensors("procrustes_partials", (pred, gt, x2d, traj, cam), (conn,))
    dev = pred.device
    out = _state_out("procrustes_partials", out, procrustes_partials_bytes(B, T, P_r, F, J), dev)
    wbytes = int(lib.pafuse_procrustes_partials_workspace_bytes(B, T, P_r, F, J))
    work = _lib.workspace(wbytes, dev, "procrustes_partials", torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_procrustes_partials(
            _data(pred), _data(gt), _data(x2d), _data(traj), _data(cam), _data(conn), B, T, P_r, F, J, int(h0),
            _data(out), out.numel() * 8, work.data_ptr(), work.numel() * 8, _stream(pred)))
    return out


def combine_procrustes(states, shape, num_proposals, sums=None, gt=None, conn=None, merged=None,
                       want=("jbest", "pagg", "jagg", "pick")):
    """pafuse_procrustes_combine: `states` [W, L] float64 (W flat Protocol #2 states of the same (B,T,F,J) = `shape`, one per
    row, in ascending-h0 order; rows may carry their psum tail and padding, which is not read) -> dict with the entries
    named in `want`: "jbest", "pagg", "jagg" [B,T,F,J] fp32 and "pick" [B,T,F,J] int32 (what procrustes_errors gives for all
    hypotheses).  "pagg" aligns the mean pose and needs `sums` [W, >= 3*B*T*F*J] float64 - rows that BEGIN with the
    double sum[n][3] of the same shards, i.e. the Protocol #1 states (hypothesis_partials) or pose states (pose_partials) as
    they are - plus gt [B,F,J,3] and conn int32 [J]; the sums are added in row order and divided by `num_proposals`, the
    TOTAL hypothesis count.  `merged`: a float64 buffer that receives the head of the union's state (2*B*T*F*J
    elements); of the operands it may only be states[0] (a running state)."""
    lib = _lib.load()
    B, T, F, J = (int(v) for v in shape)
    n = B * T * F * J
    want = tuple(want)
    _need(all(k in ("jbest", "pagg", "jagg", "pick") for k in want), f"combine_procrustes: want holds jbest, pagg, jagg, pick - got {want}")
    _need_rows(states, 2 * n, "combine_procrustes: states must be [W, >= 2*B*T*F*J] float64 rows (a column slice of a wider "
               "buffer is fine)", strided=True)
    _need(T > 0 and F > 0 and 0 < J <= 256 and B >= 0, "combine_procrustes: bad shape (J <= 256)")
    _need(want or merged is not None, "combine_procrustes: nothing to compute")
    _need(int(num_proposals) >= 1, "combine_procrustes: num_proposals >= 1")
    dev = states.device
    W = states.shape[0]
    row = lambda t: t.stride(0) if W > 1 else t.shape[1]   # elements between rows
    if "pagg" in want:
        _need(sums is not None and gt is not None and conn is not None, "combine_procrustes: pagg needs sums, gt and conn")
        _need_rows(sums, 3 * n, "combine_procrustes: sums must be [W, >= 3*B*T*F*J] float64 rows on the device of the states",
                   strided=True, like=states)
        _need(tuple(gt.shape) == (B, F, J, 3) and conn.numel() == J and all(t.is_cuda and t.device == dev and t.is_contiguous()
              for t in (gt, conn)) and gt.dtype == torch.float32 and conn.dtype == torch.int32,
              "combine_procrustes: gt [B,F,J,3] f32, conn [J] int32, contiguous on the device of the states")
    if merged is not None:
        _need_merged("combine_procrustes", merged, states, 2 * n, "2*B*T*F*J", (W - 1) * row(states) + 2 * n, "first")
    out = {k: torch.empty(B, T, F, J, device=dev, dtype=torch.int32 if k == "pick" else torch.float32) for k in want}
    if n == 0:
        return out
    ptr = lambda k: out[k].data_ptr() if k in out else None
    pagg = "pagg" in want
    with torch.cuda.device(dev):
        _lib.check(lib.pafuse_procrustes_combine(
            states.data_ptr(), W, row(states) * 8, sums.data_ptr() if pagg else None,
            row(sums) * 8 if pagg else 0, gt.data_ptr() if pagg else None,
            conn.data_ptr() if pagg else None, B, T, F, J, int(num_proposals),
            None if merged is None else merged.data_ptr(), ptr("jbest"), ptr("pagg"), ptr("jagg"), ptr("pick"), _stream(states)))
    return out

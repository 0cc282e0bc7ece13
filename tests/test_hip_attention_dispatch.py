"""GPU tests of the attention dispatch at head counts, sequence counts and lengths the other files never reach: the item ->
(sequence, head) map of attn_kernel / attn_long_kernel / the two backward kernels on an exhaustive small lattice, the padded
length and head-dim boundaries of attention(), large logits on the short kernels, the one-head-per-workgroup instantiations of
the fused qkv + attention kernels that only odd head counts select, and one block at 7 heads in every product mode.  Every
case runs through pafuse_amd.ops against an fp64 torch evaluation of the same operation.

Guard rows.  Every forward (and backward) call here hands the kernel a tensor with spare rows behind the last sequence: enough
that the sequences nseq .. nseq + 7 under the same addressing would still lie inside it.  The spare rows of the input hold finite
random data; the ops return zero-initialised outputs, and each test asserts that every row no sequence owns is still exactly
zero.  A wrong item map (before the fix in attn_item: odd heads, nseq = 8 mod 16, L <= 48 reached the sequences nseq .. nseq + 3)
then shows as non-zero guard rows and zero slices inside, an assertion failure, not as an access outside an allocation.
The one exception is test_block_forward_at_seven_heads: qkv and o there are the block's own workspaces, sized for its 8 sequences,
so no guard can stand behind them.  It runs the defect's shape (8 sequences, 7 heads, L = 27) and relies on the fix being in
place - the guarded item-map tests above it are the ones that would catch the defect's return.

Bounds.  None is new; each is the one the suite already holds for the same operation at the same input scale:
  * the lattice, forward: atol 3e-6 at N(0, 1) inputs (test_hip_parity.test_unit_ops_on_a_seeded_sweep_of_shapes);
  * the lattice, backward: max <= 4e-6 scale + 1e-7, mean <= 3e-7 scale, scale = max |fp64 gradient|, at 1.5 N(0, 1) inputs
    (test_hip_train.test_attention_backward_kernel_against_fp64);
  * named shapes and the dispatch boundaries: max <= 2e-6, mean <= 1.5 x the mean error of torch's fp32 evaluation + 1e-9
    (test_hip_parity.test_attention_contiguous);
  * large logits: finite, max <= max(2e-6, 2 x torch fp32's max), mean <= 1.5 x torch fp32's mean + 1e-9
    (test_hip_long_clips.test_long_attention_forward_large_logits);
  * the fused kernels: max <= 1.5e-5, mean <= 4e-7 on random data, 4e-6 on the exact selector data
    (test_hip_parity.test_fused_qkv_attention_kernel_against_fp64);
  * the block: 1e-5 pointwise at N(0, 1) inputs and the seeded G4-style weights (test_hip_parity.test_g4_blocks_golden).
"""
from functools import partial

import pytest
import torch

from oracle import d3dp_oracle as orc
from tests.golden import golden_util as gu
from tests.test_hip_parity import _qkv_attention_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_SEQS = 8      # room behind the last sequence, in sequences of the same addressing


def _layout(nseq, L, group=0):
    """(rows [nseq, L], M, kwargs of the op).  group = 0: contiguous sequences of L rows.  group = J > 0: temporal addressing,
    row (r, t, j) = (r L + t) J + j and sequence s = (r, j) = divmod(s, J).  M leaves room for GUARD_SEQS more sequences."""
    s, t = torch.arange(nseq)[:, None], torch.arange(L)[None, :]
    if group:
        rows = ((s // group) * L + t) * group + s % group
        M = -(-(nseq + GUARD_SEQS) // group) * L * group
        return rows, M, dict(group=group, group_stride=L * group, seq_stride=1, tok_stride=group)
    return s * L + t, (nseq + GUARD_SEQS) * L, {}


def _attention(qkv, heads, rows):
    """softmax(q k^T d^-1/2) v per sequence and head in the dtype of qkv (autograd-able); rows no sequence owns stay zero"""
    M, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    nseq, L = rows.shape
    x = qkv[rows].reshape(nseq, L, 3, heads, d)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                      # [nseq, heads, L, d]
    p = torch.softmax(q @ k.transpose(-2, -1) * d ** -0.5, dim=-1)
    o = torch.zeros(M, C, dtype=qkv.dtype)
    return o.index_put((rows.reshape(-1),), (p @ v).transpose(1, 2).reshape(nseq * L, C))


def _unowned_rows_are_zero(out, rows):
    free = torch.ones(out.shape[0], dtype=torch.bool)
    free[rows.reshape(-1)] = False
    assert bool(free.any())                       # the guard exists
    return not bool((out[free] != 0).any())       # (NaN != 0 is True: a NaN in a guard row fails as well)


def _owned(err, rows):
    """the error on the rows some sequence owns: the unowned rows are exactly zero on both sides and would only dilute a mean"""
    return err[rows.reshape(-1)]


def _forward(L, C, heads, nseq, group, seed, qk_gain=1.0):
    """(hip output fp64, fp64 truth, torch fp32 evaluation as fp64, rows, qkv) of one seeded case with guard rows"""
    from pafuse_amd import ops
    rows, M, kw = _layout(nseq, L, group)
    qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(seed))
    qkv[:, :2 * C] *= qk_gain
    out = ops.attention(qkv.to(DEV), heads, nseq, L, **kw).cpu().double()
    return out, _attention(qkv.double(), heads, rows), _attention(qkv, heads, rows).double(), rows, qkv


def _assert_as_close_as_torch_fp32(tag, out, truth, torch32, rows):
    """the bounds of test_attention_contiguous, and the guard rows"""
    err, err_t = _owned((out - truth).abs(), rows), _owned((torch32 - truth).abs(), rows)
    print(f"{tag}: max {float(err.max()):.2e} (torch {float(err_t.max()):.2e}) mean {float(err.mean()):.2e} (torch {float(err_t.mean()):.2e})")
    assert _unowned_rows_are_zero(out, rows), tag
    assert float(err.max()) <= 2e-6, (tag, float(err.max()))
    assert float(err.mean()) <= 1.5 * float(err_t.mean()) + 1e-9, (tag, float(err.mean()), float(err_t.mean()))


# ------------------------------------------------------------------------------------------------------ 1. the item map
LATTICE_HEADS, LATTICE_NSEQ = range(1, 10), range(1, 41)
SPARSE_HEADS, SPARSE_NSEQ = (1, 3, 7, 8), (7, 8, 16, 24)


def _forward_lattice(L, all_heads, all_nseq):
    """every (heads, nseq) at head dim 4, contiguous: [(heads, nseq, max error, guard rows zero)] of the failing cases"""
    bad, worst = [], 0.0
    for heads in all_heads:
        for nseq in all_nseq:
            out, truth, _, rows, _ = _forward(L, 4 * heads, heads, nseq, 0, (L * 16 + heads) * 64 + nseq)
            err, guard = float((out - truth).abs().max()), _unowned_rows_are_zero(out, rows)
            worst = max(worst, err) if err == err else float("nan")
            if not err <= 3e-6 or not guard:
                bad.append((heads, nseq, err, guard))
    print(f"attention forward lattice L={L}: {len(all_heads) * len(all_nseq)} cases, largest error {worst:.2e}, {len(bad)} failing")
    return bad


@pytest.mark.parametrize("L", [2, 33, 49])
def test_item_map_forward_on_the_whole_small_lattice(L):
    """attn_kernel's item order over heads 1 .. 9 x nseq 1 .. 40: L = 2 and 33 are the two forms with two items per workgroup
    (<32,*,4>, <48,*,6>), L = 49 the one-item form <80,*,5>.  Every (sequence, head) slice must be written, once, and nothing
    else: the swizzled order is a bijection only when ITEMS divides (nseq / 8) heads."""
    bad = _forward_lattice(L, LATTICE_HEADS, LATTICE_NSEQ)
    assert not bad, bad


def test_item_map_forward_long_kernel():
    """attn_long_kernel (L = 145) takes the same map with one item per workgroup"""
    bad = _forward_lattice(145, SPARSE_HEADS, SPARSE_NSEQ)
    assert not bad, bad


@pytest.mark.parametrize("L", [2, 49, 81])
def test_item_map_backward(L):
    """the backward kernels' use of the map (one item per workgroup): the matrix kernel's <32,32> and <80,32> forms and, at
    L = 81, the FMA kernel.  dqkv against fp64 autograd, zero on the rows no sequence owns."""
    from pafuse_amd import ops
    bad = []
    for heads in SPARSE_HEADS:
        for nseq in SPARSE_NSEQ:
            C = 4 * heads
            rows, M, kw = _layout(nseq, L)
            g = torch.Generator().manual_seed((L * 16 + heads) * 64 + nseq)
            qkv = torch.randn(M, 3 * C, generator=g) * 1.5
            d_o = torch.randn(M, C, generator=g)
            q64 = qkv.double().requires_grad_(True)
            _attention(q64, heads, rows).backward(d_o.double())
            got = ops.attention_backward(qkv.to(DEV), d_o.to(DEV), heads, nseq, L, **kw).cpu().double()
            err, scale = _owned((got - q64.grad).abs(), rows), float(q64.grad.abs().max())
            guard = _unowned_rows_are_zero(got, rows)
            print(f"attention backward L={L} heads={heads} nseq={nseq}: max {float(err.max()):.2e} mean {float(err.mean()):.2e} of scale {scale:.2e}")
            if not float(err.max()) <= 4e-6 * scale + 1e-7 or not float(err.mean()) <= 3e-7 * scale or not guard:
                bad.append((heads, nseq, float(err.max()), float(err.mean()), scale, guard))
    assert not bad, bad


# ------------------------------------------------------------------------------------- 2. what the model mirror reaches
def test_face_denoiser_at_seven_heads_temporal():
    """MixSTE2(embed_dim_ratio=224, num_heads=7) on the face's 68 joints, one clip, one hypothesis, flip-TTA: temporal attention
    over nseq = 2 x 68 = 136 = 8 x 17 sequences of 27 frames at head dim 32"""
    out, truth, torch32, rows, _ = _forward(27, 224, 7, 2 * 68, 68, 2207)
    _assert_as_close_as_torch_fp32("C=224 heads=7 L=27 temporal nseq=136", out, truth, torch32, rows)


def test_width_288_at_nine_heads():
    out, truth, torch32, rows, _ = _forward(24, 288, 9, 24, 0, 2889)
    _assert_as_close_as_torch_fp32("C=288 heads=9 L=24 contiguous nseq=24", out, truth, torch32, rows)


# ------------------------------------------------------------------------------- 3. the boundaries of attention()'s dispatch
BOUNDARY_LENGTHS = (1, 16, 17, 32, 33, 48, 49, 80, 81, 144, 145)
BOUNDARY_HEAD_DIMS = (4, 20, 28, 32, 36, 48)


@pytest.mark.parametrize("d", BOUNDARY_HEAD_DIMS)
@pytest.mark.parametrize("L", BOUNDARY_LENGTHS)
def test_padded_length_and_head_dim_boundaries(L, d):
    """both sides of every padded length (LP = 32 / 48 / 80 / 144 / the long kernel) x head dims that are no multiple of 16 and
    sit on both sides of DP = 32 / 48; three heads, eight sequences"""
    out, truth, torch32, rows, _ = _forward(L, 3 * d, 3, 8, 0, 1000 * L + d)
    _assert_as_close_as_torch_fp32(f"L={L} d={d} heads=3 nseq=8 contiguous", out, truth, torch32, rows)


@pytest.mark.parametrize("L", [17, 33, 49, 81, 145])
def test_padded_length_boundaries_temporal(L):
    out, truth, torch32, rows, _ = _forward(L, 3 * 28, 3, 8, 3, 1000 * L + 28 + 1)
    _assert_as_close_as_torch_fp32(f"L={L} d=28 heads=3 nseq=8 temporal (groups of 3)", out, truth, torch32, rows)


# ------------------------------------------------------------------------------------ 4. large logits, the short kernels
@pytest.mark.parametrize("L", [27, 42, 68, 134])
def test_short_attention_forward_large_logits(L):
    """test_long_attention_forward_large_logits' construction on each length form of attn_kernel (LP = 32, 48, 80, 144): q and
    k scaled by 6 at head dim 48, logits of standard deviation 36 whose largest exceed the 88.7 where fp32 exp overflows - a
    kernel without the max subtraction returns inf / NaN here (asserted: it occurs)"""
    heads, nseq, d = 8, 6, 48
    out, truth, torch32, rows, qkv = _forward(L, heads * d, heads, nseq, 3, 7 + L, qk_gain=6.0)
    x = qkv[rows].reshape(nseq, L, 3, heads, d)
    logits = torch.einsum("slhd,sthd->shlt", x[:, :, 0], x[:, :, 1]) * d ** -0.5
    assert float(logits.max()) > 88.8 and bool(torch.isinf(logits.exp()).any())
    assert bool(torch.isfinite(out).all())
    assert _unowned_rows_are_zero(out, rows)
    err, err_t = _owned((out - truth).abs(), rows), _owned((torch32 - truth).abs(), rows)
    print(f"large logits L={L}: max {float(err.max()):.2e} (torch {float(err_t.max()):.2e}) mean {float(err.mean()):.2e} (torch {float(err_t.mean()):.2e})")
    assert float(err.max()) <= max(2e-6, 2 * float(err_t.max())), (float(err.max()), float(err_t.max()))
    assert float(err.mean()) <= 1.5 * float(err_t.mean()) + 1e-9, (float(err.mean()), float(err_t.mean()))


# ---------------------------------------------------------------- 5. the fused kernels' one-head-per-workgroup instantiations
ODD_HEAD_FQA_FORMS = [   # (name, L, C, heads, temporal joints J or 0): hfqa_kernel / xfqa_kernel <32,32,1> and <48,32,1>
    ("<32,32,1> 3 heads contiguous", 27, 96, 3, 0), ("<32,32,1> 7 heads temporal", 27, 224, 7, 5),
    ("<48,32,1> 5 heads contiguous", 42, 160, 5, 0), ("<48,32,1> 3 heads temporal", 42, 96, 3, 5)]


@pytest.mark.parametrize("scheme", ["f16x2", "bf16x3_images"])
@pytest.mark.parametrize("form", ODD_HEAD_FQA_FORMS, ids=[f[0] for f in ODD_HEAD_FQA_FORMS])
def test_fused_qkv_attention_odd_head_forms_against_fp64(form, scheme):
    """fused_qkv_attention takes launch_hfqa / launch_xfqa <32,32,1> and <48,32,1> only when the head count is odd; the loop's
    8 heads never do.  The two checks of test_fused_qkv_attention_kernel_against_fp64 (random data with and without the folded
    LayerNorm's row factor; exact selector data), contiguous with a ragged last tile (23 sequences) and temporal (3 x 5)."""
    from pafuse_amd import ops
    name, L, C_, heads, J = form
    g = torch.Generator().manual_seed(17 + L + C_)
    nseq = 3 * J if J else 23                          # 23: never a multiple of the sequences per tile (4 at L = 27, 3 at L = 42)
    seqs, M, kw = _layout(nseq, L, J)
    x = torch.randn(M, C_, generator=g)
    w = torch.randn(3 * C_, C_, generator=g) * C_ ** -0.5
    b = torch.randn(3 * C_, generator=g) * 0.1
    for rstd in (None, 0.5 + torch.rand(M, generator=g)):
        truth = _qkv_attention_fp64(x, w, b, heads, seqs, rstd)
        out = ops.qkv_attention_fused(x.to(DEV), w.to(DEV), b.to(DEV), heads, nseq, L, scheme,
                                      rstd=None if rstd is None else rstd.to(DEV), **kw).cpu().double()
        err = _owned((out - truth).abs(), seqs)
        print(f"fused {name} {scheme} rstd={rstd is not None}: max {float(err.max()):.2e} mean {float(err.mean()):.2e}")
        assert _unowned_rows_are_zero(out, seqs), (name, scheme)
        assert float(err.max()) <= 1.5e-5 and float(err.mean()) <= 4e-7, (name, scheme, rstd is not None, float(err.max()), float(err.mean()))
    xi = torch.randint(-8, 9, (M, C_), generator=g).float()
    sel = torch.randint(0, C_, (C_,), generator=g)
    wi = torch.zeros(3 * C_, C_)
    wi[2 * C_ + torch.arange(C_), sel] = 1.0           # v[:, c] = x[:, sel[c]]; q = k = 0: softmax = 1 / L everywhere
    out = ops.qkv_attention_fused(xi.to(DEV), wi.to(DEV), torch.zeros(3 * C_, device=DEV), heads, nseq, L, scheme, **kw).cpu().double()
    want = torch.zeros(M, C_, dtype=torch.float64)
    want[seqs.reshape(-1)] = xi.double()[seqs][:, :, sel].mean(1, keepdim=True).expand(-1, L, -1).reshape(-1, C_)
    print(f"fused {name} {scheme} selector: max {float((out - want).abs().max()):.2e}")
    assert float((out - want).abs().max()) <= 4e-6, (name, scheme, float((out - want).abs().max()))


# --------------------------------------------------------------------------------------------------- 6. one block, 7 heads
@pytest.fixture(scope="module")
def seven_head_block():
    """(block parameters on the device, input [8, 27, 224], fp64 output of the oracle's block): the G4 construction (seeded
    weights by key, N(0, 1) rows) at the width of the face denoiser with 7 heads of 32 channels"""
    from pafuse_amd.mixste2 import _BlockParams
    blk = _BlockParams(224, 2.0, True, partial(torch.nn.LayerNorm, eps=1e-6))
    sd = gu.seeded_like(blk.state_dict(), seed=41, prefix="dispatch.face7.")
    blk.load_state_dict(sd)
    x = torch.randn(8, 27, 224, generator=torch.Generator().manual_seed(42))
    truth = orc.transformer_block({k: v.double() for k, v in sd.items()}, "", x.double(), 7)
    return blk.to(DEV), x, truth


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16x3_images", "f16x2"])
def test_block_forward_at_seven_heads(seven_head_block, precision):
    """pafuse_block_forward at C = 224, 7 heads, 8 sequences of 27 tokens: attn_kernel<32,32,4> at the sequence count whose
    swizzled order was no bijection ('f32', 'bf16x3', 'f16x2' with the image output) and xfqa_kernel<32,32,1>
    ('bf16x3_images'), on the path the model takes; test_g4_blocks_golden's bound against the fp64 block.  No guard rows are
    possible here (the block owns its workspaces): this test relies on the attn_item fix being in place."""
    from pafuse_amd import ops
    blk, x, truth = seven_head_block
    y = ops.block_forward(blk, x.to(DEV), heads=7, precision=precision).cpu().double()
    err = (y - truth).abs()
    print(f"block 7 heads {precision}: max {float(err.max()):.2e} mean {float(err.mean()):.2e}")
    assert torch.allclose(y, truth, rtol=0, atol=1e-5), (precision, float(err.max()))

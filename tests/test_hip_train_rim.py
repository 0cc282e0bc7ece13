"""Unit tests of the gradient kernels at the rim of the training step - output head, patch embedding, spatial / temporal position
embeddings, time embedding - and of the sinusoid in front of the time MLP, through their unit entries (pafuse_train_head_grad ->
head_grad, pafuse_train_patch_grad -> concat_inputs + patch_grad, pafuse_train_group_sum -> group_sum, pafuse_train_sinusoid ->
sinusoid: the host functions the step calls), against the fp64 references of tests/train_rim_reference.py (proved against
autograd in tests/test_train_rim_host.py).

Exact integers are the structural proof: with operands in -3 .. 3 every product and every partial sum is an integer below 2^24,
exact in fp32 in any order, so a dropped or doubled row, a wrong group, a missed channel pass or a transposed read is a wrong
integer.  One 24-bit operand against a single power of two per output column shows that products and partials stay fp32.
Random data: u = 2^-24; a sum of n fp32 terms (products rounded once each) in any order is within (n + 2) u sum|terms| of the
exact one - n - 1 additions and one rounding of each product, to first order, with one u to spare for the second-order terms at
the n used here (n u < 2^-9).  The head's bias gradient has 3 elements, too few for a comparison of mean errors with torch's:
the mean of n absolute errors has a relative standard error of about 0.76 / sqrt(n), the ratio of two such means 1.07 / sqrt(n)
- 62 % at n = 3, 11 % at 32 draws, 1.9 % at the 1024 draws (3072 sums) the random-data test pools for it.
"""
import math

import pytest
import torch

from tests import train_rim_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
NAN_BITS = 0x7FC0DEAD
PAD = 96                      # NaN floats in front of and behind every output
HEAD_DRAWS = 1024             # draws of dout that the head's 3-element bias gradient is pooled over


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, seed, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=_gen(seed), device=DEV).float()


def _normal(shape, seed):
    return torch.randn(shape, generator=_gen(seed), device=DEV)


def _nan_filled(n):
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def framed(shape, fill=None):
    """(buffer, view): a `shape` view with PAD NaN floats on either side, holding `fill` (None: NaN as well)"""
    n = math.prod(shape)
    buf = _nan_filled(n + 2 * PAD)
    view = buf[PAD:PAD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def frame_untouched(buf):
    bits = buf.view(torch.int32)
    edge = torch.cat((bits[:PAD], bits[-PAD:]))
    return torch.equal(edge, torch.full_like(edge, NAN_BITS))


def assert_equal(out, want, what):
    out, want = out.detach().cpu().double(), want.detach().cpu().double()
    assert out.shape == want.shape, (what, out.shape, want.shape)
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {out.numel()} elements differ, first at {bad[0].tolist()}: "
                             f"{out[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}")


def within_sum_bound(val, truth, n, abs_terms, torch32, what):
    """every element within (n + 2) u sum|terms| of the fp64 sum, and the mean error at most 1.5 x that of torch's fp32 CPU result"""
    err, err_torch = (val.detach().cpu().double() - truth).abs(), (torch32.double() - truth).abs()
    bound = (n + 2) * U * abs_terms
    line = (f"{what}: max error / bound {float((err / bound).max()):.3f}, mean error {float(err.mean()):.3e} "
            f"(torch fp32 CPU {float(err_torch.mean()):.3e})")
    print(line)
    assert bool((err <= bound).all()), line
    assert float(err.mean()) <= 1.5 * float(err_torch.mean()), line


# ==================================================================================================== group sums
@pytest.mark.parametrize("B,F,J,C", ref.GROUP_SUM_CASES)
def test_group_sums_exact_on_integers(B, F, J, C):
    """All three modes, added into an integer prefill and written over NaN, inside NaN frames; a second call adds the sum again
    (accumulate) or gives the same bits (overwrite)."""
    from pafuse_amd import ops
    x = _ints((B, F, J, C), B + F + J + C)
    xc = x.cpu()
    for mode in (0, 1, 2):
        want = ref.group_sum_ref(xc, mode)
        G = (J, F, B)[mode]
        what = (B, F, J, C, "mode", mode, "chunks", ref.split_form(ref.group_count(mode, B, F, J))[0])
        pre = _ints((G, C), 11 + mode, -50, 51)
        buf, out = framed((G, C), pre)
        got = ops.train_group_sum(x, mode, out=out, accumulate=True)
        assert got.data_ptr() == out.data_ptr()
        assert_equal(got, pre.cpu().double() + want, what + ("accumulate",))
        assert_equal(ops.train_group_sum(x, mode, out=out, accumulate=True), pre.cpu().double() + 2 * want, what + ("accumulate twice",))
        assert frame_untouched(buf), what
        buf, out = framed((G, C))
        assert_equal(ops.train_group_sum(x, mode, out=out, accumulate=False), want, what + ("overwrite",))
        first = out.clone()
        assert torch.equal(ops.train_group_sum(x, mode, out=out, accumulate=False), first), what + ("repeat",)
        assert frame_untouched(buf), what


# ===================================================================================================== output head
def head_outputs(C, M, seed):
    """framed outputs of train_head_grad: the gradients prefilled with integers, dhn with NaN"""
    pre_w, pre_b = _ints((3, C), seed, -50, 51), _ints((3,), seed + 1, -50, 51)
    bw, vw = framed((3, C), pre_w)
    bb, vb = framed((3,), pre_b)
    bh, vh = framed((M, C))
    return (pre_w, pre_b), (bw, bb, bh), {"d_head_w": vw, "d_head_b": vb, "dhn": vh}


@pytest.mark.parametrize("M,C", ref.HEAD_CASES)
def test_head_gradients_exact_on_integers(M, C):
    """d head_w = prefill + dout^T hn, d head_b = prefill + column sums, dhn = dout head_w over NaN - head_w made asymmetric in
    its two axes so that a [C,3] read of it shows; NaN frames kept; a second call on fresh prefill gives the same bits."""
    from pafuse_amd import ops
    dout, hn = _ints((M, 3), M + C), _ints((M, C), M + C + 1)
    head_w = _ints((3, C), M + C + 2) + torch.arange(3, device=DEV, dtype=torch.float32)[:, None]
    d_w, d_b, d_hn = ref.head_grad_ref(dout.cpu(), hn.cpu(), head_w.cpu())
    runs = []
    for _ in range(2):
        (pre_w, pre_b), bufs, out = head_outputs(C, M, seed=5)
        res = ops.train_head_grad(dout, hn, head_w, out=out)
        assert_equal(res["d_head_w"], pre_w.cpu().double() + d_w, (M, C, "d_head_w"))
        assert_equal(res["d_head_b"], pre_b.cpu().double() + d_b, (M, C, "d_head_b"))
        assert_equal(res["dhn"], d_hn, (M, C, "dhn"))
        assert all(frame_untouched(b) for b in bufs), (M, C)
        runs.append([res[k].clone() for k in ("d_head_w", "d_head_b", "dhn")])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), (M, C, "repeat")


@pytest.mark.parametrize("M,C", ref.HEAD_CASES)
def test_head_weight_gradient_keeps_the_full_fp32_width(M, C):
    """hn 24-bit integers; dout zero except, per output column i, one row holding a power of two 2^-3 .. 2^3: every sum has one
    term and d head_w[i] must be hn[row_i] 2^e_i bit for bit."""
    from pafuse_amd import ops
    g = torch.Generator().manual_seed(M + C)
    hn = torch.randint(-2 ** 23, 2 ** 23, (M, C), generator=g).float()
    rows = torch.randint(0, M, (3,), generator=g)
    scale = 2.0 ** torch.randint(-3, 4, (3,), generator=g).float()
    dout = torch.zeros(M, 3)
    dout[rows, torch.arange(3)] = scale
    head_w = torch.randint(-3, 4, (3, C), generator=g).float()
    res = ops.train_head_grad(dout.to(DEV), hn.to(DEV), head_w.to(DEV))
    assert_equal(res["d_head_w"], hn[rows].double() * scale.double()[:, None], (M, C, "one term per sum"))
    d_w, d_b, d_hn = ref.head_grad_ref(dout, hn, head_w)
    assert_equal(res["d_head_w"], d_w, (M, C, "d_head_w"))
    assert_equal(res["d_head_b"], d_b, (M, C, "d_head_b"))
    assert_equal(res["dhn"], d_hn, (M, C, "dhn"))


# ================================================================================================= patch embedding
PATCH_SHAPES = lambda B, F, J, C: {"d_patch_w": (C, 5), "d_patch_b": (C,), "d_pos_spatial": (J, C), "dtemb": (B, C)}   # noqa: E731


def patch_outputs(B, F, J, C, seed):
    pre, bufs, out = {}, [], {}
    for i, (k, shape) in enumerate(PATCH_SHAPES(B, F, J, C).items()):
        pre[k] = None if k == "dtemb" else _ints(shape, seed + i, -50, 51)
        buf, out[k] = framed(shape, pre[k])
        bufs.append(buf)
    return pre, bufs, out


@pytest.mark.parametrize("B,F,J,C", ref.PATCH_CASES)
def test_patch_gradients_exact_on_integers(B, F, J, C):
    """d patch_w [C,5] = prefill + g^T cat(x2d, x3d) with columns 0..1 from x2d and 2..4 from x3d, d patch_b and d pos_spatial
    added into, dtemb written over NaN; NaN frames kept; a second call on fresh prefill gives the same bits."""
    from pafuse_amd import ops
    x2d, x3d, g = _ints((B, F, J, 2), B + C), _ints((B, F, J, 3), B + C + 1), _ints((B, F, J, C), B + C + 2)
    want = dict(zip(PATCH_SHAPES(B, F, J, C), ref.patch_grad_ref(x2d.cpu(), x3d.cpu(), g.cpu())))
    g2 = g.cpu().double().reshape(-1, C)
    runs = []
    for _ in range(2):
        pre, bufs, out = patch_outputs(B, F, J, C, seed=9)
        res = ops.train_patch_grad(x2d, x3d, g, out=out)
        for k in want:
            assert_equal(res[k], want[k] if pre[k] is None else pre[k].cpu().double() + want[k], (B, F, J, C, k))
        added = res["d_patch_w"].cpu().double() - pre["d_patch_w"].cpu().double()
        assert_equal(added[:, :2], g2.t() @ x2d.cpu().double().reshape(-1, 2), (B, F, J, C, "columns 0..1 <- x2d"))
        assert_equal(added[:, 2:], g2.t() @ x3d.cpu().double().reshape(-1, 3), (B, F, J, C, "columns 2..4 <- x3d"))
        assert all(frame_untouched(b) for b in bufs), (B, F, J, C)
        runs.append([res[k].clone() for k in want])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), (B, F, J, C, "repeat")


@pytest.mark.parametrize("B,F,J,C", ref.PATCH_CASES)
def test_patch_weight_gradient_keeps_the_full_fp32_width(B, F, J, C):
    """g 24-bit integers; the inputs zero except, per input column i, one row holding a power of two 2^-3 .. 2^3: d patch_w[:, i]
    must be g[row_i] 2^e_i bit for bit."""
    from pafuse_amd import ops
    gen = torch.Generator().manual_seed(B + F + J + C)
    M = B * F * J
    g = torch.randint(-2 ** 23, 2 ** 23, (B, F, J, C), generator=gen).float()
    rows = torch.randint(0, M, (5,), generator=gen)
    scale = 2.0 ** torch.randint(-3, 4, (5,), generator=gen).float()
    inputs = torch.zeros(M, 5)
    inputs[rows, torch.arange(5)] = scale
    x2d, x3d = inputs[:, :2].reshape(B, F, J, 2).contiguous(), inputs[:, 2:].reshape(B, F, J, 3).contiguous()
    res = ops.train_patch_grad(x2d.to(DEV), x3d.to(DEV), g.to(DEV))
    assert_equal(res["d_patch_w"], (g.reshape(M, C)[rows].double() * scale.double()[:, None]).t(), (B, F, J, C, "one term per sum"))
    assert_equal(res["d_patch_w"], ref.patch_grad_ref(x2d, x3d, g)[0], (B, F, J, C, "d_patch_w"))


# ============================================================================================ random data against fp64
def test_sums_of_random_data_against_fp64():
    """One mid-size case per entry, N(0,1) operands, new (zero) gradient outputs: every element within the any-order bound
    (n + 2) u sum|terms|, mean error <= 1.5 x torch's fp32 CPU result of the same sum.  The head's 3-element bias gradient is
    pooled over HEAD_DRAWS draws of dout (see the module docstring)."""
    from pafuse_amd import ops
    # head, M = 4097 (65 chunks, the last of one row)
    M, C = 4097, 224
    dout, hn, head_w = _normal((M, 3), 1), _normal((M, C), 2), _normal((3, C), 3)
    do, h, w = dout.cpu(), hn.cpu(), head_w.cpu()
    res = ops.train_head_grad(dout, hn, head_w)
    d_w, d_b, d_hn = ref.head_grad_ref(do, h, w)
    within_sum_bound(res["d_head_w"], d_w, M, do.double().abs().t() @ h.double().abs(), do.t() @ h, "head M=4097 C=224 d_head_w")
    within_sum_bound(res["dhn"], d_hn, 3, do.double().abs() @ w.double().abs(), do @ w, "head M=4097 C=224 dhn")
    douts = _normal((HEAD_DRAWS, M, 3), 8)
    got = torch.stack([ops.train_head_grad(douts[i], hn, head_w)["d_head_b"] for i in range(HEAD_DRAWS)])
    dc = douts.cpu()
    within_sum_bound(got, dc.double().sum(1), M, dc.double().abs().sum(1), torch.stack([d.sum(0) for d in dc]),
                     f"head M=4097 C=224 d_head_b, {HEAD_DRAWS} draws")
    # patch embedding, the body model's clip at B = 2
    B, F, J, C = 2, 27, 24, 384
    M = B * F * J
    x2d, x3d, g = _normal((B, F, J, 2), 4), _normal((B, F, J, 3), 5), _normal((B, F, J, C), 6)
    a2, a3, gc = x2d.cpu(), x3d.cpu(), g.cpu()
    res = ops.train_patch_grad(x2d, x3d, g)
    d_w, d_b, d_pos, d_temb = ref.patch_grad_ref(a2, a3, gc)
    in5, g2 = torch.cat((a2, a3), -1).reshape(M, 5), gc.reshape(M, C)
    tag = "patch (2,27,24,384) "
    within_sum_bound(res["d_patch_w"], d_w, M, g2.double().abs().t() @ in5.double().abs(), g2.t() @ in5, tag + "d_patch_w")
    within_sum_bound(res["d_patch_b"], d_b, M, g2.double().abs().sum(0), g2.sum(0), tag + "d_patch_b")
    within_sum_bound(res["d_pos_spatial"], d_pos, B * F, ref.group_sum_ref(gc.abs(), 0), gc.sum((0, 1)), tag + "d_pos_spatial")
    within_sum_bound(res["dtemb"], d_temb, F * J, ref.group_sum_ref(gc.abs(), 2), gc.sum((1, 2)), tag + "dtemb")
    # group sums, the hands model's clip at B = 2
    B, F, J, C = 2, 27, 42, 384
    x = _normal((B, F, J, C), 7)
    xc = x.cpu()
    for mode, dims in ((0, (0, 1)), (1, (0, 2)), (2, (1, 2))):
        within_sum_bound(ops.train_group_sum(x, mode), ref.group_sum_ref(xc, mode), ref.group_count(mode, B, F, J),
                         ref.group_sum_ref(xc.abs(), mode), xc.sum(dims), f"group_sum (2,27,42,384) mode {mode}")


# ========================================================================================================== sinusoid
@pytest.mark.parametrize("C", (64, 224, 384))
@pytest.mark.parametrize("B", (1, 37))
def test_sinusoid_layout_and_accuracy(B, C):
    """[sin | cos](t freqs) with the module's frequency table, t holding 0, 1 and 999 (B = 1: one call each).  The argument is one
    fp32 product, formed the same way on the CPU; columns [0, C/2) are the sines and [C/2, C) the cosines (exactly 0 and 1 at
    t = 0); against sin / cos of the same fp32 argument in fp64 the error is at most 4 x (max) and 1.5 x (mean) that of torch's
    fp32 CPU sin / cos - libm implementations differ by an ulp or two, a fast-math intrinsic at 999 rad by orders of magnitude.
    Measured on MI355X, |error| of the device (max, mean) against that of torch's fp32 CPU sin / cos (max, mean):
        B = 1,  C = 64:   4.126e-08, 6.627e-09   against   3.342e-08, 6.369e-09
        B = 1,  C = 224:  4.998e-08, 7.372e-09   against   3.433e-08, 6.668e-09
        B = 1,  C = 384:  4.559e-08, 7.174e-09   against   3.536e-08, 6.604e-09
        B = 37, C = 64:   5.578e-08, 1.245e-08   against   3.540e-08, 1.084e-08
        B = 37, C = 224:  6.034e-08, 1.245e-08   against   3.541e-08, 1.090e-08
        B = 37, C = 384:  6.119e-08, 1.247e-08   against   3.583e-08, 1.086e-08
    (the device's sinf / cosf are within one ulp of 1 at every argument up to 999 rad: max 1.7 x, mean 1.15 x torch's)
    """
    from pafuse_amd import ops
    from pafuse_amd.mixste2 import sinusoid_frequencies
    freqs = sinusoid_frequencies(C)
    assert freqs.dtype == torch.float32 and freqs.shape == (C // 2,)
    if B == 1:
        ts = [torch.tensor([v]) for v in (0, 1, 999)]
    else:
        ts = [torch.cat((torch.tensor([0, 1, 999]), torch.randint(0, 1000, (B - 3,), generator=torch.Generator().manual_seed(C))))]
    errs, errs_torch = [], []
    for t in ts:
        a = t.float()[:, None] * freqs[None]
        truth = ref.sinusoid_ref(a.double())
        buf, view = framed((B, C))
        out = ops.train_sinusoid(t.to(DEV), freqs.to(DEV), out=view)
        assert frame_untouched(buf) and not torch.isnan(out).any(), (B, C)
        assert torch.equal(ops.train_sinusoid(t.to(DEV), freqs.to(DEV)), out), (B, C, "repeat")
        out = out.cpu()
        zero = t == 0
        assert torch.equal(out[zero][:, :C // 2], torch.zeros(int(zero.sum()), C // 2)), (B, C, "sin(0)")
        assert torch.equal(out[zero][:, C // 2:], torch.ones(int(zero.sum()), C // 2)), (B, C, "cos(0)")
        # the halves taken one at a time: a swapped or interleaved layout is off by O(1)
        assert float((out[:, :C // 2].double() - a.double().sin()).abs().max()) < 1e-5, (B, C, "sines in front")
        assert float((out[:, C // 2:].double() - a.double().cos()).abs().max()) < 1e-5, (B, C, "cosines behind")
        errs.append((out.double() - truth).abs().reshape(-1))
        errs_torch.append((ref.sinusoid_ref(a).double() - truth).abs().reshape(-1))
    err, err_torch = torch.cat(errs), torch.cat(errs_torch)
    print(f"sinusoid B={B} C={C}: device max {float(err.max()):.3e} mean {float(err.mean()):.3e}, "
          f"torch fp32 CPU max {float(err_torch.max()):.3e} mean {float(err_torch.mean()):.3e}")
    assert float(err.max()) <= 4 * float(err_torch.max()), (float(err.max()), float(err_torch.max()))
    assert float(err.mean()) <= 1.5 * float(err_torch.mean()), (float(err.mean()), float(err_torch.mean()))


# ========================================================================================================== refusals
def test_invalid_argument_sets_are_refused_before_any_launch():
    """Each inconsistent argument set returns its error code and pafuse_last_error() names the problem, and no output changes;
    a call without rows is a no-op.  (Every pointer handed over is a real buffer.)"""
    from pafuse_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    E_ARG, E_SHAPE, E_WS = -1, -2, -3
    B, F, J, Cc = 2, 27, 24, 384
    M = B * F * J
    src = torch.zeros(M * Cc, device=DEV)
    t = torch.zeros(B, dtype=torch.int64, device=DEV)
    out = _nan_filled(M * Cc)
    P, O, T = src.data_ptr(), out.data_ptr(), t.data_ptr()
    need = {"head": lib.pafuse_train_head_grad_bytes(M, Cc), "patch": lib.pafuse_train_patch_grad_bytes(B, F, J, Cc),
            "group": lib.pafuse_train_group_sum_bytes(2, B, F, J, Cc)}
    # the partials the helpers write: 21 chunks of 3 C (head), [M,5] + [5,C] + the largest of the four reductions (patch), 31 chunks of B C
    assert need["head"] >= 21 * 3 * Cc * 4 and need["group"] >= 31 * B * Cc * 4
    assert need["patch"] >= (M * 5 + 5 * Cc + max(21 * 5 * Cc, 4 * J * Cc, 31 * B * Cc)) * 4
    ws = torch.empty(max(need.values()) + 64, dtype=torch.uint8, device=DEV)
    W = ws.data_ptr()

    def head(dout=P, hn=P, w=P, dw=O, db=O, dhn=O, m=M, c=Cc, wsp=W, ws_bytes=None):
        return lib.pafuse_train_head_grad(dout, hn, w, dw, db, dhn, m, c, wsp, need["head"] if ws_bytes is None else ws_bytes, stream)

    def patch(x2d=P, x3d=P, g=P, dw=O, db=O, dpos=O, dtemb=O, b=B, f=F, j=J, c=Cc, wsp=W, ws_bytes=None):
        nb = lib.pafuse_train_patch_grad_bytes(b, f, j, c) if ws_bytes is None else ws_bytes
        return lib.pafuse_train_patch_grad(x2d, x3d, g, dw, db, dpos, dtemb, b, f, j, c, wsp, nb, stream)

    def group(x=P, o=O, mode=2, acc=1, b=B, f=F, j=J, c=Cc, wsp=W, ws_bytes=None):
        nb = need["group"] if ws_bytes is None else ws_bytes
        return lib.pafuse_train_group_sum(x, o, mode, acc, b, f, j, c, wsp, nb, stream)

    def sinus(tt=T, fr=P, o=O, b=B, c=Cc):
        return lib.pafuse_train_sinusoid(tt, fr, o, b, c, stream)

    cases = [
        (lambda: head(dout=None), E_ARG, "null pointer"),
        (lambda: head(dhn=None), E_ARG, "null pointer"),
        (lambda: head(wsp=None), E_ARG, "null pointer"),
        (lambda: head(m=-1), E_ARG, "negative M"),
        (lambda: head(c=0), E_SHAPE, "C=0 out of range"),
        (lambda: head(m=2 ** 32 // Cc + 1), E_SHAPE, "out of range"),          # more elements of dhn than one grid has threads
        (lambda: head(ws_bytes=need["head"] - 1), E_WS, "workspace too small"),
        (lambda: patch(x3d=None), E_ARG, "null pointer"),
        (lambda: patch(dtemb=None), E_ARG, "null pointer"),
        (lambda: patch(f=-27), E_ARG, "negative size"),
        (lambda: patch(c=0), E_SHAPE, "C=0 out of range"),
        (lambda: patch(ws_bytes=need["patch"] - 1), E_WS, "workspace too small"),
        (lambda: group(x=None), E_ARG, "null pointer"),
        (lambda: group(o=None), E_ARG, "null pointer"),
        (lambda: group(b=-1), E_ARG, "negative size"),
        (lambda: group(mode=3), E_ARG, "mode 3"),
        (lambda: group(mode=-1), E_ARG, "mode -1"),
        (lambda: group(acc=2), E_ARG, "accumulate 2"),
        (lambda: group(c=-4), E_SHAPE, "C=-4 out of range"),
        (lambda: group(b=2 ** 31 - 1, f=2 ** 31 - 1, j=0), E_SHAPE, "out of range"),   # no rows, but B F leaves int
        (lambda: group(b=65536, f=256, j=128), E_SHAPE, "out of range"),               # 2^31 rows
        (lambda: group(ws_bytes=need["group"] - 1), E_WS, "workspace too small"),
        (lambda: group(mode=0, ws_bytes=lib.pafuse_train_group_sum_bytes(0, B, F, J, Cc) - 1), E_WS, "workspace too small"),
        (lambda: sinus(tt=None), E_ARG, "null pointer"),
        (lambda: sinus(o=None), E_ARG, "null pointer"),
        (lambda: sinus(b=-1), E_ARG, "negative B"),
        (lambda: sinus(c=383), E_SHAPE, "C=383 must be even"),
        (lambda: sinus(c=0), E_SHAPE, "C=0 must be even"),
    ]
    for i, (call, code, text) in enumerate(cases):
        rc = call()
        msg = lib.pafuse_last_error().decode()
        assert rc == code and text in msg, (i, rc, code, msg)
    assert lib.pafuse_train_group_sum_bytes(3, B, F, J, Cc) == 0 and lib.pafuse_train_head_grad_bytes(-1, Cc) == 0
    torch.cuda.synchronize()
    untouched = lambda: torch.equal(out.view(torch.int32), torch.full_like(out.view(torch.int32), NAN_BITS))   # noqa: E731
    assert untouched(), "a refused call wrote an output"
    assert head(m=0) == 0 and patch(b=0) == 0 and patch(j=0) == 0 and group(f=0) == 0 and sinus(b=0) == 0
    torch.cuda.synchronize()
    assert untouched(), "an empty call wrote an output"

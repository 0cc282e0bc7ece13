"""GPU tests that a non-finite value stays in its own row or sequence in every tiled kernel: each case runs an op of
pafuse_amd.ops on clean seeded N(0, 1) operands (`clean`), plants ONE non-finite value, runs the op again (`got`) and evaluates
the same operation in fp64 torch on the CPU on the poisoned operands (tests/test_nonfinite_host.py, whose masks are asserted
there without a GPU); mask = isnan(reference).  Three assertions per output, auxiliary outputs (stats, head, db, dw, dbranch,
out_scaled, the decoded images) included - _check():

  1. the reference stays within its conditions: mask is neither empty nor everything (the case is not vacuous);
  2. persistence: isnan(got) == mask - a kernel that swallows the NaN (fmaxf / fminf, a clamp, a select) fails here, and with
     it the promise that 'f16x2' fails loudly: finalize can only raise the range flag for what is still non-finite.  For the
     poison kinds +inf and 1e5 (finite in fp32, beyond fp16; 'f16x2' routes only) on the activation of a GEMM-like op:
     every element of the poisoned row is non-finite (the split of inf is (inf, NaN): either is right);
  3. containment: got[~mask] is BIT-equal to clean[~mask], through an int32 view (-0.0 and payloads count) - a neighbour's
     NaN times a weight of 0, a dead row's contribution, a deferred store of the previous tile fail here.  Every op is
     run-to-run reproducible and has no data-dependent tiling, so no tolerance is involved.

A failure of 2 or 3 is a kernel defect, not a rounding matter.  Which kernel a parametrisation reaches (pafuse_hip.hip):

  qkv_attention_fused   'f16x2' -> launch_hfqa: hfqa_kernel, 'bf16x3_images' -> launch_xfqa: xfqa_kernel; forms <32,48,2>
                        (L = 24, 27 at C = 384), <32,32,2> (L = 27 at 224 / 256), <48,32,2> (L = 42), <80,32,2> (L = 68, five
                        waves) and - odd head counts - <32,32,1>, <48,32,1>.  fqa_nseq_tile: 5 / 4 / 3 / 2 sequences per tile
                        at L = 24 / 27 / 42 / 68; token_of aliases absent sequences to the last token; phase 3 is
                        fqa_attention_from_lds, whose masked keys read the sequence's own last V row.  Positions: (a) first token
                        of the second sequence of tile 1 - the rows the first sequence's masked keys cover; (b) last token of the
                        last sequence - what absent sequences alias (23 sequences: a ragged last tile); (c) last token of the
                        first sequence of tile 1; (d) token 0 of sequence 0; and rstd[token (a)] = NaN with finite x.
  fqa_kernel            ('bf16x3', no unit entry): through the model with MixSTE2.fuse_qkv_attention on, a NaN in one
                        hypothesis' noise - test_fused_bf16x3_blocks_keep_a_hypothesis_apart.
  attention             attn_kernel <32,*,4> (L = 2, 27), <48,*,6> (33), <80,*,5> (49), <144,..> (134), attn_long_kernel
                        (145); DP = 32 (d = 28) and 48; heads 3 (plain item order) and 8 (swizzled order at nseq = 8); the item
                        once first and once second in its two-item workgroup (attn_item).
  attention_backward    attn_bwd matrix kernel <32,48> (27, 48), <80,32> (68, 28), <32,32> (17, 16); the FMA kernel (81, 8);
                        attn_bwd_long_kernel (145, 32).
  linear                gemm_kernel fp32 (and its bf16-operand form); linear_split 'bf16x3' layout 0 -> gemm16_kernel, layout 2
                        -> sgemm2_kernel (K >= 128) or gemm16_kernel (K = 64); 'bf16x3_images' -> xgemm_kernel, 'f16x2' ->
                        hgemm_kernel, both also with the image output; linear_train -> plain_linear (sgemm2_kernel with the
                        out_act epilogue at M >= 128 in 'bf16x3', else gemm_kernel).  The 8997-row stream: sgemm2_kernel walking
                        two tiles per workgroup, the stores of the first deferred into the second.
  linear_rowln(_group)  gemm_rowln_as: every route of tests/test_hip_rowln.py routes() (modes f32 / bf16 / bf16x3 at six widths,
                        f16x2 / bf16x3_images at three, fp32 or centred-image residual), EPI_ROWLN_TRAIN, grouped_rowln_kernel.
  mlp_fused             hmlp_kernel at C = 224, 256, 384.
  training backward     input_grad (transposed image + sgemm2 / gemm16, fp32 gemm_kernel), weight_grad (split-K wgrad kernels
                        + reduce), ln_backward_quad_kernel (C = 384, 224) / ln_backward_kernel (130, 768) + reduce_partials
                        (dbranch = the column sums of out_scaled: ALL of it is NaN once a row of dx is), gelu_bwd, group_sum.
  the rim               layernorm_kernel, embed_kernel (plain and one image form per mode), time_embed; and the whole loop in
                        'f16x2', which must RAISE on a NaN input and run clean again afterwards.
"""
import pytest
import torch

from tests import test_nonfinite_host as host
from tests.test_hip_attention_dispatch import ODD_HEAD_FQA_FORMS, _layout, _unowned_rows_are_zero
from tests.test_hip_parity import FQA_FORMS
from tests.test_hip_rowln import MODES, WIDTHS, route_id, routes

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF, BIG = float("nan"), float("inf"), 1e5       # BIG: finite in fp32, beyond fp16's 65504
KIND = {"nan": NAN, "inf": INF, "1e5": BIG}


# ---------------------------------------------------------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _planted(t, index, value=NAN):
    """a copy of t with one element replaced"""
    out = t.clone()
    out[index] = value
    return out


def _no_zero(*tensors):
    """no operand that multiplies the poisoned element is exactly 0 (0 x NaN is the case under test, not an accident of the data)"""
    return all(bool((t != 0).all()) for t in tensors)


def _dev(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def _row_mask(shape, row):
    m = torch.zeros(shape, dtype=torch.bool)
    m[row] = True
    return m


def _check(clean, got, mask, what, kind="nan"):
    """the three assertions of the module docstring on one output; prints the counts of poisoned and compared elements and
    reports the first differing index"""
    clean, got, mask = clean.detach().cpu().float(), got.detach().cpu().float(), mask.cpu()
    assert clean.shape == got.shape == mask.shape, (what, clean.shape, got.shape, mask.shape)
    print(f"{what}: {int(mask.sum())} poisoned, {int((~mask).sum())} compared")
    assert bool(torch.isfinite(clean).all()), (what, "the clean run is not finite")
    assert host.mask_within_its_conditions(mask), (what, "the reference's mask is empty or everything", int(mask.sum()))
    if kind == "nan":
        for fault, wrong in (("leaked: NaN where the reference has none", (torch.isnan(got) & ~mask).nonzero()),
                             ("swallowed: a number where the reference has NaN", (~torch.isnan(got) & mask).nonzero())):
            if wrong.shape[0]:
                i = tuple(wrong[0].tolist())
                raise AssertionError(f"{what}: persistence, isnan(got) != mask - {fault}, {wrong.shape[0]} elements, first at {list(i)}: "
                                     f"got {float(got[i])}, clean {float(clean[i])}")
    else:
        finite = (torch.isfinite(got) & mask).nonzero()
        if finite.shape[0]:
            i = tuple(finite[0].tolist())
            raise AssertionError(f"{what}: persistence ({kind}) - {finite.shape[0]} elements of the poisoned rows are finite, first at "
                                 f"{list(i)}: got {float(got[i])}, clean {float(clean[i])}")
    zero = torch.zeros_like(got)
    diff = host.first_difference(torch.where(mask, zero, got), torch.where(mask, zero, clean))
    if diff is not None:
        raise AssertionError(f"{what}: containment - {diff[0]} elements outside the mask differ from the clean run, first at {diff[1]}: "
                             f"{diff[2]} != {diff[3]}")


def _check_same(clean, got, what):
    """an output the poison must not reach at all: the clean run's bits"""
    diff = host.first_difference(got.detach().cpu().float(), clean.detach().cpu().float())
    assert diff is None, f"{what}: containment - {diff[0]} elements differ from the clean run, first at {diff[1]}: {diff[2]} != {diff[3]}"


# ----------------------------------------------------------------------------------------------- 1. fused qkv + attention
ALL_FQA_FORMS = [(n, L, C, 8, J) for n, L, C, J in FQA_FORMS] + list(ODD_HEAD_FQA_FORMS)
FQA_POSITIONS = ("a", "b", "c", "d", "rstd")


def _fqa_nseq_tile(L):
    """fqa_nseq_tile(L, lp) of pafuse_hip.hip: whole sequences per tile, lp = 32 / 48 / 80 the padded length, 128 / 132 / 160 rows"""
    lp = 32 if L <= 32 else (48 if L <= 48 else 80)
    rows = 160 if lp == 80 else 128 + (4 if lp == 48 else 0)
    return (rows - lp) // L + 1


def _fqa_case(form):
    name, L, C_, heads, J = form
    nseq = 3 * J if J else 23                          # 23: never a multiple of the sequences per tile (5, 4, 3, 2)
    rows, M, kw = _layout(nseq, L, J)
    g = _gen(170 + L + C_ + heads)
    x, w, b = _randn(g, M, C_), _randn(g, 3 * C_, C_, scale=C_ ** -0.5), _randn(g, 3 * C_, scale=0.1)
    rstd = 0.5 + torch.rand(M, generator=g)
    return nseq, rows, M, kw, x, w, b, rstd


@pytest.mark.parametrize("position", FQA_POSITIONS)
@pytest.mark.parametrize("scheme", ["f16x2", "bf16x3_images"])
@pytest.mark.parametrize("form", ALL_FQA_FORMS, ids=[f[0] for f in ALL_FQA_FORMS])
def test_fused_qkv_attention_keeps_a_nan_in_its_sequence(form, scheme, position):
    """hfqa_kernel / xfqa_kernel, every form, 23 contiguous or 3 x J temporal sequences with guard rows, with and without the
    folded LayerNorm's row factor: one NaN in x[token, channel] (or in rstd[token]) makes the token's sequence NaN in all
    heads, and leaves every other sequence - of the same tile too - and the guard rows with the clean run's bits."""
    from pafuse_amd import ops
    name, L, C_, heads, J = form
    nseq, rows, M, kw, x, w, b, rstd = _fqa_case(form)
    T = _fqa_nseq_tile(L)
    assert nseq > 2 * T and (J or nseq % T)            # two full tiles and - contiguous - a ragged last one
    seq, tok = {"a": (T + 1, 0), "b": (nseq - 1, L - 1), "c": (T, L - 1), "d": (0, 0), "rstd": (T + 1, 0)}[position]
    token, ch = int(rows[seq, tok]), C_ // 2 + 3
    assert _no_zero(w[:, ch], rstd[rows[seq]], x[rows[seq]])
    run = lambda x_, r_: ops.qkv_attention_fused(x_.to(DEV), *_dev(w, b), heads, nseq, L, scheme, rstd=None if r_ is None else r_.to(DEV), **kw)  # noqa: E731
    for with_rstd in ((True,) if position == "rstd" else (False, True)):
        r = rstd if with_rstd else None
        clean = run(x, r)
        bad_x, bad_r = (x, _planted(rstd, token)) if position == "rstd" else (_planted(x, (token, ch)), r)
        got = run(bad_x, bad_r)
        mask = torch.isnan(host.qkv_attention_ref(bad_x, w, b, heads, rows, bad_r))
        want = torch.zeros(M, C_, dtype=torch.bool)
        want[rows[seq]] = True
        assert torch.equal(mask, want)                 # the whole poisoned sequence, all heads
        _check(clean, got, mask, f"fused {name} {scheme} ({position}) rstd={with_rstd}")
        assert _unowned_rows_are_zero(got.cpu(), rows), (name, scheme, position)


def test_fused_bf16x3_blocks_keep_a_hypothesis_apart():
    """fqa_kernel ('bf16x3' with MixSTE2.fuse_qkv_attention: 16 + 8 + 16 fused blocks) has no unit entry: the loop at B = 2,
    P = 2, one step, a NaN in the noise of (clip 0, hypothesis 1).  The spatial tiles hold five 24-joint frames, so frames of
    both hypotheses share tiles.  NaN exactly where the oracle has them, the clean run's bits elsewhere."""
    import ctypes
    from __graft_entry__ import make_model
    from oracle import d3dp_oracle as orc
    from pafuse_amd import _lib
    from tests.golden import golden_util as gu
    B, P, T = 2, 2, 1
    model, sd = make_model(P, T, seed=59)
    model.precision = "bf16x3"
    for m in model.denoisers().values():
        m.fuse_qkv_attention = True
    x2d, x2f = gu.synthetic_inputs_2d(B=B, seed=1234)
    noises = gu.synthetic_noises(B=B, P=P, n=T, seed=9)
    model.noise_fn = lambda k, shape, device: noises[k]
    clean = model(x2d.to(DEV), None, input_2d_flip=x2f.to(DEV)).cpu()
    count = lambda m: _lib.check(_lib.load().pafuse_mixste2_fused_blocks(ctypes.byref(m.weights_struct())))      # noqa: E731
    assert {name: count(m) for name, m in model.denoisers().items()} == {"body": 16, "face": 8, "hands": 16}
    badn = [n.clone() for n in noises]
    badn[0][0, 1, 3, 9, 2] = NAN
    model.noise_fn = lambda k, shape, device: badn[k]
    got = model(x2d.to(DEV), None, input_2d_flip=x2f.to(DEV)).cpu()
    ref = orc.ddim_sample(sd, x2d, badn, T, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, inputs_2d_flip=x2f)
    _check(clean, got, torch.isnan(ref), "loop bf16x3 fused blocks, NaN in one hypothesis")


# ---------------------------------------------------------------------------------------------------- 2. attention forward
ATTN_LENGTHS = (2, 27, 33, 49, 134, 145)


def _item_position(seq, head, nseq, heads, items=2):
    """position of (seq, head) inside its workgroup of `items` items: attn_item of kernels.hpp, inverted by enumeration"""
    for i in range(nseq * heads):
        if nseq % 8 == 0 and ((nseq // 8) * heads) % items == 0:
            blk = i // items
            u = (blk // 8) * items + i % items
            s, h = (u // heads) * 8 + blk % 8, u % heads
        else:
            s, h = divmod(i, heads)
        if (s, h) == (seq, head):
            return i % items
    raise AssertionError((seq, head))


@pytest.mark.parametrize("which", ["q", "k", "v"])
@pytest.mark.parametrize("group", [0, 3], ids=["contiguous", "temporal"])
@pytest.mark.parametrize("L", ATTN_LENGTHS)
def test_attention_forward_keeps_a_nan_in_its_item(L, group, which):
    """ops.attention at 3 and 8 heads, d = 28 and 48, 8 sequences with guard rows: a NaN in q, k or v of one (sequence, token,
    head, channel), the item once first and once second in its two-item workgroup.  q: the row of (s, h); k: all rows of (s, h);
    v: one channel of all rows of (s, h) - the other item of the workgroup, the other heads and the guard rows keep their bits."""
    from pafuse_amd import ops
    nseq, seq = 8, 5
    rows, M, kw = _layout(nseq, L, group)
    tok = L - 1
    for heads in (3, 8):
        for d in (28, 48):
            C = heads * d
            qkv = _randn(_gen(L * 100 + heads * 10 + d), M, 3 * C)
            assert _no_zero(qkv[rows[seq]])
            clean = ops.attention(qkv.to(DEV), heads, nseq, L, **kw)
            picked = {_item_position(seq, h, nseq, heads): h for h in (heads - 1, heads - 2)}
            assert sorted(picked) == [0, 1]
            for pos, head in sorted(picked.items()):
                col = "qkv".index(which) * C + head * d + d - 3
                bad = _planted(qkv, (int(rows[seq, tok]), col))
                got = ops.attention(bad.to(DEV), heads, nseq, L, **kw)
                mask = torch.isnan(host.attention_ref(bad, heads, rows))
                _check(clean, got, mask, f"attention L={L} group={group} heads={heads} d={d} {which} item position {pos}")
                assert _unowned_rows_are_zero(got.cpu(), rows), (L, group, heads, d, which, pos)


# --------------------------------------------------------------------------------------------------- 3. attention backward
ATTN_BWD_SHAPES = ((27, 48), (68, 28), (17, 16), (81, 8), (145, 32))


@pytest.mark.parametrize("which", ["d_o", "q", "k", "v"])
@pytest.mark.parametrize("group", [0, 3], ids=["contiguous", "temporal"])
@pytest.mark.parametrize("L,d", ATTN_BWD_SHAPES)
def test_attention_backward_keeps_a_nan_in_its_item(L, d, group, which):
    """ops.attention_backward, 3 heads, 8 sequences with guard rows: a NaN in d_o, q, k or v of one (sequence, token, head,
    channel); the mask is fp64 autograd's, inside (s, h) of dq | dk | dv."""
    from pafuse_amd import ops
    nseq, heads, seq, head = 8, 3, 5, 1
    C = heads * d
    rows, M, kw = _layout(nseq, L, group)
    g = _gen(L * 64 + d)
    qkv, d_o = _randn(g, M, 3 * C), _randn(g, M, C)
    assert _no_zero(qkv[rows[seq]], d_o[rows[seq]])
    clean = ops.attention_backward(*_dev(qkv, d_o), heads, nseq, L, **kw)
    row = int(rows[seq, L // 2])
    if which == "d_o":
        bad_qkv, bad_do = qkv, _planted(d_o, (row, head * d + 2))
    else:
        bad_qkv, bad_do = _planted(qkv, (row, "qkv".index(which) * C + head * d + 2)), d_o
    got = ops.attention_backward(*_dev(bad_qkv, bad_do), heads, nseq, L, **kw)
    mask = torch.isnan(host.attention_backward_ref(bad_qkv, bad_do, heads, rows))
    own = torch.zeros(M, 3, heads, d, dtype=torch.bool)
    own[rows[seq], :, head] = True
    assert not bool((mask & ~own.reshape(M, 3 * C)).any())
    _check(clean, got, mask, f"attention backward L={L} d={d} group={group} NaN in {which}")
    assert _unowned_rows_are_zero(got.cpu(), rows), (L, d, group, which)


# --------------------------------------------------------------------------------------------------- 4. plain linear layers
LINEAR_SHAPES = ((129, 1152, 384), (65, 448, 224), (33, 128, 64))
LINEAR_ROUTES = [("linear", None), ("linear", "gelu"), ("linear-bf16", None), ("linear-bf16", "gelu")] + \
                [(f"split-{s}", a) for s in ("bf16x3-l0", "bf16x3-l2", "bf16x3_images", "f16x2") for a in (None, "gelu")] + \
                [("train-f32", "gelu"), ("train-bf16x3", "gelu")]


def _linear_outputs(route, act, x, w, b):
    """{name: output} of one plain linear route; image schemes also return the decoded image output"""
    from pafuse_amd import ops
    xd, wd, bd = _dev(x, w, b)
    M, N = x.shape[0], w.shape[0]
    if route.startswith("linear"):
        return {"y": ops.linear(xd, wd, bd, act, bf16=route.endswith("bf16"))}
    if route.startswith("train"):
        u, h = ops.linear_train(xd, wd, bd, gelu=True, precision=route.split("-")[1])
        return {"u": u, "y": h}
    scheme = route.split("-", 1)[1]
    if scheme.startswith("bf16x3-l"):
        return {"y": ops.linear_split(xd, wd, bd, act, layout=int(scheme[-1]), scheme="bf16x3")}
    join = ops.hjoin_rows if scheme == "f16x2" else ops.xjoin_rows
    return {"y": ops.linear_split(xd, wd, bd, act, scheme=scheme),
            "y_img": join(ops.linear_split(xd, wd, bd, act, scheme=scheme, out_image=True), M, N)}


def _linear_case(M, N, K, seed):
    g = _gen(seed)
    return _randn(g, M, K), _randn(g, N, K, scale=K ** -0.5), _randn(g, N, scale=0.1)


def _check_linear(route, act, x, w, b, clean, row, k, kind, what):
    bad = _planted(x, (row, k), KIND[kind])
    got = _linear_outputs(route, act, bad, w, b)
    mask = torch.isnan(host.linear_ref(_planted(x, (row, k)), w, b, act))
    assert torch.equal(mask, _row_mask(mask.shape, row))
    for name in clean:
        _check(clean[name], got[name], mask, f"{what} {name} row {row} {kind}", kind)


def _kinds(route):
    return ("nan", "inf", "1e5") if "f16x2" in route else ("nan", "inf")


@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
@pytest.mark.parametrize("route,act", LINEAR_ROUTES, ids=[f"{r}-{a}" for r, a in LINEAR_ROUTES])
def test_linear_keeps_a_nonfinite_activation_in_its_row(route, act, M, N, K):
    """ops.linear / linear_split / linear_train: a NaN, +inf or (f16x2) 1e5 at x[row, k] for row 0, the wave seam 31 / 32 and
    M - 1 (the only live row of the last tile): that output row is NaN (non-finite), every other row keeps its bits."""
    x, w, b = _linear_case(M, N, K, M + N + K)
    k = K // 2 + 1
    assert _no_zero(w[:, k])
    clean = _linear_outputs(route, act, x, w, b)
    for row in (0, 31, 32, M - 1):
        for kind in _kinds(route):
            _check_linear(route, act, x, w, b, clean, row, k, kind, f"{route} act={act} ({M},{N},{K})")


def _strip_walk(M, N, cus, b=0):
    """row tiles (first, last) that workgroup b of sgemm2_kernel walks and how many tiles it takes - launch_strip2 and tile_of
    of sgemm.hpp: tiles of 128 rows x BN columns, G = 2 workgroups per CU rounded down to a multiple of 8 (all tiles when
    there are fewer), workgroup b takes v = b, b + G, ..; v -> tile = first tile of XCD v & 7's contiguous share + (v >> 3)."""
    BN = 128 if N % 128 == 0 else (112 if N % 112 == 0 else 96)
    tiles_n, tiles_m = N // BN, -(-M // 128)
    ntiles = tiles_m * tiles_n
    G = cus * 2 // 8 * 8
    if G >= ntiles or G <= 0:
        G = ntiles
    mine = (ntiles - b + G - 1) // G

    def tile_row(j):
        v = b + j * G
        xcd, q, rem = v & 7, ntiles >> 3, ntiles & 7
        tile = (xcd * (q + 1) if xcd < rem else rem * (q + 1) + (xcd - rem) * q) + (v >> 3)
        return tile // tiles_n
    return tile_row(0), tile_row(mine - 1), mine


def test_strip_kernel_stream_keeps_a_nan_in_its_row():
    """sgemm2_kernel on the (8997, 1152, 384) stream of test_strip_kernel_tile_streams: 71 x 9 = 639 tiles of 128 x 128 on
    G = 512 workgroups (256 CUs x 2), so workgroups 0 .. 126 walk two tiles and the stores of the first are deferred into the
    chunks of the second.  Workgroup 0: v = 0 -> XCD 0, tile 0 (row tile 0, rows 0 .. 127); v = 512 -> XCD 0 (512 & 7), whose
    share starts at tile 0 (q = 79, rem = 7: shares of 80), + (512 >> 3) = tile 64 = row tile 7 (64 // 9), rows 896 .. 1023.
    Poisoned rows: 5 (the first tile) and 996 (row 100 of the last tile of the same walk); _strip_walk recomputes both from the
    device's CU count, so the case holds where that count differs."""
    from pafuse_amd import ops
    M, N, K = 8997, 1152, 384
    assert _strip_walk(M, N, 256) == (0, 7, 2)
    first, last, mine = _strip_walk(M, N, torch.cuda.get_device_properties(0).multi_processor_count)
    assert mine >= 2 and first != last
    x, w, b = _linear_case(M, N, K, 8997)
    k = 200
    assert _no_zero(w[:, k])
    for act in (None, "gelu"):
        clean = _linear_outputs("split-bf16x3-l2", act, x, w, b)
        for row in (first * 128 + 5, last * 128 + 100):
            _check_linear("split-bf16x3-l2", act, x, w, b, clean, row, k, "nan", f"strip stream act={act}")


# --------------------------------------------------------------------------------------------------- 5. whole-row layers
def _rowln_case(M, N, K, seed):
    g = _gen(seed)
    ln = lambda: (1 + _randn(g, N, scale=0.1), _randn(g, N, scale=0.1), 1e-6)      # noqa: E731
    p = dict(x=_randn(g, M, K, scale=0.7), w=_randn(g, N, K, scale=K ** -0.5), b=_randn(g, N, scale=0.1), r=_randn(g, M, N))
    p["post"], p["next"] = ln(), ln()
    p["pos"] = (_randn(g, 3, N, scale=0.02), 17, 3)
    p["head"] = (_randn(g, 3, N, scale=N ** -0.5), _randn(g, 3, scale=0.1))
    return p


def _rowln_options(p, fold, dev=True):
    """the full chain: post, pos, next + head - or, folded, next's statistics"""
    mv = (lambda t: t.to(DEV)) if dev else (lambda t: t)
    ln = lambda v: (mv(v[0]), mv(v[1]), v[2])      # noqa: E731
    kw = dict(post=ln(p["post"]), pos=(mv(p["pos"][0]), p["pos"][1], p["pos"][2]), next=ln(p["next"]), fold=fold)
    if not fold:
        kw["head"] = (mv(p["head"][0]), mv(p["head"][1]))
    return kw


def _rowln_run(p, x, r, mode, fold, ri, in_place, **more):
    from pafuse_amd import ops
    xd, wd, bd = _dev(x, p["w"], p["b"])
    return ops.linear_rowln(xd, wd, bd, r.to(DEV).clone(), MODES[mode], resid_image=ri, in_place=in_place, **_rowln_options(p, fold), **more)


def _check_rowln(clean, got, ref, what, kind="nan"):
    """every output against the reference output of its name; the decoded images against the fp32 output they stand for"""
    assert set(clean) == set(got)
    for name in clean:
        _check(clean[name], got[name], torch.isnan(ref[name.replace("_img", "")]), f"{what} {name}", kind)


@pytest.mark.parametrize("M", (33, 129))
@pytest.mark.parametrize("route", routes(), ids=route_id)
def test_whole_row_layers_keep_a_nonfinite_value_in_its_row(route, M):
    """ops.linear_rowln on every route with the full chain (post, pos, next + head; folded: the statistics), in place and out of
    place: a NaN at x[row] or resid[row], row 0 and M - 1 (+inf and, in f16x2, 1e5 at x): x, n, stats, head and the decoded
    images are NaN (non-finite) in that row and keep the clean run's bits in every other."""
    mode, N, ri = route
    K = 2 * N
    p = _rowln_case(M, N, K, 3 * N + M + mode)
    k, n = K // 2 + 3, N // 2 + 1
    assert _no_zero(p["w"][:, k], p["post"][0], p["next"][0], p["head"][0])
    for fold in ((True,) if ri else (False, True)):          # (the centred-image residual exists with the fold only)
        if ri:
            p["r"] = p["r"] - p["r"].mean(1, keepdim=True)
        for in_place in (False, True):
            clean = _rowln_run(p, p["x"], p["r"], mode, fold, ri, in_place)
            for row in (0, M - 1):
                for name, kinds in (("x", ("nan", "inf", "1e5") if mode == 3 else ("nan", "inf")), ("resid", ("nan",))):
                    for kind in kinds:
                        plant = lambda v: (_planted(p["x"], (row, k), v), p["r"]) if name == "x" else (p["x"], _planted(p["r"], (row, n), v))  # noqa: E731
                        got = _rowln_run(p, *plant(KIND[kind]), mode, fold, ri, in_place)
                        ref = host.rowln_ref(*plant(NAN)[:1], p["w"], p["b"], plant(NAN)[1], **_rowln_options(p, fold, dev=False))
                        assert torch.equal(torch.isnan(ref["x"]), _row_mask(ref["x"].shape, row))
                        _check_rowln(clean, got, ref, f"rowln {route_id(route)} M={M} fold={fold} in_place={in_place} {name}[{row}] {kind}", kind)


@pytest.mark.parametrize("mode,N", [(m, n) for m in (0, 2) for n in WIDTHS])
def test_whole_row_training_route_keeps_a_nan_row_factor_in_its_sequence(mode, N):
    """EPI_ROWLN_TRAIN: y = resid + rowscale[seq(m)] (x W^T + b), temporal map.  A NaN in rowscale[sequence] makes that
    sequence's rows NaN in pre, x, n and head; a NaN in x[row] / resid[row] that row; nothing else changes."""
    M, F_, J = 129, 4, 5
    p = _rowln_case(M, N, N, 7 * N + mode)
    nseq = -(-M // (F_ * J)) * J
    rs = 0.5 + torch.rand(nseq, generator=_gen(N))
    assert _no_zero(p["w"][:, 3], rs)
    kw = dict(training=True, rs_map=(1, J, F_ * J))
    clean = _rowln_run(p, p["x"], p["r"], mode, False, False, False, rowscale=rs.to(DEV), **kw)
    for what, x, r, s in (("rowscale", p["x"], p["r"], _planted(rs, J + 2)), ("x", _planted(p["x"], (M - 1, 3)), p["r"], rs),
                          ("resid", p["x"], _planted(p["r"], (0, 3)), rs)):
        got = _rowln_run(p, x, r, mode, False, False, False, rowscale=s.to(DEV), **kw)
        ref = host.rowln_ref(x, p["w"], p["b"], r, rowscale=s, **kw, **_rowln_options(p, False, dev=False))
        if what == "rowscale":
            assert torch.equal(torch.isnan(ref["pre"])[:, 0], host.seq_of_row(M, 1, J, F_ * J) == J + 2)
        _check_rowln(clean, got, ref, f"rowln training {MODES[mode]}-{N} NaN in {what}")


@pytest.mark.parametrize("fold", [False, True])
def test_grouped_whole_row_layers_keep_a_nan_in_its_layer_and_row(fold):
    """linear_rowln_group on the shared grid (grouped_rowln_kernel): three layers in one launch, a NaN in one row of the middle
    layer's x - that row of that layer, and neither of the other layers."""
    from pafuse_amd import ops
    cases = [_rowln_case(M, N, 2 * N, 11 * N + M) for N, M in ((256, 129), (384, 33), (256, 65))]

    def layers(xs):
        return [dict(x=x.to(DEV), weight=p["w"].to(DEV), bias=p["b"].to(DEV), resid=p["r"].to(DEV), precision="bf16x3", **_rowln_options(p, fold))
                for p, x in zip(cases, xs)]
    xs = [p["x"] for p in cases]
    clean = ops.linear_rowln_group(layers(xs), shared_grid=True)
    for row in (0, 32):
        bad = [xs[0], _planted(xs[1], (row, 5)), xs[2]]
        got = ops.linear_rowln_group(layers(bad), shared_grid=True)
        ref = host.rowln_ref(bad[1], cases[1]["w"], cases[1]["b"], cases[1]["r"], **_rowln_options(cases[1], fold, dev=False))
        _check_rowln(clean[1], got[1], ref, f"grouped rowln fold={fold} layer 1 row {row}")
        for i in (0, 2):
            for name in clean[i]:
                _check_same(clean[i][name], got[i][name], f"grouped rowln fold={fold} layer {i} {name}")


# ------------------------------------------------------------------------------------------------------------ 6. fused MLP
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("M", (129, 300))
@pytest.mark.parametrize("C_", (224, 256, 384))
def test_fused_mlp_keeps_a_nonfinite_value_in_its_row(C_, M, in_place):
    """hmlp_kernel: NaN, +inf, 1e5 in xc[row] and NaN in rstd[row] at row 0, a middle row and M - 1: y (decoded from the H image)
    and stats are NaN (non-finite) in that row only - nothing is swallowed through the GELU, nothing reaches the tile's other rows."""
    from pafuse_amd import ops
    g = _gen(3 + C_ + M)
    x = _randn(g, M, C_)
    xc = x - x.mean(1, keepdim=True)
    rstd = (1.0 / torch.sqrt(xc.double().pow(2).mean(1) + 1e-6)).float()
    W1, b1 = _randn(g, 2 * C_, C_, scale=C_ ** -0.5), _randn(g, 2 * C_, scale=0.1)
    W2, b2 = _randn(g, C_, 2 * C_, scale=(2 * C_) ** -0.5), _randn(g, C_, scale=0.1)
    ch = C_ // 2 + 5
    assert _no_zero(W1[:, ch], rstd, W2)
    run = lambda a, s: ops.mlp_fused(*_dev(a, s, W1, b1, W2, b2), in_place=in_place)      # noqa: E731
    clean = run(xc, rstd)
    for row in (0, 70, M - 1):
        for what, kind in (("xc", "nan"), ("xc", "inf"), ("xc", "1e5"), ("rstd", "nan")):
            a, s = (_planted(xc, (row, ch), KIND[kind]), rstd) if what == "xc" else (xc, _planted(rstd, row))
            got = run(a, s)
            ref = host.mlp_ref(_planted(xc, (row, ch)) if what == "xc" else xc, s, W1, b1, W2, b2)
            for name, c, o, r in zip(("y", "stats"), clean, got, ref):
                assert torch.equal(torch.isnan(r), _row_mask(r.shape, row))
                _check(c, o, torch.isnan(r), f"mlp_fused C={C_} M={M} in_place={in_place} {what}[{row}] {kind} {name}", kind)


# ---------------------------------------------------------------------------------------------------- 7. training backward
@pytest.mark.parametrize("M", (129, 4097))
@pytest.mark.parametrize("image_source", (0, 1))
@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_input_gradient_keeps_a_nan_in_its_row(precision, image_source, M):
    """ops.linear_input_grad with dact_u (the dX GEMM of fc2, C = 256): a NaN in dy[row] makes that row of dX NaN, a NaN in
    dact_u[row, k] that element; rows 0 and M - 1."""
    from pafuse_amd import ops
    N, K = 256, 512
    g = _gen(M + image_source)
    dy, w, u = _randn(g, M, N), _randn(g, N, K, scale=N ** -0.5), _randn(g, M, K)
    assert _no_zero(w[7], u[0], u[M - 1], dy[0], dy[M - 1])
    run = lambda d, a: ops.linear_input_grad(*_dev(d, w, a), precision, image_source)      # noqa: E731
    clean = run(dy, u)
    for row in (0, M - 1):
        for what, d, a in (("dy", _planted(dy, (row, 7)), u), ("dact_u", dy, _planted(u, (row, 9)))):
            _check(clean, run(d, a), torch.isnan(host.input_grad_ref(d, w, a)), f"input_grad {precision} src={image_source} M={M} {what}[{row}]")


@pytest.mark.parametrize("N,K,M", ((768, 256, 4696), (200, 72, 389), (256, 512, 37)))
@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_weight_gradient_keeps_a_nan_in_its_row_or_column(precision, N, K, M):
    """ops.linear_weight_grad: a NaN at dy[m, n] is exactly row n of dW and db[n]; at x[m, k] exactly column k of dW with db
    untouched; m once in the first and once in the last split-K chunk."""
    from pafuse_amd import ops
    g = _gen(N + K + M)
    dy, x = _randn(g, M, N), _randn(g, M, K)
    assert _no_zero(dy[1], dy[M - 2], x[1], x[M - 2])
    clean = ops.linear_weight_grad(*_dev(dy, x), precision)
    n, k = N - 3, K // 2 + 1
    for m in (1, M - 2):
        for what, d, a in (("dy", _planted(dy, (m, n)), x), ("x", dy, _planted(x, (m, k)))):
            got = ops.linear_weight_grad(*_dev(d, a), precision)
            ref = host.weight_grad_ref(d, a)
            tag = f"weight_grad {precision} ({N},{K},{M}) {what}[{m}]"
            _check(clean[0], got[0], torch.isnan(ref[0]), tag + " dW")
            if what == "dy":
                _check(clean[1], got[1], torch.isnan(ref[1]), tag + " db")
            else:
                assert not bool(torch.isnan(ref[1]).any())
                _check_same(clean[1], got[1], tag + " db")


@pytest.mark.parametrize("M", (65, 1985))
@pytest.mark.parametrize("C_", (384, 224, 130, 768))
def test_layer_norm_backward_keeps_a_nan_in_its_row_and_column(C_, M):
    """ops.layer_norm_backward with add, drop, scaled, branch: a NaN in dy[m, c] is row m of dx / out_scaled and column c of
    dw / db; a NaN in x[m, c] row m of dx / out_scaled, ALL of dw, and db untouched.  dbranch is the column sums of out_scaled,
    whose row m is NaN in every column: the fp64 reference has all of dbranch NaN in both cases, and so must the kernel."""
    from pafuse_amd import ops
    J = 5
    g = _gen(C_ + M)
    dy, x, w, add = _randn(g, M, C_), _randn(g, M, C_), 1 + _randn(g, C_, scale=0.1), _randn(g, M, C_)
    drop = 0.5 + torch.rand(-(-M // J), generator=g)
    assert _no_zero(dy[0], dy[M - 1], x[0], x[M - 1], dy[:, C_ - 2], x[:, C_ - 2], w, drop)
    run = lambda d, a: ops.layer_norm_backward(*_dev(d, a, w), 1e-6, add=add.to(DEV), drop=drop.to(DEV), seq_map=(0, J, 1), scaled=True, branch=True)  # noqa: E731
    clean = run(dy, x)
    for m in (0, M - 1):
        c = C_ - 2
        for what, d, a in (("dy", _planted(dy, (m, c)), x), ("x", dy, _planted(x, (m, c)))):
            got = run(d, a)
            ref = host.ln_backward_ref(d, a, w, 1e-6, add, drop, (0, J, 1))
            tag = f"ln_backward C={C_} M={M} {what}[{m}]"
            for name in ("dx", "out_scaled") + (("dw", "db") if what == "dy" else ()):
                _check(clean[name], got[name], torch.isnan(ref[name]), f"{tag} {name}")
            # dbranch = the column sums of out_scaled, whose row m is NaN in every column: all of it, in the reference and here
            assert bool(torch.isnan(ref["dbranch"]).all()) and bool(torch.isnan(got["dbranch"]).all()), tag
            if what == "x":
                assert bool(torch.isnan(ref["dw"]).all()) and not bool(torch.isnan(ref["db"]).any())
                assert bool(torch.isnan(got["dw"]).all()), tag
                _check_same(clean["db"], got["db"], f"{tag} db")


@pytest.mark.parametrize("N", (448, 768))
def test_gelu_backward_keeps_a_nan_in_its_element_and_column(N):
    from pafuse_amd import ops
    M = 129
    g = _gen(N)
    u, dh = _randn(g, M, N), _randn(g, M, N)
    assert _no_zero(u[M - 1], dh[M - 1], u[0], dh[0])
    clean = ops.gelu_backward(*_dev(u, dh))
    for what, a, d in (("u", _planted(u, (M - 1, 5)), dh), ("dh", u, _planted(dh, (0, N - 1)))):
        got = ops.gelu_backward(*_dev(a, d))
        ref = host.gelu_backward_ref(a, d)
        assert int(torch.isnan(ref[0]).sum()) == 1
        for name, c, o, r in zip(("du", "db"), clean, got, ref):
            _check(c, o, torch.isnan(r), f"gelu_backward N={N} NaN in {what}: {name}")


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_group_sum_keeps_a_nan_in_its_group(mode):
    from pafuse_amd import ops
    B, F_, J, C_ = 3, 5, 7, 224
    x = _randn(_gen(mode), B, F_, J, C_)
    clean = ops.train_group_sum(x.to(DEV), mode)
    for index in ((0, 0, 0, 0), (B - 1, F_ - 1, J - 1, C_ - 1), (1, 3, 4, 100)):
        bad = _planted(x, index)
        ref = host.group_sum_ref(bad, mode)
        assert int(torch.isnan(ref).sum()) == 1
        _check(clean, ops.train_group_sum(bad.to(DEV), mode), torch.isnan(ref), f"group_sum mode {mode} NaN at {index}")


# ------------------------------------------------------------------------------------------------------ 8. the elementwise rim
@pytest.mark.parametrize("C_", (384, 224))
def test_layer_norm_keeps_a_nan_in_its_row(C_):
    from pafuse_amd import ops
    M = 65
    g = _gen(C_)
    x, w, b = _randn(g, M, C_), 1 + _randn(g, C_, scale=0.1), _randn(g, C_, scale=0.1)
    clean = ops.layer_norm(*_dev(x, w, b), 1e-6)
    for row in (0, 31, M - 1):
        bad = _planted(x, (row, C_ - 1))
        _check(clean, ops.layer_norm(*_dev(bad, w, b), 1e-6), torch.isnan(host.layer_norm_ref(bad, w, b, 1e-6)), f"layer_norm C={C_} row {row}")


EMBED_NAN_FORMS = [("f32", False, False), ("bf16x3", True, False), ("f16x2", True, False), ("bf16x3_images", True, False)]


@pytest.mark.parametrize("form", EMBED_NAN_FORMS, ids=lambda f: f[0] + ("-folded" if f[1] else ""))
def test_embed_keeps_a_nan_in_its_tokens(form):
    """ops.embed_unit, the plain form and one image form per mode, with the flipped half and the clamp: a NaN in x2d of one
    (clip, frame, joint) reaches that token of every hypothesis of the clip, a NaN in x3d of one hypothesis that token alone (in
    the flipped half: at the mirrored joint) - torch.clamp keeps a NaN, and so must the kernel's."""
    from pafuse_amd import ops
    from tests import loop_rim_reference as rim
    from tests.test_hip_loop_rim import embed_inputs
    precision, folded, h_only = form
    C_ = 64
    t = embed_inputs(rim.EMBED_DIMS[0], C_, True, 5)
    M = t["M"]
    assert _no_zero(t["pw"])

    def run(x3d, x2d):
        d = t["dev"]
        out = ops.embed_unit(x3d.to(DEV), x2d.to(DEV), d["pw"], d["pb"], d["pos"], d["temb"], d["nw"], d["nb"], 1e-6, perm=d["perm"],
                             x2d_flip=d["x2f"], do_clamp=True, scale=1.0, precision=precision, folded=folded, h_residual_only=h_only)
        if "image" in out:
            out["image"] = (ops.hjoin_rows if precision == "f16x2" else ops.xjoin_rows)(out["image"], M, C_)
        return out

    clean = run(t["x3d"], t["x2d"])
    for what, x3d, x2d in (("x2d", t["x3d"], _planted(t["x2d"], (1, 2, 3, 0))), ("x3d", _planted(t["x3d"], (0, 1, 1, 2, 1)), t["x2d"])):
        got = run(x3d, x2d)
        r = rim.embed_ref(x3d, x2d, t["pw"], t["pb"], t["pos"], t["temb"], t["nw"], t["nb"], 1e-6, perm=t["perm"], x2d_flip=t["x2f"], scale=1.0)
        rows = torch.isnan(r["x"]).reshape(M, C_)
        ref = {"x": rows, "xn": rows, "image": rows, "stats": rows[:, :2]}
        assert int(rows[:, 0].sum()) == (3 if what == "x2d" else 2)      # x2d: P tokens of the plain half; x3d: one per half
        assert set(got) == set(clean)
        for name in clean:
            _check(clean[name], got[name], ref[name], f"embed {form} NaN in {what}: {name}")


def test_time_embed_carries_a_nan_bias_through_the_gelu():
    """a NaN cannot enter through t; one in b1 (the bias of the first linear layer) is in every row's hidden vector, and every
    output element must be NaN: nothing swallows it through the GELU (the reference: all NaN as well)"""
    import pafuse_amd
    from pafuse_amd import ops
    from tests import loop_rim_reference as rim
    from tests.golden import golden_util as gu
    C_ = 224
    t = torch.tensor(rim.TIME_STEPS)
    outs = []
    for poisoned in (False, True):
        m = pafuse_amd.MixSTE2(2, 2, 5, C_, 1, 8, drop_path_rate=0.0, is_train=False)
        sd = {k: gu.seeded_tensor(f"nonfinite.{C_}.time_mlp.{k}", v.shape, 31) for k, v in m.time_mlp.state_dict().items()}
        if poisoned:
            sd["1.bias"][C_ + 1] = NAN
        m.time_mlp.load_state_dict(sd)
        ref = rim.time_embed_ref(t, m._freqs.clone(), sd["1.weight"], sd["1.bias"], sd["3.weight"], sd["3.bias"])
        outs.append((ops.time_embed(m.to(DEV), t.to(DEV)).cpu(), ref))
    (clean, clean_ref), (got, ref) = outs
    assert _no_zero(sd["3.weight"][:, C_ + 1])
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(clean_ref).all())
    assert bool(torch.isnan(ref).all())
    print(f"time_embed: {int(torch.isnan(got).sum())} of {got.numel()} NaN")
    assert bool(torch.isnan(got).all())


# ------------------------------------------------------------------------------------------------------ 9. the loop, f16x2
def test_f16x2_loop_raises_on_a_nan_input_and_the_flag_does_not_stick():
    """'f16x2' at B = 2, P = 2: a NaN in x2d of clip 1 stays non-finite through every kernel down to finalize, which raises the
    range flag - D3DP raises PafuseError ('fp16 range') rather than return a pose; the same model on the clean inputs afterwards
    returns the bits it returned before (the flag is per call)."""
    from __graft_entry__ import make_model
    from pafuse_amd._lib import PafuseError
    from tests.golden import golden_util as gu
    B, P, T = 2, 2, 2
    model, _ = make_model(P, T, seed=59)
    model.precision = "f16x2"
    x2d, x2f = gu.synthetic_inputs_2d(B=B, seed=1234)
    noises = gu.synthetic_noises(B=B, P=P, n=T, seed=9)
    model.noise_fn = lambda k, shape, device: noises[k]
    clean = model(x2d.to(DEV), None, input_2d_flip=x2f.to(DEV)).cpu()
    assert bool(torch.isfinite(clean).all())
    bad2d = _planted(x2d, (1, 5, 7, 0))
    with pytest.raises(PafuseError, match="fp16 range"):
        model(bad2d.to(DEV), None, input_2d_flip=x2f.to(DEV))
    _check_same(clean, model(x2d.to(DEV), None, input_2d_flip=x2f.to(DEV)).cpu(), "f16x2 loop after the raise")

"""Where a single NaN goes in each operation of the project, stated in plain fp64 torch: the reference evaluators of
tests/test_hip_nonfinite.py and, asserted here on a machine without a GPU (and without the library), the NaN masks they give
per op family.  The GPU module holds every HIP kernel to exactly these masks, so its expectations rest on something that runs
everywhere:

  linear / fused MLP / whole-row chain    x[m, k] -> row m of every output (and of stats / head), nothing else
  fused qkv + attention                   x[token, c] or rstd[token] -> the token's whole sequence, all heads
  attention forward                       q[s, t, h, c] -> (s, h, row t);  k[s, t, h, c] -> (s, h, all rows);
                                          v[s, t, h, c] -> (s, h, all rows, channel c)
  attention backward (fp64 autograd)      d_o / q / k / v of (s, h) -> inside (s, h) of dq | dk | dv only
  weight gradient                         dy[m, n] -> row n of dW and db[n];  x[m, k] -> column k of dW, db clean
  input gradient                          dy[m, n] -> row m of dX;  dact_u[m, k] -> the element (m, k)
  LayerNorm backward                      dy[m, c] -> row m of dx / out_scaled, column c of dw / db;
                                          x[m, c]  -> row m of dx / out_scaled, all of dw, db clean;
                                          dbranch = the column sums of out_scaled, whose row m is NaN: all of it, both times
  GELU backward / group sums / LayerNorm  the element and its db column / the element's group / the row

Every evaluator takes CPU tensors of any float dtype and computes in float64.  Nothing here is fitted to a kernel.
"""
import pytest
import torch
import torch.nn.functional as F

NAN = float("nan")


def f64(t):
    return None if t is None else t.detach().double()


# --------------------------------------------------------------------------------------------------------- the evaluators
def linear_ref(x, w, b, act=None):
    y = f64(x) @ f64(w).t() + f64(b)
    return F.gelu(y) if act == "gelu" else y


def attention_ref(qkv, heads, rows):
    """softmax(q k^T d^-1/2) v per sequence and head, rows [nseq, L] = the token rows of every sequence; [M, C], rows no
    sequence owns 0 (autograd-able: qkv may require grad)"""
    qkv = qkv.double()
    M, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    nseq, L = rows.shape
    x = qkv[rows].reshape(nseq, L, 3, heads, d)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                      # [nseq, heads, L, d]
    p = torch.softmax(q @ k.transpose(-2, -1) * d ** -0.5, dim=-1)
    o = torch.zeros(M, C, dtype=torch.float64)
    return o.index_put((rows.reshape(-1),), (p @ v).transpose(1, 2).reshape(nseq * L, C))


def attention_backward_ref(qkv, d_o, heads, rows):
    """dqkv [M, 3C] by fp64 autograd of attention_ref"""
    q64 = f64(qkv).requires_grad_(True)
    attention_ref(q64, heads, rows).backward(f64(d_o))
    return q64.grad


def qkv_attention_ref(x, w, b, heads, rows, rstd=None):
    """the fused kernel's function: qkv = rstd (x W^T) + b, then attention_ref"""
    y = f64(x) @ f64(w).t()
    if rstd is not None:
        y = y * f64(rstd)[:, None]
    return attention_ref(y + f64(b), heads, rows)


def layer_norm_ref(x, w, b, eps):
    x = f64(x)
    return F.layer_norm(x, (x.shape[-1],), f64(w), f64(b), eps)


def seq_of_row(M, temporal, J, FJ):
    m = torch.arange(M)
    return (m // FJ) * J + m % J if temporal else m // J


def rowln_ref(x, w, b, resid, post=None, pos=None, next=None, head=None, fold=False, rowscale=None, rs_map=(0, 1, 1),
              training=False):
    """one whole-row layer: y = x W^T + b + resid (training: resid + rowscale[seq(m)] (x W^T + b), 'pre'), post-norm, pos,
    then next-norm 'n' (+ 'head') or, folded, 'stats' = (mean, rstd) of the row and 'x' centred on that mean"""
    acc = f64(x) @ f64(w).t() + f64(b)
    M, N = acc.shape
    if training and rowscale is not None:
        acc = acc * f64(rowscale)[seq_of_row(M, *rs_map)][:, None]
    y = acc + f64(resid)
    out = {"pre": y} if training else {}
    z = y
    if post is not None:
        z = layer_norm_ref(z, post[0], post[1], post[2])
    if pos is not None:
        tab, pj, pf = pos
        z = z + f64(tab)[(torch.arange(M) // pj) % pf]
    out["x"] = z
    if next is not None:
        if fold:
            mu = z.mean(1, keepdim=True)
            out["stats"] = torch.cat((mu, 1 / torch.sqrt(((z - mu) ** 2).mean(1, keepdim=True) + next[2])), dim=1)
            out["x"] = z - mu
        else:
            out["n"] = layer_norm_ref(z, *next)
            if head is not None:
                out["head"] = out["n"] @ f64(head[0]).t() + f64(head[1])
    return out


def mlp_ref(xc, rstd, w1, b1, w2, b2, eps=1e-6):
    """(y - mean(y), stats [M, 2] = (mean, rstd) of y), y = xc + GELU(rstd (xc W1^T) + b1) W2^T + b2"""
    xc = f64(xc)
    u = xc @ f64(w1).t()
    if rstd is not None:
        u = u * f64(rstd)[:, None]
    y = xc + F.gelu(u + f64(b1)) @ f64(w2).t() + f64(b2)
    mu = y.mean(1, keepdim=True)
    return y - mu, torch.cat((mu, 1 / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + eps)), dim=1)


def gelu_grad(u):
    u = f64(u).requires_grad_(True)
    F.gelu(u).sum().backward()
    return u.grad


def input_grad_ref(dy, w, dact_u=None):
    dx = f64(dy) @ f64(w)
    return dx if dact_u is None else dx * gelu_grad(dact_u)


def weight_grad_ref(dy, x):
    return f64(dy).t() @ f64(x), f64(dy).sum(0)


def ln_backward_ref(dy, x, w, eps, add=None, drop=None, seq_map=(0, 1, 1)):
    """fp64 autograd of layer_norm: dx (+ add), dw, db and - with drop [nseq] - out_scaled = drop[seq(m)] dx, dbranch = its
    column sums"""
    M, C = x.shape
    x64, w64 = f64(x).requires_grad_(True), f64(w).requires_grad_(True)
    b64 = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (C,), w64, b64, eps).backward(f64(dy))
    out = {"dx": x64.grad + (f64(add) if add is not None else 0.0), "dw": w64.grad, "db": b64.grad}
    if drop is not None:
        out["out_scaled"] = f64(drop)[seq_of_row(M, *seq_map)][:, None] * out["dx"]
        out["dbranch"] = out["out_scaled"].sum(0)
    return out


def gelu_backward_ref(u, dh):
    du = f64(dh) * gelu_grad(u)
    return du, du.sum(0)


def group_sum_ref(x, mode):
    """x [B, F, J, C] summed over the rows of each group: mode 0 per joint [J, C], 1 per frame [F, C], 2 per sample [B, C]"""
    return f64(x).sum(((0, 1), (0, 2), (1, 2))[mode])


# ------------------------------------------------------------------------------------------- what the GPU module asserts
def nan_mask(ref):
    return torch.isnan(ref)


def mask_within_its_conditions(mask):
    """the reference's mask is neither empty nor everything: the case is not vacuous"""
    return bool(mask.any()) and not bool(mask.all())


def first_difference(a, b):
    """(count, first index, the two values) where two fp32 tensors differ in their BITS (-0.0 and NaN payloads count)"""
    bad = (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).nonzero()
    if bad.shape[0] == 0:
        return None
    i = tuple(bad[0].tolist())
    return bad.shape[0], list(i), float(a[i]), float(b[i])


# ---------------------------------------------------------------------------------------------------------------- tests
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rows(nseq, L):
    return torch.arange(nseq * L).reshape(nseq, L)


def test_linear_mask_is_the_row():
    g = _g(1)
    x, w, b = torch.randn(9, 16, generator=g), torch.randn(12, 16, generator=g), torch.randn(12, generator=g)
    for act in (None, "gelu"):
        x2 = x.clone()
        x2[4, 3] = NAN
        want = torch.zeros(9, 12, dtype=torch.bool)
        want[4] = True
        assert torch.equal(nan_mask(linear_ref(x2, w, b, act)), want)
        assert mask_within_its_conditions(want)


def test_fused_qkv_attention_mask_is_the_sequence_all_heads():
    g = _g(2)
    nseq, L, C, heads = 4, 5, 12, 3
    x, w, b = torch.randn(nseq * L, C, generator=g), torch.randn(3 * C, C, generator=g), torch.randn(3 * C, generator=g)
    rstd = 0.5 + torch.rand(nseq * L, generator=g)
    want = torch.zeros(nseq * L, C, dtype=torch.bool)
    want[2 * L:3 * L] = True
    x2 = x.clone()
    x2[2 * L + 1, 7] = NAN
    assert torch.equal(nan_mask(qkv_attention_ref(x2, w, b, heads, _rows(nseq, L), rstd)), want)
    r2 = rstd.clone()
    r2[3 * L - 1] = NAN
    assert torch.equal(nan_mask(qkv_attention_ref(x, w, b, heads, _rows(nseq, L), r2)), want)


@pytest.mark.parametrize("which", ["q", "k", "v"])
def test_attention_forward_masks(which):
    g = _g(3)
    nseq, L, heads, d = 3, 6, 2, 4
    C = heads * d
    qkv = torch.randn((nseq + 1) * L, 3 * C, generator=g)                  # a spare sequence of rows nobody owns
    s, t, h, c = 1, 4, 1, 2
    qkv[s * L + t, "qkv".index(which) * C + h * d + c] = NAN
    mask = nan_mask(attention_ref(qkv, heads, _rows(nseq, L))).reshape(nseq + 1, L, heads, d)
    want = torch.zeros_like(mask)
    if which == "q":
        want[s, t, h, :] = True                                              # (sequence, head, row)
    elif which == "k":
        want[s, :, h, :] = True                                              # (sequence, head, all rows)
    else:
        want[s, :, h, c] = True                                              # (sequence, head, all rows, one channel)
    assert torch.equal(mask, want)


@pytest.mark.parametrize("which", ["d_o", "q", "k", "v"])
def test_attention_backward_mask_stays_in_its_sequence_and_head(which):
    g = _g(4)
    nseq, L, heads, d = 3, 5, 2, 4
    C = heads * d
    qkv, d_o = torch.randn(nseq * L, 3 * C, generator=g), torch.randn(nseq * L, C, generator=g)
    s, t, h, c = 2, 1, 0, 3
    if which == "d_o":
        d_o[s * L + t, h * d + c] = NAN
    else:
        qkv[s * L + t, "qkv".index(which) * C + h * d + c] = NAN
    mask = nan_mask(attention_backward_ref(qkv, d_o, heads, _rows(nseq, L))).reshape(nseq, L, 3, heads, d)
    inside = torch.zeros_like(mask)
    inside[s, :, :, h, :] = True
    assert bool(mask.any()) and not bool((mask & ~inside).any())
    if which == "d_o":                                                       # dv: one channel; dq: the row; dk: all of (s, h)
        assert bool(mask[s, :, 2, h, c].all()) and int(mask[s, :, 2, h].sum()) == L
        assert bool(mask[s, t, 0, h].all()) and int(mask[s, :, 0, h].sum()) == d and bool(mask[s, :, 1, h].all())


def test_weight_gradient_masks_are_a_row_or_a_column():
    g = _g(5)
    M, N, K = 11, 6, 7
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    d2 = dy.clone()
    d2[3, 4] = NAN
    dw, db = weight_grad_ref(d2, x)
    assert torch.equal(nan_mask(dw), torch.arange(N)[:, None].eq(4).expand(N, K))
    assert torch.equal(nan_mask(db), torch.arange(N).eq(4))
    x2 = x.clone()
    x2[9, 2] = NAN
    dw, db = weight_grad_ref(dy, x2)
    assert torch.equal(nan_mask(dw), torch.arange(K)[None, :].eq(2).expand(N, K)) and not bool(nan_mask(db).any())


def test_input_gradient_masks():
    g = _g(6)
    M, N, K = 7, 6, 5
    dy, w, u = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g), torch.randn(M, K, generator=g)
    d2 = dy.clone()
    d2[2, 1] = NAN
    assert torch.equal(nan_mask(input_grad_ref(d2, w, u)), torch.arange(M)[:, None].eq(2).expand(M, K))
    u2 = u.clone()
    u2[5, 3] = NAN
    want = torch.zeros(M, K, dtype=torch.bool)
    want[5, 3] = True
    assert torch.equal(nan_mask(input_grad_ref(dy, w, u2)), want)


def test_layer_norm_backward_pattern():
    g = _g(7)
    M, C, J = 12, 8, 3
    dy, x, w = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g), 1 + 0.1 * torch.randn(C, generator=g)
    add, drop = torch.randn(M, C, generator=g), 0.5 + torch.rand(M // J, generator=g)
    row = torch.arange(M)[:, None].eq(5).expand(M, C)
    col = torch.arange(C).eq(6)
    d2 = dy.clone()
    d2[5, 6] = NAN
    r = ln_backward_ref(d2, x, w, 1e-6, add, drop, (0, J, 1))
    assert torch.equal(nan_mask(r["dx"]), row) and torch.equal(nan_mask(r["out_scaled"]), row)
    assert all(torch.equal(nan_mask(r[k]), col) for k in ("dw", "db"))
    assert bool(nan_mask(r["dbranch"]).all())                                # column sums of out_scaled, whose row 5 is NaN
    x2 = x.clone()
    x2[5, 6] = NAN
    r = ln_backward_ref(dy, x2, w, 1e-6, add, drop, (0, J, 1))
    assert torch.equal(nan_mask(r["dx"]), row) and bool(nan_mask(r["dw"]).all()) and not bool(nan_mask(r["db"]).any())
    assert bool(nan_mask(r["dbranch"]).all())                                # column sums of out_scaled, whose row 5 is NaN


def test_whole_row_chain_and_mlp_masks_are_the_row():
    g = _g(8)
    M, N, K = 10, 8, 16
    x, w, b, r = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ln = lambda: (1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g), 1e-6)      # noqa: E731
    kw = dict(post=ln(), pos=(torch.randn(3, N, generator=g), 2, 3), next=ln(), head=(torch.randn(3, N, generator=g), torch.randn(3, generator=g)))
    for name in ("x", "resid"):
        x2, r2 = x.clone(), r.clone()
        (x2 if name == "x" else r2)[7, 5] = NAN
        for fold in (False, True):
            out = rowln_ref(x2, w, b, r2, fold=fold, **kw)
            assert set(out) == ({"x", "stats"} if fold else {"x", "n", "head"})
            for k, v in out.items():
                assert torch.equal(nan_mask(v), torch.arange(M)[:, None].eq(7).expand_as(v)), (name, fold, k)
    rs = 0.5 + torch.rand(5, generator=g)
    rs[3] = NAN                                                              # spatial map, J = 2: rows 6 and 7
    out = rowln_ref(x, w, b, r, training=True, rowscale=rs, rs_map=(0, 2, 1), **kw)
    for k, v in out.items():
        assert torch.equal(nan_mask(v), (torch.arange(M)[:, None] // 2).eq(3).expand_as(v)), k
    w1, b1 = torch.randn(2 * N, N, generator=g), torch.randn(2 * N, generator=g)
    w2, b2 = torch.randn(N, 2 * N, generator=g), torch.randn(N, generator=g)
    xc, rstd = r - r.mean(1, keepdim=True), 0.5 + torch.rand(M, generator=g)
    for poison in ("xc", "rstd"):
        a, s = xc.clone(), rstd.clone()
        if poison == "xc":
            a[7, 1] = NAN
        else:
            s[7] = NAN
        for v in mlp_ref(a, s, w1, b1, w2, b2):
            assert torch.equal(nan_mask(v), torch.arange(M)[:, None].eq(7).expand_as(v)), poison


def test_elementwise_masks():
    g = _g(9)
    u, dh = torch.randn(6, 5, generator=g), torch.randn(6, 5, generator=g)
    d2 = dh.clone()
    d2[4, 2] = NAN
    du, db = gelu_backward_ref(u, d2)
    assert int(nan_mask(du).sum()) == 1 and bool(nan_mask(du)[4, 2]) and torch.equal(nan_mask(db), torch.arange(5).eq(2))
    x = torch.randn(2, 3, 4, 5, generator=g)
    x[1, 2, 3, 4] = NAN
    for mode, grp in ((0, 3), (1, 2), (2, 1)):
        m = nan_mask(group_sum_ref(x, mode))
        assert int(m.sum()) == 1 and bool(m[grp, 4])
    m = nan_mask(layer_norm_ref(x.reshape(24, 5), torch.ones(5), torch.zeros(5), 1e-6))
    assert torch.equal(m, torch.arange(24)[:, None].eq(23).expand(24, 5))


def test_bit_comparison_sees_signed_zero_and_payloads():
    a = torch.tensor([0.0, 1.0, NAN])
    b = torch.tensor([-0.0, 1.0, NAN])
    assert first_difference(a, a.clone()) is None
    assert first_difference(a, b)[:2] == (1, [0])
    c = a.clone()
    c.view(torch.int32)[2] = 0x7FC0DEAD
    assert first_difference(a, c)[:2] == (1, [2])

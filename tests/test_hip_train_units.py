"""Unit tests of the training step's LayerNorm backward, dX GEMMs, fc1 forward and GELU backward through their unit entries
(pafuse_layernorm_backward -> ln_backward, pafuse_linear_input_grad -> input_grad, pafuse_linear_train -> plain_linear,
pafuse_gelu_backward -> gelu_bwd: the host functions the step calls), against exact integers and fp64.

Error bounds.  u = 2^-24.  Accumulated roundings use the probabilistic bound of Higham & Mary (SIAM J. Sci. Comput. 41(5),
2019): a sum of n terms computed in fp32, in any order, is within gam(n) sum|terms| of the exact sum, gam(n) = LAM sqrt(n) u,
with probability >= 1 - 2 n exp(-LAM^2 / 2) per sum (LAM = 9), rounding errors taken as independent and mean-zero.  First-order
error terms are summed with their absolute values; a factor 1.01 covers the second-order ones.
  dX GEMM (each element): dX = dY W with an N-term contraction.  A bf16x3 product keeps every operand term above 2^-24 of
    |a w|: it drops a1 w2 + a2 w1 + a2 w2 <= (2 2^-8 2^-16 + 2^-32) |a w| < 2^-22 |a w| (PROD = 2^-22; fp32 products: u).  At
    most six products per k plus the zero bias are n = 6 N + 1 accumulated terms, their sum <= 1.01 S, S = |dY| |W|:
      e = PROD S + gam(6 N + 1) 1.01 S          with dact_u: |g| e + u |dX|, g the epilogue's gelu'(dact_u)
    (g itself is read out of the kernel by an identity-weight run on the same shape - dY = 1, W = 1 where k % N == n, so the
    product is exactly 1 and dX = g - and its accuracy is checked on its own against fp64 and torch's CPU fp32 GELU backward.)
  LayerNorm backward (rows x, dy; w; fp32 fixed-order sums over C; xh = (x - mu) rstd, g = dy w, c1 = mean g, c2 = mean g xh):
      mean:  em  = gam(C) mean|x| + 2 u |mu|                       rstd: rho = gam(C) / 2 + 4 u + (rstd em)^2   (relative)
      xh:    Exh = rstd (em + u |x - mu|) + |xh| (rho + u)
      c1:    dc1 = (gam(C) + u) mean|g| + 2 u |c1|                  c2: dc2 = (sum |g| Exh + (2 u + gam(C)) sum |g xh|) / C + 2 u |c2|
      t = g - c1 - xh c2:  dt = u |g| + dc1 + |c2| Exh + |xh| dc2 + 3 u (|g| + |c1| + |xh c2|)
      dx = add + rstd t:   E = 1.01 (rstd dt + rstd |t| rho) + u |rstd t| + u |dx|   (the last term with add only)
      dw = sum_m dy xh:    1.01 sum |dy| (Exh + u |xh|) + gam(M) sum |dy xh| + u |dw|;    db = sum dy: gam(M) sum |dy| + u |db|
      dbranch = column sums of the kernel's own out_scaled: gam(M) sum |out_scaled| + u |dbranch|
  GELU backward (gelu_backward_kernel, libm erff / expf, their ulp bounds taken as 4 and 2): du = dh (Phi(x) + x phi(x)):
      dPhi <= 0.5 8 u |erf| + 0.25 u + u Phi <= 6 u,   dphi <= phi (x^2 u / 2 + 6 u)
      E = |dh| (6 u + |x| phi (x^2 u / 2 + 7 u) + u |gelu'|) + u |du|;     db = sum du: sum E + gam(M) sum |du| + u |db|
Nothing here is fitted to a measurement.  Sensitivity: dX from one bf16 per operand (host emulation) must FAIL every bf16x3
bound - so the bounds would catch a dropped slice.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
LAM = 9.0
PROD = {0: U, 2: 2.0 ** -22}
MODES = {0: "f32", 2: "bf16x3"}
NAN_BITS = 0x7FC0DEAD
QUAD_WIDTHS = (384, 288, 256, 224, 128, 64)           # ln_backward_quad_kernel (C % 4 == 0, C <= 384)
GENERIC_WIDTHS = (130, 388, 512, 768)                 # ln_backward_kernel
LN_M = (1, 7, 8, 9, 63, 64, 65, 1984, 1985, 4097)     # 1984 / 1985: reduce_partials_kernel<1> -> <16> (31 -> 32 parts)
# the step at B = 37, F = 27: rows and channel width of the three parts (body 24 joints, face 68, hands 42)
STEP = {"body": (23976, 384), "face": (67932, 224), "hands": (41958, 256)}
DX_WIDTHS = (384, 224, 256, 128, 64)
DX_M = (1, 31, 127, 128, 129, 4097)
TIME_B = (1, 8, 37)


def gam(n):
    return LAM * math.sqrt(n) * U


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi, shape, generator=_gen(seed), device=DEV).float()


def _normal(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed), device=DEV) * scale


def _nan_filled(n):
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _untouched(t, start):
    tail = t.view(-1)[start:].view(torch.int32)
    return torch.equal(tail, torch.full_like(tail, NAN_BITS))


def assert_equal(out, ref, what):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if not torch.equal(out.double(), ref.double()):
        bad = (out.double() != ref.double()).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: "
                             f"{out.double()[tuple(bad[0])].item()} != {ref.double()[tuple(bad[0])].item()}")


def within(val, ref, bound, what):
    """every element within its bound; returns (max error / bound, mean error / mean bound)"""
    err = (val.double() - ref).abs()
    q = (err / bound).max().item()
    assert q <= 1.0, (what, q)
    return q, (err.mean() / bound.mean()).item()


REPORT = []


def report(line):
    REPORT.append(line)
    print(line)


# ================================================================================================ LayerNorm backward
def ln_rows(M, C, seed):
    """x ~ N(0, 1) with every 5th row at mean 300 and every 7th with a variance near eps (1e-6); dy ~ N(0, 1); w ~ 1 + N(0, 0.1)"""
    x = _normal((M, C), seed)
    x[2::5] += 300.0
    x[3::7] = 0.5 + _normal((len(range(3, M, 7)), C), seed + 1, 1e-3)
    dy = _normal((M, C), seed + 2)
    w = 1 + _normal((C,), seed + 3, 0.1)
    return x, dy, w


def lnb_ref(dy, x, w, eps, add=None):
    """fp64 LayerNorm backward (autograd of torch.nn.functional.layer_norm) and the bounds of the module docstring"""
    M, Cc = x.shape
    eps = float(torch.tensor(eps, dtype=torch.float32))          # the value the kernel adds
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = torch.zeros(Cc, dtype=torch.float64, device=DEV, requires_grad=True)
    torch.nn.functional.layer_norm(x64, (Cc,), w64, b64, eps).backward(dy.double())
    dx = x64.grad + (add.double() if add is not None else 0.0)
    xd, dyd = x.double(), dy.double()
    mu = xd.mean(1, keepdim=True)
    d = xd - mu
    rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    xh = d * rstd
    em = gam(Cc) * xd.abs().mean(1, keepdim=True) + 2 * U * mu.abs()
    rho = gam(Cc) / 2 + 4 * U + (rstd * em) ** 2
    exh = rstd * (em + U * d.abs()) + xh.abs() * (rho + U)
    g = dyd * w.double()
    ga = g.abs()
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dc1 = (gam(Cc) + U) * ga.mean(1, keepdim=True) + 2 * U * c1.abs()
    dc2 = ((ga * exh).sum(1, keepdim=True) + (2 * U + gam(Cc)) * (ga * xh.abs()).sum(1, keepdim=True)) / Cc + 2 * U * c2.abs()
    t = g - c1 - xh * c2
    dt = U * ga + dc1 + c2.abs() * exh + xh.abs() * dc2 + 3 * U * (ga + c1.abs() + (xh * c2).abs())
    edx = 1.01 * (rstd * dt + rstd * t.abs() * rho) + U * (rstd * t).abs() + (U * dx.abs() if add is not None else 0.0)
    dw, db = w64.grad, b64.grad
    edw = 1.01 * (dyd.abs() * (exh + U * xh.abs())).sum(0) + gam(M) * (dyd * xh).abs().sum(0) + U * dw.abs()
    edb = gam(M) * dyd.abs().sum(0) + U * db.abs()
    return dict(dx=dx, dw=dw, db=db, edx=edx, edw=edw, edb=edb)


def lnb(dy, x, w, eps=1e-6, **kw):
    from pafuse_amd import ops
    return ops.layer_norm_backward(dy, x, w, eps, **kw)


def check_lnb(M, C, seed, eps=1e-6):
    x, dy, w = ln_rows(M, C, seed)
    add = _normal((M, C), seed + 4)
    ref = lnb_ref(dy, x, w, eps, add)
    out = lnb(dy, x, w, eps, add=add)
    q = {k: within(out[k], ref[k], ref["e" + k], (M, C, k)) for k in ("dx", "dw", "db")}
    return q


@pytest.mark.parametrize("C", QUAD_WIDTHS + GENERIC_WIDTHS)
def test_layer_norm_backward_against_fp64(C):
    """dx, dw, db against fp64 under the derived bounds at every M of LN_M (a single row, ragged 64-row blocks, both
    reduce_partials forms), rows with large means and rows whose variance is near eps."""
    worst = {}
    for M in LN_M:
        for k, (qmax, qmean) in check_lnb(M, C, 1000 + M + C).items():
            worst[k] = max(worst.get(k, (0, 0)), (qmax, qmean))
    kernel = "quad" if C % 4 == 0 and C <= 384 else "generic"
    report(f"ln_backward C={C} ({kernel}): error / bound max (mean err / mean bound): " +
           ", ".join(f"{k} {a:.2e} ({b:.2e})" for k, (a, b) in worst.items()))


@pytest.mark.parametrize("part", list(STEP))
def test_layer_norm_backward_at_the_step_sizes(part):
    M, C = STEP[part]
    q = check_lnb(M, C, 7)
    report(f"ln_backward {part} M={M} C={C}: " + ", ".join(f"{k} {a:.2e} ({b:.2e})" for k, (a, b) in q.items()))


def seq_index(M, temporal, J, FJ):
    m = torch.arange(M, device=DEV)
    return (m // FJ) * J + m % J if temporal else m // J


@pytest.mark.parametrize("C,J", [(384, 24), (224, 68), (256, 42), (130, 24), (768, 42)])
def test_layer_norm_backward_bit_invariants(C, J):
    """out_scaled == fp32(drop[seq(m)] dx) bit for bit under both sequence maps (F = 27, a different factor per sequence);
    accumulation into non-zero dw / db / dbranch == fp32(init + fresh); add aliased to dx == separate buffers; add = None ==
    add = 0; a repeat run; a row's dx independent of where it sits; dbranch == column sums of out_scaled within gam(M); NaN
    guard rows past M (and past C in dw / db / dbranch) untouched."""
    F, B = 27, 2
    M, FJ = B * F * J, F * J
    x, dy, w = ln_rows(M, C, 31 + C)
    add = _normal((M, C), 32 + C)
    for temporal in (0, 1):
        nseq = B * J if temporal else B * F
        drop = 0.5 + torch.rand(nseq, generator=_gen(33 + temporal), device=DEV)
        assert drop.unique().numel() == nseq
        kw = dict(add=add, drop=drop, seq_map=(temporal, J, FJ), scaled=True, branch=True)
        fresh = lnb(dy, x, w, **kw)
        dx, sc = fresh["dx"], fresh["out_scaled"]
        assert_equal(sc, drop[seq_index(M, temporal, J, FJ)][:, None] * dx, (C, J, temporal, "out_scaled"))
        colsum = sc.double().sum(0)
        within(fresh["dbranch"], colsum, gam(M) * sc.double().abs().sum(0) + U * colsum.abs(), (C, J, "dbranch"))
        init = {k: _normal((C,), 40 + i) for i, k in enumerate(("dw", "db", "dbranch"))}
        acc = lnb(dy, x, w, out={k: v.clone() for k, v in init.items()}, **kw)
        for k in init:
            assert_equal(acc[k], init[k] + fresh[k], (C, J, temporal, k, "accumulate"))
        assert_equal(acc["dx"], dx, (C, J, "dx with accumulation"))
        alias = add.clone()
        al = lnb(dy, x, w, add=alias, drop=drop, seq_map=(temporal, J, FJ), scaled=True, branch=True, out={"dx": alias})
        for k in ("dx", "out_scaled", "dw", "db", "dbranch"):
            assert_equal(al[k], fresh[k], (C, J, temporal, k, "add aliased to dx"))
        rep = lnb(dy, x, w, **kw)
        for k in ("dx", "out_scaled", "dw", "db", "dbranch"):
            assert torch.equal(rep[k], fresh[k]), (C, J, temporal, k, "repeat")
    no_add = lnb(dy, x, w)
    zero_add = lnb(dy, x, w, add=torch.zeros_like(x))
    for k in ("dx", "dw", "db"):
        assert_equal(no_add[k], zero_add[k], (C, k, "add None vs 0"))
    for s, m2 in ((51, 100), (100, 700), (1, M - 1)):
        sub = lnb(dy[s:s + m2].contiguous(), x[s:s + m2].contiguous(), w)
        assert torch.equal(sub["dx"], no_add["dx"][s:s + m2]), (C, s, m2, "row shift")
    SP = 70
    bufs = {"dx": _nan_filled((M + SP) * C), "out_scaled": _nan_filled((M + SP) * C)}
    for k in ("dw", "db", "dbranch"):
        bufs[k] = _nan_filled(C + SP)
        bufs[k][:C] = 0.0
    g = lnb(dy, x, w, add=add, drop=drop, seq_map=(1, J, FJ), scaled=True, branch=True, out=bufs)
    for k, t in bufs.items():
        n = M * C if k in ("dx", "out_scaled") else C
        assert _untouched(t, n), (C, k, "written past its end")
        assert not torch.isnan(g[k]).any(), (C, k)


# ============================================================================================= dX GEMM and fc1 forward
def dx_layers(Cc):
    """(name, N, K) of every dX GEMM of a block: dY [M,N] (the layer's output gradient), W [N,K] (its weight), dX [M,K]"""
    return [("qkv", 3 * Cc, Cc), ("proj", Cc, Cc), ("fc1", 2 * Cc, Cc), ("fc2", Cc, 2 * Cc)]


def gemm_route(M, N, K, split):
    """the kernel gemm_bias picks for out [M,N] = A [M,K] W^T on the training step's options (pafuse_hip.hip)"""
    if split:
        if K >= 128 and (N % 128 == 0 or N % 112 == 0 or N % 96 == 0) and M * N < 2 ** 31 and M * K < 2 ** 31:
            return f"sgemm2_kernel<{8 if N % 128 == 0 else (7 if N % 112 == 0 else 6)}>"
        return f"gemm16_kernel<{8 if N % 128 == 0 else (6 if N % 96 == 0 else (7 if N % 112 == 0 else 4))}>"
    return f"gemm_kernel<4,1,{2 if N % 64 == 0 else (3 if N % 96 == 0 else 1)}> fp32"


def dx_route(M, N, K, mode):
    split = mode == 2 and M >= 128           # plain_splits: mode 2 below 128 rows runs fp32 products
    return ("split_weights_transposed image + " if split else "transpose_kernel + ") + gemm_route(M, K, N, split)


def dx_cases(Cc, with_step=True):
    Ms = list(DX_M) + ([STEP[p][0] for p in STEP if STEP[p][1] == Cc] if with_step else [])
    return [(M, name, N, K) for M in Ms for name, N, K in dx_layers(Cc)]


def grad_in(dy, w, mode, dact_u=None, image_source=0, out=None):
    from pafuse_amd import ops
    return ops.linear_input_grad(dy, w, dact_u, MODES[mode], image_source, out=out)


def tiled_identity(N, K):
    """W [N,K] = 1 where k % N == n (K a multiple of N): dX = dY W is the row of dY tiled, exactly"""
    return (torch.arange(K, device=DEV)[None, :] % N == torch.arange(N, device=DEV)[:, None]).float()


def kernel_gelu_grad(u, N, mode):
    """gelu'(u) as the dX epilogue of this shape computes it: dY = 1 through the tiled identity"""
    M, K = u.shape
    return grad_in(torch.ones(M, N, device=DEV), tiled_identity(N, K), mode, dact_u=u)


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("Cc", DX_WIDTHS)
def test_dx_exact_on_integers(Cc, mode):
    """Every dX GEMM of a block (qkv 3C -> C, proj, fc1 2C -> C, fc2 C -> 2C with dact_u) at M = 1 .. 4097 and the step's rows:
    small-integer dY and W give exact sums, and dact_u in {0, 10} gives gelu' = 0.5 / 1.0 exactly (established first, through
    the identity run) - so the result must equal the integer result bit for bit; a dact_u row or column slip is a wrong element."""
    for M, name, N, K in dx_cases(Cc):
        what = (Cc, MODES[mode], M, name, dx_route(M, N, K, mode))
        dy = _ints((M, N), -3, 4, M + N)
        w = _ints((N, K), -3, 4, M + K + 1) + (torch.arange(K, device=DEV)[None, :] % 5).float()
        ref = dy.double() @ w.double()
        u = None
        if name == "fc2":
            u = 10.0 * _ints((M, K), 0, 2, M + 7)
            g = kernel_gelu_grad(u, N, mode)
            assert_equal(g, torch.where(u == 0, 0.5, 1.0), what + ("gelu'(0) = 0.5, gelu'(10) = 1",))
            ref = ref * torch.where(u == 0, 0.5, 1.0).double()
        assert_equal(grad_in(dy, w, mode, u), ref, what)


@pytest.mark.parametrize("Cc", DX_WIDTHS)
def test_dx_exact_needs_every_slice(Cc):
    """24-bit integer weights against one-hot power-of-two rows of dY (every slice of the transposed weight image must reach
    the product), and the mirror case: 24-bit dY against one power of two per column of W (every slice of dY)."""
    for M in (129, 4097):
        for name, N, K in dx_layers(Cc):
            for mode in (0, 2):
                what = (Cc, M, name, MODES[mode], dx_route(M, N, K, mode))
                g = _gen(M + N + K)
                sign = torch.randint(0, 2, (N, K), generator=g, device=DEV) * 2 - 1
                w = torch.randint(2 ** 23, 2 ** 24, (N, K), generator=g, device=DEV).float() * sign
                hot = torch.randint(0, N, (M,), generator=g, device=DEV)
                scale = 2.0 ** torch.randint(-3, 4, (M,), generator=g, device=DEV).float()
                dy = torch.zeros(M, N, device=DEV)
                dy[torch.arange(M, device=DEV), hot] = scale
                assert_equal(grad_in(dy, w, mode), w[hot] * scale[:, None], what + ("wide W",))
                dyw = torch.randint(2 ** 23, 2 ** 24, (M, N), generator=g, device=DEV).float() * (
                    torch.randint(0, 2, (M, N), generator=g, device=DEV) * 2 - 1)
                kn = torch.randint(0, N, (K,), generator=g, device=DEV)
                ks = 2.0 ** torch.randint(-3, 4, (K,), generator=g, device=DEV).float()
                w1 = torch.zeros(N, K, device=DEV)
                w1[kn, torch.arange(K, device=DEV)] = ks
                assert_equal(grad_in(dyw, w1, mode), dyw[:, kn] * ks, what + ("wide dY",))


def bf16(t):
    return t.bfloat16().double()


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("Cc", DX_WIDTHS)
def test_dx_against_fp64_image_sources_and_sensitivity(Cc, mode):
    """Random dY, W (and dact_u ~ N(0, 1.5) for fc2) against fp64 under the derived bound at every dX shape; in mode 2 the image
    from the step's batch kernel (image_source 1) gives the same bits as the single kernel's; one bf16 per operand (host
    emulation) fails the bound."""
    worst = (0.0, 0.0)
    for M, name, N, K in dx_cases(Cc):
        what = (Cc, MODES[mode], M, name, dx_route(M, N, K, mode))
        dy = _normal((M, N), M + N + 3)
        w = (torch.rand((N, K), generator=_gen(M + K + 4), device=DEV) * 2 - 1) / math.sqrt(N)
        u = _normal((M, K), M + 5, 1.5) if name == "fc2" else None
        out = grad_in(dy, w, mode, u)
        S = dy.double().abs() @ w.double().abs()
        e = PROD[mode] * S + gam(6 * N + 1) * 1.01 * S
        ref = dy.double() @ w.double()
        bad = bf16(dy) @ bf16(w)
        if u is not None:
            g = kernel_gelu_grad(u, N, mode).double()
            ref, bad = ref * g, bad * g
            e = g.abs() * e + U * ref.abs()
        q = within(out, ref, e, what)
        worst = max(worst, q)
        assert ((bad - ref).abs() / e).max().item() > 1, what + ("one bf16 per operand passes the bound",)
        if mode == 2 and M >= 128:
            assert torch.equal(grad_in(dy, w, mode, u, image_source=1), out), what + ("image sources differ",)
    report(f"dX GEMM C={Cc} {MODES[mode]}: error / bound max {worst[0]:.2e} (mean err / mean bound {worst[1]:.2e})")


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("Cc", DX_WIDTHS)
def test_time_mlp_dx_against_fp64(Cc, mode):
    """The time MLP's dX GEMM (d hid = d temb W3: M = B, N = C, K = 2C; fp32 products at every mode, M < 128)."""
    for B in TIME_B:
        dy = _normal((B, Cc), B + 11)
        w = (torch.rand((Cc, 2 * Cc), generator=_gen(B + 12), device=DEV) * 2 - 1) / math.sqrt(Cc)
        S = dy.double().abs() @ w.double().abs()
        within(grad_in(dy, w, mode), dy.double() @ w.double(), U * S + gam(6 * Cc + 1) * 1.01 * S,
               (Cc, B, dx_route(B, Cc, 2 * Cc, mode)))


@pytest.mark.parametrize("mode", (0, 2))
def test_gelu_erf_grad_against_fp64_and_torch(mode):
    """gelu_erf_grad (the fc2 dX epilogue's gelu') on u ~ N(0, 1.5) and a sweep of [-8, 8], read out through the identity run
    on three routes (mode 2: the strip kernel at C = 256 and gemm16_kernel at C = 64; mode 0: the fp32 slab epilogue): max and
    mean error against fp64 no worse than torch's own CPU fp32 GELU backward on the same inputs."""
    u_all = torch.cat([_normal((240000,), 5, 1.5), torch.linspace(-8, 8, 65536, device=DEV)])
    ud = u_all.double().cpu().requires_grad_(True)
    torch.nn.functional.gelu(ud).sum().backward()
    ref = ud.grad.to(DEV)
    tch = torch.ops.aten.gelu_backward(torch.ones(u_all.numel()), u_all.cpu()).double().to(DEV)
    t_err = (tch - ref).abs()
    for Cc in ((256, 64) if mode == 2 else (256,)):
        K = 2 * Cc
        rows = (u_all.numel() + K - 1) // K
        u = torch.zeros(rows * K, device=DEV)
        u[:u_all.numel()] = u_all
        g = kernel_gelu_grad(u.view(rows, K), Cc, mode).reshape(-1)[:u_all.numel()].double()
        err = (g - ref).abs()
        report(f"gelu_erf_grad via {dx_route(rows, Cc, K, mode)}: max {err.max().item():.2e} mean {err.mean().item():.2e}; "
               f"torch CPU fp32: max {t_err.max().item():.2e} mean {t_err.mean().item():.2e}")
        assert err.max() <= t_err.max() and err.mean() <= t_err.mean(), (Cc, mode, err.max().item(), t_err.max().item())


def train_fwd(x, w, b, mode, gelu=True, out=None):
    from pafuse_amd import ops
    return ops.linear_train(x, w, b, gelu, MODES[mode], out=out)


def fwd_cases(Cc):
    """(M, N, K): mlp.fc1 (N = 2C, K = C) at the dX row counts, and the time MLP's two layers at M = B"""
    Ms = list(DX_M) + [STEP[p][0] for p in STEP if STEP[p][1] == Cc]
    return [(M, 2 * Cc, Cc, True) for M in Ms] + [(B, 2 * Cc, Cc, True) for B in TIME_B] + [(B, Cc, 2 * Cc, False) for B in TIME_B]


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("Cc", DX_WIDTHS)
def test_linear_train_equals_the_inference_launches(Cc, mode):
    """u and h = gelu(u) of the training forward's fc1 (out_act: sgemm2 flag 8, gemm16 and the fp32 slab epilogue) bit-equal
    to the inference launches on the same data and shape: ops.linear_split (layout 2) without and with GELU where the step
    runs split products (mode 2, M >= 128), ops.linear (fp32) elsewhere - the same accumulation and the same gelu_erf."""
    from pafuse_amd import ops
    for M, N, K, act in fwd_cases(Cc):
        x = _normal((M, K), M + 21)
        w = (torch.rand((N, K), generator=_gen(M + 22), device=DEV) * 2 - 1) / math.sqrt(K)
        b = _normal((N,), M + 23, 0.1)
        split = mode == 2 and M >= 128
        what = (Cc, MODES[mode], M, N, K, gemm_route(M, N, K, split))
        u, h = train_fwd(x, w, b, mode, act)
        if split:
            img = ops.split_weights(w, 2)
            u_inf = ops.linear_split(x, w, b, image=img, layout=2)
            h_inf = ops.linear_split(x, w, b, act="gelu", image=img, layout=2)
        else:
            u_inf, h_inf = ops.linear(x, w, b), ops.linear(x, w, b, act="gelu")
        assert_equal(u, u_inf, what + ("u",))
        if act:
            assert_equal(h, h_inf, what + ("h",))
        S = x.double().abs() @ w.double().abs().t()
        within(u, x.double() @ w.double().t() + b.double(), PROD[mode] * S + gam(6 * K + 1) * (1.01 * S + b.double().abs()),
               what + ("u vs fp64",))


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("Cc", (384, 224, 64))
def test_dx_and_fc1_write_nothing_past_row_M_and_repeat(Cc, mode):
    """Outputs in buffers with 70 NaN rows past M keep them; a second launch gives the same bits."""
    SP = 70
    for M in (31, 129, 4097):
        for name, N, K in dx_layers(Cc):
            dy, w = _normal((M, N), 51), _normal((N, K), 52, 0.05)
            u = _normal((M, K), 53) if name == "fc2" else None
            buf = _nan_filled((M + SP) * K)
            out = grad_in(dy, w, mode, u, out=buf)
            assert _untouched(buf, M * K), (Cc, mode, M, name, dx_route(M, N, K, mode))
            assert not torch.isnan(out).any()
            assert torch.equal(grad_in(dy, w, mode, u), out), (Cc, mode, M, name, "repeat")
        x, w, b = _normal((M, Cc), 54), _normal((2 * Cc, Cc), 55, 0.05), _normal((2 * Cc,), 56)
        bufs = {"u": _nan_filled((M + SP) * 2 * Cc), "h": _nan_filled((M + SP) * 2 * Cc)}
        uu, hh = train_fwd(x, w, b, mode, out=bufs)
        for k, t in bufs.items():
            assert _untouched(t, M * 2 * Cc), (Cc, mode, M, "fc1", k)
        u2, h2 = train_fwd(x, w, b, mode)
        assert torch.equal(uu, u2) and torch.equal(hh, h2), (Cc, mode, M, "fc1 repeat")


# ==================================================================================================== GELU backward
@pytest.mark.parametrize("N", (448, 512, 768))
def test_gelu_backward_against_fp64(N):
    """du = dh gelu'(u) (libm erff / expf) and db against fp64 under the derived bounds; in place gives the same bits."""
    from pafuse_amd import ops
    worst = {}
    for M in (1, 31, 37, 4097):
        u = _normal((M, N), M + N, 1.5)
        u.view(-1)[:min(M * N, 4096)] = torch.linspace(-8, 8, min(M * N, 4096), device=DEV)
        dh = _normal((M, N), M + N + 1)
        ud = u.double().requires_grad_(True)
        torch.nn.functional.gelu(ud).backward(dh.double())
        du_ref = ud.grad
        xd = u.double()
        phi = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
        gp = 0.5 * (1 + torch.erf(xd / math.sqrt(2))) + xd * phi
        e = dh.double().abs() * (6 * U + xd.abs() * phi * (xd * xd * U / 2 + 7 * U) + U * gp.abs()) + U * du_ref.abs()
        du, db = ops.gelu_backward(u, dh)
        worst["du"] = max(worst.get("du", (0, 0)), within(du, du_ref, e, (M, N, "du")))
        db_ref = du_ref.sum(0)
        worst["db"] = max(worst.get("db", (0, 0)), within(db, db_ref, e.sum(0) + gam(M) * du_ref.abs().sum(0) + U * db_ref.abs(), (M, N, "db")))
        dh2 = dh.clone()
        du2, db2 = ops.gelu_backward(u, dh2, in_place=True)
        assert du2.data_ptr() == dh2.data_ptr() and torch.equal(du2, du) and torch.equal(db2, db), (M, N, "in place")
    report(f"gelu_backward N={N}: error / bound max (mean err / mean bound): " +
           ", ".join(f"{k} {a:.2e} ({b:.2e})" for k, (a, b) in worst.items()))


# =========================================================================================================== refusals
def test_invalid_argument_sets_are_refused_before_any_launch():
    """Each inconsistent argument set returns its error code and pafuse_last_error() names the problem, and no output changes;
    M = 0 is a no-op.  (Every pointer handed over is a real buffer; the misaligned ones are 4 bytes into one.)"""
    from pafuse_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    E_ARG, E_SHAPE, E_WS = -1, -2, -3
    M, Cc = 4097, 384
    big = torch.zeros(M * 3 * Cc + 64, device=DEV)
    out = _nan_filled(M * 3 * Cc + 64)
    vec = _nan_filled(4 * Cc)
    P, O, V = big.data_ptr(), out.data_ptr(), vec.data_ptr()
    nbytes = lib.pafuse_train_unit_bytes(M, 3 * Cc, 3 * Cc)
    ws = torch.empty(nbytes + 64, dtype=torch.uint8, device=DEV)
    W = ws.data_ptr()
    # the LayerNorm partials alone: ceil(M / 64) 3 C floats
    assert lib.pafuse_train_unit_bytes(M, Cc, 0) >= (M + 63) // 64 * 3 * Cc * 4
    ln_need = lib.pafuse_train_unit_bytes(M, Cc, 0)

    def lnb_call(**edit):
        a = _lib.LnbArgs()
        a.dy, a.x, a.w, a.eps, a.add, a.dx, a.drop = P, P, P, 1e-6, None, O, None
        a.temporal, a.J, a.FJ, a.out_scaled, a.dw, a.db, a.dbranch, a.M, a.C = 0, 1, 1, O, V, V, None, M, Cc
        ws_bytes = edit.pop("ws_bytes", ln_need)
        for k, v in edit.items():
            setattr(a, k, v)
        return lib.pafuse_layernorm_backward(C.byref(a), W, ws_bytes, stream)

    def dx_call(dY=P, Wt=P, dact=None, dX=O, m=M, n=Cc, k=Cc, mode=2, src=0, ws_bytes=None):
        need = lib.pafuse_train_unit_bytes(m, n, k) if ws_bytes is None else ws_bytes
        return lib.pafuse_linear_input_grad(dY, Wt, dact, dX, m, n, k, mode, src, W, need, stream)

    def fwd_call(A=P, Wt=P, bias=P, u=O, h=O, m=M, n=2 * Cc, k=Cc, mode=2, ws_bytes=None):
        need = lib.pafuse_train_unit_bytes(m, n, k) if ws_bytes is None else ws_bytes
        return lib.pafuse_linear_train(A, Wt, bias, u, h, m, n, k, mode, W, need, stream)

    def gelu_call(u=P, dh=P, du=O, db=V, m=M, n=2 * Cc, ws_bytes=None, wsp=W):
        need = lib.pafuse_train_unit_bytes(m, n, 0) if ws_bytes is None else ws_bytes
        return lib.pafuse_gelu_backward(u, dh, du, db, m, n, wsp, need, stream)

    cases = [
        (lambda: lnb_call(dy=None), E_ARG, "null pointer"),
        (lambda: lnb_call(dw=None), E_ARG, "null pointer"),
        (lambda: lnb_call(M=-1), E_ARG, "negative M"),
        (lambda: lnb_call(C=0), E_SHAPE, "C=0 outside 1 .. 768"),
        (lambda: lnb_call(C=769), E_SHAPE, "C=769 outside 1 .. 768"),
        (lambda: lnb_call(C=1024), E_SHAPE, "C=1024 outside 1 .. 768"),
        (lambda: lnb_call(x=P + 4), E_ARG, "not 16-byte aligned"),
        (lambda: lnb_call(out_scaled=O + 4), E_ARG, "not 16-byte aligned"),
        (lambda: lnb_call(add=P + 8), E_ARG, "not 16-byte aligned"),
        (lambda: lnb_call(dbranch=V, out_scaled=None), E_ARG, "dbranch without out_scaled"),
        (lambda: lnb_call(drop=P, J=0), E_ARG, "drop with J=0"),
        (lambda: lnb_call(drop=P, temporal=1, J=24, FJ=0), E_ARG, "drop with J=24, FJ=0"),
        (lambda: lnb_call(ws_bytes=ln_need - 1), E_WS, "workspace too small"),
        (lambda: dx_call(Wt=None), E_ARG, "null pointer"),
        (lambda: dx_call(mode=1), E_ARG, "matrix-product mode 1"),
        (lambda: dx_call(mode=4), E_ARG, "matrix-product mode 4"),
        (lambda: dx_call(src=2), E_ARG, "image source 2"),
        (lambda: dx_call(n=100), E_SHAPE, "N=100, K=384 must be positive multiples of 32"),
        (lambda: dx_call(k=200), E_SHAPE, "must be positive multiples of 32"),
        (lambda: dx_call(dact=P, k=224, mode=0), E_SHAPE, "dact_u on fp32 products needs K % 64 == 0"),
        (lambda: dx_call(dact=P, k=224, m=127), E_SHAPE, "dact_u on fp32 products needs K % 64 == 0"),
        (lambda: dx_call(dY=P + 4), E_ARG, "not 16-byte aligned"),
        (lambda: dx_call(dact=P + 4, k=2 * Cc), E_ARG, "not 16-byte aligned"),
        (lambda: dx_call(ws_bytes=lib.pafuse_train_unit_bytes(M, Cc, Cc) - 1), E_WS, "workspace too small"),
        (lambda: fwd_call(bias=None), E_ARG, "null pointer"),
        (lambda: fwd_call(mode=3), E_ARG, "matrix-product mode 3"),
        (lambda: fwd_call(n=224, mode=0), E_SHAPE, "h on fp32 products needs N % 64 == 0"),
        (lambda: fwd_call(h=O + 4), E_ARG, "not 16-byte aligned"),
        (lambda: fwd_call(ws_bytes=lib.pafuse_train_unit_bytes(M, 2 * Cc, Cc) - 1), E_WS, "workspace too small"),
        (lambda: gelu_call(db=None), E_ARG, "null pointer"),
        (lambda: gelu_call(n=6), E_SHAPE, "N=6 must be a positive multiple of 4"),
        (lambda: gelu_call(u=P + 4), E_ARG, "not 16-byte aligned"),
        (lambda: gelu_call(wsp=W + 4), E_ARG, "not 16-byte aligned"),
        (lambda: gelu_call(ws_bytes=lib.pafuse_train_unit_bytes(M, 2 * Cc, 0) - 1), E_WS, "workspace too small"),
    ]
    for i, (call, code, text) in enumerate(cases):
        rc = call()
        msg = lib.pafuse_last_error().decode()
        assert rc == code and text in msg, (i, rc, code, msg)
    torch.cuda.synchronize()
    assert _untouched(out, 0) and _untouched(vec, 0), "a refused call wrote an output"
    # M = 0: nothing is launched
    assert lnb_call(M=0) == 0 and dx_call(m=0) == 0 and fwd_call(m=0) == 0 and gelu_call(m=0) == 0
    torch.cuda.synchronize()
    assert _untouched(out, 0) and _untouched(vec, 0), "an empty call wrote an output"

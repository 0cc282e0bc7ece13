"""Unit tests of the whole-row layers (attn.proj, mlp.fc2 + residual + the LayerNorm chain in the epilogue) through
pafuse_linear_rowln / pafuse_linear_rowln_group: every route of gemm_rowln_as, against exact integers and against fp64
evaluations of the same layer on the device.

Error bounds (b).  u = 2^-24.  Accumulated roundings use the probabilistic bound of Higham & Mary (SIAM J. Sci. Comput. 41(5),
2019): a sum of n terms computed in fp32, in any order, is within gam(n) * sum|terms| of the exact sum, gam(n) = LAM sqrt(n) u,
with probability >= 1 - 2 n exp(-LAM^2 / 2) per sum (LAM = 9: < 1e-13 for the largest n here), rounding errors taken as
independent and mean-zero.  The same model treats the errors of different elements of one output row as independent.
  GEMM + residual (each element):  y = (A W^T + b) + r.  A split-precision product keeps every operand term above 2^-24 of
    |a w|: bf16x3 drops a1 w2 + a2 w1 + a2 w2 <= (2 2^-8 2^-16 + 2^-32) |a w| < 2^-22 |a w|; f16x2 drops lo w1 and rounds
    both operands to 22 bits, <= 3 2^-22 < 2^-20 |a w|; an fp32 product rounds once, u |a w|  (PROD below).  The products
    (at most six per k, their sum <= 1.01 sum_k |a_k w_k| = 1.01 S) and the bias are n = 6 K + 1 accumulated terms; the
    residual add is one more rounding of the result:
      e_y = PROD S + gam(6 K + 1) (1.01 S + |b|) + u |y|
      (training, y = r + rs (acc + b):  |rs| (PROD S + gam(6 K + 1) (1.01 S + |b|)) + u |rs (acc + b)| + u |y|)
  An H image (f16x2) of an fp32 value v holds hi + 2^-11 lo, within 2^-22 |v| of it; an X image is exact.
  LayerNorm of a row y with elementwise input bounds e (fp32: two fixed-order sums over C, one fma per element):
      mean:  em  = sqrt(sum e^2) / C + gam(C) mean|y| + 2 u |mu|             (the rounded 1 / C and product: 2 u)
      rstd:  rho = rstd^2 sqrt(sum (d e)^2) / C + gam(C) / 2 + 4 u + (rstd (em + max e))^2    (relative; d = y - mu: var
             moves by 2 / C sum d dy; sum d = 0 removes the mean's error to first order; the squares' fma sum gam(C); eps add,
             sqrt, division, the rounding of d: 4 u)
      out_i: E_i = |g_i| (rstd (e_i + em + u |d_i|) + |zhat_i| (rho + u)) + u |out_i|
  pos:   + u |z + pos|.    Head k (3 outputs, C-term dot product of n with head_w):
      sqrt(sum (hw g rstd e)^2) + LAM sqrt(sum (hw r)^2) + rstd em |sum hw g| + rho |sum hw g zhat| + gam(C + 1) (sum |n hw| + |hb|)
      (independent GEMM errors add in quadrature, the row-common mean / rstd errors with their signs, r_i = the per-element
      LayerNorm roundings of E_i).
Nothing here is fitted to a measurement.  Sensitivity: the opt-in bf16 mode (one bf16 per operand, ~2^-9 per operand) must
FAIL every bf16x3 bound on the elementwise outputs and the head - so the bounds would catch a dropped slice.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

MODES = {0: "f32", 1: "bf16", 2: "bf16x3", 3: "f16x2", 4: "bf16x3_images"}
WIDTHS = (384, 256, 288, 224, 128, 64)          # every width gemm_rowln_as has a kernel for
IMAGE_WIDTHS = (384, 256, 224)                  # modes 3 and 4
SMALL_M = (1, 31, 33, 63, 65, 129)
# production tile streams of the whole-row layers at P = 20 (B = 1, flip: 40 hypotheses x 27 frames x joints of the part):
# body 384 wide, 64-row tiles: 405 tiles; face 224, 128-row tiles: 574; hands 256, 64-row tiles: 709; and a stream of more
# than two rounds of the 512 workgroup slots of a launch (1101 tiles)
STREAMS = {"body": (25920, 384), "face": (73440, 224), "hands": (45360, 256), "rounds": (64 * 1100 + 17, 384)}
U = 2.0 ** -24
LAM = 9.0
PROD = {0: U, 1: 2.0 ** -22, 2: 2.0 ** -22, 3: 2.0 ** -20, 4: 2.0 ** -22}   # mode 1 is held to the bf16x3 bound: it must fail it
NAN_BITS = 0x7FC0DEAD


def gam(n):
    return LAM * math.sqrt(n) * U


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi, shape, generator=_gen(seed), device=DEV).float()


def _normal(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed), device=DEV) * scale


def int_layer(M, N, K, seed):
    """small-integer operands: every result is an exact integer in fp32 (|y| < 2^15)"""
    x = _ints((M, K), -3, 4, seed)
    w = _ints((N, K), -3, 4, seed + 1) + (torch.arange(N, device=DEV)[:, None] % 5).float()   # |w| <= 7: one bf16
    b = (torch.arange(N, device=DEV).float() % 17) - 8
    r = _ints((M, N), -50, 51, seed + 2)
    return x, w, b, r


def exact(x, w, b, r):
    return x.double() @ w.double().t() + b.double() + r.double()


def run(x, w, b, r, mode, **kw):
    from pafuse_amd import ops
    return ops.linear_rowln(x, w, b, r, MODES[mode], **kw)


def assert_equal(out, ref, what):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if not torch.equal(out.double(), ref.double()):
        bad = (out.double() != ref.double()).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: "
                             f"{out.double()[tuple(bad[0])].item()} != {ref.double()[tuple(bad[0])].item()}")


def routes():
    """(mode, N, resid_image) of every route: modes 0 - 2 at every width, 3 and 4 at theirs with either residual form"""
    out = [(m, n, False) for m in (0, 1, 2) for n in WIDTHS]
    return out + [(m, n, ri) for m in (3, 4) for n in IMAGE_WIDTHS for ri in (False, True)]


def route_id(p):
    m, n, ri = p
    return f"{MODES[m]}-{n}" + ("-hres" if ri else "")


# ---------------------------------------------------------------------------------------------------- (a) exact integers
@pytest.mark.parametrize("route", routes(), ids=route_id)
def test_exact_integers(route):
    """x W^T + b + resid on small integers, with and without pos: bit for bit the integer result, at every small M (ragged
    last tiles, a single row) and K = C, 2C (and 3C, the widest MLP mlp_hidden allows, at 256 and 64)."""
    mode, N, ri = route
    posF, posJ = 3, 5
    pos = _ints((posF, N), -20, 21, 7)
    rows = torch.arange(129, device=DEV)
    pos_rows = pos[(rows // posJ) % posF]
    for K in (N, 2 * N) + ((3 * N,) if N in (256, 64) else ()):
        for M in SMALL_M:
            x, w, b, r = int_layer(M, N, K, 100 + M + K)
            ref = exact(x, w, b, r)
            out = run(x, w, b, r, mode, resid_image=ri)
            assert_equal(out["x"], ref, (route, M, K))
            out = run(x, w, b, r, mode, resid_image=ri, pos=(pos, posJ, posF))
            assert_equal(out["x"], ref + pos_rows[:M].double(), (route, M, K, "pos"))


@pytest.mark.parametrize("mode,N", [(m, n) for m in (0, 2) for n in WIDTHS] + [(4, n) for n in IMAGE_WIDTHS] +
                         [(3, n) for n in IMAGE_WIDTHS])
def test_exact_wide_activations_need_every_slice(mode, N):
    """24-bit activations (22-bit in f16x2) against one power of two per weight row: exact only if every slice of the
    activation reaches the product (bf16x3: three bf16 slices; f16x2: hi and the 2^11-scaled lo)."""
    M, K = 129, 2 * N
    g = _gen(31 + N)
    bits = 22 if mode == 3 else 24
    sign = torch.randint(0, 2, (M, K), generator=g, device=DEV) * 2 - 1
    x = torch.randint(2 ** (bits - 1), 2 ** bits, (M, K), generator=g, device=DEV).float() * sign
    if mode == 3:
        x = x * 2.0 ** -8                      # |x| < 65504: the fp16 hi slice holds it
    kn = torch.randint(0, K, (N,), generator=g, device=DEV)
    w = torch.zeros(N, K, device=DEV)
    scale = 2.0 ** torch.randint(-3, 4, (N,), generator=g, device=DEV).float()
    w[torch.arange(N, device=DEV), kn] = scale
    zero_b, zero_r = torch.zeros(N, device=DEV), torch.zeros(M, N, device=DEV)
    out = run(x, w, zero_b, zero_r, mode)
    assert_equal(out["x"], x[:, kn] * scale, (mode, N))


@pytest.mark.parametrize("name", list(STREAMS))
def test_exact_integers_production_tile_streams(name):
    """The production streams (hundreds of tiles, more than two rounds of the launch's slots, a ragged last tile) in mode 2
    and - at the image widths - both image modes with the centred-image residual written in place, as the denoisers run them."""
    M, N = STREAMS[name]
    for K in (N, 2 * N):
        x, w, b, r = int_layer(M, N, K, 7 + K)
        ref = exact(x, w, b, r)
        assert_equal(run(x, w, b, r, 2)["x"], ref, (name, K, "bf16x3"))
        for mode in (3, 4):
            assert_equal(run(x, w, b, r, mode, resid_image=True, in_place=True)["x"], ref, (name, K, MODES[mode]))


@pytest.mark.parametrize("M", (4095, 4096, 4097))
def test_exact_integers_across_the_224_tile_switch(M):
    """224 wide: 64-row tiles below M = 4096, 128-row tiles from 4096 up (and the grouped kernel's variant)."""
    for K in (224, 448):
        x, w, b, r = int_layer(M, 224, K, M + K)
        assert_equal(run(x, w, b, r, 2)["x"], exact(x, w, b, r), (M, K))
        assert_equal(run(x, w, b, r, 0)["x"], exact(x, w, b, r), (M, K, "f32"))


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("N,M", [(384, 333), (384, 4160), (256, 4160), (224, 4160), (224, 333), (288, 333), (128, 333), (64, 333)])
def test_exact_integers_training(mode, N, M):
    """The training form y = resid + rowscale[seq(m)] (A W^T + b) (EPI_ROWLN_TRAIN), spatial and temporal row maps, with
    powers-of-two row factors (and 0, a dropped path): out_pre and out_x exact; split tiles where gemm_rowln_train has them
    (384 / 256 at any M, 224 from M = 4096), the fp32 kernels elsewhere."""
    F, J = 13, 5
    for K in (N, 2 * N):
        x, w, b, r = int_layer(M, N, K, 50 + K)
        acc = x.double() @ w.double().t() + b.double()
        for temporal in (0, 1):
            nseq = (M + F * J - 1) // (F * J) * J if temporal else (M + J - 1) // J
            rs = 2.0 ** _ints((nseq,), -2, 3, 9 + temporal)
            rs[::5] = 0.0
            m = torch.arange(M, device=DEV)
            seq = (m // (F * J)) * J + m % J if temporal else m // J
            ref = r.double() + rs[seq].double()[:, None] * acc
            pos = _ints((3, N), -20, 21, 3)
            out = run(x, w, b, r, mode, training=True, rowscale=rs, rs_map=(temporal, J, F * J), pos=(pos, 7, 3))
            assert_equal(out["pre"], ref, (N, M, K, temporal, "pre"))
            assert_equal(out["x"], ref + pos[(m // 7) % 3].double(), (N, M, K, temporal, "x"))


@pytest.mark.parametrize("route", routes(), ids=route_id)
def test_folded_statistics_on_exact_rows(route):
    """ln_stats on exact-integer y: the mean is fp32(sum y) * fp32(1/C) rounded once (sum y is exact), so within u |mu| +
    0.5 ulp of the exact mean; rstd within the bound of the module docstring with e = 0; the stored row is fp32(y - mean)
    with the STORED mean, bit for bit (fp32 rows) or - as an image - the image of exactly that fp32 row."""
    from pafuse_amd import ops
    mode, N, ri = route
    if mode == 1:
        return _folded_mode1_exact(N)
    M, K = 333, 2 * N
    x, w, b, r = int_layer(M, N, K, 5)
    r[::7] += 2000.0                                         # large row means
    y = exact(x, w, b, r)
    g1, b1 = 1 + _normal((N,), 1, 0.1), _normal((N,), 2, 0.1)
    out = run(x, w, b, r, mode, resid_image=ri, next=(g1, b1, 1e-6), fold=True)
    st = out["stats"]
    mean32 = (y.sum(1).float() * torch.tensor(1.0 / N, dtype=torch.float32)).double()   # fp32(S) exact; one fp32 product
    assert_equal(st[:, 0], mean32.float(), (route, "mean = fp32(sum) * fp32(1/C)"))
    mu = y.mean(1)
    ulp = torch.nextafter(mu.float().abs(), torch.tensor(math.inf, device=DEV)).double() - mu.float().abs().double()
    assert ((st[:, 0].double() - mu).abs() <= U * mu.abs() + 0.5 * ulp).all()
    var = ((y - mu[:, None]) ** 2).mean(1)
    rstd = 1 / torch.sqrt(var + 1e-6)
    em = (st[:, 0].double() - mu).abs()
    rho = gam(N) / 2 + 4 * U + (rstd * em) ** 2
    assert ((st[:, 1].double() / rstd - 1).abs() <= rho).all(), ((st[:, 1].double() / rstd - 1).abs() / rho).max()
    centred = (y.float() - st[:, :1])                         # fp32(y - stored mean): y is exact in fp32
    if mode >= 3:
        split, join = (ops.hsplit_rows, ops.hjoin_rows) if mode == 3 else (ops.xsplit_rows, ops.xjoin_rows)
        assert_equal(out["x_img"], join(split(centred.contiguous()), M, N), (route, "image of the centred row"))
    if not ri:
        assert_equal(out["x"], centred, (route, "stored row = y - stored mean"))


def _folded_mode1_exact(N):
    x, w, b, r = int_layer(129, N, N, 6)
    y = exact(x, w, b, r)
    out = run(x, w, b, r, 1, next=(torch.ones(N, device=DEV), torch.zeros(N, device=DEV), 1e-6), fold=True)
    assert_equal(out["x"], y.float() - out["stats"][:, :1], (N, "bf16 stored row"))


# ----------------------------------------------------------------------------------------------- (b) chains against fp64
def ln64(y, e, g, beta, eps, C):
    """fp64 LayerNorm of exact rows y and the bound on the fp32 result given input bounds e (module docstring)"""
    mu = y.mean(1, keepdim=True)
    d = y - mu
    rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    zh = d * rstd
    out = zh * g + beta
    em = (e * e).sum(1, keepdim=True).sqrt() / C + gam(C) * y.abs().mean(1, keepdim=True) + 2 * U * mu.abs()
    rho = rstd ** 2 * ((d * e) ** 2).sum(1, keepdim=True).sqrt() / C + gam(C) / 2 + 4 * U + (rstd * (em + e.amax(1, keepdim=True))) ** 2
    rnd = g.abs() * (U * rstd * d.abs() + U * zh.abs()) + U * out.abs()      # this stage's own per-element roundings
    E = g.abs() * (rstd * (e + em) + zh.abs() * rho) + rnd
    return out, E, dict(mu=mu, rstd=rstd, em=em, rho=rho, zh=zh, g=g, rnd=rnd, e=e)


CHAINS = {
    # run_blocks' four whole-row epilogues (pafuse_hip.hip make_block, run_mixste_layers_n)
    "proj_norm2": dict(K=1, post=False, pos=False, next_eps=1e-6, head=False),
    "fc2_post_norm1": dict(K=2, post=True, pos=False, next_eps=1e-6, head=False),
    "fc2_spatial0_pos_norm1": dict(K=2, post=True, pos=True, next_eps=1e-6, head=False),
    "fc2_last_temporal_head": dict(K=2, post=True, pos=False, next_eps=1e-5, head=True),
}


def chain_case(N, chain, M=333, seed=0, kmul=None):
    """seeded operands at the model's scales and the fp64 evaluation of the chain with its bounds"""
    spec = CHAINS[chain]
    K = N * (kmul or spec["K"])
    s = 1000 * seed + N
    x = _normal((M, K), s + 1, 0.7)
    w = (torch.rand((N, K), generator=_gen(s + 2), device=DEV) * 2 - 1) / math.sqrt(K)
    b = (torch.rand((N,), generator=_gen(s + 3), device=DEV) * 2 - 1) / math.sqrt(K)
    r = _normal((M, N), s + 4, 1.0)
    r[3::7] += 300.0                                        # rows with large means (outlier channels of a trained stream)
    p = dict(x=x, w=w, b=b, r=r, K=K)
    if spec["post"]:
        p["post"] = (1 + _normal((N,), s + 5, 0.1), _normal((N,), s + 6, 0.1) + 10.0, 1e-6)   # post-norm bias 10: mean-10 rows
    if spec["pos"]:
        p["pos"] = (_normal((3, N), s + 7, 0.02), 17, 3)
    p["next"] = (1 + _normal((N,), s + 8, 0.1), _normal((N,), s + 9, 0.1), spec["next_eps"])
    if spec["head"]:
        p["head"] = ((torch.rand((3, N), generator=_gen(s + 10), device=DEV) * 2 - 1) / math.sqrt(N), _normal((3,), s + 11, 0.1))
    return p


def chain_ref(p, mode, resid=None):
    """fp64 values and bounds of every output of the chain for matrix-product mode `mode` (resid: the residual as the
    kernel sees it - the joined image in the centred-image form)"""
    x, w, b, K = p["x"].double(), p["w"].double(), p["b"].double(), p["K"]
    r = (p["r"] if resid is None else resid).double()
    N = w.shape[0]
    y = x @ w.t() + b + r
    S = x.abs() @ w.abs().t()
    e = PROD[mode] * S + gam(6 * K + 1) * (1.01 * S + b.abs()) + U * y.abs()
    ref = {}
    z, ez = y, e
    if "post" in p:
        pw, pb, peps = p["post"]
        z, ez, _ = ln64(y, e, pw.double(), pb.double(), peps, N)
    if "pos" in p:
        tab, pj, pf = p["pos"]
        m = torch.arange(y.shape[0], device=DEV)
        z = z + tab.double()[(m // pj) % pf]
        ez = ez + U * z.abs()
    ref["x"], ref["ex"] = z, ez
    nw, nb, neps = p["next"]
    n, en, st = ln64(z, ez, nw.double(), nb.double(), neps, N)
    ref["n"], ref["en"], ref["st"] = n, en, st
    if "head" in p:
        hw, hb = p["head"][0].double(), p["head"][1].double()
        gg, rstd = st["g"], st["rstd"]
        ref["head"] = n @ hw.t() + hb
        ref["ehead"] = (((hw[None] * (gg * rstd * st["e"])[:, None]) ** 2).sum(-1).sqrt()
                        + LAM * ((hw[None] * st["rnd"][:, None]) ** 2).sum(-1).sqrt()
                        + rstd * st["em"] * (hw * gg[None]).sum(-1).abs()[None]
                        + st["rho"] * ((hw[None] * (gg * st["zh"])[:, None]).sum(-1)).abs()
                        + gam(N + 1) * ((n.abs() @ hw.abs().t()) + hb.abs()))
    return ref


def chain_kwargs(p, fold):
    kw = {k: p[k] for k in ("post", "pos", "next", "head") if k in p}
    kw["fold"] = fold
    return kw


def check_chain(out, ref, fold, what, x_from_image=False):
    """every output within its bound (x_from_image: 'x' is an H image joined back - 2^-22 relative more); returns the largest
    error / bound ratio per output"""
    worst = {}
    himg = 2.0 ** -22 if x_from_image else 0.0

    def within(name, val, r, bound):
        q = (val.double() - r).abs() / bound
        worst[name] = q.max().item()
        return worst[name] <= 1.0

    if fold:
        st = ref["st"]
        mean, rstd = out["stats"][:, :1].double(), out["stats"][:, 1:].double()
        assert ((mean - st["mu"]).abs() <= st["em"]).all(), (what, "mean", ((mean - st["mu"]).abs() / st["em"]).max())
        assert ((rstd / st["rstd"] - 1).abs() <= st["rho"]).all(), (what, "rstd", ((rstd / st["rstd"] - 1).abs() / st["rho"]).max())
        # the stored row is z - (stored mean): against the exact z - mu, the stored mean's own error and one rounding on top
        cb = ref["ex"] + st["em"] + U * (ref["x"] - st["mu"]).abs()
        assert within("x", out["x"], ref["x"] - st["mu"], cb + himg * (ref["x"] - st["mu"]).abs()), (what, "centred x", worst["x"])
        if "x_img" in out:
            assert within("x_img", out["x_img"], ref["x"] - st["mu"], cb + 2.0 ** -22 * (ref["x"] - st["mu"]).abs()), (what, worst)
    else:
        assert within("x", out["x"], ref["x"], ref["ex"] + himg * ref["x"].abs()), (what, "x", worst["x"])
        if "x_img" in out:
            assert within("x_img", out["x_img"], ref["x"], ref["ex"] + 2.0 ** -22 * ref["x"].abs()), (what, "x image", worst)
        if "head" in ref:
            assert within("head", out["head"], ref["head"], ref["ehead"]), (what, "head", worst["head"])
        assert within("n", out["n"], ref["n"], ref["en"]), (what, "n", worst["n"])
        if "n_img" in out:
            assert within("n_img", out["n_img"], ref["n"], ref["en"] + 2.0 ** -22 * ref["n"].abs()), (what, "n image", worst)
    return worst


def chain_cases():
    out = []
    for chain in CHAINS:
        for fold in ((False,) if CHAINS[chain]["head"] else (False, True)):
            out += [(m, n, False, chain, fold) for m in (0, 2) for n in WIDTHS]
            out += [(m, n, ri, chain, fold) for m in (3, 4) for n in IMAGE_WIDTHS for ri in (False, True)
                    if not (ri and not fold)]          # the centred-image residual exists with the fold only
    return out


@pytest.mark.parametrize("case", chain_cases(), ids=lambda c: f"{route_id(c[:3])}-{c[3]}" + ("-fold" if c[4] else ""))
def test_epilogue_chains_against_fp64(case):
    """The four epilogue chains run_blocks builds, unfolded and folded, every route, against fp64 under the derived bounds.
    Where the residual goes in as a centred image the reference uses the number that image holds."""
    from pafuse_amd import ops
    mode, N, ri, chain, fold = case
    p = chain_case(N, chain, seed=1)
    resid = None
    if ri:   # production: the stream is stored centred; the image holds exactly r - mean(r) (X) or its 22-bit split (H)
        p["r"] = p["r"] - p["r"].mean(1, keepdim=True)
        split, join = (ops.hsplit_rows, ops.hjoin_rows) if mode == 3 else (ops.xsplit_rows, ops.xjoin_rows)
        resid = join(split(p["r"].contiguous()), *p["r"].shape)
    out = run(p["x"], p["w"], p["b"], p["r"], mode, resid_image=ri, in_place=ri, **chain_kwargs(p, fold))
    check_chain(out, chain_ref(p, mode, resid), fold, case, x_from_image=ri and mode == 3)


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_bounds_catch_a_dropped_slice(N, chain):
    """Sensitivity: mode 1 (one bf16 per operand - what losing two of the three slices leaves) against the bf16x3 bounds must
    fail every checked elementwise output and the head; mode 2 on the same data passes them."""
    p = chain_case(N, chain, seed=2)
    ref = chain_ref(p, 2)
    check_chain(run(p["x"], p["w"], p["b"], p["r"], 2, **chain_kwargs(p, False)), ref, False, (N, chain, "bf16x3"))
    bad = run(p["x"], p["w"], p["b"], p["r"], 1, **chain_kwargs(p, False))
    q = lambda name, bound: ((bad[name].double() - ref[name]).abs() / bound).max().item()
    assert q("x", ref["ex"]) > 1 and q("n", ref["en"]) > 1, (N, chain, q("x", ref["ex"]), q("n", ref["en"]))
    if "head" in ref:
        assert q("head", ref["ehead"]) > 1, (N, chain, q("head", ref["ehead"]))


@pytest.mark.parametrize("N", (256, 64))
def test_three_c_hidden_width(N):
    """fc2 with an MLP hidden width of 3C (mlp_ratio = 3, the largest pafuse_mixste2_weights.mlp_hidden allows)."""
    p = chain_case(N, "fc2_post_norm1", seed=3, kmul=3)
    for mode in (0, 2):
        check_chain(run(p["x"], p["w"], p["b"], p["r"], mode, **chain_kwargs(p, True)), chain_ref(p, mode), True, (N, mode))


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("N,M", [(384, 333), (256, 4160), (224, 4160), (224, 333), (128, 333)])
def test_training_chain_against_fp64(mode, N, M):
    """EPI_ROWLN_TRAIN with seeded row factors (temporal map) and the spatial-block-0 chain: pre, x and n within the bounds
    (row factor folded into S and |b|)."""
    p = chain_case(N, "fc2_spatial0_pos_norm1", M=M, seed=4)
    F, J = 9, 7
    nseq = (M + F * J - 1) // (F * J) * J
    rs = 1 + _normal((nseq,), 77, 0.3)
    m = torch.arange(M, device=DEV)
    f = rs[(m // (F * J)) * J + m % J].double()[:, None]
    out = run(p["x"], p["w"], p["b"], p["r"], mode, training=True, rowscale=rs, rs_map=(1, J, F * J), **chain_kwargs(p, False))
    x, w, b, r = p["x"].double(), p["w"].double(), p["b"].double(), p["r"].double()
    y = r + f * (x @ w.t() + b)
    S = f.abs() * (x.abs() @ w.abs().t())
    acc = f * (x @ w.t() + b)
    e = PROD[mode] * S + gam(6 * p["K"] + 1) * (1.01 * S + f.abs() * b.abs()) + U * acc.abs() + U * y.abs()
    assert ((out["pre"].double() - y).abs() <= e).all(), ((out["pre"].double() - y).abs() / e).max()
    pw, pb, peps = p["post"]
    z, ez, _ = ln64(y, e, pw.double(), pb.double(), peps, N)
    tab, pj, pf = p["pos"]
    z = z + tab.double()[(m // pj) % pf]
    ez = ez + U * z.abs()
    assert ((out["x"].double() - z).abs() <= ez).all(), ((out["x"].double() - z).abs() / ez).max()
    nw, nb, neps = p["next"]
    n, en, _ = ln64(z, ez, nw.double(), nb.double(), neps, N)
    assert ((out["n"].double() - n).abs() <= en).all(), ((out["n"].double() - n).abs() / en).max()


# -------------------------------------------------------------------------------------------------- (c) bit invariants
def _bits_equal(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k].double() - b[k].double()).abs().max().item())


INVARIANT_ROUTES = [(2, n, False) for n in WIDTHS] + [(0, 384, False), (0, 224, False), (1, 256, False)] + \
                   [(m, n, True) for m in (3, 4) for n in IMAGE_WIDTHS] + [(3, 256, False), (4, 224, False)]


@pytest.mark.parametrize("route", INVARIANT_ROUTES, ids=route_id)
def test_in_place_repeat_and_row_shift_give_the_same_bits(route):
    """out_x over its own residual equals out-of-place; a second launch equals the first; rows [s, s + M') of a launch equal
    a launch on those rows alone (s a multiple of the pos period, so every row keeps its pos entry: rows move across tile
    boundaries and, at 224, across the 64 / 128-row tile switch)."""
    mode, N, ri = route
    chain = "fc2_spatial0_pos_norm1"
    M = 4097 if N == 224 else 1000
    p = chain_case(N, chain, M=M, seed=5)
    for fold in (False, True):
        kw = chain_kwargs(p, fold)
        a = run(p["x"], p["w"], p["b"], p["r"], mode, resid_image=ri, **kw)
        if not ri:   # (the centred-image form is written in place inside the wrapper both ways: compare with a copy of r)
            b_ = run(p["x"], p["w"], p["b"], p["r"].clone(), mode, resid_image=ri, in_place=True, **kw)
            _bits_equal(a, b_, (route, fold, "in place"))
        _bits_equal(a, run(p["x"], p["w"], p["b"], p["r"], mode, resid_image=ri, **kw), (route, fold, "repeat"))
        for s, m2 in ((51, 100), (153, 700), (510, 490), (51 * 20, 2000), (51 * 40, 2057)):
            if s + m2 > M:
                continue
            sub = run(p["x"][s:s + m2].contiguous(), p["w"], p["b"], p["r"][s:s + m2].contiguous(), mode, resid_image=ri, **kw)
            for k in sub:
                assert torch.equal(sub[k], a[k][s:s + m2]), (route, fold, s, m2, k)


GROUPS = [
    [(384, 25920 // 16 + 5), (224, 73440 // 16 + 3), (256, 45360 // 16 + 7)],          # the three parts at P ~ 1: 27 / 36 / 45 tiles
    [(224, 4097), (384, 777)],
    [(256, 1001), (256, 65), (384, 130), (224, 5000)],
    [(224, 333), (384, 200)],                                                             # no grouped variant: part by part
]


@pytest.mark.parametrize("gi", range(len(GROUPS)))
@pytest.mark.parametrize("chain,fold", [(c, f) for c in CHAINS for f in ((False,) if CHAINS[c]["head"] else (False, True))])
def test_grouped_grid_equals_part_by_part(gi, chain, fold):
    """linear_rowln_group with the shared grid (grouped_rowln_kernel, the direct row-per-lane epilogue, slot table with padded
    first[] entries: tile counts not multiples of 8) against the per-part launches (slab epilogue): the same bits for every
    option chain; a layer the grouped kernel has no variant for (224 below 4096 rows) sends the whole group part by part."""
    from pafuse_amd import ops
    layers = []
    for i, (N, M) in enumerate(GROUPS[gi]):
        p = chain_case(N, chain, M=M, seed=10 + i)
        layers.append(dict(x=p["x"], weight=p["w"], bias=p["b"], resid=p["r"], precision="bf16x3", **chain_kwargs(p, fold)))
    shared = ops.linear_rowln_group(layers, shared_grid=True)
    apart = ops.linear_rowln_group(layers, shared_grid=False)
    single = [ops.linear_rowln(**layer) for layer in layers]
    for i in range(len(layers)):
        _bits_equal(shared[i], apart[i], (gi, chain, fold, i, "shared grid"))
        _bits_equal(apart[i], single[i], (gi, chain, fold, i, "group of one-by-one"))


# ---------------------------------------------------------------------------------------------------------- (d) guard band
def _nan_filled(n, dtype=torch.float32):
    t = torch.full((n,), NAN_BITS, dtype=torch.int32, device=DEV)
    return t.view(torch.float32) if dtype == torch.float32 else t.view(torch.uint8)


@pytest.mark.parametrize("route", routes() + [(2, 224, False, 4097)], ids=lambda r: route_id(r[:3]) + (f"-M{r[3]}" if len(r) > 3 else ""))
def test_nothing_is_written_past_row_M(route):
    """Every output in a buffer with 70 spare rows (ln_stats / out_head: spare entries) filled with a NaN bit pattern: after the
    launch the spare part holds exactly that pattern (dead rows of the last tile store nothing)."""
    mode, N, ri = route[:3]
    M = route[3] if len(route) > 3 else 129
    SP = 70
    eb = 6 if mode == 4 else 4
    for chain, fold in (("fc2_spatial0_pos_norm1", True), ("fc2_last_temporal_head", False), ("proj_norm2", False)):
        if ri and not fold:
            continue
        p = chain_case(N, chain, M=M, seed=6)
        bufs = {"x": _nan_filled((M + SP) * N), "n": _nan_filled((M + SP) * N), "stats": _nan_filled((M + SP) * 2),
                "head": _nan_filled((M + SP) * 3)}
        if mode >= 3:
            bufs["x_img"] = _nan_filled((M + SP) * N * eb // 4, torch.uint8)
            bufs["n_img"] = _nan_filled((M + SP) * N * eb // 4, torch.uint8)
        kw = chain_kwargs(p, fold)
        used = {k: v for k, v in bufs.items() if k in ("x", "x_img") or (k in ("n", "n_img") and not fold) or
                (k == "stats" and fold) or (k == "head" and "head" in kw)}
        if ri:
            used.pop("x")
        run(p["x"], p["w"], p["b"], p["r"], mode, resid_image=ri, out=dict(used), **kw)
        per_row = {"x": N, "n": N, "stats": 2, "head": 3, "x_img": N * eb, "n_img": N * eb}
        for k, t in used.items():
            tail = t.view(torch.uint8)[M * per_row[k] * (4 if t.dtype == torch.float32 else 1):]
            assert torch.equal(tail.view(torch.int32), torch.full_like(tail.view(torch.int32), NAN_BITS)), (route, chain, k)
            head = t.view(torch.uint8)[:M * per_row[k] * (4 if t.dtype == torch.float32 else 1)].view(torch.int32)
            assert not (head == NAN_BITS).all(), (route, chain, k, "nothing written")


# -------------------------------------------------------------------------------------------------------------- (e) refusals
def test_invalid_argument_sets_are_refused_before_any_launch():
    """Each inconsistent argument set returns its error code and pafuse_last_error() names the problem; M = 0 is a no-op.
    (Every pointer handed over is a real, large-enough buffer.)"""
    import ctypes as C
    from pafuse_amd import _lib, ops
    lib = _lib.load()
    N, M = 256, 64
    p = chain_case(N, "fc2_last_temporal_head", M=M, seed=7)
    base = dict(x=p["x"], weight=p["w"], bias=p["b"], resid=p["r"], precision="bf16x3")
    stream = torch.cuda.current_stream().cuda_stream
    keep = []

    def call(edit=None, n=1, **kw):
        a, k, _ = ops.rowln_args(**dict(base, **kw))
        keep.append(k)
        if edit:
            edit(a)
        if n == 1:
            return lib.pafuse_linear_rowln(C.byref(a), stream), lib.pafuse_last_error().decode()
        arr = (_lib.RowLNArgs * max(n, 1))(*([a] * max(n, 1)))
        return lib.pafuse_linear_rowln_group(arr, n, 1, stream), lib.pafuse_last_error().decode()

    E_ARG, E_SHAPE = -1, -2
    nxt, hd = p["next"], p["head"]
    stats = torch.zeros(M, 2, device=DEV)
    cases = [
        (dict(next=nxt, head=hd, edit=lambda a: setattr(a, "next_w", None) or setattr(a, "next_b", None)), E_ARG, "head without next"),
        (dict(next=nxt, fold=True, edit=lambda a: setattr(a, "next_w", None) or setattr(a, "next_b", None)), E_ARG, "ln_stats without next"),
        (dict(next=nxt, head=hd, edit=lambda a: setattr(a, "ln_stats", stats.data_ptr())), E_ARG, "ln_stats together with the head"),
        (dict(next=nxt, fold=True, edit=lambda a: setattr(a, "out_n", stats.data_ptr())), E_ARG, "out_n needs next"),
        (dict(pos=(p["post"][0][None].contiguous(), 0, 1)), E_ARG, "pos with posJ=0"),
        (dict(pos=(p["post"][0][None].contiguous(), 1, 0)), E_ARG, "posF=0"),
        (dict(edit=lambda a: setattr(a, "N", 192)), E_SHAPE, "no whole-row kernel for width 192"),
        (dict(precision="f16x2", edit=lambda a: setattr(a, "N", 288)), E_SHAPE, "no whole-row kernel for width 288"),
        (dict(edit=lambda a: setattr(a, "K", 240)), E_SHAPE, "K=240 must be a positive multiple of 32"),
        (dict(edit=lambda a: setattr(a, "Wsplit", None)), E_ARG, "mode 2 needs the layout-1 image"),
        (dict(precision="f16x2", edit=lambda a: setattr(a, "A_img", None)), E_ARG, "needs the images of A and W"),
        (dict(precision="bf16x3_images", edit=lambda a: setattr(a, "Wsplit", None)), E_ARG, "needs the images of A and W"),
        (dict(precision="bf16x3_images", resid_image=True, edit=lambda a: setattr(a, "resid", p["r"].data_ptr())), E_ARG,
         "exactly one residual"),
        (dict(precision="bf16", edit=lambda a: setattr(a, "training", 1)), E_ARG, "training runs modes 0 and 2 only"),
        (dict(edit=lambda a: setattr(a, "operand_bf16", 5)), E_ARG, "matrix-product mode 5"),
        (dict(n=0), E_ARG, "linear_rowln_group: 0 layers"),
        (dict(n=5), E_ARG, "linear_rowln_group: 5 layers"),
        (dict(n=2, training=True, rowscale=None), E_ARG, "training layers run one by one"),
    ]
    for kw, code, text in cases:
        kw = dict(kw)
        rc, msg = call(kw.pop("edit", None), kw.pop("n", 1), **kw)
        assert rc == code and text in msg, (kw, rc, msg)
    # M = 0: nothing is launched (every pointer may point anywhere: none is read)
    rc, _ = call(lambda a: setattr(a, "M", 0), next=nxt, head=hd)
    assert rc == 0
    torch.cuda.synchronize()

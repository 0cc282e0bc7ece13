"""GPU: the three kernels at the rim of the sampling loop, each held to a reference on its own (tests/loop_rim_reference.py;
tests/test_loop_rim_host.py proves those references against the oracle on a machine without a GPU).

  * embed_kernel      its arithmetic against fp64 at every width class; every output form the loop launches (folded LayerNorm,
                      H / X image, centred rows, no fp32 rows) bit for bit against the plain form; row windows bit for bit
                      against the full launch - all through pafuse_embed_unit, i.e. through the host function that fills the
                      loop's own launches
  * time_embed_kernel against fp64, with the oracle's fp32 evaluation as the yardstick
  * finalize_kernel   bit for bit against oracle.ddim_sample run on canned denoiser outputs, step by step over a whole chain, both
                      samplers (finalize_seeded_kernel: tests/test_hip_noise.py::test_seeded_loop_equals_the_buffer_loop_on_the_
                      same_normals holds the seeded loop torch.equal to the buffer loop fed ops.noise_fill's draws)

Every output buffer lies between guard rows of a sentinel that must survive.  Not reached here: the scalar-t path of
time_embed_kernel (the loop's; the unit entry passes a tensor of timesteps) and finalize's range flag (the unit entry passes none)."""
import pytest
import torch

from oracle import d3dp_oracle as orc
from pafuse_amd import synthetic as gu
from tests import loop_rim_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 3                  # guard rows on either side of every output
SENT, BYTE = -12345.0, 0xA5
EPS = 1e-6
PLAIN = ref.EMBED_FORMS[0]


class Guarded:
    """`rows` rows of `width` elements between `guard` sentinel rows before and as many after"""

    def __init__(self, rows, width, dtype=torch.float32, guard=G):
        self.n, self.w, self.g = rows, width, guard
        self.fill = SENT if dtype.is_floating_point else BYTE
        self.full = torch.full(((rows + 2 * guard) * width,), self.fill, dtype=dtype, device=DEV)
        self.flat = self.full[guard * width:(guard + rows) * width]

    def rows(self):
        return self.flat.view(self.n, self.w)

    def guards_intact(self):
        lo, hi = self.full[:self.g * self.w], self.full[(self.g + self.n) * self.w:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())

    def untouched_outside(self, row0=0, nrows=0):
        r = self.rows()
        return self.guards_intact() and bool((r[:row0] == self.fill).all()) and bool((r[row0 + nrows:] == self.fill).all())


def assert_as_close_as_fp32(what, got, truth, stmt32, lines=None, show=True):
    """the idiom of test_layernorm / test_attention_contiguous: as close to fp64 on average as the fp32 statement (x 1.5), and at
    the worst element within twice the statement's worst - or one final rounding of the largest output, which keeps a case where
    torch happens to be exact from failing"""
    err, err32 = (got.double() - truth).abs(), (stmt32.double() - truth).abs()
    floor = 2.0 ** -23 * float(truth.abs().max())
    line = (f"{what}: mean |err| {float(err.mean()):.3e} (fp32 statement {float(err32.mean()):.3e}), "
            f"max {float(err.max()):.3e} (statement {float(err32.max()):.3e}, 1 ulp of the largest {floor:.3e})")
    if show:
        print(line)
    if lines is not None:
        lines.append((float(err.mean()), float(err32.mean()), float(err.max()), float(err32.max())))
    assert float(err.mean()) <= 1.5 * float(err32.mean()) + 1e-9, line
    assert float(err.max()) <= max(2.0 * float(err32.max()), floor), line


# ------------------------------------------------------------------------------------------------------------------ embed
def embed_inputs(dims, C, flip, seed):
    B, P, Fr, J3, joints, sides = dims
    J = len(joints) if joints else J3
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    t = dict(x3d=rn(B, P, Fr, J3, 3), x2d=rn(B, Fr, J3, 2), pw=rn(C, 5) * 5 ** -0.5, pb=0.1 * rn(C), pos=0.1 * rn(J, C),
             temb=0.1 * rn(B, C), nw=1 + 0.1 * rn(C), nb=0.1 * rn(C))
    t["joints"], t["perm"], t["x2f"] = (None if joints is None else torch.tensor(joints, dtype=torch.int32)), None, None
    if flip:
        t["perm"] = orc.flip_permutation(*sides, J3).to(torch.int32)
        t["x2f"] = t["x2d"][:, :, t["perm"].long()].clone()
        t["x2f"][..., 0] *= -1
    t["M"], t["C"] = (2 if flip else 1) * B * P * Fr * J, C
    t["dev"] = {k: v.to(DEV) for k, v in t.items() if torch.is_tensor(v)}
    return t


def embed_statement(t, scale, dtype):
    return ref.embed_ref(t["x3d"], t["x2d"], t["pw"], t["pb"], t["pos"], t["temb"], t["nw"], t["nb"], EPS, joints=t["joints"],
                         perm=t["perm"], x2d_flip=t["x2f"], scale=scale, dtype=dtype)


def embed_buffers(t, form, nrows):
    from pafuse_amd import _lib
    M, C = t["M"], t["C"]
    # (the statistics' guards are as long as the token matrix: an index by the absolute row, or by a dead token, lands in them)
    b = dict(x=Guarded(M, C), xn=Guarded(M, C), stats=Guarded(nrows, 2, guard=M + 8))
    mode = _lib.PRECISIONS[form[0]]
    if mode in _lib.IMAGE_BYTES:
        b["image"] = Guarded(M, C * _lib.IMAGE_BYTES[mode], torch.uint8)
    return b


def written_by(form):
    from pafuse_amd import _lib
    precision, folded, h_only = form
    images = _lib.PRECISIONS[precision] in _lib.IMAGE_BYTES
    return {"x": not h_only, "xn": not images and not folded, "image": images, "stats": folded}


def embed_launch(t, scale, form=PLAIN, window=None, bufs=None):
    """one pafuse_embed_unit launch into guarded buffers (every buffer is handed over, also those the form must not write);
    -> the buffers, after the checks that hold for every launch: guards intact, rows outside the window and buffers outside the
    form untouched (`bufs` given: a launch on top of earlier ones, only the guards are checked)"""
    from pafuse_amd import ops
    d = t["dev"]
    row0, nrows = window or (0, t["M"])
    fresh = bufs is None
    bufs = bufs or embed_buffers(t, form, nrows)
    out = {k: (b.flat if k == "image" else b.rows()) for k, b in bufs.items()}
    if not fresh:
        out["stats"] = bufs["stats"].rows()[row0:row0 + nrows]      # where the loop's offset_rows puts a lane's statistics
    got = ops.embed_unit(d["x3d"], d["x2d"], d["pw"], d["pb"], d["pos"], d["temb"], d["nw"], d["nb"], EPS, joints=d.get("joints"),
                         perm=d.get("perm"), x2d_flip=d.get("x2f"), do_clamp=True, scale=scale, precision=form[0], folded=form[1],
                         h_residual_only=form[2], window=window, out=out)
    torch.cuda.synchronize()
    want = written_by(form)
    assert set(got) == {k for k, w in want.items() if w}
    for k, b in bufs.items():
        assert b.guards_intact(), (form, window, k)
        if fresh and not want[k]:
            assert b.untouched_outside(), (form, window, k, "written by a form that has no such output")
        elif fresh and k != "stats":
            assert b.untouched_outside(row0, nrows), (form, window, k, "rows outside the window written")
    return bufs


@pytest.mark.parametrize("C", ref.EMBED_WIDTHS)
def test_embed_arithmetic_against_fp64(C):
    """x = Linear(5 -> C) + position + time and xn = LayerNorm(x) with real weights at every class of width, the project's part
    sizes and joint lists, both scales (the clamp cuts on both sides), with and without the flipped half."""
    from pafuse_amd import ops
    worst = {"x": [], "xn": []}
    for n, dims in enumerate(ref.EMBED_DIMS):
        for scale in ref.EMBED_SCALES:
            for flip in (False, True):
                t = embed_inputs(dims, C, flip, seed=1000 + 10 * n + flip)
                assert bool((t["x3d"] > 1.1 * scale).any()) and bool((t["x3d"] < -1.1 * scale).any())
                truth, stmt = embed_statement(t, scale, torch.float64), embed_statement(t, scale, torch.float32)
                b = embed_launch(t, scale)
                for k in ("x", "xn"):
                    got = b[k].rows().cpu().view(truth[k].shape)
                    assert_as_close_as_fp32(f"embed C={C} dims={dims[:4]} scale={scale} flip={flip} {k}", got, truth[k], stmt[k],
                                            worst[k], show=False)               # (printed per width below)
                if n == 1:      # pafuse_embed is the same launch
                    d = t["dev"]
                    x, xn = ops.embed(d["x3d"], d["x2d"], d["pw"], d["pb"], d["pos"], d["temb"], d["nw"], d["nb"], EPS,
                                      joints=d.get("joints"), perm=d.get("perm"), x2d_flip=d.get("x2f"), do_clamp=True, scale=scale)
                    assert torch.equal(x.view(-1, C), b["x"].rows()) and torch.equal(xn.view(-1, C), b["xn"].rows())
    for k, v in worst.items():
        print(f"embed C={C} {k}: over {len(v)} launches mean |err| <= {max(a[0] for a in v):.3e} (fp32 statement <= "
              f"{max(a[1] for a in v):.3e}), max |err| <= {max(a[2] for a in v):.3e} (statement <= {max(a[3] for a in v):.3e})")


@pytest.mark.parametrize("C", ref.IMAGE_WIDTHS)
def test_embed_forms_equal_the_plain_form(C):
    """every other (product mode, folded LayerNorm, H-residual-only) form - nine, over all five product modes - writes the plain
    form's numbers: 'bf16' and unfolded 'bf16x3' the plain launch itself, the rest the same rows, the
    images of the same normalised rows, and - folded - statistics as close to fp64 as torch's, rows centred on the STORED mean
    and the images of exactly those."""
    from pafuse_amd import ops
    for dims, flip, scale in ((ref.EMBED_DIMS[1], True, 0.3), (ref.EMBED_DIMS[3], True, 1.0)):
        t = embed_inputs(dims, C, flip, seed=2000 + C)
        M = t["M"]
        plain = embed_launch(t, scale)
        x_plain, xn_plain = plain["x"].rows(), plain["xn"].rows()
        x64 = x_plain.cpu().double()
        stats64 = torch.stack((x64.mean(-1), 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + EPS)), -1)
        x32 = x_plain.cpu()
        stats32 = torch.stack((x32.mean(-1), (x32.var(-1, unbiased=False) + EPS).rsqrt()), -1)
        for form in ref.EMBED_FORMS[1:]:
            precision, folded, h_only = form
            b = embed_launch(t, scale, form)
            split = {"f16x2": ops.hsplit_rows, "bf16x3_images": ops.xsplit_rows}.get(precision)
            if not folded:
                assert torch.equal(b["x"].rows(), x_plain), form
                if split is None:
                    assert torch.equal(b["xn"].rows(), xn_plain), form
                else:
                    assert torch.equal(b["image"].flat, split(xn_plain.contiguous())), form
                if precision == "bf16x3_images":
                    assert torch.equal(ops.xjoin_rows(b["image"].flat, M, C), xn_plain), form
                continue
            stats = b["stats"].rows().cpu()
            for i, name in enumerate(("mean", "rstd")):
                assert_as_close_as_fp32(f"embed C={C} dims={dims[:4]} folded {name}", stats[:, i], stats64[:, i], stats32[:, i],
                                        show=form == ref.EMBED_FORMS[2])        # (the same numbers in every folded form)
            centred = (x_plain.cpu() - stats[:, :1]).to(DEV)          # one fp32 subtraction per element: nothing can contract
            if split is None:                                        # 'bf16x3': the fp32 rows themselves are stored centred
                assert torch.equal(b["x"].rows(), centred), form
                continue
            assert torch.equal(b["image"].flat, split(centred.contiguous())), form
            if not h_only:                                           # the image pipelines keep the plain rows beside the image
                assert torch.equal(b["x"].rows(), x_plain), form
            if precision == "bf16x3_images":
                assert torch.equal(ops.xjoin_rows(b["image"].flat, M, C), centred), form


@pytest.mark.parametrize("C", [64, 288])
@pytest.mark.parametrize("form", ref.WINDOW_FORMS, ids=lambda f: f"{f[0]}{'-folded' if f[1] else ''}{'-honly' if f[2] else ''}")
def test_embed_windows_equal_the_full_launch(form, C):
    """a launch over rows [row0, row0 + nrows) writes those rows of the full launch, bit for bit, and nothing else: rows and
    image by the absolute row, the statistics from index 0 of the pointer it was handed.  45 rows = 5 (mod 8), so the last
    workgroup of most windows replays a row in its dead half-waves."""
    t = embed_inputs(ref.WINDOW_DIMS, C, False, seed=3000 + C)
    assert t["M"] == ref.WINDOW_ROWS
    full = embed_launch(t, 0.3, form)
    keys = [k for k, w in written_by(form).items() if w]
    for row0, nrows in ref.WINDOWS:
        b = embed_launch(t, 0.3, form, window=(row0, nrows))         # (checks that nothing outside the window is written)
        for k in keys:
            if k == "stats":
                assert b[k].n == nrows and torch.equal(b[k].rows(), full[k].rows()[row0:row0 + nrows]), (row0, nrows, k)
            else:
                assert torch.equal(b[k].rows()[row0:row0 + nrows], full[k].rows()[row0:row0 + nrows]), (row0, nrows, k)
    # three lanes into the same buffers, each handed the statistics pointer of its first row: together the full launch
    lanes = embed_buffers(t, form, t["M"])
    for window in ref.WINDOWS[-3:]:
        embed_launch(t, 0.3, form, window=window, bufs=lanes)
    for k, buf in lanes.items():
        assert torch.equal(buf.full, full[k].full), k


# --------------------------------------------------------------------------------------------------------- time embedding
@pytest.mark.parametrize("C", ref.TIME_WIDTHS)
def test_time_embed_against_fp64(C):
    import pafuse_amd
    from pafuse_amd import ops
    m = pafuse_amd.MixSTE2(2, 2, 5, C, 1, 8, drop_path_rate=0.0, is_train=False)
    sd = {k: gu.seeded_tensor(f"loop_rim.{C}.time_mlp.{k}", v.shape, 31) for k, v in m.time_mlp.state_dict().items()}
    m.time_mlp.load_state_dict(sd)
    t = torch.tensor(ref.TIME_STEPS)
    freqs = m._freqs.clone()
    truth = ref.time_embed_ref(t, freqs, sd["1.weight"], sd["1.bias"], sd["3.weight"], sd["3.bias"])
    stmt = orc.timestep_embedding({"time_mlp." + k: v for k, v in sd.items()}, "", t, C)
    out = Guarded(len(t), C)
    got = ops.time_embed(m.to(DEV), t.to(DEV), out=out.rows())
    torch.cuda.synchronize()
    assert got.data_ptr() == out.rows().data_ptr() and out.guards_intact()
    assert_as_close_as_fp32(f"time_embed C={C}", out.rows().cpu(), truth, stmt)


# ---------------------------------------------------------------------------------------------------------------- finalize
@pytest.fixture(scope="module")
def sampler():
    """the model's own step scalars at sampling_timesteps = 4, and the schedule buffers the oracle reads"""
    from __graft_entry__ import make_model
    model, sd = make_model(1, ref.FINALIZE_T, device="cpu", depth=1)
    steps = model.ddim_steps()
    assert [s.time for s in steps] == [p[0] for p in orc.ddim_time_pairs(1000, ref.FINALIZE_T)] and steps[ref.FINALIZE_T - 1].last
    return steps, sd


def same_bits(a, b):
    """equal, NaNs in the same places (their payloads are not compared)"""
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def run_finalize_chain(case, scale, flip, sampler, plant=None):
    from pafuse_amd import ops
    steps, sd = sampler
    c = ref.FINALIZE_CASES[case]
    B, P, Fr, parts, T = c["B"], c["P"], c["F"], c["parts"], ref.FINALIZE_T
    J = sum(len(p) for p in parts)
    g = torch.Generator().manual_seed(4000 + J + flip)
    rnd = lambda s: torch.randn(B, P, Fr, J, 3, generator=g) * s      # noqa: E731
    noises = [rnd(1.0) for _ in range(T)]
    preds = [(rnd(0.7), rnd(0.7)) if flip else rnd(0.7) for _ in range(T)]
    if plant is not None:
        plant(preds)
    x0_ref, img_ref = ref.oracle_chain(sd, preds, noises, T, scale, *((c["left"], c["right"]) if flip else ()))
    lim = ref.f32_scalar(1.1 * scale)
    assert bool((x0_ref == lim).any()) and bool((x0_ref == -lim).any())            # the clamp cuts on both sides
    joint_part, joint_local = torch.empty(J, dtype=torch.int32), torch.empty(J, dtype=torch.int32)
    for i, idx in enumerate(parts):
        joint_part[idx], joint_local[idx] = i, torch.arange(len(idx), dtype=torch.int32)
    perm = orc.flip_permutation(c["left"], c["right"], J).to(torch.int32).to(DEV) if flip else None
    n = B * P * Fr * J * 3
    img_buf, out_buf = Guarded(1, n), Guarded(1, T * n)
    img, out = img_buf.flat.view(B, P, Fr, J, 3), out_buf.flat.view(B, T, P, Fr, J, 3)
    img.copy_(noises[0])
    for k in range(T):
        halves = preds[k] if flip else (preds[k],)
        dev_preds = [torch.stack([h[..., idx, :] for h in halves]).contiguous().to(DEV) for idx in parts]
        ops.ddim_finalize(dev_preds, joint_part.to(DEV), joint_local.to(DEV), img, steps[k],
                          noise=None if steps[k].last else noises[k + 1].to(DEV), flip_perm=perm, scale=scale, T=T, step=k, out=out)
        torch.cuda.synchronize()
        got = out.cpu()
        assert same_bits(got[:, :k + 1], x0_ref[:, :k + 1]), (case, scale, flip, k, "x0")
        assert bool((got[:, k + 1:] == SENT).all()), (k, "a later slot of out was written")
        assert same_bits(img.cpu(), img_ref[k]), (case, scale, flip, k, "img",
                                                 float((img.cpu() - img_ref[k]).abs().nan_to_num().max()))
        assert img_buf.guards_intact() and out_buf.guards_intact()
    assert same_bits(img.cpu(), x0_ref[:, T - 1])                                    # the last step leaves x0 in img
    return x0_ref, got


@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
@pytest.mark.parametrize("scale", ref.FINALIZE_SCALES)
@pytest.mark.parametrize("case", list(ref.FINALIZE_CASES))
def test_finalize_chain_equals_the_oracle_bit_for_bit(case, scale, flip, sampler):
    """T = 4 steps of pafuse_ddim_finalize on one img and one out against the reference's own lines (un-flip, TTA mean, scale,
    clamp, fp64 epsilon, the update with torch's scalar demotion per sampler): x0 and img after EVERY step, torch.equal."""
    x0_ref, got = run_finalize_chain(case, scale, flip, sampler)
    assert not bool(x0_ref.isnan().any()) and torch.equal(got, x0_ref)


def test_finalize_carries_nan_and_inf_where_the_oracle_does(sampler):
    """a NaN, a +inf and a -inf planted in the predictions of step 1 come out where the reference puts them (the NaN stays a NaN
    through the clamp and rides img until the last step; an infinity is clamped) and nowhere else."""
    def plant(preds):
        plain, flipped = preds[1]
        plain[0, 1, 0, 2, 1] = float("nan")
        plain[1, 0, 1, 3, 0] = float("inf")
        flipped[1, 2, 0, 130, 2] = float("-inf")

    x0_ref, got = run_finalize_chain("parts134", 1.0, True, sampler, plant)
    clean, _ = run_finalize_chain("parts134", 1.0, True, sampler)
    assert int(x0_ref.isnan().sum()) >= 1 and int((x0_ref != clean).sum()) <= 8      # the oracle shows them, in a few elements
    assert same_bits(got, x0_ref)
    assert torch.equal(got[x0_ref == clean], clean[x0_ref == clean])                 # the neighbours are untouched

"""CPU-only: the statements of tests/loop_rim_reference.py (what tests/test_hip_loop_rim.py holds time_embed_kernel, embed_kernel
and finalize_kernel to) equal the oracle where the oracle has the piece, the canned-denoiser chain is the oracle's own sampler,
the case tables contain every form they claim, and pafuse_embed_unit refuses bad operands before it launches anything."""
import ctypes as C

import torch

from oracle import d3dp_oracle as orc
from pafuse_amd import synthetic as gu
from tests import loop_rim_reference as ref

E_ARG, E_SHAPE = -1, -2


def _mixste(Fr, J, width, seed):
    import pafuse_amd
    m = pafuse_amd.MixSTE2(Fr, J, 5, width, 1, 8, drop_path_rate=0.0, is_train=False)
    return m, gu.seeded_like(m.state_dict(), seed=seed)


def test_statements_in_fp32_equal_the_oracle():
    Fr, J3, width, B, P = 3, 7, 32, 2, 3
    idx, left, right = [5, 0, 3, 6, 2], [1, 3, 5], [2, 4, 6]
    m, sd = _mixste(Fr, len(idx), width, seed=5)
    g = torch.Generator().manual_seed(11)
    x2d, x3d = torch.randn(B, Fr, J3, 2, generator=g), torch.randn(B, P, Fr, J3, 3, generator=g)
    t = torch.tensor([999, 250])
    # the timestep embedding, bit for bit - and the table of frequencies the kernel is handed is the oracle's
    temb = orc.timestep_embedding(sd, "", t, width)
    tm = [sd[f"time_mlp.{k}"] for k in ("1.weight", "1.bias", "3.weight", "3.bias")]
    assert torch.equal(m._freqs, orc.sinusoid_frequencies(width))
    assert torch.equal(ref.time_embed_ref(t, m._freqs, *tm, dtype=torch.float32), temb)
    assert torch.allclose(ref.time_embed_ref(t, m._freqs, *tm).float(), temb, rtol=0, atol=1e-5)
    # the embed stage: the first lines of mixste2_eval at depth 1 (tap "embed") and its first LayerNorm, on the inputs the
    # flip sampler makes for the plain and for the flipped call (oracle.model_predictions_flip's own lines)
    scale = 0.3
    x_t = torch.clamp(x3d, min=-1.1 * scale, max=1.1 * scale) / scale
    lr, rl = left + right, right + left
    x_f = x_t.clone()
    x_f[..., 0] *= -1
    x_f[:, :, :, lr] = x_f[:, :, :, rl]
    x2f = x2d.clone()
    x2f[..., 0] *= -1
    x2f[:, :, lr] = x2f[:, :, rl]
    perm = orc.flip_permutation(left, right, J3)
    got = ref.embed_ref(x3d, x2d, sd["Spatial_patch_to_embedding.weight"], sd["Spatial_patch_to_embedding.bias"],
                        sd["Spatial_pos_embed"][0], temb, sd["STEblocks.0.norm1.weight"], sd["STEblocks.0.norm1.bias"], 1e-6,
                        joints=idx, perm=perm, x2d_flip=x2f, scale=scale, dtype=torch.float32)
    assert got["x"].shape == (2, B, P, Fr, len(idx), width) and got["mean"].shape == got["rstd"].shape == (2, B, P, Fr, len(idx))
    assert bool((x3d.abs() > 1.1 * scale).any()) and bool((x3d.abs() < 1.1 * scale).any())       # the clamp cuts, not everywhere
    for half, (a2, a3) in enumerate(((x2d, x_t), (x2f, x_f))):
        taps = {}
        orc.mixste2_eval(sd, "", a2[..., idx, :], a3[..., idx, :], t, depth=1, heads=8, taps=taps)
        assert torch.equal(got["x"][half].reshape(-1, len(idx), width), taps["embed"]), half
        assert torch.equal(got["xn"][half].reshape(-1, len(idx), width), orc._layer_norm(sd, "STEblocks.0.norm1", taps["embed"], 1e-6))
    # the intermediates are those of that LayerNorm
    d = ref.embed_ref(x3d, x2d, sd["Spatial_patch_to_embedding.weight"], sd["Spatial_patch_to_embedding.bias"],
                      sd["Spatial_pos_embed"][0], temb, sd["STEblocks.0.norm1.weight"], sd["STEblocks.0.norm1.bias"], 1e-6, joints=idx,
                      scale=scale)
    again = d["xc"] * d["rstd"][..., None] * sd["STEblocks.0.norm1.weight"].double() + sd["STEblocks.0.norm1.bias"].double()
    assert torch.allclose(again, d["xn"], rtol=0, atol=1e-12) and torch.allclose(d["x"].float(), got["x"][:1], rtol=0, atol=1e-5)


def test_canned_chain_is_the_oracle_s_sampler():
    sd = orc.schedule_buffers()
    B, P, Fr, J, left, right = 2, 3, 2, 5, [1, 3], [2, 4]
    g = torch.Generator().manual_seed(12)
    rnd = lambda s=1.0: torch.randn(B, P, Fr, J, 3, generator=g) * s      # noqa: E731
    noises, preds = [rnd(), rnd()], [(rnd(0.7), rnd(0.7)), (rnd(0.7), rnd(0.7))]
    keep = (orc.predict_parts, orc._eps_from_x0)
    (time, time_next), _ = orc.ddim_time_pairs(1000, 2)
    t = torch.full((B,), time, dtype=torch.long)
    x2d = torch.zeros(B, Fr, J, 2)
    sqrt_an, c, sigma = orc.ddim_coefficients(sd["alphas_cumprod"], time, time_next, 1.0)
    for scale in (1.0, 0.3):
        # flip sampler: step 0 of the chain is model_predictions_flip on the canned pair, then the sampler's update line
        x0s, imgs = ref.oracle_chain(sd, preds, noises, 2, scale, left, right)
        with ref.canned_denoiser(list(preds[0])):
            eps, x0 = orc.model_predictions_flip(sd, noises[0], x2d, x2d, t, left, right, scale)
        assert eps.dtype == torch.float32 and torch.equal(x0s[:, 0], x0)
        assert torch.equal(imgs[0], x0 * sqrt_an + c * eps + sigma * noises[1]) and imgs[0].dtype == torch.float32
        assert torch.equal(imgs[1], x0s[:, 1]) and len(imgs) == 2
        un = preds[0][1].clone()                                  # the un-flip the chain applied, spelled with the permutation
        un[..., 0] *= -1
        un = un[:, :, :, orc.flip_permutation(left, right, J)]
        assert torch.equal(x0, torch.clamp(((preds[0][0] + un) / 2) * scale, min=-1.1 * scale, max=1.1 * scale))
        assert bool((x0.abs() == ref.f32_scalar(1.1 * scale)).any())       # the clamp cuts
        # no-flip sampler: epsilon stays fp64, img is cast at the end of the update
        x0s, imgs = ref.oracle_chain(sd, [p[0] for p in preds], noises, 2, scale)
        with ref.canned_denoiser([preds[0][0]]):
            eps, x0 = orc.model_predictions_noflip(sd, noises[0], x2d, t, scale)
        assert eps.dtype == torch.float64 and torch.equal(x0s[:, 0], x0)
        assert torch.equal(imgs[0], (x0 * sqrt_an + c * eps + sigma * noises[1]).float())
    assert (orc.predict_parts, orc._eps_from_x0) == keep           # both originals are back


def test_case_tables_contain_every_form_they_claim():
    # embed widths: every round of 32 lanes from empty through partly filled to full
    assert {C: C // 4 for C in ref.EMBED_WIDTHS} == {4: 1, 64: 16, 128: 32, 132: 33, 224: 56, 256: 64, 288: 72, 384: 96}
    forms = {C: ref.embed_quads(C) for C in ref.EMBED_WIDTHS}
    assert forms[4] == forms[64] == ("part", "empty", "empty") and forms[128] == ("full", "empty", "empty")
    assert forms[132] == forms[224] == ("full", "part", "empty") and forms[256] == ("full", "full", "empty")
    assert forms[288] == ("full", "full", "part") and forms[384] == ("full", "full", "full")
    assert {f[i] for f in forms.values() for i in (1, 2)} == {"empty", "part", "full"}
    assert set(ref.IMAGE_WIDTHS) == {64, 224, 256, 288, 384} and all(C % 32 == 0 for C in ref.IMAGE_WIDTHS)
    dims = ref.EMBED_DIMS
    for B, P, Fr, J3, joints, _ in dims[:2]:
        assert len({B, P, Fr, len(joints) if joints else J3}) == 4
    assert dims[0][4] is None and list(dims[1][4]) != sorted(dims[1][4])          # identity, and a gather out of order
    assert [(d[2], len(d[4]), d[3]) for d in dims[2:]] == [(2, 24, 134), (2, 68, 134), (2, 42, 134)]
    assert any((2 * B * P * Fr * (len(j) if j else J3)) % 8 for B, P, Fr, J3, j, _ in dims)       # a dead half-wave somewhere
    assert set(ref.EMBED_SCALES) == {1.0, 0.3}
    # every (mode, folded, H-only) the loop can derive, over EVERY product mode the library names (a new mode cannot be left
    # out silently): folded in the split modes only, H-only in the folded image pipelines only
    from pafuse_amd import _lib
    assert set(_lib.PRECISIONS) == {"f32", "bf16", "bf16x3", "f16x2", "bf16x3_images"} and set(_lib.SPLIT_FLAG) <= set(_lib.PRECISIONS.values())
    want = {(p, f, h) for p, mode in _lib.PRECISIONS.items() for f in (False, True) for h in (False, True)
            if (not f or mode in _lib.SPLIT_FLAG) and (not h or (f and mode in _lib.IMAGE_BYTES))}
    assert {p for p, _, _ in ref.EMBED_FORMS} == set(_lib.PRECISIONS)
    assert set(ref.EMBED_FORMS) == want and len(ref.EMBED_FORMS) == len(want) == 10 and ref.EMBED_FORMS[0] == ("f32", False, False)
    # windows
    B, P, Fr, J3, joints, flip = ref.WINDOW_DIMS
    M = ref.WINDOW_ROWS
    assert flip is None and M == B * P * Fr * len(joints) and M % 8 == 5
    w = ref.WINDOWS
    assert w[:4] == [(0, M), (0, 1), (1, 1), (3, 8)] and (M - 3, 3) in w and any(r % 2 and n % 2 and n > 1 for r, n in w)
    lanes = w[-3:]
    assert [r for r, _ in lanes] == [0, lanes[0][1], lanes[0][1] + lanes[1][1]] and sum(n for _, n in lanes) == M
    assert all(n == Fr * len(joints) and n % 8 for _, n in lanes) and all(0 <= r and r + n <= M for r, n in w)
    assert {(f, bool(ref_images(p))) for p, f, _ in ref.WINDOW_FORMS} == {(False, False), (True, False), (True, True)}
    assert set(ref.WINDOW_FORMS) <= set(ref.EMBED_FORMS)
    # the rest
    assert set(ref.TIME_WIDTHS) == {64, 224, 256, 288, 384} and ref.TIME_STEPS == (0, 1, 2, 250, 499, 998, 999)
    assert ref.FINALIZE_T == 4 and set(ref.FINALIZE_SCALES) == {1.0, 0.3}
    big, small = ref.FINALIZE_CASES["parts134"], ref.FINALIZE_CASES["one_part5"]
    assert [len(p) for p in big["parts"]] == [24, 68, 42] and sorted(sum(big["parts"], [])) == list(range(134))
    assert small["parts"] == [[0, 1, 2, 3, 4]]
    for case in (big, small):
        assert (case["B"], case["P"], case["F"]) == (2, 3, 2)
        assert (case["B"] * case["P"] * case["F"] * sum(len(p) for p in case["parts"])) % 256


def ref_images(precision):
    from pafuse_amd import _lib
    return _lib.PRECISIONS[precision] in _lib.IMAGE_BYTES


def test_embed_unit_refuses_before_any_launch():
    """every refusal happens before the first HIP call: the pointers are host memory and are never followed"""
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    L = _lib.load()
    assert _lib.ABI_VERSION == 8 and L.pafuse_abi_version() == 8          # the new entry is additive: no struct changed
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(**kw):
        a = _lib.EmbedArgs()
        for n in ("x3d", "x2d", "patch_w", "patch_b", "pos_spatial", "temb", "norm_w", "norm_b", "x", "xn", "image", "stats"):
            setattr(a, n, p)
        a.norm_eps, a.scale = 1e-6, 1.0
        a.B, a.P, a.F, a.J, a.J3, a.C, a.nflip, a.do_clamp = 1, 2, 3, 4, 4, 64, 1, 1
        a.row0, a.nrows = 0, 24
        for n, v in kw.items():
            setattr(a, n, v)
        return L.pafuse_embed_unit(C.byref(a), None)

    def refused(rc, code, word):
        assert rc == code, (rc, L.pafuse_last_error())
        assert word in L.pafuse_last_error(), L.pafuse_last_error()

    assert L.pafuse_embed_unit(None, None) == E_ARG
    # what pafuse_embed refuses
    refused(call(x3d=None), E_ARG, b"null")
    refused(call(J3=8), E_ARG, b"joint list")
    refused(call(nflip=2), E_ARG, b"flipped half")
    refused(call(C=66), E_SHAPE, b"C=66")
    refused(call(C=388), E_SHAPE, b"C=388")
    refused(call(scale=0.0), E_ARG, b"scale")
    # the form
    refused(call(operand_bf16=5), E_ARG, b"mode 5")
    refused(call(operand_bf16=-1), E_ARG, b"mode -1")
    for mode in (0, 1):
        refused(call(operand_bf16=mode, ln_folded=1), E_ARG, b"folded")
    for mode, folded in ((0, 0), (2, 1), (3, 0), (4, 0)):
        refused(call(operand_bf16=mode, ln_folded=folded, h_residual_only=1), E_ARG, b"H-residual-only")
    # a window outside the token matrix (24 rows)
    for row0, nrows in ((0, 25), (24, 1), (-1, 2), (0, 0), (3, -1), (23, 2), (1 << 62, 1 << 62)):
        refused(call(row0=row0, nrows=nrows), E_ARG, b"outside")
    # an image at a width its layout does not allow: H images in sub-blocks of 8, X images in chunks of 32
    refused(call(operand_bf16=3, C=4), E_SHAPE, b"H image")
    refused(call(operand_bf16=3, C=132), E_SHAPE, b"H image")
    refused(call(operand_bf16=4, C=8), E_SHAPE, b"X image")
    refused(call(operand_bf16=4, C=72), E_SHAPE, b"X image")
    refused(call(operand_bf16=4, ln_folded=1, h_residual_only=1, C=132), E_SHAPE, b"X image")
    # missing outputs
    for mode in (0, 1, 2):
        refused(call(operand_bf16=mode, xn=None), E_ARG, b"no xn")
        refused(call(operand_bf16=mode, x=None), E_ARG, b"no x")
    refused(call(operand_bf16=2, ln_folded=1, x=None), E_ARG, b"no x")
    refused(call(operand_bf16=2, ln_folded=1, stats=None), E_ARG, b"no stats")
    for mode in (3, 4):
        refused(call(operand_bf16=mode, image=None), E_ARG, b"no image")
        refused(call(operand_bf16=mode, x=None), E_ARG, b"no x")
        refused(call(operand_bf16=mode, ln_folded=1, x=None), E_ARG, b"no x")
        refused(call(operand_bf16=mode, ln_folded=1, stats=None), E_ARG, b"no stats")
        refused(call(operand_bf16=mode, ln_folded=1, h_residual_only=1, image=None), E_ARG, b"no image")
        refused(call(operand_bf16=mode, ln_folded=1, h_residual_only=1, x=None, stats=None), E_ARG, b"no stats")
    assert not any(buf)                                                # nothing was written through the host pointers


def test_embed_unit_python_layer_refuses_before_touching_the_device():
    import pytest
    from pafuse_amd import ops
    z = torch.zeros
    args = (z(1, 2, 3, 4, 3), z(1, 3, 4, 2), z(64, 5), z(64), z(4, 64), z(1, 64), z(64), z(64))
    # (all operands are host tensors, so a call that got past its refusal would still raise - on the buffers' device; each
    # case is therefore held to the words of ITS refusal)
    for kw, words in ((dict(precision="fp8"), "precision must be one of"),
                      (dict(window=(0, 25)), r"window \(0, 25\) outside the 24 rows"),
                      (dict(window=(24, 1)), r"window \(24, 1\) outside"), (dict(window=(0, 0)), r"window \(0, 0\) outside"),
                      (dict(window=(-1, 2)), r"window \(-1, 2\) outside"),
                      (dict(folded=True), "folded LayerNorm exists in"), (dict(precision="bf16", folded=True), "folded LayerNorm exists in"),
                      (dict(precision="bf16x3", folded=True, h_residual_only=True), "h_residual_only is a folded image"),
                      (dict(precision="f16x2", h_residual_only=True), "h_residual_only is a folded image"),
                      (dict(out={"y": z(1)}), "out holds x / xn / image / stats")):
        with pytest.raises(ValueError, match=words):
            ops.embed_unit(*args, **kw)
    wide = (z(1, 2, 3, 4, 3), z(1, 3, 4, 2), z(132, 5), z(132), z(4, 132), z(1, 132), z(132), z(132))
    with pytest.raises(ValueError, match="no f16x2 image at C = 132"):
        ops.embed_unit(*wide, precision="f16x2")
    with pytest.raises(ValueError, match="no bf16x3_images image at C = 132"):
        ops.embed_unit(*wide, precision="bf16x3_images")
    with pytest.raises(ValueError, match="no bf16x3_images image at C = 72"):       # an H image exists at 72, an X image does not
        ops.embed_unit(z(1, 2, 3, 4, 3), z(1, 3, 4, 2), z(72, 5), z(72), z(4, 72), z(1, 72), z(72), z(72), precision="bf16x3_images")

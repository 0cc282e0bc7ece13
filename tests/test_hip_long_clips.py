"""GPU tests of 243-frame clips: the long-sequence attention kernels (forward attn_long_kernel for 144 < L <= 256, backward
attn_backward_long_kernel for 80 < L <= 256 where the FMA kernel's two L x L planes do not fit the LDS) on their own, and the
denoiser, the DDIM loop and a training step at F = 243 against the CPU oracle, the DDIM loop against the reference's own
output (golden G22), and the two example scripts at 243 frames.

Bounds, derived:
  * attention forward.  Every output is a convex combination of L values of V, formed from fp32 products summed in a fixed
    order: the kernel's error against fp64 is that of any fp32 evaluation, a few ulps of O(1) numbers, 1e-7 .. 1e-6 for the
    N(0, 1) inputs here.  Asserted: max <= 2e-6 absolute (the bound test_attention_contiguous uses at L <= 144) and mean
    <= 1.5 x the mean error of torch's own fp32 attention against the same fp64 truth.  Long rows change the constant, not
    the form: the softmax sum runs over 243 terms instead of 27, and torch's fp32 error grows with it.
  * attention backward.  dq, dk, dv are sums over L of products of O(1) fp32 numbers.  Asserted per output against fp64
    autograd: max <= 2 x and mean <= 1.5 x torch fp32 autograd's error on the same inputs, plus a floor of 1e-7 x the
    gradient's scale (torch's error can be exactly 0 on a few entries).  The key-blocked softmax statistics (an online sum
    rescaled when the max grows) add at most a few ulps of relative error to 1 / sum, which the 2 x max covers.
  * the denoiser at F = 243 (one part per width, depth 2, B = 1, P = 2): the HIP output is about as far from an fp64
    evaluation of the same function as the oracle's fp32 evaluation is: 1.5 x mean, 2 x max, the rule
    test_hip_parity.test_accuracy_equivalent_to_reference_fp32 applies to one denoiser call at 27 frames (measured at
    F = 243 on MI355X: up to 1.25 x the oracle's mean error; the two sides sum in different orders).
  * the DDIM loop at F = 243 (full widths, depth 2, P = 2, T = 2): pointwise 1e-5 m, the parity tests' bound after 16 blocks
    x T steps (this is 4 blocks x 2 steps), and |dMPJPE| <= 5e-4 mm, the parity tests' blanket bound.
  * training at F = 243 (B = 2 clips, depth 2): the forward output within 1e-5 and every parameter gradient within
    2e-4 x the tensor's largest entry of torch autograd over the oracle, test_hip_train's bounds for depth 2.
"""
import pytest
import torch

from oracle import d3dp_oracle as orc
from tests.golden import golden_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = (145, 160, 200, 243, 256)
WIDTHS = (384, 224, 256)   # body, face, hands at 8 heads: d = 48, 28, 32


def _rows(nseq, L, temporal, other):
    """index tensors of the rows of each sequence; temporal: rows (r, t, j) = (r L + t) other + j, sequence s = (r, j)"""
    if temporal:
        return [torch.arange(L) * other + (s // other) * L * other + s % other for s in range(nseq)]
    return [torch.arange(L) + s * L for s in range(nseq)]


def _kw(L, temporal, other):
    return dict(group=other, group_stride=L * other, seq_stride=1, tok_stride=other) if temporal else {}


def _attention(qkv, heads, rows_of):
    """softmax(q k^T d^-1/2) v per sequence and head in the dtype of qkv (autograd-able)"""
    M, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    o = torch.zeros(M, C, dtype=qkv.dtype)
    for rows in rows_of:
        x = qkv[rows].reshape(len(rows), 3, heads, d)
        q, k, v = x[:, 0].transpose(0, 1), x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)
        p = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, dim=-1)
        o = o.index_put((rows,), (p @ v).transpose(0, 1).reshape(len(rows), C))
    return o


def _case(L, C, temporal, seed, qk_gain=1.0):
    heads, other = 8, 3
    nseq = 2 * other
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(nseq * L, 3 * C, generator=g)
    qkv[:, :2 * C] *= qk_gain
    return qkv, heads, nseq, _rows(nseq, L, temporal, other), _kw(L, temporal, other)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("temporal", [False, True])
def test_long_attention_forward_vs_fp64(L, C, temporal):
    from pafuse_amd import ops
    qkv, heads, nseq, rows_of, kw = _case(L, C, temporal, 10 * L + C + temporal)
    out = ops.attention(qkv.to(DEV), heads, nseq, L, **kw).cpu().double()
    truth = _attention(qkv.double(), heads, rows_of)
    err, err_t = (out - truth).abs(), (_attention(qkv, heads, rows_of).double() - truth).abs()
    assert float(err.max()) <= 2e-6, float(err.max())
    assert float(err.mean()) <= 1.5 * float(err_t.mean()) + 1e-9, (float(err.mean()), float(err_t.mean()))


@pytest.mark.parametrize("L", [160, 243])
def test_long_attention_forward_large_logits(L):
    """q and k scaled by 6: logits of standard deviation 36, the largest of each case's ~1-3 M scores near 180 - above the
    88.7 where fp32 exp overflows, so a kernel without the max subtraction returns inf / NaN here (asserted: it occurs)"""
    from pafuse_amd import ops
    qkv, heads, nseq, rows_of, kw = _case(L, 384, True, 7 + L, qk_gain=6.0)
    x = qkv[torch.cat(rows_of)].reshape(nseq, L, 3, heads, 48)
    logits = torch.einsum("slhd,sthd->shlt", x[:, :, 0], x[:, :, 1]) * 48 ** -0.5
    assert float(logits.max()) > 88.8 and bool(torch.isinf(logits.exp()).any())
    out = ops.attention(qkv.to(DEV), heads, nseq, L, **kw).cpu().double()
    assert bool(torch.isfinite(out).all())
    truth = _attention(qkv.double(), heads, rows_of)
    err, err_t = (out - truth).abs(), (_attention(qkv, heads, rows_of).double() - truth).abs()
    # near-one-hot rows: the error is that of the few V values the row picks, still fp32 rounding of O(1) numbers
    assert float(err.max()) <= max(2e-6, 2 * float(err_t.max())), (float(err.max()), float(err_t.max()))
    assert float(err.mean()) <= 1.5 * float(err_t.mean()) + 1e-9, (float(err.mean()), float(err_t.mean()))


def _backward(L, C, temporal, seed):
    from pafuse_amd import ops
    qkv, heads, nseq, rows_of, kw = _case(L, C, temporal, seed)
    d_o = torch.randn(qkv.shape[0], C, generator=torch.Generator().manual_seed(seed + 1))
    q64 = qkv.double().requires_grad_(True)
    _attention(q64, heads, rows_of).backward(d_o.double())
    q32 = qkv.clone().requires_grad_(True)
    _attention(q32, heads, rows_of).backward(d_o)
    got = ops.attention_backward(qkv.to(DEV), d_o.to(DEV), heads, nseq, L, **kw)
    return got, q64.grad, q32.grad.double(), (qkv, d_o, heads, nseq, kw)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("temporal", [False, True])
def test_long_attention_backward_vs_fp64(L, C, temporal):
    got, truth, torch32, _ = _backward(L, C, temporal, 100 * L + C + temporal)
    got = got.cpu().double()
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        e, et = (got[:, sl] - truth[:, sl]).abs(), (torch32[:, sl] - truth[:, sl]).abs()
        floor = 1e-7 * float(truth[:, sl].abs().max())
        print(f"attention backward L={L} C={C} {name}: max {float(e.max()):.2e} (torch {float(et.max()):.2e}) "
              f"mean {float(e.mean()):.2e} (torch {float(et.mean()):.2e})")
        assert float(e.max()) <= 2 * float(et.max()) + floor, (name, float(e.max()), float(et.max()))
        assert float(e.mean()) <= 1.5 * float(et.mean()) + floor, (name, float(e.mean()), float(et.mean()))


@pytest.mark.parametrize("L,C", [(99, 384), (100, 384), (109, 224), (110, 224), (100, 256)])
def test_attention_backward_hand_off_lengths_vs_fp64(L, C):
    """80 < L where the FMA kernel's two L x L planes still fit the LDS (L <= 99 at d = 48, L <= 109 at d = 28 / 32) and
    just past that, where the long kernel takes over: training reaches both for clips of 81 .. 109 frames since frames above
    80 are accepted; the same bounds as the long lengths"""
    test_long_attention_backward_vs_fp64(L, C, True)


def test_long_attention_backward_is_bit_reproducible():
    from pafuse_amd import ops
    got, _, _, (qkv, d_o, heads, nseq, kw) = _backward(243, 384, True, 5)
    again = ops.attention_backward(qkv.to(DEV), d_o.to(DEV), heads, nseq, 243, **kw)
    assert torch.equal(got, again)


def test_lengths_above_256_are_refused():
    from pafuse_amd import _lib, ops
    qkv, heads, nseq, _, kw = _case(257, 384, True, 3)
    with pytest.raises(_lib.PafuseError, match="need <=256"):
        ops.attention(qkv.to(DEV), heads, nseq, 257, **kw)
    with pytest.raises(_lib.PafuseError, match="up to 256 tokens"):
        ops.attention_backward(qkv.to(DEV), torch.zeros(qkv.shape[0], 384, device=DEV), heads, nseq, 257, **kw)


def test_f16x2_is_refused_for_clips_above_144_frames():
    import pafuse_amd
    from pafuse_amd import _lib
    m = pafuse_amd.MixSTE2(num_frame=243, num_joints=24, in_chans=5, embed_dim_ratio=384, depth=1, num_heads=8,
                           is_train=False)
    m = m.to(DEV).eval()
    m.operand_bf16 = 3
    x2d, x3d, t = torch.zeros(1, 243, 24, 2), torch.zeros(1, 1, 243, 24, 3), torch.tensor([5])
    with pytest.raises(_lib.PafuseError, match="use mode 2"):
        m(x2d.to(DEV), x3d.to(DEV), t.to(DEV))


# --------------------------------------------------------------------------------------------- the denoiser at F = 243
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("part", ["body", "face", "hands"])
def test_mixste2_forward_243_frames_vs_fp64(part, precision):
    import pafuse_amd
    F, J, C, depth = 243, len(gu.PART_JOINTS[part]), gu.PART_WIDTH[part], 2
    m = pafuse_amd.MixSTE2(num_frame=F, num_joints=J, in_chans=5, embed_dim_ratio=C, depth=depth, num_heads=8,
                           is_train=False)
    sd = {k: gu.seeded_tensor(k, v.shape, 243) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.operand_bf16 = {"f32": 0, "bf16x3": 2}[precision]
    g = torch.Generator().manual_seed(244)
    x2d = torch.rand(1, F, J, 2, generator=g) * 2 - 1
    x3d = torch.randn(1, 2, F, J, 3, generator=g).clamp(-1.1, 1.1)
    t = torch.tensor([499])
    hip = m(x2d.to(DEV), x3d.to(DEV), t.to(DEV)).cpu().double()
    sd64 = {k: v.double() for k, v in sd.items()}
    truth = orc.mixste2_eval(sd64, "", x2d.double(), x3d.double(), t, depth=depth)
    ref32 = orc.mixste2_eval(sd, "", x2d, x3d, t, depth=depth).double()
    e_hip, e_ref = (hip - truth).abs(), (ref32 - truth).abs()
    print(f"{part} {precision} F=243: hip mean {float(e_hip.mean()):.2e} max {float(e_hip.max()):.2e}; "
          f"oracle fp32 mean {float(e_ref.mean()):.2e} max {float(e_ref.max()):.2e}")
    assert float(e_hip.mean()) <= 1.5 * float(e_ref.mean()), (float(e_hip.mean()), float(e_ref.mean()))
    assert float(e_hip.max()) <= 2.0 * float(e_ref.max()), (float(e_hip.max()), float(e_ref.max()))


def _mpjpe_mm(poses, target):
    return 1000 * (poses - target).norm(dim=-1).mean(dim=(-1, -2))   # [.., hypotheses] per clip


@pytest.mark.parametrize("flip", [True, False])
def test_ddim_loop_243_frames_vs_oracle(flip):
    from __graft_entry__ import make_model
    P, T, F, depth = 2, 2, 243, 2
    model, sd = make_model(P, T, seed=243, flip=flip, depth=depth, frames=F)
    x2d, x2f = gu.synthetic_inputs_2d(B=1, frames=F)
    noises = gu.synthetic_noises(B=1, P=P, n=T, seed=9, frames=F)
    model.noise_fn = lambda k, shape, device: noises[k].to(device)
    out = model(x2d.to(DEV), None, input_2d_flip=x2f.to(DEV) if flip else None).cpu()
    ref = orc.ddim_sample(sd, x2d, noises, T, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                          inputs_2d_flip=x2f if flip else None, depth=depth)
    assert out.shape == ref.shape == (1, T, P, F, 134, 3)
    err = float((out - ref).abs().max())
    target = orc.center_pose_parts(gu.synthetic_target_3d(1, frames=F))[:, None, None]
    dm = float((_mpjpe_mm(out, target) - _mpjpe_mm(ref, target)).abs().max())
    print(f"DDIM F=243 flip={flip}: max |hip - oracle| {err:.2e} m, |dMPJPE| {dm:.2e} mm")
    assert err <= 1e-5, err
    assert dm <= 5e-4, dm


def test_g22_reference_loop_at_243_frames():
    """golden G22: the REFERENCE's own D3DP at 243-frame clips (tests/golden/make_golden_long.py: flip-TTA, P = 1, T = 2,
    depth 2, real widths), seeded weights and inputs pinned by SHA-256; pointwise 1e-5 m, the G5 bound"""
    from __graft_entry__ import make_model
    from tests.conftest import load_golden
    from tests.golden import g22_inputs as g22
    z = load_golden("g22_long_clips.npz")
    inp = g22.inputs()
    assert g22.digest(inp) == z["inputs_sha"].numpy().tobytes()
    model, sd = make_model(g22.P, g22.T, seed=g22.SEED, depth=g22.DEPTH, frames=g22.FRAMES)
    assert gu.sha256_of(sd) == z["sha"].numpy().tobytes()
    model.noise_fn = lambda k, shape, device: inp["noise_flip"][k].to(device)
    for precision in ("f32", "bf16x3"):
        model.precision = precision
        out = model(inp["x2d"].to(DEV), None, input_2d_flip=inp["x2d_flip"].to(DEV)).cpu()
        assert out.shape == z["flip_out"].shape == (1, g22.T, g22.P, 243, 134, 3)
        err = float((out - z["flip_out"]).abs().max())
        print(f"G22 {precision}: max |hip - reference| {err:.2e} m")
        assert err <= 1e-5, (precision, err)


def test_examples_run_at_243_frames(tmp_path):
    """examples/infer_in_the_wild.py and examples/evaluate_h3wb.py with model.number_of_frames=243 model.stride=243 on the
    synthetic H3WB files (fresh processes): the in-the-wild poses are [T, P, frames of the video, 134, 3], the evaluation log
    has finite protocol lines"""
    import os
    import re
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    over = ["model.number_of_frames=243", "model.stride=243", "ft2d.num_proposals=2", "ft2d.sampling_timesteps=2"]
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "infer_in_the_wild.py"), "--out", str(tmp_path)] + over,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    poses = np.load(tmp_path / "test_3d_output.npy")
    assert poses.shape == (2, 2, 70, 134, 3) and np.isfinite(poses).all()       # the synthetic video has 70 frames
    assert np.load(tmp_path / "test_3d_output_postprocess.npy").shape == poses.shape
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "evaluate_h3wb.py")] + over,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    mm = [float(v) for v in re.findall(r"Protocol #1 Error \(MPJPE\)[^:]*: ([-0-9.naninf]+) mm", r.stdout)]
    assert mm and all(np.isfinite(mm)), r.stdout[-2000:]


# --------------------------------------------------------------------------------------------- training at F = 243
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("part", ["body", "face", "hands"])
def test_train_step_243_frames_vs_oracle(part, precision, F=243):
    import pafuse_amd
    B, depth, rate = 2, 2, 0.3
    J, C = len(gu.PART_JOINTS[part]), gu.PART_WIDTH[part]
    m = pafuse_amd.MixSTE2(num_frame=F, num_joints=J, in_chans=5, embed_dim_ratio=C, depth=depth, num_heads=8,
                           drop_path_rate=rate, is_train=True)
    sd = {k: gu.seeded_tensor(k, v.shape, 245) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.operand_bf16 = {"f32": 0, "bf16x3": 2}[precision]
    g = torch.Generator().manual_seed(246)
    drops = []
    for r in orc.drop_path_rates(rate, depth):
        for nseq in (B * F, B * J):
            drops.append(tuple((torch.rand(nseq, generator=g) < 1 - r).float() / (1 - r) if r > 0 else None
                               for _ in range(2)))
    m.drop_fn = lambda block, branch, nseq, rate: drops[block][branch]
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, F, J, 3, generator=g)
    t = torch.tensor([999, 250])
    target = torch.randn(B, F, J, 3, generator=g)
    out = m(x2d.to(DEV), x3d.to(DEV), t.to(DEV))
    loss = orc.mpjpe(out, target.to(DEV))
    loss.backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = orc.mixste2_train(leaves, "", x2d, x3d, t, depth=depth, heads=8, drop=drops)
    assert torch.allclose(out.detach().cpu(), ref.detach(), rtol=0, atol=1e-5), (out.detach().cpu() - ref).abs().max()
    ref_loss = orc.mpjpe(ref, target)
    assert torch.allclose(loss.detach().cpu(), ref_loss.detach(), rtol=1e-5, atol=0), (float(loss), float(ref_loss))
    ref_loss.backward()
    for n, p in m.named_parameters():
        tol = 2e-4 * float(leaves[n].grad.abs().max()) + 1e-7
        e = float((p.grad.cpu() - leaves[n].grad).abs().max())
        assert e <= tol, (n, e, tol)


@pytest.mark.parametrize("part", ["body", "face"])
def test_train_step_100_frames_vs_oracle(part):
    """a 100-frame clip: the temporal attention backward is the long kernel for the body (d = 48: the FMA kernel's planes fit
    up to 99 tokens) and the FMA kernel for the face (d = 28: up to 109)"""
    test_train_step_243_frames_vs_oracle(part, "bf16x3", F=100)

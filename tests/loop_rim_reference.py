"""Plain-torch statements of the sampling loop's rim - the embed stage and the timestep embedding - parameterised by dtype
(float64: the ground truth; float32: the yardstick of what fp32 arithmetic costs), the oracle's own DDIM chain run on canned
denoiser outputs (the reference of the finalize stage: nothing of the update is restated here), and the case tables of
tests/test_hip_loop_rim.py.  tests/test_loop_rim_host.py proves the statements against the oracle on a machine without a GPU."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import d3dp_oracle as orc


def f32_scalar(v):
    """the fp32 number a Python scalar becomes beside an fp32 tensor, as a Python float"""
    return torch.tensor(v, dtype=torch.float32).item()


def embed_ref(x3d, x2d, pw, pb, pos, temb, nw, nb, eps=1e-6, joints=None, perm=None, x2d_flip=None, scale=None,
              dtype=torch.float64):
    """The embed stage of one part in `dtype`: x3d [B,P,F,J3,3], x2d / x2d_flip [B,F,J3,2], joints = the part's indices (None:
    all), perm with x2d_flip = the flipped half, scale = clamp at +-float(1.1 scale) and divide by float(scale) (None: neither).
    Returns dict(x, mean, rstd, xc, xn): rows [nflip,B,P,F,J,C] as the kernel orders them, mean / rstd [nflip,B,P,F,J]."""
    to = lambda t: t.to(dtype)      # noqa: E731
    B, P, Fr, J3, _ = x3d.shape
    idx = list(range(J3)) if joints is None else [int(j) for j in joints]
    x_t = to(x3d)
    if scale is not None:
        lim, div = f32_scalar(1.1 * scale), f32_scalar(scale)          # the fp64 product demoted, the scale demoted
        x_t = torch.clamp(x_t, min=-lim, max=lim) / div
    halves = [(x_t, to(x2d))]
    if x2d_flip is not None:
        x_f = x_t.clone()
        x_f[..., 0] *= -1
        halves.append((x_f[:, :, :, [int(j) for j in perm]], to(x2d_flip)))
    rows = []
    for x3, x2 in halves:
        x3, x2 = x3[..., idx, :], x2[..., idx, :]
        tok = torch.cat((x2[:, None].expand(B, P, Fr, len(idx), 2), x3), dim=-1).reshape(B * P * Fr, len(idx), 5)
        x = F.linear(tok, to(pw), to(pb)) + to(pos).reshape(1, len(idx), -1)
        x = x + to(temb)[:, None, None, None, :].expand(B, P, Fr, 1, temb.shape[-1]).reshape(B * P * Fr, 1, -1)
        rows.append(x.reshape(B, P, Fr, len(idx), -1))
    x = torch.stack(rows)
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + eps)
    xn = F.layer_norm(x, (x.shape[-1],), to(nw), to(nb), eps)
    return dict(x=x, mean=mean, rstd=rstd, xc=x - mean[..., None], xn=xn)


def time_embed_ref(t, freqs, w1, b1, w3, b3, dtype=torch.float64):
    """sinusoid -> Linear(C,2C) -> GELU(erf) -> Linear(2C,C) in `dtype`.  The ARGUMENT of sin / cos is the fp32 product
    float(t) freqs[i] in every dtype: that number is the kernel's and the reference's input (at 999 rad an fp64 product would
    move the sine by up to 3e-5, which is nobody's rounding error)."""
    arg = (t[:, None] * freqs[None, :].float()).to(dtype)
    emb = torch.cat((arg.sin(), arg.cos()), dim=-1)
    hid = F.gelu(F.linear(emb, w1.to(dtype), b1.to(dtype)))
    return F.linear(hid, w3.to(dtype), b3.to(dtype))


@contextlib.contextmanager
def canned_denoiser(outputs):
    """For the duration of the block oracle.predict_parts returns clones of `outputs` in call order (per step: the plain call,
    then - flip sampler - the call on the flipped input) and the tensor entering every epsilon is recorded: the block's value is
    that list, imgs[k] = the img step k starts from.  Both originals are restored.

    oracle._eps_from_x0 is wrapped - it calls the original, so no arithmetic changes - only because ddim_sample returns x0 and not
    img: the epsilon of a step is the one place both samplers hand the current img to.  The wrapper is found through the oracle's
    module global; were the oracle to reach that helper another way, oracle_chain's `len(imgs) == T` fails at once, and
    tests/test_loop_rim_host.py pins the recorded tensors to the sampler's update line."""
    queue, imgs = list(outputs), []
    keep_predict, keep_eps = orc.predict_parts, orc._eps_from_x0

    def predict(sd, inputs_2d, x_t, t, *a, **kw):
        return queue.pop(0).clone()

    def eps(sd, x, t, x0):
        imgs.append(x.clone())
        return keep_eps(sd, x, t, x0)

    orc.predict_parts, orc._eps_from_x0 = predict, eps
    try:
        yield imgs
    finally:
        orc.predict_parts, orc._eps_from_x0 = keep_predict, keep_eps


def oracle_chain(sd, preds, noises, T, scale, joints_left=None, joints_right=None):
    """oracle.ddim_sample over all T steps on canned denoiser outputs.  preds[k] = the plain output of step k [B,P,F,J,3] or,
    with joints_left / joints_right (the flip sampler), the pair (plain, output on the flipped input).  Returns
    (x0 [B,T,P,F,J,3], [img after step k for k < T]) - the reference's own lines for un-flip, TTA mean, scale, clamp, fp64
    epsilon and both update forms."""
    flip = joints_left is not None
    B, _, _, J, _ = noises[0].shape
    flat = [t for p in preds for t in (p if flip else (p,))]
    x2d = torch.zeros(B, noises[0].shape[2], J, 2)
    with canned_denoiser(flat) as imgs:
        x0 = orc.ddim_sample(sd, x2d, noises, T, joints_left, joints_right, inputs_2d_flip=x2d if flip else None, scale=scale)
        assert len(imgs) == T and torch.equal(imgs[0], noises[0])
    return x0, imgs[1:] + [x0[:, T - 1]]


# ---------------------------------------------------------------------------------------------------------- case tables
EMBED_WIDTHS = (4, 64, 128, 132, 224, 256, 288, 384)     # 1, 16, 32, 33, 56, 64, 72, 96 channel quads over the 32 lanes of a token
IMAGE_WIDTHS = (64, 224, 256, 288, 384)                  # all multiples of 32: an H image (C % 8) and an X image (C % 32) exist
# (B, P, F, J3, joints of the part or None, (left, right) of the flip): small with no two of B, P, F, J equal - the whole
# skeleton, then a part gathered out of order - and the three real parts at F = 2 with the project's joint lists and flip lists
EMBED_DIMS = [(2, 3, 4, 5, None, ([1, 3], [2, 4])), (1, 2, 3, 7, (5, 0, 3, 6, 2), ([1, 3, 5], [2, 4, 6]))] + \
             [(1, 2, 2, orc.NUM_KPS, tuple(orc.PART_JOINTS[p]), (orc.SYN_JOINTS_LEFT, orc.SYN_JOINTS_RIGHT)) for p in orc.PART_ORDER]
EMBED_SCALES = (1.0, 0.3)


def embed_quads(C):
    """how the C / 4 channel quads of a token fill the three rounds of 32 lanes: per round 'empty', 'part' or 'full'"""
    nq = C // 4
    return tuple("empty" if nq <= 32 * i else ("full" if nq >= 32 * (i + 1) else "part") for i in range(3))


# (precision, folded, h_residual_only) of every output form the loop can ask for, all five product modes; plain = the first
# ('bf16' changes the GEMMs' operands only: its embed launch must be the plain one, number for number)
EMBED_FORMS = [("f32", False, False), ("bf16", False, False), ("bf16x3", False, False), ("bf16x3", True, False),
               ("f16x2", False, False), ("f16x2", True, False), ("f16x2", True, True),
               ("bf16x3_images", False, False), ("bf16x3_images", True, False), ("bf16x3_images", True, True)]

# one token matrix of 1 * 3 * 5 * 3 = 45 rows (= 5 mod 8: six workgroups, the last with three live tokens) and its windows
# (row0, nrows); the last three are the lanes of the loop's split of the R = 3 hypothesis passes over three streams, 15 rows each
WINDOW_DIMS = (1, 3, 5, 5, (4, 0, 2), None)              # as EMBED_DIMS; no flipped half (its row count would be even)
WINDOW_ROWS = 45
WINDOWS = [(0, 45), (0, 1), (1, 1), (3, 8), (7, 11), (42, 3), (0, 15), (15, 15), (30, 15)]
WINDOW_FORMS = [("f32", False, False), ("bf16x3", True, False), ("f16x2", True, True)]      # plain, folded, a folded image form

TIME_WIDTHS = (64, 224, 256, 288, 384)
TIME_STEPS = (0, 1, 2, 250, 499, 998, 999)

# finalize: (B, P, F, parts as joint lists, flip lists or None) - the project's three parts, and one part of five joints whose
# element count B P F J = 60 is no multiple of the 256 threads of a workgroup (nor is 2 * 3 * 2 * 134 = 1608)
FINALIZE_T = 4
FINALIZE_CASES = {
    "parts134": dict(B=2, P=3, F=2, parts=[list(v) for v in orc.PART_JOINTS.values()], left=orc.SYN_JOINTS_LEFT,
                     right=orc.SYN_JOINTS_RIGHT),
    "one_part5": dict(B=2, P=3, F=2, parts=[[0, 1, 2, 3, 4]], left=[1, 3], right=[2, 4]),
}
FINALIZE_SCALES = (1.0, 0.3)

"""The inference forward at row counts no tile divides, against an fp64 evaluation of the same function.

The training step has an odd-shape sweep (tests/test_hip_train.py); the inference path through the same arenas was compared with
fp64 only at the three real parts, where B P F J is a multiple of 4 or more.  Here M = B P F J is 2, 105, 459, 150, 648, 1836 and
1134, in each of the four product modes.

Which mode runs: images.effective_mode hands 'bf16x3_images' to the 'bf16x3' kernels where the image pipeline has none (then the
bits are those of the 'bf16x3' run, asserted); a (shape, mode) pair pafuse_mode_supported has no kernels for after that is
refused loudly by design, and the refusal is what the test asserts for it: 'f16x2' at the widths 64 and 128 (the image
pipelines serve 224 / 256 / 384), and EVERY mode at (F, J, C, heads) = (3, 5, 96, 3) - width 96 has no kernel in this library
(width_supported: 384, 288, 256, 224, 128, 64), so the M = 150 case contributes a refusal and no numbers.

Bounds (those of test_accuracy_equivalent_to_reference_fp32, pooled per mode over the shapes that ran, because on 6 .. 300 output
values a ratio of two means is noise): mean |hip - fp64| <= 1.5 x mean |oracle32 - fp64|, max <= 2.0 x the oracle's max; per case
max |hip - oracle32| <= 1e-5, the loop tests' pointwise bound.  The same runs under GuardedArenas("ones") give the same bits."""
import functools

import pytest
import torch

from oracle import d3dp_oracle as orc
from pafuse_amd import _lib
from pafuse_amd._lib import PRECISIONS
from tests.golden import golden_util as gu
from tests.test_hip_partials import same_bits
from tests.test_hip_workspaces import MODES, ran_mode
from tests.workspace_policy import GuardedArenas

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (F, J, C, heads, depth, B, P)
SHAPES = [(2, 1, 64, 8, 1, 1, 1), (5, 7, 128, 8, 1, 1, 3), (9, 17, 64, 8, 2, 3, 1), (3, 5, 96, 3, 1, 2, 5), (27, 24, 384, 8, 1, 1, 1),
          (27, 68, 224, 8, 1, 1, 1), (27, 42, 256, 8, 1, 1, 1)]
ROWS = [2, 105, 459, 150, 648, 1836, 1134]
MEAN_FACTOR, MAX_FACTOR, POINTWISE = 1.5, 2.0, 1e-5


@functools.lru_cache(maxsize=None)
def case(shape):
    """the model, its inputs and the two oracle runs (fp64, and the reference's fp32 arithmetic) of one shape, computed once;
    then per mode ("ran", mode, output) or ("refused", mode, None)"""
    import pafuse_amd
    F, J, Cw, heads, depth, B, P = shape
    m = pafuse_amd.MixSTE2(num_frame=F, num_joints=J, in_chans=5, embed_dim_ratio=Cw, depth=depth, num_heads=heads,
                           drop_path_rate=0.0, is_train=False)
    sd = {k: gu.seeded_tensor(k, v.shape, 95) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(96 + F * J)
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, P, F, J, 3, generator=g).clamp(-1.1, 1.1)
    t = torch.randint(0, 1000, (B,), generator=g)
    truth = orc.mixste2_eval({k: v.double() for k, v in sd.items()}, "", x2d.double(), x3d.double(), t, depth=depth, heads=heads)
    ref32 = orc.mixste2_eval(sd, "", x2d, x3d, t, depth=depth, heads=heads)
    dev = tuple(v.to(DEV) for v in (x2d, x3d, t))
    runs = {}
    for precision in MODES:
        m.operand_bf16 = PRECISIONS[precision]
        mode, ok = ran_mode(precision, Cw, heads, J, F)
        if not ok:
            with pytest.raises(_lib.PafuseError):
                m(*dev)
            runs[precision] = ("refused", mode, None)
            continue
        out = m(*dev)
        arenas = GuardedArenas("ones")
        with _lib.workspace_policy(arenas):
            dirty = m(*dev)
        arenas.check()
        assert arenas.names() == ["mixste2_forward"] and same_bits(dirty, out), (shape, precision)
        runs[precision] = ("ran", mode, out.cpu())
    return {"truth": truth, "ref32": ref32, "runs": runs}


def test_row_counts():
    assert [B * P * F * J for F, J, _, _, _, B, P in SHAPES] == ROWS


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_ragged_forward_pointwise_and_which_mode_ran(shape):
    F, J, Cw, heads, depth, B, P = shape
    c = case(shape)
    runs = c["runs"]
    has_kernels, images = Cw in (384, 288, 256, 224, 128, 64), Cw in (384, 256, 224)
    want = {"f32": ("ran" if has_kernels else "refused", 0), "bf16x3": ("ran" if has_kernels else "refused", 2),
            "f16x2": ("ran" if images else "refused", 3)}
    for precision, (what, mode) in want.items():
        assert runs[precision][:2] == (what, mode), (shape, precision, runs[precision][:2])
    what, mode, out = runs["bf16x3_images"]
    assert what == ("ran" if has_kernels else "refused") and mode in ((4, 2) if images else (2,)), (shape, what, mode)
    if what == "ran" and mode == 2:          # the fall-back runs the 'bf16x3' kernels: their bits
        assert same_bits(out, runs["bf16x3"][2]), shape
    for precision in MODES:
        what, mode, out = runs[precision]
        if what != "ran":
            continue
        assert out.shape == c["ref32"].shape and bool(torch.isfinite(out).all()), (shape, precision)
        d = float((out - c["ref32"]).abs().max())
        print(f"{shape} {precision} (mode {mode}): max |hip - oracle32| = {d:.3e}")
        assert d <= POINTWISE, (shape, precision, d)


@pytest.mark.parametrize("precision", MODES)
def test_ragged_forward_pooled_against_fp64(precision):
    from tests.test_hip_parity import PARITY_LINES
    n = 0
    hip_sum = ref_sum = hip_max = ref_max = 0.0
    ran = []
    for shape in SHAPES:
        c = case(shape)
        what, mode, out = c["runs"][precision]
        if what != "ran":
            continue
        e_hip, e_ref = (out.double() - c["truth"]).abs(), (c["ref32"].double() - c["truth"]).abs()
        n += e_hip.numel()
        hip_sum, ref_sum = hip_sum + float(e_hip.sum()), ref_sum + float(e_ref.sum())
        hip_max, ref_max = max(hip_max, float(e_hip.max())), max(ref_max, float(e_ref.max()))
        ran.append((shape[0] * shape[1] * shape[5] * shape[6], mode))
    assert len(ran) >= 3, (precision, ran)      # the three part widths run in every mode
    line = (f"ragged forward {precision}: {len(ran)} shapes (M, mode) {ran}, {n} values; |hip - fp64| mean {hip_sum / n:.3e} max {hip_max:.3e} / "
            f"|oracle32 - fp64| mean {ref_sum / n:.3e} max {ref_max:.3e} (bounds {MEAN_FACTOR} x, {MAX_FACTOR} x)")
    print(line)
    PARITY_LINES.append(line)
    assert hip_sum / n <= MEAN_FACTOR * ref_sum / n, line
    assert hip_max <= MAX_FACTOR * ref_max, line

"""The two public surfaces make the same weight images: the module (MixSTE2.weights_struct, its dict kept in
_wcache_by_device) and the schema'd ops (torch_ops.mixste_struct, its dict in the keep-alive) both consume the one plan of
pafuse_amd/images.py.  Per precision: the same keys, every image and vector torch.equal (the device split is deterministic
and both are made from the same tensors by the same builders), the same null / non-null pattern over every
pafuse_block_weights field, the same mode handed to the library.

Shapes: frames 3, joints 5, depth 1, heads 8 - width 256 (d = 32, hidden 512: every image mode has kernels and the fused MLP is
on by default) and width 288 (d = 36: 'bf16x3_images' has no kernels, both surfaces fall back to 'bf16x3')."""
import pytest
import torch

from pafuse_amd import _lib, torch_ops
from pafuse_amd._lib import MODE_BF16X3, PRECISIONS
from pafuse_amd.mixste2 import MixSTE2

pytestmark = pytest.mark.gpu
DEV = "cuda"
_models = {}


def model(channels):
    if channels not in _models:
        torch.manual_seed(17)
        _models[channels] = MixSTE2(num_frame=3, num_joints=5, embed_dim_ratio=channels, depth=1, num_heads=8,
                                    is_train=False).to(DEV).eval()
    return _models[channels]


def both(channels, precision):
    """(struct, image dict) of the module and of the ops for the same parameters."""
    m = model(channels)
    m.operand_bf16 = PRECISIONS[precision]
    w_mod = m.weights_struct()
    made = m._wcache_by_device[m._freqs.device.index][2]
    w_ops, keep = torch_ops.mixste_struct(list(m.parameters()), 3, 5, 1, 8, precision)
    torch.cuda.synchronize()
    present = lambda d: {k: v for k, v in (d or {}).items() if v is not None}      # noqa: E731
    return (w_mod, present(made)), (w_ops, present(keep[2]))


def null_pattern(w):
    return [(part, field, getattr(blocks[0], field) is None) for part, blocks in (("ste", w.ste), ("tte", w.tte))
            for field in _lib.BlockWeights._names]


def check_same(mod, ops):
    (w_mod, i_mod), (w_ops, i_ops) = mod, ops
    assert sorted(i_mod) == sorted(i_ops)
    for key in i_mod:
        assert torch.equal(i_mod[key], i_ops[key]), key
    assert null_pattern(w_mod) == null_pattern(w_ops)
    assert w_mod.operand_bf16 == w_ops.operand_bf16
    for w in (w_mod, w_ops):
        assert all(null for _, field, null in null_pattern(w) if field in ("qkv_ls", "fc1_ls", "qkv_hl"))


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_module_and_ops_make_the_same_images(precision):
    mod, ops = both(256, precision)
    check_same(mod, ops)
    assert mod[0].operand_bf16 == PRECISIONS[precision]
    assert bool(mod[1]) == (PRECISIONS[precision] >= MODE_BF16X3)
    if precision == "f16x2":
        assert "STEblocks.0.mlp.fc2.hp" in mod[1] and "TTEblocks.0.attn.qkv.hs" in mod[1]
    if precision == "bf16x3_images":
        assert "STEblocks.0.attn.qkv.weight" not in mod[1] and "STEblocks.0.attn.qkv.hb" in mod[1] and mod[0].ste[0].qkv_ws is None


def test_both_surfaces_fall_back_to_bf16x3_where_the_image_pipeline_has_no_kernels():
    mod, ops = both(288, "bf16x3_images")
    check_same(mod, ops)
    assert mod[0].operand_bf16 == ops[0].operand_bf16 == MODE_BF16X3
    images = {k: v.clone() for k, v in mod[1].items()}
    plain, plain_ops = both(288, "bf16x3")
    check_same(plain, plain_ops)
    assert sorted(images) == sorted(plain[1]) and all(torch.equal(images[k], plain[1][k]) for k in images)
    assert null_pattern(mod[0]) == null_pattern(plain[0])

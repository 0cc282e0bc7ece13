"""pafuse_amd/images.py on the host: which weight images a mode needs (resolve_options, plan_images), the fallback of
'bf16x3_images' (effective_mode) and the image cache (cached).  No GPU and no library: the planner and the resolver are pure, and
make_images runs here with split_image replaced by a stand-in.

The per-block tables below are written out from the two loops this module replaced (MixSTE2._split_images for the modules,
torch_ops.mixste_struct for the schema'd ops), not from the planner."""
import pytest
import torch

from pafuse_amd import images
from pafuse_amd._lib import MODE_BF16, MODE_BF16X3, MODE_BF16X3_IMAGES, MODE_F16X2, MODE_F32
from pafuse_amd.mixste2 import MixSTE2

PREFIXES = ("STEblocks.0.", "TTEblocks.0.")
QKV, PROJ, FC1, FC2 = "attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"
FOLDED = [(QKV, "folded", 2), (PROJ, "plain", 1), (FC1, "folded", 2), (FC2, "plain", 1)]
UNFOLDED = [(QKV, "plain", 2), (PROJ, "plain", 1), (FC1, "plain", 2), (FC2, "plain", 1)]
HEAD_MAJOR = ("attn.qkv.hs", "head-major-folded", 2)
FUSED_MLP = ("mlp.fc2.hp", "fused-mlp", 1)
# dict keys per kind: a folded layer also gets its vector lt, the head-major image its bias hb
KEYS = {"plain": lambda stem: (stem + "weight",), "folded": lambda stem: (stem + "weight", stem + "lt"),
        "folded-vector": lambda stem: (stem + "lt",), "head-major": lambda stem: (stem + "hs", stem + "hb"),
        "head-major-folded": lambda stem: (stem + "hs", stem + "hb"), "fused-mlp": lambda stem: (stem + "hp",)}


def _names(channels=256, mlp_ratio=2.):
    with torch.device("meta"):
        m = MixSTE2(num_frame=3, num_joints=5, embed_dim_ratio=channels, depth=1, num_heads=8, mlp_ratio=mlp_ratio, is_train=False)
    return tuple(n for n, _ in m.named_parameters())


def _plan(mode, channels=256, hidden=None, **options):
    hidden = 2 * channels if hidden is None else hidden
    return images.plan_images(_names(channels, hidden / channels), mode, images.resolve_options(mode, channels, hidden, **options))


def _whole(table):
    return [(prefix + key, kind, layout) for prefix in PREFIXES for key, kind, layout in table]


@pytest.mark.parametrize("mode", [MODE_F32, MODE_BF16])
def test_unsplit_modes_need_no_images(mode):
    assert _plan(mode) == [] and _plan(mode, fuse_qkv_attention=True, fuse_mlp=True) == []


def test_bf16x3_plans():
    assert _plan(MODE_BF16X3) == _whole(FOLDED)                                     # no hs, hb or hp
    assert _plan(MODE_BF16X3, fold_layernorm=False) == _whole(UNFOLDED)             # no lt either
    assert _plan(MODE_BF16X3, fuse_qkv_attention=True) == _whole([FOLDED[0], HEAD_MAJOR] + FOLDED[1:])
    assert _plan(MODE_BF16X3, fuse_mlp=True) == _whole(FOLDED)                      # the fused MLP is an f16x2 kernel


def test_f16x2_plans():
    with_hs = [FOLDED[0], HEAD_MAJOR] + FOLDED[1:]
    assert _plan(MODE_F16X2, 256) == _whole(with_hs + [FUSED_MLP])
    assert _plan(MODE_F16X2, 224) == _whole(with_hs + [FUSED_MLP])
    assert _plan(MODE_F16X2, 384) == _whole(with_hs)                                # built, but not a default width
    assert _plan(MODE_F16X2, 384, fuse_mlp=True) == _whole(with_hs + [FUSED_MLP])
    assert _plan(MODE_F16X2, 288, fuse_mlp=True) == _whole(with_hs)                 # no kernel at this width
    assert _plan(MODE_F16X2, 256, fuse_mlp=False) == _whole(with_hs)
    assert _plan(MODE_F16X2, 256, fuse_qkv_attention=False) == _whole(FOLDED + [FUSED_MLP])
    for channels in (224, 256, 384):
        assert _plan(MODE_F16X2, channels, fuse_mlp=True, keep_f32_residual=True) == _whole(with_hs)
        assert _plan(MODE_F16X2, channels, hidden=channels, fuse_mlp=True) == _whole(with_hs)        # hidden != 2 C
    # without the fold the fused kernels' inputs do not exist in their form: head-major unfolded, no fused MLP
    assert _plan(MODE_F16X2, 256, fold_layernorm=False) == _whole([UNFOLDED[0], ("attn.qkv.hs", "head-major", 2)] + UNFOLDED[1:])


def test_bf16x3_images_plans():
    table = [("attn.qkv.lt", "folded-vector", None), HEAD_MAJOR] + FOLDED[1:]       # no plain attn.qkv.weight image
    for channels in (224, 256, 384):
        assert _plan(MODE_BF16X3_IMAGES, channels) == _whole(table)
        assert _plan(MODE_BF16X3_IMAGES, channels, fuse_mlp=True) == _whole(table)  # never hp
    assert _plan(MODE_BF16X3_IMAGES, fuse_qkv_attention=False) == _whole(table)     # its only form
    assert _plan(MODE_BF16X3_IMAGES, fold_layernorm=False) == _whole([("attn.qkv.hs", "head-major", 2)] + UNFOLDED[1:])


def test_block_plan_is_unfolded_and_fused_only_on_the_image_pipeline():
    names = [key for _, key in images.BLOCK_PARAMS]
    for mode in (MODE_BF16X3, MODE_F16X2):
        assert images.plan_images(names, mode, (False, False, False)) == UNFOLDED
    assert images.plan_images(names, MODE_BF16X3_IMAGES, (False, True, False)) == [("attn.qkv.hs", "head-major", 2)] + UNFOLDED[1:]


def test_default_options_are_the_conditions_the_ops_spelled_out():
    """torch_ops.mixste_struct hard-coded: LayerNorm folded in every split mode, qkv + attention fused in 'f16x2' and
    'bf16x3_images', the fused MLP in 'f16x2' at widths 224 and 256 with hidden = 2 C."""
    for mode in (MODE_F32, MODE_BF16, MODE_BF16X3, MODE_F16X2, MODE_BF16X3_IMAGES):
        for channels in (32, 224, 256, 288, 384):
            for hidden in (channels, 2 * channels):
                want = (mode >= 2, mode >= 3, mode == 3 and channels in (224, 256) and hidden == 2 * channels)
                assert images.resolve_options(mode, channels, hidden) == want, (mode, channels, hidden)
    assert (MODE_BF16X3, MODE_F16X2, MODE_BF16X3_IMAGES) == (2, 3, 4)


def test_effective_mode_falls_back_by_name():
    calls = []

    def supported(answer):
        def query(*args):
            calls.append(args)
            return answer
        return query
    shape = (288, 576, 8, 5, 3)
    assert images.effective_mode(MODE_BF16X3_IMAGES, *shape, supported=supported(1)) == MODE_BF16X3_IMAGES
    assert images.effective_mode(MODE_BF16X3_IMAGES, *shape, supported=supported(0)) == MODE_BF16X3
    assert calls == [(MODE_BF16X3_IMAGES,) + shape] * 2           # (mode, channels, hidden, heads, joints, frames), as given
    assert images.effective_mode(MODE_BF16X3_IMAGES, *shape, training=True, supported=supported(1)) == MODE_BF16X3
    for mode in (MODE_F32, MODE_BF16, MODE_BF16X3, MODE_F16X2):
        for training in (False, True):
            assert images.effective_mode(mode, *shape, training=training, supported=supported(0)) == mode
    assert len(calls) == 2                                        # only the image pipeline's inference shapes are asked about


@pytest.mark.parametrize("mode,options", [(MODE_BF16X3, {}), (MODE_BF16X3, {"fold_layernorm": False}), (MODE_F16X2, {}),
                                          (MODE_BF16X3_IMAGES, {})])
def test_make_images_fills_the_planned_keys(mode, options, monkeypatch):
    """make_images with a stand-in for the device split: the dict has exactly the keys the plan names (nothing None), the
    folded vector is W beta + b in fp64 and the folded image is made from W (.) g."""
    torch.manual_seed(5)
    m = MixSTE2(num_frame=3, num_joints=5, embed_dim_ratio=256, depth=1, num_heads=8, is_train=False)
    for p in m.parameters():
        p.data.normal_()
    get = dict(m.named_parameters()).__getitem__
    seen = []

    def split(weight, layout, mode_=MODE_BF16X3):
        seen.append((weight, layout, mode_))
        return torch.zeros(1, dtype=torch.uint8)
    monkeypatch.setattr(images, "split_image", split)
    plan = _plan(mode, **options)
    made = images.make_images(plan, get, mode, 8)
    want = [k for key, kind, _ in plan for k in KEYS[kind](key[:key.rindex(".") + 1])]
    assert sorted(made) == sorted(want) and len(set(want)) == len(want) and all(v is not None for v in made.values())
    assert len(seen) == sum(kind != "folded-vector" for _, kind, _ in plan) and all(mode_ == mode for _, _, mode_ in seen)
    if options.get("fold_layernorm", True):
        W, g, beta, b = (get("STEblocks.0." + k).detach() for k in ("mlp.fc1.weight", "norm2.weight", "norm2.bias", "mlp.fc1.bias"))
        assert torch.equal(made["STEblocks.0.mlp.fc1.lt"], (W.double() @ beta.double() + b.double()).float())
        assert any(torch.equal(w, (W * g[None, :]).contiguous()) and layout == 2 for w, layout, _ in seen)


def test_cache_hits_misses_evicts_and_pins(monkeypatch):
    monkeypatch.setattr(images, "_image_cache", {})
    monkeypatch.setattr(images, "_IMAGE_CACHE_MAX", 4)
    built = []

    def build():
        built.append(len(built))
        return built[-1]
    w, v = torch.ones(4, 4), torch.ones(4)
    assert images.cached(("a", 1), (w, v), build) == 0 and images.cached(("a", 1), (w, v), build) == 0      # a hit on the same tensors
    v.mul_(2.0)                                                                                               # version bump of one source
    assert images.cached(("a", 1), (w, v), build) == 1
    assert images.cached(("a", 2), (w, v), build) == 2 and images.cached(("b", 1), (w, v), build) == 3       # another key_head
    assert images.cached(("a", 1), (w, v.view(2, 2)), build) == 4                                            # same storage, another shape
    assert len(images._image_cache) == 4 and built == [0, 1, 2, 3, 4]                                         # the oldest entry went
    assert images.cached(("a", 1), (w, v), build) == 1                                                        # ... and only that one
    for i in range(10):
        images.cached(("fill", i), (w,), build)
    assert len(images._image_cache) == 4
    t = torch.zeros(3)
    images.cached(("pin",), (t,), build)
    (_, sources), = [e for k, e in images._image_cache.items() if k[0] == "pin"]
    assert sources[0] is t                                                                                    # the entry holds its sources

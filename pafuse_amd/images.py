"""Weight images of the split-precision modes: which images a model or a block needs (resolve_options, plan_images), how each
is built (split_image, folded_linear, head_major_qkv, fused_mlp_fc2_image), where they go in a pafuse_block_weights
(fill_block_struct) and the cache the schema'd ops keep them in (cached).  The modules (mixste2.py), the tensor-level wrappers
(ops.py) and the torch ops (torch_ops.py) all consume the one plan, so both public surfaces hand the library the same bits."""
import torch

from . import _lib
from ._lib import MODE_BF16X3, MODE_BF16X3_IMAGES, MODE_F16X2, SPLIT_FLAG

SPLIT_SUFFIXES = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
# pafuse_split_weights' layout per linear layer: 1 the whole-row layers, 2 the 16x16x32-MFMA kernels of qkv and fc1
LAYOUT_OF = {"attn.qkv.weight": 2, "attn.proj.weight": 1, "mlp.fc1.weight": 2, "mlp.fc2.weight": 1}
# the LayerNorm folded into a linear layer: linear weight suffix -> the norm of the same block in front of it
FOLDED_LINEAR = {"attn.qkv.weight": "norm1", "mlp.fc1.weight": "norm2"}
FOLD_SUFFIXES = ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.qkv.bias", "mlp.fc1.bias")
FUSED_MLP_WIDTHS = (224, 256, 384)     # channel widths hmlp_kernel is built for (csrc/pafuse_hip.hip fused_mlp)
FUSED_MLP_DEFAULT_WIDTHS = (224, 256)  # ... and where MixSTE2.fuse_mlp = None turns it on
# pafuse_block_weights: field -> state-dict key inside a block, and field -> key of the image dict (the fields qkv_ls, fc1_ls
# and qkv_hl are read by no kernel and stay null)
BLOCK_PARAMS = (("norm1_w", "norm1.weight"), ("norm1_b", "norm1.bias"), ("qkv_w", "attn.qkv.weight"),
                ("qkv_b", "attn.qkv.bias"), ("proj_w", "attn.proj.weight"), ("proj_b", "attn.proj.bias"),
                ("norm2_w", "norm2.weight"), ("norm2_b", "norm2.bias"), ("fc1_w", "mlp.fc1.weight"),
                ("fc1_b", "mlp.fc1.bias"), ("fc2_w", "mlp.fc2.weight"), ("fc2_b", "mlp.fc2.bias"))
BLOCK_IMAGES = (("qkv_ws", "attn.qkv.weight"), ("proj_ws", "attn.proj.weight"), ("fc1_ws", "mlp.fc1.weight"),
                ("fc2_ws", "mlp.fc2.weight"), ("qkv_lt", "attn.qkv.lt"), ("fc1_lt", "mlp.fc1.lt"),
                ("qkv_hs", "attn.qkv.hs"), ("qkv_hb", "attn.qkv.hb"), ("fc2_hp", "mlp.fc2.hp"))


def _ptr(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise _lib.PafuseError(f"{what}: expected a contiguous fp32 tensor on the HIP device, got "
                               f"{t.dtype} contiguous={t.is_contiguous()} device={t.device}")
    return t.data_ptr()


def effective_mode(mode, channels, hidden, heads, joints, frames, training=False, supported=None):
    """The matrix-product mode the library is handed: the requested one, except that 'bf16x3_images' falls back to the same
    products on the 'bf16x3' kernels where the image pipeline has none - training and shapes outside its set
    (`supported`: pafuse_mode_supported unless a test passes a stub)."""
    if mode == MODE_BF16X3_IMAGES and (training or not (supported or _lib.load().pafuse_mode_supported)(
            mode, channels, hidden, heads, joints, frames)):
        return MODE_BF16X3
    return mode


def resolve_options(mode, channels, hidden, fold_layernorm=None, fuse_qkv_attention=None, fuse_mlp=None, keep_f32_residual=False):
    """(fold, fuse, fuse_mlp) of a model in `mode` from MixSTE2's options of the same names; None = the modules' defaults.
    fold: LayerNorm folded into qkv / fc1 (on in every split mode); fuse: qkv + attention in one kernel ('bf16x3_images' has
    no other form; on in 'f16x2', off in 'bf16x3'); fuse_mlp: fc1 -> GELU -> fc2 in one kernel ('f16x2', folded, image-only
    residual, mlp_ratio 2; on at FUSED_MLP_DEFAULT_WIDTHS, with True wherever the kernel exists)."""
    split = mode >= MODE_BF16X3
    fold = split and (True if fold_layernorm is None else bool(fold_layernorm))
    fuse = split and (mode == MODE_BF16X3_IMAGES or (mode == MODE_F16X2 if fuse_qkv_attention is None else bool(fuse_qkv_attention)))
    mlp = (mode == MODE_F16X2 and fold and not keep_f32_residual and hidden == 2 * channels and channels in FUSED_MLP_WIDTHS
           and (channels in FUSED_MLP_DEFAULT_WIDTHS if fuse_mlp is None else bool(fuse_mlp)))
    return fold, fuse, mlp


def image_layout(name):
    """pafuse_split_weights' layout argument for a state-dict key of a linear weight (include/pafuse_hip.h)."""
    return next(layout for suffix, layout in LAYOUT_OF.items() if name.endswith(suffix))


def plan_images(names, mode, options):
    """What to make for the parameters `names` in `mode` under options = (fold, fuse, fuse_mlp) of resolve_options: the ordered
    list of (key of the image dict, kind, layout).  Kinds: 'plain' the image of the weight; 'folded' the image of W (.) g under
    the weight's own key and the vector <stem>lt; 'folded-vector' that vector alone ('bf16x3_images' multiplies the head-major qkv
    image only: no plain qkv image); 'head-major' / 'head-major-folded' <stem>hs and the vector <stem>hb; 'fused-mlp'
    <stem>hp.  No tensors, no device."""
    fold, fuse, fuse_mlp = options
    plan = []
    for name in names if mode >= MODE_BF16X3 else ():
        if not name.endswith(SPLIT_SUFFIXES):
            continue
        stem, layout, qkv = name[:-len("weight")], image_layout(name), name.endswith("attn.qkv.weight")
        plain = not (mode == MODE_BF16X3_IMAGES and qkv)
        if fold and name.endswith(tuple(FOLDED_LINEAR)):
            plan.append((name, "folded", layout) if plain else (stem + "lt", "folded-vector", None))
        elif plain:
            plan.append((name, "plain", layout))
        if fuse and qkv:
            plan.append((stem + "hs", "head-major-folded" if fold else "head-major", 2))
        if fuse_mlp and name.endswith("mlp.fc2.weight"):
            plan.append((stem + "hp", "fused-mlp", layout))
    return plan


def make_images(plan, get, mode, heads, cache=None):
    """The image dict of a plan (plan_images) from ``get(state-dict key) -> tensor``.  `cache`: `cached` to make every entry
    once per version of its sources (the schema'd ops), None to build afresh (the modules keep their dict per module)."""
    make = cache or (lambda key_head, sources, build: build())
    images = {}
    for key, kind, layout in plan:
        stem = key[:key.rindex(".") + 1]
        name = stem + "weight"
        if kind == "plain":
            images[key] = make(("plain", mode, layout), (get(name),), lambda: split_image(get(name), layout, mode))
        elif kind in ("folded", "folded-vector"):
            image, images[stem + "lt"] = make(("fold", mode, kind == "folded"), fold_sources(get, name),
                                              lambda: folded_linear(get, name, mode, kind == "folded"))
            if image is not None:
                images[name] = image
        elif kind in ("head-major", "head-major-folded"):
            fold = kind == "head-major-folded"
            images[key], images[stem + "hb"] = make(("head-major", mode, int(heads), fold),
                                                    fold_sources(get, name) if fold else (get(name), get(stem + "bias")),
                                                    lambda: head_major_qkv(get, name, heads, fold, mode))
        else:
            images[key] = make(("fused-mlp",), (get(name),), lambda: fused_mlp_fc2_image(get(name)))
    return images


def block_images(get, mode, heads, cache=None):
    """The image dict of one block on its own (Block.forward normalises: nothing folded; qkv + attention fused where it is the
    mode's only form), keyed as BLOCK_IMAGES."""
    names = [key for _, key in BLOCK_PARAMS]
    return make_images(plan_images(names, mode, (False, mode == MODE_BF16X3_IMAGES, False)), get, mode, heads, cache)


def fill_block_struct(dst, get, prefix="", images=None, what=None):
    """Fill a pafuse_block_weights from ``get(prefix + key)`` and the image dict (make_images); fields without an image stay
    null.  `what(key)`: the name a refused tensor goes by (default: its key)."""
    for field, key in BLOCK_PARAMS:
        setattr(dst, field, _ptr(get(prefix + key), what(key) if what else prefix + key))
    for field, key in BLOCK_IMAGES:
        t = images.get(prefix + key) if images else None
        setattr(dst, field, t.data_ptr() if t is not None else None)


# --------------------------------------------------------------------------------------------------- the cache
_image_cache = {}        # key_head + (data_ptr, _version, shape) per source + (device,) -> (what build() returned, the sources)
_IMAGE_CACHE_MAX = 2048  # ~ three models' worth of linear weights; the oldest entries go first


def cached(key_head, sources, build):
    """build() once per (key_head, storage, version and shape of every tensor in `sources`, device).  An entry keeps a reference
    to its sources: while it lives their storage cannot be freed, so no other tensor can come to sit at that address with a
    matching version and shape and hit a stale image (a freed temporary such as `w.float()` made per call would otherwise do
    exactly that)."""
    key = tuple(key_head) + tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in sources) + (sources[0].device,)
    hit = _image_cache.get(key)
    if hit is None:
        while len(_image_cache) >= _IMAGE_CACHE_MAX:
            _image_cache.pop(next(iter(_image_cache)))
        hit = _image_cache[key] = (build(), tuple(sources))
    return hit[0]


def cached_split_image(weight, layout, mode=MODE_BF16X3):
    """split_image through the cache: the schema'd ops take plain parameter tensors, so they build and cache the images the
    split-precision kernels read."""
    return cached(("plain", mode, int(layout)), (weight,), lambda: split_image(weight, layout, mode))


# ------------------------------------------------------------------------------------------------ the builders
def split_image(weight, layout, mode=MODE_BF16X3):
    """The pre-split image of one linear weight [N,K] on its device (pafuse_split_weights), a uint8 tensor.  `layout`: 0 the
    plain unit op (no model layer), 1 the whole-row layers (attn.proj, mlp.fc2), 2 attn.qkv and mlp.fc1 ('bf16x3' has these
    three geometries; the image pipelines one each).  `mode`: 'bf16x3' three bf16 slices, 6 bytes per element; 'f16x2' the H
    image (two fp16 slices of the power-of-two-scaled weight, 4 bytes per element + a 256-byte tail); 'bf16x3_images' the X
    image (three bf16 slices, [N][K/32][3][32])."""
    lib = _lib.load()
    N, K = weight.shape
    flags = int(layout) | SPLIT_FLAG[mode]
    img = torch.empty(lib.pafuse_split_image_bytes(N, K, flags), dtype=torch.uint8, device=weight.device)
    with torch.cuda.device(weight.device):
        _lib.check(lib.pafuse_split_weights(_ptr(weight.detach(), "weight"), N, K, flags, img.data_ptr(),
                                            torch.cuda.current_stream(weight.device).cuda_stream))
    return img


def fused_mlp_column_order(hidden, device=None):
    """Column order of fc2.weight in the fused MLP kernel's image (include/pafuse_hip.h pafuse_block_weights.fc2_hp): column
    16 b + 8 h + i of the image is column 16 b + 8 (i >> 2) + 4 h + (i & 3) of the weight - inside every group of 16 hidden
    units, the order in which fc1's accumulators hold them."""
    c = torch.arange(hidden, device=device)
    b, h, i = c // 16, (c // 8) % 2, c % 8
    return 16 * b + 8 * (i // 4) + 4 * h + (i % 4)


def fused_mlp_fc2_image(weight):
    """The f16x2 image of fc2.weight [C, 2C] for the fused MLP kernel: the image of W[:, fused_mlp_column_order]."""
    w = weight.detach()
    return split_image(w[:, fused_mlp_column_order(w.shape[1], w.device)].contiguous(), LAYOUT_OF["mlp.fc2.weight"], MODE_F16X2)


def fold_sources(get, name):
    """(W, g, beta, b): the linear weight `name` (a key ending in attn.qkv.weight / mlp.fc1.weight), the LayerNorm of its
    block in front of it, and its bias - what the folded images and vectors are made from."""
    suffix = next(s for s in FOLDED_LINEAR if name.endswith(s))
    norm = name[:-len(suffix)] + FOLDED_LINEAR[suffix]
    return get(name), get(norm + ".weight"), get(norm + ".bias"), get(name[:-len("weight")] + "bias")


def folded_linear(get, name, mode, image=True):
    """(image | None, lt) of the linear layer `name` with the LayerNorm in front of it folded in (include/pafuse_hip.h,
    pafuse_block_weights.qkv_lt): the split image of W (.) g (one fp32 rounding per element, then split exactly) and
    lt = W beta + b formed in fp64, rounded once.  (The stream is stored centred: there is no mean term.)"""
    weight, g, beta, bias = (t.detach() for t in fold_sources(get, name))
    lt = (weight.double() @ beta.double() + bias.double()).float().contiguous()
    return (split_image((weight * g[None, :]).contiguous(), image_layout(name), mode) if image else None), lt


def head_major_qkv(get, name, heads, fold, mode):
    """(image, hb) for the fused qkv + attention kernel (include/pafuse_hip.h pafuse_block_weights.qkv_hs): the qkv weight
    [3C, C] re-ordered head by head - q_h, k_h, v_h, each zero-padded from d to DP rows (DP = 32 for d <= 32, else 48) - as
    a layout-2 image; hb = the bias in that order; with the LayerNorm folded the image is that of W (.) g and hb = W beta + b
    (folded_linear's vector, re-ordered)."""
    weight, bias = get(name).detach(), get(name[:-len("weight")] + "bias").detach()
    d = weight.shape[0] // 3 // heads
    dp = 32 if d <= 32 else 48
    if fold:
        _, g, beta, _ = (t.detach() for t in fold_sources(get, name))
        bias = (weight.double() @ beta.double() + bias.double()).float()
        weight = weight * g[None, :]

    def reorder(t):                     # [3C, ...] -> [heads * 3 * dp, ...]
        t = t.reshape(3, heads, d, *t.shape[1:])
        out = t.new_zeros((heads, 3, dp) + tuple(t.shape[3:]))
        out[:, :, :d] = t.transpose(0, 1)
        return out.reshape(heads * 3 * dp, *t.shape[3:]).contiguous()
    return split_image(reorder(weight), 2, mode), reorder(bias)

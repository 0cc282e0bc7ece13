#!/usr/bin/env python3
"""sha256 of everything the attention forward writes, on seeded inputs: the record a change of the kernel is held against.

    python tools/record_attention_digests.py [LIB] [--label "commit ..."] [--out tests/golden/attention_parent_digests.json]

LIB: the library to record (pafuse_amd._lib.load(path), an explicit argument) - for the committed file the build of the
PARENT commit of the change under test, run from the tree that holds this tool; default: the tree's own library.
tests/test_attention_wave_items.py runs the same cases (cases() / run_rows() / run_image() below) on the tree's library and
asserts equal digests.

  rows    pafuse_attention on every L x head dim x heads x nseq of the lists below, contiguous and temporal (groups of GROUP
          sequences, tok_stride = GROUP); the output buffer, guard rows included, as raw bytes.  qkv is a window of one
          seeded pool, o a buffer of SENTINEL with GUARD rows in front of and behind the rows the call may touch.
  image   the f16x2 H image the kernel writes for the proj GEMM: pafuse_block_forward in 'f16x2' (qkv GEMM + attention with
          the image output) at one shape per kernel form; hashed: the block's output and its whole, zero-initialised
          workspace (the image lies in it), so no byte hashed is one the library did not write or the tool did not set.
All inputs are drawn on the CPU from seeded generators: two libraries see the same bytes.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
from functools import partial
from operator import attrgetter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (1, 15, 16, 17, 24, 27, 32, 33, 42, 48, 49, 68, 80)
HEAD_DIMS = (4, 28, 32, 48)
HEADS = (1, 7, 8)
NSEQ = (1, 3, 8, 9, 24)
GROUP = 3            # temporal addressing: row (r, t, j) = (r L + t) GROUP + j, sequence s = (r, j) = divmod(s, GROUP)
GUARD = 5            # rows of SENTINEL in front of and behind o
SENTINEL = -3.0
POOL_SEED, POOL_SHIFTS = 20261, 1021
IMAGE_FORMS = ((27, 224, 7), (42, 256, 8), (68, 224, 7), (27, 384, 8), (42, 384, 8), (68, 384, 8))   # (L, C, heads), 9 sequences


def cases():
    """[(key, L, d, heads, nseq, temporal)] in a fixed order"""
    return [(f"L{L}.d{d}.h{h}.n{n}.{'t' if t else 's'}", L, d, h, n, t)
            for L in LENGTHS for d in HEAD_DIMS for h in HEADS for n in NSEQ for t in (False, True)]


def layout(L, nseq, temporal):
    """(rows [nseq, L] of the sequences, M rows in all, addressing arguments of pafuse_attention)"""
    import torch
    s, t = torch.arange(nseq)[:, None], torch.arange(L)[None, :]
    if temporal:
        return ((s // GROUP) * L + t) * GROUP + s % GROUP, -(-nseq // GROUP) * L * GROUP, (GROUP, L * GROUP, 1, GROUP)
    return s * L + t, nseq * L, (1, L, 0, 1)


def pool(device="cuda"):
    """the seeded N(0, 1) pool every case's qkv is a window of, on the host and on the device"""
    import torch
    n = (max(NSEQ) * max(LENGTHS) + 2 * GUARD) * 3 * max(HEADS) * max(HEAD_DIMS) + 4 * POOL_SHIFTS
    host = torch.randn(n, generator=torch.Generator().manual_seed(POOL_SEED))
    return host, host.to(device)


def window(pool_t, index, M, C3):
    """qkv [GUARD + M + GUARD, 3C] of case number `index` (16-byte aligned: a multiple of four floats into the pool)"""
    off = 4 * ((index * 811) % POOL_SHIFTS)
    return pool_t[off:off + (M + 2 * GUARD) * C3].view(M + 2 * GUARD, C3)


def run_rows(lib, pool_dev, index, case):
    """o [GUARD + M + GUARD, C] on the device after pafuse_attention on case `index`"""
    import torch
    from pafuse_amd import _lib
    _, L, d, heads, nseq, temporal = case
    Cc = heads * d
    _, M, addressing = layout(L, nseq, temporal)
    qkv = window(pool_dev, index, M, 3 * Cc)
    o = torch.full((M + 2 * GUARD, Cc), SENTINEL, device=pool_dev.device)
    with torch.cuda.device(pool_dev.device):
        _lib.check(lib.pafuse_attention(qkv[GUARD:].data_ptr(), o[GUARD:].data_ptr(), nseq, L, Cc, heads, *addressing,
                                        torch.cuda.current_stream(pool_dev.device).cuda_stream))
    return o


def run_image(lib, form, device="cuda"):
    """(block output, workspace bytes) of pafuse_block_forward in 'f16x2' on 9 seeded sequences of `form`"""
    import torch
    from pafuse_amd import _lib
    from pafuse_amd.images import block_images, fill_block_struct
    from pafuse_amd.mixste2 import _BlockParams
    L, Cc, heads = form
    g = torch.Generator().manual_seed(1000 * L + Cc + heads)
    blk = _BlockParams(Cc, 2.0, True, partial(torch.nn.LayerNorm, eps=1e-6))

    def seeded(key, like):   # matrices at fan-in scale, LayerNorm gains around 1, biases small
        t = torch.randn(like.shape, generator=g)
        if like.dim() == 2:
            return t * like.shape[1] ** -0.5
        return 1 + 0.1 * t if "norm" in key and key.endswith("weight") else 0.1 * t
    blk.load_state_dict({k: seeded(k, v) for k, v in blk.state_dict().items()})
    blk = blk.to(device)
    y = torch.randn(9, L, Cc, generator=g).to(device)
    mode = _lib.PRECISIONS["f16x2"]
    get = lambda key: attrgetter(key)(blk)      # noqa: E731
    images = block_images(get, mode, heads)
    w = _lib.BlockWeights()
    fill_block_struct(w, get, images=images, what=lambda key: key.split(".")[-2])
    nbytes = lib.pafuse_block_workspace_bytes(9 * L, Cc)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(y.device):
        _lib.check(lib.pafuse_block_forward(C.byref(w), y.data_ptr(), 9, L, Cc, heads, mode, ws.data_ptr(), nbytes,
                                            torch.cuda.current_stream(y.device).cuda_stream))
        torch.cuda.synchronize()
    del images
    return y, ws


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def image_key(form):
    return "image.L%d.C%d.h%d" % form


def record(lib):
    _, pool_dev = pool()
    out = {case[0]: sha(run_rows(lib, pool_dev, i, case)) for i, case in enumerate(cases())}
    for form in IMAGE_FORMS:
        y, ws = run_image(lib, form)
        out[image_key(form) + ".y"], out[image_key(form) + ".workspace"] = sha(y), sha(ws)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib", nargs="?", default=None, help="the library to record (default: the tree's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attention_parent_digests.json"))
    ap.add_argument("--label", default="", help="what the library was built from (the parent's commit), kept in the file")
    a = ap.parse_args()
    from pafuse_amd import _lib
    lib = _lib.load(os.path.abspath(a.lib) if a.lib else None)
    digests = record(lib)
    with open(a.out, "w") as f:
        json.dump({"library": lib.pafuse_version().decode(), "recorded_from": a.label, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {a.out}")


if __name__ == "__main__":
    main()

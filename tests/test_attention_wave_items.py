"""GPU tests of the short attention forward through pafuse_attention - the one-item-per-wave kernel (attn_wave_kernel: the forms
<48,32>, <80,32>, <32,48>, <48,48>) and the workgroup kernel where attention() keeps it (<32,32>, <80,48>): against fp64,
against the bits of the workgroup kernel that served every form before, and for writes outside its rows.

Cases (tools/record_attention_digests.py, shared with the recording tool): every L in 1, 15, 16, 17, 24, 27, 32, 33, 42, 48, 49,
68, 80 x head dim 4, 28, 32, 48 x heads 1, 7, 8 x nseq 1, 3, 8, 9, 24, contiguous and temporal (groups of 3 sequences,
tok_stride 3): both sides of every padded length and head dim, both branches of attn_item<4>, last workgroups with one to
three idle waves, temporal groups whose last sequences do not exist.  qkv is a window of one seeded N(0, 1) pool.

Asserted per case:
  * guard rows: o is handed over as a buffer of a sentinel value with 5 rows in front of and behind the rows the call may
    touch; every row no sequence owns (the guards, and inside a temporal group the rows of sequences past nseq) still holds
    the sentinel bit for bit;
  * fp64: max |o - softmax(q k^T d^-1/2) v in fp64 on the host| <= 2e-6, the bound of test_hip_parity.test_attention_contiguous
    and test_attention_temporal_strides at the same input scale;
  * the same bits as the parent commit's kernel: sha256 of the whole o buffer == tests/golden/attention_parent_digests.json,
    which tools/record_attention_digests.py wrote from the parent commit's library on these inputs.
Asserted per L, over all its cases pooled: mean error <= 1.5 x the mean error of torch's fp32 evaluation + 1e-9
(test_attention_contiguous' second bound; pooled, because on the 4 .. 60 output values of the smallest cases a ratio of two
means is noise, and the bound is a statement about the arithmetic, which is the same in every case).
The H image output (f16x2 pipeline) has no entry point of its own: pafuse_block_forward in 'f16x2' at one shape per kernel
form, block output and whole workspace (the image lies in it) against the parent's digests.
"""
import json
import os

import pytest
import torch

from tools import record_attention_digests as rec

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_parent_digests.json")


@pytest.fixture(scope="module")
def shared():
    """(library, pool on the host, pool on the device, the parent's digests)"""
    from pafuse_amd import _lib
    with open(GOLDEN) as f:
        digests = json.load(f)["digests"]
    host, dev = rec.pool()
    return _lib.load(), host, dev, digests


def _reference(qkv, rows, heads, dtype):
    """softmax(q k^T d^-1/2) v per (sequence, head) in `dtype` -> [nseq * L, C] in fp64, row order of rows.reshape(-1)"""
    nseq, L = rows.shape
    C = qkv.shape[1] // 3
    d = C // heads
    x = qkv[rows].to(dtype).reshape(nseq, L, 3, heads, d)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-2, -1) * d ** -0.5, dim=-1)
    return (p @ v).transpose(1, 2).reshape(nseq * L, C).double()


@pytest.mark.parametrize("L", rec.LENGTHS)
def test_wave_attention_against_fp64_parent_bits_and_guards(shared, L):
    lib, host, dev, digests = shared
    bad, n, worst, err_sum, err_t_sum, count = [], 0, 0.0, 0.0, 0.0, 0
    for index, case in enumerate(rec.cases()):
        key, Lc, d, heads, nseq, temporal = case
        if Lc != L:
            continue
        n += 1
        rows, M, _ = rec.layout(L, nseq, temporal)
        o = rec.run_rows(lib, dev, index, case).cpu()
        rows = rows + rec.GUARD                      # in the buffers, behind the front guard
        owned = rows.reshape(-1)
        free = torch.ones(o.shape[0], dtype=torch.bool)
        free[owned] = False
        guards = bool(free[:rec.GUARD].all() and free[-rec.GUARD:].all()) and torch.equal(o[free], torch.full_like(o[free], rec.SENTINEL))
        qkv = rec.window(host, index, M, 3 * heads * d)
        truth = _reference(qkv, rows, heads, torch.float64)
        err = (o[owned].double() - truth).abs()
        err_t = (_reference(qkv, rows, heads, torch.float32) - truth).abs()
        e = float(err.max())
        worst = max(worst, e) if e == e else float("nan")
        err_sum, err_t_sum, count = err_sum + float(err.sum()), err_t_sum + float(err_t.sum()), count + err.numel()
        same = rec.sha(o) == digests[key]
        if not guards or not e <= 2e-6 or not same:
            bad.append((key, "guards ok" if guards else "GUARD ROWS WRITTEN", e, "bits ok" if same else "BITS DIFFER"))
    mean, mean_t = err_sum / count, err_t_sum / count
    print(f"L={L}: {n} cases, largest error {worst:.2e}, mean {mean:.2e} (torch fp32 {mean_t:.2e}), {len(bad)} failing")
    assert n == len(rec.HEAD_DIMS) * len(rec.HEADS) * len(rec.NSEQ) * 2
    assert not bad, bad
    assert mean <= 1.5 * mean_t + 1e-9, (mean, mean_t)


@pytest.mark.parametrize("form", rec.IMAGE_FORMS, ids=[rec.image_key(f) for f in rec.IMAGE_FORMS])
def test_wave_attention_h_image_has_the_parent_bits(shared, form):
    lib, _, _, digests = shared
    y, ws = rec.run_image(lib, form)
    assert bool(torch.isfinite(y).all())
    assert rec.sha(y) == digests[rec.image_key(form) + ".y"], "block output differs"
    assert rec.sha(ws) == digests[rec.image_key(form) + ".workspace"], "workspace (H image of o) differs"

"""fp64 references of the training step's first- and last-layer gradients, written from the definitions (reshape and sum,
dout^T hn), and the shapes the GPU tests run them at.  tests/test_train_rim_host.py proves the references against torch
autograd on a machine without a GPU; tests/test_hip_train_rim.py compares the HIP kernels with them."""
import torch


def group_sum_ref(x, mode):
    """x [B,F,J,C] summed per joint (mode 0 -> [J,C]), per frame (1 -> [F,C]) or per sample (2 -> [B,C])"""
    x = x.double()
    return x.sum((0, 1)) if mode == 0 else (x.sum((0, 2)) if mode == 1 else x.sum((1, 2)))


def head_grad_ref(dout, hn, head_w):
    """out = hn head_w^T + head_b: (d head_w [3,C], d head_b [3], d hn [M,C]) from dout [M,3]"""
    dout, hn, head_w = dout.double(), hn.double(), head_w.double()
    return dout.t() @ hn, dout.sum(0), dout @ head_w


def patch_grad_ref(x2d, x3d, g):
    """x0 = cat(x2d, x3d) patch_w^T + patch_b + pos_spatial[j] + temb[b]: (d patch_w [C,5], d patch_b [C], d pos_spatial [J,C],
    d temb [B,C]) from g = d x0 [B,F,J,C]"""
    g = g.double()
    C = g.shape[-1]
    inputs = torch.cat((x2d.double(), x3d.double()), -1)
    return g.reshape(-1, C).t() @ inputs.reshape(-1, 5), g.reshape(-1, C).sum(0), group_sum_ref(g, 0), group_sum_ref(g, 2)


def sinusoid_ref(a):
    """[sin(a) | cos(a)] of the argument a [B,C/2], in the dtype of a"""
    return torch.cat((a.sin(), a.cos()), -1)


# (B, F, J, C) of the group-sum cases.  The sums run over count = B F (mode 0), B J (mode 1), F J (mode 2) rows per group, cut into
# at most 32 chunks of at least 16; per mode the counts below hit: 1; below 16; a multiple of the chunk length; a ragged last
# chunk; a chunk count that drops when it is recomputed from the rounded-up chunk length (520: 32 chunks -> 17 rows -> 31 chunks);
# the cap of 32 chunks.  split_form() names the form and test_train_rim_host.py checks the coverage.  C = 384 leaves a partial
# second pass of the 256 channels a workgroup covers at a time; F != J, both > 1, everywhere but the first case.
GROUP_SUM_CASES = [
    (1, 1, 1, 4),          # 1, 1, 1
    (2, 3, 5, 64),         # 6, 10, 15: below 16
    (4, 8, 16, 224),       # 32, 64, 128: whole chunks of 16
    (26, 20, 26, 64),      # 520, 676, 520: 31 chunks after the recount
    (32, 16, 64, 256),     # 512, 2048, 1024: 32 whole chunks; mode 0 sums n = J C = 16384 columns (the one-thread-per-column join)
    (2, 27, 42, 384),      # 54, 84, 1134: ragged / whole / 32 chunks joined by 16 threads per column (n = 768 < 16384)
    (2, 27, 24, 384),      # 54, 48, 648: 648 -> 32 chunks -> 21 rows -> 31 chunks
    (37, 27, 68, 224),     # 999, 2516, 1836: the face model's step
]


def group_count(mode, B, F, J):
    return B * F if mode == 0 else (B * J if mode == 1 else F * J)


def split_form(count):
    """(chunks, set of the forms `count` rows take) under the split documented above - a statement of which cases are
    covered, not a reference of any result.  It restates group_chunks() of pafuse_amd/csrc/train_host.inc: change them together."""
    guess = min(32, (count + 15) // 16)
    per = (count + guess - 1) // guess
    chunks = (count + per - 1) // per
    forms = set()
    if count == 1:
        forms.add("one")
    elif count < 16:
        forms.add("below16")
    if count >= 16:
        forms.add("whole" if count % per == 0 else "ragged")
    if chunks < guess:
        forms.add("recount")
    if chunks == 32:
        forms.add("cap")
    return chunks, forms


HEAD_CASES = [(1, 64), (63, 224), (64, 384), (65, 64), (4097, 224), (16385, 384)]      # (M, C)
PATCH_CASES = [(1, 1, 1, 4), (3, 5, 7, 64), (2, 27, 24, 384), (37, 27, 42, 256)]       # (B, F, J, C)

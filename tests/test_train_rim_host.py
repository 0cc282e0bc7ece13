"""CPU-only: the fp64 references of tests/train_rim_reference.py (what tests/test_hip_train_rim.py holds the HIP kernels of the
training step's first and last layers to) equal torch autograd on a plain statement of those layers, and the group-sum cases
cover every form of the row split."""
import torch

from tests import train_rim_reference as ref


def test_references_equal_autograd_on_the_first_and_last_layers():
    B, F, J, C = 2, 3, 5, 8
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)      # noqa: E731
    leaf = lambda *shape: rnd(*shape).requires_grad_(True)                          # noqa: E731
    close = lambda a, b: a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-12)   # noqa: E731
    # first layer: patch embedding + spatial position embedding + time embedding
    x2d, x3d = rnd(B, F, J, 2), rnd(B, F, J, 3)
    Wp, bp, pos_s, temb = leaf(C, 5), leaf(C), leaf(J, C), leaf(B, C)
    x0 = torch.cat((x2d, x3d), -1) @ Wp.T + bp + pos_s[None, None] + temb[:, None, None]
    gx0 = rnd(B, F, J, C)
    x0.backward(gx0)
    d_w, d_b, d_pos, d_temb = ref.patch_grad_ref(x2d, x3d, gx0)
    assert close(d_w, Wp.grad) and close(d_b, bp.grad) and close(d_pos, pos_s.grad) and close(d_temb, temb.grad)
    assert close(ref.group_sum_ref(gx0, 0), pos_s.grad) and close(ref.group_sum_ref(gx0, 2), temb.grad)
    # temporal position embedding
    x, pos_t = rnd(B, F, J, C), leaf(F, C)
    y = x + pos_t[None, :, None]
    gy = rnd(B, F, J, C)
    y.backward(gy)
    assert close(ref.group_sum_ref(gy, 1), pos_t.grad)
    # output head
    hn, Wh, bh = leaf(B * F * J, C), leaf(3, C), leaf(3)
    out = hn @ Wh.T + bh
    dout = rnd(B * F * J, 3)
    out.backward(dout)
    d_w, d_b, d_hn = ref.head_grad_ref(dout, hn.detach(), Wh.detach())
    assert close(d_w, Wh.grad) and close(d_b, bh.grad) and close(d_hn, hn.grad)
    # the sinusoid's layout: sines in front, cosines behind
    a = rnd(B, C // 2)
    s = ref.sinusoid_ref(a)
    assert torch.equal(s[:, :C // 2], a.sin()) and torch.equal(s[:, C // 2:], a.cos())


def test_group_sum_cases_cover_every_form_of_the_row_split():
    want = {"one", "below16", "whole", "ragged", "recount", "cap"}
    for mode in (0, 1, 2):
        seen = set()
        for B, F, J, C in ref.GROUP_SUM_CASES:
            seen |= ref.split_form(ref.group_count(mode, B, F, J))[1]
        assert seen == want, (mode, want - seen)
    assert ref.split_form(520) == (31, {"ragged", "recount"}) and ref.split_form(512) == (32, {"whole", "cap"})
    assert {c[3] for c in ref.GROUP_SUM_CASES} >= {4, 64, 224, 256, 384}
    assert any(F != J and F > 1 and J > 1 for _, F, J, _ in ref.GROUP_SUM_CASES) and (37, 27, 68, 224) in ref.GROUP_SUM_CASES
    # the two forms of the join of the partials: 16 threads per column below 16384 columns with 32 parts, one thread otherwise
    joins = {(ref.split_form(ref.group_count(m, B, F, J))[0] >= 32 and (J, F, B)[m] * C < 16384)
             for B, F, J, C in ref.GROUP_SUM_CASES for m in (0, 1, 2)}
    assert joins == {True, False}
    assert any(ref.split_form(ref.group_count(m, B, F, J))[0] == 32 and (J, F, B)[m] * C >= 16384      # 32 parts, one thread
               for B, F, J, C in ref.GROUP_SUM_CASES for m in (0, 1, 2))
    assert (ref.split_form(27 * 42)[0], 2 * 384 < 16384) == (32, True)      # mode 2 of (2, 27, 42, 384): F J = 1134 rows, n = B C
    assert {M for M, _ in ref.HEAD_CASES} == {1, 63, 64, 65, 4097, 16385} and {C for _, C in ref.HEAD_CASES} == {64, 224, 384}

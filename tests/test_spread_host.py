"""Host side of the hypothesis spread (no GPU): the state size formula, the refusals of the C ABI that happen before the
first HIP call (each with its entry's name in pafuse_last_error), the argument checks of the Python layers, the stitching of
std and covariance clips, and the example's option."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

E_ARG = -1


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def test_abi_version_is_unchanged():
    from pafuse_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib().pafuse_abi_version() == 8
    for name in ("pafuse_spread_partials_bytes", "pafuse_spread_partials", "pafuse_spread_combine"):
        assert name in _lib.SIGNATURES


def test_state_size_formula_needs_no_library_and_has_no_p_in_it():
    from pafuse_amd import ops
    assert list(inspect.signature(ops.spread_partials_bytes).parameters) == ["B", "T", "F", "J"]
    shapes = ((1, 10, 27, 134), (64, 10, 27, 134), (2, 2, 3, 134), (1, 1, 1, 134), (1, 1, 1, 1), (1, 1, 1, 5), (3, 2, 243, 133))
    L = lib()
    for B, T, F, J in shapes:
        want = (9 * B * T * F * J + 1) * 8
        assert ops.spread_partials_bytes(B, T, F, J) == want == L.pafuse_spread_partials_bytes(B, T, F, J)
    assert ops.spread_partials_bytes(1, 10, 27, 134) == (9 * 36180 + 1) * 8 == 2_604_968
    for bad in ((0, 1, 4, 17), (-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0)):
        assert L.pafuse_spread_partials_bytes(*bad) == 0
        assert ops.spread_partials_bytes(*bad) == 0


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call: host pointers are never followed"""
    L = lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok = [p, p, 1, 1, 1, 1, 1, 0, p, 512, None]                        # B = T = P_r = F = J = 1: an 80-byte state

    def partials(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_spread_partials(*a)

    def refused(rc, entry):
        assert rc == E_ARG
        assert entry in L.pafuse_last_error(), L.pafuse_last_error()

    for i in (2, 3, 4, 5, 6, 7):                                       # B, T, P_r, F, J, h0 negative
        refused(partials(**{f"a{i}": -1}), b"spread_partials")
    for i in (3, 5, 6):                                                # T, F, J zero
        refused(partials(**{f"a{i}": 0}), b"spread_partials")
    refused(partials(a0=None), b"spread_partials")                     # pred, conn with work to do
    refused(partials(a1=None), b"spread_partials")
    refused(partials(a8=None), b"spread_partials")                     # state: none, short, misaligned
    refused(partials(a9=79), b"spread_partials")
    refused(partials(a8=p + 4), b"spread_partials")
    big = 1 << 10                                                      # n = 2^40 elements: 2^32 blocks
    refused(partials(a2=big, a3=big, a5=big, a6=big, a9=(9 * big ** 4 + 1) * 8), b"spread_partials")
    assert b"grid" in L.pafuse_last_error()
    refused(partials(a2=big, a3=big, a5=big, a6=big), b"spread_partials")        # and 512 bytes are short for it

    okc = [p, 1, 80, 1, 1, 1, 1, None, p, p, p, None]

    def combine(**kw):
        a = list(okc)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_spread_combine(*a)

    refused(combine(a1=0), b"spread_combine")                          # W < 1
    for i in (3, 4, 5, 6):
        refused(combine(**{f"a{i}": -1}), b"spread_combine")
    for i in (4, 5, 6):
        refused(combine(**{f"a{i}": 0}), b"spread_combine")
    refused(combine(a2=72), b"spread_combine")                         # stride: smaller than the state
    refused(combine(a2=84), b"spread_combine")                         # ... not a multiple of 8
    refused(combine(a0=None), b"spread_combine")
    refused(combine(a0=p + 4), b"spread_combine")
    refused(combine(a8=None, a9=None, a10=None), b"spread_combine")    # no output requested
    assert b"nothing to write" in L.pafuse_last_error()
    refused(combine(a1=2, a7=p + 80, a8=None, a9=None, a10=None), b"spread_combine")      # merged over the second operand
    refused(combine(a7=p + 4, a8=None, a9=None, a10=None), b"spread_combine")             # misaligned merged state
    refused(combine(a3=big, a4=big, a5=big, a6=big, a2=(9 * big ** 4 + 1) * 8), b"spread_combine")
    assert b"grid" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import evaluate, ops
    z = torch.zeros
    with pytest.raises(ValueError):                                     # CPU tensors: no fallback
        ops.spread_partials(z(1, 1, 2, 2, 3, 3), z(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError):                                     # not [B,T,P,F,J,3]
        ops.spread_partials(z(1, 2, 2, 3, 3), z(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        ops.spread_partials(z(1, 1, 2, 2, 3, 3), z(3, dtype=torch.int32), -1)
    with pytest.raises(ValueError):
        ops.spread_partials(z(1, 1, 2, 2, 3, 3), z(3, dtype=torch.int64), 0)
    with pytest.raises(ValueError):
        ops.combine_spread(z(1, 100, dtype=torch.float64), (1, 1, 2, 3))
    with pytest.raises(ValueError):
        ops.combine_spread(z(1, 100, dtype=torch.float64), (1, 1, 2, 3), want=("median",))
    with pytest.raises(ValueError):
        ops.spread_views(z(54, dtype=torch.float64), 1, 1, 2, 3)        # 55 doubles are a state of (1,1,2,3)
    v = ops.spread_views(z(55, dtype=torch.float64), 1, 1, 2, 3)
    assert tuple(v["sum"].shape) == (1, 1, 2, 3, 3) and tuple(v["m2"].shape) == (1, 1, 2, 3, 6) and tuple(v["count"].shape) == (1,)
    with pytest.raises(ValueError):
        evaluate.aggregate_poses_sharded(None, None, 5, None)
    state = evaluate.PoseState((1, 1, 2, 3), "cpu", reproj=False)
    for want in (("std",), ("cov",), ("mean", "std")):
        with pytest.raises(ValueError, match="spread state"):
            evaluate.aggregate_poses_sharded(None, None, 5, None, state=state, want=want)
    spread = evaluate.SpreadState((1, 1, 2, 3), "cpu")
    with pytest.raises(ValueError, match="mean-only"):                  # a spread state alone has no pick either
        evaluate.aggregate_poses_sharded(None, None, 5, None, spread_state=spread, want=("pick", "std"))
    assert "spread_state" in inspect.signature(evaluate.aggregate_poses_sharded).parameters


def test_spread_state_refuses_a_gap():
    from pafuse_amd import evaluate
    state = evaluate.SpreadState((1, 1, 2, 3), "cpu")
    assert isinstance(state, evaluate._RunningState)
    merges = []
    fold = lambda count, h0: state.fold("accumulate_spread", count, h0, 55, None, lambda row: row.zero_(), merges.append)
    fold(2, 4)
    fold(3, 6)
    assert (state.h0, state.count, len(merges), len(state.tails)) == (4, 5, 1, 0) and state.head.numel() == 55
    with pytest.raises(ValueError, match="accumulate_spread"):
        fold(1, 10)
    with pytest.raises(ValueError, match="accumulate_spread"):
        fold(1, 8)
    assert (state.h0, state.count) == (4, 5)


def test_infer_sequence_refuses_before_touching_the_model():
    from pafuse_amd import harness
    assert inspect.signature(harness.infer_sequence).parameters["spread"].default is None
    seq = torch.zeros(30, 134, 2)
    call = lambda **kw: harness.infer_sequence(None, None, seq, [], [], **kw)
    with pytest.raises(ValueError, match="spread"):
        call(spread="std")
    with pytest.raises(ValueError, match="spread"):
        call(spread="cov", aggregate=None)
    with pytest.raises(ValueError, match="spread"):
        call(spread="variance", aggregate="mean")
    with pytest.raises(ValueError, match="spread"):
        call(spread=True, aggregate="mean")


@pytest.mark.parametrize("total", [70, 54, 27, 28, 11])
def test_stitch_spread_follows_stitch_poses(total):
    from pafuse_amd import harness
    frames = 27
    clips = harness.cut_clips(torch.zeros(total, 1, 1), frames).shape[0]
    g = torch.Generator().manual_seed(total)
    std = torch.rand(clips, 2, frames, 5, generator=g)
    cov = torch.randn(clips, 2, frames, 5, 6, generator=g)
    got = harness.stitch_spread(std, total, frames)
    assert tuple(got.shape) == (2, total, 5)
    # the rule of stitch_poses: std repeated along a trailing axis of 3 is stitched like a pose
    assert torch.equal(got, harness.stitch_poses(std[..., None].expand(-1, -1, -1, -1, 3).contiguous(), total, frames)[..., 1])
    got6 = harness.stitch_spread(cov, total, frames)
    assert tuple(got6.shape) == (2, total, 5, 6)
    for k in range(6):
        assert torch.equal(got6[..., k], harness.stitch_spread(cov[..., k].contiguous(), total, frames))
    if total > frames:                                     # the last clip gives only its final frames
        left = total - (clips - 1) * frames
        assert torch.equal(got[:, -left:], std[-1, :, -left:]) and torch.equal(got[:, :frames], std[0])


def test_example_option():
    script = os.path.join(ROOT, "examples", "infer_in_the_wild.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "--spread {std,cov}" in out.stdout
    out = subprocess.run([sys.executable, script, "--spread", "std"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 2 and "--aggregate mean" in out.stderr


def test_torch_op_schema_and_fake():
    from pafuse_amd import torch_ops  # noqa: F401
    s = str(torch.ops.pafuse.hypothesis_spread.default._schema)
    assert "Tensor pred, Tensor conn" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        mean, cov, std = torch.ops.pafuse.hypothesis_spread(torch.empty(2, 3, 5, 4, 134, 3, device="cuda"),
                                                            torch.empty(134, device="cuda", dtype=torch.int32))
        assert tuple(mean.shape) == (2, 3, 4, 134, 3) and tuple(cov.shape) == (2, 3, 4, 134, 6) and tuple(std.shape) == (2, 3, 4, 134)
        assert mean.dtype == cov.dtype == std.dtype == torch.float32

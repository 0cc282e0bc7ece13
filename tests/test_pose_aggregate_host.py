"""Host side of the pose aggregation (no GPU): stitching of aggregated clips, the argument checks of infer_sequence, the
state size formula, the refusals of the C ABI that happen before the first HIP call, and the example's options."""
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


@pytest.mark.parametrize("total", [70, 54, 27, 28, 11])
def test_stitch_poses_follows_stitch_clips(total):
    from pafuse_amd import harness
    frames = 27
    clips = harness.cut_clips(torch.zeros(total, 1, 1), frames).shape[0]
    g = torch.Generator().manual_seed(total)
    poses = torch.randn(clips, 2, frames, 5, 3, generator=g)
    got = harness.stitch_poses(poses, total, frames)
    want = harness.stitch_clips(poses[:, :, None], total, frames)
    assert tuple(got.shape) == (2, total, 5, 3) and tuple(want.shape) == (2, 1, total, 5, 3)
    assert torch.equal(got, want[:, 0])
    if total > frames:                                     # the last clip gives only its final frames
        left = total - (clips - 1) * frames
        assert torch.equal(got[:, -left:], poses[-1, :, -left:]) and torch.equal(got[:, :frames], poses[0])


def test_infer_sequence_refuses_before_touching_the_model():
    from pafuse_amd import harness
    sig = inspect.signature(harness.infer_sequence).parameters
    assert all(sig[k].default is None for k in ("aggregate", "cam", "traj", "hypothesis_chunk"))
    seq = torch.zeros(30, 134, 2)
    cam, traj = torch.zeros(9), torch.zeros(30, 3)
    call = lambda **kw: harness.infer_sequence(None, None, seq, [], [], **kw)
    with pytest.raises(ValueError, match="reproj"):
        call(aggregate="reproj")
    with pytest.raises(ValueError, match="reproj"):
        call(aggregate="reproj", cam=cam)
    with pytest.raises(ValueError, match="reproj"):
        call(aggregate="reproj", traj=traj)
    with pytest.raises(ValueError, match="aggregate"):
        call(aggregate="median")
    with pytest.raises(ValueError, match="hypothesis_chunk"):
        call(hypothesis_chunk=2)
    with pytest.raises(ValueError, match="hypothesis_chunk"):
        call(aggregate="mean", hypothesis_chunk=0)


def test_state_size_formula_needs_no_library_and_has_no_p_in_it():
    from pafuse_amd import ops
    assert list(inspect.signature(ops.pose_partials_bytes).parameters) == ["B", "T", "F", "J"]
    shapes = ((1, 10, 27, 134), (64, 10, 27, 134), (2, 2, 3, 134), (1, 1, 1, 134), (0, 1, 4, 17), (1, 1, 1, 5), (3, 2, 243, 133))
    for B, T, F, J in shapes:
        n = B * T * F * J
        want = (44 * n + 7) // 8 * 8
        assert ops.pose_partials_bytes(B, T, F, J) == want and want % 8 == 0 and 44 * n <= want < 44 * n + 8
    assert ops.pose_partials_bytes(1, 10, 27, 134) == 1_591_920       # P = 20 or P = 160: the same 1.6 MB per clip
    L = lib()
    for B, T, F, J in shapes:
        assert L.pafuse_pose_partials_bytes(B, T, F, J) == ops.pose_partials_bytes(B, T, F, J)
    for bad in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, -1, 1), (1, 1, 1, 0)):
        assert L.pafuse_pose_partials_bytes(*bad) == 0


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    L = lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok = [p, p, p, p, p, 1, 1, 1, 1, 1, 0, p, 512, None]              # B = T = P_r = F = J = 1: a 48-byte state

    def partials(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_pose_partials(*a)

    for i in (5, 6, 7, 8, 9, 10):                                      # B, T, P_r, F, J, h0 negative
        assert partials(**{f"a{i}": -1}) == E_ARG, i
    assert partials(a6=0) == E_ARG and partials(a8=0) == E_ARG and partials(a9=0) == E_ARG
    assert partials(a1=None) == E_ARG and partials(a2=None) == E_ARG and partials(a3=None) == E_ARG     # two of the three
    assert partials(a1=None, a2=None) == E_ARG and partials(a2=None, a3=None) == E_ARG                 # one of the three
    assert partials(a0=None) == E_ARG and partials(a4=None) == E_ARG                                   # pred, conn
    assert partials(a0=None, a1=None, a2=None, a3=None) == E_ARG                                       # mean-only still needs pred
    assert partials(a11=None) == E_ARG and partials(a12=47) == E_ARG and partials(a11=p + 4) == E_ARG  # state: none, short, misaligned
    assert b"pose_partials" in L.pafuse_last_error()
    okc = [p, 1, 48, 1, 1, 1, 1, 1, None, p, p, p, None]

    def combine(**kw):
        a = list(okc)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_pose_combine(*a)

    assert combine(a1=0) == E_ARG and combine(a4=0) == E_ARG and combine(a3=-1) == E_ARG
    assert combine(a2=40) == E_ARG and combine(a2=52) == E_ARG          # stride: short / not a multiple of 8
    assert combine(a0=None) == E_ARG
    assert combine(a9=None, a10=None, a11=None) == E_ARG                # nothing to write
    assert combine(a7=0) == E_ARG                                       # the mean needs P_total
    assert combine(a1=2, a8=p + 48) == E_ARG                            # merged over the second operand
    assert combine(a8=p + 4, a9=None, a10=None, a11=None) == E_ARG      # misaligned merged state
    assert b"pose_combine" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import evaluate, ops
    z = torch.zeros
    with pytest.raises(ValueError):                                     # CPU tensors: no fallback
        ops.pose_partials(z(1, 1, 2, 2, 3, 3), z(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        ops.combine_poses(z(1, 100, dtype=torch.float64), (1, 1, 2, 3), 2)
    with pytest.raises(ValueError):
        ops.combine_poses(z(1, 100, dtype=torch.float64), (1, 1, 2, 3), 2, want=("median",))
    with pytest.raises(ValueError):
        evaluate.aggregate_poses_sharded(None, None, 5, None)
    state = evaluate.PoseState((1, 1, 2, 3), "cpu", reproj=False)
    with pytest.raises(ValueError, match="mean-only"):
        evaluate.aggregate_poses_sharded(None, None, 5, None, state=state, want=("pick",))


def test_example_options():
    script = os.path.join(ROOT, "examples", "infer_in_the_wild.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "--aggregate {none,mean}" in out.stdout and "--hypothesis-chunk" in out.stdout
    out = subprocess.run([sys.executable, script, "--hypothesis-chunk", "2"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 2 and "--aggregate mean" in out.stderr


def test_torch_op_schema_and_fake():
    from pafuse_amd import torch_ops  # noqa: F401
    s = str(torch.ops.pafuse.aggregate_poses.default._schema)
    assert "Tensor pred, Tensor conn, Tensor? x2d=None" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        mean, pick, idx = torch.ops.pafuse.aggregate_poses(torch.empty(2, 3, 5, 4, 134, 3, device="cuda"),
                                                           torch.empty(134, device="cuda", dtype=torch.int32))
        assert tuple(mean.shape) == tuple(pick.shape) == (2, 3, 4, 134, 3) and tuple(idx.shape) == (2, 3, 4, 134)
        assert idx.dtype == torch.int32

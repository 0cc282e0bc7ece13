"""Host-side bookkeeping of the sharded evaluation (no GPU): state sizes against the library's own formula, the bytes a
rank receives in either gather mode, shard and chunk offsets for ragged P, argument refusals of the C ABI and of the
Python layers, and the flag plumbing down to the examples."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

from pafuse_amd.parallel import ShardedSampler, shard_counts, shard_range
from tests.conftest import ROOT

E_ARG, E_SHAPE = -1, -2


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def test_state_size_formula_matches_the_library():
    from pafuse_amd import ops
    L = lib()
    for B, T, P_r, F, J, parts in ((1, 10, 20, 27, 134, 4), (64, 10, 20, 27, 134, 4), (2, 2, 0, 5, 134, 4), (0, 1, 3, 4, 17, 1),
                                   (3, 2, 7, 243, 134, 3)):
        want = 40 * B * T * F * J + 8 * P_r * T * (1 + parts)
        assert ops.partials_bytes(B, T, P_r, F, J, parts) == want == L.pafuse_hypothesis_partials_bytes(B, T, P_r, F, J, parts)
        assert want % 8 == 0
        nblk = (F * J + 255) // 256
        assert L.pafuse_hypothesis_partials_workspace_bytes(B, T, P_r, F, J, parts) == 8 * B * T * nblk * P_r * (1 + parts)
    for bad in ((-1, 1, 1, 1, 1, 4), (1, 0, 1, 1, 1, 4), (1, 1, -1, 1, 1, 4), (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 5)):
        assert L.pafuse_hypothesis_partials_bytes(*bad) == 0


def test_bytes_per_rank_at_the_evaluation_shape():
    """BASELINE configs[3] at the reference's evaluation shape: P = 160 over 8 ranks, 64 clips per call.  What every rank
    receives: all hypotheses (B*T*P*F*J*12 bytes) against world states of 40*B*T*F*J + 8*(1+parts)*T*P_max bytes."""
    from pafuse_amd import ops
    B, T, P, F, J, world, parts = 64, 10, 160, 27, 134, 8, 4
    hypotheses = B * T * P * F * J * 3 * 4
    assert hypotheses == 4_445_798_400                                  # 4.45 GB into each rank
    pmax = max(shard_counts(P, world))
    state = ops.partials_bytes(B, T, pmax, F, J, parts)
    assert state == 40 * B * T * F * J + 8 * 5 * T * pmax == 92_628_800    # 92.6 MB per rank's state, whatever P is
    assert world * state == 741_030_400 and hypotheses / (world * state) > 5.9
    assert ops.partials_bytes(B, T, 4 * pmax, F, J, parts) - state == 8 * 5 * T * 3 * pmax    # P enters through the tail only
    # the scratch the unsharded evaluation adds (e3 + epb) does not exist on this path; the state is 1/48 of gathered + scratch
    assert (hypotheses + 2 * B * T * P * F * J * 4) / state > 79


def test_ragged_shards_and_chunks_cover_the_axis():
    assert [shard_range(20, r, 3) for r in range(3)] == [(0, 7), (7, 14), (14, 20)]
    assert shard_counts(20, 3) == [7, 7, 6] and shard_counts(5, 2) == [3, 2] and shard_counts(1, 3) == [1, 0, 0]

    class Model:
        num_proposals, proposal_shard, frames, num_kps, calls = 20, None, 3, 4, 0

        def ddim_steps(self):
            return [0, 1]

        def __call__(self, x2d, x3d, input_2d_flip=None):
            lo, hi = self.proposal_shard
            assert hi > lo
            self.calls += 1
            return torch.zeros(1, 2, hi - lo, 3, 4, 3)

    s = ShardedSampler(Model())
    x = torch.zeros(1, 3, 4, 2)
    assert s.local_range() == (0, 20)
    assert [(h0, n) for _, h0, n in s.sample_chunks(x, None, chunk=7)] == [(0, 7), (7, 7), (14, 6)]
    assert [(h0, n) for _, h0, n in s.sample_chunks(x, None)] == [(0, 20)]
    assert [(h0, n) for _, h0, n in s.sample_chunks(x, None, chunk=50)] == [(0, 20)]
    pred, h0, n = s.sample_local(x, None)
    assert (h0, n, pred.shape[2]) == (0, 20, 20) and s.model.proposal_shard is None
    s.rank, s.world = 2, 3                                             # the last rank of a ragged three-way split
    assert s.local_range() == (14, 20)
    assert [(h0, n) for _, h0, n in s.sample_chunks(x, None, chunk=4)] == [(14, 4), (18, 2)]
    with pytest.raises(ValueError):
        s.sample_local(x, None, lo=13, hi=15)
    # a rank that owns nothing (P = 1 over 3 ranks): one empty chunk of the right shape, and the model is never called
    s.model.num_proposals, calls = 1, s.model.calls
    assert s.local_range() == (1, 1)
    for chunk in (None, 4):
        got = list(s.sample_chunks(x, None, chunk=chunk))
        assert len(got) == 1 and got[0][1:] == (1, 0) and tuple(got[0][0].shape) == (1, 2, 0, 3, 4, 3)
    assert s.model.calls == calls and s.model.proposal_shard is None
    s.model.num_proposals = 20
    with pytest.raises(ValueError):
        list(s.sample_chunks(x, None, chunk=0))


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    import ctypes as C
    L = lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok = [p] * 8 + [4, 1, 1, 1, 1, 1, 0, p, 512, p, 512, None]       # B = T = P_r = F = J = 1: a 80-byte state

    def partials(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_hypothesis_partials(*a)

    assert partials(a8=0) == E_SHAPE and partials(a8=5) == E_SHAPE                     # num_parts
    for i in (9, 10, 11, 12, 13, 14):                                                   # B, T, P_r, F, J, h0 negative
        assert partials(**{f"a{i}": -1}) == E_ARG, i
    assert partials(a10=0) == E_ARG and partials(a12=0) == E_ARG and partials(a13=0) == E_ARG
    assert partials(a15=None) == E_ARG and partials(a16=79) == E_ARG                    # no state / a short one
    assert partials(a15=p + 4) == E_ARG                                                 # misaligned
    assert partials(a0=None) == E_ARG and partials(a7=None) == E_ARG                    # pred, part
    assert partials(a17=None) == -3 and partials(a18=39) == -3                          # PAFUSE_E_WORKSPACE
    assert b"hypothesis_partials" in L.pafuse_last_error()
    okc = [p, 1, 40, p, p, p, 1, 1, 1, 1, 1, None, p, p, p, p, None]

    def combine(**kw):
        a = list(okc)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_hypothesis_combine(*a)

    assert combine(a1=0) == E_ARG and combine(a7=0) == E_ARG and combine(a6=-1) == E_ARG
    assert combine(a2=39) == E_ARG and combine(a2=44) == E_ARG                          # stride: short / not a multiple of 8
    assert combine(a0=None) == E_ARG and combine(a3=None) == E_ARG
    assert combine(a12=None) == E_ARG                                                   # three maps of four
    assert combine(a12=None, a13=None, a14=None, a15=None) == E_ARG                     # nothing to write
    assert combine(a10=0) == E_ARG                                                      # P_total
    assert combine(a11=p) == E_ARG                                                      # merge over its operand + maps
    assert b"hypothesis_combine" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import harness, ops
    from pafuse_amd.evaluate import evaluate_accumulators_sharded
    z = torch.zeros
    with pytest.raises(ValueError):                                     # CPU tensors: no fallback
        ops.hypothesis_partials(z(1, 1, 2, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3, 2), z(1, 2, 3), z(9), z(3, dtype=torch.int32),
                                z(3, dtype=torch.int32), z(3, dtype=torch.int32), 1, 0)
    with pytest.raises(ValueError):
        ops.combine_partials(z(1, 100, dtype=torch.float64), z(1, 2, 3, 3), z(3, dtype=torch.int32), z(3, dtype=torch.int32),
                             (1, 1, 2, 3), 2)
    with pytest.raises(ValueError):
        evaluate_accumulators_sharded(None, None, 5, None, None, None, None, None)
    with pytest.raises(ValueError, match="gather"):
        harness.evaluate_sequence(None, None, None, None, None, [], [], gather="everything")
    with pytest.raises(ValueError, match="hypothesis_chunk"):
        harness.evaluate_sequence(None, None, None, None, None, [], [], hypothesis_chunk=5)
    with pytest.raises(ValueError, match="hypothesis_chunk"):
        harness.evaluate_sequence(None, None, None, None, None, [], [], gather="partials", hypothesis_chunk=0)


def test_options_reach_every_layer():
    from pafuse_amd import h3wb, harness
    for fn in (harness.evaluate_sequence, h3wb.evaluate):
        sig = inspect.signature(fn).parameters
        assert sig["gather"].default == "hypotheses" and sig["hypothesis_chunk"].default is None
    for script in ("evaluate_h3wb.py", "evaluate_synthetic.py"):
        src = open(os.path.join(ROOT, "examples", script)).read()
        assert "gather=a.gather, hypothesis_chunk=a.hypothesis_chunk" in src
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), "--help"], capture_output=True, text=True,
                             timeout=300, cwd=ROOT)
        assert out.returncode == 0 and "--gather {hypotheses,partials}" in out.stdout and "--hypothesis-chunk" in out.stdout


def test_torch_op_schemas():
    from pafuse_amd import torch_ops  # noqa: F401
    s = str(torch.ops.pafuse.hypothesis_partials.default._schema)
    assert "Tensor part, SymInt num_parts, SymInt h0" in s and s.endswith("-> Tensor")
    s = str(torch.ops.pafuse.combine_partials.default._schema)
    assert "Tensor pbroot, SymInt T, SymInt num_proposals" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        st = torch.ops.pafuse.hypothesis_partials(torch.empty(2, 3, 5, 4, 134, 3, device="cuda"), *[torch.empty(1, device="cuda")] * 7, 4, 0)
        assert st.dtype == torch.float64 and st.numel() == 5 * 2 * 3 * 4 * 134 + 5 * 3 * 5

"""Host-side bookkeeping of Protocol #2 from partial states (no GPU): state sizes against the library's own formula, the
bytes a rank receives with both protocols in one exchange, argument refusals of the C ABI and of the Python layers before
any device or model is touched, and the p2_gather option down to the examples."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

from pafuse_amd.parallel import shard_counts
from tests.conftest import ROOT

E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


def lib():
    import __graft_entry__ as g
    g.build()
    from pafuse_amd import _lib
    return _lib.load()


def test_state_size_formula_matches_the_library():
    from pafuse_amd import ops
    L = lib()
    for B, T, P_r, F, J in ((1, 10, 20, 27, 134), (64, 10, 20, 27, 134), (2, 2, 0, 5, 134), (0, 1, 3, 4, 17), (3, 2, 7, 243, 256)):
        want = 16 * B * T * F * J + 8 * P_r * T
        assert ops.procrustes_partials_bytes(B, T, P_r, F, J) == want == L.pafuse_procrustes_partials_bytes(B, T, P_r, F, J)
        assert want % 8 == 0
        assert L.pafuse_procrustes_partials_workspace_bytes(B, T, P_r, F, J) == 8 * B * T * P_r * F
        # no P in the head: the hypotheses enter through the tail only
        assert ops.procrustes_partials_bytes(B, T, P_r + 5, F, J) - want == 8 * 5 * T
        assert ops.procrustes_partials_bytes(B, T, 0, F, J) == ops.PROCRUSTES_HEAD_BYTES_PER_ELEMENT * B * T * F * J
    for bad in ((-1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0)):
        assert L.pafuse_procrustes_partials_bytes(*bad) == 0 and L.pafuse_procrustes_partials_workspace_bytes(*bad) == 0


def test_bytes_per_rank_at_the_evaluation_shape():
    """The reference's evaluation shape, P = 160 over 8 ranks, 64 clips per call: what every rank receives with Protocol #2
    switched on - all hypotheses (12 bytes per (b,t,h,f,j)) against world x (56 bytes per (b,t,f,j) + the two tails)."""
    from pafuse_amd import ops
    B, T, P, F, J, world, parts = 64, 10, 160, 27, 134, 8, 4
    n = B * T * F * J
    hypotheses = 12 * B * T * P * F * J
    assert hypotheses == 4_445_798_400
    pmax = max(shard_counts(P, world))
    per_rank = ops.partials_bytes(B, T, pmax, F, J, parts) + ops.procrustes_partials_bytes(B, T, pmax, F, J)
    assert per_rank == 56 * n + 8 * T * pmax * (1 + parts) + 8 * T * pmax == 129_678_720
    assert world * per_rank == 1_037_429_760 and hypotheses / (world * per_rank) > 4.2


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call"""
    import ctypes as C
    L = lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ok = [p] * 6 + [1, 1, 1, 1, 1, 0, p, 512, p, 512, None]          # B = T = P_r = F = J = 1: a 24-byte state

    def partials(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_procrustes_partials(*a)

    for i in (6, 7, 8, 9, 10, 11):                                     # B, T, P_r, F, J, h0 negative
        assert partials(**{f"a{i}": -1}) == E_ARG, i
    assert partials(a7=0) == E_ARG and partials(a9=0) == E_ARG and partials(a10=0) == E_ARG
    assert partials(a10=257) == E_SHAPE
    assert partials(a12=None) == E_ARG and partials(a13=23) == E_ARG    # no state / a short one
    assert partials(a12=p + 4) == E_ARG                                 # misaligned
    for i in range(6):
        assert partials(**{f"a{i}": None}) == E_ARG, i
    assert partials(a14=None) == E_WORKSPACE and partials(a15=7) == E_WORKSPACE
    assert b"procrustes_partials" in L.pafuse_last_error()
    okc = [p, 1, 16, p, 24, p, p, 1, 1, 1, 1, 1, None, p + 256, p + 264, p + 272, p + 280, None]

    def combine(**kw):
        a = list(okc)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.pafuse_procrustes_combine(*a)

    assert combine(a1=0) == E_ARG and combine(a8=0) == E_ARG and combine(a7=-1) == E_ARG and combine(a10=-1) == E_ARG
    assert combine(a11=0) == E_ARG                                      # P_total
    assert combine(a10=257) == E_SHAPE
    assert combine(a0=None) == E_ARG
    assert combine(a3=None) == E_ARG                                    # pagg wanted without sums
    assert combine(a5=None) == E_ARG and combine(a6=None) == E_ARG      # ... without gt / conn
    assert combine(a2=8) == E_ARG and combine(a2=20) == E_ARG           # stride: short / not a multiple of 8
    assert combine(a4=16) == E_ARG                                      # sums closer than 24 bytes per element
    assert combine(a13=None, a14=None, a15=None, a16=None) == E_ARG     # nothing to write
    assert combine(a1=2, a12=p + 16) == E_ARG                           # merged over the second operand
    assert b"procrustes_combine" in L.pafuse_last_error()


def test_python_layers_refuse_before_touching_the_device():
    from pafuse_amd import h3wb, harness, ops
    from pafuse_amd.evaluate import accumulate_procrustes, protocol2_accumulators_sharded
    z = torch.zeros
    i32 = dict(dtype=torch.int32)
    with pytest.raises(ValueError):                                     # CPU tensors: no fallback
        ops.procrustes_partials(z(1, 1, 2, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3, 2), z(1, 2, 3), z(9), z(3, **i32), 0)
    with pytest.raises(ValueError):
        ops.combine_procrustes(z(1, 100, dtype=torch.float64), (1, 1, 2, 3), 2, want=("jbest",))
    with pytest.raises(ValueError):
        ops.procrustes_partial_views(z(3, dtype=torch.float64), 1, 1, 2, 2, 3)
    from pafuse_amd import _lib
    with pytest.raises(_lib.PafuseError):
        accumulate_procrustes(None, z(1, 1, 2, 2, 3, 3), 0, z(1, 2, 3, 3), z(1, 2, 3, 2), z(1, 2, 3), z(9), None)
    with pytest.raises(ValueError):
        protocol2_accumulators_sharded(None, None, 5, None, None)
    # p2_gather="partials" needs p2=True and gather="partials": refused before the model (None here) is touched
    for kw in (dict(p2_gather="partials"), dict(p2=True, p2_gather="partials"), dict(gather="partials", p2_gather="partials"),
               dict(p2=True, gather="partials", p2_gather="everything")):
        with pytest.raises(ValueError, match="p2_gather"):
            harness.evaluate_sequence(None, None, None, None, None, [], [], **kw)
    for fn in (harness.evaluate_sequence, h3wb.evaluate):
        assert inspect.signature(fn).parameters["p2_gather"].default == "hypotheses"


def test_examples_pass_the_option_on():
    for script in ("evaluate_h3wb.py", "evaluate_synthetic.py"):
        src = open(os.path.join(ROOT, "examples", script)).read()
        assert "p2_gather=a.p2_gather" in src
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), "--help"], capture_output=True, text=True,
                             timeout=300, cwd=ROOT)
        assert out.returncode == 0 and "--p2-gather {hypotheses,partials}" in out.stdout
    src = open(os.path.join(ROOT, "examples", "evaluate_synthetic.py")).read()
    assert '"--p2"' in src and "p2=a.p2" in src


def test_torch_op_schemas():
    from pafuse_amd import torch_ops  # noqa: F401
    s = str(torch.ops.pafuse.procrustes_partials.default._schema)
    assert "Tensor conn, SymInt h0" in s and s.endswith("-> Tensor")
    s = str(torch.ops.pafuse.procrustes_combine.default._schema)
    assert "Tensor states, Tensor sums, Tensor gt, Tensor conn, SymInt T, SymInt num_proposals" in s and s.endswith("-> Tensor[]")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *shape, **kw: torch.empty(*shape, device="cuda", **kw)
        st = torch.ops.pafuse.procrustes_partials(e(2, 3, 5, 4, 134, 3), *[e(1)] * 5, 0)
        assert st.dtype == torch.float64 and st.numel() == 2 * 2 * 3 * 4 * 134 + 5 * 3
        maps = torch.ops.pafuse.procrustes_combine(e(2, st.numel(), dtype=torch.float64), e(2, 3 * 2 * 3 * 4 * 134, dtype=torch.float64),
                                                   e(2, 4, 134, 3), e(134, dtype=torch.int32), 3, 10)
        assert [tuple(m.shape) for m in maps] == [(2, 3, 4, 134)] * 4
        assert [m.dtype for m in maps] == [torch.float32] * 3 + [torch.int32]

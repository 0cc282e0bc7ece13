"""Protocol #2 from per-shard partial states on the device: pafuse_procrustes_partials / pafuse_procrustes_combine, the
ops and torch ops over them, evaluate.accumulate_procrustes / protocol2_accumulators_sharded and
evaluate_sequence(p2_gather="partials").

Criteria, strongest first.  (1) Across every way of cutting P into shards: jbest, jagg, pick and the concatenated psum are
bit-equal (the same kernel does the same per-pose arithmetic, min and first-minimum are grouping-free, psum has one fixed
order); pagg - the one output that adds per-shard fp64 sums - is equal or adjacent in fp32.  (2) Against
pafuse_procrustes_errors on all hypotheses: the pick is equal, the three maps equal or adjacent in fp32, psum within 1e-12
relative of pbest_sums added on the host in fp64.  (3) Against the fp64 truth of tests/test_p2_report.py: the bounds
test_kernel_vs_fp64_truth applies to the unsharded kernel (1e-6 m per map element, 1e-6 relative for the sums).

Measured on an MI355X (gfx950): elements adjacent rather than equal - 0 for jbest, jagg and pagg at every shape and split,
against pafuse_procrustes_errors and across the splits (the tests print the counts); at most 6.0e-8 m from the fp64 truth."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT
from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, run_sequence
from tests.test_hip_procrustes import P2_KEYS, random_inputs, small_conn
from tests.test_p2_report import G21_ATOL, conn_table, g21_case, p2_truth, same_nan_and_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
SHAPES = [(2, 2, 5, 3, 134), (2, 3, 3, 5, 17), (1, 2, 4, 4, 256), (1, 1, 1, 2, 134)]
MAPS = ("jbest", "pagg", "jagg")
EXACT = ("jbest", "jagg", "pick", "psum")


def bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def adjacent_count(a, b):
    """a, b fp32: asserts that every element is equal or adjacent (|a - b| <= |nextafter(b, inf) - b|, NaN matching NaN) and
    returns how many are adjacent rather than equal"""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    ok = ~torch.isnan(b)
    a, b = a[ok], b[ok]
    step = (torch.nextafter(b, torch.full_like(b, float("inf"))) - b).abs()
    d = (a - b).abs()
    assert bool((d <= step).all()), (d / step).max()
    return int((d > 0).sum())


def splits_of(P):
    s = {"one": (P,)}
    if P > 1:
        s["two"] = (P - P // 2, P // 2)          # P = 5: the ragged 3 + 2
        s["ones"] = (1,) * P
        s["running"] = tuple(min(2, P - lo) for lo in range(0, P, 2))
    return s


def on_device(z, conn):
    pred, gt, x2d, traj, cam = (t.contiguous().to(DEV) for t in z)
    return pred, gt, x2d, traj, cam, conn.contiguous().to(DEV)


def reduce_shards(z, conn, sizes, running=False):
    """Every shard of the cut `sizes` of P reduced on its own (a Protocol #2 state, and a mean-only pose state for the sums
    of the mean pose), then combined.  running=False: the states side by side, padded with NaN to the largest shard as an
    all-gather leaves them, one combine over W rows.  running=True: a running state merged in place chunk after chunk."""
    from pafuse_amd import ops
    pred, gt, x2d, traj, cam, conn = on_device(z, conn)
    B, T, P, F, J, _ = pred.shape
    assert sum(sizes) == P
    shape = (B, T, F, J)
    W, pmax = len(sizes), max(sizes)
    L = ops.procrustes_partials_bytes(B, T, pmax, F, J) // 8
    LP = ops.pose_partials_bytes(B, T, F, J) // 8
    states = torch.full((2 if running else W, L), float("nan"), device=DEV, dtype=torch.float64)
    poses = torch.full((2 if running else W, LP), float("nan"), device=DEV, dtype=torch.float64)
    psum, lo = [], 0
    for r, c in enumerate(sizes):
        row = (0 if r == 0 else 1) if running else r
        chunk = pred[:, :, lo:lo + c].contiguous()
        ops.procrustes_partials(chunk, gt, x2d, traj, cam, conn, lo, out=states[row])
        ops.pose_partials(chunk, conn, lo, out=poses[row])
        psum.append(ops.procrustes_partial_views(states[row], B, T, c, F, J)["psum"].clone())
        if running and r > 0:
            ops.combine_procrustes(states, shape, 1, merged=states[0], want=())
            ops.combine_poses(poses, shape, 1, merged=poses[0], want=())
        lo += c
    if running:
        states, poses = states[:1], poses[:1]
    out = ops.combine_procrustes(states, shape, P, sums=poses, gt=gt, conn=conn)
    out["psum"] = torch.cat(psum)
    return out


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs, connection table, the unsharded kernel's outputs and every split's, computed once per shape"""
    from pafuse_amd import ops
    B, T, P, F, J = shape
    z = random_inputs(B, T, P, F, J, seed=2000 + J + P)
    conn = conn_table(J) if J == 134 else small_conn(J, J)
    ref = ops.procrustes_errors(*on_device(z, conn))
    got = {name: reduce_shards(z, conn, sizes, running=name == "running") for name, sizes in splits_of(P).items()}
    return z, conn, ref, got


@pytest.mark.parametrize("shape", SHAPES)
def test_every_split_gives_the_same_bits(shape):
    _, _, _, got = case(shape)
    one = got["one"]
    for name, r in got.items():
        for k in EXACT:
            assert same_bits(r[k], one[k]), (name, k)
        print(f"{shape} {name}: pagg elements adjacent to the one-shard result: {adjacent_count(r['pagg'], one['pagg'])}")


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_unsharded_kernel(shape):
    B, T, P, F, J = shape
    _, _, ref, got = case(shape)
    want_psum = ref["pbest_sums"].double().cpu().permute(2, 1, 0, 3).reshape(P, T, -1).sum(-1)     # [P,T], fp64 on the host
    for name, r in got.items():
        assert torch.equal(r["pick"], ref["pick"]), name
        counts = {k: adjacent_count(r[k], ref[k]) for k in MAPS}
        print(f"{shape} {name}: adjacent rather than equal to pafuse_procrustes_errors: {counts}")
        assert torch.allclose(r["psum"].cpu(), want_psum, rtol=1e-12, atol=0), name


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_fp64_truth(shape):
    z, conn, _, got = case(shape)
    B, T, P, F, J = shape
    for name in ("one", "two", "running"):
        if name not in got:
            continue
        r = got[name]
        truth = p2_truth(*z, conn=conn, pick=r["pick"])          # J-Agg at the kernel's own pick
        for k, w in (("jbest", truth["jbest"]), ("pagg", truth["e_mean"]), ("jagg", truth["jagg"])):
            d = (r[k].cpu().double() - w).abs().max().item()
            print(f"{shape} {name} {k}: max |kernel - fp64| = {d:.3e} m")
            assert d <= 1e-6, (name, k, d)
        sums = truth["e"].permute(2, 1, 0, 3, 4).reshape(P, T, -1).sum(-1)
        assert torch.allclose(r["psum"].cpu(), sums, rtol=1e-6, atol=0), name


def test_pick_is_the_protocol1_partials_index():
    """one pick for both protocols: the index pafuse_hypothesis_partials keeps is the one the Protocol #2 states keep"""
    from pafuse_amd import ops
    from tests.test_hip_partials import tables
    z, conn, _, got = case(SHAPES[0])
    pred, gt, x2d, traj, cam, _ = on_device(z, conn)
    c, pbroot, part = tables()
    assert torch.equal(c.cpu(), conn)
    B, T, P, F, J = SHAPES[0]
    s = ops.hypothesis_partials(pred, gt, x2d, traj, cam, c, pbroot, part, 4, 0)
    assert torch.equal(ops.partials_views(s, B, T, P, F, J, 4)["idx"], got["two"]["pick"])
    # and the Protocol #1 state can stand in for the pose state as the source of the mean pose's sums
    st = ops.procrustes_partials(pred, gt, x2d, traj, cam, c, 0)
    m = ops.combine_procrustes(st.view(1, -1), (B, T, F, J), P, sums=s.view(1, -1), gt=gt, conn=c, want=("pagg",))
    assert same_bits(m["pagg"], got["one"]["pagg"])


def test_ties_across_a_shard_border_go_to_the_lower_index():
    """the same hypothesis in the last slot of shard 0 and the first of shard 1 (3 + 2): exact ties in e2 everywhere"""
    from pafuse_amd import ops
    B, T, P, F, J = 2, 2, 5, 3, 134
    z = list(random_inputs(B, T, P, F, J, seed=31))
    z[0][:, :, 3] = z[0][:, :, 2]
    conn = conn_table(J)
    r = reduce_shards(z, conn, (3, 2))
    ref = ops.procrustes_errors(*on_device(z, conn))
    assert torch.equal(r["pick"], ref["pick"]) and not bool((r["pick"] == 3).any()) and bool((r["pick"] == 2).any())
    assert same_bits(r["jagg"], ref["jagg"]) and same_bits(r["jbest"], ref["jbest"])


def test_degenerate_pose_in_the_middle_shard():
    """G21 `degenerate` (hypothesis 1 of step 0 is all zero) with that hypothesis a shard of its own in the middle: its NaN
    survives the combine in jbest and in its psum column, the other step is finite, and so is pagg"""
    z = g21_case("degenerate")
    P = z["pred_parts"].shape[2]
    assert P >= 3
    zz = (z["pred_parts"], z["gt_parts"], z["x2d"], z["traj"].reshape(*z["traj"].shape[:2], 3), z["cam"].reshape(9))
    r = reduce_shards(zz, conn_table(), (1, 1, P - 2))
    assert torch.isnan(r["jbest"][:, 0]).all() and torch.isfinite(r["jbest"][:, 1]).all()
    assert torch.isnan(r["psum"][1, 0]) and torch.isfinite(r["psum"][:, 1]).all()
    assert torch.isfinite(r["psum"][0, 0]) and torch.isfinite(r["psum"][2:, 0]).all()
    assert torch.isfinite(r["pagg"]).all()


def test_a_joint_without_a_finite_reprojection_error_has_no_pick():
    B, T, P, F, J = 2, 2, 5, 3, 134
    z = list(random_inputs(B, T, P, F, J, seed=33))
    z[2][:, 1, 50] = float("nan")
    for sizes, running in (((5,), False), ((3, 2), False), ((2, 2, 1), True)):
        r = reduce_shards(z, conn_table(J), sizes, running)
        assert bool((r["pick"][:, :, 1, 50] == -1).all()) and bool((r["jagg"][:, :, 1, 50] == 0).all())
        none = torch.zeros(B, T, F, J, dtype=torch.bool, device=DEV)
        none[:, :, 1, 50] = True
        assert bool((r["pick"][~none] >= 0).all())
        assert torch.isfinite(r["jbest"]).all() and torch.isfinite(r["pagg"]).all()


def test_empty_shards_in_first_and_middle_position_change_nothing():
    from pafuse_amd import ops
    z, conn, _, got = case(SHAPES[0])
    r = reduce_shards(z, conn, (0, 3, 0, 2))
    for k in EXACT + ("pagg",):
        assert same_bits(r[k], got["two"][k]), k
    pred, gt, x2d, traj, cam, c = on_device(z, conn)
    B, T, P, F, J = SHAPES[0]
    v = ops.procrustes_partial_views(ops.procrustes_partials(pred[:, :, :0].contiguous(), gt, x2d, traj, cam, c, 2), B, T, 0, F, J)
    assert bool(torch.isinf(v["jbest"]).all()) and bool(torch.isinf(v["e2"]).all()) and bool((v["sel"] == 0).all())
    assert bool((v["idx"] == -1).all()) and v["psum"].numel() == 0


def test_two_calls_same_bits():
    from pafuse_amd import ops
    z, conn, _, got = case(SHAPES[0])
    args = on_device(z, conn)
    a, b = ops.procrustes_partials(*args, 3), ops.procrustes_partials(*args, 3)
    assert same_bits(a, b)
    again = reduce_shards(z, conn, (3, 2))
    for k in EXACT + ("pagg",):
        assert same_bits(again[k], got["two"][k]), k


def sharded_accumulators(z, chunk):
    from pafuse_amd.evaluate import accumulate_partials, accumulate_procrustes, protocol2_accumulators_sharded
    pred, gt, x2d, traj, cam = (z[k].to(DEV) for k in ("pred_parts", "gt_parts", "x2d", "traj", "cam"))
    P = pred.shape[2]
    p1 = p2 = None
    for lo in range(0, P, chunk):
        p1 = accumulate_partials(p1, pred[:, :, lo:lo + chunk], lo, gt, x2d, traj, cam, dataset())
        p2 = accumulate_procrustes(p2, pred[:, :, lo:lo + chunk], lo, gt, x2d, traj, cam, dataset())
    return protocol2_accumulators_sharded(p2, p1, P, gt, dataset())


@pytest.mark.parametrize("name", ("random", "rigid", "degenerate"))
def test_g21_through_the_partial_states(name):
    z = g21_case(name)
    got = sharded_accumulators(z, 2)
    assert set(got) == set(P2_KEYS)
    for k in P2_KEYS:
        same_nan_and_close(got[k], z[k], 1e-6, G21_ATOL)


def test_refusals():
    from pafuse_amd import _lib, ops
    from pafuse_amd.evaluate import accumulate_procrustes
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV, dtype=torch.float64)
    p = buf.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    st, ws, o = p + (1 << 13), p + (1 << 14), [p + (1 << 15) + 1024 * k for k in range(4)]    # nothing written over an operand
    ok = [p] * 6 + [1, 1, 2, 1, 17, 0, st, 1 << 12, ws, 1 << 12, s]

    def partials(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.pafuse_procrustes_partials(*a)

    assert partials() == 0
    for i in range(6):
        assert partials(**{f"a{i}": None}) == E_ARG, i
    for i in range(6, 12):
        assert partials(**{f"a{i}": -1}) == E_ARG, i
    assert partials(a10=257) == E_SHAPE
    assert partials(a12=None) == E_ARG and partials(a13=16 * 17 + 8 * 2 - 1) == E_ARG and partials(a12=st + 4) == E_ARG
    assert partials(a14=None) == E_WORKSPACE and partials(a15=15) == E_WORKSPACE
    okc = [st, 1, 16 * 17, p, 24 * 17, p, p, 1, 1, 1, 17, 2, None, *o, s]

    def combine(**kw):
        a = list(okc)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.pafuse_procrustes_combine(*a)

    assert combine() == 0
    assert combine(a0=None) == E_ARG and combine(a1=0) == E_ARG and combine(a7=-1) == E_ARG and combine(a8=0) == E_ARG
    assert combine(a11=0) == E_ARG                                                       # P_total
    assert combine(a3=None) == E_ARG                                                     # pagg without sums
    assert combine(a5=None) == E_ARG and combine(a6=None) == E_ARG                       # pagg without gt / conn
    assert combine(a2=16 * 17 - 8) == E_ARG and combine(a4=24 * 17 - 8) == E_ARG         # rows closer than a state
    assert combine(a10=257) == E_SHAPE
    assert combine(a13=None, a14=None, a15=None, a16=None) == E_ARG                      # nothing to write
    assert combine(a1=2, a12=st + 16 * 17) == E_ARG                                      # merged over the second operand
    assert combine(a12=p) == E_ARG                                                       # merged over the sums
    assert combine(a14=None, a3=None, a12=st) == 0                                       # merged over the first: fine
    torch.cuda.synchronize()
    z = random_inputs(1, 1, 2, 2, 134, seed=3)
    pred, gt, x2d, traj, cam, conn = on_device(z, conn_table())
    with pytest.raises(ValueError):
        ops.procrustes_partials(pred, gt[:, :1].contiguous(), x2d, traj, cam, conn, 0)
    with pytest.raises(ValueError):
        ops.procrustes_partials(pred, gt, x2d, traj, cam, conn, -1)
    with pytest.raises(ValueError):
        ops.procrustes_partials(pred, gt, x2d, traj, cam, conn, 0, out=torch.empty(3, device=DEV, dtype=torch.float64))
    st = ops.procrustes_partials(pred, gt, x2d, traj, cam, conn, 0)
    with pytest.raises(ValueError):                                                      # pagg without the sums
        ops.combine_procrustes(st.view(1, -1), (1, 1, 2, 134), 2)
    with pytest.raises(ValueError):
        ops.combine_procrustes(st.view(1, -1), (1, 1, 2, 134), 0, want=("jbest",))
    state = accumulate_procrustes(None, pred, 0, gt, x2d, traj, cam, dataset())
    with pytest.raises(ValueError):                                                      # a gap: the next chunk starts at 2
        accumulate_procrustes(state, pred, 3, gt, x2d, traj, cam, dataset())


def test_torch_ops_are_the_ops_pair():
    from pafuse_amd import ops, torch_ops  # noqa: F401
    z, conn, _, got = case(SHAPES[0])
    pred, gt, x2d, traj, cam, c = on_device(z, conn)
    B, T, P, F, J = SHAPES[0]
    st = torch.ops.pafuse.procrustes_partials(pred, gt, x2d, traj, cam, c, 0)
    assert same_bits(st, ops.procrustes_partials(pred, gt, x2d, traj, cam, c, 0))
    poses = ops.pose_partials(pred, c, 0)
    jbest, pagg, jagg, pick = torch.ops.pafuse.procrustes_combine(st.view(1, -1), poses.view(1, -1), gt, c, T, P)
    for k, v in (("jbest", jbest), ("pagg", pagg), ("jagg", jagg), ("pick", pick)):
        assert same_bits(v, got["one"][k]), k


# ---------------------------------------------------------------------------------------------------- end to end
def scaled_adjacent(got, want, mult):
    """evaluate_sequence returns mult * v in fp32 (mult = clips x frames) for an accumulator v.  Two accumulators that are
    equal or adjacent in fp32, |a - b| <= u(v), give products |fl(mult a) - fl(mult b)| <= mult u(v) + one spacing of the
    product (half a spacing of rounding each): the adjacency criterion carried through that multiplication."""
    got, want = got.double(), want.double()
    v = (want / mult).float()
    u = (torch.nextafter(v, torch.full_like(v, float("inf"))) - v).abs().double()
    w32 = want.float()
    us = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).abs().double()
    d = (got - want).abs()
    assert bool((d <= mult * u + us).all()), (got, want)
    return d.max().item()


@pytest.fixture(scope="module")
def model():
    from __graft_entry__ import make_model
    return make_model(4, 1, depth=2)[0]


def test_evaluate_sequence_p2_from_partials(model):
    want, n = run_sequence(model, 27, p2=True, gather="partials", hypothesis_chunk=3, p2_gather="hypotheses")
    got, n2 = run_sequence(model, 27, p2=True, gather="partials", hypothesis_chunk=3, p2_gather="partials")
    assert n == n2 == 27 and len(got) == 18 and set(got) == set(want)
    for k in want:
        if not k.startswith("p2_") or k in ("p2_j_best", "p2_j_agg"):
            assert torch.equal(got[k], want[k]), k
        else:
            print(f"{k}: max |partials - hypotheses| of the sums = {scaled_adjacent(got[k], want[k], n):.3e}")
    for chunk in (1, None):
        other, _ = run_sequence(model, 27, p2=True, gather="partials", hypothesis_chunk=chunk, p2_gather="partials")
        for k in got:
            if k == "p2_p_agg":
                scaled_adjacent(other[k], got[k], n)
            else:
                assert torch.equal(other[k], got[k]), (chunk, k)


def test_chunked_p1_and_p2_evaluation_never_holds_the_full_tensor():
    """P = 160 in chunks of 5, every chunk generated when it is needed and folded into both states: the peak allocation of
    the whole Protocol #1 + #2 evaluation stays below the bytes of the [B,T,P,F,J,3] tensor alone"""
    from pafuse_amd.evaluate import (accumulate_partials, accumulate_procrustes, evaluate_accumulators_sharded,
                                     gather_partial_states, protocol2_accumulators_sharded)
    from tests.test_hip_partials import inputs
    B, T, P, F, J, chunk = 4, 2, 160, 27, 134, 5
    _, gt, x2d, traj, cam = inputs(B, T, 1, F, seed=9, special=False)
    full_bytes = B * T * P * F * J * 3 * 4
    g = torch.Generator(device=DEV).manual_seed(1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    p1 = p2 = None
    for lo in range(0, P, chunk):
        pred = gt[:, None, None] + torch.randn(B, T, chunk, F, J, 3, device=DEV, generator=g) * 0.05
        p1 = accumulate_partials(p1, pred, lo, gt, x2d, traj, cam, dataset())
        p2 = accumulate_procrustes(p2, pred, lo, gt, x2d, traj, cam, dataset())
        del pred
    gathered = gather_partial_states(p1, P, None, p2_state=p2)
    acc = evaluate_accumulators_sharded(None, None, P, gt, x2d, traj, cam, dataset(), state=gathered)
    acc.update(protocol2_accumulators_sharded(None, gathered, P, gt, dataset()))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak / 1e6:.2f} MB over the evaluation; the full tensor alone: {full_bytes / 1e6:.2f} MB")
    assert len(acc) == 18 and all(torch.isfinite(v).all() for v in acc.values())
    assert peak < full_bytes, (peak, full_bytes)


def test_two_rank_p2_partials_rehearsal_on_one_gpu(tmp_path):
    """Two real ranks sharing this box's one GPU over gloo (the states travel through the host), P = 5: a ragged 3 + 2
    split.  Both ranks must report what a single process computes with p2_gather="partials"."""
    import socket
    from __graft_entry__ import make_model
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "p2_partials_rank_worker.py"),
                                       str(tmp_path / f"rank{r}.pt")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    model, _ = make_model(5, 2, depth=2)
    want, n = run_sequence(model, 54, p2=True, gather="partials", p2_gather="partials")
    r0, r1 = (torch.load(str(tmp_path / f"rank{r}.pt")) for r in range(2))
    assert r0["world"] == 2 and r0["local"] == [0, 3] and r1["local"] == [3, 5] and r0["n"] == n and len(want) == 18
    for k in want:
        assert torch.equal(r0["sums"][k], r1["sums"][k]), k
    for k in ("p2_j_best", "p2_j_agg", "p2_p_best"):
        assert torch.equal(r0["sums"][k], want[k]), k
    print(f"p2_p_agg: max |two ranks - one process| of the sums = {scaled_adjacent(r0['sums']['p2_p_agg'], want['p2_p_agg'], n):.3e}")

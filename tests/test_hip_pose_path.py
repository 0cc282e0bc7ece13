"""J-Agg coherent in time on the device: pose_path_kernel (pafuse_pose_path), ops.pose_path, torch.ops.pafuse.pose_path,
evaluate.path_poses, infer_sequence(path_weight=...) and evaluate_frames(path_weight=...).

What is asserted and why it can be asserted.  The kernel and pafuse_amd.posepath perform the same IEEE operations in the
same order on the same operands - fp64 subtractions, products, sums and a correctly rounded sqrt with contraction off, a
first minimum under strict < in ascending h', a minimum (order-free: no NaN among its operands) subtracted per frame - so
idx is torch.equal and cost is the same double.  The one operand the statement cannot restate bit for bit is e2 itself:
reproj_error is an fp32 expression the device compiler may contract (rootfit.py says the same of the fitted pick), so the
statement is fed the e2 the DEVICE computes for every hypothesis on its own - pose_partials_kernel on one hypothesis at a
time, which calls the same reproj_error (`device_e2`).  A NaN e2 comes back from there as +inf; the statement treats every
non-finite e2 alike.  pick is a copy of a whole-body joint -> torch.equal to a gather of harness.wb_pose_from_parts.

Shapes: (2,2,5,3) at J = 134 - 536 lines, 134 workgroups; (1,1,70,9) at J = 134 - two hypotheses per lane, the second round
ragged (6 of 64 lanes); P = 64 and P = 65 at F = 2, J = 5 - the last size of one hypothesis per lane and the first of two,
five lines (a full workgroup and a ragged one); P = 130 and P = 256 at J = 5 - the kernel's forms with three and four hypotheses
per lane, the latter at the largest P it takes; P = F = 1.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_hip_partials import dataset, same_bits, sequence, tables
from tests.test_hip_pose_aggregate import BIG, DEV, J, e2e_inputs, gather_at, infer, inputs, whole_body

pytestmark = pytest.mark.gpu
WEIGHTS = (0.0, 0.5, 8.0)
WIDE = (1, 1, 70, 9)
C5 = [0, 0, 1, 1, 2]


def inputs5(P, F, seed):
    """the J = 5 inputs: a connection table of their own, no part structure"""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(1, 1, P, F, 5, 3, generator=g) * 0.25
    x2d = torch.rand(1, F, 5, 2, generator=g) * 2 - 1
    traj = torch.randn(1, F, 3, generator=g) * 0.1
    traj[..., 2] = 4.0
    z = {"pred": pred, "x2d": x2d, "traj": traj, "cam": sequence(1)[2]}
    return {k: v.contiguous().to(DEV) for k, v in z.items()}


def conn_of(z):
    return tables()[0] if z["pred"].shape[4] == J else torch.tensor(C5, dtype=torch.int32, device=DEV)


def wb_of(z):
    from pafuse_amd import rootfit
    if z["pred"].shape[4] == J:
        return whole_body(z["pred"])
    return torch.from_numpy(rootfit.whole_body(z["pred"].cpu().numpy(), C5))


def device_e2(z, conn, root):
    """e2 [B,T,P,F,J] of every hypothesis as the device computes it: pose_partials_kernel on ONE hypothesis keeps that
    hypothesis's e2 (+inf where it is not finite).  root: [B,F,3] or [B,T,P,F,3]."""
    from pafuse_amd import ops
    pred, x2d, cam = z["pred"], z["x2d"], z["cam"]
    B, T, P, F, Jn = pred.shape[:5]
    x2d_bt = x2d[:, None].expand(B, T, F, Jn, 2).reshape(B * T, F, Jn, 2).contiguous()
    out = []
    for h in range(P):
        one = pred[:, :, h].reshape(B * T, 1, 1, F, Jn, 3).contiguous()
        tr = (root[:, :, h] if root.dim() == 5 else root[:, None].expand(B, T, F, 3)).reshape(B * T, F, 3).contiguous()
        out.append(ops.pose_views(ops.pose_partials(one, conn, 0, x2d_bt, tr, cam), B * T, 1, F, Jn)["e2"].view(B, T, F, Jn).clone())
    return torch.stack(out, dim=2)


class Case:
    """one input with everything both sides need, computed once: the mean pose, fitted roots, device e2 per root kind"""

    def __init__(self, z, conf=None):
        from pafuse_amd import ops
        self.z, self.conn, self.conf = z, conn_of(z), conf
        pred = z["pred"]
        self.B, self.T, self.P, self.F, self.J = pred.shape[:5]
        self.shape = (self.B, self.T, self.F, self.J)
        self.wb = wb_of(z)
        self.tfit = torch.full((self.B, self.T, self.P, self.F, 3), 7.0, device=DEV)
        fit = ops.pose_partials_fit(pred, self.conn, 0, z["x2d"], z["cam"], conf=conf, tfit=self.tfit)
        self.fit_pick = ops.combine_poses(fit.view(1, -1), self.shape, self.P, no_pick_ok=True)
        full = ops.pose_partials(pred, self.conn, 0, z["x2d"], z["traj"], z["cam"])
        self.combine = ops.combine_poses(full.view(1, -1), self.shape, self.P, no_pick_ok=True)
        self.mean = self.combine["mean"]
        self.e2 = {}

    def root(self, kind):
        return self.z["traj"] if kind == "traj" else self.tfit

    def unary(self, kind, gated):
        """the statement's e2 [B,T,P,F,J] (numpy): the device's, +inf where conf is not > 0 when the call passes conf"""
        from pafuse_amd import posepath
        if kind not in self.e2:
            self.e2[kind] = device_e2(self.z, self.conn, self.root(kind)).cpu().numpy()
        return posepath.gate(self.e2[kind], self.conf.cpu().numpy()) if gated else self.e2[kind]

    def run(self, kind, weight, gated, mean=True, **kw):
        from pafuse_amd import ops
        z = self.z
        return ops.pose_path(z["pred"], self.conn, z["x2d"], self.root(kind), z["cam"], weight, conf=self.conf if gated else None,
                             mean=self.mean if mean else None, want=ops.PATH_OUTPUTS, **kw)

    def want(self, kind, weight, gated, mean=True):
        from pafuse_amd import posepath
        return posepath.pick(self.wb.numpy(), self.unary(kind, gated), weight, self.mean.cpu().numpy() if mean else None)


def fifth_off(B, F, Jn, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, F, Jn, generator=g) >= 0.2).float().to(DEV)


def adjacent64(a, b):
    """equal, or neighbours in fp64 (NaN with NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    near = np.abs(a - b) <= np.abs(np.nextafter(a, np.inf) - a)
    return bool((both_nan | near).all())


def compare(case, kind, weight, gated, mean=True):
    got, want = case.run(kind, weight, gated, mean), case.want(kind, weight, gated, mean)
    tag = (kind, weight, gated, mean)
    idx = got["idx"].cpu()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == case.shape
    assert torch.equal(idx, torch.from_numpy(want["idx"])), tag
    cost = got["cost"].cpu().numpy()
    same = np.array_equal(cost, want["cost"], equal_nan=True)
    print(f"{tag}: cost {'equal' if same else 'ADJACENT'}; lines without a path {int((idx[:, :, 0] < 0).sum())}")
    assert adjacent64(cost, want["cost"]), tag
    assert np.array_equal(got["pick"].cpu().numpy(), want["pick"], equal_nan=True), tag
    assert np.array_equal(got["e2"].cpu().numpy(), want["e2"]), tag
    alive = idx >= 0
    gathered = torch.gather(case.wb, 2, idx.clamp(min=0).long()[:, :, None, :, :, None].expand(*idx.shape[:2], 1, *idx.shape[2:], 3)).squeeze(2)
    assert torch.equal(got["pick"].cpu()[alive], gathered[alive]) and torch.isnan(got["pick"].cpu()[~alive]).all(), tag
    return got


@pytest.fixture(scope="module")
def big():
    return Case(inputs(*BIG, seed=21), conf=fifth_off(BIG[0], BIG[3], J, 22))


@pytest.fixture(scope="module")
def wide():
    return Case(inputs(*WIDE, seed=23), conf=fifth_off(WIDE[0], WIDE[3], J, 24))


@pytest.mark.parametrize("which", ["big", "wide"])
@pytest.mark.parametrize("kind,gated", [("traj", False), ("traj", True), ("fit", False), ("fit", True)])
def test_path_is_the_statement(big, wide, which, kind, gated):
    case = big if which == "big" else wide
    moved = 0
    for weight in WEIGHTS:
        got = compare(case, kind, weight, gated)
        if weight == 0.0:
            free = got["idx"]
        else:
            moved += int((got["idx"] != free).sum())
    assert moved > 0          # the penalty changed picks: the comparison is not the weight = 0 case three times
    if gated:                 # an unobserved (frame, joint) reports no error, and on a line with a path it still gets a hypothesis
        off = ~(case.conf > 0)[:, None].expand(case.shape)
        assert off.any() and (got["idx"][off] >= 0).any() and torch.isinf(got["e2"][off]).all()
        seen_line = (case.conf > 0).any(dim=1)[:, None].expand(case.B, case.T, case.J)      # [B,T,J]: some frame has a weight
        if kind == "traj":    # (with fitted roots a frame may also be unobserved for want of a fit)
            assert torch.equal((got["idx"] >= 0).all(dim=2), seen_line) and torch.equal((got["idx"] < 0).all(dim=2), ~seen_line)


@pytest.mark.parametrize("P,F", [(64, 2), (65, 2), (130, 2), (256, 3), (1, 1)])
def test_small_shapes(P, F):
    z = inputs5(P, F, 30 + P) if P > 1 else inputs(1, 1, 1, 1, seed=31)
    case = Case(z, conf=fifth_off(1, F, z["pred"].shape[4], 32))
    for weight in WEIGHTS:
        for gated in (False, True):
            compare(case, "traj", weight, gated)
        compare(case, "fit", weight, False, mean=False)


def test_zero_weight_is_the_pick_of_pose_combine(big, wide):
    for case in (big, wide):
        got = case.run("traj", 0.0, False)
        assert (case.combine["idx"] >= 0).all()
        assert torch.equal(got["idx"], case.combine["idx"]) and torch.equal(got["pick"], case.combine["pick"])
    # on the fitted roots with the weights: wherever pose_combine has a pick it is the path's; where it has none (a
    # weight not > 0: unobserved) the path still carries a hypothesis through
    got, fit = big.run("fit", 0.0, True), big.fit_pick
    has = fit["idx"] >= 0
    line_has = has.any(dim=2)[:, :, None].expand(big.shape)             # only a line without a single pick has no path
    assert has.any() and (~has).any() and torch.equal(got["idx"] >= 0, line_has)
    assert torch.equal(got["idx"][has], fit["idx"][has]) and torch.equal(got["pick"][has], fit["pick"][has])


def raw_call(case, weight, pred=None, x2d=None, mean="own", pad=5):
    """the C entry itself on buffers with guard rows: -> (pick, idx, e2, cost, guards intact?)"""
    from pafuse_amd import _lib, ops
    lib = _lib.load()
    z = case.z
    pred = z["pred"] if pred is None else pred
    x2d = z["x2d"] if x2d is None else x2d
    B, T, P, F, Jn = pred.shape[:5]
    n, lines = B * T * F * Jn, B * T * Jn
    mean = case.mean if isinstance(mean, str) else mean
    pick = torch.full((pad + n * 3 + pad,), 7.0, device=DEV)
    idx = torch.full((pad + n + pad,), 77, device=DEV, dtype=torch.int32)
    e2 = torch.full((pad + n + pad,), 7.0, device=DEV)
    cost = torch.full((pad + lines + pad,), 7.0, device=DEV, dtype=torch.float64)
    need = ops.pose_path_workspace_bytes(B, T, P, F, Jn)
    assert need == lib.pafuse_pose_path_workspace_bytes(B, T, P, F, Jn)
    ws = torch.full((8 + need + 64,), 0xAB, device=DEV, dtype=torch.uint8)
    _lib.check(lib.pafuse_pose_path(
        pred.data_ptr(), x2d.data_ptr(), z["traj"].data_ptr(), 0, z["cam"].data_ptr(), None, case.conn.data_ptr(),
        None if mean is None else mean.data_ptr(), float(weight), B, T, P, F, Jn, pick[pad:].data_ptr(), idx[pad:].data_ptr(),
        e2[pad:].data_ptr(), cost[pad:].data_ptr(), ws[8:].data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    used = lines * F * P
    intact = bool((pick[:pad] == 7).all() and (pick[-pad:] == 7).all() and (idx[:pad] == 77).all() and (idx[-pad:] == 77).all()
                  and (e2[:pad] == 7).all() and (e2[-pad:] == 7).all() and (cost[:pad] == 7).all() and (cost[-pad:] == 7).all()
                  and (ws[:8] == 0xAB).all() and (ws[8 + used:] == 0xAB).all())
    return (pick[pad:pad + n * 3].view(B, T, F, Jn, 3), idx[pad:pad + n].view(B, T, F, Jn), e2[pad:pad + n].view(B, T, F, Jn),
            cost[pad:pad + lines].view(B, T, Jn), intact)


def test_planted_nans_touch_only_their_lines_and_guards_stay(big):
    from pafuse_amd import posepath
    case, weight = big, 0.5
    B, T, P, F = BIG
    conn = case.conn.cpu()
    clean = raw_call(case, weight)
    assert clean[4]
    want = case.run("traj", weight, False)
    assert torch.equal(clean[1], want["idx"]) and torch.equal(clean[0], want["pick"]) and torch.equal(clean[2], want["e2"])
    assert torch.equal(clean[3], want["cost"])
    again = raw_call(case, weight)                                   # two calls give the same bits
    assert all(same_bits(a, b) for a, b in zip(clean[:4], again[:4]))
    b, t, h, f, j = 1, 0, 2, 1, 40
    hit_j = sorted({j} | {k for k in range(1, J) if int(conn[k]) == j})      # the joint and the joints that hang on it
    e2_clean = case.unary("traj", False)

    def statement(pred, e2, mean):
        return posepath.pick(whole_body(pred).numpy(), e2, weight, None if mean is None else mean.cpu().numpy())

    def same_elsewhere(out, lines_hit):
        keep = torch.ones(B, T, J, dtype=torch.bool, device=DEV)
        for (bb, tt, jj) in lines_hit:
            keep[bb, tt, jj] = False
        k4 = keep[:, :, None].expand(B, T, F, J)
        return (torch.equal(out[1][k4], clean[1][k4]) and torch.equal(out[0][k4], clean[0][k4]) and torch.equal(out[2][k4], clean[2][k4])
                and torch.equal(out[3][keep], clean[3][keep]))

    # (a) one hypothesis at one frame, absolute offsets (a mean over a NaN is a NaN): only that (h, f) leaves the line
    abs_clean = raw_call(case, weight, mean=None)
    pred = case.z["pred"].clone()
    pred[b, t, h, f, j] = float("nan")
    out = raw_call(case, weight, pred=pred, mean=None)
    lines_hit = [(b, t, k) for k in hit_j]
    keep = torch.ones(B, T, J, dtype=torch.bool, device=DEV)
    keep[b, t, hit_j] = False
    k4 = keep[:, :, None].expand(B, T, F, J)
    assert out[4] and torch.equal(out[1][k4], abs_clean[1][k4]) and torch.equal(out[0][k4], abs_clean[0][k4])
    assert (out[1][b, t, :, hit_j] >= 0).all() and (out[1][b, t, f, hit_j] != h).all()
    st = statement(pred, e2_clean, None)          # (the availability mask hides whatever e2 the NaN pose has)
    assert torch.equal(out[1].cpu(), torch.from_numpy(st["idx"])) and np.array_equal(out[3].cpu().numpy(), st["cost"], equal_nan=True)
    # (b) a NaN detection: the frame is unobserved for that joint in every t of its clip, and is carried through
    x2d = case.z["x2d"].clone()
    x2d[b, f, j, 1] = float("nan")
    out = raw_call(case, weight, x2d=x2d)
    assert out[4] and same_elsewhere(out, [(b, tt, j) for tt in range(T)])
    assert (out[1][b, :, :, j] >= 0).all() and torch.isinf(out[2][b, :, f, j]).all() and torch.isfinite(out[3][b, :, j]).all()
    e2_b = e2_clean.copy()
    e2_b[b, :, :, f, j] = np.inf
    st = statement(case.z["pred"], e2_b, case.mean)
    assert torch.equal(out[1].cpu(), torch.from_numpy(st["idx"])) and np.array_equal(out[3].cpu().numpy(), st["cost"])
    # (c) every hypothesis of one frame of one joint: its lines have no path
    pred = case.z["pred"].clone()
    pred[b, t, :, f, j] = float("nan")
    out = raw_call(case, weight, pred=pred, mean=None)
    assert out[4] and torch.equal(out[1][k4], abs_clean[1][k4]) and torch.equal(out[3][keep], abs_clean[3][keep])
    assert (out[1][b, t, :, hit_j] == -1).all() and torch.isnan(out[0][b, t, :, hit_j]).all()
    assert torch.isinf(out[2][b, t, :, hit_j]).all() and torch.isnan(out[3][b, t, hit_j]).all()


def test_refusals(big):
    from pafuse_amd import _lib, ops
    z, conn = big.z, big.conn
    args = lambda pred: (pred, conn, z["x2d"], z["traj"], z["cam"])
    with pytest.raises(_lib.PafuseError, match="256"):
        ops.pose_path(*args(torch.zeros(2, 2, 257, 3, J, 3, device=DEV)), 0.5)
    with pytest.raises(_lib.PafuseError, match="workspace"):
        ops.pose_path(*args(z["pred"]), 0.5, workspace=torch.empty(ops.pose_path_workspace_bytes(*BIG, J) - 8, device=DEV, dtype=torch.uint8))
    for weight in (-0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.PafuseError, match="weight"):
            ops.pose_path(*args(z["pred"]), weight)
    with pytest.raises(ValueError):
        ops.pose_path(*args(z["pred"]), 0.5, mean=big.mean[:1])
    empty = ops.pose_path(z["pred"][:0], conn, z["x2d"][:0], z["traj"][:0], z["cam"], 0.5)      # B == 0 launches nothing
    assert tuple(empty["idx"].shape) == (0, BIG[1], BIG[3], J)


def test_torch_op_and_path_poses(big):
    from pafuse_amd import evaluate, ops, torch_ops  # noqa: F401
    z = big.z
    want = big.run("traj", 0.5, False)
    got = torch.ops.pafuse.pose_path(z["pred"], big.conn, z["x2d"], z["traj"], z["cam"], 0.5, None, big.mean)
    assert all(torch.equal(g, want[k]) for g, k in zip(got, ops.PATH_OUTPUTS))
    out = evaluate.path_poses(z["pred"], dataset(), z["x2d"], z["cam"], 0.5, traj=z["traj"])
    assert torch.equal(out["idx"], want["idx"]) and torch.equal(out["pick"], want["pick"]) and torch.equal(out["cost"], want["cost"])
    assert torch.equal(out["mean"], big.mean)
    v = ops.pose_views(out["state"], *big.shape)
    full = ops.pose_views(ops.pose_partials(z["pred"], big.conn, 0, z["x2d"], z["traj"], z["cam"]), *big.shape)
    assert torch.equal(v["idx"], want["idx"]) and torch.equal(v["sel"], want["pick"]) and torch.equal(v["e2"], want["e2"])
    assert torch.equal(v["sum"], full["sum"])
    fit = evaluate.path_poses(z["pred"], dataset(), z["x2d"], z["cam"], 0.5, conf=big.conf, fit=True)
    want = big.run("fit", 0.5, True)
    assert torch.equal(fit["idx"], want["idx"]) and torch.equal(fit["pick"], want["pick"])


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model():
    from __graft_entry__ import make_model
    return make_model(5, 2, depth=2)[0]


def test_infer_sequence_with_a_path_weight(model):
    plain = infer(model, aggregate="reproj")
    pose, idx = infer(model, aggregate="reproj", path_weight=None)
    assert torch.equal(pose, plain[0]) and torch.equal(idx, plain[1])
    pose0, idx0 = infer(model, aggregate="reproj", path_weight=0.0)
    assert not pose0.is_cuda and torch.equal(idx0, plain[1]) and torch.equal(pose0, plain[0])
    wb = infer(model)
    pose8, idx8 = infer(model, aggregate="reproj", path_weight=8.0)
    assert idx8.dtype == torch.int32 and (idx8 >= 0).all() and not torch.equal(idx8, plain[1])
    assert torch.equal(pose8, gather_at(wb, idx8))
    both = infer(model, aggregate="reproj", path_weight=8.0, spread="std")
    assert torch.equal(both["pose"], pose8) and torch.equal(both["idx"], idx8)
    assert torch.equal(both["std"], infer(model, aggregate="reproj", spread="std")["std"])
    seq_2d, traj, cam = e2e_inputs()
    fit_plain = infer(model, aggregate="reproj_fit", cam=cam)
    fit0 = infer(model, aggregate="reproj_fit", cam=cam, path_weight=0.0)
    assert torch.equal(fit0[1], fit_plain[1]) and torch.equal(fit0[0], fit_plain[0])
    frames = infer(model, aggregate="reproj", path_weight=8.0, stride=27)        # the clips of cut_clips, folded into frames
    assert tuple(frames["pose"].shape) == (2, 30, J, 3) and torch.isfinite(frames["pose"]).all()
    # the clips start at 0 and 3: alone at the ends, and in the overlap every joint is one of the two paths' (the fold's rule)
    assert torch.equal(frames["pose"][:, :3], pose8[0][:, :3]) and torch.equal(frames["idx"][:, 27:], idx8[1][:, 24:])
    mid, a, b = frames["pose"][:, 3:27], pose8[0][:, 3:], pose8[1][:, :24]
    assert ((mid == a).all(dim=-1) | (mid == b).all(dim=-1)).all() and (frames["window"] >= 0).all()
    for kw in ({"hypothesis_chunk": 2}, {"stride": 9}, {"aggregate": "mean"}, {"aggregate": None}, {"path_weight": -1.0}):
        with pytest.raises(ValueError):
            infer(model, **{"aggregate": "reproj", "path_weight": 1.0, **kw})


def test_evaluate_frames_with_a_path_weight(model):
    from pafuse_amd import harness
    seq_2d, seq_3d, cam = sequence(30)

    def run(**kw):
        model.noise_fn, model.noise, model.noise_seed = None, "device", 3
        return harness.evaluate_frames(model, dataset(), seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, aggregate="reproj", **kw)

    plain, zero, held = run(), run(path_weight=0.0), run(path_weight=8.0)
    for k in plain[0]:
        assert torch.equal(zero[0][k], plain[0][k]) and torch.equal(zero[1][k], plain[1][k]), k
    accel = held[0]["accel"]
    print("accel sums (synthetic weights: the sizes mean nothing): per-frame pick", plain[0]["accel"].tolist(), "path, weight 8", accel.tolist())
    assert torch.isfinite(accel).all() and torch.equal(held[1]["accel"], plain[1]["accel"])
    with pytest.raises(ValueError):
        run(path_weight=1.0, stride=9)

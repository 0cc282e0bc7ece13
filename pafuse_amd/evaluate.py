"""Hypothesis aggregation + the 14 accumulators of the reference's evaluate() on the device
(main_h3wb.py:327-379).

``hypothesis_errors`` is one HIP kernel over the gathered predictions (whole-body poses from parts, 2-D
reprojection, per-joint J-Best / P-Agg / J-Agg and the part-re-centred variants); the remaining means over
(b, f, j) and the P-Best argmin are a handful of reductions over small tensors.  With ``p2=True`` a second kernel
(``procrustes_errors``) adds Protocol #2, the same four numbers after the reference's similarity alignment
(main_h3wb.py:381-395, common/loss.py:251-458).

``evaluate_accumulators_sharded`` gives the same 14 vectors without ever holding all P hypotheses: every shard of the
hypothesis axis (a rank's, or a chunk on one device) is reduced to a small state (``ops.hypothesis_partials``), states
are merged (``ops.combine_partials``), and ranks exchange states - not hypotheses - in one all-gather.  Protocol #2 has
two modes: by default it keeps the gather of ``pafuse_amd.parallel.gather_hypotheses`` and runs ``procrustes_errors`` on
all P hypotheses; opt-in (``accumulate_procrustes`` / ``protocol2_accumulators_sharded``) every shard is reduced to a
16-byte-per-(b,t,f,j) state (``ops.procrustes_partials``) that travels in the same all-gather, and only the mean pose of
P-Agg is aligned at combine time (``ops.combine_procrustes``), from the fp64 sums the Protocol #1 states already hold.

``accumulate_poses`` / ``aggregate_poses_sharded`` return the aggregates themselves - the P-Agg mean pose and the J-Agg
pose with its hypothesis index - by the same scheme and without a ground truth (``ops.pose_partials``, ``ops.combine_poses``).

``accumulate_spread`` keeps, by the same scheme again, the first and second moments of the whole-body hypotheses
(``ops.spread_partials``, ``ops.combine_spread``); ``aggregate_poses_sharded(spread_state=...)`` returns their per-joint
covariance and std beside the pose.

``frame_metrics`` scores a per-frame pose (and its camera-space root) against ground truth at the level of frames - position,
velocity, acceleration, root and part-based errors (``ops.frame_errors``; ``pafuse_amd.framemetrics`` states the arithmetic).

The four families share their host code: ``_operands`` checks and converts the arguments of every entry point,
``_RunningState.fold`` is the one running reduction (``PartialState``, ``Procrustes2State``, ``PoseState`` and ``SpreadState`` only declare
what each family keeps; every ``accumulate_*`` hands ``fold`` its partials op and its combine op), and ``_exchange`` is the
one collective (``gather_partial_states`` and ``aggregate_poses_sharded`` give it their pieces).
"""
import torch
import torch.distributed as dist

from . import _lib


def _tables(dataset, num_kps, device):
    conn = torch.zeros(num_kps, dtype=torch.int32)
    pbroot = torch.zeros(num_kps, dtype=torch.int32)
    connection = dict(dataset.parts_connection_indices)
    connection["body"] = 0                                   # common/utils.py:116
    for part, idx in dataset.parts_joint_indices.items():
        conn[idx] = connection[part]
        pbroot[idx] = dataset.root_indices[part]
    return conn.to(device), pbroot.to(device)


def _operands(pred_parts, gt_parts, inputs_2d, traj, cam, dataset, who, name="pred_parts", axis="P"):
    """The argument checks and conversions every evaluation entry point shares: -> contiguous fp32 pred, gt, x2d,
    traj [B,F,3], cam [9] on the device of the predictions, and the conn / pbroot index tables.  gt_parts=None (the pose
    aggregation has no ground truth): inputs_2d, traj and cam may then be absent too, all three; what is absent comes
    back as None."""
    if not pred_parts.is_cuda:
        raise _lib.PafuseError(f"{who} runs on the HIP device only (no CPU fallback)")
    dev = pred_parts.device
    if pred_parts.dim() != 6 or pred_parts.shape[-1] != 3:
        raise ValueError(f"{name} must be [B,T,{axis},F,J,3], got {tuple(pred_parts.shape)}")
    B, T, P, F, J, _ = pred_parts.shape
    given = [t is not None for t in (inputs_2d, traj, cam)]
    if gt_parts is None and any(given) and not all(given):
        raise ValueError(f"{who}: inputs_2d, traj and cam come together (none of them: mean-only)")
    reproj = gt_parts is not None or all(given)
    # the kernels index every operand by (B, F, J): check before launching
    if ((gt_parts is not None and tuple(gt_parts.shape) != (B, F, J, 3))
            or (reproj and (tuple(inputs_2d.shape) != (B, F, J, 2) or traj.numel() != B * F * 3 or cam.numel() < 9))):
        seen = (("gt", gt_parts), ("2d", inputs_2d), ("traj", traj), ("cam", cam))
        raise ValueError(f"{who}: operands do not match pred {tuple(pred_parts.shape)}: "
                         + ", ".join(f"{k} {tuple(t.shape)}" for k, t in seen if t is not None))
    if any(t is not None and t.device != dev for t in (gt_parts, inputs_2d, traj)):
        raise ValueError(f"{who}: all tensors must live on the device of {name}")
    covered = sorted(j for idx in dataset.parts_joint_indices.values() for j in idx)
    if covered != list(range(J)):
        raise ValueError("dataset.parts_joint_indices must cover every joint exactly once")
    conn, pbroot = _tables(dataset, J, dev)
    x2d = tr = cm = None
    if reproj:
        x2d, tr = inputs_2d.contiguous().float(), traj.reshape(B, F, 3).contiguous().float()
        cm = cam.reshape(-1)[:9].contiguous().float().to(dev)
    return (pred_parts.contiguous().float(), None if gt_parts is None else gt_parts.contiguous().float(), x2d, tr, cm,
            conn, pbroot)


def _per_t(x):
    """[B,T,F,J'] fp32 -> [T]: the mean over (b, f, j) in fp32"""
    return x.permute(1, 0, 2, 3).reshape(x.shape[1], -1).mean(dim=-1)


def _per_t64(x):
    """[B,T,F,J] fp32 -> [T]: the mean over (b, f, j) in fp64, rounded to fp32 once (Protocol #2, like the reference)"""
    return x.double().permute(1, 0, 2, 3).reshape(x.shape[1], -1).mean(dim=-1).float()


def evaluate_accumulators(pred_parts, gt_parts, inputs_2d, traj, cam, dataset, p2=False):
    """pred_parts [B,T,P,F,J,3], gt_parts [B,F,J,3] (part-centred, metres), inputs_2d [B,F,J,2], traj [B,F,1,3],
    cam [9] or [1,9] -> dict of the 14 per-step vectors [T] the reference accumulates per batch (same names as
    oracle.d3dp_oracle.evaluate_accumulators; multiply by 1000 for mm).  ``p2=True`` (the reference's ``ft2d.p2``)
    adds the four Protocol #2 vectors p2_j_best, p2_p_best, p2_p_agg, p2_j_agg; the 14 others are unchanged."""
    lib = _lib.load()
    pred, gt, x2d, tr, cm, conn, pbroot = _operands(pred_parts, gt_parts, inputs_2d, traj, cam, dataset, "evaluate_accumulators")
    dev = pred.device
    B, T, P, F, J, _ = pred.shape
    e3 = torch.empty(B, T, P, F, J, device=dev)
    epb = torch.empty_like(e3)
    jbest, pagg, jagg, paggpb = (torch.empty(B, T, F, J, device=dev) for _ in range(4))
    _lib.check(lib.pafuse_hypothesis_errors(
        pred.data_ptr(), gt.data_ptr(), x2d.data_ptr(), tr.data_ptr(), cm.data_ptr(), conn.data_ptr(),
        pbroot.data_ptr(), B, T, P, F, J, e3.data_ptr(), epb.data_ptr(), jbest.data_ptr(), pagg.data_ptr(),
        jagg.data_ptr(), paggpb.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))

    out = {"j_best": _per_t(jbest), "p_agg": _per_t(pagg), "j_agg": _per_t(jagg), "p_agg_pb": _per_t(paggpb)}
    out["p_best"] = e3.permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(dim=-1).min(dim=1).values
    eh = epb.permute(1, 2, 0, 3, 4)                          # t h b f n
    per_h = eh.reshape(T, P, -1).mean(dim=-1)
    best = per_h.argmin(dim=1)
    out["p_best_pb"] = per_h.min(dim=1).values
    for part, idx in dataset.parts_joint_indices.items():
        ph = eh[..., idx].reshape(T, P, -1).mean(dim=-1)
        out["p_best_pb_" + part] = ph.gather(1, best.view(-1, 1)).squeeze(1)
        out["p_agg_pb_" + part] = _per_t(paggpb[..., idx])
    if p2:
        out.update(_protocol2(pred, gt, x2d, tr, cm, conn))
    return out


def _protocol2(pred, gt, x2d, traj, cam, conn):
    """The four Protocol #2 vectors [T] from the per-joint / per-pose aligned errors: means over (b, f, j) in fp64,
    P-Best's minimum over h NaN-propagating like the reference's np.min; fp32 like the reference's accumulators."""
    from .ops import procrustes_errors
    B, T, P, F, J, _ = pred.shape
    r = procrustes_errors(pred, gt, x2d, traj, cam, conn, pick=False)

    per_h = r["pbest_sums"].permute(1, 2, 0, 3).reshape(T, P, -1).sum(dim=-1) / (B * F * J)
    return {"p2_j_best": _per_t64(r["jbest"]), "p2_p_best": per_h.min(dim=1).values.float(), "p2_p_agg": _per_t64(r["pagg"]),
            "p2_j_agg": _per_t64(r["jagg"])}


def protocol2_accumulators(pred_parts, gt_parts, inputs_2d, traj, cam, dataset):
    """the four Protocol #2 vectors of evaluate_accumulators(p2=True) alone, from all P hypotheses"""
    pred, gt, x2d, tr, cm, conn, _ = _operands(pred_parts, gt_parts, inputs_2d, traj, cam, dataset, "protocol2_accumulators")
    return _protocol2(pred, gt, x2d, tr, cm, conn)


def _part_table(dataset, num_kps, device):
    """part number of every joint, parts numbered in the order of dataset.parts_joint_indices"""
    part = torch.zeros(num_kps, dtype=torch.int32)
    for i, idx in enumerate(dataset.parts_joint_indices.values()):
        part[idx] = i
    return part.to(device)


class _RunningState:
    """The running reduction of the hypotheses one rank has seen so far, for any family of partial states: `slots` [2, L]
    float64 with the merged head in row 0 and the newest chunk's state in row 1, `tails` the per-hypothesis rows of every
    chunk [(h0, [P_c, ...] f64)] in ascending h0 (a family without a tail keeps none), `h0` / `count` the hypotheses
    [h0, h0 + count) folded so far."""

    def __init__(self, shape, device):
        self.shape, self.device = tuple(shape), device    # shape = (B, T, F, J)
        self.slots, self.tails = None, []
        self.h0, self.count, self.head_len = None, 0, None

    @property
    def head(self):
        return self.slots[0, :self.head_len]

    def tail(self):
        """the tails of all chunks so far as one [count, ...] tensor (None: nothing kept)"""
        return torch.cat([t for _, t in self.tails]) if self.tails else None

    def expect(self, who, shape, device, same=True):
        if self.shape != shape or self.device != device or not same:
            raise ValueError(f"{who}: the state holds {self.shape}, the chunk is {shape}")

    def fold(self, who, count, h0, head, tail, write, merge):
        """Fold the chunk of `count` hypotheses from `h0` on and return self.  `head`: float64 elements of the family's
        head; `tail`: shape of its per-hypothesis row behind the head (None: no tail); `write(row)` writes the chunk's
        state into the flat buffer `row`; `merge(slots)` merges slots[1] into slots[0] in place."""
        h0 = int(h0)
        if self.h0 is not None and h0 != self.h0 + self.count:
            raise ValueError(f"{who}: chunk starts at hypothesis {h0}, the state ends at {self.h0 + self.count}")
        L = head + (count * torch.Size(tail).numel() if tail is not None else 0)
        first = self.slots is None
        if first or self.slots.shape[1] < L:
            slots = torch.empty(2, L, device=self.device, dtype=torch.float64)
            if not first:
                slots[0, :head] = self.slots[0, :head]
            self.slots = slots
        row = self.slots[0 if first else 1]
        write(row)
        if tail is not None:
            self.tails.append((h0, row[head:L].view(count, *tail).clone()))
        if not first:     # running head <- running head (+) this chunk, in place (the combine kernels read each element before they write it)
            merge(self.slots)
        if self.h0 is None:
            self.h0 = h0
        self.count += count
        self.head_len = head
        return self


class PartialState(_RunningState):
    """The running reduction of the hypotheses one rank has seen so far: the merged head of the kernel's state (40 bytes
    per (b,t,f,j), independent of how many hypotheses went in) and the per-hypothesis sums of every chunk."""

    def __init__(self, shape, num_parts, device):
        super().__init__(shape, device)
        self.num_parts = num_parts

    hsums = property(lambda self: self.tails)             # [(h0, hsum [P_c,T,1+num_parts] f64)] in ascending h0


def accumulate_partials(state, pred_local, h0, gt_parts, inputs_2d, traj, cam, dataset):
    """Fold the hypotheses pred_local [B,T,P_c,F,J,3] = global [h0, h0 + P_c) into `state` (None: start one) and return
    it.  Chunks come in ascending h0 and follow each other without a gap; memory: the chunk, two 40-byte-per-(b,t,f,j)
    heads and [P_c,T,1+parts] doubles - never anything of size P."""
    from . import ops
    who = "accumulate_partials"
    pred, gt, x2d, tr, cm, conn, pbroot = _operands(pred_local, gt_parts, inputs_2d, traj, cam, dataset, who, name="pred_local",
                                                    axis="P_c")
    B, T, P_c, F, J, _ = pred.shape
    shape = (B, T, F, J)
    np_ = len(dataset.parts_joint_indices)
    if not 1 <= np_ <= _lib.MAX_PARTS:
        raise ValueError(f"the partial reductions keep per-part sums for 1 .. {_lib.MAX_PARTS} parts")
    part = _part_table(dataset, J, pred.device)
    if state is None:
        state = PartialState(shape, np_, pred.device)
    state.expect(who, shape, pred.device, state.num_parts == np_)
    return state.fold(
        who, P_c, h0, 5 * B * T * F * J, (T, 1 + np_),
        lambda row: ops.hypothesis_partials(pred, gt, x2d, tr, cm, conn, pbroot, part, np_, int(h0), out=row),
        lambda slots: ops.combine_partials(slots, gt, conn, pbroot, shape, 1, merged=slots[0], maps=False))


class GatheredStates:
    """What one exchange leaves on every rank: `states` [W, L] the ranks' Protocol #1 states in rank (= ascending-h0) order
    and `hsums` [P,T,1+parts] their concatenated per-hypothesis sums; with Protocol #2 states in the same exchange also
    `p2_states` [W, L2] (a column slice of the same buffer) and `psum` [P,T]."""

    def __init__(self, shape, num_parts, device, states, hsums, p2_states=None, psum=None):
        self.shape, self.num_parts, self.device = tuple(shape), num_parts, device
        self.states, self.hsums, self.p2_states, self.psum = states, hsums, p2_states, psum


def _exchange(pieces, h0, count, num_proposals, group, device):
    """The one collective of an evaluation.  `pieces`: [(head, tail)], reductions of the SAME hypotheses [h0, h0 + count)
    of this rank - head a flat float64 tensor, tail [count, ...] float64 per-hypothesis rows or None.  On the wire every
    rank sends one flat buffer: piece after piece, each its head and then its tail padded to the largest shard
    (parallel.shard_counts); ONE all_gather_into_tensor (through the host on a gloo group).  -> per piece (rows, tail):
    rows [W, >= head] the ranks' rows in rank (= ascending-h0) order - column slices of the one received buffer - and
    tail [P, ...] the un-padded tails concatenated in that order.  Without torch.distributed: the pieces as they are."""
    from .parallel import shard_counts, shard_range
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    if world == 1:
        if h0 != 0 or count != num_proposals:
            raise ValueError(f"the state holds hypotheses [{h0}, {h0 + count}) of {num_proposals}")
        return [(head.view(1, -1), tail) for head, tail in pieces]
    rank = dist.get_rank(group)
    lo, hi = shard_range(num_proposals, rank, world)
    if (h0, count) != (lo, hi - lo):
        raise ValueError(f"rank {rank} of {world} owns hypotheses [{lo}, {hi}) of {num_proposals}, its state holds "
                         f"[{h0}, {h0 + count})")
    counts = shard_counts(num_proposals, world)
    pmax = max(counts)
    spans, off = [], 0                                     # per piece: where its head begins, its tail begins, the piece ends
    for head, tail in pieces:
        end = off + head.numel() + (0 if tail is None else pmax * tail.shape[1:].numel())
        spans.append((off, off + head.numel(), end))
        off = end
    send = torch.zeros(off, device=device, dtype=torch.float64)
    for (head, tail), (a, b, _) in zip(pieces, spans):
        send[a:b] = head
        if tail is not None:
            send[b:b + tail.numel()] = tail.reshape(-1)
    if dist.get_backend(group) == "gloo":                  # rehearsal on a box with fewer GPUs than ranks
        send = send.cpu()
    recv = send.new_empty(world * send.numel())
    dist.all_gather_into_tensor(recv, send, group=group)
    recv = recv.view(world, -1).to(device)
    out = []
    for (_, tail), (a, b, end) in zip(pieces, spans):
        if tail is not None:
            tail = torch.cat([recv[r, b:end].view(pmax, *tail.shape[1:])[:counts[r]] for r in range(world)])
        out.append((recv[:, a:end], tail))
    return out


def gather_partial_states(state, num_proposals, group=None, p2_state=None):
    """ONE all-gather of equal-sized flat buffers (ragged shards are padded to the largest; through the host on a gloo
    group): per rank the Protocol #1 state and, when `p2_state` (a Procrustes2State over the same hypotheses) is given,
    the Protocol #2 state right behind it.  -> GatheredStates."""
    pieces = [(state.head, state.tail())]
    if p2_state is not None:
        if (p2_state.shape != state.shape or p2_state.device != state.device
                or (p2_state.h0, p2_state.count) != (state.h0, state.count)):
            raise ValueError(f"the Protocol #2 state holds [{p2_state.h0}, +{p2_state.count}) of {p2_state.shape}, the "
                             f"Protocol #1 state [{state.h0}, +{state.count}) of {state.shape}")
        pieces.append((p2_state.head, p2_state.tail()))
    got = _exchange(pieces, state.h0, state.count, num_proposals, group, state.device)
    return GatheredStates(state.shape, state.num_parts, state.device, *(x for piece in got for x in piece))


def evaluate_accumulators_sharded(pred_local, h0, num_proposals, gt_parts, inputs_2d, traj, cam, dataset, group=None,
                                  state=None):
    """evaluate_accumulators from partial reductions: pred_local [B,T,P_r,F,J,3] holds hypotheses [h0, h0 + P_r) of
    the `num_proposals` of the run - this rank's share (pafuse_amd.parallel.shard_range) or, with `state`, the last chunk
    of it (`state`: what accumulate_partials returned for the chunks before; pred_local=None evaluates the state as it
    is).  -> the same dict of 14 vectors [T].  With torch.distributed initialised the ranks exchange their states in
    ONE all_gather_into_tensor (through the host on a gloo group): 40 bytes per (b,t,f,j) plus 8 * (1 + parts) * T bytes
    per hypothesis of the largest shard, whatever P is.  j_best and j_agg are bit-equal to evaluate_accumulators;
    p_agg*, p_best* sum in fp64 where that kernel sums in fp32 (last-bit differences, closer to exact) and do not
    depend on how the hypotheses are cut.  Protocol #1 only.  `state` may also be the GatheredStates of an exchange that
    has already happened (gather_partial_states: the one all-gather can carry the Protocol #2 states too)."""
    from . import ops
    if pred_local is not None:
        state = accumulate_partials(state, pred_local, h0, gt_parts, inputs_2d, traj, cam, dataset)
    if state is None:
        raise ValueError("evaluate_accumulators_sharded: neither hypotheses nor a state")
    B, T, F, J = state.shape
    dev = state.device
    gathered = state if isinstance(state, GatheredStates) else gather_partial_states(state, int(num_proposals), group)
    states, hs = gathered.states, gathered.hsums
    P = hs.shape[0]
    if P != int(num_proposals):
        raise ValueError(f"the gathered states hold {P} hypotheses of {num_proposals}")
    conn, pbroot = _tables(dataset, J, dev)
    m = ops.combine_partials(states.contiguous(), gt_parts.contiguous().float(), conn, pbroot, (B, T, F, J), P)
    jbest, pagg, jagg, paggpb = m["jbest"], m["pagg"], m["jagg"], m["paggpb"]
    out = {"j_best": _per_t(jbest), "p_agg": _per_t(pagg), "j_agg": _per_t(jagg), "p_agg_pb": _per_t(paggpb)}
    hs = hs.permute(1, 0, 2)                                 # [T,P,1+parts] sums over (b,f,j), fp64
    out["p_best"] = (hs[..., 0] / (B * F * J)).float().min(dim=1).values
    per_h = (hs[..., 1:].sum(dim=-1) / (B * F * J)).float()
    best = per_h.argmin(dim=1)
    out["p_best_pb"] = per_h.min(dim=1).values
    for i, (part, idx) in enumerate(dataset.parts_joint_indices.items()):
        ph = (hs[..., 1 + i] / (B * F * len(idx))).float()
        out["p_best_pb_" + part] = ph.gather(1, best.view(-1, 1)).squeeze(1)
        out["p_agg_pb_" + part] = _per_t(paggpb[..., idx])
    return out


# ------------------------------------------------------------------------------- Protocol #2 from partial states
class Procrustes2State(_RunningState):
    """The running Protocol #2 reduction of the hypotheses one rank has seen so far: the merged head of the kernel's state
    (16 bytes per (b,t,f,j), ops.procrustes_partial_views) and the per-hypothesis sums psum [P_c,T] of every chunk."""

    psums = property(lambda self: self.tails)             # [(h0, psum [P_c,T] f64)] in ascending h0


def accumulate_procrustes(state, pred_local, h0, gt_parts, inputs_2d, traj, cam, dataset):
    """Fold the hypotheses pred_local [B,T,P_c,F,J,3] = global [h0, h0 + P_c) into the Protocol #2 state `state` (None:
    start one) and return it.  Chunks come in ascending h0 and follow each other without a gap; memory: the chunk, two
    16-byte-per-(b,t,f,j) heads, [B,T,P_c,F] doubles of workspace and [P_c,T] doubles - never anything of size P."""
    from . import ops
    who = "accumulate_procrustes"
    pred, gt, x2d, tr, cm, conn, _ = _operands(pred_local, gt_parts, inputs_2d, traj, cam, dataset, who, name="pred_local",
                                               axis="P_c")
    B, T, P_c, F, J, _ = pred.shape
    shape = (B, T, F, J)
    if state is None:
        state = Procrustes2State(shape, pred.device)
    state.expect(who, shape, pred.device)
    return state.fold(who, P_c, h0, 2 * B * T * F * J, (T,),
                      lambda row: ops.procrustes_partials(pred, gt, x2d, tr, cm, conn, int(h0), out=row),
                      lambda slots: ops.combine_procrustes(slots, shape, 1, merged=slots[0], want=()))


def protocol2_accumulators_sharded(state, p1, num_proposals, gt_parts, dataset, group=None):
    """The four Protocol #2 vectors [T] (p2_j_best, p2_p_best, p2_p_agg, p2_j_agg) without ever holding all P hypotheses.
    `state`: this rank's Procrustes2State (accumulate_procrustes over its hypotheses).  `p1`: this rank's PartialState
    over the same hypotheses - the two flat buffers are concatenated and travel in ONE all_gather_into_tensor (through the
    host on a gloo group), 56 bytes per (b,t,f,j) plus the per-hypothesis tails per rank - or the GatheredStates of that
    exchange (gather_partial_states(p1, P, group, p2_state=state)) when the Protocol #1 evaluation has made it already;
    `state` may then be None.  The mean pose of P-Agg comes from the fp64 sums heading the Protocol #1 states, added in rank
    order.  p2_j_best and p2_j_agg are bit-equal to protocol2_accumulators on all hypotheses; p2_p_agg (sums per shard
    first) and p2_p_best (per-hypothesis sums reduced in one fixed order) differ from it by fp64 roundings, and only
    p2_p_agg depends on how the hypotheses are cut."""
    from . import ops
    if p1 is None or (state is None and not isinstance(p1, GatheredStates)):
        raise ValueError("protocol2_accumulators_sharded: needs the Protocol #2 state and the Protocol #1 state of this rank, "
                         "or the GatheredStates of their exchange")
    gathered = p1 if isinstance(p1, GatheredStates) else gather_partial_states(p1, int(num_proposals), group, p2_state=state)
    if gathered.p2_states is None:
        raise ValueError("protocol2_accumulators_sharded: the gathered states carry no Protocol #2 states")
    B, T, F, J = gathered.shape
    dev = gathered.device
    P = int(num_proposals)
    if gathered.psum.shape[0] != P:
        raise ValueError(f"the gathered states hold {gathered.psum.shape[0]} hypotheses of {P}")
    if tuple(gt_parts.shape) != (B, F, J, 3) or gt_parts.device != dev:
        raise ValueError(f"protocol2_accumulators_sharded: gt_parts must be {(B, F, J, 3)} on {dev}")
    conn, _ = _tables(dataset, J, dev)
    m = ops.combine_procrustes(gathered.p2_states, (B, T, F, J), P, sums=gathered.states, gt=gt_parts.contiguous().float(),
                               conn=conn, want=("jbest", "pagg", "jagg"))
    per_h = (gathered.psum.permute(1, 0) / (B * F * J)).float()          # [T,P]
    return {"p2_j_best": _per_t64(m["jbest"]), "p2_p_best": per_h.min(dim=1).values, "p2_p_agg": _per_t64(m["pagg"]),
            "p2_j_agg": _per_t64(m["jagg"])}


# ------------------------------------------------------------------------------------------- aggregates as poses
class PoseState(_RunningState):
    """The running pose reduction of the hypotheses one rank has seen so far: 44 bytes per (b,t,f,j) (ops.pose_views),
    independent of how many hypotheses went in.  `reproj`: the chunks came with 2-D input, trajectory and camera, so the
    state holds J-Agg candidates; a mean-only state has none."""

    def __init__(self, shape, device, reproj, fit=False):
        super().__init__(shape, device)
        self.reproj = bool(reproj)
        self.fit = bool(fit)      # the roots were fitted (accumulate_poses(fit=True)): a state without any pick is legitimate


def accumulate_poses(state, pred_local, h0, dataset, inputs_2d=None, traj=None, cam=None, *, fit=False, conf=None, tfit=None):
    """Fold the part-centred hypotheses pred_local [B,T,P_c,F,J,3] = global [h0, h0 + P_c) into the pose state `state`
    (None: start one) and return it.  inputs_2d [B,F,J,2], traj [B,F,3] (or [B,F,1,3]) and cam [9] together keep the J-Agg
    candidate; none of them: mean-only.  Chunks come in ascending h0 without a gap.  Memory: the chunk and two 44-byte
    per-(b,t,f,j) states - never anything of size P.

    fit=True: J-Agg WITHOUT a trajectory - inputs_2d and cam, no traj; the root of every (hypothesis, frame) is fitted on
    the device (ops.pose_partials_fit, pafuse_amd.rootfit) with the weights conf [B,F,J] (None: all 1; not > 0: the joint
    takes no part and gets no pick).  tfit: a contiguous fp32 [B,T,P_c,F,3] device tensor that receives this chunk's roots
    (NaN: no fit).  The state is a PoseState(reproj=True) and combines like any other."""
    from . import ops
    who = "accumulate_poses"
    if fit:
        return _accumulate_poses_fit(state, pred_local, h0, dataset, inputs_2d, traj, cam, conf, tfit)
    if conf is not None or tfit is not None:
        raise ValueError("accumulate_poses: conf and tfit belong to fit=True")
    pred, _, x2d, tr, cm, conn, _ = _operands(pred_local, None, inputs_2d, traj, cam, dataset, who, name="pred_local", axis="P_c")
    B, T, P_c, F, J, _ = pred.shape
    shape = (B, T, F, J)
    reproj = x2d is not None
    if state is None:
        state = PoseState(shape, pred.device, reproj)
    state.expect(who, shape, pred.device)
    if state.reproj != reproj:
        raise ValueError("accumulate_poses: a state is either mean-only or keeps candidates, for all of its chunks")
    if state.fit:
        raise ValueError("accumulate_poses: a state is fitted for all of its chunks or for none")
    return state.fold(who, P_c, h0, ops.pose_partials_bytes(B, T, F, J) // 8, None,
                      lambda row: ops.pose_partials(pred, conn, int(h0), x2d, tr, cm, out=row),
                      lambda slots: ops.combine_poses(slots, shape, 1, merged=slots[0], want=()))


def _accumulate_poses_fit(state, pred_local, h0, dataset, inputs_2d, traj, cam, conf, tfit):
    from . import ops
    who = "accumulate_poses"
    if inputs_2d is None or cam is None or traj is not None:
        raise ValueError("accumulate_poses: fit=True takes inputs_2d and cam and no traj (the root is what it fits)")
    pred, _, _, _, _, conn, _ = _operands(pred_local, None, None, None, None, dataset, who, name="pred_local", axis="P_c")
    B, T, P_c, F, J, _ = pred.shape
    shape = (B, T, F, J)
    dev = pred.device
    if (tuple(inputs_2d.shape) != (B, F, J, 2) or cam.numel() < 9 or (conf is not None and tuple(conf.shape) != (B, F, J))
            or (tfit is not None and tuple(tfit.shape) != (B, T, P_c, F, 3))):
        raise ValueError(f"{who}: operands do not match pred {tuple(pred.shape)}: 2d {tuple(inputs_2d.shape)}, cam "
                         f"{tuple(cam.shape)}" + ("" if conf is None else f", conf {tuple(conf.shape)}")
                         + ("" if tfit is None else f", tfit {tuple(tfit.shape)}"))
    if inputs_2d.device != dev or (conf is not None and conf.device != dev) or (tfit is not None and tfit.device != dev):
        raise ValueError(f"{who}: all tensors must live on the device of pred_local")
    x2d = inputs_2d.contiguous().float()
    cm = cam.reshape(-1)[:9].contiguous().float().to(dev)
    cf = None if conf is None else conf.contiguous().float()
    if state is None:
        state = PoseState(shape, dev, True, fit=True)
    state.expect(who, shape, dev)
    if not (state.reproj and state.fit):
        raise ValueError("accumulate_poses: a state is fitted for all of its chunks or for none")
    return state.fold(who, P_c, h0, ops.pose_partials_bytes(B, T, F, J) // 8, None,
                      lambda row: ops.pose_partials_fit(pred, conn, int(h0), x2d, cm, conf=cf, out=row, tfit=tfit),
                      lambda slots: ops.combine_poses(slots, shape, 1, merged=slots[0], want=()))


def aggregate_poses_sharded(pred_local, h0, num_proposals, dataset, inputs_2d=None, traj=None, cam=None, group=None,
                            state=None, want=None, spread_state=None, merged=False):
    """The aggregates as poses without ever holding all P hypotheses: pred_local [B,T,P_r,F,J,3] holds the part-centred
    hypotheses [h0, h0 + P_r) of the `num_proposals` of the run - this rank's share (pafuse_amd.parallel.shard_range) or,
    with `state`, the last chunk of it (`state`: what accumulate_poses returned for the chunks before; pred_local=None
    aggregates the state as it is).  -> dict "mean" [B,T,F,J,3] (P-Agg, the mean whole-body pose) and, when the state
    keeps candidates, "pick" [B,T,F,J,3] and "idx" [B,T,F,J] int32 (J-Agg: per joint the hypothesis whose reprojection is
    closest to the 2-D input - the hypothesis the evaluation kernels pick).  `want`: a subset of those names.  With
    torch.distributed initialised the ranks exchange their states in ONE all_gather_into_tensor (through the host on a
    gloo group): 44 bytes per (b,t,f,j), whatever P is.  pick and idx do not depend on how the hypotheses are cut; the
    mean adds the shards' fp64 sums in shard order.

    `spread_state` (what accumulate_spread returned for the same hypotheses; a last chunk pred_local is folded into it
    too) adds the names "cov" [B,T,F,J,6] and "std" [B,T,F,J] (ops.combine_spread); its 72 bytes per (b,t,f,j) ride in
    the same all-gather behind the pose state.  `state` may then be None: the spread state holds the sums, so "mean" comes
    from it - the same bits, there is no pick.  Without a spread state nothing changes, and "cov" / "std" are refused.

    merged=True also hands back the state of the UNION across ranks and chunks, as the same combine call writes it: "state"
    (the flat pose state, ops.pose_views; absent without a pose state), "spread_state" (ops.spread_views; with a spread
    state) and "shape" = (B,T,F,J) - what accumulate_frames folds into per-frame states.  `want` may then be empty.  Every
    rank holds the same merged states."""
    from . import ops
    if pred_local is not None:
        if state is not None or spread_state is None or inputs_2d is not None:
            state = accumulate_poses(state, pred_local, h0, dataset, inputs_2d, traj, cam)
        if spread_state is not None:
            spread_state = accumulate_spread(spread_state, pred_local, h0, dataset)
    if state is None and spread_state is None:
        raise ValueError("aggregate_poses_sharded: neither hypotheses nor a state")
    reproj = state is not None and state.reproj
    if want is None:
        want = (("mean", "pick", "idx") if reproj else ("mean",)) + (("cov", "std") if spread_state is not None else ())
    want = tuple(want)
    if not reproj and ("pick" in want or "idx" in want):
        raise ValueError("aggregate_poses_sharded: a mean-only state has no pick (give inputs_2d, traj and cam)")
    if spread_state is None and ("cov" in want or "std" in want):
        raise ValueError('aggregate_poses_sharded: "cov" and "std" need a spread state (accumulate_spread)')
    P = int(num_proposals)
    union = lambda like: torch.empty(like.shape[1], device=like.device, dtype=torch.float64) if merged else None
    if spread_state is None:
        (states, _), = _exchange([(state.head, None)], state.h0, state.count, P, group, state.device)
        states = states.contiguous()
        into = union(states)
        out = ops.combine_poses(states, state.shape, P, merged=into, want=want, no_pick_ok=state.fit)
        if merged:
            out.update(state=into, shape=state.shape)
        return out
    first = spread_state if state is None else state
    if state is not None and (state.shape != spread_state.shape or state.device != spread_state.device
                              or (state.h0, state.count) != (spread_state.h0, spread_state.count)):
        raise ValueError(f"the spread state holds [{spread_state.h0}, +{spread_state.count}) of {spread_state.shape}, the "
                         f"pose state [{state.h0}, +{state.count}) of {state.shape}")
    pieces = ([] if state is None else [(state.head, None)]) + [(spread_state.head, None)]
    got = _exchange(pieces, first.h0, first.count, P, group, first.device)      # one all-gather for both families
    from_pose = tuple(k for k in want if k in ("pick", "idx") or (k == "mean" and state is not None))
    from_spread = tuple(k for k in want if k not in from_pose)
    out = {}
    if from_pose or (merged and state is not None):
        states = got[0][0].contiguous()
        into = union(states)
        out.update(ops.combine_poses(states, first.shape, P, merged=into, want=from_pose,
                                     no_pick_ok=state is not None and state.fit))
        if merged:
            out["state"] = into
    if from_spread or merged:
        states = got[-1][0].contiguous()
        into = union(states)
        out.update(ops.combine_spread(states, first.shape, merged=into, want=from_spread))
        if merged:
            out.update(spread_state=into, shape=first.shape)
    return out


def path_poses(pred_parts, dataset, inputs_2d, cam, weight, traj=None, conf=None, fit=False):
    """J-Agg coherent in time (ops.pose_path; pafuse_amd.posepath states it): per line (b, t, j) a path through ALL P
    hypotheses pred_parts [B,T,P,F,J,3] (part-centred, P <= 256, F <= 256) that minimises the reprojection error plus
    `weight` times the distance the joint jumps relative to the mean pose.  The recursion needs every hypothesis of a clip
    at once: there is no per-shard state, so callers gather the hypotheses first.

    It runs the existing pose pair first - accumulate_poses on inputs_2d [B,F,J,2], traj [B,F,3] and cam [9], or with
    fit=True on inputs_2d, cam and conf [B,F,J], which also gives the root of every (hypothesis, frame) - for the mean pose,
    then the path kernel against that mean.  conf (None: all observed) marks a (frame, joint) whose weight is not > 0 as
    unobserved: the path crosses it by smoothness alone.  weight >= 0 in normalised screen length per metre (cam[0] / depth:
    a jump costs what it projects to); 0 gives the per-frame pick.

    -> dict "pick" [B,T,F,J,3], "idx" [B,T,F,J] int32 (NaN / -1 on a line without a path), "mean" [B,T,F,J,3],
    "cost" [B,T,J] float64, "state" the flat pose state of the P hypotheses whose (e2, idx, sel) hold the path's pick (sum
    as the pair wrote it) and "shape" = (B,T,F,J): what accumulate_frames folds like any merged state."""
    from . import ops
    if fit:
        if traj is not None:
            raise ValueError("path_poses: fit=True takes no traj (the root is what it fits)")
        B, T, P, F = pred_parts.shape[:4]
        root = torch.empty(B, T, P, F, 3, device=pred_parts.device)
        state = accumulate_poses(None, pred_parts, 0, dataset, inputs_2d, None, cam, fit=True, conf=conf, tfit=root)
    else:
        if traj is None:
            raise ValueError("path_poses: a trajectory [B,F,3], or fit=True")
        state = accumulate_poses(None, pred_parts, 0, dataset, inputs_2d, traj, cam)
    if fit:   # (accumulate_poses checked inputs_2d, cam and conf against pred)
        pred, _, _, _, _, conn, _ = _operands(pred_parts, None, None, None, None, dataset, "path_poses")
        x2d, tr, cm = inputs_2d.contiguous().float(), None, cam.reshape(-1)[:9].contiguous().float().to(pred.device)
    else:
        pred, _, x2d, tr, cm, conn, _ = _operands(pred_parts, None, inputs_2d, traj, cam, dataset, "path_poses")
    B, T, F, J = shape = state.shape
    merged = torch.empty(state.head.numel(), device=pred.device, dtype=torch.float64)
    mean = ops.combine_poses(state.head.unsqueeze(0), shape, pred.shape[2], merged=merged, want=("mean",))["mean"]
    cf = None if conf is None else conf.contiguous().float()
    out = ops.pose_path(pred, conn, x2d, root if fit else tr, cm, weight, conf=cf, mean=mean, want=("pick", "idx", "e2", "cost"))
    views = ops.pose_views(merged, B, T, F, J)
    views["e2"].copy_(out["e2"]), views["idx"].copy_(out["idx"]), views["sel"].copy_(out["pick"])
    return {"pick": out["pick"], "idx": out["idx"], "mean": mean, "cost": out["cost"], "state": merged, "shape": shape}


# ------------------------------------------------------------------------------------- spread of the hypotheses
class SpreadState(_RunningState):
    """The running first and second moments of the hypotheses one rank has seen so far: 72 bytes per (b,t,f,j) and a
    count (ops.spread_views), independent of how many hypotheses went in."""


def accumulate_spread(state, pred_local, h0, dataset):
    """Fold the part-centred hypotheses pred_local [B,T,P_c,F,J,3] = global [h0, h0 + P_c) into the spread state `state`
    (None: start one) and return it.  Chunks come in ascending h0 without a gap.  Memory: the chunk and two
    72-byte-per-(b,t,f,j) states - never anything of size P."""
    from . import ops
    who = "accumulate_spread"
    pred, _, _, _, _, conn, _ = _operands(pred_local, None, None, None, None, dataset, who, name="pred_local", axis="P_c")
    B, T, P_c, F, J, _ = pred.shape
    shape = (B, T, F, J)
    if state is None:
        state = SpreadState(shape, pred.device)
    state.expect(who, shape, pred.device)
    return state.fold(who, P_c, h0, ops.spread_partials_bytes(B, T, F, J) // 8, None,
                      lambda row: ops.spread_partials(pred, conn, int(h0), out=row),
                      lambda slots: ops.combine_spread(slots, shape, merged=slots[0], want=()))


# ----------------------------------------------------------------- overlapping windows pooled into one pose per frame
class FrameState:
    """The running per-frame reduction of the windows folded so far (ops.frame_views): `pose` the frame pose state - 48
    bytes per (t,n,j) and a count per frame - or None, `spread` the frame spread state (72 bytes) or None, `windows` the
    number of windows folded (the global index of the next batch's first window)."""

    def __init__(self, N, T, J, device):
        self.N, self.T, self.J, self.device = int(N), int(T), int(J), device
        self.pose = self.spread = None
        self.windows = 0


def accumulate_frames(frames, merged, starts, valid, N, num_proposals):
    """Fold one batch of windows into the per-frame state `frames` (None: start one over N video frames) and return it.
    `merged`: what aggregate_poses_sharded(..., merged=True) returned for the batch - the pose and / or spread state of
    the union of the `num_proposals` hypotheses across ranks and chunks, so the fold happens behind the cross-rank combine,
    every rank holds the same frame state and no collective is added.  starts, valid: the batch's rows of
    pafuse_amd.windows.window_starts (host integers); batches come in ascending window order.  Memory: the frame states
    and the batch's merged states - nothing grows with the number of windows.  ops.finish_frames writes the result."""
    from . import ops
    if "shape" not in merged or not ("state" in merged or "spread_state" in merged):
        raise ValueError("accumulate_frames: needs the merged states of aggregate_poses_sharded(..., merged=True)")
    B, T, F, J = merged["shape"]
    first = merged["state"] if "state" in merged else merged["spread_state"]
    if frames is None:
        frames = FrameState(N, T, J, first.device)
        if "state" in merged:
            frames.pose = ops.frame_state(N, T, J, first.device)
        if "spread_state" in merged:
            frames.spread = ops.frame_state(N, T, J, first.device, spread=True)
    if (frames.N, frames.T, frames.J, frames.device) != (int(N), T, J, first.device):
        raise ValueError(f"accumulate_frames: the frame state holds {(frames.N, frames.T, frames.J)}, the batch {(int(N), T, J)}")
    if (frames.pose is None) != ("state" not in merged) or (frames.spread is None) != ("spread_state" not in merged):
        raise ValueError("accumulate_frames: every batch brings the states the first one brought")
    if frames.pose is not None:
        ops.fold_windows(frames.pose, N, merged["state"], (B, T, F, J), starts, valid, frames.windows, num_proposals)
    if frames.spread is not None:
        ops.fold_spread_windows(frames.spread, N, merged["spread_state"], (B, T, F, J), starts, valid)
    frames.windows += B
    return frames


def path_frames(pred_windows, dataset, seq_2d, cam, weight, starts, valid, N, frames, traj=None, conf=None, fit=False):
    """The J-Agg path of a whole VIDEO (ops.frames_path; pafuse_amd.posepath.frames_path states it): per line (t, j) one path
    along the N video frames whose candidates at frame n are ALL P hypotheses of ALL windows that cover n - it crosses clip
    seams and pooled windows.  pred_windows [W,T,P,F,J,3] part-centred, the hypotheses of every window of the video, on the
    device (memory grows with the length of the video: W*T*P*F*J*3*4 bytes, plus one back-pointer byte per (t, j, n,
    candidate)); starts, valid: the rows of pafuse_amd.windows.window_starts (host integers, the whole video); seq_2d
    [N,J,2] the detections of the video; cam [9]; `frames` the FrameState already folded from the pose states of the same
    windows (accumulate_frames): its pooled mean (ops.finish_frames) is what the offsets are taken against.  traj [N,3]
    the root trajectory of the video, or fit=True (no traj): the root of every (window, hypothesis, frame) as
    ops.pose_partials_fit fits it (tfit) under the weights conf [N,J].  conf (None: all observed) also marks a (frame,
    joint) whose weight is not > 0 as unobserved: the path crosses it by smoothness alone.  At most 256 candidates per frame
    (P times the windows covering one frame).
    -> dict "pick" [T,N,J,3], "idx" and "window" [T,N,J] int32 (NaN / -1 / -1 at every frame of a line without a path:
    one frame without an available candidate removes the joint's path for the video), "e2" [T,N,J], "cost" [T,J] float64
    and "mean" [T,N,J,3]."""
    from . import ops
    who = "path_frames"
    pred, _, _, _, _, conn, _ = _operands(pred_windows, None, None, None, None, dataset, who, name="pred_windows")
    W, T, P, F, J, _ = pred.shape
    dev, N = pred.device, int(N)
    if frames is None or frames.pose is None or (frames.N, frames.T, frames.J) != (N, T, J) or frames.windows != W:
        raise ValueError(f"{who}: `frames` must hold the folded pose states of the same {W} windows over N = {N} frames")
    if cam is None or tuple(seq_2d.shape) != (N, J, 2) or (conf is not None and tuple(conf.shape) != (N, J)):
        raise ValueError(f"{who}: seq_2d [N,J,2] = {(N, J, 2)}, cam [9] and conf [N,J] or None")
    x2d = seq_2d.to(dev).contiguous().float()
    cm = torch.as_tensor(cam, dtype=torch.float32).reshape(-1)[:9].contiguous().to(dev)
    cf = None if conf is None else conf.to(dev).contiguous().float()
    if fit:
        if traj is not None:
            raise ValueError(f"{who}: fit=True takes no traj (the root is what it fits)")
        first = torch.as_tensor(starts, dtype=torch.long, device=dev)
        at = (first[:, None] + torch.arange(F, device=dev)[None]).clamp(max=N - 1)     # [W,F]: a short video repeats its last frame
        root = torch.empty(W, T, P, F, 3, device=dev)
        ops.pose_partials_fit(pred, conn, 0, x2d[at].contiguous(), cm, conf=None if cf is None else cf[at].contiguous(), tfit=root)
    else:
        if traj is None or tuple(traj.shape) != (N, 3):
            raise ValueError(f"{who}: a trajectory [N,3] with N = {N}, or fit=True")
        root = traj.to(dev).contiguous().float()
    mean = ops.finish_frames(N, T, J, frame=frames.pose, want=("mean",))["mean"]
    out = ops.frames_path(pred, conn, x2d, root, cm, weight, starts, valid, conf=cf, mean=mean, want=ops.FRAMES_PATH_OUTPUTS)
    out["mean"] = mean
    return out


# ----------------------------------------------------------------- the per-frame pose scored against ground truth
FRAME_METRICS = ("mpjpe", "mpjve", "accel", "root", "root_vel", "abs_mpjpe")   # ops.FRAME_ERROR_SLOTS; then one slot per part


def frame_metric_names(dataset):
    """the slots of ops.frame_errors by name: FRAME_METRICS, then "mpjpe_pb_<part>" in the order of dataset.parts_joint_indices"""
    return FRAME_METRICS + tuple("mpjpe_pb_" + part for part in dataset.parts_joint_indices)


def frame_metrics(pose, gt_wb, dataset, traj=None, gt_root=None, p2=False, per_frame=False):
    """The per-frame output scored against ground truth on the device (ops.frame_errors; pafuse_amd.framemetrics states the
    arithmetic): pose [T,N,J,3] whole-body and root-relative - infer_sequence(stride=)["pose"] or stitch_poses, NaN where there
    is no pose - gt_wb [N,J,3] likewise (joint 0 at 0), traj [T,N,3] the fitted or smoothed root with gt_root [N,3] (both or
    neither).  Returns a dict of ``(sum [T] float64, count [T] int64)`` on the device, a metric being sum / count in metres:

      mpjpe       the position error per joint             mpjve   its first difference along the frames (m/frame)
      accel       its second difference (m/frame^2)        mpjpe_pb_<part>, mpjpe_pb   the part re-centred error, per part and all
      root, root_vel, abs_mpjpe   (with traj) the root error, its first difference, and the camera-space error per joint

    A joint takes part in a frame only where its pose and its gt are finite; the counts say how many did.  ``p2=True`` adds
    ``p_mpjpe``: the error after the reference's similarity alignment of every frame's pose to its gt - the existing
    ops.procrustes_errors on the pose as a single hypothesis (its P-Agg of one hypothesis is the aligned error of the pose
    itself) - summed as the mean over the joints of every frame in which all joints are finite; its count is the number of
    frames scored.  It needs joint 0 at the origin in both (wb_joint pins it there) and J <= 256.  ``per_frame=True`` adds
    ``"err"`` [T,N,K] float64 and ``"cnt"`` [T,N,K] int32, the maps per frame in the order of frame_metric_names."""
    from . import ops
    if not (isinstance(pose, torch.Tensor) and pose.is_cuda):
        raise _lib.PafuseError("frame_metrics runs on the HIP device only (no CPU fallback)")
    if pose.dim() != 4 or pose.shape[-1] != 3:
        raise ValueError(f"pose must be [T,N,J,3], got {tuple(pose.shape)}")
    T, N, J, _ = pose.shape
    if tuple(gt_wb.shape) != (N, J, 3):
        raise ValueError(f"gt_wb must be [N,J,3] = {(N, J, 3)}, got {tuple(gt_wb.shape)}")
    if (traj is None) != (gt_root is None):
        raise ValueError("traj and gt_root come together (or neither)")
    covered = sorted(j for idx in dataset.parts_joint_indices.values() for j in idx)
    if covered != list(range(J)):
        raise ValueError("dataset.parts_joint_indices must cover every joint exactly once")
    dev = pose.device
    _, pbroot = _tables(dataset, J, dev)
    part = _part_table(dataset, J, dev)
    names = frame_metric_names(dataset)
    num_parts = len(names) - len(FRAME_METRICS)
    pose, gt = pose.contiguous().float(), gt_wb.to(dev).contiguous().float()
    if traj is not None:
        traj, gt_root = traj.to(dev).contiguous().float(), gt_root.to(dev).reshape(N, 3).contiguous().float()
    m = ops.frame_errors(pose, gt, pbroot, part, num_parts, traj=traj, gt_root=gt_root, per_frame=per_frame)
    out = {k: (m["sums"][:, i], m["counts"][:, i]) for i, k in enumerate(names) if traj is not None or k not in ("root", "root_vel", "abs_mpjpe")}
    out["mpjpe_pb"] = (m["sums"][:, 6:].sum(dim=1), m["counts"][:, 6:].sum(dim=1))
    if p2:
        scored = (torch.isfinite(pose).all(dim=-1) & torch.isfinite(gt).all(dim=-1)[None]).all(dim=-1)     # [T,N]
        cam = torch.tensor([1.0, 1.0, 0, 0, 0, 0, 0, 0, 0], device=dev)
        root = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(1, N, 3).contiguous()   # x2d, traj, cam: only outputs ignored here see them
        r = ops.procrustes_errors(pose.view(1, T, 1, N, J, 3), gt.view(1, N, J, 3), torch.zeros(1, N, J, 2, device=dev), root, cam,
                                  torch.zeros(J, dtype=torch.int32, device=dev), pick=False)
        per_frame_mean = r["pagg"][0].double().sum(dim=-1) / J                                                # [T,N]
        out["p_mpjpe"] = (torch.where(scored, per_frame_mean, torch.zeros_like(per_frame_mean)).sum(dim=1), scored.sum(dim=1))
    if per_frame:
        out["err"], out["cnt"] = m["err"], m["cnt"]
    return out

"""Hypothesis-axis sharding across the GPUs of one node (one process per GPU, torch.distributed over RCCL).

DDIM trajectories are independent per hypothesis (nothing in common/diffusionpose.py:192-316 or
common/mixste.py reduces over P), so rank r owns hypotheses [lo, hi) for all clips and all steps, weights are
replicated, and the only exchange is ONE all-gather of the per-rank predictions before the aggregation
protocols (J-Agg & co.) - 8.7 MB per rank at P_local=20, T=10, B=1.  With the model's default noise source
('torch') every rank draws the full-P noise tensor from the same seed and keeps its slice, so the sharded run reproduces
the single-GPU hypotheses - at the price of the full-P noise on every rank.  With ``model.noise = "device"`` a rank's
kernels generate exactly its own hypotheses of the stream (pafuse_amd/noise.py): nothing is drawn and thrown away, and
the hypotheses of a (noise_seed, noise_call) are the same for every world size and every chunking.

Evaluation does not need the hypotheses themselves on every rank: ``ShardedSampler.sample_local`` /
``sample_chunks`` hand out the local ones, and ``pafuse_amd.evaluate.evaluate_accumulators_sharded`` exchanges their
partial reductions instead (40 bytes per (b,t,f,j), whatever P is).
"""
import torch
import torch.distributed as dist


def shard_range(num_proposals, rank, world):
    """Contiguous, balanced [lo, hi) of the hypothesis axis for `rank` (first P % world ranks get one more)."""
    base, rem = divmod(num_proposals, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_counts(num_proposals, world):
    return [shard_range(num_proposals, r, world)[1] - shard_range(num_proposals, r, world)[0] for r in range(world)]


def gather_hypotheses(local, num_proposals=None, group=None):
    """all-gather per-rank predictions [B,T,P_r,F,J,3] along the hypothesis axis -> [B,T,P,F,J,3] on every rank.

    ONE collective (RCCL all-gather into a [world, B, T, P_max, F, J, 3] buffer, rank-major as the collective lays it
    out) and ONE pass over the result (the permute that moves the rank axis next to the hypothesis axis).  Ragged shards
    (P % world != 0) are padded to the largest shard for the collective and dropped in that same pass."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local
    if local.is_cuda and dist.get_backend(group) == "gloo":          # rehearsal on a box with fewer GPUs than ranks
        return gather_hypotheses(local.cpu(), num_proposals, group).to(local.device)
    world = dist.get_world_size(group)
    B, T, P_r = local.shape[:3]
    tail = tuple(local.shape[3:])
    if num_proposals is None:
        sizes = [torch.zeros(1, dtype=torch.int64, device=local.device) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor([P_r], dtype=torch.int64, device=local.device), group=group)
        counts = [int(s.item()) for s in sizes]
    else:
        counts = shard_counts(num_proposals, world)
    pmax = max(counts)
    send = local.contiguous()
    if P_r < pmax:
        send = torch.cat([send, send.new_zeros((B, T, pmax - P_r) + tail)], dim=2)
    recv = send.new_empty((world * B, T, pmax) + tail)               # concatenation along dim 0 = rank-major
    dist.all_gather_into_tensor(recv, send, group=group)
    recv = recv.view((world, B, T, pmax) + tail)
    out = recv.permute(1, 2, 0, 3, *range(4, recv.dim()))            # [B, T, world, P_max, ...] view
    if all(c == pmax for c in counts):
        return out.reshape((B, T, world * pmax) + tail)              # the one copy
    keep = torch.tensor([r * pmax + i for r in range(world) for i in range(counts[r])], device=local.device)
    return out.reshape((B, T, world * pmax) + tail).index_select(2, keep)


def rank_census(p_local, group=None):
    """What the collective layer actually sees: every rank contributes (rank, local hypothesis count) to one all-gather.
    Returns {"ranks_seen": n, "P_local": [count of rank 0, 1, ...]} on every rank (bench.py prints it, so a run whose
    ranks did not all join the job cannot report an N-GPU number)."""
    if not (dist.is_available() and dist.is_initialized()):
        return {"ranks_seen": 1, "P_local": [int(p_local)]}
    world = dist.get_world_size(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    mine = torch.tensor([dist.get_rank(group), int(p_local)], dtype=torch.int64, device=dev)
    got = torch.empty(world * 2, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(got, mine, group=group)
    got = got.view(world, 2).cpu()
    ranks = sorted(set(int(r) for r in got[:, 0]))
    by_rank = {int(r): int(c) for r, c in got.tolist()}
    return {"ranks_seen": len(ranks), "P_local": [by_rank[r] for r in ranks]}


class ShardedSampler:
    """Wrap a pafuse_amd.D3DP so that ``__call__`` runs this rank's hypotheses and returns the gathered result."""

    def __init__(self, model, group=None):
        self.model, self.group = model, group
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1

    def local_range(self):
        """[lo, hi): the hypotheses of the run this rank samples"""
        return shard_range(self.model.num_proposals, self.rank, self.world)

    def sample_local(self, input_2d, input_3d, input_2d_flip=None, lo=None, hi=None):
        """This rank's hypotheses WITHOUT the gather -> (pred_local [B,T,P_r,F,J,3], h0, P_r).  `lo`, `hi` (global
        indices inside local_range()) narrow the call to a part of them.  Noise source 'torch': the model draws the
        full-P noise and keeps the slice, so the values are those of the unsharded run provided the generator stands
        where that run would find it (sample_chunks sees to that between chunks).  Noise source 'device': the values are
        those of the unsharded run of the same (noise_seed, noise_call); a call of its own advances noise_call once, on
        every rank, the ranks without a hypothesis included."""
        m = self.model
        a, b = self.local_range()
        lo, hi = a if lo is None else int(lo), b if hi is None else int(hi)
        if not a <= lo <= hi <= b:
            raise ValueError(f"hypotheses [{lo}, {hi}) are not inside this rank's [{a}, {b})")
        if hi == lo:      # nothing to sample (a rank beyond the P-th when P < world): no model call, an empty tensor of the right shape
            T = len(m.ddim_steps())
            if getattr(m, "noise", "torch") == "device":
                m.advance_noise_call()
            return input_2d.new_zeros((input_2d.shape[0], T, 0, m.frames, m.num_kps, 3), dtype=torch.float32), lo, 0
        m.proposal_shard = (lo, hi)
        try:
            local = m(input_2d, input_3d, input_2d_flip=input_2d_flip)
        finally:
            m.proposal_shard = None
        return local, lo, hi - lo

    def sample_chunks(self, input_2d, input_3d, input_2d_flip=None, chunk=None):
        """Generator over this rank's hypotheses in chunks of at most `chunk` (None: all at once), ascending:
        yields (pred_chunk, h0, P_c).  Every chunk's call starts from the same state of the device's random generator,
        so each draws the full-P noise of the unsharded run and keeps its own slice; after the last chunk the generator
        stands where one unsharded call leaves it.  The workspace and the predictions follow the chunk, not P; the noise
        does not: every chunk draws and stacks the full-P tensor of every draw.
        With ``model.noise = "device"`` there is no generator to rewind and no noise tensor: all chunks run under one
        noise_call, which advances once after the last chunk (identically on every rank, whatever its share), and peak
        memory does follow the chunk."""
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"hypothesis chunk must be a positive count, got {chunk}")
        a, b = self.local_range()
        step = max(b - a, 1) if chunk is None else int(chunk)
        dev = input_2d.device
        m = self.model
        seeded = getattr(m, "noise", "torch") == "device"
        rng = torch.cuda.get_rng_state(dev) if (input_2d.is_cuda and b - a > step and not seeded) else None
        if seeded:
            held, call = m._hold_noise_call, m.noise_call        # the chunks are ONE logical call: one noise_call for all
        lo = a
        try:
            while True:
                hi = min(b, lo + step)
                if rng is not None and lo > a:
                    torch.cuda.set_rng_state(rng, dev)
                if seeded:
                    m._hold_noise_call, m.noise_call = True, call
                try:
                    item = self.sample_local(input_2d, input_3d, input_2d_flip, lo, hi)
                finally:
                    if seeded:
                        m._hold_noise_call = held                # (not while the consumer runs between two chunks)
                yield item
                lo = hi
                if lo >= b:
                    return
        finally:
            if seeded:
                m._hold_noise_call, m.noise_call = held, call
                m.advance_noise_call()

    def __call__(self, input_2d, input_3d, input_2d_flip=None):
        m = self.model
        m.proposal_shard = shard_range(m.num_proposals, self.rank, self.world) if self.world > 1 else None
        try:
            local = m(input_2d, input_3d, input_2d_flip=input_2d_flip)
        finally:
            m.proposal_shard = None
        return gather_hypotheses(local, m.num_proposals, self.group)

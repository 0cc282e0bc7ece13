"""The "device" noise source on the GPU: noise_fill_kernel / finalize_seeded_kernel (pafuse_noise_fill,
pafuse_d3dp_sample_seeded) behind pafuse_amd.D3DP.noise = "device".

What is asserted and why it can be asserted:
  * kernel vs host: both sides evaluate the same fp64 expression with log / sincospi / sin / cos good to ~1e-15 relative and
    round once to fp32, so a value may differ only where the fp64 result lies within ~1e-15 relative of an fp32 rounding
    boundary: probability ~3e-8 per value.  Every value within one fp32 ulp, and at most 1e-5 of them not bit-equal (a
    condition on the two math libraries, not a measurement: the expected count on 2e6 values is below one).
  * loop equivalence: the seeded loop runs the arithmetic of the buffer loop on the same normals -> torch.equal with the
    'torch' source fed the noise_fill tensors of the same key through noise_fn.
  * invariance: a value of the stream is a function of (seed, call, k, b, p, f, j) only -> torch.equal between the one-call
    run and any sharding / hypothesis chunking / clip chunking of it.
  * memory: a shard call allocates what an unsharded call of that many hypotheses allocates (1 MB of slack for allocator
    rounding); the 'torch' source of the same shard call holds at least one full-P draw more than its slice:
    B * (P - P_local) * F * J * 3 * 4 bytes = 2 * 140 * 27 * 134 * 3 * 4 = 12.2 MB (a lower bound: the slices are views
    of the full draws).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from pafuse_amd import noise as host
from pafuse_amd.parallel import ShardedSampler, shard_range
from tests.golden import golden_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda"
J = 134


def _ordered(x):
    """fp32 bit patterns as integers that are monotone in the value (ulp distance = difference)"""
    i = x.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _inject(model, seed, call):
    """the 'torch' source fed the noise_fill tensors of (seed, call) through the existing buffer path"""
    from pafuse_amd import ops
    model.noise = "torch"
    model.noise_fn = lambda k, shape, device: ops.noise_fill(ops.noise_key(seed, call, 0, 0, device), k, *shape[:4])


def _device(model, seed, call=0):
    model.noise_fn = None
    model.noise = "device"
    model.noise_seed = seed
    model.noise_call = call


def _inputs(B):
    x2d, x2f = gu.synthetic_inputs_2d(B=B)
    return x2d.to(DEV), x2f.to(DEV)


def test_noise_fill_matches_the_host_statement():
    from pafuse_amd import ops
    cases = [dict(seed=123, call=9, k=4, b0=3, p0=150, B=4, P=16, F=27),
             dict(seed=2 ** 32 - 1, call=2 ** 32 - 1, k=10, b0=1, p0=13, B=2, P=7, F=243),
             dict(seed=0, call=0, k=0, b0=0, p0=0, B=1, P=1, F=27)]
    total = differ = 0
    worst = 0
    for c in cases:
        key = ops.noise_key(c["seed"], c["call"], c["b0"], c["p0"], DEV)
        got = ops.noise_fill(key, c["k"], c["B"], c["P"], c["F"], J)
        assert got.shape == (c["B"], c["P"], c["F"], J, 3) and got.dtype == torch.float32
        got = got.cpu().numpy()
        want = host.reference_draw(c["seed"], c["call"], c["k"], c["b0"], c["p0"], c["B"], c["P"], c["F"], J)
        assert np.isfinite(got).all()
        d = np.abs(_ordered(got) - _ordered(want))
        total += d.size
        differ += int((d != 0).sum())
        worst = max(worst, int(d.max()))
        print(f"noise_fill {c}: {d.size} values, {int((d != 0).sum())} not bit-equal, max distance {int(d.max())} ulp")
    print(f"noise_fill vs host: {total} values, {differ} not bit-equal ({differ / total:.2e}), worst {worst} ulp")
    assert total >= 2_000_000
    assert worst <= 1
    assert differ / total <= 1e-5


def test_noise_fill_op_and_argument_checks():
    from pafuse_amd import _lib, ops, torch_ops  # noqa: F401
    key = ops.noise_key(7, 1, 0, 2, DEV)
    a = ops.noise_fill(key, 3, 2, 3, 27, J)
    assert torch.equal(torch.ops.pafuse.noise_fill(key, 3, 2, 3, 27, J), a)
    assert torch.equal(ops.noise_fill(ops.noise_key(7, 1, 1, 3, DEV), 3, 1, 2, 27, J), a[1:, 1:])      # a slice of the stream
    assert not torch.equal(ops.noise_fill(key, 2, 2, 3, 27, J), a)
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    out = torch.empty(1, 1, 27, J, 3, device=DEV)
    E_ARG = lib.pafuse_noise_fill(None, 0, 1, 1, 27, J, out.data_ptr(), s)
    assert E_ARG < 0
    for bad in ((key.data_ptr(), -1, 1, 1, 27, J, out.data_ptr()), (key.data_ptr(), 0, 0, 1, 27, J, out.data_ptr()),
                (key.data_ptr(), 0, 1, 1, 27, J, None)):
        assert lib.pafuse_noise_fill(*bad, s) == E_ARG, bad
    with pytest.raises(ValueError):
        ops.noise_fill(key.cpu(), 0, 1, 1, 27, J)
    # the seeded loop refuses a null key like its neighbour refuses null noise
    from __graft_entry__ import make_model
    model, _ = make_model(1, 1)
    cfg, steps = model.config_struct(True), model.ddim_steps()
    x2d, x2f = _inputs(1)
    nbytes = lib.pafuse_d3dp_workspace_bytes(C.byref(cfg), 1, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    res = torch.empty(1, 1, 1, 27, J, 3, device=DEV)
    aux = (C.c_void_p * 1)()
    assert lib.pafuse_d3dp_sample_seeded(C.byref(cfg), steps, 1, x2d.data_ptr(), x2f.data_ptr(), None, 1, 1, res.data_ptr(),
                                         ws.data_ptr(), nbytes, s, aux, 0) == E_ARG
    assert lib.pafuse_d3dp_sample_seeded(C.byref(cfg), steps, 1, x2d.data_ptr(), x2f.data_ptr(), key.data_ptr(), 1, 1,
                                         res.data_ptr(), ws.data_ptr(), nbytes - 1, s, aux, 0) < 0       # workspace too small
    torch.cuda.synchronize()


@pytest.mark.parametrize("flip", [True, False])
def test_seeded_loop_equals_the_buffer_loop_on_the_same_normals(flip):
    from __graft_entry__ import make_model
    B, P = 2, 3
    model, _ = make_model(P, 10, flip=flip)
    x2d, x2f = _inputs(B)
    for T in (1, 2, 10):
        model.sampling_timesteps = T
        _device(model, seed=40 + T, call=5)
        got = model(x2d, None, input_2d_flip=x2f if flip else None)
        assert model.noise_call == 6                                  # one public call
        _inject(model, seed=40 + T, call=5)
        want = model(x2d, None, input_2d_flip=x2f if flip else None)
        model.noise_fn = None
        torch.cuda.synchronize()
        assert got.shape == (B, T, P, 27, J, 3) and torch.isfinite(got).all()
        assert torch.equal(got, want), (flip, T, (got - want).abs().max().item())


@pytest.mark.parametrize("precision", ["f32", "bf16x3_images", "f16x2", "bf16"])
def test_seeded_loop_in_every_precision(precision):
    from __graft_entry__ import make_model
    model, _ = make_model(2, 2)
    model.precision = precision
    x2d, x2f = _inputs(1)
    _device(model, seed=3)
    got = model(x2d, None, input_2d_flip=x2f)
    _inject(model, seed=3, call=0)
    want = model(x2d, None, input_2d_flip=x2f)
    torch.cuda.synchronize()
    assert torch.equal(got, want), precision


def test_seeded_graph_replays_take_their_key_from_16_bytes():
    from __graft_entry__ import make_model
    B, P, T = 2, 3, 2
    model, _ = make_model(P, T)
    x2d, x2f = _inputs(B)
    _device(model, seed=77)
    model.use_graph = True
    first = model(x2d, None, input_2d_flip=x2f)           # capture + replay 1 under call 0
    second = model(x2d, None, input_2d_flip=x2f)          # replay 2 under call 1
    assert model.noise_call == 2 and len(model._graphs) == 1
    st = next(iter(model._graphs.values()))[1]
    assert st["noise"].numel() == 4 and st["noise"].dtype == torch.int32      # what a replay refreshes: the 16-byte key
    model.use_graph = False
    for call, got in ((0, first), (1, second)):
        _inject(model, seed=77, call=call)
        want = model(x2d, None, input_2d_flip=x2f)
        model.noise_fn = None
        torch.cuda.synchronize()
        assert torch.equal(got, want), call
    assert not torch.equal(first, second)
    model._graphs.clear()


def test_shards_chunks_and_clip_chunks_see_the_one_call_run():
    from __graft_entry__ import make_model
    P, T = 8, 2
    model, _ = make_model(P, T)
    x2d, x2f = _inputs(4)
    _device(model, seed=9, call=3)
    whole = model(x2d, None, input_2d_flip=x2f)                        # B = 4, one launch, one call
    assert model.clips_per_launch(P, True) >= 4 and model.noise_call == 4

    # P = 8 as shards (3, 3, 2): three "ranks", each one call under the same (seed, call)
    sampler = ShardedSampler(model)
    parts = []
    for rank in range(3):
        sampler.rank, sampler.world = rank, 3
        model.noise_call = 3
        pred, h0, n = sampler.sample_local(x2d[:2], None, input_2d_flip=x2f[:2])
        assert (h0, h0 + n) == shard_range(P, rank, 3) and model.noise_call == 4 and model.proposal_shard is None
        parts.append(pred)
    assert [p.shape[2] for p in parts] == [3, 3, 2]
    assert torch.equal(torch.cat(parts, dim=2), whole[:2])

    # the same with hypothesis_chunk = 1: every chunk under one call, which advances once behind the last chunk
    parts = []
    for rank in range(3):
        sampler.rank, sampler.world = rank, 3
        model.noise_call = 3
        for pred, h0, n in sampler.sample_chunks(x2d[:2], None, input_2d_flip=x2f[:2], chunk=1):
            assert n == 1 and h0 == sum(p.shape[2] for p in parts)
            parts.append(pred)
        assert model.noise_call == 4, rank
    assert len(parts) == P and torch.equal(torch.cat(parts, dim=2), whole[:2])
    # a rank without hypotheses (P < world) still counts the call
    sampler.rank, sampler.world = 9, 10
    model.noise_call = 3
    pred, _, n = sampler.sample_local(x2d[:2], None, input_2d_flip=x2f[:2])
    assert n == 0 and pred.shape[2] == 0 and model.noise_call == 4

    # B = 4 with the clips one per launch
    model.noise_call = 3
    model.max_rows_per_launch = 2 * P
    assert model.clips_per_launch(P, True) == 1
    one_by_one = model(x2d, None, input_2d_flip=x2f)
    model.max_rows_per_launch = 640
    torch.cuda.synchronize()
    assert torch.equal(one_by_one, whole)
    # and the next call is another draw
    assert model.noise_call == 4
    assert not torch.equal(model(x2d, None, input_2d_flip=x2f), whole)


def test_shard_call_allocates_no_full_P_noise():
    from __graft_entry__ import make_model
    B, T, P, lo, hi = 2, 10, 160, 20, 40
    model, _ = make_model(P, T)
    x2d, x2f = _inputs(B)

    def peak(run):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - base

    def shard_call():
        model.proposal_shard = (lo, hi)
        try:
            return model(x2d, None, input_2d_flip=x2f)
        finally:
            model.proposal_shard = None

    def plain_call():
        model.num_proposals = hi - lo
        try:
            return model(x2d, None, input_2d_flip=x2f)
        finally:
            model.num_proposals = P

    _device(model, seed=1)
    plain_call()                                     # the weight images and the side streams exist from here on
    unsharded = peak(plain_call)
    shard_device = peak(shard_call)
    model.noise = "torch"
    shard_torch = peak(shard_call)
    one_discarded_draw = B * (P - (hi - lo)) * 27 * J * 3 * 4
    print(f"peak bytes above the resident set: unsharded P=20 'device' {unsharded}, shard (20,40) of 160 'device' {shard_device}, "
          f"'torch' {shard_torch} (+{(shard_torch - shard_device) / 1e6:.1f} MB; one discarded draw = {one_discarded_draw / 1e6:.1f} MB)")
    assert abs(shard_device - unsharded) <= 1_000_000
    assert shard_torch - shard_device >= one_discarded_draw

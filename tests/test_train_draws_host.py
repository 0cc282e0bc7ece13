"""The training half of noise stream v1 on the host: pafuse_amd.noise.reference_train_draws /
reference_droppath - the statement the kernels are compared with bit for bit in tests/test_hip_train_draws.py - and the
attribute logic of D3DP.train_draws that needs no device.

The uniformity checks are a sanity check of the STATEMENT on one committed seed (chosen on the CPU so that both hold; the
bounds are 3.4 sigma of chi^2 with 999 degrees of freedom and 4.5 sigma of a binomial fraction); the GPU is never asked
this question."""
import numpy as np
import pytest
import torch

from pafuse_amd import noise as host

SEED = 20261018


def test_timestep_formula_against_big_integers():
    clips = [0, 1, 2, 7, 1000, 2 ** 31, 2 ** 32 - 1] + list(range(100, 164))
    for call in (0, 5, 2 ** 32 - 1):
        r0 = host.philox4x32_10((np.uint32(0), np.uint32(0), np.array(clips, dtype=np.uint32), np.uint32(0xFFFFFFFE)),
                                (np.uint32(SEED), np.uint32(call)))[0]
        for T in (1, 2, 1000, 2 ** 31):
            t, _ = host.reference_train_draws(SEED, call, clips, 1, 1, T)
            assert t.dtype == np.int64 and t.shape == (len(clips),)
            assert t.tolist() == [(int(r) * T) >> 32 for r in r0], T
            assert 0 <= t.min() and t.max() < T
            if T == 1:
                assert not t.any()
    assert len(set(host.reference_train_draws(SEED, 0, clips, 1, 1, 1000)[0].tolist())) > 50
    for bad in (0, 2 ** 32 + 1):
        with pytest.raises(ValueError):
            host.reference_train_draws(SEED, 0, [0], 1, 1, bad)
    with pytest.raises(ValueError):
        host.reference_train_draws(SEED, 0, [2 ** 32], 1, 1, 10)


def test_noise_is_draw_0xffffffff_of_stream_v1_for_strided_clips():
    assert host.STREAM_VERSION == 1 and (host.K_NOISE, host.K_TIMESTEP, host.K_DROPPATH) == (2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 3)
    F, J = 3, 5
    for clips in ([0, 1, 2], [1, 3, 5], [3, 7, 11, 15], [2 ** 32 - 9, 2 ** 32 - 7]):
        _, z = host.reference_train_draws(SEED, 4, clips, F, J, 1000)
        assert z.dtype == np.float32 and z.shape == (len(clips), F, J, 3)
        for i, g in enumerate(clips):
            want = host.reference_draw(SEED, 4, 0xFFFFFFFF, g, 0, 1, 1, F, J)[0, 0]
            assert np.array_equal(z[i].view(np.int32), want.view(np.int32)), g
    # the last clip of the index space (reference_draw's range check stops one short of it): finite, and its own values
    _, z = host.reference_train_draws(SEED, 4, [2 ** 32 - 1, 2 ** 32 - 2], F, J, 1000)
    assert np.isfinite(z).all() and not np.array_equal(z[0], z[1])


def test_a_clip_draws_the_same_in_every_list():
    F, J, keep, factor = 4, 3, [1.0, 1.0, 0.5, 0.5], [1.0, 1.0, 2.0, 2.0]
    whole = list(range(6))
    t, z = host.reference_train_draws(SEED, 9, whole, F, J, 1000)
    d = host.reference_droppath(SEED, 9, whole, 1, F, J, keep, factor)
    assert d.shape == (4, 2, 6 * 4) and set(np.unique(d[2:]).tolist()) <= {0.0, 1.0, 2.0} and (d[:2] == 1).all()
    assert 0 < (d[2:, :, :18] == 0).sum() < d[2:, :, :18].size
    assert (d[3, :, 18:] == 1).all()                                   # temporal rows: 6 * 3 sequences, then the tail
    for clips in ([0, 2, 4], [1, 3, 5], [5], [3, 0]):
        t2, z2 = host.reference_train_draws(SEED, 9, clips, F, J, 1000)
        d2 = host.reference_droppath(SEED, 9, clips, 1, F, J, keep, factor)
        assert np.array_equal(t2, t[clips]) and np.array_equal(z2, z[clips])
        for k in range(4):
            L = J if k % 2 else F
            got = d2[k, :, :len(clips) * L].reshape(2, len(clips), L)
            assert np.array_equal(got, d[k, :, :6 * L].reshape(2, 6, L)[:, clips]), (clips, k)
    assert not np.array_equal(host.reference_train_draws(SEED, 10, whole, F, J, 1000)[1], z)          # another call
    assert not np.array_equal(host.reference_droppath(SEED, 10, whole, 1, F, J, keep, factor), d)


def test_reserved_counter_words_and_denoisers_do_not_share_draws():
    key = (np.uint32(SEED), np.uint32(0))
    g = np.arange(64, dtype=np.uint32)
    words = {k: np.stack(host.philox4x32_10((np.uint32(0), np.uint32(0), g, np.uint32(k)), key))
             for k in (host.K_NOISE, host.K_TIMESTEP, host.K_DROPPATH, 0, 1, 999)}
    names = list(words)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not (words[a] == words[b]).any(), (a, b)
    per_d = [np.stack(host.philox4x32_10((np.uint32(3), np.uint32((d << 16) | (5 << 1) | 1), g, np.uint32(host.K_DROPPATH)), key))
             for d in (0, 1, 2)]
    assert not (per_d[0] == per_d[1]).any() and not (per_d[0] == per_d[2]).any() and not (per_d[1] == per_d[2]).any()
    keep, factor = [0.5, 0.5], [2.0, 2.0]
    tables = [host.reference_droppath(SEED, 0, list(range(8)), d, 27, 24, keep, factor) for d in (0, 1, 2)]
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[0], tables[2]) and not np.array_equal(tables[1], tables[2])
    assert not np.array_equal(tables[0][0, 0], tables[0][0, 1])                                       # the two branches


def test_uniformity_of_the_statement_on_the_committed_seed():
    t, _ = host.reference_train_draws(SEED, 0, range(100_000), 1, 1, 1000)
    counts = np.bincount(t, minlength=1000)
    chi2 = float(((counts - 100.0) ** 2 / 100.0).sum())
    print(f"timestep chi^2 = {chi2:.1f} (999 degrees of freedom)")
    assert counts.shape == (1000,) and chi2 < 1150
    d = host.reference_droppath(SEED, 0, range(1000), 0, 100, 1, [0.8, 0.8], [1.25, 1.25])
    kept = d[0]                                                          # spatial block: 1000 * 100 sequences x 2 branches
    assert kept.size == 200_000 and set(np.unique(kept).tolist()) == {0.0, 1.25}
    frac = float((kept != 0).mean())
    print(f"DropPath keep fraction = {frac:.5f}")
    assert abs(frac - 0.8) <= 0.004
    ones = host.reference_droppath(SEED, 0, range(4), 0, 5, 7, [1.0, 1.0], [1.0, 1.0])
    assert (ones == 1).all()                                             # rate 0: u < 1 always


# ------------------------------------------------------------------------------------------ D3DP attributes, no device
def _model(depth=1):
    from __graft_entry__ import make_model
    return make_model(1, 1, device="cpu", is_train=True, depth=depth)[0]


def test_train_draws_and_injected_draws_exclude_each_other():
    m = _model()
    assert m.train_draws == "torch" and m.train_call == 0 and m.train_clips == (0, 1)
    with pytest.raises(ValueError):
        m.train_draws = "philox"
    m.train_draw_fn = lambda i: None
    with pytest.raises(ValueError):
        m.train_draws = "device"
    assert m.train_draws == "torch"
    m.train_draw_fn = None
    m.train_draws = "device"
    with pytest.raises(ValueError):
        m.train_draw_fn = lambda i: None
    assert m.train_draw_fn is None
    m.noise = "device"                     # the eval loop's property is another one: both may be on, neither implies the other
    m.noise = "torch"
    assert m.train_draws == "device"
    # a denoiser that holds a key refuses injected DropPath factors
    body = next(iter(m.denoisers().values()))
    body.drop_fn = lambda *a: None
    body.drop_key = (torch.zeros(4, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        body.drop_path_factors(2, torch.device("cpu"))


def test_seed_restarts_the_call_and_forward_advances_it(monkeypatch):
    from pafuse_amd import ops
    m = _model()
    m.train_draws = "device"
    m.noise_seed = 77
    keys, fills = [], []

    def train_key(seed, call, first, stride, device, clips=None):
        keys.append((seed, call, first, stride, clips))
        return torch.tensor([seed, call], dtype=torch.int64)

    def qsample_seeded(x0, key4, sqrt_ac, sqrt_1mac, scale, num_timesteps, want_noise=False):
        assert num_timesteps == 1000 and scale == 1.0
        return x0 + 1, torch.arange(x0.shape[0]), (torch.zeros_like(x0) if want_noise else None)

    monkeypatch.setattr(ops, "train_key", train_key)
    monkeypatch.setattr(ops, "qsample_seeded", qsample_seeded)
    monkeypatch.setattr(m, "_check_targets", lambda targets: None)

    def pred_parts(input_2d, x_poses, t):
        fills.append([mod.drop_key for mod in m.denoisers().values()])
        assert t.shape == (3,)
        return x_poses

    monkeypatch.setattr(m, "pred_parts", pred_parts)
    x2d, x3d = torch.zeros(3, 27, 134, 2), torch.zeros(3, 27, 134, 3)
    m.train_clips = (1, 2)
    for step in range(3):
        assert m.train_call == step
        assert torch.equal(m(x2d, x3d), x3d + 1)
    assert keys == [(77, 0, 1, 2, 3), (77, 1, 1, 2, 3), (77, 2, 1, 2, 3)]
    assert [[d for _, d in f] for f in fills] == [[0, 1, 2]] * 3                     # D3DP.denoisers() order
    assert all(int(k[1]) == step for step, f in enumerate(fills) for k, _ in f)
    assert all(mod.drop_key is None for mod in m.denoisers().values())               # only while the forward runs
    x_t, noise, t = m.prepare_targets(x3d)                                           # looks at the next step, does not consume it
    assert m.train_call == 3 and keys[-1][1] == 3 and noise is not None and t.shape == (3, 1)
    m.noise_call = 5
    m.noise_seed = 78
    assert (m.noise_seed, m.noise_call, m.train_call) == (78, 0, 0)
    m.train_call = 2 ** 32 - 1
    from pafuse_amd import _lib
    with pytest.raises(_lib.PafuseError):
        m(x2d, x3d)


def test_train_key_checks_the_clip_map_on_the_host():
    from pafuse_amd import ops
    k = ops.train_key(7, 2 ** 32 - 1, 2 ** 32 - 9, 2, "cpu", clips=5)
    assert k.dtype == torch.int32 and k.numpy().view(np.uint32).tolist() == [7, 2 ** 32 - 1, 2 ** 32 - 9, 2]
    for bad in (dict(stride=0), dict(first=2 ** 32 - 9, stride=2, clips=6), dict(seed=-1), dict(call=2 ** 32), dict(first=1.5)):
        kw = dict(seed=0, call=0, first=0, stride=1, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.train_key(**kw)


def test_checkpoint_carries_the_stream_only_in_device_mode(tmp_path):
    from pafuse_amd import h3wb, harness
    m = _model()
    opt = torch.optim.AdamW(m.parameters(), lr=6e-5)
    plain = harness.read_checkpoint(h3wb.save_state(m, opt, 1, 6e-5, str(tmp_path), random_state=np.random.RandomState(3), tag="a"))
    assert set(plain) == {"optimizer", "epoch", "lr", "model_pos", "random_state"}
    m.train_draws = "device"
    m.noise_seed = 41
    m.train_call = 12
    for wrapped in (m, torch.nn.DataParallel(m)):
        fname = h3wb.save_state(wrapped, opt, 1, 6e-5, str(tmp_path), random_state=np.random.RandomState(3), tag="b")
        ckpt = harness.read_checkpoint(fname)
        assert set(ckpt) == set(plain) | {"train_stream"} and ckpt["train_stream"] == {"seed": 41, "call": 12}
        assert set(ckpt["model_pos"]) == set(plain["model_pos"])
    fresh = _model()
    fresh.train_draws = "device"
    harness.load_checkpoint(fresh, fname)
    assert (fresh.noise_seed, fresh.train_call) == (41, 12)
    harness.load_checkpoint(fresh, plain)                                 # a default run's file leaves the stream alone
    assert (fresh.noise_seed, fresh.train_call) == (41, 12)


def test_train_epoch_places_the_rank_in_the_global_batch(monkeypatch):
    from types import SimpleNamespace
    from pafuse_amd import h3wb
    m = _model()
    gen = SimpleNamespace(shard=(3, 8), next_epoch=lambda: iter(()))
    h3wb.train_epoch(m, None, gen, None, "cpu")
    assert m.train_clips == (0, 1)                                        # the default mode is not touched
    m.train_draws = "device"
    h3wb.train_epoch(torch.nn.DataParallel(m), None, gen, None, "cpu")
    assert m.train_clips == (3, 8)
    gen.shard = None
    h3wb.train_epoch(m, None, gen, None, "cpu")
    assert m.train_clips == (0, 1)


def test_drop_path_tables_are_the_torch_path_s_numbers():
    import pafuse_amd
    m = pafuse_amd.MixSTE2(num_frame=3, num_joints=5, embed_dim_ratio=64, depth=4, drop_path_rate=0.2, is_train=True)
    rates, keep, factor = m.drop_path_tables("cpu")
    want = [x.item() for x in torch.linspace(0, 0.2, 4)]
    assert rates == want and keep.dtype == torch.float64 and factor.dtype == torch.float32
    assert keep.tolist() == [1.0 - r for r in want for _ in range(2)] and keep[0] == 1.0 and factor[0] == 1.0
    for k in range(8):
        assert factor[k] == torch.ones(()).div_(float(keep[k]))
    assert m.drop_path_tables("cpu")[1] is keep                           # cached
    m.drop_path_rate = 0.999
    assert abs(float(m.drop_path_tables("cpu")[1][-1]) - 0.001) < 1e-6

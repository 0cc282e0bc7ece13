"""CPU tests of 243-frame clips (no GPU): the config, the model's parameters and checkpoints, the clip cutting and the
synthetic helpers at F = 243, and the library's mode table for long clips."""
import torch

from pafuse_amd import config, harness
from tests.golden import golden_util as gu

F = 243


def _model(frames=F, depth=1):
    from __graft_entry__ import make_model
    return make_model(2, 1, device="cpu", depth=depth, frames=frames)


def test_config_with_243_frames_loads():
    args = config.load(None, ["model.number_of_frames=243", "model.stride=243"])
    assert args.model.number_of_frames == 243 and args.model.stride == 243
    assert config.load(None, []).model.number_of_frames == 27


def test_d3dp_builds_243_frame_denoisers():
    model, sd = _model()
    assert model.frames == F
    for part, C in gu.PART_WIDTH.items():
        assert tuple(sd[f"pose_estimator.{part}.Temporal_pos_embed"].shape) == (1, F, C)
        assert model.pose_estimator[part].num_frame == F


def test_state_dict_round_trips_in_both_layouts(tmp_path):
    model, sd = _model()
    plain = {k: v.clone() for k, v in model.state_dict().items()}
    wrapped = {"module." + k: v for k, v in plain.items()}
    for layout in (plain, wrapped):
        fresh, _ = _model()
        for p in fresh.parameters():
            p.data.zero_()
        path = tmp_path / "ck.bin"
        torch.save({"model_pos": layout}, path)
        harness.load_checkpoint(fresh, harness.read_checkpoint(str(path)))
        got = fresh.state_dict()
        assert set(got) == set(plain)
        assert all(torch.equal(got[k], plain[k]) for k in plain)
    # a 27-frame checkpoint does not load into a 243-frame model: the temporal position embedding has another shape
    small, _ = _model(frames=27)
    fresh, _ = _model()
    try:
        harness.load_checkpoint(fresh, {"model_pos": small.state_dict()})
    except RuntimeError as e:
        assert "Temporal_pos_embed" in str(e)
    else:
        raise AssertionError("a 27-frame checkpoint loaded into a 243-frame model")


def _seq(n):
    return torch.arange(n, dtype=torch.float32)[:, None, None].expand(n, 134, 2).clone()


def test_cut_and_stitch_at_243_frames():
    for n in (100, 2 * F, 2 * F + 57):
        seq = _seq(n)
        clips = harness.cut_clips(seq, frames=F)
        assert clips.shape == (max(1, -(-n // F)), F, 134, 2)
        if n < F:   # padded with the last frame
            assert torch.equal(clips[0, n:, 0, 0], torch.full((F - n,), float(n - 1)))
        else:       # the last clip holds the last F frames
            assert torch.equal(clips[-1, :, 0, 0], torch.arange(n - F, n, dtype=torch.float32))
        # "predictions" that carry the frame index: stitching gives back 0 .. n-1 in order
        pred = clips[:, None, None, :, :, :1].expand(clips.shape[0], 1, 2, F, 134, 3)
        out = harness.stitch_clips(pred, n, frames=F)
        assert out.shape == (1, 2, n, 134, 3)
        assert torch.equal(out[0, 0, :, 0, 0], torch.arange(n, dtype=torch.float32))


def test_synthetic_helpers_take_frames():
    x, xf = gu.synthetic_inputs_2d(B=2, frames=F)
    assert x.shape == xf.shape == (2, F, 134, 2)
    noises = gu.synthetic_noises(B=1, P=3, n=2, frames=F)
    assert [tuple(n.shape) for n in noises] == [(1, 3, F, 134, 3)] * 2
    assert gu.synthetic_target_3d(B=2, frames=F).shape == (2, F, 134, 3)
    # the default stays 27 frames, bit for bit what it was
    assert gu.FRAMES == 27
    assert torch.equal(gu.synthetic_inputs_2d(B=1)[0], gu.synthetic_inputs_2d(B=1, frames=27)[0])
    assert gu.synthetic_noises(B=1, P=1, n=1)[0].shape == (1, 1, 27, 134, 3)


def test_mode_table_for_long_clips():
    from pafuse_amd import _lib
    lib = _lib.load()
    for mode in (0, 2):
        assert lib.pafuse_mode_supported(mode, 384, 0, 8, 24, 243) == 1
        assert lib.pafuse_mode_supported(mode, 224, 0, 8, 68, 256) == 1
        assert lib.pafuse_mode_supported(mode, 384, 0, 8, 24, 257) == 0
    assert lib.pafuse_mode_supported(3, 384, 0, 8, 24, 144) == 1
    assert lib.pafuse_mode_supported(3, 384, 0, 8, 24, 243) == 0      # f16x2: no long-sequence form
    assert lib.pafuse_mode_supported(4, 384, 0, 8, 24, 243) == 0      # bf16x3 on images: no fused form



def _workspace_bytes(frames, B, P, flip=True):
    """pafuse_d3dp_workspace_bytes of the three-part model (operand mode 2) for B clips of `frames` frames"""
    from pafuse_amd import _lib
    cfg = _lib.D3DPConfig()
    cfg.num_parts, cfg.num_kps, cfg.frames, cfg.flip = 3, 134, frames, int(flip)
    for i, part in enumerate(("body", "face", "hands")):
        w = cfg.part[i]
        w.frames, w.joints, w.channels, w.operand_bf16 = frames, len(gu.PART_JOINTS[part]), gu.PART_WIDTH[part], 2
    return _lib.load().pafuse_d3dp_workspace_bytes(cfg, B, P)


def test_batches_are_cut_by_token_rows_at_243_frames():
    """the clip-axis cutting keeps a library call's token rows - and so its workspace - at the 27-frame budget: at the
    reference's evaluation batch (model.batch_size 1024 // 243 = 4 clips of a sequence per call, up to 16-32 clips for long
    sequences) with P = 20 under flip-TTA, one clip per call at 243 frames; 27-frame clips are cut exactly as before"""
    model, _ = _model()
    short, _ = _model(frames=27)
    assert model.max_rows_per_launch == short.max_rows_per_launch == 640
    assert short.clips_per_launch(20, True) == 16 and short.clips_per_launch(10, False) == 64      # 640 // (2 P), 640 // P
    assert model.clips_per_launch(20, True) == 1 and model.clips_per_launch(2, True) == 17         # 640 * 27 // 243 = 71
    assert model.clips_per_launch(100, True) == 1                                                 # never fewer than one
    short.max_rows_per_launch = 8                  # test_large_batches_are_cut_along_the_clip_axis's setting: unchanged
    assert short.clips_per_launch(2, True) == 2
    # the workspace a call asks for: per clip it grows with the frames; per call it stays near the 27-frame budget
    per_clip_27, per_clip_243 = _workspace_bytes(27, 1, 20), _workspace_bytes(F, 1, 20)
    assert 8.5 < per_clip_243 / per_clip_27 < 9.5
    call_27 = _workspace_bytes(27, 16, 20)                                                        # 16 clips per call
    call_243 = _workspace_bytes(F, model.clips_per_launch(20, True), 20)
    assert call_243 <= 1.2 * call_27, (call_243 / 2 ** 30, call_27 / 2 ** 30)
    assert call_243 < 10 * 2 ** 30, call_243 / 2 ** 30                                             # ~8.2 GB for 40 rows
    # the largest call of a 243-frame evaluation in sizes the library indexes in 64 bits: row counts stay below 2^31
    rows = 2 * model.clips_per_launch(2, True) * 2 * F * 68
    assert rows < 2 ** 31


def test_oracle_matches_the_reference_fixture_at_243_frames():
    """G22 (the reference's own D3DP at 243 frames, tests/golden/make_golden_long.py) against the CPU oracle: the oracle the
    GPU tests compare with computes what the reference computes at this clip length"""
    from oracle import d3dp_oracle as orc
    from tests.conftest import load_golden
    from tests.golden import g22_inputs as g22
    z = load_golden("g22_long_clips.npz")
    inp = g22.inputs()
    assert g22.digest(inp) == z["inputs_sha"].numpy().tobytes()
    _, sd = make_model_g22()
    assert gu.sha256_of(sd) == z["sha"].numpy().tobytes()
    out = orc.ddim_sample(sd, inp["x2d"], list(inp["noise_flip"]), g22.T, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                          inputs_2d_flip=inp["x2d_flip"], depth=g22.DEPTH)
    assert out.shape == z["flip_out"].shape
    assert float((out - z["flip_out"]).abs().max()) <= 1e-5


def make_model_g22():
    from __graft_entry__ import make_model
    from tests.golden import g22_inputs as g22
    return make_model(g22.P, g22.T, seed=g22.SEED, device="cpu", depth=g22.DEPTH, frames=g22.FRAMES)

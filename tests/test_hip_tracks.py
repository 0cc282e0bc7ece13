"""People followed through a video on the device: track_nodes_kernel, track_links_kernel (pafuse_tracks_links),
track_path_kernel (pafuse_tracks_path), track_gather_kernel (pafuse_tracks_gather), ops.track_people,
torch.ops.pafuse.track_people, harness.track_people, evaluate_frames(distract=..., track=...) and the --track logic of examples/infer_in_the_wild.py.

What is asserted and why it can be asserted:
  * links vs statement: the kernels and pafuse_amd/tracks.py perform the same IEEE fp64 operations in the same order (lane sums
    in SUM_ORDER, contraction off, correctly rounded divides and square roots) -> the design goal is equal bits.  Where gain is
    -inf and where size is NaN must be identical; the values are accepted equal or ADJACENT in fp64 - the rule of
    tests/test_hip_frame_metrics.py - and the number that differ is printed.
  * the path kernel alone, on the statement's gains and on constructed tables: selections under strict > and single fp64
    additions along one path, in one order -> assign and frames torch.equal, score the same double.
  * planted case A of tests/test_tracks_host.py is exact by construction -> the truth.
Shapes: J in {1, 5, 64, 65, 134} x (N, K, G) in {(1,1,1), (2,2,1), (9,7,3), (70,5,4), (12,64,8)}.
"""
import json

import numpy as np
import pytest
import torch

from tests.test_hip_partials import dataset, same_bits
from tests.test_hip_rootfit import equal_or_adjacent
from tests.test_tracks_host import CASE_A_SEEDS, case_a, example, rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1), (2, 2, 1), (9, 7, 3), (70, 5, 4), (12, 64, 8)]
CASES = [(J,) + s for J in (1, 5, 64, 65, 134) for s in SHAPES]


def support_for(J):
    return 1 if J == 1 else 2 if J == 5 else 5


def inputs(J, N, K, seed):
    """a random walk per candidate with random confidences; 30 % of the slots absent (all zero), 30 % of the joints unobserved
    (confidence 0), one NaN coordinate under a positive confidence, and one candidate that coincides with one of the frame
    before (cost exactly 0) -> (x2d [N,K,J,2], conf [N,K,J]) on the host"""
    rng = np.random.default_rng(seed)
    body = rng.uniform(-0.2, 0.2, (1, K, J, 2))
    centre = rng.uniform(-0.5, 0.5, (1, K, 1, 2)) + np.cumsum(rng.standard_normal((N, K, 1, 2)) * 0.02, axis=0)
    x = (body + centre + 0.004 * rng.standard_normal((N, K, J, 2))).astype(np.float32)
    c = rng.uniform(0.1, 1.0, (N, K, J)).astype(np.float32)
    c[rng.random((N, K, J)) < 0.3] = 0
    if N > 1:
        n = N // 2
        x[n, K - 1], c[n, K - 1] = x[n - 1, 0], c[n - 1, 0]
    gone = rng.random((N, K)) < 0.3
    if N > 1:
        gone[N // 2, K - 1] = gone[N // 2 - 1, 0] = False
    x[gone], c[gone] = 0, 0
    seen = np.argwhere(c > 0)
    if len(seen):
        n, k, j = seen[len(seen) // 3]
        x[n, k, j, 1] = np.nan
    return x, c


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def same_pattern_and_adjacent(got, want):
    """-inf and NaN in the same places; the other values equal or adjacent in fp64 -> the number that are not equal"""
    got, want = got.cpu(), torch.from_numpy(want)
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)) and torch.equal(torch.isnan(got), torch.isnan(want))
    assert not bool(torch.isposinf(got).any()) and not bool(torch.isposinf(want).any())
    off = torch.isneginf(want)
    return equal_or_adjacent(torch.where(off, torch.zeros_like(got), got), torch.where(off, torch.zeros_like(want), want))


@pytest.fixture(scope="module")
def link_cases():
    """inputs and the statement's gain and size for every case, computed once and never modified"""
    from pafuse_amd import tracks
    out = {}
    for J, N, K, G in CASES:
        x, c = inputs(J, N, K, seed=7 * J + N + K)
        out[J, N, K, G] = (x, c) + tracks.links(x, c, max_gap=G, support=support_for(J))
    return out


def run_path(gain, size, M, min_frames=1, seed=None):
    """pafuse_tracks_path alone, on tables from anywhere -> (assign, score, frames) on the host"""
    from pafuse_amd import _lib
    lib = _lib.load()
    gain, size = dev(np.asarray(gain, dtype=np.float64), np.asarray(size, dtype=np.float64))
    N, G, K, _ = gain.shape
    need = lib.pafuse_tracks_workspace_bytes(N, K, 1, G)
    work = torch.empty(need // 8, device=DEV, dtype=torch.float64)
    assign = torch.full((M, N), -7, device=DEV, dtype=torch.int32)
    score = torch.full((M,), 123.0, device=DEV, dtype=torch.float64)
    frames = torch.full((M,), -7, device=DEV, dtype=torch.int32)
    sn, sk = (-1, -1) if seed is None else seed
    _lib.check(lib.pafuse_tracks_path(gain.data_ptr(), size.data_ptr(), N, K, G, M, min_frames, sn, sk, assign.data_ptr(), score.data_ptr(),
                                      frames.data_ptr(), work.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return assign.cpu(), score.cpu(), frames.cpu()


def assert_path(gain, size, M, min_frames=1, seed=None, note=""):
    from pafuse_amd import tracks
    want = tracks.path(gain, size, M, min_frames, seed)
    got = run_path(gain, size, M, min_frames, seed)
    assert torch.equal(got[0], torch.from_numpy(want[0])), note
    assert torch.equal(got[2], torch.from_numpy(want[2])), note
    assert same_bits(got[1], torch.from_numpy(want[1])), note
    return want


# ------------------------------------------------------------------------------------------------------------ links
@pytest.mark.parametrize("case", CASES, ids=lambda c: "J%d-N%d-K%d-G%d" % c)
def test_links_equal_the_statement(case, link_cases):
    from pafuse_amd import ops
    J, N, K, G = case
    x, c, gain, size = link_cases[case]
    got = ops.track_people(*dev(x, c), max_gap=G, support=support_for(J), min_frames=1, want=("gain", "size"))
    assert tuple(got["gain"].shape) == (N, G, K, K) and tuple(got["size"].shape) == (N, K) and got["gain"].dtype == torch.float64
    differ = {"gain": same_pattern_and_adjacent(got["gain"], gain), "size": same_pattern_and_adjacent(got["size"], size)}
    allowed = int(np.isfinite(gain).sum())
    print(f"(J, N, K, G) = {case}: values that differ from the statement (by one fp64 step): {differ} of {allowed} allowed links / "
          f"{int((~np.isnan(size)).sum())} present candidates")
    if J > 1 and N > 1:                                                        # the coinciding pair: cost exactly 0
        assert float(got["gain"][N // 2, 0, 0, K - 1]) == 0.5
    if J == 1:
        assert allowed == 0


# ------------------------------------------------------------------------------------------------------------ the path kernel alone
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (64, 134)], ids=lambda c: "J%d-N%d-K%d-G%d" % c)
@pytest.mark.parametrize("M", (1, 3))
def test_path_on_the_statements_gains(case, M, link_cases):
    x, c, gain, size = link_cases[case]
    assert_path(gain, size, M, 1)
    assert_path(gain, size, M, 3)
    present = np.argwhere(~np.isnan(size))
    if M == 1 and len(present):
        n0, k0 = (int(v) for v in present[len(present) // 2])
        assert_path(gain, size, 1, 1, seed=(n0, k0))
        assert_path(gain, size, 1, 1, seed=(0, 0))


def dyadic_table(N, K, G, seed, allowed=0.5, absent=0.2):
    """random gains, multiples of 1/64 in (-0.25, 0.5) - so equal sums, ties, are frequent - a share of them -inf"""
    rng = np.random.default_rng(seed)
    gain = rng.integers(-16, 33, (N, G, K, K)) / 64.0
    gain[rng.random(gain.shape) > allowed] = -np.inf
    for g in range(1, G + 1):
        gain[:g, g - 1] = -np.inf
    size = np.where(rng.random((N, K)) < absent, np.nan, 1.0)
    return gain, size


@pytest.mark.parametrize("N", (1, 2, 63, 64, 65, 200))
def test_path_lengths(N):
    gain, size = dyadic_table(N, 4, 3, seed=N)
    for M, mf in ((1, 1), (3, 1), (3, 5)):
        assert_path(gain, size, M, mf, note=(N, M, mf))
    present = np.argwhere(~np.isnan(size))
    n0, k0 = (int(v) for v in present[len(present) // 2])
    assert_path(gain, size, 1, 1, seed=(n0, k0))
    assert_path(gain, size, 1, 1, seed=(N - 1, k0))


def test_path_constructed_tables():
    ninf = -np.inf
    N, K, G = 20, 5, 3
    ones = np.ones((N, K))
    ties = np.zeros((N, G, K, K))                                              # every link allowed at gain 0: nothing beats a start
    want = assert_path(ties, ones, 3, 1)
    assert want[0][:, 0].tolist() == [0, 1, 2] and (want[0][:, 1:] == -1).all() and want[2].tolist() == [1, 1, 1]
    assert_path(ties, ones, 3, 2)                                              # ... and no path has two nodes
    nothing = np.full((N, G, K, K), ninf)
    assert_path(nothing, ones, 2, 1)
    assert_path(nothing, np.full((N, K), np.nan), 2, 1)                        # nobody anywhere
    rng = np.random.default_rng(3)
    chain = np.full((N, G, K, K), ninf)
    ks = rng.integers(0, K, N)
    for n in range(1, N):
        chain[n, 0, ks[n - 1], ks[n]] = 0.25
    want = assert_path(chain, ones, 2, 1)
    assert want[0][0].tolist() == ks.tolist() and want[1][0] == 0.25 * (N - 1) and want[2][0] == N
    jumps = np.full((N, G, K, K), ninf)                                        # only lag-G links gain
    jumps[G:, G - 1] = rng.integers(1, 9, (N - G, K, K)) / 16.0
    jumps[G:, 0] = -0.125
    want = assert_path(jumps, ones, 3, 1)
    assert want[2][0] == len(range(0, N, G)) and set(np.diff(np.nonzero(want[0][0] >= 0)[0])) == {G}
    nan = np.where(rng.random((N, G, K, K)) < 0.3, np.nan, dyadic_table(N, K, G, 5)[0])      # a NaN never wins
    assert_path(nan, ones, 3, 1)


def test_path_every_lane_busy():
    gain, size = dyadic_table(24, 64, 8, seed=11, allowed=0.3, absent=0.0)
    want = assert_path(gain, size, 3, 1)
    assert (want[2] > 8).all()
    assert_path(gain, size, 1, 1, seed=(5, 63))
    gain, size = dyadic_table(16, 64, 8, seed=12, allowed=1.0, absent=0.5)
    assert_path(gain, size, 64, 1)


def test_path_exhaustion():
    gain, size = dyadic_table(30, 3, 2, seed=21, allowed=0.6)
    want = assert_path(gain, size, 64, 5)
    done = int((want[2] > 0).sum())
    assert 1 <= done < 64 and (want[2][done:] == 0).all() and np.isnan(want[1][done:]).all() and (want[0][done:] == -1).all()
    want = assert_path(gain, size, 64, 1)                                      # every present node ends up in some track
    assert int(want[2].sum()) == int((~np.isnan(size)).sum())


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("seed", CASE_A_SEEDS[:3])
def test_planted_case_a_end_to_end(seed):
    from pafuse_amd import harness, ops, tracks
    v = case_a(seed)
    want = tracks.track(v["x2d"], v["conf"], tracks=3)
    x, c = dev(v["x2d"], v["conf"])
    got = ops.track_people(x, c, tracks=3, want=ops.TRACK_OUTPUTS)
    assert rows(got["assign"].cpu().numpy()) == rows(v["truth"])
    assert torch.equal(got["assign"].cpu(), torch.from_numpy(want["assign"])) and torch.equal(got["frames"].cpu(), torch.from_numpy(want["frames"]))
    assert same_bits(got["x2d"].cpu(), torch.from_numpy(want["x2d"])) and same_bits(got["conf"].cpu(), torch.from_numpy(want["conf"]))
    own = tracks.path(got["gain"].cpu().numpy(), got["size"].cpu().numpy(), 3, 5)           # the score: exact on the kernel's own gains
    assert same_bits(got["score"].cpu(), torch.from_numpy(own[1])) and np.array_equal(own[0], want["assign"])
    assert np.allclose(own[1], want["score"], rtol=1e-12, atol=0)
    host = harness.track_people(v["x2d"], v["conf"], tracks=3)
    assert all(same_bits(host[k], got[k].cpu()) for k in ("x2d", "conf", "assign", "score", "frames"))
    # padding K with absent slots changes nothing
    pad = ops.track_people(torch.cat([x, torch.zeros_like(x[:, :3])], 1), torch.cat([c, torch.zeros_like(c[:, :3])], 1), tracks=3)
    assert all(same_bits(pad[k], got[k]) for k in ("x2d", "conf", "assign", "score", "frames"))
    # the torch op is the same entry
    import pafuse_amd.torch_ops  # noqa: F401
    op = torch.ops.pafuse.track_people(x, c, 3)
    assert all(same_bits(a, got[k]) for a, k in zip(op, ("x2d", "conf", "assign", "score", "frames")))
    if seed == 0:
        # a seed on every person: that person's row on both sides of the seed
        for p in range(3):
            truth = v["truth"][p]
            n0 = int(np.nonzero(truth >= 0)[0][30])
            s = ops.track_people(x, c, seed=(n0, int(truth[n0])))
            ref = tracks.track(v["x2d"], v["conf"], seed=(n0, int(truth[n0])))
            assert s["assign"].cpu()[0].tolist() == truth.tolist() and int(s["frames"][0]) == int((truth >= 0).sum())
            assert np.allclose(s["score"].cpu().numpy(), ref["score"], rtol=1e-12, atol=0) and same_bits(s["x2d"].cpu(), torch.from_numpy(ref["x2d"]))
            op = torch.ops.pafuse.track_people(x, c, 1, [n0, int(truth[n0])])
            assert same_bits(op[2], s["assign"]) and same_bits(op[3], s["score"])
        empty = np.argwhere(v["conf"].sum(-1) == 0)[0]
        s = ops.track_people(x, c, seed=(int(empty[0]), int(empty[1])))
        assert bool((s["assign"] == -1).all()) and bool(torch.isnan(s["score"]).all()) and int(s["frames"][0]) == 0 and not bool(s["x2d"].any())
        # a track goes straight into the screen and the repair
        m = 0
        chain = lambda tx, tc: harness.repair_detections(*[harness.screen_detections(tx, tc)[k] for k in ("x2d", "conf")], dataset=dataset())
        mine, ref = chain(host["x2d"][m], host["conf"][m]), chain(torch.from_numpy(want["x2d"][m]), torch.from_numpy(want["conf"][m]))
        assert all(same_bits(mine[k], ref[k]) for k in ("x2d", "conf", "status"))
        lost = host["assign"][m] < 0
        assert bool(lost.any()) and bool((mine["status"][lost] != 0).all())


def test_degenerate_inputs_on_the_device():
    from pafuse_amd import ops, tracks
    from tests.test_tracks_host import boxes
    for off, kw in ((np.zeros((1, 1)), dict(min_frames=1)), (np.zeros((1, 1)), {}), (np.full((6, 3), np.nan), dict(tracks=2, min_frames=1)),
                    (np.zeros((4, 2)), dict(tracks=3))):
        x, c = boxes(off)
        want = tracks.track(x, c, **kw)
        got = ops.track_people(*dev(x, c), want=ops.TRACK_OUTPUTS, **kw)
        assert all(same_bits(got[k].cpu(), torch.from_numpy(want[k])) for k in ops.TRACK_OUTPUTS), kw
    x, c = boxes(np.zeros((8, 2)))
    x[3, 0, 2, 0], x[4, 1], x[5, 0] = np.nan, np.nan, np.inf
    want = tracks.track(x, c, tracks=2, support=4, min_frames=1)
    got = ops.track_people(*dev(x, c), tracks=2, support=4, min_frames=1, want=ops.TRACK_OUTPUTS)
    assert all(same_bits(got[k].cpu(), torch.from_numpy(want[k])) for k in ops.TRACK_OUTPUTS)
    assert not bool(torch.isnan(got["gain"]).any())


# ------------------------------------------------------------------------------------------------------------ the example
def test_in_the_wild_follows_one_person(tmp_path):
    """two people listed in alternating order: --track lifts the detections of the one-person file of person 0"""
    from types import SimpleNamespace
    from __graft_entry__ import make_model
    from pafuse_amd import h3wb, harness
    from tests.golden import golden_util as gu
    ex = example()
    rng = np.random.default_rng(5)
    N = 40
    body = rng.uniform(0, 1, (2, 1, 133, 2)) * np.array([150.0, 400.0])
    centre = np.array([[250.0, 300.0], [700.0, 280.0]])[:, None, None] + 3.0 * np.arange(N)[None, :, None, None] * np.array([[[[1.0, 0.2]]], [[[-0.5, 0.1]]]])
    people = np.round(body + centre + rng.standard_normal((2, N, 133, 2)), 2)
    conf = np.round(rng.uniform(0.3, 1.0, (2, N, 133)), 3)
    entry = lambda p, n: {"keypoints": np.concatenate([people[p, n], conf[p, n, :, None]], axis=1).reshape(-1).tolist()}
    one, two = tmp_path / "one.json", tmp_path / "two.json"
    one.write_text("".join(json.dumps({"predictions": [entry(0, n)]}) + "\n" for n in range(N)))
    two.write_text("".join(json.dumps({"predictions": [entry(n % 2, n), entry(1 - n % 2, n)]}) + "\n" for n in range(N)))
    alone = ex.select_people(ex.parse_args(["--keypoints", str(one), "--out", str(tmp_path)]), 134)
    spliced = ex.select_people(ex.parse_args(["--keypoints", str(two), "--out", str(tmp_path)]), 134)
    followed = ex.select_people(ex.parse_args(["--keypoints", str(two), "--out", str(tmp_path), "--track", "--track-seed", "0:0"]), 134)
    both = ex.select_people(ex.parse_args(["--keypoints", str(two), "--out", str(tmp_path), "--track", "--people", "3"]), 134)
    assert len(alone) == len(spliced) == len(followed) == 1 and len(both) == 2
    assert not np.array_equal(spliced[0][0], alone[0][0])                                   # entry 0: a splice of both people
    assert np.array_equal(followed[0][0], alone[0][0]) and np.array_equal(followed[0][1], alone[0][1]) and followed[0][2] == str(tmp_path)
    table = np.load(tmp_path / "test_3d_output_track.npy")
    assert table.shape == (3, N) and (table[2] == -1).all() and {tuple(table[0]), tuple(table[1])} == {tuple(np.arange(N) % 2), tuple(1 - np.arange(N) % 2)}
    mine = [b for b in both if np.array_equal(b[0], alone[0][0])]
    assert len(mine) == 1 and mine[0][2].startswith(str(tmp_path / "person_"))
    # the video handed to the sampler, sampled once: P = 1, T = 1
    model, _ = make_model(1, 1, seed=83)
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES, parts_connection_indices=dict(gu.CONNECTION_INDICES))
    keypoints = h3wb.normalize_screen_coordinates(followed[0][0][..., :2], w=1000, h=1002).astype(np.float32)
    out = harness.infer_sequence(model, ds, keypoints, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2)
    assert out.shape == (2, 1, 1, 27, 134, 3) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ evaluate_frames
def test_evaluate_frames_with_distractors(tmp_path):
    """other people planted on a one-person video: slot 0 is a splice, track 0 is the subject - the same detections, the same score"""
    from __graft_entry__ import make_model
    from pafuse_amd import h3wb, harness, tracks
    from tests.golden import golden_util as gu
    from tests.test_hip_partials import sequence
    N = 60
    model = make_model(1, 1, depth=2)[0]
    model.noise_fn, model.noise = None, "device"
    _, seq_3d, cam = sequence(N)
    rng = np.random.default_rng(9)
    seq_2d = torch.from_numpy((rng.uniform(-1, 1, (1, 134, 2)) * np.array([0.1, 0.3]) + 0.1 * np.sin(np.arange(N) / 15.0)[:, None, None]
                               + 0.003 * rng.standard_normal((N, 134, 2))).astype(np.float32))
    def run(**kw):
        model.noise_seed = 2468                                                # every run draws the same noise: the call counter starts over
        return harness.evaluate_frames(model, dataset(), seq_2d, seq_3d, cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, stride=27, **kw)

    alone = run()
    spliced = run(distract=(2, 7))
    followed = run(distract=(2, 7), track=True)
    assert len(alone) == 2 and len(spliced) == len(followed) == 3
    crowd = tracks.plant_people(seq_2d.numpy(), np.ones((N, 134), np.float32), 3, seed=7)
    seen = spliced[2]
    assert bool((seen["tracked"] == 0).all()) and np.array_equal(seen["truth_slot"].numpy(), crowd["truth"][0])
    assert int((seen["truth_slot"] == 0).sum()) < N // 2 and same_bits(seen["x2d"], torch.from_numpy(crowd["x2d"][:, 0].copy()))
    seen = followed[2]
    assert torch.equal(seen["tracked"], seen["truth_slot"]) and same_bits(seen["x2d"], seq_2d) and bool((seen["conf"] == 1).all())
    assert all(torch.equal(followed[0][k], alone[0][k]) and torch.equal(followed[1][k], alone[1][k]) for k in alone[0])
    assert not all(torch.equal(spliced[0][k], alone[0][k]) for k in alone[0])
    lines = []
    rep = h3wb.evaluate_frames(model, dataset(), [cam.numpy()] * 2, [seq_3d.numpy()] * 2, [seq_2d.numpy()] * 2, gu.SYN_JOINTS_LEFT,
                               gu.SYN_JOINTS_RIGHT, stride=27, log=lines.append, distract=(2, 7), track=True)
    assert all(v == v for v in rep["mpjpe"])
    told = [l for l in lines if "track 0 among 3 people" in l]
    assert len(told) == 2 and all("in %d frames, another person's in 0, nobody in 0, 0 switches" % N in l for l in told)

"""Host side of the people tracker (no GPU): the numpy statement pafuse_amd/tracks.py, its planting helpers, the loader of
all people of a detection file, and the refusals of pafuse_tracks_* and of the Python layers, which happen before the first HIP
call.

Why the brute force can be exact.  The boxes below are 1/2 wide and 2 high, so size = sqrt(1) = 1; they move along x only, by
multiples of 1/8, with confidences 1 or 1/2: sqrt(dx*dx) = |dx| exactly, every weighted sum is dyadic, cost = |dx| and every
gain a multiple of 1/16.  Sums of such gains are exact in any order, so "the maximum over all admissible paths" has one value
and ties are frequent - which is what the tie rules are about.

Why planted case A is exact by construction.  The three people stay in lanes 0.6 apart and move 0.1 at most, so two different
people are never closer than 0.4 - 0.8 of their size of about 0.5, beyond the gate of 0.5 - while one person moves less than
0.02 a frame (cost below 0.1 over a lag of 4).  Ghosts sit at y = 2.  No link joins two people, every link of a person is
allowed, a dropout of at most G - 1 frames is bridged, and a link always gains more than the skip it costs: the three best
paths are the three people, whatever the rounding.
"""
import ctypes as C
import importlib.util
import itertools
import json
import os

import numpy as np
import pytest
import torch

from pafuse_amd import tracks
from tests.test_detections_host import bits, dataset, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
CASE_A_SEEDS = (0, 1, 2, 3, 4, 5)


# ------------------------------------------------------------------------------------------------------------ videos
def boxes(offsets, conf=None):
    """offsets [N,K] multiples of 1/8 (NaN: an empty slot) -> (x2d [N,K,5,2], conf [N,K,5]): a box 1/2 wide and 2 high (its
    corners and centre) per candidate, moved along x; exact in fp32"""
    offsets = np.asarray(offsets, dtype=np.float64)
    N, K = offsets.shape
    box = np.array([[0, 0], [0.5, 0], [0, 2], [0.5, 2], [0.25, 1]], dtype=np.float64)
    on = ~np.isnan(offsets)
    x = np.where(on[..., None, None], box[None, None] + np.stack([np.where(on, offsets, 0), np.zeros((N, K))], -1)[:, :, None], 0)
    c = np.where(on[..., None], np.float32(1) if conf is None else np.asarray(conf, dtype=np.float32), np.float32(0))
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    return x32, np.broadcast_to(c, (N, K, 5)).astype(np.float32).copy()


def case_a(seed, N=70, K=5, J=134, G=4):
    """planted case A -> plant_video's dict: three people in lanes, shuffled slots, dropouts of at most G - 1 frames, ghosts"""
    rng = np.random.default_rng(1000 + seed)
    P = 3
    body = rng.uniform(-1, 1, (P, 1, J, 2)) * np.array([0.15, 0.4])
    n = np.arange(N)[None, :, None]
    phase = rng.random((P, 1, 1))
    centre = np.stack([np.array([-0.6, 0.0, 0.6])[:, None, None] + 0.1 * np.sin(2 * np.pi * (n / 40.0 + phase)),
                       0.05 * np.sin(2 * np.pi * (n / 55.0 + phase))], axis=-1)                        # [P,N,1,2]
    px = (body + centre + 0.004 * rng.standard_normal((P, N, J, 2))).astype(np.float32)
    pc = rng.uniform(0.5, 1.0, (P, N, J)).astype(np.float32)
    pc[rng.random((P, N, J)) < 0.15] = 0                                                                # unobserved joints
    return tracks.plant_video(px, pc, slots=K, seed=seed, drop=(0.1, G - 1), ghost=(0.3, 2.0))


def crossing_case(seed, N=200, K=6, J=134):
    """the prototype's hard case: three people walking through each other on straight lines, a tenth of the detections
    dropped, a ghost in a fifth of the frames, six slots shuffled every frame"""
    rng = np.random.default_rng(2000 + seed)
    P = 3
    body = rng.uniform(-1, 1, (P, 1, J, 2)) * np.array([0.15, 0.4])
    n = np.arange(N)[None, :, None, None] / (N - 1.0)
    a, b = rng.uniform(-0.8, 0.8, (P, 1, 1, 2)), rng.uniform(-0.8, 0.8, (P, 1, 1, 2))
    px = (body + a + (b - a) * n + 0.004 * rng.standard_normal((P, N, J, 2))).astype(np.float32)
    pc = rng.uniform(0.5, 1.0, (P, N, J)).astype(np.float32)
    return tracks.plant_video(px, pc, slots=K, seed=seed, drop=(0.1, 1), ghost=(0.2, 2.0))


def rows(a):
    return {tuple(int(v) for v in r) for r in np.asarray(a)}


# ------------------------------------------------------------------------------------------------------------ the statement
def all_paths(gain, present):
    """every admissible path [(n, k), ...] of a gain table and its summed gain, by exhaustion"""
    N, G, K, _ = gain.shape
    nodes = [(n, k) for n in range(N) for k in range(K) if present[n, k]]

    def grow(path, score):
        yield path, score
        n, a = path[-1]
        for g in range(1, G + 1):
            if n + g < N:
                for b in range(K):
                    if present[n + g, b] and gain[n + g, g - 1, a, b] > -np.inf:
                        yield from grow(path + [(n + g, b)], score + gain[n + g, g - 1, a, b])

    for node in nodes:
        yield from grow([node], 0.0)


@pytest.mark.parametrize("seed", range(8))
def test_single_track_is_the_best_of_all_paths(seed):
    rng = np.random.default_rng(seed)
    N, K, G = int(rng.integers(2, 7)), int(rng.integers(1, 4)), int(rng.integers(1, 3))
    off = rng.integers(0, 6, (N, K)) / 8.0
    off[rng.random((N, K)) < 0.2] = np.nan
    x, c = boxes(off, conf=rng.choice([0.5, 1.0], (N, K, 1)))
    gain, size = tracks.links(x, c, gate=0.5, skip=1 / 16, max_gap=G, support=5)
    present = ~np.isnan(size)
    assert np.array_equal(present, ~np.isnan(off)) and (size[present] == 1.0).all()
    k16 = gain[gain > -np.inf] * 16
    assert np.array_equal(k16, np.round(k16))                                  # dyadic: every sum of gains is exact
    assign, score, frames = tracks.path(gain, size, 1, 1)
    if not present.any():
        assert (assign == -1).all() and np.isnan(score[0]) and frames[0] == 0
        return
    everything = list(all_paths(gain, present))
    top = max(s for _, s in everything)
    assert score[0] == top
    mine = [(n, int(k)) for n, k in enumerate(assign[0]) if k >= 0]
    assert (mine, top) in [(p, s) for p, s in everything if s == top] and frames[0] == len(mine)
    # the first maximum in (n, b) order: no maximal path ends at an earlier node
    assert min(p[-1] for p, s in everything if s == top) == mine[-1]


def test_tie_rules():
    ninf = -np.inf
    size = np.ones((3, 2))
    # every link allowed at gain exactly 0: extending never beats "start here" -> one node, the first in (n, b) order
    gain = np.zeros((3, 2, 2, 2))
    gain[0], gain[1, 1] = ninf, ninf
    assign, score, frames = tracks.path(gain, size, 1, 1)
    assert assign.tolist() == [[0, -1, -1]] and score[0] == 0.0 and frames[0] == 1
    # two ways to the same total at (2, 0): lag 1 from (1, 1) and lag 2 from (0, 0) -> the lower g; then the lower a
    gain = np.full((3, 2, 2, 2), ninf)
    gain[1, 0, 0, 1] = 0.25                       # (0,0) -> (1,1)
    gain[2, 0, 1, 0] = 0.25                       # (1,1) -> (2,0): total 0.5
    gain[2, 1, 0, 0] = 0.5                        # (0,0) -> (2,0) over lag 2: total 0.5
    assert tracks.path(gain, size, 1, 1)[0].tolist() == [[0, 1, 0]]
    gain[2, 0, 1, 0] = ninf
    gain[1, 0, 0, 0] = 0.25                       # (0,0) -> (1,0)
    gain[2, 0, 0, 0] = gain[2, 0, 1, 0] = 0.25    # (1,0) -> (2,0) and (1,1) -> (2,0): the lower a
    assert tracks.path(gain, size, 1, 1)[0].tolist() == [[0, 0, 0]]
    # two ends with the same score: the first in (n, b) order; a NaN gain never wins
    gain = np.full((3, 2, 2, 2), ninf)
    gain[1, 0, 0, 0] = gain[1, 0, 0, 1] = 0.5
    gain[2, 0, 1, 1] = np.nan
    assert tracks.path(gain, size, 1, 1)[0].tolist() == [[0, 0, -1]]
    # greedy rounds mark their nodes used; a round below min_frames ends the extraction for good
    assign, score, frames = tracks.path(gain, size, 4, 2)
    assert assign.tolist() == [[0, 0, -1]] + [[-1] * 3] * 3 and frames.tolist() == [2, 0, 0, 0]
    assert score[0] == 0.5 and np.isnan(score[1:]).all()
    assign, score, frames = tracks.path(gain, size, 3, 1)
    assert assign.tolist() == [[0, 0, -1], [1, -1, -1], [-1, 1, -1]] and score.tolist() == [0.5, 0.0, 0.0]


@pytest.mark.parametrize("seed", CASE_A_SEEDS)
def test_planted_case_a_comes_back_exactly(seed):
    v = case_a(seed)
    assert (v["truth"] >= 0).all(axis=0).sum() < 70 and (v["truth"] == -1).any()          # people are dropped at times
    out = tracks.track(v["x2d"], v["conf"], tracks=3, min_frames=5)
    assert rows(out["assign"]) == rows(v["truth"])
    assert (out["frames"] == (v["truth"] >= 0).sum(axis=1)[[list(map(tuple, v["truth"])).index(tuple(r)) for r in out["assign"]]]).all()
    err = tracks.track_error(out["assign"], v["truth"])
    assert all(e["wrong"] == 0 and e["missed"] == 0 and e["switches"] == 0 for e in err) and sorted(e["person"] for e in err) == [0, 1, 2]
    assert (np.diff(out["score"]) <= 0).all()                                              # greedy: best first


def test_slot_zero_is_a_splice_and_the_crossing_case_is_reported():
    v = case_a(0)
    held = int((v["truth"][0] == 0).sum())
    assert held < 0.4 * 70, held                      # what predictions[0] lifts: person 0 in about a fifth of the frames
    for seed in range(2):
        c = crossing_case(seed)
        out = tracks.track(c["x2d"], c["conf"], tracks=3)
        print("crossing case, seed", seed, "slot 0 holds person 0 in", int((c["truth"][0] == 0).sum()), "of 200 frames;",
              tracks.track_error(out["assign"], c["truth"]))


@pytest.mark.parametrize("person", range(3))
def test_seeded_track_follows_the_seeds_person(person):
    v = case_a(1)
    truth = v["truth"][person]
    n0 = int(np.nonzero(truth >= 0)[0][30])
    out = tracks.track(v["x2d"], v["conf"], seed=(n0, int(truth[n0])))
    assert np.array_equal(out["assign"][0], truth) and out["frames"][0] == (truth >= 0).sum()
    free = tracks.track(v["x2d"], v["conf"], tracks=3)
    m = [tuple(r) for r in free["assign"]].index(tuple(truth))
    assert abs(out["score"][0] - free["score"][m]) < 1e-9 * free["score"][m]              # the same links, summed in another order
    ghost = np.argwhere((v["conf"].sum(-1) == 0))[0]                                       # an empty slot as the seed: no track
    out = tracks.track(v["x2d"], v["conf"], seed=tuple(int(i) for i in ghost))
    assert (out["assign"] == -1).all() and np.isnan(out["score"][0]) and out["frames"][0] == 0


def test_degenerate_inputs():
    x, c = boxes(np.zeros((1, 1)))
    out = tracks.track(x, c, min_frames=1)                                                 # N = 1, K = 1
    assert out["assign"].tolist() == [[0]] and out["score"][0] == 0.0 and out["frames"][0] == 1
    assert tracks.track(x, c)["assign"].tolist() == [[-1]]                                 # fewer than min_frames
    x, c = boxes(np.full((6, 3), np.nan))                                                  # all absent
    out = tracks.track(x, c, tracks=2, min_frames=1)
    assert (out["assign"] == -1).all() and np.isnan(out["score"]).all() and not out["x2d"].any() and not out["conf"].any()
    assert np.isnan(out["size"]).all() and (out["gain"] == -np.inf).all()
    x, c = boxes(np.zeros((8, 2)))
    x[3, 0, 2, 0] = np.nan                                                                 # a NaN under a positive confidence:
    x[4, 1] = np.nan                                                                       # the joint, or the candidate, is unobserved
    x[5, 0] = np.inf
    out = tracks.track(x, c, tracks=2, support=4, min_frames=1)
    assert not np.isnan(out["x2d"][out["assign"] >= 0][:, [0, 1, 3, 4]]).any() and np.isnan(out["size"][4, 1]) and np.isnan(out["size"][5, 0])
    assert np.isfinite(out["score"]).all() and not np.isnan(out["gain"]).any()
    empty = out["assign"] < 0
    assert not out["x2d"][empty].any() and not out["conf"][empty].any()
    assert out["assign"][:, 4].tolist().count(-1) == 1 and out["assign"][:, 5].tolist().count(-1) == 1


def test_gather_moves_bits():
    v = case_a(2, N=12)
    x, c = v["x2d"].copy(), v["conf"].copy()
    x.view(np.uint32)[3, 1, 7, 0] = 0x7fc12345                                             # a NaN payload survives the gather
    assign = np.array([[1] * 12, [-1, 0, 4, 2] * 3], dtype=np.int32)
    gx, gc = tracks.gather(x, c, assign)
    for m, n in itertools.product(range(2), range(12)):
        k = assign[m, n]
        if k < 0:
            assert not gx[m, n].any() and not gc[m, n].any()
        else:
            assert np.array_equal(bits(gx[m, n]), bits(x[n, k])) and np.array_equal(bits(gc[m, n]), bits(c[n, k]))


def test_planting_helpers():
    v = case_a(3)
    x, c, truth = v["x2d"], v["conf"], v["truth"]
    assert x.shape == (70, 5, 134, 2) and c.shape == (70, 5, 134) and truth.shape == (3, 70)
    for n in range(70):
        held = truth[:, n][truth[:, n] >= 0]
        assert len(set(held)) == len(held)                                                 # no slot holds two people
    gone = truth < 0
    run = max(len(list(g)) for p in range(3) for k, g in itertools.groupby(gone[p]) if k)
    assert 1 <= run <= 3 and not gone[:, 0].any() and not gone[:, -1].any()
    ghosts = (c.sum(-1) > 0).sum(1) - (truth >= 0).sum(0)
    assert set(ghosts) == {0, 1} and 8 <= ghosts.sum() <= 35 and (x[..., 1][c > 0].max() > 1.5)
    one_x, one_c = x[np.arange(70), np.where(truth[0] >= 0, truth[0], 0)], c[np.arange(70), np.where(truth[0] >= 0, truth[0], 0)]
    two = tracks.plant_people(one_x, one_c, 3, seed=5, slots=4)
    assert two["x2d"].shape == (70, 4, 134, 2) and (two["truth"] >= 0).all()
    assert np.array_equal(bits(two["x2d"][np.arange(70), two["truth"][0]]), bits(one_x))
    shifted = two["x2d"][np.arange(70), two["truth"][1]] - one_x
    assert (shifted[..., 1] == 0).all() and (shifted[..., 0][one_c > 0] > 0.3).all()
    other = tracks.plant_people(one_x, one_c, 2, seed=5, others=[(one_x[:10] + 5, one_c[:10])])
    assert np.array_equal(other["x2d"][np.arange(70), other["truth"][1]], np.tile(one_x[:10] + 5, (7, 1, 1)))
    with pytest.raises(ValueError, match="plant_video"):
        tracks.plant_video(x[:, :3].transpose(1, 0, 2, 3), c[:, :3].transpose(1, 0, 2), slots=2)
    e = tracks.track_error(np.array([0, 0, 1, -1, 1, 2]), np.array([0, 0, 0, 0, 1, -1]))
    assert e == {"right": 3, "wrong": 2, "missed": 1, "switches": 3}
    both = tracks.track_error(np.array([[0, 0, 1], [-1, -1, -1]]), np.array([[5, 5, 5], [0, 0, 0]]))
    assert both[0]["person"] == 1 and both[0]["right"] == 2 and both[1]["person"] == -1 and both[1]["missed"] == 3


# ------------------------------------------------------------------------------------------------------------ the loader
def test_load_pifpaf_people(tmp_path):
    from pafuse_amd import harness
    rng = np.random.default_rng(0)
    person = lambda: {"keypoints": np.round(rng.uniform(1, 900, 133 * 3), 2).tolist()}
    frames = [[person(), person()], [person()], [], [person(), person(), person()]]
    path = tmp_path / "people.json"
    path.write_text("".join(json.dumps({"predictions": f}) + "\n" for f in frames) + "\n")
    kps, conf = harness.load_pifpaf_people(str(path))
    assert kps.shape == (4, 3, 134, 2) and conf.shape == (4, 3, 134) and kps.dtype == conf.dtype == np.float32
    assert not kps[2].any() and not conf[2].any() and not kps[1, 1:].any() and not conf[0, 2].any()
    flat = np.asarray(frames[3][2]["keypoints"], dtype=np.float32).reshape(133, 3)
    assert np.array_equal(kps[3, 2, 1:], flat[:, :2]) and np.array_equal(conf[3, 2, 1:], flat[:, 2])
    assert np.array_equal(kps[3, 2, 0], (kps[3, 2, 12] + kps[3, 2, 13]) / 2) and conf[3, 2, 0] == min(conf[3, 2, 12], conf[3, 2, 13])
    capped = harness.load_pifpaf_people(str(path), max_people=2)
    assert capped[0].shape == (4, 2, 134, 2) and np.array_equal(capped[0], kps[:, :2]) and np.array_equal(capped[1], conf[:, :2])
    with pytest.raises(ValueError, match="max_people"):
        harness.load_pifpaf_people(str(path), max_people=0)
    with pytest.raises(IndexError):                                                        # the one-person loader raises there
        harness.load_pifpaf_keypoints(str(path))
    full = tmp_path / "full.json"
    full.write_text("".join(json.dumps({"predictions": f}) + "\n" for f in frames if f))
    one_k, one_c = harness.load_pifpaf_keypoints(str(full), with_conf=True)
    kps, conf = harness.load_pifpaf_people(str(full))
    assert np.array_equal(bits(kps[:, 0]), bits(one_k)) and np.array_equal(bits(conf[:, 0]), bits(one_c))
    none = tmp_path / "none.json"
    none.write_text(json.dumps({"predictions": []}) + "\n")
    kps, conf = harness.load_pifpaf_people(str(none))
    assert kps.shape == (1, 1, 134, 2) and not kps.any() and not conf.any()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_symbols_and_workspace():
    L = lib()
    from pafuse_amd import _lib
    assert L.pafuse_abi_version() == 8 == _lib.ABI_VERSION
    for name in ("pafuse_tracks_workspace_bytes", "pafuse_tracks_links", "pafuse_tracks_path", "pafuse_tracks_gather"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    with open(os.path.join(ROOT, "include", "pafuse_hip.h")) as f:
        header = f.read()
    assert "#define PAFUSE_ABI_VERSION 8" in header and all(f" {n}(" in header for n in ("pafuse_tracks_links", "pafuse_tracks_path", "pafuse_tracks_gather"))
    for N, K, J, G in ((1, 1, 1, 1), (7, 3, 134, 4), (5000, 16, 134, 4), (12, 64, 5, 8)):
        want = 8 * N * G * K * K + 8 * N * K + 2 * N * K + N * K
        assert L.pafuse_tracks_workspace_bytes(N, K, J, G) == (want + 7) // 8 * 8
    assert L.pafuse_tracks_workspace_bytes(5000, 16, 134, 4) // 10 ** 6 == 41             # the header's figure
    assert L.pafuse_tracks_workspace_bytes(5000, 64, 134, 8) > 1.3e9
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 9)):
        assert L.pafuse_tracks_workspace_bytes(*bad) == 0


def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call; the buffers stay untouched"""
    L = lib()
    N, K, J, G, M = 4, 3, 5, 2, 2
    need = L.pafuse_tracks_workspace_bytes(N, K, J, G)
    buf = (C.c_float * 4096)()
    for i in range(4096):
        buf[i] = 7.0
    p = C.addressof(buf)
    x, c, asg, sc, fr, out, cout, ws = p, p + 1024, p + 2048, p + 2304, p + 2432, p + 2560, p + 3584, p + 8192
    assert need <= 8192
    nan, inf = float("nan"), float("inf")
    # x2d, conf, N, K, J, G, support, threshold, gate, skip, workspace, bytes, stream
    ok = [x, c, N, K, J, G, 5, 0.0, 0.5, 0.05, ws, need, None]
    for i, v in [(0, None), (1, None), (2, 0), (2, -1), (3, 0), (3, 65), (4, 0), (5, 0), (5, 9), (6, 0), (6, 65536), (7, -0.5), (7, nan),
                 (7, inf), (8, 0.0), (8, -1.0), (8, nan), (8, inf), (9, -0.01), (9, nan), (9, inf), (10, None), (10, ws + 4), (11, need - 1),
                 (11, 0)]:
        a = list(ok)
        a[i] = v
        assert L.pafuse_tracks_links(*a) == E_ARG, (i, v)
        assert b"tracks_links" in L.pafuse_last_error(), (i, v)
    a = list(ok)
    a[2], a[11] = 2 ** 31 - 1, 2 ** 63                                        # N*G*K / 4 workgroups do not fit a grid
    a[3], a[5] = 64, 8
    assert L.pafuse_tracks_links(*a) == E_ARG and b"grid" in L.pafuse_last_error()
    # gain, size, N, K, G, M, min_frames, seed_n, seed_k, assign, score, frames, workspace, bytes, stream
    ok = [None, None, N, K, G, M, 5, -1, -1, asg, sc, fr, ws, need, None]
    for i, v in [(9, None), (10, None), (11, None), (2, 0), (3, 0), (3, 65), (4, 0), (4, 9), (5, 0), (5, 65), (6, 0), (6, -3), (7, N), (7, 0),
                 (8, K), (8, 1), (12, None), (12, ws + 4), (13, need - 1), (0, ws + 4), (1, ws + 4)]:
        a = list(ok)
        a[i] = v
        assert L.pafuse_tracks_path(*a) == E_ARG, (i, v)
        assert b"tracks_path" in L.pafuse_last_error(), (i, v)
    a = list(ok)
    a[7], a[8] = 1, 1                                                         # a seed names one person
    assert L.pafuse_tracks_path(*a) == E_ARG and b"seed" in L.pafuse_last_error()
    for seed in ((N, 0), (0, K), (-1, 0), (0, -1), (-2, 0)):
        a = list(ok)
        a[5], a[7], a[8] = 1, seed[0], seed[1]
        assert L.pafuse_tracks_path(*a) == E_ARG and b"seed" in L.pafuse_last_error(), seed
    a = list(ok)
    a[2], a[3], a[4], a[13] = 2 ** 31 - 1, 64, 8, 2 ** 63
    assert L.pafuse_tracks_path(*a) == E_ARG and b"grid" in L.pafuse_last_error()
    # x2d, conf, assign, N, K, J, M, out, conf_out, stream
    ok = [x, c, asg, N, K, J, M, out, cout, None]
    for i, v in [(0, None), (1, None), (2, None), (7, None), (8, None), (3, 0), (4, 0), (4, 65), (5, 0), (6, 0), (6, 65)]:
        a = list(ok)
        a[i] = v
        assert L.pafuse_tracks_gather(*a) == E_ARG, (i, v)
        assert b"tracks_gather" in L.pafuse_last_error(), (i, v)
    a = list(ok)
    a[3], a[5], a[6] = 2 ** 31 - 1, 2 ** 31 - 1, 64
    assert L.pafuse_tracks_gather(*a) == E_ARG and b"grid" in L.pafuse_last_error()
    assert all(v == 7.0 for v in buf)


def test_python_layers_refuse_before_touching_the_device():
    lib()
    from pafuse_amd import harness, ops
    z = torch.zeros
    x, c = z(6, 3, 7, 2), z(6, 3, 7)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.track_people(x, c)
    with pytest.raises(ValueError, match="conf must be"):
        ops.track_people(x, z(6, 3, 6))
    with pytest.raises(ValueError, match="x2d must be"):
        ops.track_people(z(6, 7, 2), z(6, 7))
    with pytest.raises(ValueError, match="K must lie"):
        ops.track_people(z(2, 65, 7, 2), z(2, 65, 7))
    nan, inf = float("nan"), float("inf")
    for key, values in (("tracks", (0, 65, 1.5, True)), ("max_gap", (0, 9, 2.5)), ("support", (0, 65536, 2.5)), ("min_frames", (0, -1, 1.5)),
                        ("gate", (0.0, -1.0, nan, inf)), ("skip", (-0.1, nan, inf)), ("threshold", (-1.0, nan, inf))):
        for v in values:
            with pytest.raises(ValueError, match=key):
                ops.track_people(x, c, **{key: v})
    for seed in ((6, 0), (0, 3), (-1, 0)):
        with pytest.raises(ValueError, match="seed"):
            ops.track_people(x, c, seed=seed)
    with pytest.raises(ValueError, match="one person"):
        ops.track_people(x, c, seed=(0, 0), tracks=2)
    with pytest.raises(ValueError, match="want"):
        ops.track_people(x, c, want=("x2d", "mean"))
    with pytest.raises(ValueError, match="kps must be"):
        harness.track_people(z(6, 7, 2), z(6, 7))
    with pytest.raises(ValueError, match="assign must be"):
        ops.gather_tracks(x, c, z(2, 5, dtype=torch.int32))
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    ev = (model, dataset(), z(60, 134, 2), z(60, 134, 3), z(9), [], [])
    with pytest.raises(ValueError, match="track needs distract"):
        harness.evaluate_frames(*ev, track=True)
    for bad in (2, (0, 1), (64, 1), (1.5, 0), (True, 0), (1, 2, 3)):
        with pytest.raises(ValueError, match="distract"):
            harness.evaluate_frames(*ev, distract=bad)
    with pytest.raises(ValueError, match="track must be"):
        harness.evaluate_frames(*ev, distract=(1, 0), track="yes")


def test_torch_op_has_a_schema_and_a_fake():
    import pafuse_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.pafuse.track_people.default._schema)
    assert "Tensor x2d, Tensor conf" in s and "tracks=1" in s and "[]? seed=None" in s and "float gate=0.5" in s and "max_gap=4" in s
    assert "support=5" in s and "min_frames=5" in s and "float threshold=0." in s
    assert s.endswith("-> Tensor[]")
    with FakeTensorMode():
        x, conf, assign, score, frames = torch.ops.pafuse.track_people(torch.empty(9, 4, 7, 2, device="cuda"), torch.empty(9, 4, 7, device="cuda"), 3)
        assert x.shape == (3, 9, 7, 2) and conf.shape == (3, 9, 7) and assign.shape == (3, 9) and score.shape == frames.shape == (3,)
        assert x.dtype == conf.dtype == torch.float32 and assign.dtype == frames.dtype == torch.int32 and score.dtype == torch.float64


def example():
    spec = importlib.util.spec_from_file_location("infer_in_the_wild_example", os.path.join(ROOT, "examples", "infer_in_the_wild.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_flags(capsys):
    ex = example()
    a = ex.parse_args([])
    assert not a.track and a.people is None and a.track_seed is None and (a.track_gate, a.track_gap, a.track_skip) == (0.5, 4, 0.05)
    a = ex.parse_args(["--track", "--people", "3", "--track-gap", "8", "--track-gate", "0.25", "--track-skip", "0"])
    assert a.track and a.people == 3 and (a.track_gate, a.track_gap, a.track_skip) == (0.25, 8, 0.0)
    assert ex.parse_seed(ex.parse_args(["--track", "--track-seed", "12:1", "--people", "1"]).track_seed) == (12, 1)
    for argv, word in ((["--people", "2"], "need --track"), (["--track-seed", "0:0"], "need --track"),
                       (["--track", "--track-seed", "3"], "FRAME:PERSON"), (["--track", "--track-seed", "-1:0"], "FRAME:PERSON"),
                       (["--track", "--track-seed", "a:b"], "FRAME:PERSON"), (["--track", "--track-seed", "1:0", "--people", "2"], "one person"),
                       (["--track", "--people", "0"], "1 .. 64"), (["--track", "--people", "65"], "1 .. 64"),
                       (["--track", "--track-gap", "0"], "--track-gap"), (["--track", "--track-gap", "9"], "--track-gap"),
                       (["--track", "--track-gate", "0"], "--track-gate"), (["--track", "--track-gate", "nan"], "--track-gate"),
                       (["--track", "--track-skip", "-1"], "--track-skip"), (["--track", "--track-skip", "inf"], "--track-skip")):
        with pytest.raises(SystemExit) as e:
            ex.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv

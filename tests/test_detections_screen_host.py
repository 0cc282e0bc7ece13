"""Host side of the screening of observed 2-D detections (no GPU): the numpy statement pafuse_amd/detscreen.py, its helpers, and the
refusals of pafuse_detections_screen and of the Python layers, which happen before the first HIP call.

Why the exact cases can be exact.  r = 3: (r+1)^2 = 16, so the taper g = (1 - d*d/16)^2 is dyadic.  The planted coordinates are
multiples of 2^-6 below 32 and the confidences 1 or 0.5, so every product and sum of the walk is exact in fp64, a series a + b*d
gives S2*Q0 - S1*Q1 = a*D exactly and the divide returns a, bit for bit (tests/test_detections_host.py).  A detection on a line
whose accepted neighbours are on that line therefore has the residual 0, exactly.

The caps on the planted case (at least 95 % of the outliers rejected, at most 1 % of the untouched detections rejected, no false
swap, every status-2 frame the truth's bits) are conditions on the statement alone, not measurements; DESIGN.md section 6o has
the observed counts (299 of 309 rejected, 15 of 5 619 false rejects).  The planting is dense - a tenth of all detections wrong -
and the scale comes from pass 1, whose residuals the planted errors inflate: the outliers it misses are the smallest, 0.05 - 0.1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_detections_host import bits, dataset, lib

E_ARG = -1
# The exact cases run at r = 3, where a window holds 6 neighbours.  The middle frame of a 5-frame run sees 2 accepted ones, and the
# neighbours of a run are re-admitted from the outside in, one frame per pass and side once fewer than `support` accepted frames are
# in reach: with support = 2 three passes re-admit all of them, with the default 3 (meant for r = 13) they do not.
SUPPORT_EXACT = 2
MIRROR6 = [1, 0, 3, 2, -1, -1]


def exact_lines(N=40, J=6):
    """dyadic lines per joint with confidences 1 or 0.5; the pairs (0, 1) and (2, 3) are 4 apart -> (x2d, conf), exact in fp32"""
    t = np.arange(N, dtype=np.float64)
    a = np.array([1.0, 5.0, 2.0, 6.0, 3.0, 7.0])[:J]
    b = np.array([1 / 8, -1 / 16, 1 / 32, 1 / 8, -1 / 8, 1 / 64])[:J]
    x = np.stack([a[None, :] + b[None, :] * t[:, None], (a[None, :] / 2) - (b[None, :] / 2) * t[:, None]], axis=-1)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    conf = np.where((np.arange(N * J).reshape(N, J) % 3) == 0, np.float32(0.5), np.float32(1)).astype(np.float32)
    return x32, conf


def planted_exact():
    """-> (x2d, conf, truth x2d, truth conf, swapped frames of the pair (0, 1), outlier frames of joint 4): a 5-frame swap and a
    3-frame outlier on exact lines, r = 3"""
    truth, conf = exact_lines()
    x, c = truth.copy(), conf.copy()
    swapped, out = np.arange(10, 15), np.arange(25, 28)
    x[swapped, 0], x[swapped, 1] = truth[swapped, 1], truth[swapped, 0]
    c[swapped, 0], c[swapped, 1] = conf[swapped, 1], conf[swapped, 0]
    x[out, 4] += np.float32(2.0)
    return x, c, truth, conf, swapped, out


def noisy_video(N=300, J=20, seed=1):
    """smooth motion with 0.004 noise; the pairs (2k, 2k+1) of the first 16 joints are 0.6 apart -> (x2d, conf, mirror)"""
    rng = np.random.default_rng(seed)
    t = np.arange(N)[:, None, None] / 30.0
    centre = rng.uniform(-0.3, 0.3, (1, J, 2))
    centre[0, 1:16:2] = centre[0, 0:16:2] + np.array([0.6, 0.0])
    motion = 0.1 * np.sin(2 * np.pi * (0.1 * t + rng.random((1, J, 2)))) + 0.01 * t * rng.uniform(-1, 1, (1, J, 2))
    x = (centre + motion + rng.normal(0.0, 0.004, (N, J, 2))).astype(np.float32)
    conf = rng.uniform(0.5, 1.0, (N, J)).astype(np.float32)
    mirror = np.full(J, -1, dtype=np.int32)
    mirror[0:16:2], mirror[1:16:2] = np.arange(1, 16, 2), np.arange(0, 16, 2)
    return x, conf, mirror


# ------------------------------------------------------------------------------------------------------------ the statement
def test_leave_one_out_fit_is_local_line_with_the_frame_weighted_0():
    from pafuse_amd import detscreen, trajectory
    x, conf = exact_lines()
    rng = np.random.default_rng(0)
    x = x + (rng.integers(-8, 9, x.shape) / 64).astype(np.float32)          # dyadic, off the lines: the fit has work to do
    acc = rng.random(conf.shape) < 0.8
    x64, w64 = x.astype(np.float64), conf.astype(np.float64)
    pred, fit = detscreen.loo_line(x64, w64, acc, 3, 2)
    for n in range(x.shape[0]):
        w0 = w64.copy()
        w0[n] = 0.0                                                           # frame n takes part with weight 0: it adds 0.0, exactly
        value, code = trajectory.local_line(x64, acc | (np.arange(x.shape[0]) == n)[:, None], w0, 3)
        line = code[n] == trajectory.LINE
        assert np.array_equal(fit[n], line)
        assert np.array_equal(pred[n][line], value[n][line])
    assert fit.sum() > 200
    assert not detscreen.loo_line(x64, w64, acc, 3, 7)[1].any()              # 2r = 6 neighbours at the most


def test_median_rule():
    from pafuse_amd import detscreen
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rng = np.random.default_rng(1)
    for c in (1, 2, 3, 4, 7, 64, 65):
        v = rng.integers(0, 5, c).astype(np.float32)                          # ties
        assert detscreen.lower_median(v) == np.sort(v)[(c - 1) // 2]
        w = np.concatenate([v, [nan, nan]]).astype(np.float32)
        rng.shuffle(w)
        assert detscreen.lower_median(w) == np.sort(v)[(c - 1) // 2]          # NaN takes no part
    assert detscreen.lower_median([nan, 3.0, nan]) == 3.0
    assert detscreen.lower_median([nan, nan]) == 0.0 and detscreen.lower_median([]) == 0.0
    assert detscreen.lower_median([inf, 1.0]) == 1.0 and detscreen.lower_median([inf, inf, 1.0]) == inf
    assert detscreen.lower_median([inf, nan]) == inf
    x, conf = exact_lines(9, 2)
    x[4, 0] += 1.0
    e = detscreen.screen(x, conf, None, 3, gate=1e6, passes=1, support=2)[3]       # nothing is rejected: resid is e_1
    tau = detscreen.screen(x, conf, None, 3, gate=2.0, floor=0.25, passes=1, support=2)[4]
    assert e[4, 0] > 0.5 and tau[0] == np.float32(2.0 * max(1.4826 * float(np.sort(e[:, 0])[4]), 0.25)) > 0.5 and tau[1] == 0.5


def test_a_clean_exact_line_is_accepted_everywhere():
    from pafuse_amd import detscreen
    x, conf = exact_lines()
    out, conf_out, status, resid, scale = detscreen.screen(x, conf, MIRROR6, 3)
    assert (resid == 0).all() and (status == 0).all()
    assert np.array_equal(scale, np.full(6, np.float32(np.float64(np.float32(4.0)) * np.float64(np.float32(0.005)))))
    assert np.array_equal(bits(out), bits(x)) and np.array_equal(bits(conf_out), bits(conf))
    assert out.dtype == conf_out.dtype == resid.dtype == scale.dtype == np.float32 and status.dtype == np.uint8


def test_planted_exact_swap_and_outlier_are_restored():
    from pafuse_amd import detscreen
    x, c, truth, conf, swapped, outl = planted_exact()
    out, conf_out, status, resid, scale = detscreen.screen(x, c, MIRROR6, 3, support=SUPPORT_EXACT)
    want = np.zeros(status.shape, np.uint8)
    want[swapped, 0] = want[swapped, 1] = 2
    want[outl, 4] = 1
    assert np.array_equal(status, want)
    keep = status != 1
    assert np.array_equal(bits(out[keep]), bits(truth[keep])) and np.array_equal(bits(conf_out[keep]), bits(conf[keep]))
    assert (conf_out[status == 1] == 0).all() and np.array_equal(bits(out[status == 1]), bits(x[status == 1]))
    assert np.array_equal(detscreen.counts(status), [40 * 6 - 13, 3, 10, 0])
    # without a table the swapped frames are outliers of both tracks
    status0 = detscreen.screen(x, c, None, 3, support=SUPPORT_EXACT)[2]
    assert (status0[swapped, :2] == 1).all() and (status0 != 2).all()


def test_statuses_and_untouched_bits():
    from pafuse_amd import detscreen
    x, conf = exact_lines()
    conf[5, 0] = 0                                       # lost
    x[6, 1, 0] = np.nan                                  # a NaN coordinate under a positive confidence: not observed
    conf[:, 5] = 0
    conf[[13, 20], 5] = 1                                # observed twice, 7 frames apart: no neighbour in reach, never tested
    x[13, 5] += 100.0
    x[13, 2] = x[13, 3]                                  # a pair that coincides in one frame: no swap, whatever is rejected
    out, conf_out, status, resid, scale = detscreen.screen(x, conf, MIRROR6, 3, support=SUPPORT_EXACT)
    assert status[5, 0] == 3 and status[6, 1] == 3 and np.isnan(resid[5, 0]) and np.isnan(resid[6, 1])
    assert (status[:, 5] == np.where(conf[:, 5] > 0, 0, 3)).all() and np.isnan(resid[:, 5]).all() and scale[5] == np.float32(0.02)
    assert status[13, 2] == 1 and status[13, 3] == 0 and (status != 2).all() and int((status == 1).sum()) == 1
    assert np.array_equal(bits(out), bits(x))            # nothing swapped: every bit kept, the NaN included
    assert np.array_equal(conf_out == 0, (status == 1) | (conf == 0))
    assert np.array_equal(np.isnan(resid), (status == 3) | (np.arange(6) == 5)[None, :])


def test_planted_outliers_and_swaps_are_found():
    """the conditions of DESIGN.md section 6o, on 300 x 20 with seed 1: the observed counts are printed"""
    from pafuse_amd import detscreen
    x, conf, mirror = noisy_video()
    bad = detscreen.corrupt(x, conf, mirror, outliers=(0.04, 1, (0.05, 0.6), 11), swaps=(0.02, 4, 12))
    runs, shift = detscreen.plant_outliers(300, 20, 0.008, 4, 0.3, 13)
    runs &= ~bad["planted_swap"] & ~bad["planted_out"]
    xin = np.where(runs[..., None], bad["x2d"] + shift, bad["x2d"]).astype(np.float32)
    planted_out = bad["planted_out"] | runs
    res = {}
    for name, kw in (("default", {}), ("one pass", dict(passes=1)), ("gate 6", dict(gate=6.0))):
        out, conf_out, status, _, _ = detscreen.screen(xin, bad["conf"], mirror, 13, **kw)
        err = detscreen.screen_error(status, planted_out, bad["planted_swap"])
        restored = int(((status == 2) & bad["planted_swap"] & (bits(out) == bits(x)).all(-1) & (bits(conf_out) == bits(conf))).sum())
        print(f"{name}: {err}; restored bit for bit {restored}")
        res[name] = (err, status, out, conf_out)
    err, status, out, conf_out = res["default"]
    n_out, n_swap = int(planted_out.sum()), int(bad["planted_swap"].sum())
    assert n_out > 150 and n_swap > 40
    assert err["out_found"] >= 0.95 * n_out
    assert err["false_rejects"] <= 0.01 * err["untouched"]
    two = status == 2
    assert two.any() and np.array_equal(bits(out[two]), bits(x[two])) and np.array_equal(bits(conf_out[two]), bits(conf[two]))
    assert err["false_swaps"] == 0
    assert np.array_equal(bits(out[~two]), bits(xin[~two]))                 # everything else keeps its coordinates
    assert res["default"][0]["false_rejects"] < res["one pass"][0]["false_rejects"]      # the passes re-admit the neighbours
    clean = detscreen.screen(x, conf, mirror, 13)[2]
    print(f"clean video: {detscreen.counts(clean).tolist()}")
    assert int((clean == 1).sum()) <= 0.01 * clean.size and int((clean == 2).sum()) == 0


def test_check_mirror_and_mirror_table():
    from pafuse_amd import detscreen
    J = 6
    assert detscreen.partners(None, J).tolist() == [-1] * J
    assert detscreen.partners([1, 0, 3, 2, -1, -5], J).tolist() == [1, 0, 3, 2, -1, -1]
    table = [1, 0, 2, 4, 6, 100]      # 2: itself; 3: its partner does not point back; 4, 5: out of range
    assert detscreen.partners(table, J).tolist() == [1, 0, -1, -1, -1, -1]
    assert detscreen.check_mirror(np.array([1, 0, 3, 2, -1, -7]), J).tolist() == [1, 0, 3, 2, -1, -7]
    assert detscreen.check_mirror(np.array([1, 0, 3, 2, -1, -7]), J).dtype == np.int32
    for bad in ([1, 0, 2, -1, -1, -1], [1, 0, -1, 4, -1, -1], [1, 0, -1, -1, 6, -1], [1, 0, -1, -1, -1, 100], [1, 0], [[1, 0]]):
        with pytest.raises(ValueError, match="mirror"):
            detscreen.check_mirror(np.array(bad), J)
    with pytest.raises(ValueError, match="mirror"):
        detscreen.check_mirror(np.zeros(J), J)                                # not integers
    assert detscreen.mirror_table([0, 2], [1, 5], J).tolist() == [1, 0, 5, -1, -1, 2]
    assert detscreen.mirror_table([], [], 3).tolist() == [-1, -1, -1]
    for left, right in (([0], [1, 2]), ([0, 0], [1, 2]), ([0], [0]), ([0], [6]), ([-1], [1])):
        with pytest.raises(ValueError, match="mirror_table"):
            detscreen.mirror_table(left, right, J)
    x, conf = exact_lines()
    a = detscreen.screen(x, conf, table, 3)
    b = detscreen.screen(x, conf, [1, 0, -1, -1, -1, -1], 3)
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))
    for kw in (dict(radius=0), dict(radius=65), dict(gate=0.0), dict(gate=np.inf), dict(floor=-1.0), dict(floor=np.nan), dict(passes=0),
               dict(passes=9), dict(support=1), dict(support=130), dict(threshold=-0.1), dict(threshold=np.nan)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            detscreen.screen(x, conf, None, **{"radius": 3, **kw})


def test_planting_helpers():
    from pafuse_amd import detscreen
    x, conf, mirror = noisy_video(100, 20)
    on, shift = detscreen.plant_outliers(100, 20, 0.05, 3, (0.1, 0.2), 5)
    again = detscreen.plant_outliers(100, 20, 0.05, 3, (0.1, 0.2), 5)
    assert np.array_equal(on, again[0]) and np.array_equal(shift, again[1]) and not np.array_equal(on, detscreen.plant_outliers(100, 20, 0.05, 3, 0.1, 6)[0])
    length = np.sqrt((shift.astype(np.float64) ** 2).sum(-1))
    assert on.any() and (length[~on] == 0).all() and (length[on] > 0.0999).all() and (length[on] < 0.2001).all()
    sw = detscreen.plant_swaps(100, mirror, 0.05, 3, 7)
    assert sw.any() and not sw[:, 16:].any() and np.array_equal(sw[:, 0:16:2], sw[:, 1:16:2])
    bad = detscreen.corrupt(x, conf, mirror, outliers=(0.05, 3, (0.1, 0.2), 5), swaps=(0.05, 3, 7))
    assert np.array_equal(bad["planted_swap"], sw) and np.array_equal(bad["planted_out"], on & ~sw)
    q = detscreen.partners(mirror, 20)
    assert np.array_equal(bits(bad["x2d"][sw]), bits(x[:, q][sw])) and np.array_equal(bits(bad["conf"][sw]), bits(conf[:, q][sw]))
    assert np.array_equal(bits(bad["conf"][~sw]), bits(conf[~sw]))           # an outlier keeps its confidence
    moved = (bits(bad["x2d"]) != bits(x)).any(-1)
    assert np.array_equal(moved, sw | bad["planted_out"])
    with pytest.raises(ValueError, match="mirror"):
        detscreen.corrupt(x, conf, None, swaps=(0.05, 3, 7))
    status = np.zeros((100, 20), np.uint8)
    status[bad["planted_out"]] = 1
    status[sw] = 2
    status[0, 19], status[1, 19], status[2, 19] = 1, 2, 3
    free = ~(bad["planted_out"] | sw)
    err = detscreen.screen_error(status, bad["planted_out"], sw, parts={"a": range(10), "b": range(10, 20)})
    assert err["out_found"] == int(bad["planted_out"].sum()) and err["out_missed"] == 0 and err["swap_found"] == int(sw.sum())
    assert err["false_rejects"] == 1 - int(~free[0, 19]) and err["false_swaps"] == 1 - int(sw[1, 19])
    assert err["untouched"] == int(free.sum()) - int(free[2, 19])
    assert all(err["parts"]["a"][k] + err["parts"]["b"][k] == err[k] for k in err if k != "parts")
    assert detscreen.screen_error(np.zeros((3, 2), np.uint8), None, None)["untouched"] == 6


# ------------------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_arguments():
    """every refusal below happens before the first HIP call; the buffers stay untouched"""
    L = lib()
    N, J = 2, 3
    assert L.pafuse_detections_screen_workspace_bytes(N, J) == 8 * J + 14 * N * J
    assert L.pafuse_detections_screen_workspace_bytes(0, J) == 0 and L.pafuse_detections_screen_workspace_bytes(N, -1) == 0
    buf = (C.c_float * 1024)()
    for i in range(1024):
        buf[i] = 7.0
    p = C.addressof(buf)
    q, c, cq, s, rs, sc, ws = p + 256, p + 512, p + 640, p + 768, p + 896, p + 1024, p + 2048
    need = 8 * J + 14 * N * J
    # x2d, conf, mirror, N, J, radius, passes, support, threshold, gate, floor, out, conf_out, status, resid, scale, workspace, bytes, stream
    ok = [p, c, None, N, J, 13, 3, 3, 0.0, 4.0, 0.005, q, cq, s, rs, sc, ws, need, None]
    cases = [(0, None), (1, None), (11, None), (12, None), (13, None), (3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, 65), (5, -1),
             (6, 0), (6, 9), (7, 1), (7, 130), (8, -0.5), (8, float("nan")), (8, float("inf")), (9, 0.0), (9, -1.0), (9, float("nan")),
             (9, float("inf")), (10, 0.0), (10, -0.005), (10, float("nan")), (10, float("inf")), (11, p), (12, c), (16, None),
             (16, ws + 4), (17, need - 1), (17, 0)]
    for i, v in cases:
        a = list(ok)
        a[i] = v
        assert L.pafuse_detections_screen(*a) == E_ARG, (i, v)
        assert b"detections_screen" in L.pafuse_last_error(), (i, v)
    a = list(ok)
    a[3], a[4], a[17] = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 63             # N*J / 256 workgroups do not fit a grid
    assert L.pafuse_detections_screen(*a) == E_ARG and b"grid" in L.pafuse_last_error()
    assert all(v == 7.0 for v in buf)


def test_python_layers_refuse_before_touching_the_device():
    lib()
    from pafuse_amd import harness, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.screen_detections(z(4, 3, 2), z(4, 3))
    with pytest.raises(ValueError, match="conf must be"):
        ops.screen_detections(z(4, 3, 2), z(4, 2))
    with pytest.raises(ValueError, match="x2d must be"):
        ops.screen_detections(z(4, 3, 3), z(4, 3))
    for key, values in (("radius", (0, 65, 2.5, True)), ("passes", (0, 9, 1.5, True)), ("support", (1, 130, 2.5, True)),
                        ("gate", (0.0, -1.0, float("nan"), float("inf"), True)), ("floor", (0.0, -1.0, float("nan"), float("inf"))),
                        ("threshold", (-1.0, float("nan"), float("inf")))):
        for v in values:
            with pytest.raises(ValueError, match=key):
                ops.screen_detections(z(4, 3, 2), z(4, 3), **{key: v})
    with pytest.raises(ValueError, match="want"):
        ops.screen_detections(z(4, 3, 2), z(4, 3), want=("x2d", "mean"))
    for bad in ([1, 0, 2], [1, 2, 0], [1, 0, 3], [1, 0], torch.zeros(3)):
        with pytest.raises(ValueError, match="mirror"):
            ops.screen_detections(z(4, 3, 2), z(4, 3), mirror=bad)
    assert ops.screen_mirror_table([1, 0, -1], 3).tolist() == [1, 0, -1]
    model = torch.nn.Linear(1, 1)
    model.frames = 27
    seq, conf = z(60, 134, 2), z(60, 134)
    args = (model, dataset(), seq, [], [])
    with pytest.raises(ValueError, match="screen needs conf"):
        harness.infer_sequence(*args, screen=13)
    with pytest.raises(ValueError, match="screen needs conf"):
        harness.infer_sequence(*args, aggregate="mean", stride=9, screen=13)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="screen"):
            harness.infer_sequence(*args, conf=conf, screen=bad)
    for key in ("screen_gate", "screen_floor"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=key):
                harness.infer_sequence(*args, conf=conf, screen=13, **{key: bad})
    with pytest.raises(ValueError, match="conf must be"):
        harness.infer_sequence(*args, conf=z(60, 133), screen=13)
    with pytest.raises(ValueError, match="mirror_table"):
        harness.infer_sequence(model, dataset(), seq, [0, 1], [2], conf=conf, screen=13)
    with pytest.raises(ValueError, match="conf belongs"):               # unchanged without a screen
        harness.infer_sequence(*args, conf=conf)
    ev = (model, dataset(), seq, z(60, 134, 3), z(9), [], [])
    with pytest.raises(ValueError, match="screen needs conf"):
        harness.evaluate_frames(*ev, screen=13)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="screen"):
            harness.evaluate_frames(*ev, conf=conf, screen=bad)
    for bad in ((0.2, 10, 0.3), (1.5, 10, 0.3, 0), (0.2, 0, 0.3, 0), 0.2):
        with pytest.raises(ValueError, match="corrupt"):
            harness.evaluate_frames(*ev, corrupt=bad)
    for bad in ((0.2, 10), (1.5, 10, 0), (0.2, 0, 0), 0.2):
        with pytest.raises(ValueError, match="swap"):
            harness.evaluate_frames(*ev, swap=bad)
    with pytest.raises(ValueError, match="radius"):
        harness.screen_detections(seq, conf, radius=0)
    with pytest.raises(ValueError, match="seq_2d must be"):
        harness.screen_detections(seq, z(60, 133))
    with pytest.raises(ValueError, match="mirror_table"):
        harness.screen_detections(seq, conf, kps_left=[0], kps_right=[0])


def test_torch_op_has_a_schema_and_a_fake():
    import pafuse_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.pafuse.screen_detections.default._schema)
    assert "Tensor x2d, Tensor conf" in s and "[]? mirror=None" in s and "radius=13" in s and "float gate=4." in s and "passes=3, " in s and "support=3" in s
    assert s.endswith("-> Tensor[]")
    with FakeTensorMode():
        x, conf, status, resid, scale = torch.ops.pafuse.screen_detections(torch.empty(5, 7, 2, device="cuda"), torch.empty(5, 7, device="cuda"),
                                                                           [1, 0, -1, -1, -1, -1, -1], 3)
        assert x.shape == (5, 7, 2) and conf.shape == status.shape == resid.shape == (5, 7) and scale.shape == (7,)
        assert x.dtype == conf.dtype == resid.dtype == scale.dtype == torch.float32 and status.dtype == torch.uint8

"""The screening of observed 2-D detections on the device: detections_residual_kernel, detections_scale_kernel and
detections_screen_finish_kernel (pafuse_detections_screen), ops.screen_detections, torch.ops.pafuse.screen_detections,
harness.screen_detections, infer_sequence(screen=...) and evaluate_frames(corrupt=..., swap=..., screen=...).

What is asserted and why it can be asserted:
  * kernel vs statement: the kernels and pafuse_amd/detscreen.py perform the same IEEE fp64 operations in the same order (the walk
    ascending, contraction off, correctly rounded divides and square roots), then round once to fp32 -> the design goal is equal
    bits.  status, conf and out are decisions and copies: torch.equal / the same bits.  resid and scale are accepted equal or
    ADJACENT in fp32 with NaN exactly where the statement has it - the rule of tests/test_hip_rootfit.py - and the number that
    differ is printed.  (A residual one fp32 step off that sat exactly on a gate could flip a decision; the decisions are
    asserted equal all the same.)
  * the scale kernel alone: the median is a selection by integer counts, no rounding takes part, and tau is three fp64
    operations on it -> torch.equal.
  * the planted case of tests/test_detections_screen_host.py is exact in fp64 (dyadic taper at r = 3, dyadic data) -> the truth.
Shapes: J in {1, 5, 64, 65, 134} x N in {1, 2, 9, 70} x r in {1, 3, 64} as in tests/test_hip_detections.py.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_detections_screen_host import MIRROR6, SUPPORT_EXACT, planted_exact
from tests.test_hip_detections import F27, N_VIDEO, SEED, SimpleVideo
from tests.test_hip_partials import dataset, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 5
R = 5
CASES = [(J, N, r) for J in (1, 5, 64, 65, 134) for N in (1, 2, 9, 70) for r in (1, 3, 64)]
KEYS = ("x2d", "conf", "status", "resid", "scale")


def inputs(J, N, seed, junk=0.0):
    """tests/test_hip_detections.inputs - a random walk per joint with random confidences, 30 % of the confidences 0 with their
    coordinates at `junk`, one NaN coordinate under a positive confidence - with mirror pairs (2k, 2k+1) over the first half of
    the joints, 5 % of the detections displaced by 0.3 .. 1, swapped runs of 3 frames, joint J - 1 observed in at most two
    frames and, from J = 5 on, the pair (0, 1) coinciding -> (x2d, conf, mirror list or None) on the host"""
    from pafuse_amd import detscreen
    g = torch.Generator().manual_seed(seed)
    x = torch.cumsum(torch.randn(N, J, 2, generator=g) * 0.02, dim=0) + torch.rand(1, J, 2, generator=g) - 0.5
    conf = torch.rand(N, J, generator=g) * 0.9 + 0.1
    lost = torch.rand(N, J, generator=g) < 0.3
    mirror = None
    if J >= 4:
        mirror = np.full(J, -1, dtype=np.int64)
        half = (J // 4) * 2
        mirror[0:half:2], mirror[1:half:2] = np.arange(1, half, 2), np.arange(0, half, 2)
        x[:, 1] = x[:, 0]                                     # a pair whose two joints coincide
    bad = detscreen.corrupt(x.numpy(), conf.numpy(), mirror, outliers=(0.05, 1, (0.3, 1.0), seed), swaps=None if mirror is None else (0.1, 3, seed))
    x, conf = torch.from_numpy(bad["x2d"]), torch.from_numpy(bad["conf"])
    lost[:, J - 1] = True
    lost[N // 2:N // 2 + 2, J - 1] = False                    # a joint observed in fewer than `support` frames
    conf[lost] = 0
    x[lost] = junk
    seen = (~lost).nonzero()
    if len(seen):
        n, j = seen[len(seen) // 2].tolist()
        x[n, j, 1] = float("nan")
    return x.contiguous(), conf.contiguous(), None if mirror is None else mirror.tolist()


def statement(x, conf, mirror, r, **kw):
    from pafuse_amd import detscreen
    return dict(zip(KEYS, (torch.from_numpy(np.ascontiguousarray(v)) for v in detscreen.screen(x.numpy(), conf.numpy(), mirror, r, **kw))))


def check(got, want, x, label):
    got = {k: v.cpu() for k, v in got.items()}
    assert torch.equal(got["status"], want["status"]), label
    assert same_bits(got["conf"], want["conf"]) and same_bits(got["x2d"], want["x2d"]), label
    differ = equal_or_adjacent(got["resid"], want["resid"]) + equal_or_adjacent(got["scale"], want["scale"])
    assert not bool((torch.isnan(got["x2d"]) & ~torch.isnan(x)).any())              # NaN nowhere it was not
    return differ


@pytest.mark.parametrize("case", CASES)
def test_kernels_are_the_statement(case):
    from pafuse_amd import ops
    J, N, r = case
    x, conf, mirror = inputs(J, N, seed=2000 + 31 * J + 7 * N + r)
    xd, cd = x.to(DEV), conf.to(DEV)
    differ, counts = 0, None
    for table in ((mirror, None) if mirror is not None else (None,)):
        for kw in (dict(passes=1, support=2), {}, dict(passes=2, threshold=0.5)):
            got = ops.screen_detections(xd, cd, mirror=table, radius=r, **kw)
            want = statement(x, conf, table, r, **kw)
            differ += check(got, want, x, (case, table is not None, kw))
            counts = counts if counts is not None else torch.bincount(want["status"].reshape(-1).long(), minlength=4).tolist()
    print(f"(J, N, r) = {case}: {differ} resid / scale values differ from the statement (by one fp32 step); "
          f"status counts with passes=1, support=2 {counts}")


def scale_inputs(N):
    """columns: 0 an exact line (equal residuals: 0), 1 observed at frames 0, 3 and 6 (with support = 2 and r = 3 only frame 3 has
    a fit: one tested value; with support = 3 none), 2 never observed, 3 zeros but three coordinates of +-3.4e38 (a residual that
    rounds to +inf in fp32), 4 a random walk, 5 a zigzag of period 2 (residuals tied up to rounding), 6 a zigzag between +-3.4e38
    (most residuals +inf: the median is +inf and so is the scale) -> (x2d, conf)"""
    g = torch.Generator().manual_seed(N)
    x = torch.cumsum(torch.randn(N, 7, 2, generator=g) * 0.02, dim=0)
    conf = torch.rand(N, 7, generator=g) * 0.9 + 0.1
    t = torch.arange(N, dtype=torch.float32)
    x[:, 0, 0], x[:, 0, 1] = t / 8, 1 - t / 16
    conf[:, 0] = 1.0
    conf[:, 1] = 0
    conf[[n for n in (0, 3, 6) if n < N], 1] = 1.0
    conf[:, 2] = 0
    x[:, 3] = 0.0
    if N > 2:
        x[N // 2, 3, 0], x[N // 2 - 1, 3, 0], x[N // 2 + 1, 3, 0] = 3.4e38, -3.4e38, -3.4e38
    x[:, 5, 0], x[:, 5, 1] = t % 2, 0.0
    x[:, 6, 0], x[:, 6, 1] = (t % 2 * 2 - 1) * 3.4e38, 0.0
    return x, conf


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 200])
def test_scale_kernel_alone(N):
    """one frame per lane, the wave edge, three to four frames per lane; the median is a selection, so the scale is torch.equal"""
    from pafuse_amd import ops
    x, conf = scale_inputs(N)
    for kw in (dict(support=2), dict(support=3), dict(support=2, gate=2.5, floor=0.001, passes=1)):
        got = ops.screen_detections(x.to(DEV), conf.to(DEV), radius=3, want=("scale",), **kw)
        assert set(got) == {"scale"}
        want = statement(x, conf, None, 3, **kw)
        assert torch.equal(got["scale"].cpu(), want["scale"]), (N, kw, got["scale"].cpu(), want["scale"])
    if N >= 9:                                                                           # the columns are what they claim to be
        from pafuse_amd import detscreen
        x64, observed = x.numpy().astype(np.float64), (conf > 0).numpy()
        pred, fit = detscreen.loo_line(x64, conf.numpy().astype(np.float64), observed, 3, 2)
        with np.errstate(all="ignore"):
            e1 = np.where(observed & fit, detscreen.distance(x64, pred), np.float32(np.nan))
        assert (e1[:, 0] == 0).all() and int((~np.isnan(e1[:, 1])).sum()) == 1 and np.isnan(e1[:, 2]).all()
        assert np.isinf(e1[:, 3]).any() and (e1[:, 3] == 0).any()
        assert np.isinf(e1[:, 6]).sum() > N // 2 and bool(torch.isinf(want["scale"][6]))


def raw(x, conf, mirror, N, J, r, out, conf_out, status, resid, scale, passes=3, support=3, threshold=0.0, gate=4.0, floor=0.005, work=None):
    from pafuse_amd import _lib
    lib = _lib.load()
    need = lib.pafuse_detections_screen_workspace_bytes(N, J) if N > 0 and J > 0 else 64
    if work is None:
        work = torch.empty((need + 7) // 8, dtype=torch.float64, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.pafuse_detections_screen(ptr(x), ptr(conf), ptr(mirror), N, J, r, passes, support, threshold, gate, floor, ptr(out),
                                      ptr(conf_out), ptr(status), ptr(resid), ptr(scale), ptr(work), work.numel() * 8, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 70, 64), (65, 9, 3), (1, 1, 1)])
def test_canaries(case):
    """guard elements before and after out, conf_out, status, resid and scale are untouched"""
    from pafuse_amd import ops
    J, N, r = case
    x, conf, mirror = inputs(J, N, seed=77)
    x, conf = x.to(DEV), conf.to(DEV)
    table = None if mirror is None else torch.tensor(mirror, dtype=torch.int32, device=DEV)
    out = torch.full((PAD + N * J * 2 + PAD,), 7.0, device=DEV)
    conf_out = torch.full((PAD + N * J + PAD,), 7.0, device=DEV)
    resid = torch.full((PAD + N * J + PAD,), 7.0, device=DEV)
    scale = torch.full((PAD + J + PAD,), 7.0, device=DEV)
    status = torch.full((PAD + 3 + N * J + PAD,), 7, dtype=torch.uint8, device=DEV)
    assert raw(x, conf, table, N, J, r, out[PAD:], conf_out[PAD:], status[PAD + 3:], resid[PAD:], scale[PAD:]) == 0
    want = ops.screen_detections(x, conf, mirror=mirror, radius=r)
    for buf, lead, n, k in ((out, PAD, N * J * 2, "x2d"), (conf_out, PAD, N * J, "conf"), (status, PAD + 3, N * J, "status"),
                            (resid, PAD, N * J, "resid"), (scale, PAD, J, "scale")):
        assert bool((buf[:lead] == 7).all()) and bool((buf[lead + n:] == 7).all()), k
        assert same_bits(buf[lead:lead + n], want[k].reshape(-1)), k


def test_planted_exact_swap_and_outlier_are_restored_on_the_device():
    from pafuse_amd import ops
    x, c, truth, conf, swapped, outl = planted_exact()
    got = ops.screen_detections(torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV), mirror=MIRROR6, radius=3, support=SUPPORT_EXACT)
    status = got["status"].cpu()
    want = torch.zeros_like(status)
    want[swapped, 0] = want[swapped, 1] = 2
    want[outl, 4] = 1
    assert torch.equal(status, want)                                             # status 1 exactly on the planted outlier
    two = status == 2
    assert torch.equal(got["x2d"].cpu()[two], torch.from_numpy(truth)[two]) and torch.equal(got["conf"].cpu()[two], torch.from_numpy(conf)[two])
    keep = status != 1
    assert torch.equal(got["x2d"].cpu()[keep], torch.from_numpy(truth)[keep])
    assert bool((got["conf"].cpu()[~keep] == 0).all()) and bool((got["resid"].cpu()[status == 0] == 0).all())
    assert torch.equal(got["scale"].cpu(), torch.full((6,), 0.02))


@pytest.mark.parametrize("junk", [1e30, float("inf"), float("nan"), 12345.0])
def test_garbage_in_unobserved_joints_does_not_leak_on_the_device(junk):
    from pafuse_amd import ops
    J, N, r = 134, 70, 3
    x, conf, mirror = inputs(J, N, seed=6)
    base = ops.screen_detections(x.to(DEV), conf.to(DEV), mirror=mirror, radius=r)
    y = x.clone()
    y[conf == 0] = junk
    got = ops.screen_detections(y.to(DEV), conf.to(DEV), mirror=mirror, radius=r)
    assert torch.equal(got["status"], base["status"]) and same_bits(got["conf"], base["conf"])
    assert same_bits(got["resid"], base["resid"]) and same_bits(got["scale"], base["scale"])
    seen = (base["status"] != 3).cpu()
    assert same_bits(got["x2d"].cpu()[seen], base["x2d"].cpu()[seen]) and bool(torch.isfinite(got["x2d"].cpu()[seen]).all())
    assert same_bits(got["x2d"].cpu()[~seen], y[~seen])                # not observed: the input's bits, whatever they are


def test_table_forms_and_layers():
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import harness, ops
    J, N, r = 65, 70, 3
    x, conf, mirror = inputs(J, N, seed=5)
    xd, cd = x.to(DEV), conf.to(DEV)
    none = ops.screen_detections(xd, cd, mirror=None, radius=r)
    flat = ops.screen_detections(xd, cd, mirror=[-1] * J, radius=r)
    assert all(same_bits(none[k], flat[k]) for k in none)
    # a table with entries the partner rule drops only passes the raw entry, which reads it by the rule
    dropped = torch.full((J,), -1, dtype=torch.int32)
    dropped[0], dropped[1], dropped[2], dropped[3], dropped[4], dropped[5], dropped[6], dropped[J - 1] = 1, 0, 2, 4, J, 2 ** 31 - 1, -9, 3
    cleaned = torch.full((J,), -1, dtype=torch.int32)
    cleaned[0], cleaned[1] = 1, 0
    both = []
    for table in (dropped, cleaned):
        bufs = [torch.empty(N, J, 2, device=DEV), torch.empty(N, J, device=DEV), torch.empty(N, J, dtype=torch.uint8, device=DEV),
                torch.empty(N, J, device=DEV), torch.empty(J, device=DEV)]
        assert raw(xd, cd, table.to(DEV), N, J, r, *bufs) == 0
        both.append(bufs)
    assert all(same_bits(a, b) for a, b in zip(*both))
    want = ops.screen_detections(xd, cd, mirror=cleaned.tolist(), radius=r)
    assert all(same_bits(b, want[k]) for b, k in zip(both[1], KEYS))
    bufs = [torch.empty(N, J, 2, device=DEV), torch.empty(N, J, device=DEV), torch.empty(N, J, dtype=torch.uint8, device=DEV)]
    assert raw(xd, cd, None, N, J, r, *bufs, None, None) == 0                     # resid = scale = NULL is accepted
    assert all(same_bits(b, none[k]) for b, k in zip(bufs, KEYS))
    # the torch op, the harness
    kw = dict(radius=r, gate=3.0, floor=0.01, passes=2, support=2, threshold=0.25)
    want = ops.screen_detections(xd, cd, mirror=mirror, **kw)
    assert int((want["status"] == 1).sum()) > 0 and int((want["status"] == 2).sum()) > 0
    got = torch.ops.pafuse.screen_detections(xd, cd, mirror, r, 3.0, 0.01, 2, 2, 0.25)
    assert all(same_bits(g, want[k]) for g, k in zip(got, KEYS))
    host = harness.screen_detections(x, conf, mirror=mirror, **kw)
    assert set(host) == set(KEYS) | {"counts"} and all(not v.is_cuda for v in host.values())
    assert all(same_bits(host[k], want[k].cpu()) for k in KEYS)
    assert host["counts"].tolist() == torch.bincount(host["status"].reshape(-1).long(), minlength=4).tolist() and int(host["counts"].sum()) == N * J
    pairs = [(j, mirror[j]) for j in range(J) if mirror[j] > j]
    by_lists = harness.screen_detections(x, conf, kps_left=[a for a, _ in pairs], kps_right=[b for _, b in pairs], **kw)
    assert all(same_bits(by_lists[k], host[k]) for k in KEYS)
    # the raw entry refuses on the device as on the host; nothing is launched
    out = torch.full((N, J, 2), 7.0, device=DEV)
    status = torch.full((N, J), 7, dtype=torch.uint8, device=DEV)
    a = dict(x=xd, conf=cd, mirror=None, N=N, J=J, r=r, out=out, conf_out=torch.full((N, J), 7.0, device=DEV), status=status, resid=None, scale=None)
    for kw in (dict(x=None), dict(out=None), dict(conf_out=None), dict(N=0), dict(r=65), dict(passes=0), dict(support=1), dict(gate=0.0),
               dict(floor=float("nan")), dict(out=xd), dict(conf_out=cd), dict(work=torch.empty(1, dtype=torch.float64, device=DEV))):
        assert raw(**{**a, **kw}) == -1, kw
    assert bool((out == 7.0).all()) and bool((status == 7).all())


# --------------------------------------------------------------------------------------------------------- infer_sequence
@pytest.fixture(scope="module")
def video():
    """the suite's seeded video with planted outliers far outside its noise (displaced by 8 .. 10), swapped runs and dropouts, its
    screen and the repair behind it, and the small model; computed once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import detections, detscreen, harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, seq_3d, cam = sequence(N_VIDEO)
    mirror = detscreen.mirror_table(gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, 134)
    g = torch.Generator().manual_seed(3)
    conf = torch.rand(N_VIDEO, 134, generator=g) * 0.5 + 0.5
    bad = detscreen.corrupt(seq_2d.numpy(), conf.numpy(), mirror, outliers=(0.03, 2, (8.0, 10.0), 3), swaps=(0.05, 3, 4))
    lost = torch.from_numpy(detections.plant_dropouts(N_VIDEO, 134, 0.1, 4, 13))    # (seed 3 would draw the outliers' own starts)
    x = torch.where(lost.unsqueeze(-1), torch.tensor(detections.DROPPED_XY), torch.from_numpy(bad["x2d"]))
    conf = torch.where(lost, torch.zeros(()), torch.from_numpy(bad["conf"]))
    v = SimpleVideo(model, x, conf, None, seq_2d, seq_3d, cam)
    v.screened = harness.screen_detections(x, conf, mirror=mirror, radius=R)
    v.fixed = harness.repair_detections(v.screened["x2d"], v.screened["conf"], dataset=dataset(), radius=R)
    return v


def test_infer_sequence_screen_none_is_the_call_without_it(video):
    assert same_bits(video.infer(video.x, aggregate="mean"), video.infer(video.x, aggregate="mean", screen=None))
    assert same_bits(video.infer(video.x), video.infer(video.x, screen=None, screen_gate=4.0, screen_floor=0.005))


def test_infer_sequence_screen_is_infer_sequence_on_the_screened_pair(video):
    screened, fixed = video.screened, video.fixed
    assert int(screened["counts"][1]) > 50 and int(screened["counts"][3]) == int((video.conf == 0).sum())
    # aggregate="mean" and None: a tensor keeps its type
    got = video.infer(video.x, aggregate="mean", conf=video.conf, screen=R)
    assert isinstance(got, torch.Tensor) and same_bits(got, video.infer(screened["x2d"], aggregate="mean"))
    assert same_bits(video.infer(video.x, conf=video.conf, screen=R), video.infer(screened["x2d"]))
    # (a rejection zeroes a confidence and moves no detection: that the argument is not ignored shows below, in the fit)
    # with a stride: the dict gains exactly "screened" (and "repaired" with a repair)
    got = video.infer(video.x, aggregate="mean", stride=F27 - 1, conf=video.conf, screen=R)
    want = video.infer(screened["x2d"], aggregate="mean", stride=F27 - 1)
    assert set(got) == set(want) | {"screened"} and all(same_bits(got[k], want[k]) for k in want)
    assert got["screened"].dtype == torch.uint8 and torch.equal(got["screened"], screened["status"])
    # screen and repair: screen -> repair -> infer by hand
    got = video.infer(video.x, aggregate="mean", stride=F27 - 1, conf=video.conf, screen=R, repair=R)
    want = video.infer(fixed["x2d"], aggregate="mean", stride=F27 - 1)
    assert set(got) == set(want) | {"screened", "repaired"} and all(same_bits(got[k], want[k]) for k in want)
    assert torch.equal(got["repaired"], fixed["status"]) and torch.equal(got["screened"], screened["status"])
    assert torch.equal(fixed["status"] != 0, screened["conf"] == 0)               # the repair fills what the screen rejected
    # aggregate="reproj_fit": the fit and the pick see the zeroed confidences; a tuple stays a tuple
    got = video.infer(video.x, aggregate="reproj_fit", cam=video.cam, conf=video.conf, screen=R, repair=R)
    want = video.infer(fixed["x2d"], aggregate="reproj_fit", cam=video.cam, conf=fixed["conf"])
    assert isinstance(got, tuple) and len(got) == 2 and same_bits(got[0], want[0]) and torch.equal(got[1], want[1])
    got = video.infer(video.x, aggregate="reproj_fit", cam=video.cam, conf=video.conf, screen=R)
    want = video.infer(screened["x2d"], aggregate="reproj_fit", cam=video.cam, conf=screened["conf"])
    assert same_bits(got[0], want[0]) and torch.equal(got[1], want[1])
    other = video.infer(screened["x2d"], aggregate="reproj_fit", cam=video.cam, conf=video.conf)
    assert not torch.equal(got[1], other[1])                                   # the confidences that arrive are the screened ones


def run_frames(video, **kw):
    from pafuse_amd import harness
    video.model.noise_fn, video.model.noise, video.model.noise_seed = None, "device", SEED
    return harness.evaluate_frames(video.model, dataset(), video.clean, video.seq_3d, video.cam, gu.SYN_JOINTS_LEFT,
                                   gu.SYN_JOINTS_RIGHT, aggregate="reproj_fit", stride=F27, **kw)


CORRUPT, SWAP = (0.03, 2, (8.0, 10.0), 3), (0.05, 3, 4)


def test_evaluate_frames_with_planted_outliers_swaps_and_screen(video):
    clean = run_frames(video)
    wrong = run_frames(video, corrupt=CORRUPT)
    swapped = run_frames(video, corrupt=CORRUPT, swap=SWAP)
    screened = run_frames(video, corrupt=CORRUPT, swap=SWAP, screen=R)
    fixed = run_frames(video, corrupt=CORRUPT, swap=SWAP, screen=R, repair=R)
    assert len(clean) == 2 and all(len(v) == 3 for v in (wrong, swapped, screened, fixed))
    for sums, counts, _ in (wrong, swapped, screened, fixed):
        assert set(sums) == set(clean[0]) and all(bool(torch.isfinite(v).all()) for v in sums.values())
        assert all(torch.equal(counts[k], clean[1][k]) for k in counts)
    chain = [clean[0]["mpjpe"], wrong[0]["mpjpe"], swapped[0]["mpjpe"], screened[0]["mpjpe"], fixed[0]["mpjpe"]]
    assert all(not torch.equal(a, b) for a, b in zip(chain, chain[1:]))           # no argument is silently ignored
    assert set(wrong[2]) == set(swapped[2]) == {"planted_out", "planted_swap", "x2d", "conf"}
    assert set(screened[2]) == {"planted_out", "planted_swap", "screened", "x2d", "conf"}
    assert set(fixed[2]) == {"planted_out", "planted_swap", "screened", "status", "x2d", "conf"}
    assert int(wrong[2]["planted_swap"].sum()) == 0 and int(swapped[2]["planted_swap"].sum()) > 0
    for other in (screened, fixed):                                              # the planting is the same whatever screen is
        assert torch.equal(other[2]["planted_out"], swapped[2]["planted_out"]) and torch.equal(other[2]["planted_swap"], swapped[2]["planted_swap"])
    from pafuse_amd import harness
    by_hand = harness.screen_detections(swapped[2]["x2d"], swapped[2]["conf"], kps_left=gu.SYN_JOINTS_LEFT, kps_right=gu.SYN_JOINTS_RIGHT, radius=R)
    assert same_bits(screened[2]["x2d"], by_hand["x2d"]) and same_bits(screened[2]["conf"], by_hand["conf"])
    assert torch.equal(screened[2]["screened"], by_hand["status"]) and torch.equal(fixed[2]["screened"], by_hand["status"])
    assert int((by_hand["status"] == 1).sum()) > 50
    assert torch.equal(fixed[2]["status"] != 0, by_hand["conf"] == 0)


def test_h3wb_evaluate_frames_plants_per_video_and_logs_the_screen_error(video):
    from pafuse_amd import detscreen, h3wb
    clean, gt, cam = video.clean.numpy(), video.seq_3d.numpy(), video.cam.numpy()
    lines = []
    video.model.noise_fn, video.model.noise, video.model.noise_seed = None, "device", SEED
    rep = h3wb.evaluate_frames(video.model, dataset(), [cam, cam], [gt, gt], [clean, clean], gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                               stride=F27, log=lines.append, corrupt=CORRUPT, swap=SWAP, screen=R)
    assert all(v == v for v in rep["mpjpe"])
    counts = [l for l in lines if "detections accepted" in l]
    errors = [l for l in lines if "screen error all" in l]
    assert len(counts) == 2 and len(errors) == 2 and counts[0] != counts[1] and errors[0] != errors[1]     # seed + the video's number
    assert sum("screen error" in l for l in lines) == 2 * (1 + len(dataset().parts_joint_indices))
    one = run_frames(video, corrupt=CORRUPT[:3] + (CORRUPT[3] + 1,), swap=SWAP[:2] + (SWAP[2] + 1,), screen=R)
    assert counts[1] == "video 1 : detections accepted %d, rejected %d, swapped %d, not observed %d" % tuple(
        detscreen.counts(one[2]["screened"].numpy()))
    err = detscreen.screen_error(one[2]["screened"].numpy(), one[2]["planted_out"].numpy(), one[2]["planted_swap"].numpy())
    assert errors[1].startswith("video 1 : screen error all: outliers found %d, missed %d," % (err["out_found"], err["out_missed"]))

"""The repair of missing 2-D detections on the device: detections_repair_kernel (pafuse_detections_repair), ops.repair_detections,
torch.ops.pafuse.repair_detections, harness.repair_detections, infer_sequence(repair=...) and evaluate_frames(drop=..., repair=...).

What is asserted and why it can be asserted:
  * kernel vs statement: the kernel and pafuse_amd/detections.py perform the same IEEE fp64 operations in the same order (the walk
    ascending, contraction off, correctly rounded divides), then round once to fp32 -> the design goal is equal bits.  status and
    conf_out are decisions, not roundings: torch.equal.  out is accepted equal or ADJACENT in fp32 with NaN nowhere it was not -
    the rule of tests/test_hip_rootfit.py - and the number that differ is printed.
  * the planted case of tests/test_detections_host.py is exact in fp64 (dyadic taper at r = 3, dyadic data) -> torch.equal to the truth.
  * level 0 vs the smoother: the same kernel arithmetic on the same series -> torch.equal at the missing frames that were filled.
Shapes: J in {1, 5, 64, 65, 134} - lanes without work, exactly a wave, one joint into the next wave, the real layout - x N in
{1, 2, 9, 70} x r in {1, 3, 64} (r >= N); 70 x 134 = 9380 threads is 37 workgroups with a ragged last one.
"""
import numpy as np
import pytest
import torch

from tests.golden import golden_util as gu
from tests.test_detections_host import planted
from tests.test_hip_partials import dataset, same_bits, sequence
from tests.test_hip_rootfit import equal_or_adjacent

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 5
CASES = [(J, N, r) for J in (1, 5, 64, 65, 134) for N in (1, 2, 9, 70) for r in (1, 3, 64)]


def inputs(J, N, seed, junk=0.0):
    """a random walk per joint with random confidences, 30 % of the confidences 0 with their coordinates at `junk`, one NaN
    coordinate under a positive confidence, and anchors drawn from the first quarter of the joints (which hang on nothing)
    -> (x2d, conf, anchor list or None) on the host"""
    g = torch.Generator().manual_seed(seed)
    x = torch.cumsum(torch.randn(N, J, 2, generator=g) * 0.02, dim=0) + torch.rand(1, J, 2, generator=g) - 0.5
    conf = torch.rand(N, J, generator=g) * 0.9 + 0.1
    lost = torch.rand(N, J, generator=g) < 0.3
    conf[lost] = 0
    x[lost] = junk
    seen = (~lost).nonzero()
    if len(seen):
        n, j = seen[len(seen) // 2].tolist()
        x[n, j, 1] = float("nan")
    quarter = J // 4
    anchor = None
    if quarter:
        anchor = torch.randint(0, quarter, (J,), generator=g)
        anchor[:quarter] = -1
        anchor[torch.rand(J, generator=g) < 0.2] = -1
        anchor = anchor.tolist()
    return x.contiguous(), conf.contiguous(), anchor


def statement(x, conf, anchor, r, threshold=0.0):
    from pafuse_amd import detections
    return [torch.from_numpy(v) for v in detections.repair(x.numpy(), conf.numpy(), anchor, r, threshold)]


@pytest.mark.parametrize("case", CASES)
def test_kernel_is_the_statement(case):
    from pafuse_amd import ops
    J, N, r = case
    x, conf, anchor = inputs(J, N, seed=1000 + 31 * J + 7 * N + r)
    got = ops.repair_detections(x.to(DEV), conf.to(DEV), anchor=anchor, radius=r)
    want = statement(x, conf, anchor, r)
    assert torch.equal(got["status"].cpu(), want[2]) and same_bits(got["conf"].cpu(), want[1])
    differ = equal_or_adjacent(got["x2d"].cpu(), want[0])
    assert not bool((torch.isnan(got["x2d"].cpu()) & ~torch.isnan(x)).any())       # NaN nowhere it was not
    print(f"(J, N, r) = {case}: {differ} of {got['x2d'].numel()} values differ from the statement (by one fp32 step); "
          f"status counts {torch.bincount(want[2].reshape(-1).long(), minlength=4).tolist()}")
    thr = ops.repair_detections(x.to(DEV), conf.to(DEV), anchor=anchor, radius=r, threshold=0.5)
    want = statement(x, conf, anchor, r, 0.5)
    assert torch.equal(thr["status"].cpu(), want[2]) and same_bits(thr["conf"].cpu(), want[1])
    equal_or_adjacent(thr["x2d"].cpu(), want[0])


def raw(x, conf, anchor, N, J, r, threshold, out, conf_out, status):
    from pafuse_amd import _lib
    lib = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.pafuse_detections_repair(ptr(x), ptr(conf), ptr(anchor), N, J, r, threshold, ptr(out), ptr(conf_out), ptr(status), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", [(134, 70, 64), (65, 9, 3), (1, 1, 1)])
def test_canaries(case):
    """guard elements before and after out, conf_out and status are untouched"""
    from pafuse_amd import ops
    J, N, r = case
    x, conf, anchor = inputs(J, N, seed=77)
    x, conf = x.to(DEV), conf.to(DEV)
    table = None if anchor is None else torch.tensor(anchor, dtype=torch.int32, device=DEV)
    out = torch.full((PAD + N * J * 2 + PAD,), 7.0, device=DEV)
    conf_out = torch.full((PAD + N * J + PAD,), 7.0, device=DEV)
    status = torch.full((PAD + 3 + N * J + PAD,), 7, dtype=torch.uint8, device=DEV)
    assert raw(x, conf, table, N, J, r, 0.0, out[PAD:], conf_out[PAD:], status[PAD + 3:]) == 0
    want = ops.repair_detections(x, conf, anchor=anchor, radius=r)
    for buf, lead, n, k in ((out, PAD, N * J * 2, "x2d"), (conf_out, PAD, N * J, "conf"), (status, PAD + 3, N * J, "status")):
        assert bool((buf[:lead] == 7).all()) and bool((buf[lead + n:] == 7).all()), k
        assert same_bits(buf[lead:lead + n], want[k].reshape(-1)), k


def test_planted_hand_moves_with_its_wrist_exactly_on_the_device():
    from pafuse_amd import ops
    x, conf, truth, lost = planted()
    got = ops.repair_detections(torch.from_numpy(x).to(DEV), torch.from_numpy(conf).to(DEV), anchor=[-1, 0], radius=3)
    assert torch.equal(got["x2d"].cpu(), torch.from_numpy(truth))
    assert bool((got["status"].cpu()[lost, 1] == 1).all()) and int((got["status"] != 0).sum()) == len(lost)
    absolute = ops.repair_detections(torch.from_numpy(x).to(DEV), torch.from_numpy(conf).to(DEV), anchor=[-1, -1], radius=3)
    assert not torch.equal(absolute["x2d"].cpu(), torch.from_numpy(truth))


def test_forms_are_equivalent_and_level_0_is_the_smoother():
    from pafuse_amd import ops
    J, N, r = 65, 70, 3
    x, conf, _ = inputs(J, N, seed=5)
    x, conf = x.to(DEV), conf.to(DEV)
    none = ops.repair_detections(x, conf, anchor=None, radius=r)
    flat = ops.repair_detections(x, conf, anchor=[-1] * J, radius=r)
    assert all(same_bits(none[k], flat[k]) for k in none)
    # a table of demoted entries (nested, self-anchored, out of range) only passes the raw entry, which reads it by the level rule
    demoted = torch.full((J,), -1, dtype=torch.int32)
    demoted[1], demoted[2], demoted[3], demoted[4], demoted[5], demoted[J - 1] = 0, 1, 3, J, 2 ** 31 - 1, J - 1
    level1 = torch.full((J,), -1, dtype=torch.int32)
    level1[1] = 0                                                    # what the rule leaves of it
    both = []
    for table in (demoted, level1):
        out = torch.empty(N, J, 2, device=DEV)
        status = torch.empty(N, J, dtype=torch.uint8, device=DEV)
        assert raw(x, conf, table.to(DEV), N, J, r, 0.0, out, None, status) == 0        # conf_out=None is accepted
        both.append((out, status))
    assert same_bits(both[0][0], both[1][0]) and torch.equal(both[0][1], both[1][1])
    want = ops.repair_detections(x, conf, anchor=level1.tolist(), radius=r)
    assert same_bits(both[1][0], want["x2d"]) and torch.equal(both[1][1], want["status"])
    assert set(ops.repair_detections(x, conf, radius=r, want=("status",))) == {"status"}
    # level 0 against the smoother: x and y in the first two components, 0 in the third, conf (0 at missing frames) as the weight
    series = torch.cat([x, torch.zeros(N, J, 1, device=DEV)], dim=-1).transpose(0, 1).contiguous()      # [J,N,3]
    weight = torch.where(torch.isfinite(x).all(-1), conf, torch.zeros_like(conf)).t().contiguous()
    smooth = ops.smooth_trajectory(series, weight, r).transpose(0, 1)[..., :2]
    filled = (none["status"] == 1) | (none["status"] == 2)
    assert int(filled.sum()) > 100 and torch.equal(none["x2d"][filled], smooth[filled])
    assert bool(torch.isnan(smooth[none["status"] == 3]).all())


@pytest.mark.parametrize("junk", [1e30, float("inf"), float("nan"), 12345.0])
def test_garbage_in_missing_joints_does_not_leak_on_the_device(junk):
    from pafuse_amd import ops
    J, N, r = 134, 70, 3
    x, conf, anchor = inputs(J, N, seed=6)
    base = ops.repair_detections(x.to(DEV), conf.to(DEV), anchor=anchor, radius=r)
    y = x.clone()
    y[conf == 0] = junk
    got = ops.repair_detections(y.to(DEV), conf.to(DEV), anchor=anchor, radius=r)
    assert torch.equal(got["status"], base["status"]) and same_bits(got["conf"], base["conf"])
    keep = (base["status"] != 3).cpu()
    assert same_bits(got["x2d"].cpu()[keep], base["x2d"].cpu()[keep]) and bool(torch.isfinite(got["x2d"].cpu()[keep]).all())
    assert same_bits(got["x2d"].cpu()[~keep], y[~keep])              # unfilled: the input's bits


def test_idempotent_on_the_device():
    from pafuse_amd import ops
    x, conf, anchor = inputs(134, 70, seed=8)
    for r in (3, 13):
        once = ops.repair_detections(x.to(DEV), conf.to(DEV), anchor=anchor, radius=r)
        twice = ops.repair_detections(once["x2d"], once["conf"], anchor=anchor, radius=r)
        assert same_bits(twice["x2d"], once["x2d"]) and torch.equal(twice["status"], once["status"]) and same_bits(twice["conf"], once["conf"])


def test_the_torch_op_is_the_op_and_the_raw_entry_refuses():
    import pafuse_amd.torch_ops  # noqa: F401
    from pafuse_amd import harness, ops
    J, N, r = 134, 9, 3
    x, conf, anchor = inputs(J, N, seed=9)
    xd, cd = x.to(DEV), conf.to(DEV)
    want = ops.repair_detections(xd, cd, anchor=anchor, radius=r, threshold=0.25)
    got = torch.ops.pafuse.repair_detections(xd, cd, anchor, r, 0.25)
    assert same_bits(got[0], want["x2d"]) and same_bits(got[1], want["conf"]) and torch.equal(got[2], want["status"])
    host = harness.repair_detections(x, conf, anchor=anchor, radius=r, threshold=0.25)
    assert set(host) == {"x2d", "conf", "status", "counts"} and all(not v.is_cuda for v in host.values())
    assert same_bits(host["x2d"], want["x2d"].cpu()) and torch.equal(host["status"], want["status"].cpu())
    assert host["counts"].tolist() == torch.bincount(host["status"].reshape(-1).long(), minlength=4).tolist() and int(host["counts"].sum()) == N * J
    by_dataset = harness.repair_detections(x, conf, dataset=dataset(), radius=r)
    from pafuse_amd.detections import repair_anchors
    assert same_bits(by_dataset["x2d"], ops.repair_detections(xd, cd, anchor=repair_anchors(dataset()), radius=r)["x2d"].cpu())
    out = torch.full((N, J, 2), 7.0, device=DEV)
    status = torch.full((N, J), 7, dtype=torch.uint8, device=DEV)
    E_ARG = -1
    for kw in (dict(x=None), dict(conf=None), dict(out=None), dict(status=None), dict(N=0), dict(J=0), dict(r=0), dict(r=65),
               dict(threshold=-1.0), dict(threshold=float("nan")), dict(out=xd), dict(conf_out=cd)):
        a = dict(x=xd, conf=cd, anchor=None, N=N, J=J, r=r, threshold=0.0, out=out, conf_out=None, status=status)
        a.update(kw)
        assert raw(**a) == E_ARG, kw
    assert bool((out == 7.0).all()) and bool((status == 7).all())    # nothing was launched on them


# --------------------------------------------------------------------------------------------------------- infer_sequence
SEED = 2468
F27 = 27
N_VIDEO = 2 * F27 + 6
R = 5


@pytest.fixture(scope="module")
def video():
    """the suite's seeded video with planted dropouts (runs of 4 frames, a fifth of the joints), its repair, and the small model;
    computed once and never modified"""
    from __graft_entry__ import make_model
    from pafuse_amd import detections, harness
    model = make_model(5, 2, depth=2)[0]
    seq_2d, seq_3d, cam = sequence(N_VIDEO)
    lost = detections.plant_dropouts(N_VIDEO, 134, 0.2, 4, 3)
    x, conf = (torch.from_numpy(v) for v in detections.drop(seq_2d.numpy(), lost))
    fixed = harness.repair_detections(x, conf, dataset=dataset(), radius=R)
    return SimpleVideo(model, x, conf, fixed, seq_2d, seq_3d, cam)


class SimpleVideo:
    def __init__(self, model, x, conf, fixed, clean, seq_3d, cam):
        self.model, self.x, self.conf, self.fixed, self.clean, self.seq_3d, self.cam = model, x, conf, fixed, clean, seq_3d, cam

    def infer(self, seq_2d, **kw):
        from pafuse_amd import harness
        self.model.noise_fn, self.model.noise, self.model.noise_seed = None, "device", SEED
        return harness.infer_sequence(self.model, dataset(), seq_2d, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT, batch_size=2, **kw)


def test_infer_sequence_repair_none_is_the_call_without_it(video):
    assert same_bits(video.infer(video.x, aggregate="mean"), video.infer(video.x, aggregate="mean", repair=None))
    assert same_bits(video.infer(video.x), video.infer(video.x, repair=None, repair_threshold=0.0))


def test_infer_sequence_repair_is_infer_sequence_on_the_repaired_pair(video):
    fixed = video.fixed
    assert int(fixed["counts"][1]) > 1000 and int(fixed["counts"][0]) == int((video.conf > 0).sum())
    # aggregate="mean": a tensor keeps its type
    got = video.infer(video.x, aggregate="mean", conf=video.conf, repair=R)
    want = video.infer(fixed["x2d"], aggregate="mean")
    assert isinstance(got, torch.Tensor) and same_bits(got, want)
    assert not same_bits(got, video.infer(video.x, aggregate="mean"))           # the argument is not ignored
    # with a stride: a dict, which gains "repaired"
    got = video.infer(video.x, aggregate="mean", stride=F27 - 1, conf=video.conf, repair=R)
    want = video.infer(fixed["x2d"], aggregate="mean", stride=F27 - 1)
    assert set(got) == set(want) | {"repaired"} and all(same_bits(got[k], want[k]) for k in want)
    assert got["repaired"].dtype == torch.uint8 and torch.equal(got["repaired"], fixed["status"])
    # aggregate="reproj_fit": the fit and the pick see the repaired detections and the zeroed confidences; a tuple stays a tuple
    got = video.infer(video.x, aggregate="reproj_fit", cam=video.cam, conf=video.conf, repair=R)
    want = video.infer(fixed["x2d"], aggregate="reproj_fit", cam=video.cam, conf=fixed["conf"])
    assert isinstance(got, tuple) and len(got) == 2 and same_bits(got[0], want[0]) and torch.equal(got[1], want[1])
    other = video.infer(fixed["x2d"], aggregate="reproj_fit", cam=video.cam, conf=video.conf.clamp(min=0.5))
    assert not torch.equal(got[1], other[1])                                   # the confidences that arrive are the zeroed ones


def test_evaluate_frames_with_dropouts_and_repair(video):
    from pafuse_amd import harness

    def run(**kw):
        video.model.noise_fn, video.model.noise, video.model.noise_seed = None, "device", SEED
        return harness.evaluate_frames(video.model, dataset(), video.clean, video.seq_3d, video.cam, gu.SYN_JOINTS_LEFT,
                                       gu.SYN_JOINTS_RIGHT, aggregate="mean", stride=F27, **kw)

    clean = run()
    dropped = run(drop=(0.2, 4, 3))
    both = run(drop=(0.2, 4, 3), repair=R)
    assert len(clean) == 2 and len(dropped) == 3 and len(both) == 3
    for sums, counts in (dropped[:2], both[:2]):
        assert set(sums) == set(clean[0]) and all(bool(torch.isfinite(v).all()) for v in sums.values())
        assert all(torch.equal(counts[k], clean[1][k]) for k in counts)
    assert not torch.equal(dropped[0]["mpjpe"], clean[0]["mpjpe"])               # drop alone changes the sums
    assert not torch.equal(both[0]["mpjpe"], dropped[0]["mpjpe"])
    assert set(dropped[2]) == {"lost", "x2d", "conf"} and set(both[2]) == {"lost", "status", "x2d", "conf"}
    assert same_bits(dropped[2]["x2d"], video.x) and same_bits(dropped[2]["conf"], video.conf)    # the same planting
    assert same_bits(both[2]["x2d"], video.fixed["x2d"]) and torch.equal(both[2]["status"], video.fixed["status"])
    assert torch.equal(both[2]["status"] != 0, both[2]["lost"])


def test_h3wb_evaluate_frames_plants_per_video_and_logs_the_repair_error(video):
    from pafuse_amd import h3wb, harness
    clean, gt, cam = video.clean.numpy(), video.seq_3d.numpy(), video.cam.numpy()
    lines = []
    video.model.noise_fn, video.model.noise, video.model.noise_seed = None, "device", SEED
    rep = h3wb.evaluate_frames(video.model, dataset(), [cam, cam], [gt, gt], [clean, clean], gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                               stride=F27, log=lines.append, drop=(0.2, 4, 3), repair=R)
    assert all(v == v for v in rep["mpjpe"])
    counts = [l for l in lines if "detections observed" in l]
    errors = [l for l in lines if "repair error all" in l]
    assert len(counts) == 2 and len(errors) == 2 and counts[0] != counts[1]          # seed + the video's number: other dropouts
    assert counts[0] == "video 0 : detections observed %d, filled %d, held %d, unfilled %d" % tuple(video.fixed["counts"].tolist())
    assert sum("repair error" in l for l in lines) == 2 * (1 + len(dataset().parts_joint_indices))
    video.model.noise_seed = SEED
    one = harness.evaluate_frames(video.model, dataset(), video.clean, video.seq_3d, video.cam, gu.SYN_JOINTS_LEFT, gu.SYN_JOINTS_RIGHT,
                                  stride=F27, drop=(0.2, 4, 4), repair=R)
    assert counts[1] == "video 1 : detections observed %d, filled %d, held %d, unfilled %d" % tuple(
        torch.bincount(one[2]["status"].reshape(-1).long(), minlength=4).tolist())

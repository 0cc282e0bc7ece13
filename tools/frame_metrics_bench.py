"""Cost of the frame-level evaluation against the kernel that produces the array it consumes.

    python tools/frame_metrics_bench.py [--out profiles/frame_metrics_bench.json] [--reps 30]

A frame pose state of N video frames (T = 10, J = 134; N = 27: one window, N = 594: 22 clips' worth of video) is filled once with
seeded sums.  Leg "finish", the yardstick: pafuse_frames_finish writing the mean pose [T,N,J,3] of that state (mean only).  Leg
"errors": pafuse_frame_errors on that mean pose with a ground truth, a trajectory and its ground truth, writing err and cnt
[T,N,10].  Leg "reduce": pafuse_frame_errors_reduce of those maps.  All legs are bare ctypes calls on buffers allocated before the
timed region; HIP events around each leg, warm, the legs alternating.  These are call times (launches included), not kernel times.

The expectation, stated from the bytes before the measurement (r = T N J rows): finish reads 24 r + 4 N and writes 12 r; the
errors kernel asks for up to 3 x 12 r of pose and 3 x 12 N J of gt (the rows of frames n-1 and n+1 are read again by the
neighbouring waves, and the part roots' rows lie in them), of which 12 r + 12 N J are distinct bytes, and writes 120 T N; the
reduce reads 120 T N and writes 160 T.  If L2 serves the repeats the pair moves about a third of the finish's bytes; if it cost
more than the 3x traffic explains, the time is latency (one wave per frame, three dependent rounds of loads, eight butterflies).
Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats; a difference between two legs' minima below the larger
spread is not a difference.  One run on one box is a single observation.  Nothing is asserted on the times.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, J, P, PARTS = 10, 134, 5, 4


class Legs:
    """the three legs on one frame state as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, ops, N, seed):
        from pafuse_amd import synthetic as gu
        from pafuse_amd.evaluate import _part_table, _tables
        from types import SimpleNamespace
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(seed)
        ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                             parts_connection_indices=dict(gu.CONNECTION_INDICES))
        self.pbroot, self.part = _tables(ds, J, "cuda")[1], _part_table(ds, J, "cuda")
        self.frame = ops.frame_state(N, T, J)
        v = ops.frame_views(self.frame, N, T, J)
        pose = torch.randn(T, N, J, 3, generator=g) * 0.25                       # the mean the state holds: sum = P * pose
        pose[:, :, 0] = 0
        v["sum"].copy_((pose.double() * P).cuda())
        v["count"].fill_(P)
        gt = pose[0] + torch.randn(N, J, 3, generator=g) * 0.05
        gt[:, 0] = 0
        root = torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.3, -0.2, 4.5])
        self.gt, self.gt_root = gt.contiguous().cuda(), root.contiguous().cuda()
        self.traj = (root[None] + torch.randn(T, N, 3, generator=g) * 0.02).contiguous().cuda()
        self.mean = torch.empty(T, N, J, 3, device="cuda")
        K = 6 + PARTS
        self.err, self.cnt = torch.empty(T, N, K, device="cuda", dtype=torch.float64), torch.empty(T, N, K, device="cuda", dtype=torch.int32)
        self.sums, self.counts = torch.empty(T, K, device="cuda", dtype=torch.float64), torch.empty(T, K, device="cuda", dtype=torch.int64)
        p = lambda t: t.data_ptr()
        self.finish = [p(self.frame), None, N, T, J, p(self.mean), None, None, None, None, None, stream]
        self.errors = [p(self.mean), p(self.gt), p(self.traj), p(self.gt_root), p(self.pbroot), p(self.part), PARTS, T, N, J,
                       p(self.err), p(self.cnt), stream]
        self.reduce = [p(self.err), p(self.cnt), T, N, K, p(self.sums), p(self.counts), stream]
        r = T * N * J
        self.bytes = {"finish": 24 * r + 4 * N + 12 * r, "errors": 12 * r + 12 * N * J + 12 * T * N + 12 * N + 12 * K * T * N,
                      "reduce": 12 * K * T * N + 16 * K * T}
        self.pose, self.N = pose, N

    def finish_leg(self):
        self.check(self.lib.pafuse_frames_finish(*self.finish))

    def errors_leg(self):
        self.check(self.lib.pafuse_frame_errors(*self.errors))

    def reduce_leg(self):
        self.check(self.lib.pafuse_frame_errors_reduce(*self.reduce))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_metrics_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, ops
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    names = ("finish", "errors", "reduce")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "cost": []}
    for N in (27, 594):
        legs = Legs(torch, lib, _lib.check, ops, N, seed=230 + N)
        times = {k: [] for k in names}
        for _ in range(3):                                           # warm: code objects, caches
            for k in names:
                getattr(legs, k + "_leg")()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, k + "_leg")()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_frame_metrics.py): the mean is the pose the
        # state was filled with, every joint of every frame was scored, and the errors are the planted 5 cm and 2 cm
        assert torch.equal(legs.mean.cpu(), legs.pose)
        counts, sums = legs.counts.cpu(), legs.sums.cpu()
        assert counts[:, 0].tolist() == [N * J] * T and counts[:, 3].tolist() == [N] * T
        assert 0.02 < float(sums[0, 0] / counts[0, 0]) < 0.5 and float(sums[0, 3] / counts[0, 3]) < 0.1
        row = {"T": T, "N": N, "J": J, "num_parts": PARTS}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "useful_bytes": legs.bytes[k],
                      "useful_GB_per_s": round(legs.bytes[k] / t[0] / 1e3, 1)}
        row["errors_plus_reduce_over_finish_min"] = round((row["errors"]["min_us"] + row["reduce"]["min_us"]) / row["finish"]["min_us"], 3)
        row["errors_over_finish_min"] = round(row["errors"]["min_us"] / row["finish"]["min_us"], 3)
        row["ratio_spread"] = round((max(row["errors"]["spread_us"], row["reduce"]["spread_us"], row["finish"]["spread_us"]))
                                    / row["finish"]["min_us"], 3)
        doc["cost"].append(row)
        print(json.dumps(row), flush=True)
        del legs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Cost of the camera-space root trajectory against the kernel that produces the array it consumes.

    python tools/trajectory_bench.py [--out profiles/trajectory_bench.json] [--reps 30]

A frame pose state of N video frames (T = 10, J = 134; N = 27: one window, N = 594: 22 clips' worth of video) is filled once with
seeded sums.  Leg "finish", the yardstick: pafuse_frames_finish writing the mean pose [T,N,J,3] of that state (mean only).  Leg
"fit": pafuse_frames_root_fit on that mean pose with detections, confidences and intrinsics, writing traj, wsum and resid.  Leg
"smooth": pafuse_trajectory_smooth (radius 4) of the fitted trajectory with wsum as weights.  All legs are bare ctypes calls on
buffers allocated before the timed region; HIP events around each leg, warm, the legs alternating.  These are call times
(launches included), not kernel times.

The expectation, stated from the bytes before the measurement (r = T N J rows): finish reads 24 r + 4 N and writes 12 r; the fit
reads 12 r + 12 N J (+ 4 N J of weights) and writes 20 T N - about 0.4 of the finish's bytes, the same order; the smoother reads
at most 9 x 16 bytes per (t, n) out of a 95 KB array and writes 12: it is launch-bound at either N, and at N = 27 so are all three.
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

T, J, RADIUS, P = 10, 134, 4, 5


class Legs:
    """the three legs on one frame state as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, ops, N, seed):
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(seed)
        self.frame = ops.frame_state(N, T, J)
        v = ops.frame_views(self.frame, N, T, J)
        pose = torch.randn(T, N, J, 3, generator=g) * 0.25                       # the mean the state holds: sum = P * pose
        pose[:, :, 0] = 0
        v["sum"].copy_((pose.double() * P).cuda())
        v["count"].fill_(P)
        X = pose[0].double() + torch.tensor([0.3, -0.2, 4.5], dtype=torch.float64)
        self.x2d = (2.29 * X[..., :2] / X[..., 2:]).float().contiguous().cuda()  # [N,J,2]: step 0's pose seen from 4.5 m
        self.conf = (torch.rand(N, J, generator=g) * 0.9 + 0.1).cuda()
        self.cam = torch.tensor([2.29, 2.29, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32).cuda()
        self.mean = torch.empty(T, N, J, 3, device="cuda")
        self.traj, self.out = torch.empty(T, N, 3, device="cuda"), torch.empty(T, N, 3, device="cuda")
        self.wsum, self.resid = torch.empty(T, N, device="cuda"), torch.empty(T, N, device="cuda")
        p = lambda t: t.data_ptr()
        self.finish = [p(self.frame), None, N, T, J, p(self.mean), None, None, None, None, None, stream]
        self.fit = [p(self.mean), p(self.x2d), p(self.conf), p(self.cam), T, N, J, p(self.traj), p(self.wsum), p(self.resid), stream]
        self.smooth = [p(self.traj), p(self.wsum), T, N, RADIUS, p(self.out), stream]
        r = T * N * J
        self.bytes = {"finish": 24 * r + 4 * N + 12 * r, "fit": 12 * r + 16 * N * J + 20 * T * N, "smooth": 28 * T * N}
        self.pose = pose

    def finish_leg(self):
        self.check(self.lib.pafuse_frames_finish(*self.finish))

    def fit_leg(self):
        self.check(self.lib.pafuse_frames_root_fit(*self.fit))

    def smooth_leg(self):
        self.check(self.lib.pafuse_trajectory_smooth(*self.smooth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, ops
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    names = ("finish", "fit", "smooth")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "cost": []}
    for N in (27, 594):
        legs = Legs(torch, lib, _lib.check, ops, N, seed=90 + N)
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
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_trajectory.py): the mean is the pose the
        # state was filled with, step 0's fit finds the root it was seen from, and the filter leaves no frame without a root
        assert torch.equal(legs.mean.cpu(), legs.pose)
        assert float((legs.traj[0].cpu() - torch.tensor([0.3, -0.2, 4.5])).abs().max()) < 1e-3
        assert bool(torch.isfinite(legs.out).all())
        row = {"T": T, "N": N, "J": J, "radius": RADIUS}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "useful_bytes": legs.bytes[k],
                      "useful_GB_per_s": round(legs.bytes[k] / t[0] / 1e3, 1)}
        row["fit_plus_smooth_over_finish_min"] = round((row["fit"]["min_us"] + row["smooth"]["min_us"]) / row["finish"]["min_us"], 3)
        row["fit_over_finish_min"] = round(row["fit"]["min_us"] / row["finish"]["min_us"], 3)
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

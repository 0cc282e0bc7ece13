"""Cost of the focal-length estimate against the root fit that runs on the same frames.

    python tools/focal_bench.py [--out profiles/focal_bench.json] [--reps 30]

A per-frame pose [T,N,J,3] (T = 10, J = 134; N = 27: one window, N = 594: 22 clips' worth of video) seen from 4.5 m through a camera
of focal length 2.29, with seeded confidences.  Leg "fit", the yardstick: pafuse_frames_root_fit on it with the true intrinsics,
writing traj, wsum and resid.  Leg "sums": pafuse_frames_focal_sums on the same operands, writing the state [T,N,4].  Leg "solve":
pafuse_focal_solve of that state, writing focal, r2, frames and cam_out.  All legs are bare ctypes calls on buffers allocated
before the timed region; HIP events around each leg, warm, the legs alternating.  These are call times (launches included), not
kernel times.

The expectation, stated from the bytes before the measurement (r = T N J rows): the sums read what the fit reads, 12 r + 12 N J
(+ 4 N J of weights), and write 32 T N where the fit writes 20 T N; thirteen butterfly chains instead of the fit's seven plus one
behind the solve - about twice the cross-lane traffic, none of it through memory.  The solve reads 32 T N and writes 48 T: it is
launch-bound at either N, and at N = 27 so are all three.  So sums + solve should cost about the fit plus one launch.
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

T, J, FOCAL = 10, 134, 2.29
ROOT_TRUE = (0.3, -0.2, 4.5)


class Legs:
    """the three legs on one per-frame pose as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, N, seed):
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(seed)
        pose = torch.randn(1, N, J, 3, generator=g) * 0.25
        pose[:, :, 0] = 0
        X = pose[0].double() + torch.tensor(ROOT_TRUE, dtype=torch.float64)
        self.x2d = (FOCAL * X[..., :2] / X[..., 2:]).float().contiguous().cuda()  # [N,J,2]: the pose seen from 4.5 m
        self.pose = pose.expand(T, N, J, 3).contiguous().cuda()
        self.conf = (torch.rand(N, J, generator=g) * 0.9 + 0.1).cuda()
        self.cam = torch.tensor([FOCAL, FOCAL, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32).cuda()
        self.guess = torch.tensor([1, 1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32).cuda()
        self.traj = torch.empty(T, N, 3, device="cuda")
        self.wsum, self.resid = torch.empty(T, N, device="cuda"), torch.empty(T, N, device="cuda")
        self.state = torch.empty(T, N, 4, device="cuda", dtype=torch.float64)
        self.focal, self.r2 = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
        self.frames, self.cam_out = torch.empty(T, device="cuda", dtype=torch.int32), torch.empty(T, 9, device="cuda")
        p = lambda t: t.data_ptr()
        self.fit = [p(self.pose), p(self.x2d), p(self.conf), p(self.cam), T, N, J, p(self.traj), p(self.wsum), p(self.resid), stream]
        self.sums = [p(self.pose), p(self.x2d), p(self.conf), p(self.guess), T, N, J, p(self.state), stream]
        self.solve = [p(self.state), T, N, p(self.guess), 9, p(self.focal), p(self.r2), p(self.frames), p(self.cam_out), stream]
        r = T * N * J
        self.bytes = {"fit": 12 * r + 16 * N * J + 20 * T * N, "sums": 12 * r + 16 * N * J + 32 * T * N, "solve": 32 * T * N + 48 * T}

    def fit_leg(self):
        self.check(self.lib.pafuse_frames_root_fit(*self.fit))

    def sums_leg(self):
        self.check(self.lib.pafuse_frames_focal_sums(*self.sums))

    def solve_leg(self):
        self.check(self.lib.pafuse_focal_solve(*self.solve))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    names = ("fit", "sums", "solve")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "cost": []}
    for N in (27, 594):
        legs = Legs(torch, lib, _lib.check, N, seed=90 + N)
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
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_focal.py): the fit finds the root the pose
        # was seen from, every frame took part, and the estimate is the focal length the detections were made with
        assert float((legs.traj[0].cpu() - torch.tensor(ROOT_TRUE)).abs().max()) < 1e-3
        assert legs.frames.tolist() == [N] * T
        assert float((legs.focal.cpu() / FOCAL - 1).abs().max()) < 1e-4
        row = {"T": T, "N": N, "J": J}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "useful_bytes": legs.bytes[k],
                      "useful_GB_per_s": round(legs.bytes[k] / t[0] / 1e3, 1)}
        row["sums_plus_solve_over_fit_min"] = round((row["sums"]["min_us"] + row["solve"]["min_us"]) / row["fit"]["min_us"], 3)
        row["sums_over_fit_min"] = round(row["sums"]["min_us"] / row["fit"]["min_us"], 3)
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

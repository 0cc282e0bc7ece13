"""Cost of the ground-plane estimate against the root fit and the smoother that run on the same frames.

    python tools/ground_bench.py [--out profiles/ground_bench.json] [--reps 30]

A per-frame pose [T,N,J,3] (T = 10, J = 134, K = 6 foot points, radius 3, 3 passes; N = 27: one window, N = 594: 22 clips' worth of
video, N = 5 000: three minutes of it): a seeded rigid figure seen from 4.5 m whose root drifts at 5 mm/frame, so that every foot
point is a contact in every frame - the most arithmetic the sums can meet.  Legs, each a bare ctypes call on buffers allocated before
the timed region: "contacts" pafuse_foot_contacts; "sums" pafuse_ground_sums without a plane (the first pass); "sums_later" the
same reading a plane and a scale; "solve" pafuse_ground_solve; "world" pafuse_frames_to_world; "chain" the 1 + 2*3 + 1 calls of
ops.estimate_ground back to back.  The yardsticks on the same frames: "fit" pafuse_frames_root_fit, "smooth"
pafuse_trajectory_smooth (radius 3), and "copy" one device-to-device copy of pose (Tensor.copy_: the price of touching the pose
once).  HIP events around each leg, warm, the legs alternating in one process.  These are call times (launches included), not
kernel times.

The expectation, stated from the bytes before the measurement (r = T N J rows): contacts read K/J of the pose seven times over
(the windows overlap; the caches see it once) and write 20 T N K bytes; the sums read those and write 112 T N; the solve reads
112 T N with T waves - ten waves on a chip of 256 CUs: latency-bound whatever N is; the world reads 12 r + 12 T N and writes the
same: the one leg that touches the whole pose, so it should cost about the copy and dominate the chain once N is large, with
everything launch-bound at N = 27.  Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats; a difference between
two legs' minima below the larger spread is not a difference.  One run on one box is a single observation.  Nothing is asserted
on the times.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, J, K, RADIUS, PASSES, FOCAL = 10, 134, 6, 3, 3, 2.29
SPEED, GATE, FLOOR, SPREAD = 0.015, 2.5, 0.005, 0.03           # the defaults of ops.estimate_ground: defaults, not tuned values
ROOT_TRUE = (0.3, -0.2, 4.5)
DRIFT = (0.004, 0.0, 0.003)                                   # metres per frame: 5 mm


class Legs:
    """the legs on one per-frame pose as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, N, seed):
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(seed)
        figure = torch.randn(1, 1, J, 3, generator=g) * 0.25
        figure[:, :, 0] = 0
        there_and_back = (((torch.arange(N) + 250) % 500) - 250).abs().double()          # 250 frames out, 250 back: the figure stays in view
        root = torch.tensor(ROOT_TRUE, dtype=torch.float64) + there_and_back[:, None] * torch.tensor(DRIFT, dtype=torch.float64)
        X = figure[0].double() + root[:, None]
        self.x2d = (FOCAL * X[..., :2] / X[..., 2:]).float().contiguous().cuda()       # [N,J,2]
        self.pose = figure.expand(T, N, J, 3).contiguous().cuda()
        self.root = root
        self.conf = (torch.rand(N, J, generator=g) * 0.9 + 0.1).cuda()
        self.cam = torch.tensor([FOCAL, FOCAL, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32).cuda()
        self.points = torch.arange(18, 18 + K, dtype=torch.int32).cuda()
        f32 = lambda *s: torch.empty(*s, device="cuda")
        f64 = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float64)
        self.raw, self.wsum, self.resid, self.traj = f32(T, N, 3), f32(T, N), f32(T, N), f32(T, N, 3)
        self.foot, self.speed, self.contact = f32(T, N, K, 3), f32(T, N, K), f32(T, N, K)
        self.state, self.plane, self.scale = f64(T, N, 14), f64(T, 4), f64(T)
        self.up, self.height, self.rms, self.eig = f32(T, 3), f32(T), f32(T), f32(T, 3)
        self.count, self.code = torch.empty(T, device="cuda", dtype=torch.int32), torch.empty(T, device="cuda", dtype=torch.uint8)
        self.pose_world, self.traj_world, self.pose_copy = f32(T, N, J, 3), f32(T, N, 3), f32(T, N, J, 3)
        p = lambda t: t.data_ptr()
        self.a_fit = [p(self.pose), p(self.x2d), p(self.conf), p(self.cam), T, N, J, p(self.raw), p(self.wsum), p(self.resid), stream]
        self.a_smooth = [p(self.raw), p(self.wsum), T, N, RADIUS, p(self.traj), stream]
        self.a_contacts = [p(self.pose), p(self.traj), p(self.points), T, N, J, K, RADIUS, SPEED, p(self.foot), p(self.speed), p(self.contact), stream]
        sums = lambda plane, scale: [p(self.foot), p(self.contact), p(self.traj), plane, scale, T, N, K, GATE, p(self.state), stream]
        self.a_sums, self.a_sums_later = sums(None, None), sums(p(self.plane), p(self.scale))
        self.a_solve = [p(self.state), T, N, FLOOR, SPREAD, p(self.plane), p(self.scale), p(self.up), p(self.height), p(self.rms), p(self.eig),
                        p(self.count), p(self.code), stream]
        self.a_world = [p(self.pose), p(self.traj), p(self.plane), T, N, J, p(self.pose_world), p(self.traj_world), stream]
        r = T * N * J
        self.bytes = {"fit": 12 * r + 16 * N * J + 20 * T * N, "smooth": 16 * T * N + 12 * T * N, "copy": 24 * r,
                      "contacts": 12 * T * N * K + 12 * T * N + 20 * T * N * K, "sums": 16 * T * N * K + 12 * T * N + 112 * T * N,
                      "sums_later": 16 * T * N * K + 12 * T * N + 112 * T * N + 40 * T, "solve": 112 * T * N + 78 * T,
                      "world": 24 * r + 24 * T * N + 32 * T}
        self.bytes["chain"] = self.bytes["contacts"] + self.bytes["sums"] + (PASSES - 1) * self.bytes["sums_later"] + PASSES * self.bytes["solve"] + self.bytes["world"]

    def fit_leg(self):
        self.check(self.lib.pafuse_frames_root_fit(*self.a_fit))

    def smooth_leg(self):
        self.check(self.lib.pafuse_trajectory_smooth(*self.a_smooth))

    def copy_leg(self):
        self.pose_copy.copy_(self.pose)

    def contacts_leg(self):
        self.check(self.lib.pafuse_foot_contacts(*self.a_contacts))

    def sums_leg(self):
        self.check(self.lib.pafuse_ground_sums(*self.a_sums))

    def sums_later_leg(self):
        self.check(self.lib.pafuse_ground_sums(*self.a_sums_later))

    def solve_leg(self):
        self.check(self.lib.pafuse_ground_solve(*self.a_solve))

    def world_leg(self):
        self.check(self.lib.pafuse_frames_to_world(*self.a_world))

    def chain_leg(self):
        self.contacts_leg()
        self.sums_leg()
        self.solve_leg()
        for _ in range(PASSES - 1):
            self.sums_later_leg()
            self.solve_leg()
        self.world_leg()


NAMES = ("fit", "smooth", "copy", "contacts", "sums", "solve", "sums_later", "world", "chain")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "shape": {"T": T, "J": J, "K": K, "radius": RADIUS, "passes": PASSES}, "cost": []}
    for N in (27, 594, 5000):
        legs = Legs(torch, lib, _lib.check, N, seed=90 + N)
        times = {k: [] for k in NAMES}
        for _ in range(3):                                           # warm: code objects, caches; the order gives every leg its operands
            for k in NAMES:
                getattr(legs, k + "_leg")()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k in NAMES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, k + "_leg")()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_ground.py): the fit finds the roots the figure
        # was seen from, every foot point is a contact before the re-weighting, and the chain ends with a plane
        assert float((legs.raw[0].double().cpu() - legs.root).abs().max()) < 1e-3
        assert bool((legs.contact > 0).all()) if N > 2 * RADIUS else True
        assert bool((legs.code != 0).all()) and bool(torch.isfinite(legs.pose_world).all())
        row = {"N": N, "codes": legs.code.tolist(), "points": legs.count.tolist()}
        for k in NAMES:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "useful_bytes": legs.bytes[k],
                      "useful_GB_per_s": round(legs.bytes[k] / t[0] / 1e3, 1)}
        parts = row["contacts"]["min_us"] + row["sums"]["min_us"] + (PASSES - 1) * row["sums_later"]["min_us"] + PASSES * row["solve"]["min_us"] + row["world"]["min_us"]
        row["sum_of_the_legs_min_us"] = round(parts, 2)
        row["chain_over_fit_min"] = round(row["chain"]["min_us"] / row["fit"]["min_us"], 3)
        row["chain_over_fit_plus_smooth_min"] = round(row["chain"]["min_us"] / (row["fit"]["min_us"] + row["smooth"]["min_us"]), 3)
        row["world_over_copy_min"] = round(row["world"]["min_us"] / row["copy"]["min_us"], 3)
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

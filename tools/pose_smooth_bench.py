"""Cost of the covariance-weighted pose smoother against the kernel that produces the arrays it consumes.

    python tools/pose_smooth_bench.py [--out profiles/pose_smooth_bench.json] [--reps 30]

A frame pose state and a frame spread state of N video frames (T = 10, J = 134; N = 27: one window, N = 594: 22 clips' worth of
video, N = 5000: a long video) are filled once with seeded sums.  Leg "finish", the yardstick: pafuse_frames_finish writing the
mean pose [T,N,J,3] and the covariance [T,N,J,6] of those states.  Leg "smooth": pafuse_pose_smooth (radius 13, floor 1 mm; its
pair of launches) on that mean and covariance, writing the smoothed pose and the code.  Leg "smooth_nocov": the same with cov =
NULL.  All legs are bare ctypes calls on buffers allocated before the timed region, the workspace included; HIP events around
each leg, warm, the legs alternating in one process.  These are call times (launches included), not kernel times.

No time is fixed in advance.  What is reported per leg: min, median, p90 and `spread_us` = p90 - min of its repeats (a
difference between two legs' minima below the larger spread is not a difference); the bytes every array is read or written ONCE
(`once_bytes`: per row 36 in, 48 of precision out and in again, 12 of pose in again, 13 out for the smoother - the (2r+1)-fold
re-reads of its second kernel are meant to be cache hits - and 72 + 36 for the finish) and the rate they give at the minimum; the
bytes the second kernel's loads ask for (`visit_bytes`: 60 per visit); and the fp64 work: per row 26 additions /
multiplications and 6 divisions (the precision), per visit 60 and 1 (the taper, G, z, the 24 sums), per output 106 and 18 (the 6x6
LDL^T) - `fp64_Gop_per_s` counts a division as ONE operation, so the true instruction rate is higher by the length of the division
sequence.  Contraction is off: a multiply-add is two instructions, which halves the ceiling a fused peak would give.  One run on one
box is a single observation.  Nothing is asserted on the times.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, J, RADIUS, P, FLOOR = 10, 134, 13, 5, 1e-3
ROW_OPS, ROW_DIVS, VISIT_OPS, VISIT_DIVS, SOLVE_OPS, SOLVE_DIVS = 26, 6, 60, 1, 106, 18


def visits(N, r):
    """the (frame, neighbour) pairs one track walks"""
    return sum(min(N - 1, n + r) - max(0, n - r) + 1 for n in range(N))


class Legs:
    """the legs on one pair of frame states as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, ops, N, seed):
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(seed)
        self.frame = ops.frame_state(N, T, J)
        self.spread = ops.frame_state(N, T, J, spread=True)
        pose = torch.cumsum(torch.randn(T, N, J, 3, generator=g) * 0.02, dim=1) + torch.randn(T, 1, J, 3, generator=g) * 0.25
        v = ops.frame_views(self.frame, N, T, J)
        v["sum"].copy_((pose.double() * P).cuda())
        v["count"].fill_(P)
        A = torch.randn(T, N, J, 3, 3, generator=g, dtype=torch.float64) * 0.03     # Sigma = A A^T: a few centimetres, anisotropic
        S = A @ A.transpose(-1, -2)
        m2 = torch.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2], S[..., 2, 2]], dim=-1) * P
        s = ops.frame_views(self.spread, N, T, J, spread=True)
        s["sum"].copy_((pose.double() * P).cuda())
        s["m2"].copy_(m2.cuda())
        s["count"].fill_(P)
        self.mean, self.cov = torch.empty(T, N, J, 3, device="cuda"), torch.empty(T, N, J, 6, device="cuda")
        self.out, self.code = torch.empty(T, N, J, 3, device="cuda"), torch.empty(T, N, J, dtype=torch.uint8, device="cuda")
        p = lambda t: t.data_ptr()
        self.finish = [p(self.frame), p(self.spread), N, T, J, p(self.mean), None, None, None, None, p(self.cov), stream]
        self.ws = torch.empty(T * N * J * 6, dtype=torch.float64, device="cuda")
        assert self.ws.numel() * 8 == lib.pafuse_pose_smooth_workspace_bytes(T, N, J)
        tail = [T, N, J, RADIUS, FLOOR, p(self.out), p(self.code), p(self.ws), self.ws.numel() * 8, stream]
        self.smooth, self.smooth_nocov = [p(self.mean), p(self.cov)] + tail, [p(self.mean), None] + tail
        r, w = T * N * J, T * J * visits(N, RADIUS)
        self.once_bytes = {"finish": (72 + 36) * r + 12 * N, "smooth": (36 + 48 + 48 + 12 + 13) * r, "smooth_nocov": (12 + 48 + 48 + 12 + 13) * r}
        self.visit_bytes = {"smooth": 60 * w, "smooth_nocov": 60 * w}
        self.ops = w * (VISIT_OPS + VISIT_DIVS) + r * (ROW_OPS + ROW_DIVS + SOLVE_OPS + SOLVE_DIVS)
        self.divs = w * VISIT_DIVS + r * (ROW_DIVS + SOLVE_DIVS)
        self.pose = pose

    def finish_leg(self):
        self.check(self.lib.pafuse_frames_finish(*self.finish))

    def smooth_leg(self):
        self.check(self.lib.pafuse_pose_smooth(*self.smooth))

    def smooth_nocov_leg(self):
        self.check(self.lib.pafuse_pose_smooth(*self.smooth_nocov))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_smooth_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, ops
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    names = ("finish", "smooth", "smooth_nocov")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "fp64_ops_counted": {"per_row": [ROW_OPS, ROW_DIVS], "per_visit": [VISIT_OPS, VISIT_DIVS], "per_output": [SOLVE_OPS, SOLVE_DIVS],
                                "note": "additions/multiplications and divisions; a division counts as one operation"},
           "cost": []}
    for N in (27, 594, 5000):
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
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_pose_smooth.py): the mean is the pose the
        # states were filled with, and the last leg - no covariance - left a line at every (t, frame, joint)
        assert float((legs.mean.cpu() - legs.pose).abs().max()) < 1e-6
        assert bool(torch.isfinite(legs.out).all()) and bool((legs.code == 1).all())
        row = {"T": T, "N": N, "J": J, "radius": RADIUS, "floor": FLOOR}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "once_bytes": legs.once_bytes[k],
                      "once_GB_per_s": round(legs.once_bytes[k] / t[0] / 1e3, 1)}
            if k in legs.visit_bytes:
                row[k]["visit_bytes"] = legs.visit_bytes[k]
                row[k]["visit_GB_per_s"] = round(legs.visit_bytes[k] / t[0] / 1e3, 1)
        row["smooth"]["fp64_ops"], row["smooth"]["fp64_divisions"] = legs.ops, legs.divs
        row["smooth"]["fp64_Gop_per_s"] = round(legs.ops / row["smooth"]["min_us"] / 1e3, 1)
        row["smooth_over_finish_min"] = round(row["smooth"]["min_us"] / row["finish"]["min_us"], 3)
        row["smooth_nocov_over_smooth_min"] = round(row["smooth_nocov"]["min_us"] / row["smooth"]["min_us"], 3)
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

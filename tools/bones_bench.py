"""Cost of holding the bone lengths constant along a video against the kernel that produces the arrays it consumes.

    python tools/bones_bench.py [--out profiles/bones_bench.json] [--reps 30]

A frame pose state and a frame spread state of N video frames (T = 10, J = 134; N = 27: one window, N = 594: 22 clips' worth of
video, N = 5000: a long video) are filled once with seeded sums.  Leg "finish", the yardstick: pafuse_frames_finish writing the
mean pose [T,N,J,3] and the covariance [T,N,J,6] of those states.  Leg "lengths": pafuse_bone_lengths on that mean and covariance
with the H3WB tables of h3wb.bone_tables, mirror partners pooled, writing length, dev and frames.  Leg "project":
pafuse_bone_project with those lengths, 16 sweeps and the snap, writing the pose, the code and the residuals.  Leg "project_0": the
same with 0 sweeps - the set-up of a frame in LDS, the child lists, the snap and the residuals alone, so project - project_0 is what
the 16 sweeps cost.  All legs are bare ctypes calls on buffers allocated before the timed region; HIP events around each leg,
warm, the legs alternating in one process.  These are call times (launches included), not kernel times.

No time is fixed in advance.  What is reported per leg: min, median, p90 and `spread_us` = p90 - min of its repeats (a
difference between two legs' minima below the larger spread is not a difference); the bytes every array is read or written ONCE
(`once_bytes`: per (t, frame, joint) 36 in for both bone kernels, 13 out for the projection; 72 + 36 for the finish) and the
rate they give at the minimum; for the projection the frames per second and the time of one sweep of one frame's wave
(`us_per_sweep`: (project - project_0) / 16 / the rounds of waves the device holds at two workgroups per CU - an upper bound
where the grid does not fill the device).  The projection is latency-bound by design: 32 dependent LDS phases per wave, 134 of
192 lane slots busy, an fp64 square root and four divisions per bone and sweep with contraction off.  One run on one box is a
single observation.  Nothing is asserted on the times.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, J, SWEEPS, P, FLOOR = 10, 134, 16, 5, 1e-3


class Legs:
    """the legs on one pair of frame states as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, ops, N, seed):
        from pafuse_amd import h3wb
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(seed)
        parent, mirror = h3wb.bone_tables(68)
        self.parent, self.mirror = torch.from_numpy(parent).cuda(), torch.from_numpy(mirror).cuda()
        self.frame = ops.frame_state(N, T, J)
        self.spread = ops.frame_state(N, T, J, spread=True)
        # a skeleton with constant bone lengths whose bones turn slowly, plus 1 cm of noise: what the projection takes away
        u = torch.randn(T, 1, J, 3, generator=g) + torch.cumsum(torch.randn(T, N, J, 3, generator=g) * 0.05, dim=1)
        u = u / u.norm(dim=-1, keepdim=True)
        length = torch.where(torch.arange(J) >= 92, torch.rand(J, generator=g) * 0.03 + 0.02, torch.rand(J, generator=g) * 0.35 + 0.1)
        for j in range(J):                                            # left and right alike: the mirror partners pool their frames
            if mirror[j] > j:
                length[mirror[j]] = length[j]
        pose = torch.randn(T, 1, J, 3, generator=g).expand(T, N, J, 3).clone() * 0.05
        pose[:, :, 0] = 0
        for j in range(1, J):
            if parent[j] >= 0:
                pose[:, :, j] = pose[:, :, parent[j]] + u[:, :, j] * length[j]
        pose[:, :, 1:] += torch.randn(T, N, J - 1, 3, generator=g) * 0.01
        v = ops.frame_views(self.frame, N, T, J)
        v["sum"].copy_((pose.double() * P).cuda())
        v["count"].fill_(P)
        A = torch.randn(T, N, J, 3, 3, generator=g, dtype=torch.float64) * 0.01       # Sigma = A A^T: about a centimetre, anisotropic
        S = A @ A.transpose(-1, -2)
        m2 = torch.stack([S[..., 0, 0], S[..., 0, 1], S[..., 0, 2], S[..., 1, 1], S[..., 1, 2], S[..., 2, 2]], dim=-1) * P
        s = ops.frame_views(self.spread, N, T, J, spread=True)
        s["sum"].copy_((pose.double() * P).cuda())
        s["m2"].copy_(m2.cuda())
        s["count"].fill_(P)
        self.mean, self.cov = torch.empty(T, N, J, 3, device="cuda"), torch.empty(T, N, J, 6, device="cuda")
        self.length, self.dev = torch.empty(T, J, device="cuda"), torch.empty(T, J, device="cuda")
        self.frames = torch.empty(T, J, dtype=torch.int32, device="cuda")
        self.out, self.code = torch.empty(T, N, J, 3, device="cuda"), torch.empty(T, N, J, dtype=torch.uint8, device="cuda")
        self.resid = torch.empty(T, N, 2, device="cuda")
        p = lambda t: t.data_ptr()
        self.finish = [p(self.frame), p(self.spread), N, T, J, p(self.mean), None, None, None, None, p(self.cov), stream]
        self.lengths = [p(self.mean), p(self.cov), p(self.parent), p(self.mirror), T, N, J, FLOOR, p(self.length), p(self.dev), p(self.frames), stream]
        project = lambda sweeps: [p(self.mean), p(self.cov), p(self.parent), p(self.length), T, N, J, sweeps, 1, FLOOR, p(self.out), p(self.code),
                                  p(self.resid), stream]
        self.project, self.project_0 = project(SWEEPS), project(0)
        r = T * N * J
        self.once_bytes = {"finish": (72 + 36) * r + 12 * N, "lengths": 36 * r + 12 * T * J, "project": (36 + 13) * r + 8 * T * N,
                           "project_0": (36 + 13) * r + 8 * T * N}
        self.pose, self.bones = pose, int((parent >= 0).sum())

    def finish_leg(self):
        self.check(self.lib.pafuse_frames_finish(*self.finish))

    def lengths_leg(self):
        self.check(self.lib.pafuse_bone_lengths(*self.lengths))

    def project_leg(self):
        self.check(self.lib.pafuse_bone_project(*self.project))

    def project_0_leg(self):
        self.check(self.lib.pafuse_bone_project(*self.project_0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bones_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, ops
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    names = ("finish", "lengths", "project_0", "project")               # project last: its outputs are what the checks below read
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    doc = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box", "cost": []}
    for N in (27, 594, 5000):
        legs = Legs(torch, lib, _lib.check, ops, N, seed=70 + N)
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
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_bones.py): the mean is the pose the states
        # were filled with, every bone rests on all frames of both partners, and the snap left every frame exact in fp32
        assert float((legs.mean.cpu() - legs.pose).abs().max()) < 1e-6
        assert int((legs.frames > 0).sum()) == T * legs.bones and bool(torch.isfinite(legs.out).all())
        assert float(legs.resid[..., 1].max()) <= 1e-6 < float(legs.resid[..., 0].max())
        row = {"T": T, "N": N, "J": J, "sweeps": SWEEPS, "snap": 1, "floor": FLOOR, "bones": legs.bones,
               "resid_before_max_mm": round(float(legs.resid[..., 0].max()) * 1e3, 2), "bone_dev_mean_mm": round(float(legs.dev.nanmean()) * 1e3, 2)}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "once_bytes": legs.once_bytes[k],
                      "once_GB_per_s": round(legs.once_bytes[k] / t[0] / 1e3, 1)}
        waves = T * N
        rounds = -(-waves // (cus * 8))                              # two workgroups of four waves per CU
        row["project"]["frames_per_s"] = round(waves / row["project"]["min_us"] * 1e6)
        row["project"]["wave_rounds"] = rounds
        row["project"]["us_per_sweep"] = round((row["project"]["min_us"] - row["project_0"]["min_us"]) / SWEEPS / rounds, 3)
        both = row["lengths"]["min_us"] + row["project"]["min_us"]
        row["lengths_plus_project_min_us"] = round(both, 2)
        row["bones_over_finish_min"] = round(both / row["finish"]["min_us"], 3)
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

"""Cost of the repair of missing 2-D detections against the floor of touching every byte once and against the smoother it is made of.

    python tools/detections_bench.py [--out profiles/detections_bench.json] [--reps 30]

A video of N frames (J = 134, the anchors of detections.repair_anchors: 24 body joints at level 0, 110 face and hand joints at level 1)
with the dropouts of detections.plant_dropouts(rate 0.2, run 10) at detections.DROPPED_XY and confidence 0; N = 27: one clip, N = 594:
22 clips, N = 5 000: about three minutes of video.  Leg "repair": pafuse_detections_repair (radius 13), the pair of launches, writing
out, conf_out and status.  Leg "copy", the every-byte-once floor: two hipMemcpyAsync device-to-device, x2d and conf into other
buffers.  Leg "smooth": pafuse_trajectory_smooth (radius 13) at T = 1 on [1,N,3] roots with weights - one series of the same
filter, the launch the repair's kernel was modelled on.  All legs are bare ctypes calls on buffers allocated before the timed region;
HIP events around each leg, warm, the legs alternating within one process.  These are call times (launches included), not kernel times.

The expectation, stated from the bytes before the measurement: the repair reads 12 N J and writes 13 N J, 16.8 MB at N = 5 000, and a
missing joint (a fifth of them) walks up to 27 frames of 12 bytes, all of it from L2 - two launches bound by launch and latency, not
by bandwidth; the copy moves the same 12 N J twice; the smoother is one launch of N threads.  Per leg: min, median, p90 and
`spread_us` = p90 - min of its repeats; a difference between two legs' minima below the larger spread is not a difference.  One run
on one box is a single observation.  Nothing is asserted on the times.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

J, RADIUS, RATE, RUN = 134, 13, 0.2, 10
HIP_MEMCPY_DEVICE_TO_DEVICE = 3


def hip_runtime():
    """the HIP runtime this process has already loaded (torch's), for hipMemcpyAsync"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                lib = C.CDLL(line.split()[-1])
                lib.hipMemcpyAsync.restype = C.c_int
                lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
                return lib
    raise RuntimeError("no HIP runtime is loaded in this process")


class Legs:
    """the three legs on one video as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, hip, check, N, seed):
        import numpy as np
        from types import SimpleNamespace
        from pafuse_amd import detections, synthetic
        self.lib, self.hip, self.check, stream = lib, hip, check, torch.cuda.current_stream().cuda_stream
        ds = SimpleNamespace(parts_joint_indices=synthetic.DATASET_PART_JOINTS, parts_connection_indices=synthetic.CONNECTION_INDICES)
        rng = np.random.default_rng(seed)
        truth = (np.cumsum(rng.standard_normal((N, J, 2)) * 0.01, axis=0) + rng.uniform(-0.5, 0.5, (1, J, 2))).astype(np.float32)
        self.lost = detections.plant_dropouts(N, J, RATE, RUN, seed)
        x, conf = detections.drop(truth, self.lost)
        self.x2d, self.conf = torch.from_numpy(x).cuda(), torch.from_numpy(conf).cuda()
        self.anchor = torch.from_numpy(detections.repair_anchors(ds)).cuda()
        self.out, self.conf_out = torch.empty(N, J, 2, device="cuda"), torch.empty(N, J, device="cuda")
        self.status = torch.empty(N, J, dtype=torch.uint8, device="cuda")
        self.x2d_copy, self.conf_copy = torch.empty_like(self.x2d), torch.empty_like(self.conf)
        self.traj = torch.from_numpy(np.cumsum(rng.standard_normal((1, N, 3)) * 0.01, axis=1).astype(np.float32)).cuda()
        self.weight = torch.from_numpy(np.where(self.lost[:, 0], 0, 1).astype(np.float32)[None]).cuda()
        self.smoothed = torch.empty(1, N, 3, device="cuda")
        p = lambda t: t.data_ptr()
        self.repair = [p(self.x2d), p(self.conf), p(self.anchor), N, J, RADIUS, 0.0, p(self.out), p(self.conf_out), p(self.status), stream]
        self.copies = [(p(self.x2d_copy), p(self.x2d), 8 * N * J, HIP_MEMCPY_DEVICE_TO_DEVICE, stream),
                       (p(self.conf_copy), p(self.conf), 4 * N * J, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)]
        self.smooth = [p(self.traj), p(self.weight), 1, N, RADIUS, p(self.smoothed), stream]
        self.bytes = {"repair": 25 * N * J, "copy": 24 * N * J, "smooth": 28 * N}
        self.truth = truth

    def repair_leg(self):
        self.check(self.lib.pafuse_detections_repair(*self.repair))

    def copy_leg(self):
        for c in self.copies:
            if self.hip.hipMemcpyAsync(*c) != 0:
                raise RuntimeError("hipMemcpyAsync failed")

    def smooth_leg(self):
        self.check(self.lib.pafuse_trajectory_smooth(*self.smooth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detections_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, detections
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    torch.zeros(1, device="cuda")                                    # the runtime is up before it is looked for
    hip = hip_runtime()
    names = ("repair", "copy", "smooth")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "cost": []}
    for N in (27, 594, 5000):
        legs = Legs(torch, lib, hip, _lib.check, N, seed=70 + N)
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
        # sanity of the run only (what the kernel computes is pinned by tests/test_hip_detections.py): exactly the dropped joints
        # are not observed, the copies are copies, and the filled joints are nearer the truth than the dropped ones were
        status = legs.status.cpu().numpy()
        assert ((status != 0) == legs.lost).all()
        assert torch.equal(legs.x2d_copy, legs.x2d) and torch.equal(legs.conf_copy, legs.conf)
        err = detections.repair_error(legs.truth, legs.out.cpu().numpy(), legs.lost, status)
        assert not err["n_filled"] or err["filled"] < 0.5
        row = {"N": N, "J": J, "radius": RADIUS, "dropout": {"rate": RATE, "run": RUN, "lost_share": round(float(legs.lost.mean()), 4)},
               "status_counts": detections.counts(status).tolist(),
               "repair_error_rms": {k: (None if err[k] != err[k] else round(err[k], 5)) for k in ("filled", "unfilled")}}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2), "useful_bytes": legs.bytes[k],
                      "useful_GB_per_s": round(legs.bytes[k] / t[0] / 1e3, 1)}
        row["repair_over_copy_min"] = round(row["repair"]["min_us"] / row["copy"]["min_us"], 3)
        row["repair_over_smooth_min"] = round(row["repair"]["min_us"] / row["smooth"]["min_us"], 3)
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

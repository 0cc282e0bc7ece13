"""Cost of the screening of observed 2-D detections against the repair behind it and against the floor of touching every byte once.

    python tools/detections_screen_bench.py [--out profiles/detections_screen_bench.json] [--reps 30]

A video of N frames (J = 134, the mirror pairs of synthetic.SYN_JOINTS_LEFT / RIGHT), a random walk per joint with 3 % of the
detections displaced by 0.05 .. 0.6 and swapped runs of 3 frames (detscreen.corrupt), every confidence kept; N = 27: one clip,
N = 594: 22 clips, N = 5 000: about three minutes of video - the shapes of tools/detections_bench.py.  Leg "screen":
pafuse_detections_screen (radius 13, 3 passes, support 3, gate 4, floor 0.005), its chain of 6 launches - residual, scale,
residual x 2, residual with e_cross, finish.  Leg "screen1": the same with 1 pass, 4 launches: half the difference of the two is
one residual launch.  Leg "repair": pafuse_detections_repair (radius 13, the anchors of detections.repair_anchors) on the
screened video - what it sees in the pipeline: the rejected 3 % at confidence 0 - its pair of launches.  Leg "copy", the
every-byte-once floor: two hipMemcpyAsync device-to-device, x2d and conf.  All legs are bare ctypes calls on buffers allocated before the timed region; HIP events around each leg, warm, the legs alternating within
one process.  These are call times (launches included), not kernel times; per-kernel times come from a kernel trace of this script.

The expectation, stated before the measurement: every residual launch walks 26 neighbours of 12 to 13 bytes per observed detection,
all from L2, a dependent chain of fp64 adds per thread - bound by latency like the repair, but on EVERY detection where the repair
walks only the missing fifth; the scale kernel puts J = 134 waves on the device and reads its column 33 times with a stride of J
floats.  Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats; a difference between two legs' minima below the
larger spread is not a difference.  One run on one box is a single observation.  Nothing is asserted on the times.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from detections_bench import HIP_MEMCPY_DEVICE_TO_DEVICE, hip_runtime  # noqa: E402

J, RADIUS, PASSES, SUPPORT, GATE, FLOOR = 134, 13, 3, 3, 4.0, 0.005
OUTLIERS, SWAPS = (0.03, 1, (0.05, 0.6)), (0.02, 3)


class Legs:
    """the legs on one video as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, hip, check, N, seed):
        import numpy as np
        from types import SimpleNamespace
        from pafuse_amd import detections, detscreen, synthetic
        self.lib, self.hip, self.check, stream = lib, hip, check, torch.cuda.current_stream().cuda_stream
        ds = SimpleNamespace(parts_joint_indices=synthetic.DATASET_PART_JOINTS, parts_connection_indices=synthetic.CONNECTION_INDICES)
        rng = np.random.default_rng(seed)
        truth = (np.cumsum(rng.standard_normal((N, J, 2)) * 0.004, axis=0) + rng.uniform(-0.5, 0.5, (1, J, 2))).astype(np.float32)
        conf = rng.uniform(0.5, 1.0, (N, J)).astype(np.float32)
        mirror = detscreen.mirror_table(synthetic.SYN_JOINTS_LEFT, synthetic.SYN_JOINTS_RIGHT, J)
        self.bad = detscreen.corrupt(truth, conf, mirror, outliers=OUTLIERS + (seed,), swaps=SWAPS + (seed + 1,))
        self.truth, self.truth_conf = truth, conf
        self.x2d, self.conf = torch.from_numpy(self.bad["x2d"]).cuda(), torch.from_numpy(self.bad["conf"]).cuda()
        self.mirror = torch.from_numpy(mirror).cuda()
        self.anchor = torch.from_numpy(detections.repair_anchors(ds)).cuda()
        self.out, self.conf_out = torch.empty(N, J, 2, device="cuda"), torch.empty(N, J, device="cuda")
        self.status = torch.empty(N, J, dtype=torch.uint8, device="cuda")
        self.resid, self.scale = torch.empty(N, J, device="cuda"), torch.empty(J, device="cuda")
        need = lib.pafuse_detections_screen_workspace_bytes(N, J)
        self.work = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
        self.out2, self.conf_out2 = torch.empty_like(self.out), torch.empty_like(self.conf_out)
        self.status2 = torch.empty_like(self.status)
        self.x2d_copy, self.conf_copy = torch.empty_like(self.x2d), torch.empty_like(self.conf)
        p = lambda t: t.data_ptr()
        screen = lambda passes: [p(self.x2d), p(self.conf), p(self.mirror), N, J, RADIUS, passes, SUPPORT, 0.0, GATE, FLOOR, p(self.out),
                                 p(self.conf_out), p(self.status), p(self.resid), p(self.scale), p(self.work), need, stream]
        self.screen_args, self.screen1_args = screen(PASSES), screen(1)
        self.repair = [p(self.out), p(self.conf_out), p(self.anchor), N, J, RADIUS, 0.0, p(self.out2), p(self.conf_out2), p(self.status2), stream]
        self.copies = [(p(self.x2d_copy), p(self.x2d), 8 * N * J, HIP_MEMCPY_DEVICE_TO_DEVICE, stream),
                       (p(self.conf_copy), p(self.conf), 4 * N * J, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)]
        self.workspace_bytes = need

    def screen1_leg(self):
        self.check(self.lib.pafuse_detections_screen(*self.screen1_args))

    def screen_leg(self):          # the last screen leg of a round: its outputs are what the sanity check reads
        self.check(self.lib.pafuse_detections_screen(*self.screen_args))

    def repair_leg(self):
        self.check(self.lib.pafuse_detections_repair(*self.repair))

    def copy_leg(self):
        for c in self.copies:
            if self.hip.hipMemcpyAsync(*c) != 0:
                raise RuntimeError("hipMemcpyAsync failed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detections_screen_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, detscreen
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    torch.zeros(1, device="cuda")                                    # the runtime is up before it is looked for
    hip = hip_runtime()
    names = ("screen1", "screen", "repair", "copy")
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
        # sanity of the run only (what the kernels compute is pinned by tests/test_hip_detections_screen.py): the copies are copies,
        # a detection keeps its coordinates unless it is swapped, and the planted detections are counted
        status = legs.status.cpu().numpy()
        assert torch.equal(legs.x2d_copy, legs.x2d) and torch.equal(legs.conf_copy, legs.conf)
        two = status == 2
        assert (legs.out.cpu().numpy()[~two] == legs.bad["x2d"][~two]).all()
        err = detscreen.screen_error(status, legs.bad["planted_out"], legs.bad["planted_swap"])
        err["swapped_back_to_the_truth"] = int(((legs.out.cpu().numpy() == legs.truth).all(-1) & two).sum())
        row = {"N": N, "J": J, "radius": RADIUS, "passes": PASSES, "support": SUPPORT, "gate": GATE, "floor": FLOOR,
               "planted": {"outliers": OUTLIERS, "swaps": SWAPS}, "status_counts": detscreen.counts(status).tolist(), "screen_error": err,
               "workspace_bytes": legs.workspace_bytes}
        for k in names:
            t = sorted(times[k])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                      "spread_us": round(p90 - t[0], 2)}
        row["residual_launch_us"] = round((row["screen"]["min_us"] - row["screen1"]["min_us"]) / (PASSES - 1), 2)
        row["screen_over_repair_min"] = round(row["screen"]["min_us"] / row["repair"]["min_us"], 3)
        row["screen_over_copy_min"] = round(row["screen"]["min_us"] / row["copy"]["min_us"], 3)
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

"""Cost of following people through a video against the floor of touching every input byte once and against the screen behind it.

    python tools/tracks_bench.py [--out profiles/tracks_bench.json] [--reps 30]

A video of N frames with K candidate slots per frame (J = 134): three people in lanes, 15 % of their joints unobserved, the
slots shuffled per frame, dropouts of at most 3 frames, a ghost in 30 % of the frames where a slot is free (the planted case
of tests/test_tracks_host.py, tracks.plant_video); the other slots all-zero.  K in {4, 16}, G = 4, M = 3; N = 27: one clip,
N = 594: 22 clips, N = 5 000: about three minutes of video - the shapes of tools/detections_screen_bench.py.  Leg "tracks":
pafuse_tracks_links + pafuse_tracks_path + pafuse_tracks_gather, 5 launches.  Legs "links" (2 launches: nodes, links), "path"
(1 launch of ONE wave, the M rounds inside it) and "gather" (1 launch): the three entries on their own, whose medians are the
per-kernel figures (call times; "links" holds two kernels).  Leg "screen": pafuse_detections_screen (radius 13, 3 passes, the
defaults) on track 0 - what runs next in the pipeline.  Leg "copy", the every-byte-once floor: two hipMemcpyAsync
device-to-device, x2d [N,K,J,2] and conf [N,K,J].  All legs are bare ctypes calls on buffers allocated before the timed region;
HIP events around each leg, warm, the legs alternating within one process.  These are call times (launches included).

The expectation, stated before the measurement: the links kernel puts N*G*K waves on the device and, per wave, walks the present
candidates of one earlier frame - a few L2 reads and two butterflies each: short.  The path kernel is ONE wave for the whole
video: M rounds of N dependent frame steps, each a handful of dependent loads (size, used, the gains of the live predecessors,
an LDS broadcast) and a butterfly.  It is bound by latency, not bandwidth, and grows as M * N: `path_us_per_frame_step` = the
path leg's minimum / (M * N) is the figure to watch.  Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats; a
difference between two legs' minima below the larger spread is not a difference.  One run on one box is a single observation.
Nothing is asserted on the times.
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

J, G, M, SUPPORT, MIN_FRAMES, GATE, SKIP = 134, 4, 3, 5, 5, 0.5, 0.05
PEOPLE = 3


def planted(N, K, seed):
    """three people in lanes 0.6 apart, moving 0.1 at most -> tracks.plant_video's dict"""
    import numpy as np
    from pafuse_amd import tracks
    rng = np.random.default_rng(seed)
    body = rng.uniform(-1, 1, (PEOPLE, 1, J, 2)) * np.array([0.15, 0.4])
    n = np.arange(N)[None, :, None]
    phase = rng.random((PEOPLE, 1, 1))
    centre = np.stack([np.array([-0.6, 0.0, 0.6])[:, None, None] + 0.1 * np.sin(2 * np.pi * (n / 40.0 + phase)),
                       0.05 * np.sin(2 * np.pi * (n / 55.0 + phase))], axis=-1)
    px = (body + centre + 0.004 * rng.standard_normal((PEOPLE, N, J, 2))).astype(np.float32)
    pc = rng.uniform(0.5, 1.0, (PEOPLE, N, J)).astype(np.float32)
    pc[rng.random((PEOPLE, N, J)) < 0.15] = 0
    return tracks.plant_video(px, pc, slots=K, seed=seed, drop=(0.1, G - 1), ghost=(0.3, 2.0))


class Legs:
    """the legs on one video as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, hip, check, N, K, seed):
        self.lib, self.hip, self.check, stream = lib, hip, check, torch.cuda.current_stream().cuda_stream
        self.video = planted(N, K, seed)
        self.x2d, self.conf = torch.from_numpy(self.video["x2d"]).cuda(), torch.from_numpy(self.video["conf"]).cuda()
        need = lib.pafuse_tracks_workspace_bytes(N, K, J, G)
        self.work = torch.empty(need // 8, dtype=torch.float64, device="cuda")
        self.assign = torch.empty(M, N, dtype=torch.int32, device="cuda")
        self.score, self.frames = torch.empty(M, dtype=torch.float64, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
        self.out, self.conf_out = torch.empty(M, N, J, 2, device="cuda"), torch.empty(M, N, J, device="cuda")
        self.x2d_copy, self.conf_copy = torch.empty_like(self.x2d), torch.empty_like(self.conf)
        sneed = lib.pafuse_detections_screen_workspace_bytes(N, J)
        self.swork = torch.empty((sneed + 7) // 8, dtype=torch.float64, device="cuda")
        self.sout, self.sconf = torch.empty(N, J, 2, device="cuda"), torch.empty(N, J, device="cuda")
        self.status = torch.empty(N, J, dtype=torch.uint8, device="cuda")
        p = lambda t: t.data_ptr()
        self.links_args = [p(self.x2d), p(self.conf), N, K, J, G, SUPPORT, 0.0, GATE, SKIP, p(self.work), need, stream]
        self.path_args = [None, None, N, K, G, M, MIN_FRAMES, -1, -1, p(self.assign), p(self.score), p(self.frames), p(self.work), need, stream]
        self.gather_args = [p(self.x2d), p(self.conf), p(self.assign), N, K, J, M, p(self.out), p(self.conf_out), stream]
        self.screen_args = [p(self.out), p(self.conf_out), None, N, J, 13, 3, 3, 0.0, 4.0, 0.005, p(self.sout), p(self.sconf), p(self.status),
                            None, None, p(self.swork), sneed, stream]
        self.copies = [(p(self.x2d_copy), p(self.x2d), 8 * N * K * J, HIP_MEMCPY_DEVICE_TO_DEVICE, stream),
                       (p(self.conf_copy), p(self.conf), 4 * N * K * J, HIP_MEMCPY_DEVICE_TO_DEVICE, stream)]
        self.workspace_bytes = need

    def links_leg(self):
        self.check(self.lib.pafuse_tracks_links(*self.links_args))

    def path_leg(self):
        self.check(self.lib.pafuse_tracks_path(*self.path_args))

    def gather_leg(self):
        self.check(self.lib.pafuse_tracks_gather(*self.gather_args))

    def tracks_leg(self):
        self.links_leg(), self.path_leg(), self.gather_leg()

    def screen_leg(self):          # on track 0 of the gather: the first [N,J] rows of out / conf_out
        self.check(self.lib.pafuse_detections_screen(*self.screen_args))

    def copy_leg(self):
        for c in self.copies:
            if self.hip.hipMemcpyAsync(*c) != 0:
                raise RuntimeError("hipMemcpyAsync failed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib, tracks
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    torch.zeros(1, device="cuda")                                    # the runtime is up before it is looked for
    hip = hip_runtime()
    names = ("links", "path", "gather", "tracks", "screen", "copy")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer allocated beforehand; one run on one box",
           "cost": []}
    for K in (4, 16):
        for N in (27, 594, 5000):
            legs = Legs(torch, lib, hip, _lib.check, N, K, seed=70 + N + K)
            times = {k: [] for k in names}
            for _ in range(3):                                       # warm: code objects, caches
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
            # sanity of the run only (what the kernels compute is pinned by tests/test_hip_tracks.py): the copies are copies and
            # the tracks are the planted people
            assert torch.equal(legs.x2d_copy, legs.x2d) and torch.equal(legs.conf_copy, legs.conf)
            assign = legs.assign.cpu().numpy()
            err = tracks.track_error(assign, legs.video["truth"])
            row = {"N": N, "K": K, "J": J, "max_gap": G, "num_tracks": M, "support": SUPPORT, "min_frames": MIN_FRAMES, "gate": GATE, "skip": SKIP,
                   "track_error": err, "frames": legs.frames.cpu().tolist(), "workspace_bytes": legs.workspace_bytes,
                   "input_bytes": 12 * N * K * J}
            for k in names:
                t = sorted(times[k])
                p90 = t[int(0.9 * (len(t) - 1))]
                row[k] = {"min_us": round(t[0], 2), "median_us": round(statistics.median(t), 2), "p90_us": round(p90, 2),
                          "spread_us": round(p90 - t[0], 2)}
            row["path_us_per_frame_step"] = round(row["path"]["min_us"] / (M * N), 4)
            row["tracks_over_copy_min"] = round(row["tracks"]["min_us"] / row["copy"]["min_us"], 3)
            row["tracks_over_screen_min"] = round(row["tracks"]["min_us"] / row["screen"]["min_us"], 3)
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

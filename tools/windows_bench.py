"""Cost of pooling one batch of overlapping windows into per-frame poses against what is done with such a state today.

    python tools/windows_bench.py [--out profiles/windows_bench.json] [--reps 30]

One pose state of B windows (T = 10, F = 27, J = 134, stride 9; B = 1 and B = 64, so N = 9 (B - 1) + 27 frames) is made once
by pafuse_pose_partials.  Leg "fold": pafuse_pose_windows_fold of that state into a neutral frame state + pafuse_frames_finish
writing mean, pick, index and window for all N frames.  Leg "combine", the yardstick: pafuse_pose_combine (W = 1) writing mean,
pick and index of the same state - one pose per (window, frame), which the caller would still have to reassemble.  Both legs are
bare ctypes calls on buffers and tables allocated before the timed region; HIP events around each leg, warm, the two legs
alternating.  The frame state is reset to neutral before every "fold" repeat, outside the timed region.  These are call times
(launches included), not kernel times.  Useful bytes are counted from the shapes (n = B T F J state rows, r = T N J frame rows):
combine reads 44 n and writes 28 n; fold reads 44 n, reads and writes 48 r + 4 N; finish reads 44 r + 4 N and writes 32 r.
Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats; a difference between the legs' minima below the larger
spread is not a difference.  One run on one box is a single observation.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.partials_bench import J, make_inputs  # noqa: E402


class Legs:
    """both legs on one batch state as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, np, lib, check, conn, z, stride):
        pred, _, x2d, traj, cam = z
        B, T, P, F, _, _ = pred.shape
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = pred.device
        self.N = N = stride * (B - 1) + F
        self.hs = np.arange(B, dtype=np.int32) * stride                  # host copies the entry checks; kept alive here
        self.hv = np.full(B, F, dtype=np.int32)
        self.tab = torch.from_numpy(np.stack([self.hs, self.hv])).to(dev)
        L = lib.pafuse_pose_partials_bytes(B, T, F, J)
        self.state = torch.empty(L // 8, device=dev, dtype=torch.float64)
        p = lambda t: t.data_ptr()
        check(lib.pafuse_pose_partials(p(pred), p(x2d), p(traj), p(cam), p(conn), B, T, P, F, J, 0, p(self.state), L, stream))
        LF = lib.pafuse_frame_pose_state_bytes(N, T, J)
        self.frame = torch.empty(LF // 8, device=dev, dtype=torch.float64)
        self.c_out = (torch.empty(B, T, F, J, 3, device=dev), torch.empty(B, T, F, J, 3, device=dev),
                      torch.empty(B, T, F, J, device=dev, dtype=torch.int32))
        self.f_out = (torch.empty(T, N, J, 3, device=dev), torch.empty(T, N, J, 3, device=dev),
                      torch.empty(T, N, J, device=dev, dtype=torch.int32), torch.empty(T, N, J, device=dev, dtype=torch.int32))
        self.init = [p(self.frame), LF, N, T, J, stream]
        self.fold = [p(self.frame), LF, N, p(self.state), L, B, T, F, J, p(self.tab[0]), p(self.tab[1]),
                     self.hs.ctypes.data, self.hv.ctypes.data, 0, P, stream]
        self.finish = [p(self.frame), None, N, T, J, *(p(t) for t in self.f_out), None, None, stream]
        self.combine = [p(self.state), 1, L, B, T, F, J, P, None, *(p(t) for t in self.c_out), stream]
        n, r = B * T * F * J, T * N * J
        self.bytes = {"combine": 44 * n + 28 * n, "fold": 44 * n + 2 * (48 * r + 4 * N) + 44 * r + 4 * N + 32 * r}

    def reset(self):
        self.check(self.lib.pafuse_frame_pose_state_init(*self.init))

    def combine_leg(self):
        self.check(self.lib.pafuse_pose_combine(*self.combine))

    def fold_leg(self):
        self.check(self.lib.pafuse_pose_windows_fold(*self.fold))
        self.check(self.lib.pafuse_frames_finish(*self.finish))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib
    from pafuse_amd import synthetic as gu
    from pafuse_amd.evaluate import _tables
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                         parts_connection_indices=dict(gu.CONNECTION_INDICES))
    conn = _tables(ds, J, "cuda")[0]
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer and table allocated beforehand; one run on one box",
           "cost": []}
    T, P, F, stride = 10, 5, 27, 9
    for B in (1, 64):
        legs = Legs(torch, np, lib, _lib.check, conn, make_inputs(torch, gu, B, T, P, F, seed=80 + B), stride)
        times = {"combine": [], "fold": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.reset(), legs.combine_leg(), legs.fold_leg()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("combine", "fold"):
                legs.reset()                                         # outside the timed region (stream order)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name + "_leg")()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the fold computes is pinned by tests/test_hip_windows.py): a frame one window covers is
        # that window's pose
        assert torch.equal(legs.f_out[0][:, :stride], legs.c_out[0][0, :, :stride])
        assert torch.equal(legs.f_out[2][:, :stride], legs.c_out[2][0, :, :stride])
        row = {"B": B, "T": T, "P": P, "F": F, "J": J, "stride": stride, "N": legs.N}
        for name in ("combine", "fold"):
            t = sorted(times[name])
            med = statistics.median(t)
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"min_us": round(t[0], 2), "median_us": round(med, 2), "p90_us": round(p90, 2),
                         "spread_us": round(p90 - t[0], 2), "useful_bytes": legs.bytes[name],
                         "useful_GB_per_s": round(legs.bytes[name] / t[0] / 1e3, 1)}
        row["fold_over_combine_min"] = round(row["fold"]["min_us"] / row["combine"]["min_us"], 3)
        row["fold_over_combine_median"] = round(row["fold"]["median_us"] / row["combine"]["median_us"], 3)
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

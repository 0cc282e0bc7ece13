"""Cost of J-Agg coherent in time against the per-frame J-Agg it extends, on the same predictions, one JSON document.

    python tools/pose_path_bench.py [--out profiles/pose_path_bench.json] [--reps 30]

The C-ABI calls pafuse_pose_partials + pafuse_pose_combine ("pair": the mean, the per-frame pick and its index, with a merged
state) against the same pair followed by pafuse_pose_path on the mean it wrote ("path": pick, index, e2 and cost of the
path), on the same [B,T,P,F,J,3] predictions: T = 10, F = 27, J = 134; P = 20 at B = 1 and B = 64, and P = 160 at B = 8,
because the recursion's work grows with P * P while the pair's grows with P.  Both legs are bare ctypes calls on operands,
index table, outputs, state and workspace that were all allocated before the timed region; HIP events around each leg,
warm, the two legs alternating.  These are call times (launches included), not kernel times.  Useful bytes are counted
from the shapes: the pair reads the predictions once, writes and reads the 44-byte state twice (chunk and merged) and
writes 28 bytes of mean, pick and index per (b,t,f,j); the path kernel reads the predictions once more, 12 bytes of mean
per (b,t,f,j), writes and reads one back-pointer byte per (line, frame, hypothesis) and writes 20 bytes per (b,t,f,j) and
8 per line.  Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats; `path_only_min_us` is the difference of
the legs' minima.  No target is fixed in advance.
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

SHAPES = ((1, 20), (64, 20), (8, 160))      # (B, P)
WEIGHT = 0.5


class Legs:
    """both legs on one set of predictions as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, conn, z):
        self.pred, _, self.x2d, self.traj, self.cam = z
        B, T, P, F, _, _ = self.pred.shape
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = self.pred.device
        L = lib.pafuse_pose_partials_bytes(B, T, F, J)
        self.state, self.merged = (torch.empty(L // 8, device=dev, dtype=torch.float64) for _ in range(2))
        self.mean, self.pick, self.path_pick = (torch.empty(B, T, F, J, 3, device=dev) for _ in range(3))
        self.idx, self.path_idx = (torch.empty(B, T, F, J, device=dev, dtype=torch.int32) for _ in range(2))
        self.path_e2 = torch.empty(B, T, F, J, device=dev)
        self.cost = torch.empty(B, T, J, device=dev, dtype=torch.float64)
        self.ws_bytes = lib.pafuse_pose_path_workspace_bytes(B, T, P, F, J)
        self.ws = torch.empty(self.ws_bytes, device=dev, dtype=torch.uint8)
        p = lambda t: t.data_ptr()
        self.partials = [p(self.pred), p(self.x2d), p(self.traj), p(self.cam), p(conn), B, T, P, F, J, 0, p(self.state), L, stream]
        self.combine = [p(self.state), 1, L, B, T, F, J, P, p(self.merged), p(self.mean), p(self.pick), p(self.idx), stream]
        self.path = [p(self.pred), p(self.x2d), p(self.traj), 0, p(self.cam), None, p(conn), p(self.mean), WEIGHT, B, T, P, F, J,
                     p(self.path_pick), p(self.path_idx), p(self.path_e2), p(self.cost), p(self.ws), self.ws_bytes, stream]

    def pair_leg(self):
        self.check(self.lib.pafuse_pose_partials(*self.partials))
        self.check(self.lib.pafuse_pose_combine(*self.combine))

    def path_leg(self):
        self.pair_leg()
        self.check(self.lib.pafuse_pose_path(*self.path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_path_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
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
           "weight": WEIGHT, "what_is_timed": "C-ABI call sequences between HIP events, every buffer and table allocated beforehand",
           "cost": []}
    T, F = 10, 27
    for B, P in SHAPES:
        legs = Legs(torch, lib, _lib.check, conn, make_inputs(torch, gu, B, T, P, F, seed=90 + B))
        times = {"pair": [], "path": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.pair_leg(), legs.path_leg()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("pair", "path"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name + "_leg")()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the kernel computes is pinned by tests/test_hip_pose_path.py): a path wherever the
        # per-frame pick has a candidate at some frame of the line, and it moved some picks
        has = (legs.idx >= 0).any(dim=2, keepdim=True).expand_as(legs.idx)
        assert torch.equal(legs.path_idx >= 0, has) and not torch.equal(legs.path_idx, legs.idx)
        n, lines = B * T * F * J, B * T * J
        read = legs.pred.numel() * 4
        pair_bytes = read + 4 * 44 * n + 28 * n
        by = {"pair": pair_bytes, "path": pair_bytes + read + 12 * n + 2 * lines * F * P + 20 * n + 8 * lines}
        row = {"B": B, "T": T, "P": P, "F": F, "J": J, "workspace_bytes": int(legs.ws_bytes),
               "changed_picks": round(float((legs.path_idx != legs.idx).float().mean()), 4)}
        for name in ("pair", "path"):
            t = sorted(times[name])
            med = statistics.median(t)
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"min_us": round(t[0], 2), "median_us": round(med, 2), "p90_us": round(p90, 2),
                         "spread_us": round(p90 - t[0], 2), "useful_bytes": by[name],
                         "useful_GB_per_s": round(by[name] / t[0] / 1e3, 1)}
        row["path_only_min_us"] = round(row["path"]["min_us"] - row["pair"]["min_us"], 2)
        row["path_over_pair_min"] = round(row["path"]["min_us"] / row["pair"]["min_us"], 3)
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

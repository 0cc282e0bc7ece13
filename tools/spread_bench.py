"""Cost of the hypothesis spread against the mean-only pose aggregation of the same predictions, one JSON document.

    python tools/spread_bench.py [--out profiles/spread_bench.json] [--reps 30]

The C-ABI calls pafuse_spread_partials + pafuse_spread_combine ("spread": mean, covariance and std written) against
pafuse_pose_partials + pafuse_pose_combine in mean-only mode ("pose": the mean written) on the same [B,T,P,F,J,3]
predictions (B = 1 and B = 64, P = 20, T = 10, F = 27, J = 134).  Both legs are bare ctypes calls on operands, index table,
outputs and state that were all allocated before the timed region; HIP events around each pair of calls, warm, the two legs
alternating, median of `--reps`.  These are call times (two launches included), not kernel times.  Useful bytes are counted
from the shapes: both read the predictions once; the spread pair writes and reads a 72-byte-per-(b,t,f,j) state and writes
40 bytes of mean, covariance and std, the pose pair writes and reads its 44-byte state and writes 12 bytes of mean.
`spread_us` of a leg is p90 - min of its repeats: a difference between the legs' medians below it is not a difference.
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
    """both pairs on one set of predictions as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, conn, pred):
        self.pred, self.conn = pred, conn
        B, T, P, F, _, _ = pred.shape
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = pred.device
        f64 = dict(device=dev, dtype=torch.float64)
        self.pose_state = torch.empty(lib.pafuse_pose_partials_bytes(B, T, F, J) // 8, **f64)
        self.spread_state = torch.empty(lib.pafuse_spread_partials_bytes(B, T, F, J) // 8, **f64)
        self.pose_mean, self.mean = (torch.empty(B, T, F, J, 3, device=dev) for _ in range(2))
        self.cov, self.std = torch.empty(B, T, F, J, 6, device=dev), torch.empty(B, T, F, J, device=dev)
        p = lambda t: t.data_ptr()
        self.pose_args = ([p(pred), None, None, None, p(conn), B, T, P, F, J, 0, p(self.pose_state), self.pose_state.numel() * 8, stream],
                          [p(self.pose_state), 1, self.pose_state.numel() * 8, B, T, F, J, P, None, p(self.pose_mean), None, None, stream])
        self.spread_args = ([p(pred), p(conn), B, T, P, F, J, 0, p(self.spread_state), self.spread_state.numel() * 8, stream],
                            [p(self.spread_state), 1, self.spread_state.numel() * 8, B, T, F, J, None, p(self.mean), p(self.cov),
                             p(self.std), stream])

    def pose(self):
        self.check(self.lib.pafuse_pose_partials(*self.pose_args[0]))
        self.check(self.lib.pafuse_pose_combine(*self.pose_args[1]))

    def spread(self):
        self.check(self.lib.pafuse_spread_partials(*self.spread_args[0]))
        self.check(self.lib.pafuse_spread_combine(*self.spread_args[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread_bench.json"))
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
           "what_is_timed": "C-ABI call pairs between HIP events, every buffer and table allocated beforehand", "cost": []}
    T, P, F = 10, 20, 27
    for B in (1, 64):
        legs = Legs(torch, lib, _lib.check, conn, make_inputs(torch, gu, B, T, P, F, seed=60 + B)[0])
        times = {"pose": [], "spread": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.pose(), legs.spread()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("pose", "spread"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name)()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the pair computes is pinned by tests/test_hip_spread.py)
        assert torch.equal(legs.mean, legs.pose_mean) and bool((legs.std >= 0).all())
        n = B * T * F * J
        read = legs.pred.numel() * 4
        by = {"pose": read + 2 * 44 * n + 12 * n, "spread": read + 2 * (72 * n + 8) + 40 * n}
        row = {"B": B, "T": T, "P": P, "F": F, "J": J}
        for name in ("pose", "spread"):
            t = sorted(times[name])
            med = statistics.median(t)
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"median_us": round(med, 2), "min_us": round(t[0], 2), "p90_us": round(p90, 2),
                         "spread_us": round(p90 - t[0], 2), "useful_bytes": by[name],
                         "useful_GB_per_s": round(by[name] / med / 1e3, 1)}
        row["spread_over_pose"] = round(row["spread"]["median_us"] / row["pose"]["median_us"], 3)
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

"""Cost of the aggregates as poses against the one-kernel evaluation of the same predictions, one JSON document.

    python tools/pose_aggregate_bench.py [--out profiles/pose_aggregate_bench.json] [--reps 30]

The C-ABI calls pafuse_pose_partials + pafuse_pose_combine ("pose": mean, pick and index written) against
pafuse_hypothesis_errors ("errors") on the same [B,T,P,F,J,3] predictions (B = 1 and B = 64, P = 20, T = 10, F = 27,
J = 134).  Both legs are bare ctypes calls on operands, index tables, outputs and state that were all allocated before the
timed region; HIP events around each call, warm, the two alternating, median of `--reps`.  These are call times (launch
included), not kernel times: for those run the tool under `rocprofv3 --kernel-trace --stats -- python
tools/pose_aggregate_bench.py` and read metrics_kernel against pose_partials_kernel + pose_combine_kernel.  Useful bytes
are counted from the shapes: both read the predictions once; the errors kernel reads the ground truth and writes two
[B,T,P,F,J] maps beside its four [B,T,F,J] ones, the pose pair writes and reads one 44-byte-per-(b,t,f,j) state and
writes 28 bytes per (b,t,f,j) of poses and indices.  `spread_us` of a leg is p90 - min of its repeats: a difference
between the legs' medians below it is not a difference.
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
    """both entries on one set of operands as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, tables, z):
        self.pred, self.gt, self.x2d, self.traj, self.cam = z
        self.conn, self.pbroot = tables
        B, T, P, F, _, _ = self.pred.shape
        self.dims = (B, T, P, F)
        self.lib, self.check, self.stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = self.pred.device
        self.e3, self.epb = (torch.empty(B, T, P, F, J, device=dev) for _ in range(2))
        self.maps = [torch.empty(B, T, F, J, device=dev) for _ in range(4)]            # jbest, pagg, jagg, paggpb
        self.state = torch.empty(lib.pafuse_pose_partials_bytes(B, T, F, J) // 8, device=dev, dtype=torch.float64)
        self.mean, self.pick = (torch.empty(B, T, F, J, 3, device=dev) for _ in range(2))
        self.idx = torch.empty(B, T, F, J, device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr()
        self.errors_args = [p(t) for t in (self.pred, self.gt, self.x2d, self.traj, self.cam, self.conn, self.pbroot)] + \
            [B, T, P, F, J, p(self.e3), p(self.epb)] + [p(t) for t in self.maps] + [self.stream]
        self.partials_args = [p(t) for t in (self.pred, self.x2d, self.traj, self.cam, self.conn)] + \
            [B, T, P, F, J, 0, p(self.state), self.state.numel() * 8, self.stream]
        self.combine_args = [p(self.state), 1, self.state.numel() * 8, B, T, F, J, P, None, p(self.mean), p(self.pick), p(self.idx),
                             self.stream]

    def errors(self):
        self.check(self.lib.pafuse_hypothesis_errors(*self.errors_args))

    def pose(self):
        self.check(self.lib.pafuse_pose_partials(*self.partials_args))
        self.check(self.lib.pafuse_pose_combine(*self.combine_args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
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
    tables = _tables(ds, J, "cuda")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer and table allocated beforehand", "cost": []}
    T, P, F = 10, 20, 27
    for B in (1, 64):
        legs = Legs(torch, lib, _lib.check, tables, make_inputs(torch, gu, B, T, P, F, seed=40 + B))
        times = {"errors": [], "pose": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.errors(), legs.pose()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("errors", "pose"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name)()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the pair computes is pinned by tests/test_hip_pose_aggregate.py)
        assert int(legs.idx.min()) >= 0 and int(legs.idx.max()) < P
        n = B * T * F * J
        read = legs.pred.numel() * 4
        by = {"errors": read + legs.gt.numel() * 4 + 2 * n * P * 4 + 4 * n * 4, "pose": read + 2 * 44 * n + 28 * n}
        row = {"B": B, "T": T, "P": P, "F": F, "J": J}
        for name in ("errors", "pose"):
            t = sorted(times[name])
            med = statistics.median(t)
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"median_us": round(med, 2), "min_us": round(t[0], 2), "p90_us": round(p90, 2),
                         "spread_us": round(p90 - t[0], 2), "useful_bytes": by[name],
                         "useful_GB_per_s": round(by[name] / med / 1e3, 1)}
        row["pose_over_errors"] = round(row["pose"]["median_us"] / row["errors"]["median_us"], 3)
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

"""Cost of Protocol #2 from partial states against the one-kernel Protocol #2 on the same predictions, one JSON document.

    python tools/p2_partials_bench.py [--out profiles/p2_partials_bench.json] [--reps 30]

The C-ABI calls pafuse_procrustes_partials (the alignment kernel + the psum reduction) + pafuse_procrustes_combine
("partials": jbest, pagg, jagg and pick written, the mean pose's sums borrowed from a pose state computed beforehand)
against pafuse_procrustes_errors ("errors", the yardstick) on the same [B,T,P,F,J,3] predictions (B = 1 and B = 64, P = 20,
T = 10, F = 27, J = 134).  Both legs are bare ctypes calls on operands, tables, outputs, state and workspace that were all
allocated before the timed region; HIP events around each call, warm, the two alternating, median of `--reps`.  These are
call times (launch included), not kernel times: for those run the tool under `rocprofv3 --kernel-trace --stats -- python
tools/p2_partials_bench.py` and read procrustes_kernel against procrustes_partials_kernel + procrustes_psum_kernel +
procrustes_combine_kernel.  `spread_us` of the errors leg (p90 - min of its repeats) is the margin: a difference between
the legs' medians below it is not a difference.  The ratio is recorded as measured; nothing gates on it.
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

    def __init__(self, torch, lib, check, conn, z):
        self.pred, self.gt, self.x2d, self.traj, self.cam = z
        B, T, P, F, _, _ = self.pred.shape
        self.lib, self.check, self.stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = self.pred.device
        f64 = dict(device=dev, dtype=torch.float64)
        self.ref = [torch.empty(B, T, F, J, device=dev) for _ in range(3)]                 # jbest, pagg, jagg
        self.ref_sums = torch.empty(B, T, P, F, **f64)
        self.ref_pick = torch.empty(B, T, F, J, device=dev, dtype=torch.int32)
        self.state = torch.empty(lib.pafuse_procrustes_partials_bytes(B, T, P, F, J) // 8, **f64)
        self.work = torch.empty(max(lib.pafuse_procrustes_partials_workspace_bytes(B, T, P, F, J) // 8, 1), **f64)
        self.pose = torch.empty(lib.pafuse_pose_partials_bytes(B, T, F, J) // 8, **f64)
        self.maps = [torch.empty(B, T, F, J, device=dev) for _ in range(3)]
        self.pick = torch.empty(B, T, F, J, device=dev, dtype=torch.int32)
        p = lambda t: t.data_ptr()
        ops6 = [p(t) for t in (self.pred, self.gt, self.x2d, self.traj, self.cam, conn)]
        check(lib.pafuse_pose_partials(p(self.pred), None, None, None, p(conn), B, T, P, F, J, 0, p(self.pose),
                                       self.pose.numel() * 8, self.stream))              # the sums of the mean pose: not timed
        self.errors_args = ops6 + [B, T, P, F, J, p(self.ref[0]), p(self.ref_sums), p(self.ref[1]), p(self.ref[2]),
                                   p(self.ref_pick), self.stream]
        self.partials_args = ops6 + [B, T, P, F, J, 0, p(self.state), self.state.numel() * 8, p(self.work),
                                     self.work.numel() * 8, self.stream]
        self.combine_args = [p(self.state), 1, self.state.numel() * 8, p(self.pose), self.pose.numel() * 8, p(self.gt), p(conn),
                             B, T, F, J, P, None, p(self.maps[0]), p(self.maps[1]), p(self.maps[2]), p(self.pick), self.stream]

    def errors(self):
        self.check(self.lib.pafuse_procrustes_errors(*self.errors_args))

    def partials(self):
        self.check(self.lib.pafuse_procrustes_partials(*self.partials_args))
        self.check(self.lib.pafuse_procrustes_combine(*self.combine_args))


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
    conn, _ = _tables(ds, J, "cuda")
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer and table allocated beforehand", "cost": []}
    T, P, F = 10, 20, 27
    for B in (1, 64):
        legs = Legs(torch, lib, _lib.check, conn, make_inputs(torch, gu, B, T, P, F, seed=60 + B))
        times = {"errors": [], "partials": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.errors(), legs.partials()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("errors", "partials"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name)()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the pair computes is pinned by tests/test_hip_p2_partials.py)
        assert torch.equal(legs.pick, legs.ref_pick)
        row = {"B": B, "T": T, "P": P, "F": F, "J": J}
        for name in ("errors", "partials"):
            t = sorted(times[name])
            med = statistics.median(t)
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"median_us": round(med, 2), "min_us": round(t[0], 2), "p90_us": round(p90, 2),
                         "spread_us": round(p90 - t[0], 2)}
        row["partials_over_errors"] = round(row["partials"]["median_us"] / row["errors"]["median_us"], 3)
        row["difference_us"] = round(row["partials"]["median_us"] - row["errors"]["median_us"], 2)
        row["margin_us"] = row["errors"]["spread_us"]
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

"""Cost of J-Agg with a fitted root against J-Agg with a given trajectory on the same predictions, one JSON document.

    python tools/rootfit_bench.py [--out profiles/rootfit_bench.json] [--reps 30]

The C-ABI calls pafuse_pose_partials_fit + pafuse_pose_combine ("fit": roots fitted on the device, confidences given, tfit not
written) against pafuse_pose_partials with a trajectory + pafuse_pose_combine ("traj": the kernel that was there before, for the
same 44-byte state) on the same [B,T,P,F,J,3] predictions (B = 1 and B = 64, P = 20, T = 10, F = 27, J = 134); both write
mean, pick and index.  Both legs are bare ctypes calls on operands, index table, outputs and state that were all allocated
before the timed region; HIP events around each pair of calls, warm, the two legs alternating.  These are call times (two
launches included), not kernel times.  Useful bytes are counted from the shapes: both read the predictions once, write and
read the state and write 28 bytes of mean, pick and index per (b,t,f,j).  Per leg: min, median, p90 and `spread_us` =
p90 - min of its repeats; a difference between the legs' minima below the larger spread is not a difference.
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

    def __init__(self, torch, lib, check, conn, z):
        self.pred, _, self.x2d, self.traj, self.cam = z
        self.conn = conn
        B, T, P, F, _, _ = self.pred.shape
        self.lib, self.check, stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = self.pred.device
        g = torch.Generator().manual_seed(B)
        conf = torch.rand(B, F, J, generator=g)
        conf[torch.rand(B, F, J, generator=g) < 0.2] = 0            # a fifth of the joints not found
        self.conf = conf.to(dev)
        L = lib.pafuse_pose_partials_bytes(B, T, F, J)
        self.states = {k: torch.empty(L // 8, device=dev, dtype=torch.float64) for k in ("traj", "fit")}
        self.out = {k: (torch.empty(B, T, F, J, 3, device=dev), torch.empty(B, T, F, J, 3, device=dev),
                        torch.empty(B, T, F, J, device=dev, dtype=torch.int32)) for k in ("traj", "fit")}
        p = lambda t: t.data_ptr()
        st = self.states
        self.partials = {
            "traj": [p(self.pred), p(self.x2d), p(self.traj), p(self.cam), p(conn), B, T, P, F, J, 0, p(st["traj"]), L, stream],
            "fit": [p(self.pred), p(self.x2d), p(self.conf), p(self.cam), p(conn), B, T, P, F, J, 0, p(st["fit"]), L, None, stream]}
        self.combine = {k: [p(st[k]), 1, L, B, T, F, J, P, None, *(p(t) for t in self.out[k]), stream] for k in st}

    def traj_leg(self):
        self.check(self.lib.pafuse_pose_partials(*self.partials["traj"]))
        self.check(self.lib.pafuse_pose_combine(*self.combine["traj"]))

    def fit_leg(self):
        self.check(self.lib.pafuse_pose_partials_fit(*self.partials["fit"]))
        self.check(self.lib.pafuse_pose_combine(*self.combine["fit"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rootfit_bench.json"))
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
        legs = Legs(torch, lib, _lib.check, conn, make_inputs(torch, gu, B, T, P, F, seed=70 + B))
        times = {"traj": [], "fit": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.traj_leg(), legs.fit_leg()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("traj", "fit"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name + "_leg")()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the pair computes is pinned by tests/test_hip_rootfit.py): the same sums, a pick wherever
        # there is a weight
        assert torch.equal(legs.out["fit"][0], legs.out["traj"][0])
        assert torch.equal(legs.out["fit"][2] >= 0, (legs.conf > 0)[:, None].expand(B, T, F, J))
        n = B * T * F * J
        read = legs.pred.numel() * 4
        by = {"traj": read + 2 * 44 * n + 28 * n, "fit": read + 2 * 44 * n + 28 * n}
        row = {"B": B, "T": T, "P": P, "F": F, "J": J}
        for name in ("traj", "fit"):
            t = sorted(times[name])
            med = statistics.median(t)
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"min_us": round(t[0], 2), "median_us": round(med, 2), "p90_us": round(p90, 2),
                         "spread_us": round(p90 - t[0], 2), "useful_bytes": by[name],
                         "useful_GB_per_s": round(by[name] / t[0] / 1e3, 1)}
        row["fit_over_traj_min"] = round(row["fit"]["min_us"] / row["traj"]["min_us"], 3)
        row["fit_over_traj_median"] = round(row["fit"]["median_us"] / row["traj"]["median_us"], 3)
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

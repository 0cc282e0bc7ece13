"""Cost and accuracy of evaluation from partial reductions against the one-kernel evaluation, one JSON document.

    python tools/partials_bench.py [--out profiles/partials_vs_unsharded.json] [--reps 30] [--only-cost]

Cost: the C-ABI calls pafuse_hypothesis_partials + pafuse_hypothesis_combine ("new") against pafuse_hypothesis_errors
("old") on the same [B,T,P,F,J,3] predictions (B = 1 and B = 64, P = 20, T = 10, F = 27, J = 134).  Both legs are bare
ctypes calls on operands, index tables, outputs, state and workspace that were all allocated before the timed region; HIP
events around each call, warm, the two alternating, median of `--reps`.  These are call times (launch included), not kernel
times: for those run the tool under `rocprofv3 --kernel-trace --stats -- python tools/partials_bench.py --only-cost` and read
metrics_kernel against partials_kernel + partials_hsum_kernel + combine_kernel.  Useful bytes are counted from the shapes:
both read the predictions once; the old kernel writes two [B,T,P,F,J] maps beside its four [B,T,F,J] ones, the new
kernels 40 bytes per (b,t,f,j), the workgroups' per-hypothesis shares (written and read once) and the four maps.
Accuracy: max |d| to an fp64 evaluation of the same predictions (the reference's formulas on the fp32 whole-body poses,
every sum in fp64) of the accumulators whose sums the old kernel forms in fp32 and the new one in fp64.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
J, PARTS = 134, 4


def make_inputs(torch, gu, B, T, P, F, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(B, F, J, 3, generator=g) * 0.3
    pred = gt[:, None, None] + torch.randn(B, T, P, F, J, 3, generator=g) * 0.05
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    traj = torch.randn(B, F, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    return tuple(t.contiguous().cuda() for t in (pred, gt, x2d, traj, cam))


class Legs:
    """both evaluations of one set of operands as bare library calls; everything they touch is allocated here, once"""

    def __init__(self, torch, lib, check, tables, z):
        self.pred, self.gt, self.x2d, self.traj, self.cam = z
        self.conn, self.pbroot, self.part = tables
        B, T, P, F, _, _ = self.pred.shape
        self.dims = (B, T, P, F)
        self.lib, self.check, self.stream = lib, check, torch.cuda.current_stream().cuda_stream
        dev = self.pred.device
        self.e3, self.epb = (torch.empty(B, T, P, F, J, device=dev) for _ in range(2))
        self.old_maps = [torch.empty(B, T, F, J, device=dev) for _ in range(4)]       # jbest, pagg, jagg, paggpb
        self.new_maps = [torch.empty(B, T, F, J, device=dev) for _ in range(4)]
        self.state = torch.empty(lib.pafuse_hypothesis_partials_bytes(B, T, P, F, J, PARTS) // 8, device=dev, dtype=torch.float64)
        self.work = torch.empty(max(lib.pafuse_hypothesis_partials_workspace_bytes(B, T, P, F, J, PARTS) // 8, 1), device=dev,
                                dtype=torch.float64)
        p = lambda t: t.data_ptr()
        self.common = [p(t) for t in (self.pred, self.gt, self.x2d, self.traj, self.cam, self.conn, self.pbroot)]
        self.old_out = [p(self.e3), p(self.epb)] + [p(t) for t in self.old_maps]
        self.new_out = [p(t) for t in self.new_maps]

    def old(self):
        B, T, P, F = self.dims
        self.check(self.lib.pafuse_hypothesis_errors(*self.common, B, T, P, F, J, *self.old_out, self.stream))

    def new(self):
        B, T, P, F = self.dims
        self.check(self.lib.pafuse_hypothesis_partials(*self.common, self.part.data_ptr(), PARTS, B, T, P, F, J, 0,
                                                       self.state.data_ptr(), self.state.numel() * 8, self.work.data_ptr(),
                                                       self.work.numel() * 8, self.stream))
        self.check(self.lib.pafuse_hypothesis_combine(self.state.data_ptr(), 1, self.state.numel() * 8, self.gt.data_ptr(),
                                                      self.conn.data_ptr(), self.pbroot.data_ptr(), B, T, F, J, P, None,
                                                      *self.new_out, self.stream))


def distances_to_fp64(torch, gu, legs):
    """max |d| (metres) of both legs' P-Agg maps and per-hypothesis means to the fp64 evaluation"""
    B, T, P, F = legs.dims
    legs.old(), legs.new()
    torch.cuda.synchronize()
    pred, gt = legs.pred.cpu(), legs.gt.cpu()
    conn, root = legs.conn.cpu().long(), legs.pbroot.cpu().long()

    def wb(pose):                                              # wb_pose_from_parts, fp32 as the reference forms it
        out = pose + pose[..., conn, :]
        out[..., 0, :] = 0
        return out

    w, g = wb(pred), wb(gt)
    wc, gc = (w - w[..., root, :]).double(), (g - g[..., root, :]).double()
    w, g = w.double(), g.double()
    mean = w.mean(dim=2)
    truth = {"pagg": (mean - g[:, None]).norm(dim=-1), "paggpb": ((mean - mean[..., root, :]) - gc[:, None]).norm(dim=-1)}
    e3, epb = (w - g[:, None, None]).norm(dim=-1), (wc - gc[:, None, None]).norm(dim=-1)
    per_h = lambda x: x.permute(1, 2, 0, 3, 4).reshape(T, P, -1).mean(-1)
    truth["per_hypothesis_mean_e3"], truth["per_hypothesis_mean_epb"] = per_h(e3), per_h(epb)
    hs = legs.state[5 * B * T * F * J:].view(P, T, 1 + PARTS).permute(1, 0, 2).cpu()
    n = B * F * J
    got = {"old": {"pagg": legs.old_maps[1], "paggpb": legs.old_maps[3], "per_hypothesis_mean_e3": per_h(legs.e3),
                   "per_hypothesis_mean_epb": per_h(legs.epb)},
           "new": {"pagg": legs.new_maps[1], "paggpb": legs.new_maps[3], "per_hypothesis_mean_e3": (hs[..., 0] / n).float(),
                   "per_hypothesis_mean_epb": (hs[..., 1:].sum(-1) / n).float()}}
    for i, (name, idx) in enumerate(gu.DATASET_PART_JOINTS.items()):
        k = "per_hypothesis_mean_epb_" + name
        truth[k] = per_h(epb[..., list(idx)])
        got["old"][k] = per_h(legs.epb[..., list(idx)])
        got["new"][k] = (hs[..., 1 + i] / (B * F * len(idx))).float()
    return {leg: {k: (v.cpu().double() - truth[k]).abs().max().item() for k, v in vals.items()} for leg, vals in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only-cost", action="store_true")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from pafuse_amd import _lib
    from pafuse_amd import synthetic as gu
    from pafuse_amd.evaluate import _part_table, _tables
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib = _lib.load()
    ds = SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                         parts_connection_indices=dict(gu.CONNECTION_INDICES))
    tables = _tables(ds, J, "cuda") + (_part_table(ds, J, "cuda"),)
    doc = {"device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps,
           "what_is_timed": "C-ABI calls between HIP events, every buffer and table allocated beforehand", "cost": [], "accuracy": []}
    T, P, F = 10, 20, 27
    for B in (1, 64):
        legs = Legs(torch, lib, _lib.check, tables, make_inputs(torch, gu, B, T, P, F, seed=40 + B))
        times = {"old": [], "new": []}
        for _ in range(3):                                           # warm: code objects, caches
            legs.old(), legs.new()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name in ("old", "new"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                getattr(legs, name)()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        n, nblk = B * T * F * J, (F * J + 255) // 256
        read = legs.pred.numel() * 4
        by = {"old": read + 2 * n * P * 4 + 4 * n * 4,
              "new": read + 40 * n + 2 * B * T * nblk * P * (1 + PARTS) * 8 + 40 * n + 4 * n * 4}
        row = {"B": B, "T": T, "P": P, "F": F, "J": J}
        for name in ("old", "new"):
            t = sorted(times[name])
            med = statistics.median(t)
            row[name] = {"median_us": round(med, 2), "min_us": round(t[0], 2), "p90_us": round(t[int(0.9 * (len(t) - 1))], 2),
                         "useful_bytes": by[name], "useful_GB_per_s": round(by[name] / med / 1e3, 1)}
        row["new_over_old"] = round(row["new"]["median_us"] / row["old"]["median_us"], 3)
        doc["cost"].append(row)
        print(json.dumps(row), flush=True)
        del legs
        torch.cuda.empty_cache()
    if not a.only_cost:
        for B, T_, P_, F_, seed in ((2, 2, 20, 5, 77), (1, 2, 160, 27, 78)):
            legs = Legs(torch, lib, _lib.check, tables, make_inputs(torch, gu, B, T_, P_, F_, seed))
            row = {"B": B, "T": T_, "P": P_, "F": F_, "J": J, "max_abs_to_fp64_m": distances_to_fp64(torch, gu, legs)}
            doc["accuracy"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

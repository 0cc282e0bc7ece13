"""Cost of the J-Agg path of a whole video against the per-clip path it generalises, one JSON document.

    python tools/frames_path_bench.py [--out profiles/frames_path_bench.json] [--reps 30]

Three legs per video length (N = 594 and N = 5 000 frames; T = 10, P = 20, F = 27, J = 134), bare C-ABI calls on operands,
tables, outputs and workspaces that were all allocated before the timed region; HIP events around each call, warm, the
legs alternating in one process:

  A  pafuse_pose_path, unchanged, on the video cut into ceil(N / 27) clips (stride = F): the yardstick
  B  pafuse_frames_path on the same clips (stride = F: K = 20 candidates per frame, 40 where the shifted last clip overlaps)
  C  pafuse_frames_path on the windows of stride 9 (K = 60 .. 80)

A and B walk the same hypotheses and, up to the seams, the same transitions; A spreads its frames over clips * T * J waves,
B and C run T * J = 1 340 waves of N dependent frames each.  These are call times (launch included), not kernel times.
`transitions` counts the (s', s) pairs of the recursion - one fp64 square root each - per call, `bytes` what a call has to
move, from the shapes: the hypotheses once, 12 bytes of mean and 8 of detection per (t, n, j), one back-pointer byte written
per (line, frame, candidate) and one read per (line, frame), 24 bytes of outputs per (t, n, j) (20 for A) and 8 per line.
Per leg: min, median, p90 and `spread_us` = p90 - min of its repeats.  No target is fixed in advance.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.partials_bench import J  # noqa: E402

T, P, F = 10, 20, 27
LENGTHS = (594, 5000)
WEIGHT = 0.5


def video(torch, N, seed):
    g = torch.Generator().manual_seed(seed)
    x2d = torch.rand(N, J, 2, generator=g) * 2 - 1
    traj = torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    mean = torch.randn(N, J, 3, generator=g) * 0.3
    cam = torch.tensor([2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001])
    return tuple(t.contiguous().cuda() for t in (x2d, traj, mean, cam))


class Windows:
    """the windows of one stride with their hypotheses (the video's mean pose plus 5 cm of noise, drawn on the device), the
    tables on both sides, outputs and workspace: everything a pafuse_frames_path call touches"""

    def __init__(self, torch, lib, conn, N, stride, vid, seed):
        from pafuse_amd.windows import coverage, window_starts
        x2d, traj, mean, cam = vid
        self.starts, self.valid = window_starts(N, F, stride)
        W = self.W = len(self.starts)
        at = torch.from_numpy(self.starts.astype(np.int64)).cuda()[:, None] + torch.arange(F, device="cuda")[None]      # [W,F]
        gd = torch.Generator(device="cuda").manual_seed(seed)
        self.pred = (mean[at][:, None, None] + torch.randn(W, T, P, F, J, 3, device="cuda", generator=gd) * 0.05).contiguous()
        self.at, self.N, self.lib = at, N, lib
        self.tables = torch.from_numpy(np.stack([self.starts, self.valid])).cuda()
        self.mean = mean[None].expand(T, N, J, 3).contiguous()
        self.pick = torch.empty(T, N, J, 3, device="cuda")
        self.idx, self.win = (torch.empty(T, N, J, device="cuda", dtype=torch.int32) for _ in range(2))
        self.e2 = torch.empty(T, N, J, device="cuda")
        self.cost = torch.empty(T, J, device="cuda", dtype=torch.float64)
        self.ws_bytes = int(lib.pafuse_frames_path_workspace_bytes(N, T, J, P, W, self.starts.ctypes.data, self.valid.ctypes.data))
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, device="cuda", dtype=torch.uint8)
        stream = torch.cuda.current_stream().cuda_stream
        p = lambda t: t.data_ptr()
        self.args = [p(self.pred), p(x2d), p(traj), 0, p(cam), None, p(conn), p(self.mean), WEIGHT, W, T, P, F, J, N,
                     p(self.tables[0]), p(self.tables[1]), self.starts.ctypes.data, self.valid.ctypes.data,
                     p(self.pick), p(self.idx), p(self.win), p(self.e2), p(self.cost), p(self.ws), self.ws_bytes, stream]
        cover = coverage(N, self.starts, self.valid) * P                                     # candidates per frame
        self.K = int(cover.max())
        self.transitions = int(T * J * int((cover[1:] * cover[:-1]).sum()))
        rows = T * N * J
        self.bytes = int(self.pred.numel() * 4 + 20 * rows + T * J * int(cover.sum()) + T * J * N + 24 * rows + 8 * T * J)

    def call(self, check):
        check(self.lib.pafuse_frames_path(*self.args))


class Clips:
    """leg A: pafuse_pose_path on the hypotheses of a Windows(stride = F), as clips"""

    def __init__(self, torch, lib, conn, w, vid):
        x2d, traj, mean, cam = vid
        B = w.W
        self.lib = lib
        self.x2d, self.traj = x2d[w.at.clamp(max=w.N - 1)].contiguous(), traj[w.at.clamp(max=w.N - 1)].contiguous()
        self.mean = mean[w.at.clamp(max=w.N - 1)][:, None].expand(B, T, F, J, 3).contiguous()
        self.pick = torch.empty(B, T, F, J, 3, device="cuda")
        self.idx = torch.empty(B, T, F, J, device="cuda", dtype=torch.int32)
        self.e2 = torch.empty(B, T, F, J, device="cuda")
        self.cost = torch.empty(B, T, J, device="cuda", dtype=torch.float64)
        self.ws_bytes = int(lib.pafuse_pose_path_workspace_bytes(B, T, P, F, J))
        self.ws = torch.empty(self.ws_bytes, device="cuda", dtype=torch.uint8)
        stream = torch.cuda.current_stream().cuda_stream
        p = lambda t: t.data_ptr()
        self.args = [p(w.pred), p(self.x2d), p(self.traj), 0, p(cam), None, p(conn), p(self.mean), WEIGHT, B, T, P, F, J,
                     p(self.pick), p(self.idx), p(self.e2), p(self.cost), p(self.ws), self.ws_bytes, stream]
        self.K, self.W = P, B
        self.transitions = B * T * J * (F - 1) * P * P
        rows, lines = B * T * F * J, B * T * J
        self.bytes = int(w.pred.numel() * 4 + 20 * rows + lines * F * P + lines * F + 20 * rows + 8 * lines)

    def call(self, check):
        check(self.lib.pafuse_pose_path(*self.args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_path_bench.json"))
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
           "weight": WEIGHT, "T": T, "P": P, "F": F, "J": J,
           "what_is_timed": "one C-ABI call between HIP events, every buffer and table allocated beforehand; legs alternating",
           "legs": {"A": "pafuse_pose_path on the clips (stride = F)", "B": "pafuse_frames_path on the same clips",
                    "C": "pafuse_frames_path on the windows of stride 9"},
           "cost": []}
    for N in LENGTHS:
        vid = video(torch, N, seed=70 + N)
        wb = Windows(torch, lib, conn, N, F, vid, seed=N)
        legs = {"A": Clips(torch, lib, conn, wb, vid), "B": wb, "C": Windows(torch, lib, conn, N, 9, vid, seed=N + 1)}
        times = {k: [] for k in legs}
        for _ in range(2):                                           # warm: code objects, caches
            for leg in legs.values():
                leg.call(_lib.check)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, leg in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                leg.call(_lib.check)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # sanity of the run only (what the kernel computes is pinned by tests/test_hip_frames_path.py): every line has a path,
        # B's picks inside a clip that no other clip overlaps come from that clip, and C's paths change window
        assert (wb.idx >= 0).all() and (legs["C"].idx >= 0).all() and (legs["A"].idx >= 0).all()
        assert (wb.win[:, :F] == 0).all() and bool((legs["C"].win[:, 1:] != legs["C"].win[:, :-1]).any())
        row = {"N": N}
        for name, leg in legs.items():
            t = sorted(times[name])
            p90 = t[int(0.9 * (len(t) - 1))]
            row[name] = {"windows": leg.W, "K": leg.K, "workspace_bytes": leg.ws_bytes, "min_us": round(t[0], 1),
                         "median_us": round(statistics.median(t), 1), "p90_us": round(p90, 1), "spread_us": round(p90 - t[0], 1),
                         "transitions": leg.transitions, "transitions_per_s": round(leg.transitions / t[0] * 1e6),
                         "bytes": leg.bytes, "GB_per_s": round(leg.bytes / t[0] / 1e3, 1)}
            if name != "A":
                row[name]["us_per_frame"] = round(t[0] / N, 3)
        row["B_over_A_min"] = round(row["B"]["min_us"] / row["A"]["min_us"], 3)
        row["C_over_A_min"] = round(row["C"]["min_us"] / row["A"]["min_us"], 3)
        doc["cost"].append(row)
        print(json.dumps(row), flush=True)
        del legs, wb
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

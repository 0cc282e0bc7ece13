"""sha256 of everything the evaluation kernels write, on seeded inputs: one JSON object, to compare two trees bit for bit.

    python tools/eval_bits.py [--out digests.json]

Every evaluation entry is called through pafuse_amd.ops (pafuse_hypothesis_errors, which has no op, through the library as
evaluate.evaluate_accumulators calls it) and every output tensor and every flat state is hashed as raw bytes.  States are
written into zeroed buffers of exactly their size, so no byte hashed is one the library did not write or the tool did not
set.  The Python API is all the tool touches: the same file runs against any tree that has these ops.  Inputs:
  hostile   B=1 T=2 P=6 cut 4+2, F=2, J=134 (hostile_inputs below: an exact tie across the cut, Z = 0, a projection clamped
            in every hypothesis, a detection that is NaN)
  random    B=2 T=2 P=70 cut 64+6, F=3, J=134; conf holds zeros, a negative and a NaN weight and one frame without any
            weight (64 and 6 behind a full chunk: the fit kernel re-reads its state between chunks)
  empty     the hostile shards with an empty shard (P_r = 0) in first and in middle position
  frames    N=40 video frames, windows of F=27 at stride 5, folded in batches of 1 and of 3, finished, root trajectory
  frame_kernels  root fit, focal sums and frame errors at J = 5, 65, 134, 200, 300 (every joint-slot form), N=7, T=2, with NaN
            joints, zero, negative and NaN weights, a NaN part root and frames with fewer than 4 valid joints; focal solve on
            states of N = 1, 65, 130
  line_filters   the smoother at (N, r) = (1, 1), (9, 4), (70, 64) and the repair at (J, N, r) = (5, 9, 3), (65, 9, 64),
            (134, 70, 13), the last on the whole-body anchors with planted dropouts, an unfillable run and a lost anchor
All inputs are drawn on the CPU from seeded generators: two trees see the same bytes.
"""
import argparse
import hashlib
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
J, PARTS = 134, 4
CAM = [2.29, 2.287, 0.025, 0.029, -0.207, 0.247, -0.003, -0.0009, -0.001]
HOSTILE = {"shape": (1, 2, 6, 2), "cut": (4, 2), "tie": (3, 4), "z0": (1, 20), "clamped": 30, "nan": (1, 50)}


def dataset():
    from pafuse_amd import synthetic as gu
    return SimpleNamespace(parts_joint_indices=gu.DATASET_PART_JOINTS, root_indices=gu.ROOT_INDICES,
                           parts_connection_indices=dict(gu.CONNECTION_INDICES))


def tables(device="cuda"):
    """conn, pbroot, part: int32 [J] each"""
    from pafuse_amd.evaluate import _part_table, _tables
    return _tables(dataset(), J, device) + (_part_table(dataset(), J, device),)


def random_inputs(B, T, P, F, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(B, F, J, 3, generator=g) * 0.3
    pred = gt[:, None, None] + torch.randn(B, T, P, F, J, 3, generator=g) * 0.05
    x2d = torch.rand(B, F, J, 2, generator=g) * 2 - 1
    traj = torch.randn(B, F, 3, generator=g) * 0.1
    traj[..., 2] = 4.0
    return {"pred": pred, "gt": gt, "x2d": x2d, "traj": traj, "cam": torch.tensor(CAM)}


def hostile_inputs(device="cuda"):
    """One input for every kernel that forms the J-Agg index (shape and places: HOSTILE).  Planted:
      * hypotheses 3 and 4, either side of the 4+2 cut, hold the same bits: an exact tie in e2;
      * in hypothesis 1 (t = 0, f = 0) the depth of joint 20 is exactly -traj_z: Z = 0, X/Z and Y/Z are +-inf;
      * joint 30 lies 100 m off the axis in every hypothesis: both projected coordinates clamp to 1, all e2 are equal;
      * the detection of joint 50 in frame 1 is NaN: e2 is NaN in every hypothesis, there is no pick (index -1)."""
    import torch
    B, T, P, F = HOSTILE["shape"]
    z = random_inputs(B, T, P, F, seed=4242)
    pred, conn = z["pred"], tables("cpu")[0].long()
    h, j = HOSTILE["z0"]
    jc = int(conn[j])
    pred[0, 0, h, 0, jc, 2] = torch.round(pred[0, 0, h, 0, jc, 2] * 1024) / 1024   # a multiple of 2^-10: the next two sums are exact
    pred[0, 0, h, 0, j, 2] = -z["traj"][0, 0, 2] - pred[0, 0, h, 0, jc, 2]
    assert float((pred[0, 0, h, 0, j, 2] + pred[0, 0, h, 0, jc, 2]) + z["traj"][0, 0, 2]) == 0.0
    pred[:, :, :, :, HOSTILE["clamped"], :2] = 100.0
    f, j = HOSTILE["nan"]
    z["x2d"][:, f, j] = float("nan")
    lo, hi = HOSTILE["tie"]
    pred[:, :, hi] = pred[:, :, lo]
    return {k: v.contiguous().to(device) for k, v in z.items()}


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class Run:
    def __init__(self):
        import torch
        from pafuse_amd import ops
        self.torch, self.ops, self.out = torch, ops, {}
        self.conn, self.pbroot, self.part = tables()

    def put(self, key, value):
        if isinstance(value, dict):
            for k, v in value.items():
                self.put(f"{key}.{k}", v)
        else:
            assert key not in self.out, key
            self.out[key] = digest(value)

    def zeros(self, nbytes):
        return self.torch.zeros(nbytes // 8, device="cuda", dtype=self.torch.float64)

    def shards(self, tag, z, cut, conf):
        """every partial-state entry on the hypotheses of z cut into `cut` (a 0 is an empty shard), then every combine:
        in one call, and as a running state merged in place"""
        torch, ops = self.torch, self.ops
        pred, gt, x2d, traj, cam = (z[k] for k in ("pred", "gt", "x2d", "traj", "cam"))
        B, T, P, F = pred.shape[:4]
        shape, n = (B, T, F, J), B * T * F * J
        pmax, W = max(cut), len(cut)
        rows = {"p1": ops.partials_bytes(B, T, pmax, F, J, PARTS), "pose": ops.pose_partials_bytes(B, T, F, J),
                "fit": ops.pose_partials_bytes(B, T, F, J), "spread": ops.spread_partials_bytes(B, T, F, J),
                "p2": ops.procrustes_partials_bytes(B, T, pmax, F, J)}
        st = {k: self.zeros(W * v).view(W, v // 8) for k, v in rows.items()}
        lo = 0
        for r, size in enumerate(cut):
            local = pred[:, :, lo:lo + size].contiguous()
            ops.hypothesis_partials(local, gt, x2d, traj, cam, self.conn, self.pbroot, self.part, PARTS, lo, out=st["p1"][r])
            ops.pose_partials(local, self.conn, lo, x2d, traj, cam, out=st["pose"][r])
            tfit = torch.zeros(B, T, size, F, 3, device="cuda")
            ops.pose_partials_fit(local, self.conn, lo, x2d, cam, conf=conf, out=st["fit"][r], tfit=tfit)
            ops.spread_partials(local, self.conn, lo, out=st["spread"][r])
            ops.procrustes_partials(local, gt, x2d, traj, cam, self.conn, lo, out=st["p2"][r])
            self.put(f"{tag}.tfit.{r}", tfit)
            lo += size
        assert lo == P
        mean_only = ops.pose_partials(pred, self.conn, 0, out=self.zeros(rows["pose"]))
        self.put(f"{tag}.states", dict(st, pose_mean_only=mean_only))
        merged = {"p1": self.zeros(40 * n), "pose": self.zeros(rows["pose"]), "fit": self.zeros(rows["fit"]),
                  "spread": self.zeros(rows["spread"]), "p2": self.zeros(16 * n)}
        self.put(f"{tag}.combine.p1", ops.combine_partials(st["p1"], gt, self.conn, self.pbroot, shape, P))
        ops.combine_partials(st["p1"], gt, self.conn, self.pbroot, shape, P, merged=merged["p1"], maps=False)
        self.put(f"{tag}.combine.pose", ops.combine_poses(st["pose"], shape, P, merged=merged["pose"]))
        self.put(f"{tag}.combine.fit", ops.combine_poses(st["fit"], shape, P, merged=merged["fit"], no_pick_ok=True))
        self.put(f"{tag}.combine.spread", ops.combine_spread(st["spread"], shape, merged=merged["spread"]))
        self.put(f"{tag}.combine.p2", ops.combine_procrustes(st["p2"], shape, P, sums=st["p1"], gt=gt, conn=self.conn,
                                                             merged=merged["p2"]))
        self.put(f"{tag}.merged", merged)
        # a running state: rows 1 .. W-1 merged into row 0 in place, one at a time
        for r in range(1, W):
            for k in ("pose", "fit", "spread", "p2"):
                st[k][1].copy_(st[k][r])
            st["p1"][1].copy_(st["p1"][r])
            ops.combine_partials(st["p1"][:2], gt, self.conn, self.pbroot, shape, P, merged=st["p1"][0], maps=False)
            ops.combine_poses(st["pose"][:2], shape, 1, merged=st["pose"][0], want=())
            ops.combine_poses(st["fit"][:2], shape, 1, merged=st["fit"][0], want=())
            ops.combine_spread(st["spread"][:2], shape, merged=st["spread"][0], want=())
            ops.combine_procrustes(st["p2"][:2], shape, P, merged=st["p2"][0], want=())
        self.put(f"{tag}.running", {k: v[0][:(40 * n if k == "p1" else 16 * n if k == "p2" else rows[k]) // 8] for k, v in st.items()})
        return merged

    def unsharded(self, tag, z):
        torch = self.torch
        from pafuse_amd import _lib
        from pafuse_amd.evaluate import evaluate_accumulators
        pred, gt, x2d, traj, cam = (z[k] for k in ("pred", "gt", "x2d", "traj", "cam"))
        B, T, P, F = pred.shape[:4]
        o = {k: torch.zeros(B, T, P, F, J, device="cuda") for k in ("e3", "epb")}
        o.update({k: torch.zeros(B, T, F, J, device="cuda") for k in ("jbest", "pagg", "jagg", "paggpb")})
        _lib.check(_lib.load().pafuse_hypothesis_errors(
            pred.data_ptr(), gt.data_ptr(), x2d.data_ptr(), traj.data_ptr(), cam.data_ptr(), self.conn.data_ptr(),
            self.pbroot.data_ptr(), B, T, P, F, J, *(o[k].data_ptr() for k in ("e3", "epb", "jbest", "pagg", "jagg", "paggpb")),
            torch.cuda.current_stream().cuda_stream))
        self.put(f"{tag}.hypothesis_errors", o)
        self.put(f"{tag}.evaluate_accumulators", evaluate_accumulators(pred, gt, x2d, traj, cam, dataset(), p2=True))
        self.put(f"{tag}.procrustes_errors", self.ops.procrustes_errors(pred, gt, x2d, traj, cam, self.conn, pick=True))

    def frames(self):
        """one video of N frames cut into windows; the window states folded into frame states in batches of 1 and of 3"""
        torch, ops = self.torch, self.ops
        from pafuse_amd.windows import window_starts
        N, T, P, F, stride = 40, 2, 3, 27, 5
        starts, valid = window_starts(N, F, stride)
        Bw = len(starts)
        g = torch.Generator().manual_seed(909)
        pred = (torch.randn(Bw, T, P, F, J, 3, generator=g) * 0.2).cuda()
        video_x2d = torch.rand(N, J, 2, generator=g) * 2 - 1
        conf = torch.rand(N, J, generator=g)
        conf[conf < 0.2] = 0
        conf[7] = 0                                                  # a frame without any weight
        x2d = torch.stack([video_x2d[s:s + F] for s in starts]).contiguous().cuda()
        traj = torch.zeros(Bw, F, 3)
        traj[..., 2] = 4.0
        traj, cam, conf, video_x2d = traj.cuda(), torch.tensor(CAM).cuda(), conf.cuda(), video_x2d.cuda()
        for batch in (1, 3):
            frame, spread = ops.frame_state(N, T, J), ops.frame_state(N, T, J, spread=True)
            for w0 in range(0, Bw, batch):
                sl = slice(w0, min(w0 + batch, Bw))
                b = sl.stop - sl.start
                ps = ops.pose_partials(pred[sl].contiguous(), self.conn, 0, x2d[sl].contiguous(), traj[sl].contiguous(), cam,
                                       out=self.zeros(ops.pose_partials_bytes(b, T, F, J)))
                ss = ops.spread_partials(pred[sl].contiguous(), self.conn, 0, out=self.zeros(ops.spread_partials_bytes(b, T, F, J)))
                ops.fold_windows(frame, N, ps, (b, T, F, J), starts[sl], valid[sl], w0, P)
                ops.fold_spread_windows(spread, N, ss, (b, T, F, J), starts[sl], valid[sl])
            done = ops.finish_frames(N, T, J, frame=frame, spread=spread)
            self.put(f"frames.batch{batch}", {"frame": frame, "spread": spread, "finish": done})
            for name in ("mean", "pick"):
                fit = ops.fit_trajectory(done[name], video_x2d, cam, conf=conf)
                fit["smooth"] = ops.smooth_trajectory(fit["traj"], fit["wsum"], 4)
                self.put(f"frames.batch{batch}.trajectory.{name}", fit)
        self.put("frames.trajectory.no_conf", ops.fit_trajectory(done["mean"], video_x2d, cam))

    def frame_kernels(self):
        """the wave-per-(t, frame) kernels at every joint-slot form (J <= 64, 128, 192, 256 and beyond), N = 7, T = 2"""
        torch, ops = self.torch, self.ops
        T, N = 2, 7
        cam = torch.tensor(CAM).cuda()
        for Jn in (5, 65, 134, 200, 300):
            g = torch.Generator().manual_seed(1000 + Jn)
            gt = torch.randn(N, Jn, 3, generator=g) * 0.3
            pose = gt[None] + torch.randn(T, N, Jn, 3, generator=g) * 0.05
            x2d = torch.rand(N, Jn, 2, generator=g) * 2 - 1
            conf = torch.rand(N, Jn, generator=g)
            traj = torch.randn(T, N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
            gt_root = torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
            part = torch.arange(Jn, dtype=torch.int32) % PARTS        # part roots: joints 0 .. 3
            pbroot = part.clone()
            conf[conf < 0.2] = 0
            conf[1, 0], conf[2, Jn - 1], conf[3, Jn // 2] = -0.5, float("nan"), 0.0
            pose[0, 1, Jn - 1, 1] = float("nan")                     # NaN joints: one component, a whole joint
            pose[1, 2, Jn // 2] = float("nan")
            pose[:, 4, 1] = float("nan")                             # a NaN part root
            pose[0, 5, 3:] = float("nan")                            # a frame with fewer than 4 valid joints
            conf[6, 2:] = 0                                          # and one by its weights
            traj[1, 3] = float("nan")
            gt[2, 0, 0] = float("nan")
            pose, gt, x2d, conf, traj, gt_root, part, pbroot = (v.contiguous().cuda() for v in (pose, gt, x2d, conf, traj, gt_root, part, pbroot))
            for tag, c in (("conf", conf), ("no_conf", None)):
                self.put(f"frame_kernels.J{Jn}.fit_trajectory.{tag}", ops.fit_trajectory(pose, x2d, cam, conf=c))
                self.put(f"frame_kernels.J{Jn}.focal_sums.{tag}", ops.focal_sums(pose, x2d, cam, conf=c))
            self.put(f"frame_kernels.J{Jn}.frame_errors.rooted", ops.frame_errors(pose, gt, pbroot, part, PARTS, traj=traj, gt_root=gt_root, per_frame=True))
            self.put(f"frame_kernels.J{Jn}.frame_errors.plain", ops.frame_errors(pose, gt, pbroot, part, PARTS, per_frame=True))
        for Nn in (1, 65, 130):
            g = torch.Generator().manual_seed(2000 + Nn)
            state = torch.rand(3, Nn, 4, generator=g, dtype=torch.float64) + 0.5
            state[..., 3] = 1.0
            state[torch.rand(3, Nn, generator=g) < 0.3] = 0.0        # frames that take no part
            state[2] = 0.0                                           # a t without any frame
            self.put(f"frame_kernels.focal_solve.N{Nn}", ops.focal_solve(state.cuda(), cam))

    def line_filters(self):
        """the smoother and the repair: both outcomes of the filter (line, mean) and none"""
        torch, ops = self.torch, self.ops
        from pafuse_amd import detections
        for Nn, r in ((1, 1), (9, 4), (70, 64)):
            g = torch.Generator().manual_seed(3000 + Nn)
            traj = torch.randn(2, Nn, 3, generator=g)
            weight = torch.rand(2, Nn, generator=g)
            traj[torch.rand(2, Nn, generator=g) < 0.3] = float("nan")
            weight[torch.rand(2, Nn, generator=g) < 0.3] = 0
            if Nn > 1:
                weight[1, 1:] = 0                                    # one frame left: the mean; t = 1, frame 0 may be NaN: none
            self.put(f"line_filters.smooth.N{Nn}_r{r}", {"weighted": ops.smooth_trajectory(traj.cuda(), weight.cuda(), r),
                                                       "plain": ops.smooth_trajectory(traj.cuda(), None, r)})
        for Jn, Nn, r in ((5, 9, 3), (65, 9, 64), (134, 70, 13)):
            g = torch.Generator().manual_seed(4000 + Jn)
            x2d = torch.rand(Nn, Jn, 2, generator=g) * 2 - 1
            if Jn == J:
                anchor = detections.repair_anchors(dataset())
                lost = torch.from_numpy(detections.plant_dropouts(Nn, Jn, 0.2, 10, seed=4000))
                lost[20:50, 40] = True                               # an unfillable run: nothing within 13 frames of its middle
                lost[:, int(anchor[100])] = True                     # a lost anchor: what hangs on it cannot be filled
                conf = torch.rand(Nn, Jn, generator=g) * 0.9 + 0.1
            else:
                anchor = [-1, 0, 0, -1, 3] if Jn == 5 else None
                lost = torch.rand(Nn, Jn, generator=g) < 0.4
                conf = torch.rand(Nn, Jn, generator=g)
                conf[0, 0], x2d[1, 1, 0] = float("nan"), float("nan")
                lost[1:, 2] = True                                   # one frame left: held
            conf[lost] = 0
            x2d[lost] = -1.0
            self.put(f"line_filters.repair.J{Jn}_N{Nn}_r{r}", ops.repair_detections(x2d.cuda(), conf.cuda(), anchor=anchor, radius=r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available(), "the kernels run on the GPU"
    run = Run()
    z = hostile_inputs()
    run.unsharded("hostile", z)
    run.shards("hostile", z, HOSTILE["cut"], torch.ones(*z["x2d"].shape[:3], device="cuda"))
    run.shards("empty_first", z, (0,) + HOSTILE["cut"], None)
    run.shards("empty_middle", z, (HOSTILE["cut"][0], 0, HOSTILE["cut"][1]), None)
    g = torch.Generator().manual_seed(70)
    z = {k: v.contiguous().cuda() for k, v in random_inputs(2, 2, 70, 3, seed=7070).items()}
    conf = torch.rand(2, 3, J, generator=g)
    conf[conf < 0.25] = 0
    conf[0, 0, 3], conf[1, 2, 4] = -0.5, float("nan")
    conf[1, 1] = 0                                                   # a frame without any weight
    run.unsharded("random", z)
    run.shards("random", z, (64, 6), conf.cuda())
    run.frames()
    run.frame_kernels()
    run.line_filters()
    torch.cuda.synchronize()
    doc = json.dumps(run.out, indent=1, sort_keys=True)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The reference's `python main_h3wb.py general.evaluate=pafuse_model.bin ...` flow on real files (main_h3wb.py:568-760,
194-531): H3WB npz -> loader -> per-camera sequences of the test subjects -> D3DP eval model with the checkpoint ->
flip-TTA DDIM sampling on the HIP path -> J-Best / P-Best / P-Agg / J-Agg and the part-based protocols in mm.

    python examples/evaluate_h3wb.py --data data/train_h3wb.npz --checkpoint checkpoint/pafuse_model.bin \
           ft2d.num_proposals=20 ft2d.sampling_timesteps=10
    torchrun --standalone --nproc-per-node 8 examples/evaluate_h3wb.py ... ft2d.num_proposals=160   # hypothesis-sharded

`ft2d.p2=True` adds Protocol #2 (P-MPJPE after similarity alignment) to the log, as in the reference.
Trailing `a.b=c` arguments override the config tree like the reference's Hydra command line (pafuse_amd/config.py).
`--frames` scores one pose per video frame instead (`--aggregate`, `--stride`, `--trajectory [R]`, `--seam-profile`): position,
velocity, acceleration, root and part-based errors of the per-frame output (harness.evaluate_frames).  `--estimate-focal` (with
`--frames --trajectory`) fits and scores the root with the focal length estimated from each video and prints the estimate against
the true one per video (H3WB knows its intrinsics: this is how the estimator can be measured).
`--drop-detections RATE:RUN[:SEED]` (with `--frames`) loses ground-truth 2-D detections on purpose - runs of RUN frames, a share of
about RATE of the joints, detections.plant_dropouts - and `--repair [R]` repairs them on the device before the model sees them
(harness.repair_detections; R in 1 .. 64, default 13); per video the joints per status and detections.repair_error are logged.
Ground-truth 2-D has no dropouts: without the planting nobody can measure whether the repair helps on H3WB.
`--corrupt-detections RATE:RUN:SIZE[:SEED]` and `--swap-detections RATE:RUN[:SEED]` (with `--frames`) plant WRONG detections with
their confidence kept - runs of RUN frames displaced by SIZE (screen-normalised units) and runs of left/right pairs exchanged,
detscreen.corrupt - and `--screen [R]` screens the detections on the device before the repair (harness.screen_detections; R in
1 .. 64, default 13): outliers leave with confidence 0, swaps leave exchanged; per video the detections per status and
detscreen.screen_error are logged.  With `--repair` the rejected detections are filled.  Whether the screen lowers the 3-D error
needs a real checkpoint and has not been measured: this is the tool that measures it.
`--distract-detections PEOPLE[:SEED]` (with `--frames`) plants PEOPLE other people - shifted copies of the subject - and a new order
of the detections in every frame (tracks.plant_people): without `--track` the first detection of every frame is lifted, as a caller
that takes `predictions[0]` does - a splice of the subject and the copies; with `--track` the candidates are linked on the device
and track 0 is lifted (harness.track_people; the defaults, which are not tuned values).  Per video tracks.track_error is logged: the
frames with the subject's detection, with another person's, with nobody, and the switches.  What the tracker buys in 3-D error on
H3WB or on real video has not been measured: this is the tool that will measure it once a real checkpoint exists.
`--path-weight L` (with `--frames --aggregate reproj|reproj_fit`, un-strided) scores the pick made coherent in time: per clip and
joint one path through the hypotheses instead of every frame's own winner (harness.evaluate_frames(path_weight=...)).
`--path-scope video` runs that path along the whole video instead, across clip seams and the pooled windows of `--stride S`
(the candidates of a frame are the hypotheses of all windows covering it; at most 256, kept on the device for the whole video).
`--smooth-pose [R]` (with `--frames`; R in 1 .. 64, default 13; `--smooth-pose-floor S` metres, default 0.001) scores the pose
SMOOTHED along the frames with the covariance of the hypotheses as matrix weight (harness.evaluate_frames(pose_smooth=...)):
compare the mpjpe and accel columns with a run without it.  What it buys on a real checkpoint has not been measured: this is the
tool that measures it.  The 1 mm floor is a regulariser (a zero covariance stays solvable), not a tuned value.
`--bone-lengths [video|symmetric]` (with `--frames`; default video; `--bone-iterations K`, default 16, 0 .. 64) scores the pose with its
BONE LENGTHS HELD CONSTANT along each video (harness.evaluate_frames(bone_lengths=...)): one length per bone from the whole video,
every frame projected onto them under the covariance of its hypotheses, behind `--smooth-pose` and before the trajectory fit.  The
mpjpe and accel columns score it; per video the mean bone-length standard deviation before and after and the largest difference of
the held lengths from the ground truth's are logged.  What it buys on a real checkpoint has not been measured: this is the tool.
16 sweeps and the 1 mm floor are defaults, not tuned values.
`--ground [R]` (with `--frames --trajectory`; R in 1 .. 64, default 3; `--ground-speed V` metres per FRAME, default 0.015) also finds
the GROUND PLANE of every video from its resting feet, behind the trajectory fit (harness.evaluate_frames(ground=...)), and logs
per video and step the code (1 plane, 2 line, 3 the body's own up, 0 none), the camera height and the contact points - and, where
the dataset's camera carries an orientation, the angle between the estimated up and the camera's true up, for the prediction and
for the same estimator run on the ground-truth 3-D, which needs no checkpoint.  The metrics are not changed by it.  What the
estimate is worth on a real checkpoint has not been measured: that angle is the tool.  The defaults are not tuned values.
Without `--data` the synthetic H3WB files of tests/golden/h3wb_synth are used (random weights: numbers are meaningless).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
import pafuse_amd  # noqa: E402
from pafuse_amd import config, h3wb, harness  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "h3wb_synth", "train_h3wb.npz"))
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--config", default="", help="a reference config.yaml (optional)")
    ap.add_argument("--gather", choices=("hypotheses", "partials"), default="hypotheses",
                    help="what the ranks exchange before the aggregation: all hypotheses, or their partial reductions")
    ap.add_argument("--hypothesis-chunk", type=int, default=None,
                    help="with --gather partials: sample and reduce this many hypotheses at a time")
    ap.add_argument("--p2-gather", choices=("hypotheses", "partials"), default="hypotheses",
                    help="with ft2d.p2=True and --gather partials: Protocol #2 from all gathered hypotheses (the default's numbers "
                         "bit for bit), or from per-shard partial states in the same exchange (no hypothesis is kept)")
    ap.add_argument("--noise", choices=("torch", "device"), default="torch",
                    help="where the loop's normals come from: torch.randn on the full tensor, or the library's counter-based "
                         "stream drawn inside the kernels (no noise tensor; other hypotheses than torch.randn's)")
    ap.add_argument("--seed", type=int, default=0, help="with --noise device: the seed of the stream, in [0, 2^32)")
    ap.add_argument("--frames", action="store_true",
                    help="score at the level of video frames instead: one pose per frame (--aggregate, --stride) against the ground "
                         "truth - position, velocity, acceleration and part-based errors (harness.evaluate_frames)")
    ap.add_argument("--aggregate", choices=("mean", "reproj", "reproj_fit"), default="mean", help="with --frames: the pose of a frame")
    ap.add_argument("--stride", type=int, default=None,
                    help="with --frames: slide the window with this stride and pool overlapping windows (default: clips end to end)")
    ap.add_argument("--trajectory", nargs="?", type=int, const=0, default=None, metavar="R",
                    help="with --frames: also fit the camera-space root and score it; R (1 .. 64) smooths it along the frames")
    ap.add_argument("--estimate-focal", action="store_true",
                    help="with --frames --trajectory: fit and score the root with the focal length estimated from each video, and "
                         "print the estimate against the true one per video")
    ap.add_argument("--seam-profile", action="store_true", help="with --frames: the position error by the frame's position in the clip")
    ap.add_argument("--drop-detections", default=None, metavar="RATE:RUN[:SEED]",
                    help="with --frames: lose detections on purpose before the model sees them - runs of RUN frames, about a share RATE "
                         "of the joints (at (-1, -1) with confidence 0), seeded per video with SEED (default 0) + the video's number")
    ap.add_argument("--repair", type=int, default=None, nargs="?", const=13, metavar="R",
                    help="with --frames --drop-detections: repair the lost detections on the device along the frames within R "
                         "(1 .. 64, default 13) and log the repair error per video")
    ap.add_argument("--corrupt-detections", default=None, metavar="RATE:RUN:SIZE[:SEED]",
                    help="with --frames: plant wrong detections with their confidence kept - runs of RUN frames, about a share RATE of "
                         "the joints, displaced by SIZE (screen-normalised units), seeded per video with SEED (default 0) + the video's number")
    ap.add_argument("--swap-detections", default=None, metavar="RATE:RUN[:SEED]",
                    help="with --frames: exchange left/right pairs of detections, confidences included, in runs of RUN frames at about "
                         "a share RATE of the pairs")
    ap.add_argument("--distract-detections", default=None, metavar="PEOPLE[:SEED]",
                    help="with --frames: add PEOPLE (1 .. 63) shifted copies of the subject to every frame and shuffle the order of the "
                         "detections per frame; the first detection of every frame is lifted unless --track")
    ap.add_argument("--track", action="store_true",
                    help="with --distract-detections: link the detections along the frames on the device and lift track 0")
    ap.add_argument("--screen", type=int, default=None, nargs="?", const=13, metavar="R",
                    help="with --frames and a planting: screen the observed detections on the device before the repair - outliers "
                         "against the leave-one-out line within R (1 .. 64, default 13) rejected, left/right swaps exchanged back - "
                         "and log the screen error per video")
    ap.add_argument("--path-weight", type=float, default=None, metavar="L",
                    help="with --frames --aggregate reproj or reproj_fit on un-strided clips: the pick coherent in time - per clip and "
                         "joint one path through the hypotheses, a jump costing L per metre (normalised screen length per metre; "
                         "about fx / depth makes a jump cost what it projects to); compare the mpjpe and accel columns")
    ap.add_argument("--path-scope", choices=("clip", "video"), default="clip",
                    help="with --path-weight: 'clip' (default) one path per un-strided clip; 'video' one path along the whole video, "
                         "across clip seams and the pooled windows of any --stride")
    ap.add_argument("--smooth-pose", type=int, default=None, nargs="?", const=13, metavar="R",
                    help="with --frames: score the pose smoothed along the frames within R (1 .. 64, default 13), every frame weighted "
                         "by the inverse covariance of its hypotheses; compare the mpjpe and accel columns")
    ap.add_argument("--smooth-pose-floor", type=float, default=1e-3, metavar="S",
                    help="with --smooth-pose: the standard deviation in metres added to every covariance (finite, > 0; default 0.001, "
                         "a regulariser, not a tuned value)")
    ap.add_argument("--bone-lengths", choices=("video", "symmetric"), default=None, nargs="?", const="video",
                    help="with --frames: score the pose with its bone lengths held constant along each video - one length per bone "
                         "from the whole video (symmetric: left and right pooled), every frame projected onto them under the covariance "
                         "of its hypotheses; compare the mpjpe and accel columns")
    ap.add_argument("--bone-iterations", type=int, default=16, metavar="K",
                    help="with --bone-lengths: Jacobi sweeps of the projection before the exact snap (0 .. 64; default 16, not a tuned value)")
    ap.add_argument("--ground", type=int, default=None, nargs="?", const=3, metavar="R",
                    help="with --frames --trajectory: find the ground plane of every video from its resting feet (a local line of radius "
                         "R frames, 1 .. 64, default 3) and log the angle between the estimated and the camera's true up, for the "
                         "prediction and for the ground-truth 3-D")
    ap.add_argument("--ground-speed", type=float, default=0.015, metavar="V",
                    help="with --ground: a foot point slower than V metres per FRAME counts as resting (default 0.015, not a tuned value)")
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args()
    if a.ground is not None and not (a.frames and a.trajectory is not None and 1 <= a.ground <= 64 and 0.0 < a.ground_speed < float("inf")):
        ap.error("--ground takes a radius in 1 .. 64, --ground-speed a finite speed > 0, and both need --frames --trajectory")
    if a.bone_lengths is not None and not (a.frames and 0 <= a.bone_iterations <= 64):
        ap.error("--bone-lengths takes --bone-iterations in 0 .. 64 and needs --frames")
    if a.smooth_pose is not None and not (a.frames and 1 <= a.smooth_pose <= 64):
        ap.error("--smooth-pose takes a radius in 1 .. 64 and needs --frames")
    if not 0.0 < a.smooth_pose_floor < float("inf"):
        ap.error("--smooth-pose-floor takes a finite length > 0 in metres")
    if a.path_scope == "video" and a.path_weight is None:
        ap.error("--path-scope video needs --path-weight")
    if a.path_weight is not None and not (a.frames and a.aggregate in ("reproj", "reproj_fit") and (a.stride is None or a.path_scope == "video")
                                          and a.hypothesis_chunk is None and 0.0 <= a.path_weight < float("inf")):
        ap.error("--path-weight takes a finite weight >= 0 and needs --frames --aggregate reproj or reproj_fit, without "
                 "--hypothesis-chunk and (unless --path-scope video) without --stride")
    drop = None
    if a.drop_detections is not None:
        try:
            fields = a.drop_detections.split(":")
            drop = (float(fields[0]), int(fields[1]), int(fields[2]) if len(fields) > 2 else 0)
            assert len(fields) <= 3 and 0.0 <= drop[0] <= 1.0 and drop[1] >= 1
        except (ValueError, IndexError, AssertionError):
            ap.error("--drop-detections takes RATE:RUN[:SEED], RATE in 0 .. 1 and RUN >= 1 frames")
    distract = None
    if a.distract_detections is not None:
        try:
            fields = a.distract_detections.split(":")
            distract = (int(fields[0]), int(fields[1]) if len(fields) > 1 else 0)
            assert len(fields) <= 2 and 1 <= distract[0] <= 63
        except (ValueError, IndexError, AssertionError):
            ap.error("--distract-detections takes PEOPLE[:SEED], PEOPLE in 1 .. 63")
    if (distract is not None or a.track) and not a.frames:
        ap.error("--distract-detections and --track need --frames")
    if a.track and distract is None:
        ap.error("--track needs --distract-detections (ground-truth 2-D holds one person)")
    corrupt = swap = None
    try:
        if a.corrupt_detections is not None:
            fields = a.corrupt_detections.split(":")
            corrupt = (float(fields[0]), int(fields[1]), float(fields[2]), int(fields[3]) if len(fields) > 3 else 0)
            assert len(fields) <= 4 and 0.0 <= corrupt[0] <= 1.0 and corrupt[1] >= 1 and 0.0 < corrupt[2] < float("inf")
        if a.swap_detections is not None:
            fields = a.swap_detections.split(":")
            swap = (float(fields[0]), int(fields[1]), int(fields[2]) if len(fields) > 2 else 0)
            assert len(fields) <= 3 and 0.0 <= swap[0] <= 1.0 and swap[1] >= 1
    except (ValueError, IndexError, AssertionError):
        ap.error("--corrupt-detections takes RATE:RUN:SIZE[:SEED] and --swap-detections RATE:RUN[:SEED], RATE in 0 .. 1, RUN >= 1 frames, SIZE > 0")
    planted = drop is not None or corrupt is not None or swap is not None
    if (planted or a.repair is not None or a.screen is not None) and not a.frames:
        ap.error("--drop-detections, --corrupt-detections, --swap-detections, --screen and --repair need --frames")
    if a.screen is not None and (not planted or not 1 <= a.screen <= 64):
        ap.error("--screen takes a radius in 1 .. 64 and needs a planting (ground-truth 2-D has nothing to screen)")
    if a.repair is not None and (not (drop is not None or a.screen is not None) or not 1 <= a.repair <= 64):
        ap.error("--repair takes a radius in 1 .. 64 and needs --drop-detections or --screen (ground-truth 2-D has nothing to repair)")
    if a.estimate_focal and not (a.frames and a.trajectory is not None):
        ap.error("--estimate-focal needs --frames --trajectory")
    args = config.load(a.config or None, a.overrides)
    world, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    ge.build()

    dataset = h3wb.Human3WBDataset(a.data)
    keypoints = h3wb.prepare_keypoints(dataset)
    kps_left, kps_right = (list(x) for x in dataset.keypoints_metadata["keypoints_symmetry"])
    joints_left, joints_right = list(dataset.skeleton().joints_left()), list(dataset.skeleton().joints_right())
    action_filter = None if args.data.actions == "*" else args.data.actions.split(",")
    cams, poses_3d, poses_2d = h3wb.fetch(args.data.subjects_test.split(","), keypoints, dataset,
                                          stride=args.experiment.downsample, action_filter=action_filter)

    model = pafuse_amd.D3DP(args, joints_left, joints_right, dataset=dataset, is_train=False,
                            num_proposals=args.ft2d.num_proposals, sampling_timesteps=args.ft2d.sampling_timesteps)
    print("INFO: Trainable parameter count:", sum(p.numel() for p in model.parameters()) / 1e6, "Million")
    if a.checkpoint:
        ckpt = harness.read_checkpoint(a.checkpoint)    # holds a pickled numpy RandomState: weights_only=False
        print("This model was trained for {} epochs".format(ckpt.get("epoch", "?")))
        harness.load_checkpoint(model, ckpt)
    model = model.to(f"cuda:{local}").eval()
    if a.noise == "device":
        model.noise, model.noise_seed = "device", a.seed
    torch.manual_seed(0)            # every rank draws the same full-P noise and keeps its hypothesis slice
    log = print if int(os.environ.get("RANK", "0")) == 0 else (lambda *x: None)
    log("Test time augmentation:", args.model.test_time_augmentation)
    if a.frames:
        h3wb.evaluate_frames(model, dataset, cams, poses_3d, poses_2d, kps_left, kps_right, aggregate=a.aggregate, stride=a.stride,
                             trajectory=None if a.trajectory is None else (a.trajectory or True), log=log,
                             hypothesis_chunk=a.hypothesis_chunk, p2=bool(args.ft2d.p2), seam_profile=a.seam_profile,
                             focal="estimate" if a.estimate_focal else None, repair=a.repair, drop=drop, path_weight=a.path_weight,
                             path_scope=a.path_scope, pose_smooth=a.smooth_pose, pose_smooth_floor=a.smooth_pose_floor,
                             bone_lengths=a.bone_lengths, bone_iterations=a.bone_iterations, corrupt=corrupt, swap=swap, screen=a.screen,
                             distract=distract, track=a.track, ground=a.ground, ground_speed=a.ground_speed,
                             orientations=None if a.ground is None else h3wb.fetch_orientations(
                                 args.data.subjects_test.split(","), keypoints, dataset, action_filter=action_filter))
    else:
        h3wb.evaluate(model, dataset, cams, poses_3d, poses_2d, kps_left, kps_right,
                      batch_size=args.model.batch_size, log=log, p2=bool(args.ft2d.p2),
                      gather=a.gather, hypothesis_chunk=a.hypothesis_chunk, p2_gather=a.p2_gather)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

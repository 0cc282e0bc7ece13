#!/usr/bin/env python3
"""In-the-wild 2D->3D lifting, the flow of the reference's in_the_wild/h3wb_diffusion.py:28-145 without the video and
rendering parts: OpenPifPaf whole-body JSON (one line per frame) -> screen-normalised keypoints -> flip-TTA DDIM
sampling on the HIP path with ``input_3d=None`` -> whole-body poses stitched back to the video's frames.

    python examples/infer_in_the_wild.py --keypoints video.openpifpaf.json --width 1920 --height 1080 \
           --data data/train_h3wb.npz --checkpoint checkpoint/pafuse_model.bin --out outputs/video \
           ft2d.num_proposals=20 ft2d.sampling_timesteps=10

Writes <out>/test_3d_output.npy [T,P,frames,134,3] (camera space) and <out>/test_3d_output_postprocess.npy (rotated
with the reference's fixed camera orientation, lowest point at height 0).  With --aggregate mean the hypotheses are
averaged on the device (P-Agg, the mean whole-body pose; --hypothesis-chunk n samples and reduces them n at a time, so
peak memory follows n instead of P) and both files hold [T,frames,134,3]: one pose per frame.  --spread std (with
--aggregate mean) also writes test_3d_output_std.npy [T,frames,134], per joint the RMS distance in metres of the P
hypotheses from that mean - the confidence of the joint; --spread cov writes test_3d_output_cov.npy [T,frames,134,6] as
well, their population covariance (xx, xy, xz, yy, yz, zz), camera space.  Without --keypoints a synthetic detection
file is generated (random weights unless --checkpoint: numbers are meaningless).

--reproj-fit FOCAL_PX adds J-Agg, the aggregate the method is known for, without a trajectory: per joint the hypothesis whose
2-D reprojection is closest to the detection, with the root position of every (hypothesis, frame) fitted on the device from
the detections, their confidences and a pinhole camera of that focal length in pixels (principal point at the image centre;
a per-frame fit, no smoothing over time).  It writes test_3d_output_pick.npy [T,frames,134,3] and test_3d_output_pick_idx.npy
[T,frames,134] (the hypothesis of every joint; -1: the detector did not find the joint and the pose holds the mean there)
next to what --aggregate asks for (the hypotheses are sampled again for that); --hypothesis-chunk and --spread (test_3d_output_pick_std.npy / _pick_cov.npy) go with it.

--stride S (1 .. the clip length; with --aggregate mean and / or --reproj-fit) slides the window over the video with that stride
instead of cutting consecutive clips, and pools on the device all windows that cover a frame: the same files, the per-frame arrays
written directly (no stitching), each frame aggregated over (windows covering it) x P hypotheses, plus test_3d_output_count.npy
[frames] and, with --reproj-fit, test_3d_output_pick_window.npy [T,frames,134].  Sampling costs about clip length / S times as much.

--trajectory FOCAL_PX (with --aggregate mean) puts the poses, which are root-relative, into camera space: the root of every (step,
frame) is fitted on the device on the mean pose from the detections, their confidences and a pinhole camera of that focal length
(the camera of --reproj-fit; a per-frame fit with a KNOWN focal length).  It writes test_3d_output_traj.npy [T,frames,3] (metres;
NaN where a frame has no fit) and test_3d_output_traj_resid.npy [T,frames] (the weighted residual of the fit in metres: large
values say the focal length is wrong), and test_3d_output_postprocess.npy is then built from poses + trajectory instead of a
rebased height.  --smooth-trajectory R (1 .. 64) also runs a confidence-weighted local-linear filter of radius R frames over the
trajectory (frames without a fit are filled from their neighbours): _traj.npy then holds the filtered roots and _traj_raw.npy
the per-frame fit.  With --stride the fit runs inside infer_sequence; without, on the stitched poses (harness.fit_trajectory).

--estimate-focal (with --aggregate mean) estimates the focal length from the video itself: one value for the whole video from the
mean poses and the detections (harness.estimate_focal; square pixels and the principal point at the image centre are assumed).  It
writes test_3d_output_focal.json: per step the focal length in pixels (f * width / 2), r2 - the fraction of the perspective signal
the estimate explains - and the number of frames it rests on.  --trajectory then needs no number: the root is fitted with the
estimate of the last step (a number given all the same is not read).  The estimate inherits a depth-scale error of the lifted pose
one for one, and a single frame or a distant person carries little signal - look at r2 and frames.  null in the file: no estimate,
and then the trajectory is NaN.

--repair [R] (default 13 frames; --repair-threshold C) repairs the detections on the device before anything else sees them
(harness.repair_detections): a keypoint the detector did not find - OpenPifPaf writes (0, 0, 0), which would enter the model as the
image corner - is filled along the frames from the frames within R in which it was found, a face keypoint relative to the nose and
a hand keypoint relative to its wrist; found keypoints are not touched, and a filled one keeps confidence 0, so the fits above go on
ignoring it.  It writes test_3d_output_repaired.npy [frames,134] (0 observed, 1 filled, 2 held, 3 unfilled) and prints the counts.

--screen [R] (default 13 frames; --screen-gate G, --screen-floor S) screens the FOUND keypoints first (harness.screen_detections): a
keypoint the detector reported wrongly with a confidence - a wrist found on a passer-by, a face point on the background - lies
far from the leave-one-out line through its neighbours within R frames; one farther than G robust scales of its joint gets
confidence 0, which --repair then fills and every fit ignores, and a left ankle and a right ankle that changed labels are
exchanged back.  It writes test_3d_output_screened.npy [frames,134] (0 accepted, 1 rejected, 2 swapped, 3 not found) and prints
the counts.  A fixed-radius linear model, not a tracker: a wrong person held for longer than about R frames is kept.  G = 4 and
S = 0.005 are defaults, not tuned values.

--path-weight L (with --reproj-fit) makes that pick coherent in time (infer_sequence(path_weight=...)): per clip and joint the path
through the hypotheses that minimises the reprojection error plus L times the distance the joint jumps relative to the mean pose,
instead of every frame's own winner.  It works per clip - the clip seams stay - and every joint written is still some hypothesis's.
--path-scope video runs that path along the whole video instead, across the clip seams and the pooled windows of --stride S: the
candidates of a frame are the hypotheses of all windows covering it (at most 256; they stay on the device for the whole video).  The
per-frame files of --stride are written, and test_3d_output_pick_path_cost.npy [steps,134], the cost of every joint's path (NaN: none).

--smooth-pose [R] (default 13 frames; --smooth-pose-floor S metres, default 0.001; with --aggregate mean, and with --reproj-fit
under --stride or --path-scope video) smooths the POSE VALUES along the frames on the device, per joint: a local-linear filter of
radius R in which every frame enters with the inverse covariance of its hypotheses as a matrix weight - a joint the hypotheses
disagree on along some direction is carried along that direction by its neighbours' line (harness.smooth_poses,
infer_sequence(pose_smooth=...)).  The files above then hold the smoothed pose - the trajectory is fitted on it - and
test_3d_output_raw.npy (_pick_raw.npy) what they held, test_3d_output_smooth_code.npy (_pick_smooth_code.npy) [T,frames,134] 1 line,
2 weighted mean, 3 nothing in reach.  The floor is a regulariser (a zero covariance stays solvable), not a tuned value.  A fixed-radius
linear smoother: no motion model, no bone lengths; what it buys on real weights has not been measured (evaluate_h3wb.py --frames
--smooth-pose measures it).

--bone-lengths [video|symmetric] (default video; --bone-iterations K, default 16; where --smooth-pose is allowed) holds the BONE
LENGTHS CONSTANT along the video on the device: one length per bone from the whole video - every frame weighing as far as its
hypotheses agree along the bone; "symmetric" pools left and right - and every frame moved onto those lengths by K Jacobi sweeps of
the covariance-weighted projection and an exact top-down snap (harness.constrain_bones, infer_sequence(bone_lengths=...)).  It runs
behind --smooth-pose and before the trajectory fit.  The files above then hold the constrained pose and test_3d_output_free.npy
(_pick_free.npy) what they held; test_3d_output_bone_length.npy, _bone_dev.npy [T,134] (metres; NaN: no bone - the root and the
face points), _bone_frames.npy, _bone_code.npy [T,frames,134] (1 moved with a bone, 0 untouched, 3 a bone was asked but the joint
had no finite pose or usable covariance) and _bone_resid.npy [T,frames,2] (the largest |length - L| of the frame before and after,
metres) come with it.  16 sweeps and the 1 mm floor are defaults, not tuned values; the estimated lengths are biased long where the
noise is comparable to the bone; what it buys on real weights has not been measured (evaluate_h3wb.py --frames --bone-lengths).

--track follows ONE PERSON through the video instead of taking entry 0 of every frame's "predictions" - OpenPifPaf lists the people
of a frame in no stable order, so with two people in view entry 0 is a splice of both.  All entries of every frame are linked
along the frames on the device (harness.load_pifpaf_people, harness.track_people; pafuse_amd/tracks.py states the arithmetic): a
link costs the distance the person moved in units of their own size, at most --track-gate (default 0.5), may jump --track-gap
frames (1 .. 8, default 4) at --track-skip (default 0.05) per frame jumped, and a track is the path with the largest summed gain.
--track lifts track 0, the best-scoring person; --track-seed FRAME:PERSON the person of that detection; --people M (1 .. 64) runs
everything above once per track, into <out>/person_<m>/.  A frame in which the person was not found enters as OpenPifPaf's own
"not found" - zeros with confidence 0, which --repair fills.  It writes test_3d_output_track.npy [M,frames] (the entry of
"predictions" followed, -1 nobody) and prints per track its frames, its score and the frames with nobody.  Without --track the
script does what it did.  What the tracker does NOT do: the cost is position only, no velocity term - identities can switch where
two people cross (on a planted video of 200 frames, 3 people and 6 slots shuffled every frame, a tenth of the detections dropped
and a ghost in a fifth of the frames, a numpy prototype had every frame right in 2 of 4 seeds and switches at the crossings in
the other two, 163 of 190 frames right in the worst track); extraction is greedy, one track after another, not a joint
assignment; a person gone for more than --track-gap - 1 frames comes back as a new track; at most 64 entries per frame; the gain
table takes frames * gap * K * K * 8 bytes; there is no appearance cue; the defaults are not tuned values; nobody has run it on
real video.

--ground [R] (with --trajectory; R the radius of the local line through every foot point, 1 .. 64 frames, default 3) finds WHICH WAY
IS UP from the video instead of rotating by CAMERA_ROTATION, the quaternion of the reference's demo camera: a toe or heel point that
moves slower than --ground-speed V metres per FRAME (default 0.015: the frame rate enters here) rests on the ground, and the ground
is the plane through those points, re-weighted three times, on the device behind the trajectory fit (harness.estimate_ground;
pafuse_amd/ground.py states the arithmetic).  It writes test_3d_output_world.npy [T,frames,134,3] and _world_traj.npy [T,frames,3]
(every step in the world of its own plane: z up, the ground at z = 0, x the camera's right levelled), _contact.npy [T,frames,6] (the
weight of every foot point as a contact) and _ground.json: per step the up direction in camera space, the camera's height, the rms
of the contacts about the plane, the three eigenvalues of their scatter, the number of contact points and the code - 1 a plane,
2 a line (a person standing: the plane through it closest to the body's own up), 3 the body's own up alone, 0 nothing (null).
test_3d_output_postprocess.npy is then the camera-space poses of every step in the world of the LAST step's plane.  Without
--ground the script does what it did.  What it does NOT do: one plane per video - no stairs, no changing slope, no moving camera; a
slow foot in the air counts as a contact until the re-weighting drops it; codes 2 and 3 lean on the lifted body's own up and
inherit its lean; the pose is rotated, not corrected (no foot locking: the contacts and heights are there for a caller to do it);
world x is the camera's right, not a direction of travel; the defaults are not tuned values; nobody has run it on real video.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
import pafuse_amd  # noqa: E402
from pafuse_amd import config, h3wb, harness  # noqa: E402

CAMERA_ROTATION = np.array([0.14070565, -0.15007018, -0.7552408, 0.62232804], dtype=np.float32)


def parse_seed(text):
    """FRAME:PERSON -> (frame, person), both integers >= 0; None if it is anything else"""
    parts = text.split(":")
    if len(parts) != 2 or not all(v.isdigit() for v in parts):
        return None
    return int(parts[0]), int(parts[1])


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--keypoints", default="")
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--height", type=int, default=1002)
    ap.add_argument("--data", default=os.path.join(ROOT, "tests", "golden", "h3wb_synth", "train_h3wb.npz"))
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "in_the_wild"))
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--noise", choices=("torch", "device"), default="torch",
                    help="where the loop's normals come from: torch.randn on the full tensor, or the library's counter-based "
                         "stream drawn inside the kernels (no noise tensor; other hypotheses than torch.randn's)")
    ap.add_argument("--seed", type=int, default=0, help="with --noise device: the seed of the stream, in [0, 2^32)")
    ap.add_argument("--aggregate", choices=("none", "mean"), default="none",
                    help="none: write all P hypotheses; mean: one pose per frame, the mean over the hypotheses, reduced on the "
                         "device (only the aggregate is copied to the host)")
    ap.add_argument("--hypothesis-chunk", type=int, default=None,
                    help="with --aggregate mean: sample and reduce the hypotheses this many at a time")
    ap.add_argument("--spread", choices=("std", "cov"), default=None,
                    help="with --aggregate mean: also write the per-joint spread of the hypotheses about the mean pose, reduced "
                         "on the device: std [T,frames,134] (metres), and for cov the covariance [T,frames,134,6] as well")
    ap.add_argument("--reproj-fit", type=float, default=None, metavar="FOCAL_PX",
                    help="also write J-Agg (test_3d_output_pick.npy, _pick_idx.npy): per joint the hypothesis whose reprojection is "
                         "closest to the detection, the root of every hypothesis fitted on the device from the detections, their "
                         "confidences and this focal length in pixels; --hypothesis-chunk and --spread go with it")
    ap.add_argument("--stride", type=int, default=None, metavar="S",
                    help="with --aggregate mean or --reproj-fit: slide the window over the video with this stride (1 .. clip length) "
                         "and pool the windows covering a frame on the device: one pose per video frame, no seam at the clip borders")
    ap.add_argument("--trajectory", type=float, default=None, nargs="?", const=0.0, metavar="FOCAL_PX",
                    help="with --aggregate mean: fit the camera-space root of every frame's pose on the device from the detections, "
                         "their confidences and this focal length in pixels; writes test_3d_output_traj.npy and _traj_resid.npy, "
                         "and the post-processed poses move with it (with --estimate-focal the number may be left out)")
    ap.add_argument("--smooth-trajectory", type=int, default=None, metavar="R",
                    help="with --trajectory: a confidence-weighted local-linear filter of radius R frames (1 .. 64) over the fitted "
                         "roots; the per-frame fit goes to test_3d_output_traj_raw.npy")
    ap.add_argument("--estimate-focal", action="store_true",
                    help="with --aggregate mean: estimate the focal length from the mean poses and the detections on the device and "
                         "write it, in pixels, with r2 and the frame count to test_3d_output_focal.json; --trajectory then fits "
                         "the root with the estimate and needs no number")
    ap.add_argument("--repair", type=int, default=None, nargs="?", const=13, metavar="R",
                    help="repair the detections on the device before lifting: a keypoint the detector did not find is filled along "
                         "the frames from the frames within R (1 .. 64, default 13) in which it was found, a face or hand keypoint "
                         "relative to the nose or its wrist; writes test_3d_output_repaired.npy [frames,134] (0 observed, 1 filled, "
                         "2 held, 3 unfilled) and prints the four counts")
    ap.add_argument("--repair-threshold", type=float, default=0.0, metavar="C",
                    help="with --repair or --screen: a keypoint counts as found if its confidence is above C (default 0)")
    ap.add_argument("--screen", type=int, default=None, nargs="?", const=13, metavar="R",
                    help="screen the found keypoints on the device before the repair: one farther from the leave-one-out line through "
                         "its neighbours within R frames (1 .. 64, default 13) than --screen-gate robust scales gets confidence 0, and a "
                         "left/right pair that fits exchanged is exchanged; writes test_3d_output_screened.npy [frames,134] (0 accepted, "
                         "1 rejected, 2 swapped, 3 not found) and prints the four counts")
    ap.add_argument("--screen-gate", type=float, default=4.0, metavar="G",
                    help="with --screen: the width of the gate in scales (finite, > 0; default 4, not a tuned value)")
    ap.add_argument("--screen-floor", type=float, default=0.005, metavar="S",
                    help="with --screen: the smallest scale in screen-normalised units (finite, > 0; default 0.005, not a tuned value)")
    ap.add_argument("--path-weight", type=float, default=None, metavar="L",
                    help="with --reproj-fit (no --stride, no --hypothesis-chunk): make the pick coherent in time - per clip and joint "
                         "one path through the hypotheses, a jump costing L per metre (normalised screen length per metre; about "
                         "2 * FOCAL_PX / width / depth makes a jump cost what it projects to; 0: the per-frame pick)")
    ap.add_argument("--path-scope", choices=("clip", "video"), default="clip",
                    help="with --path-weight: 'clip' (default) one path per clip; 'video' one path along the whole video, across clip "
                         "seams and the pooled windows of any --stride (per-frame output)")
    ap.add_argument("--smooth-pose", type=int, default=None, nargs="?", const=13, metavar="R",
                    help="smooth the pose along the frames on the device within R frames (1 .. 64, default 13), every frame weighted by "
                         "the inverse covariance of its hypotheses; the unsmoothed pose goes to test_3d_output_raw.npy")
    ap.add_argument("--smooth-pose-floor", type=float, default=1e-3, metavar="S",
                    help="with --smooth-pose: the standard deviation in metres added to every covariance (finite, > 0; default 0.001, "
                         "a regulariser, not a tuned value)")
    ap.add_argument("--bone-lengths", choices=("video", "symmetric"), default=None, nargs="?", const="video",
                    help="hold the bone lengths constant along the video on the device: one length per bone from the whole video "
                         "(symmetric: left and right pooled), every frame projected onto them under the covariance of its hypotheses; "
                         "the unconstrained pose goes to test_3d_output_free.npy")
    ap.add_argument("--bone-iterations", type=int, default=16, metavar="K",
                    help="with --bone-lengths: Jacobi sweeps of the projection before the exact snap (0 .. 64; default 16, not a tuned value)")
    ap.add_argument("--track", action="store_true",
                    help="follow one person through the video on the device instead of taking entry 0 of every frame's predictions: "
                         "lift track 0, the best-scoring person; writes test_3d_output_track.npy [M,frames]")
    ap.add_argument("--track-seed", default=None, metavar="FRAME:PERSON",
                    help="with --track: follow the person of that detection (entry PERSON of frame FRAME) instead of the best-scoring one")
    ap.add_argument("--people", type=int, default=None, metavar="M",
                    help="with --track: follow M people (1 .. 64), best first, and run everything once per track, into <out>/person_<m>/")
    ap.add_argument("--track-gate", type=float, default=0.5, metavar="C",
                    help="with --track: the farthest a person may move between linked frames, in units of their own size (finite, > 0; "
                         "default 0.5, not a tuned value)")
    ap.add_argument("--track-gap", type=int, default=4, metavar="G",
                    help="with --track: the longest link in frames (1 .. 8; default 4, not a tuned value)")
    ap.add_argument("--track-skip", type=float, default=0.05, metavar="C",
                    help="with --track: what every frame a link jumps over costs (finite, >= 0; default 0.05, not a tuned value)")
    ap.add_argument("--ground", type=int, default=None, nargs="?", const=3, metavar="R",
                    help="with --trajectory: find the ground plane from the foot points that rest (a local line of radius R frames, "
                         "1 .. 64, default 3), write world-space poses, contacts and test_3d_output_ground.json, and build the "
                         "post-processed poses from it instead of the demo camera's rotation")
    ap.add_argument("--ground-speed", type=float, default=0.015, metavar="V",
                    help="with --ground: a foot point slower than V metres per FRAME counts as resting (default 0.015, not a tuned value)")
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args(argv)
    if (a.track_seed is not None or a.people is not None) and not a.track:
        ap.error("--track-seed and --people need --track")
    if a.track_seed is not None and (parse_seed(a.track_seed) is None or a.people not in (None, 1)):
        ap.error("--track-seed takes FRAME:PERSON, two integers >= 0, and names one person (no --people above 1)")
    if a.people is not None and not 1 <= a.people <= 64:
        ap.error("--people takes 1 .. 64 people")
    if not (0.0 < a.track_gate < float("inf") and 0.0 <= a.track_skip < float("inf") and 1 <= a.track_gap <= 8):
        ap.error("--track-gate takes a finite value > 0, --track-skip a finite value >= 0 and --track-gap 1 .. 8 frames")
    if a.bone_lengths is not None and (not 0 <= a.bone_iterations <= 64 or not (
            a.aggregate == "mean" or (a.reproj_fit is not None and (a.stride is not None or a.path_scope == "video")))):
        ap.error("--bone-lengths takes --bone-iterations in 0 .. 64 and needs --aggregate mean, or --reproj-fit with --stride or "
                 "--path-scope video (one pose per video frame)")
    if a.smooth_pose is not None and (not 1 <= a.smooth_pose <= 64 or not (
            a.aggregate == "mean" or (a.reproj_fit is not None and (a.stride is not None or a.path_scope == "video")))):
        ap.error("--smooth-pose takes a radius in 1 .. 64 frames and needs --aggregate mean, or --reproj-fit with --stride or "
                 "--path-scope video (one pose per video frame)")
    if not 0.0 < a.smooth_pose_floor < float("inf"):
        ap.error("--smooth-pose-floor takes a finite length > 0 in metres")
    if a.path_scope == "video" and a.path_weight is None:
        ap.error("--path-scope video needs --path-weight")
    if a.path_weight is not None and (a.reproj_fit is None or (a.stride is not None and a.path_scope == "clip") or a.hypothesis_chunk is not None
                                      or not 0.0 <= a.path_weight < float("inf")):
        ap.error("--path-weight takes a finite weight >= 0 and needs --reproj-fit without --hypothesis-chunk and (unless --path-scope video) without --stride")
    if a.repair is not None and not 1 <= a.repair <= 64:
        ap.error("--repair takes a radius in 1 .. 64 frames")
    if not 0.0 <= a.repair_threshold < float("inf"):
        ap.error("--repair-threshold takes a finite confidence >= 0")
    if a.screen is not None and not 1 <= a.screen <= 64:
        ap.error("--screen takes a radius in 1 .. 64 frames")
    if not (0.0 < a.screen_gate < float("inf") and 0.0 < a.screen_floor < float("inf")):
        ap.error("--screen-gate and --screen-floor take finite values > 0")
    if a.estimate_focal and a.aggregate != "mean":
        ap.error("--estimate-focal needs --aggregate mean (one pose per frame)")
    if a.trajectory is not None and (a.aggregate != "mean" or not (a.trajectory > 0 or a.estimate_focal)):
        ap.error("--trajectory takes a positive focal length in pixels (or --estimate-focal) and needs --aggregate mean (one pose per frame)")
    if a.smooth_trajectory is not None and (a.trajectory is None or not 1 <= a.smooth_trajectory <= 64):
        ap.error("--smooth-trajectory takes a radius in 1 .. 64 and needs --trajectory")
    if a.ground is not None and (a.trajectory is None or not 1 <= a.ground <= 64 or not 0.0 < a.ground_speed < float("inf")):
        ap.error("--ground takes a radius in 1 .. 64 frames, --ground-speed a finite speed > 0 in metres per frame, and both need --trajectory")
    if a.stride is not None and a.aggregate == "none" and a.reproj_fit is None:
        ap.error("--stride needs --aggregate mean or --reproj-fit")
    if a.reproj_fit is not None and not a.reproj_fit > 0:
        ap.error("--reproj-fit takes a positive focal length in pixels")
    if a.spread is not None and a.aggregate == "none" and a.reproj_fit is None:
        ap.error("--spread needs --aggregate mean")
    if a.hypothesis_chunk is not None and a.aggregate == "none" and a.reproj_fit is None:
        ap.error("--hypothesis-chunk needs --aggregate mean")
    return a


def select_people(a, num_kps):
    """The detections the rest of the script lifts -> [(pixels [frames,num_kps,2], conf [frames,num_kps], output directory)]:
    entry 0 of every frame without --track (what the script always did), else one video per track; the track table is
    written and reported here."""
    if not a.track:
        pixels, conf = harness.load_pifpaf_keypoints(a.keypoints, num_kps, with_conf=True)
        return [(pixels, conf, a.out)]
    people, pconf = harness.load_pifpaf_people(a.keypoints, num_kps)
    seed = None if a.track_seed is None else parse_seed(a.track_seed)
    if seed is not None and not (seed[0] < people.shape[0] and seed[1] < people.shape[1]):
        raise SystemExit(f"--track-seed {a.track_seed}: the file has {people.shape[0]} frames and at most {people.shape[1]} people per frame")
    found = harness.track_people(people, pconf, tracks=a.people or 1, seed=seed, gate=a.track_gate, skip=a.track_skip, max_gap=a.track_gap)
    np.save(os.path.join(a.out, "test_3d_output_track.npy"), found["assign"].numpy(), allow_pickle=True)
    out = []
    for m in range(found["assign"].shape[0]):
        frames, score = int(found["frames"][m]), float(found["score"][m])
        print(f"track {m}: {frames} frames, score {score:.3f}, {people.shape[0] - frames} frames with nobody (entering as not found)")
        if frames == 0 and m > 0:
            continue                     # fewer people than asked for; track 0 is lifted whatever it holds
        where = a.out if a.people is None else os.path.join(a.out, f"person_{m}")
        os.makedirs(where, exist_ok=True)
        out.append((found["x2d"][m].numpy(), found["conf"][m].numpy(), where))
    return out


def main():
    a = parse_args()
    args = config.load(None, a.overrides)
    os.makedirs(a.out, exist_ok=True)
    ge.build()
    if not a.keypoints:
        a.keypoints = os.path.join(a.out, "synthetic.openpifpaf.json")
        rng = np.random.default_rng(0)
        with open(a.keypoints, "w") as f:
            for _ in range(70):
                flat = np.concatenate([rng.uniform(0, a.width, (133, 1)), rng.uniform(0, a.height, (133, 1)),
                                       np.ones((133, 1))], axis=1).reshape(-1)
                f.write(json.dumps({"predictions": [{"keypoints": flat.tolist()}]}) + "\n")

    dataset = h3wb.Human3WBDataset(a.data)
    kps_left, kps_right = (list(x) for x in dataset.keypoints_metadata["keypoints_symmetry"])
    model = pafuse_amd.D3DP(args, kps_left, kps_right, dataset=dataset, is_train=False,
                            num_proposals=args.ft2d.num_proposals, sampling_timesteps=args.ft2d.sampling_timesteps)
    if a.checkpoint:
        harness.load_checkpoint(model, harness.read_checkpoint(a.checkpoint))
    model = model.cuda().eval()
    if a.noise == "device":
        model.noise, model.noise_seed = "device", a.seed

    top = a.out
    for pixels, conf, where in select_people(a, args.data.num_kps):
        a.out = where
        lift(a, args, model, dataset, kps_left, kps_right, pixels, conf)
    a.out = top


def lift(a, args, model, dataset, kps_left, kps_right, pixels, conf):
    """one person's detections (pixels [frames,134,2], conf [frames,134]) -> the files of the docstring, in a.out"""
    chunk, spread = a.hypothesis_chunk, a.spread             # restored on the way out: the body narrows them for one person
    smoothing = {} if a.smooth_pose is None else dict(pose_smooth=a.smooth_pose, pose_smooth_floor=a.smooth_pose_floor)
    if a.bone_lengths is not None:       # behind the smoother, before the trajectory
        smoothing.update(bone_lengths=a.bone_lengths, bone_iterations=a.bone_iterations)
    BONE_FILES = (("bone_length", "bone_length"), ("bone_dev", "bone_dev"), ("bone_frames", "bone_frames"), ("bone_code", "bone_code"),
                  ("bone_resid", "bone_resid"))
    keypoints = h3wb.normalize_screen_coordinates(pixels[..., :2], w=a.width, h=a.height).astype(np.float32)
    save = lambda name, t: np.save(os.path.join(a.out, name), t.numpy(), allow_pickle=True)
    if a.screen is not None:             # once, up front and before the repair, as infer_sequence(screen=...) would
        screened = harness.screen_detections(keypoints, conf, kps_left=kps_left, kps_right=kps_right, radius=a.screen, gate=a.screen_gate,
                                             floor=a.screen_floor, threshold=a.repair_threshold)
        keypoints, conf = screened["x2d"].numpy(), screened["conf"].numpy()
        save("test_3d_output_screened.npy", screened["status"])
        print("detections accepted %d, rejected %d, swapped %d, not found %d (a rejected one keeps its coordinates and gets confidence 0: "
              "--repair fills it)" % tuple(screened["counts"].tolist()))
    if a.repair is not None:             # once, up front: every call below sees the repaired pair, as infer_sequence(repair=...) would
        fixed = harness.repair_detections(keypoints, conf, dataset=dataset, radius=a.repair, threshold=a.repair_threshold)
        keypoints, conf = fixed["x2d"].numpy(), fixed["conf"].numpy()
        save("test_3d_output_repaired.npy", fixed["status"])
        print("detections observed %d, filled %d, held %d, unfilled %d (unfilled ones enter the model as they are)" % tuple(fixed["counts"].tolist()))
    # screen-normalised coordinates: x in [-1, 1] over the width, the image centre at (0, 0), one scale for both axes
    pinhole = lambda focal: np.array([2 * focal / a.width, 2 * focal / a.width, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    traj = focal = None
    # the camera of the trajectory: the given focal length, or (cam=None) the estimate with square pixels and a centred principal point
    camera = dict(focal="estimate") if a.estimate_focal else dict(cam=None if a.trajectory is None else pinhole(a.trajectory))
    if a.reproj_fit is not None:
        cam = pinhole(a.reproj_fit)
        per_frame = a.stride is not None or a.path_scope == "video"
        pick = harness.infer_sequence(model, dataset, keypoints, kps_left, kps_right, batch_size=a.batch, aggregate="reproj_fit",
                                      cam=cam, conf=conf, hypothesis_chunk=a.hypothesis_chunk, spread=a.spread, stride=a.stride,
                                      path_weight=a.path_weight, path_scope=a.path_scope,
                                      **(smoothing if per_frame else {}))
        if per_frame:                    # per-frame arrays already
            for k, name in (("pose", "pick"), ("idx", "pick_idx"), ("window", "pick_window"), ("std", "pick_std"), ("cov", "pick_cov"),
                            ("path_cost", "pick_path_cost"), ("pose_raw", "pick_raw"), ("pose_smooth_code", "pick_smooth_code"),
                            ("pose_free", "pick_free")) + tuple((k, "pick_" + n) for k, n in BONE_FILES):
                if k in pick:
                    save(f"test_3d_output_{name}.npy", pick[k])
            save("test_3d_output_count.npy", pick["count"])
        elif a.spread is not None:
            for k in ("std", "cov")[:1 if a.spread == "std" else 2]:
                np.save(os.path.join(a.out, f"test_3d_output_pick_{k}.npy"),
                        harness.stitch_spread(pick[k], keypoints.shape[0], model.frames).numpy(), allow_pickle=True)
            pick = (pick["pose"], pick["idx"])
        if not per_frame:
            np.save(os.path.join(a.out, "test_3d_output_pick.npy"),
                    harness.stitch_poses(pick[0], keypoints.shape[0], model.frames).numpy(), allow_pickle=True)
            np.save(os.path.join(a.out, "test_3d_output_pick_idx.npy"),
                    harness.stitch_spread(pick[1], keypoints.shape[0], model.frames).numpy(), allow_pickle=True)
        if a.aggregate == "none":        # the chunk and the spread belonged to the pick
            a.hypothesis_chunk = a.spread = None
    if a.aggregate == "mean" and a.stride is not None:
        wanted = {} if a.trajectory is None else dict(conf=conf, trajectory=True if a.smooth_trajectory is None else a.smooth_trajectory,
                                                      **camera)
        if a.ground is not None:
            wanted.update(ground=a.ground, ground_speed=a.ground_speed)
        pred = harness.infer_sequence(model, dataset, keypoints, kps_left, kps_right, batch_size=a.batch, aggregate="mean",
                                      hypothesis_chunk=a.hypothesis_chunk, spread=a.spread, stride=a.stride, **wanted, **smoothing)
        for k, name in (("std", "std"), ("cov", "cov"), ("count", "count"), ("pose_raw", "raw"), ("pose_smooth_code", "smooth_code"),
                        ("pose_free", "free")) + BONE_FILES:
            if k in pred:
                save(f"test_3d_output_{name}.npy", pred[k])
        poses = pred["pose"]                                                        # [T,frames,134,3]
        traj = pred if a.trajectory is not None else None
    elif a.aggregate == "mean":
        pred = harness.infer_sequence(model, dataset, keypoints, kps_left, kps_right, batch_size=a.batch, aggregate="mean",
                                      hypothesis_chunk=a.hypothesis_chunk, spread="cov" if smoothing else a.spread)
        cov = None
        if isinstance(pred, dict):
            if smoothing:                    # consecutive clips: the filters run on the stitched per-frame arrays
                cov = harness.stitch_spread(pred["cov"], keypoints.shape[0], model.frames)
            for k in ("std", "cov")[:0 if a.spread is None else 1 if a.spread == "std" else 2]:
                np.save(os.path.join(a.out, f"test_3d_output_{k}.npy"),
                        harness.stitch_spread(pred[k], keypoints.shape[0], model.frames).numpy(), allow_pickle=True)
            pred = pred["pose"]
        poses = harness.stitch_poses(pred, keypoints.shape[0], model.frames)        # [T,frames,134,3]
        if a.smooth_pose is not None:        # before the trajectory: the root is fitted on the smoothed pose
            smoothed = harness.smooth_poses(poses, cov, radius=a.smooth_pose, floor=a.smooth_pose_floor)
            save("test_3d_output_raw.npy", smoothed["pose_raw"])
            save("test_3d_output_smooth_code.npy", smoothed["pose_smooth_code"])
            poses = smoothed["pose"]
        if a.bone_lengths is not None:       # behind the smoother, before the trajectory
            held = harness.constrain_bones(poses, cov, tables=h3wb.bone_tables(dataset, True, kps_left, kps_right), lengths=a.bone_lengths,
                                           iterations=a.bone_iterations)
            for k, name in (("pose_free", "free"),) + BONE_FILES:
                save(f"test_3d_output_{name}.npy", held[k])
            poses = held["pose"]
        if a.trajectory is not None:     # consecutive clips: the fit runs on the stitched per-frame array
            traj = harness.fit_trajectory(poses, keypoints, conf=conf, smooth=a.smooth_trajectory, **camera)
    else:
        pred = harness.infer_sequence(model, dataset, keypoints, kps_left, kps_right, batch_size=a.batch)
        poses = harness.stitch_clips(pred, keypoints.shape[0], model.frames)        # [T,P,frames,134,3]
    np.save(os.path.join(a.out, "test_3d_output.npy"), poses.numpy(), allow_pickle=True)
    if a.estimate_focal:                 # from the fit where there was one, else on the per-frame poses alone
        focal = traj if traj is not None else harness.estimate_focal(poses, keypoints, conf=conf)
        number = lambda v: None if v != v else v                                    # NaN (no estimate) -> null
        with open(os.path.join(a.out, "test_3d_output_focal.json"), "w") as f:
            json.dump({"width": a.width, "height": a.height,
                       "focal_px": [number(float(v) * a.width / 2) for v in focal["focal"]],
                       "r2": [number(float(v)) for v in focal["focal_r2"]],
                       "frames": [int(v) for v in focal["focal_frames"]]}, f, indent=1)
        print("estimated focal length per step, pixels:", [None if v != v else round(float(v) * a.width / 2, 1) for v in focal["focal"]])
    if traj is not None:
        for k in ("traj", "traj_raw", "traj_resid"):
            if k in traj:
                save(f"test_3d_output_{k}.npy", traj[k])
    if traj is not None and a.ground is not None:
        # inside infer_sequence where it ran (--stride), else on the stitched poses and their fitted roots
        found = traj if "ground_code" in traj else harness.estimate_ground(poses, traj["traj"], radius=a.ground, speed=a.ground_speed)
        for k, name in (("pose_world", "world"), ("traj_world", "world_traj"), ("contact", "contact")):
            save(f"test_3d_output_{name}.npy", found[k])
        number = lambda v: None if v != v else v                                    # NaN (code 0: no plane) -> null
        with open(os.path.join(a.out, "test_3d_output_ground.json"), "w") as f:
            json.dump({"radius": a.ground, "speed_m_per_frame": a.ground_speed,
                       "up": [[number(float(c)) for c in v] for v in found["up"]],
                       "camera_height_m": [number(float(v)) for v in found["camera_height"]],
                       "rms_m": [number(float(v)) for v in found["ground_rms"]],
                       "eigenvalues_m2": [[number(float(c)) for c in v] for v in found["ground_eig"]],
                       "points": [int(v) for v in found["ground_points"]],
                       "code": [int(v) for v in found["ground_code"]]}, f, indent=1)
        print("ground per step: code", [int(v) for v in found["ground_code"]], "camera height, m:",
              [None if v != v else round(float(v), 3) for v in found["camera_height"]])
        # one world for the post-processed file: every step's camera-space poses under the plane of the last, fully denoised step
        world = harness.frames_to_world(poses, traj["traj"], found["ground_plane"][-1])["pose_world"]
    elif traj is not None:
        world = harness.camera_to_world(poses + traj["traj"][:, :, None], CAMERA_ROTATION)   # a broadcast add: camera-space poses
    else:
        world = harness.camera_to_world(poses, CAMERA_ROTATION)
        world[..., 2] -= world[..., 2].min()                                        # no trajectory: rebase the height
    np.save(os.path.join(a.out, "test_3d_output_postprocess.npy"), world.numpy(), allow_pickle=True)
    print(f"{keypoints.shape[0]} frames -> poses {tuple(poses.shape)} in {a.out}")
    a.hypothesis_chunk, a.spread = chunk, spread


if __name__ == "__main__":
    main()

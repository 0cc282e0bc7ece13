"""Caller side of the hot path: what the reference's evaluate() does around ``model_eval(...)`` for one sequence
(main_h3wb.py:261-379) - flip copy, cutting into 27-frame clips, part centring, batched sampling, the 14
accumulators - with tensors kept on the HIP device.  SURVEY.md section 8f rows n1/n3 (partial: no dataset files
or Hydra here; the caller hands in arrays).
"""
import dataclasses
import math
from typing import NamedTuple

import torch

from .evaluate import (accumulate_frames, accumulate_partials, accumulate_poses, accumulate_spread, aggregate_poses_sharded,
                       evaluate_accumulators, evaluate_accumulators_sharded)
from .parallel import ShardedSampler

ACCUMULATORS = ("j_best", "p_best", "p_agg", "j_agg", "p_best_pb", "p_best_pb_body", "p_best_pb_face",
                "p_best_pb_left_hand", "p_best_pb_right_hand", "p_agg_pb", "p_agg_pb_body", "p_agg_pb_face",
                "p_agg_pb_left_hand", "p_agg_pb_right_hand")
ACCUMULATORS_P2 = ACCUMULATORS + ("p2_j_best", "p2_p_best", "p2_p_agg", "p2_j_agg")   # with ft2d.p2 (main_h3wb.py:225-228)


def flip_2d(inputs_2d, kps_left, kps_right):
    """Test-time-augmentation copy of the 2-D input: negate x, swap left/right joints (main_h3wb.py:268-270)."""
    out = inputs_2d.clone()
    out[..., 0] *= -1
    out[..., list(kps_left) + list(kps_right), :] = out[..., list(kps_right) + list(kps_left), :]
    return out


def cut_clips(seq, frames=27):
    """[N, J, c] (or [1, N, J, c]) -> [ceil(N/frames), frames, J, c]: consecutive clips, the last one holding the LAST
    `frames` frames (so it overlaps its predecessor), sequences shorter than a clip padded by repeating the final
    frame (eval_data_prepare, main_h3wb.py:122-154)."""
    if seq.dim() == 4:
        seq = seq.squeeze(0)
    n = seq.shape[0]
    if n < frames:
        seq = torch.cat([seq, seq[-1:].expand(frames - n, *seq.shape[1:])], dim=0)
        n = frames
    full = n // frames
    clips = [seq[i * frames:(i + 1) * frames] for i in range(full - (1 if n % frames == 0 else 0))]
    clips.append(seq[-frames:])
    return torch.stack(clips)


def center_pose_parts(pose, dataset):
    """Every part translated so that its own root joint is the origin (common/utils.py:97-112)."""
    out = torch.zeros_like(pose)
    for part, idx in dataset.parts_joint_indices.items():
        root = dataset.root_indices[part]
        out[..., idx, :] = pose[..., idx, :] - pose[..., root:root + 1, :]
    return out


def wb_pose_from_parts(pose, dataset):
    """Whole-body pose from part-centred poses: every joint shifted by its part's connection joint (face -> body
    joint 1, hands -> 10 / 11, body -> 0, which pins joint 0 at the origin).  Closed form of the reference's
    in-place pass (common/utils.py:113-126) - same values bit for bit, and the input is left untouched."""
    conn = dict(dataset.parts_connection_indices)
    conn["body"] = 0
    out = torch.zeros_like(pose)
    for part, idx in dataset.parts_joint_indices.items():
        if part in conn:
            out[..., idx, :] = pose[..., idx, :] + pose[..., conn[part]:conn[part] + 1, :]
    out[..., 0, :] = 0
    return out


# ------------------------------------------------------- the operand checks the stand-alone wrappers and the chain share
def _poses_operand(poses, other=None, named=None, dims=slice(0, 2), tail=(3,), empty_ok=False):
    """poses [T,N,J,3] -> fp32; with `other` its companion, refused as `named`, of shape poses.shape[dims] + tail -> the pair"""
    poses = torch.as_tensor(poses, dtype=torch.float32)
    bad = poses.dim() != 4 or poses.shape[-1] != 3 or (not empty_ok and 0 in poses.shape)
    if named is None:
        if bad:
            raise ValueError(f"poses must be [T,N,J,3], got {tuple(poses.shape)}")
        return poses
    other = torch.as_tensor(other, dtype=torch.float32)
    if bad or tuple(other.shape) != (*poses.shape[dims], *tail):
        raise ValueError(f"poses must be [T,N,J,3] and {named}, got {tuple(poses.shape)} and {tuple(other.shape)}")
    return poses, other


def _cov_operand(cov, poses):
    """cov [T,N,J,6] beside poses [T,N,J,3], or None -> fp32 or None"""
    if cov is None:
        return None
    cov = torch.as_tensor(cov, dtype=torch.float32)
    if tuple(cov.shape) != (*poses.shape[:3], 6):
        raise ValueError(f"cov must be [T,N,J,6] = {(*poses.shape[:3], 6)}, got {tuple(cov.shape)}")
    return cov


def _conf_operand(conf, shape):
    """conf [N,J] = `shape`, or None -> fp32 or None"""
    if conf is None:
        return None
    conf = torch.as_tensor(conf, dtype=torch.float32)
    if tuple(conf.shape) != tuple(shape):
        raise ValueError(f"conf must be [N,J] = {tuple(shape)}, got {tuple(conf.shape)}")
    return conf


def _detections_pair(seq_2d, conf):
    """seq_2d [N,J,2] and conf [N,J] -> the fp32 pair"""
    seq_2d = torch.as_tensor(seq_2d, dtype=torch.float32)
    conf = torch.as_tensor(conf, dtype=torch.float32)
    if seq_2d.dim() != 3 or seq_2d.shape[-1] != 2 or tuple(conf.shape) != tuple(seq_2d.shape[:2]):
        raise ValueError(f"seq_2d must be [N,J,2] and conf [N,J], got {tuple(seq_2d.shape)} and {tuple(conf.shape)}")
    return seq_2d, conf


def _run_on(operand, device, run):
    """run(dev) on the operand's own device when it is on one, else on `device`; its dict of device tensors -> CPU tensors"""
    dev = operand.device if operand.is_cuda else torch.device(device)
    return {k: v.cpu() for k, v in run(dev).items()}


def _repair_radius(repair, threshold=0.0, name="repair"):
    """infer_sequence's `repair` and `repair_threshold`: None -> None, an integer r in 1 .. 64 -> r; the threshold finite and >= 0"""
    if repair is None:
        return None
    if isinstance(repair, bool) or not isinstance(repair, int) or not 1 <= repair <= 64:
        raise ValueError(f"{name} must be None or a radius in 1 .. 64 (frames), got {repair!r}")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= float(threshold) < float("inf"):
        raise ValueError(f"{name}_threshold must be a finite confidence >= 0, got {threshold!r}")
    return repair


def _repair_detections(seq_2d, conf, dev, **options):
    """CPU or device tensors seq_2d [N,J,2], conf [N,J] -> ops.repair_detections' dict on the device; options: its anchor, radius
    and threshold"""
    from . import ops
    return ops.repair_detections(seq_2d.to(dev).contiguous(), conf.to(dev).contiguous(), **options)


@torch.no_grad()
def repair_detections(seq_2d, conf, dataset=None, anchor=None, radius=13, threshold=0.0, device="cuda"):
    """Missing 2-D detections repaired on the device before lifting (pafuse_amd.detections; ops.repair_detections): ``seq_2d``
    [N,J,2] screen-normalised detections, ``conf`` [N,J] their confidences (:func:`load_pifpaf_keypoints` with
    ``with_conf=True``).  A joint whose confidence is not > ``threshold`` (OpenPifPaf's "not found" writes (0, 0, 0)), or whose
    coordinates are not finite, is filled along the frames from the frames within ``radius`` in which it was seen, by the
    confidence-weighted local-linear filter of :func:`fit_trajectory`'s smoother; seen joints keep their bits.  ``dataset``
    gives the anchor table detections.repair_anchors(dataset): a face joint is filled relative to the nose and a hand joint
    relative to its wrist, so a hand lost for a few frames moves with the arm.  ``anchor`` [J] overrides it; with both None no
    joint hangs on another.  Returns a dict of CPU tensors: ``"x2d"`` [N,J,2], ``"conf"`` [N,J] (0 at every joint that was
    not seen: a filled joint carries no measurement), ``"status"`` [N,J] uint8 (0 observed, 1 filled, 2 held from a single
    neighbour, 3 unfilled: nothing within the radius, the input as it was) and ``"counts"`` [4] int64, the joints per status."""
    from .detections import repair_anchors
    radius = _repair_radius(radius, threshold, "radius")
    if radius is None:
        raise ValueError("radius must be a radius in 1 .. 64 (frames), got None")
    seq_2d, conf = _detections_pair(seq_2d, conf)
    if anchor is None and dataset is not None:
        anchor = repair_anchors(dataset)
    out = _run_on(seq_2d, device, lambda dev: _repair_detections(seq_2d, conf, dev, anchor=anchor, radius=radius, threshold=float(threshold)))
    out["counts"] = torch.bincount(out["status"].reshape(-1).long(), minlength=4)
    return out


def _screen_radius(screen, gate=4.0, floor=0.005, name="screen"):
    """infer_sequence's `screen`, `screen_gate` and `screen_floor`: None -> None, an integer r in 1 .. 64 -> r; gate and floor
    finite and > 0"""
    if screen is None:
        return None
    if isinstance(screen, bool) or not isinstance(screen, int) or not 1 <= screen <= 64:
        raise ValueError(f"{name} must be None or a radius in 1 .. 64 (frames), got {screen!r}")
    for key, v in (("gate", gate), ("floor", floor)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < float("inf"):
            raise ValueError(f"{name}_{key} must be finite and > 0, got {v!r}")
    return screen


def _screen_detections(seq_2d, conf, dev, **options):
    """CPU or device tensors seq_2d [N,J,2], conf [N,J] -> ops.screen_detections' dict on the device; options: its mirror, radius,
    gate, floor, passes, support and threshold"""
    from . import ops
    return ops.screen_detections(seq_2d.to(dev).contiguous(), conf.to(dev).contiguous(), **options)


@torch.no_grad()
def screen_detections(seq_2d, conf, kps_left=None, kps_right=None, mirror=None, radius=13, gate=4.0, floor=0.005, passes=3,
                      support=3, threshold=0.0, device="cuda"):
    """Observed 2-D detections screened on the device, in front of :func:`repair_detections` (pafuse_amd.detscreen;
    ops.screen_detections): ``seq_2d`` [N,J,2] screen-normalised detections, ``conf`` [N,J] their confidences.  Per joint and
    along the frames, every observed detection is compared with the leave-one-out local line through its accepted neighbours
    within ``radius``; one farther from it than ``gate`` robust scales (1.4826 times the median residual of the joint, at least
    ``floor``) is REJECTED - it leaves with confidence 0, so the repair fills it and every fit ignores it.  All frames are
    re-tested over ``passes`` passes, which re-admits the neighbours of a gross outlier.  ``kps_left`` / ``kps_right`` (paired by
    position) or ``mirror`` [J] name the mirror pairs: where one of a pair is rejected and EXCHANGING the two puts both within
    their gates, the pair leaves exchanged, confidences included - a left/right swap undone.  Returns a dict of CPU tensors:
    ``"x2d"`` [N,J,2], ``"conf"`` [N,J], ``"status"`` [N,J] uint8 (0 accepted, 1 rejected, 2 swapped, 3 not observed),
    ``"resid"`` [N,J], ``"scale"`` [J] and ``"counts"`` [4] int64, the detections per status.  gate, floor, passes and support
    are defaults, not tuned values.  A fixed-radius linear model, not a tracker: a swap or a wrong person held for longer than
    about ``radius`` frames becomes the track and is kept."""
    from .detscreen import mirror_table
    radius = _screen_radius(radius, gate, floor, "radius")
    if radius is None:
        raise ValueError("radius must be a radius in 1 .. 64 (frames), got None")
    seq_2d, conf = _detections_pair(seq_2d, conf)
    if mirror is None and kps_left is not None and kps_right is not None:
        mirror = mirror_table(kps_left, kps_right, seq_2d.shape[1])
    out = _run_on(seq_2d, device, lambda dev: _screen_detections(seq_2d, conf, dev, mirror=mirror, radius=radius, gate=float(gate), floor=float(floor),
                                                                 passes=passes, support=support, threshold=float(threshold)))
    out["counts"] = torch.bincount(out["status"].reshape(-1).long(), minlength=4)
    return out


@torch.no_grad()
def infer_sequence(model, dataset, seq_2d, kps_left, kps_right, batch_size=2, group=None, aggregate=None, cam=None, traj=None,
                   hypothesis_chunk=None, spread=None, conf=None, stride=None, trajectory=None, focal=None, repair=None,
                   repair_threshold=0.0, path_weight=None, path_scope="clip", pose_smooth=None, pose_smooth_floor=1e-3,
                   bone_lengths=None, bone_iterations=16, screen=None, screen_gate=4.0, screen_floor=0.005, ground=None,
                   ground_speed=0.015, ground_passes=3, ground_gate=2.5, ground_floor=0.005, ground_spread=0.03, ground_points=None):
    """In-the-wild inference for one 2-D keypoint sequence [N,J,2] (already screen-normalised): flip copy, 27-frame
    clips, batched sampling with ``input_3d=None``, whole-body poses (in_the_wild/utils.py:322-376).
    Returns a CPU tensor [clips, T, P, F, J, 3].  The model is taken as it is configured (``model.noise``, ``model.noise_seed``).

    ``aggregate`` asks for ONE pose per frame instead of all P hypotheses, reduced on the device (evaluate.accumulate_poses /
    aggregate_poses_sharded): every rank samples its hypotheses, ``hypothesis_chunk`` at a time when given, folds each chunk
    into a 44-byte-per-(clip,t,f,j) state and drops it; the ranks exchange states, and only the aggregate crosses to the host.
    ``"mean"`` (P-Agg): a CPU tensor [clips, T, F, J, 3], the mean whole-body pose.  ``"reproj"`` (J-Agg):
    ``(pose [clips,T,F,J,3], idx [clips,T,F,J])``, per joint the hypothesis whose 2-D reprojection is closest to the input
    and its index (NaN / -1 where no reprojection error is finite); it needs ``cam`` [9] intrinsics and ``traj`` [N,3], the
    root position of every frame (cut into clips like the 2-D input).

    ``"reproj_fit"`` is J-Agg WITHOUT a trajectory, for videos of one's own: it needs ``cam`` [9] and refuses a ``traj`` - the
    root of every (hypothesis, frame) is fitted on the device from the un-flipped 2-D input and the intrinsics
    (pafuse_amd.rootfit: a per-frame linear fit with a known focal length, no smoothing over time).  ``conf`` [N,J] weighs
    the detections (None: all 1; a weight that is not > 0 - OpenPifPaf's "not found" - takes the joint out of the fit and
    out of the pick); it is cut into clips like the 2-D input.  It returns ``(pose, idx)`` as "reproj" does, except that a
    joint without a pick (idx -1: no weight, or no hypothesis of its frame could be fitted) holds the MEAN of the
    hypotheses instead of NaN.  The fitted roots themselves are not returned (evaluate.accumulate_poses(tfit=...) has them).

    ``spread`` (with an ``aggregate``) also returns how much the hypotheses disagree per joint, reduced on the device by the
    same scheme (evaluate.accumulate_spread, 72 bytes per (clip,t,f,j)).  The return value is then a dict of CPU tensors:
    ``"pose"`` as above, ``"idx"`` for "reproj", ``"std"`` [clips,T,F,J] - the RMS distance in metres of the P whole-body
    hypotheses from their mean joint - and, for ``spread="cov"``, ``"cov"`` [clips,T,F,J,6], their population covariance
    (xx, xy, xz, yy, yz, zz).  With "mean" only the spread state is kept (it holds the sums: the pose is the same, bit
    for bit); with "reproj" every chunk is folded into both states.  Both are taken about the MEAN pose.

    ``stride`` (with an ``aggregate``; None: everything above, unchanged) slides the F-frame window over the video with that
    stride, 1 .. F (pafuse_amd.windows.window_starts: starts 0, s, 2s, ... and a last window at N - F), and pools the windows
    on the device into ONE pose per video frame: a frame covered by m windows is aggregated over its m x P hypotheses - the
    mean over all of them, the J-Agg pick the first minimum in (window, hypothesis) order, the spread about the pooled mean
    (evaluate.accumulate_frames, behind the cross-rank combine; 48 + 72 bytes per (t,frame,j) stay on the device however many
    windows there are).  Sampling costs about F / stride times as much.  The return value is a dict of CPU tensors:
    ``"pose"`` [T,N,J,3], ``"count"`` [N] (the hypotheses pooled per frame), for the reprojection aggregates ``"idx"`` and
    ``"window"`` [T,N,J] (the pick's hypothesis and its window; -1 without one), with ``spread`` ``"std"`` [T,N,J] and
    ``"cov"`` [T,N,J,6].  traj and conf are cut per window; with "reproj_fit" a joint without a pick carries the pooled mean.
    stride = F visits exactly the clips of cut_clips.

    ``trajectory`` (with ``stride``; None: everything above, unchanged) also returns the camera-space ROOT of the pose that is
    returned - every pose above is root-relative.  It needs ``cam`` (fx, fy, cx, cy first) and takes ``conf`` [N,J] with any
    aggregate.  The root of every (t, frame) is fitted on the device on the finished pose (the pooled mean, or the pick with the
    mean already filled in where idx == -1) from the detections and the intrinsics - pafuse_amd.trajectory: the per-frame linear
    fit of "reproj_fit" with a KNOWN focal length; a joint without a weight or with a NaN pose takes no part.  ``True``: the
    per-frame fit as it is.  An integer r in 1 .. 64: also a confidence-weighted local-linear filter of radius r along the
    frames (weights: the fit's summed weights), which fills frames without a fit from their neighbours.  Added keys:
    ``"traj"`` [T,N,3] (smoothed when r is given; NaN where there is no fit and nothing to fill from), ``"traj_raw"`` [T,N,3]
    when smoothed, ``"traj_weight"`` [T,N] (0: no fit) and ``"traj_resid"`` [T,N], the weighted residual of the fit in metres
    (it is what a wrong focal length shows in).  Camera-space poses are ``pose + traj[:, :, None]``.  Every rank holds the same
    frame state and runs the same fit.  Without ``stride`` use :func:`fit_trajectory` on the stitched poses.

    ``focal="estimate"`` (with ``trajectory``; None: everything above, unchanged) estimates the focal length the fit needs from
    the video itself - :func:`estimate_focal` on the pose that is returned - and fits the root with it: ``cam`` becomes optional
    (None: square pixels, the principal point at the image centre; given: its principal point, aspect and distortion terms are
    kept and its focal length is not read).  The fit runs with the estimate of the last, fully denoised step, ``"cam"[T-1]``,
    read on the device.  Added keys: ``"focal"`` [T], ``"focal_r2"`` [T], ``"focal_frames"`` [T] and ``"cam"`` [T,9].  A video
    without an estimate (NaN) has a NaN trajectory, not a guessed one.

    ``repair`` (None: everything above, unchanged, bit for bit) repairs the detections on the device BEFORE anything else sees
    them - :func:`repair_detections` with the anchors of ``dataset``, that radius (1 .. 64 frames) and ``repair_threshold``.  It
    needs ``conf`` [N,J], which is then accepted with every ``aggregate``, None included.  ``seq_2d`` and ``conf`` are replaced by
    the repaired pair before the flip copy and the cutting: the denoisers, the flip copy, the root fits, the focal estimate and
    the pick all see the same filled detections, and the zeroed confidences keep the filled joints out of every fit.  Results
    that are dicts gain ``"repaired"`` [N,J] uint8, the status of every joint (0 observed, 1 filled, 2 held, 3 unfilled);
    tensor and tuple results keep their type.

    ``screen`` (a radius 1 .. 64; None: everything above, unchanged, bit for bit) SCREENS THE OBSERVED DETECTIONS on the device
    before even the repair - :func:`screen_detections` with the mirror pairs of ``kps_left`` / ``kps_right``, that radius,
    ``screen_gate`` and ``screen_floor`` (defaults, not tuned values) and ``repair_threshold``.  It runs on the un-flipped input and
    needs ``conf`` [N,J], which is then accepted with every ``aggregate``.  An outlier leaves with confidence 0 - the repair
    fills it, the fits ignore it - and a left/right swap leaves exchanged; the repair, the flip copy and everything behind
    them see the screened pair.  Results that are dicts gain ``"screened"`` [N,J] uint8 (0 accepted, 1 rejected, 2 swapped, 3
    not observed); tensor and tuple results keep their type.  Without ``repair`` a rejected detection keeps its wrong
    coordinates in front of the denoisers: only the fits are protected.  A fixed-radius linear model with one scale per joint
    per video, no anchor levels, not a tracker; what it buys on real video has NOT been measured.

    ``path_weight`` (with "reproj" or "reproj_fit"; None: everything above, unchanged, bit for bit) makes the pick COHERENT IN
    TIME: per joint and clip, instead of the closest reprojection of every frame on its own, the path through the P hypotheses
    that minimises the reprojection error plus ``path_weight`` times the distance the joint jumps relative to the mean pose
    (evaluate.path_poses, pafuse_amd.posepath: a Viterbi recursion on the device).  The weight is in normalised screen length
    per metre - cam[0] / depth is the weight at which a jump costs as much as its own projection; 0.0 returns the per-frame
    pick.  The return types are those above.  A joint unobserved in a frame (with "reproj_fit": a confidence not > 0) is carried
    through by smoothness alone and still gets a pick; with "reproj_fit" a joint without a path (idx -1) carries the mean.  The
    recursion needs all P hypotheses of a clip at once, so ``hypothesis_chunk`` is refused and, under a process group, the
    hypotheses are gathered as ``aggregate=None`` gathers them; ``stride`` may only be None or F - a path lives inside one clip
    and crosses neither clip seams nor pooled windows.  It is not a smoother of the pose values: every returned joint is still
    some hypothesis's joint.

    ``path_scope="video"`` (with ``path_weight``; the default "clip" is everything above, refusals included) runs that
    recursion along the N frames of the VIDEO instead (evaluate.path_frames, pafuse_amd.posepath.frames_path): at every frame
    the candidates are all P hypotheses of ALL windows that cover it, so the path crosses clip seams and pooled windows.  Any
    ``stride`` is accepted (None means F) and the result is the per-frame dict of ``stride=`` plus ``"path_cost"`` [T,J]
    (float64; NaN: no path).  The windows are sampled in batches and their pose and spread states folded as without a path
    weight - ``count``, ``std`` / ``cov`` and the trajectory keys do not change - but the hypotheses of ALL windows are kept
    on the device until the end of the video: W*T*P*F*J*3*4 bytes for W windows, plus the path kernel's workspace of one
    byte per (t, j, frame, candidate) - memory grows with the length of the video.  ``pose``, ``idx`` and ``window`` come
    from the path; with "reproj_fit" a joint with idx -1 carries the pooled mean.  A joint's path dies whole: one frame at
    which none of its candidates is finite removes it for the video.  Refused: ``hypothesis_chunk``, ``aggregate`` None /
    "mean", and more than 256 candidates per frame (P times the windows that cover one frame).  Under a process group the
    hypotheses are gathered as ``aggregate=None`` gathers them.

    ``pose_smooth`` (a radius r in 1 .. 64, with ``stride`` and an ``aggregate``; None: everything above, unchanged, bit for bit)
    SMOOTHS THE POSE VALUES along the frames, per joint, on the device (:func:`smooth_poses`; pafuse_amd.posesmooth states the
    arithmetic): a local-linear filter of radius r in which every frame enters with the matrix weight (cov + floor^2 I)^-1, cov
    the covariance of the hypotheses pooled at that (t, frame, joint) - a frame is trusted in each direction as far as its
    hypotheses agree in that direction and is otherwise carried by its neighbours' line.  The spread state is folded for it
    even when ``spread`` is None; ``"std"`` / ``"cov"`` appear only when ``spread`` asks for them and are unchanged: they
    describe the hypotheses (about the pooled mean, also when the pick is what gets smoothed), not the smoothed pose.  The
    filter runs right behind the finish (or the video path) on the pose that is returned - with "reproj_fit" the mean already
    filled in where idx is -1 - and EVERYTHING DOWNSTREAM SEES THE SMOOTHED POSE: the root fit, the focal estimate, the
    trajectory.  ``"pose"`` is the smoothed pose; added keys: ``"pose_raw"`` [T,N,J,3], what "pose" was, and
    ``"pose_smooth_code"`` [T,N,J] uint8 (1: local line, 2: weighted mean - a single frame in reach, 3: nothing in reach, NaN).
    ``idx`` / ``window`` still name the pick, but the returned joint is no longer any hypothesis's joint.
    ``pose_smooth_floor`` (metres, finite and > 0; default 1 mm) is a regulariser - it keeps P = 1, whose covariance is
    exactly 0, and identical hypotheses solvable - not a tuned value.  A fixed-radius linear smoother: no motion model, no
    bone-length constraint, no covariance of the result; weights that are constant along the frames cancel.  What it buys on
    real weights has NOT been measured.  Every rank holds the same frame state and runs the same filter.  Without ``stride``
    use :func:`smooth_poses` on the stitched poses.

    ``bone_lengths`` (with ``stride`` and an ``aggregate``; None: everything above, unchanged, bit for bit) HOLDS THE BONE
    LENGTHS CONSTANT along the video, on the device (:func:`constrain_bones`; pafuse_amd.bones states the arithmetic).
    "video": one length per bone and step, the mean of its per-frame lengths with every frame weighing as far as its hypotheses
    agree along the bone; "symmetric": the same with left and right pooled (the ``joints_left()`` / ``joints_right()`` of the dataset's
    skeleton, else ``kps_left`` / ``kps_right``, paired by position);
    a tensor [J] or [T,J]: the caller's own lengths in metres (a calibration, another video; NaN: that bone is left alone).
    Every frame is then moved onto those lengths by ``bone_iterations`` (0 .. 64) Jacobi sweeps of the covariance-weighted
    projection - both ends of a wrong bone give way by the least Mahalanobis distance under the covariance of the hypotheses
    pooled at that joint - and an exact top-down snap.  The bones are h3wb.bone_tables': the body's real topology and the
    hands; the face points hang on nothing and are not touched; the root never moves.  It runs AFTER ``pose_smooth`` (smoothing
    bends bones, this straightens them) and before the trajectory fit: the root fit, the focal estimate and the metrics see
    the constrained pose.  ``"pose"`` is the constrained pose; added keys: ``"pose_free"`` [T,N,J,3], what "pose" was (the
    smoothed pose with ``pose_smooth``), ``"bone_length"`` [T,J] the lengths held, ``"bone_dev"`` [T,J] the weighted standard
    deviation of the free pose's bone lengths and ``"bone_frames"`` [T,J] int32 the frames they rest on (both of the video,
    also when the lengths are the caller's), ``"bone_code"`` [T,N,J] uint8 (1 moved with a bone, 0 untouched, 3 untouched
    although a bone was asked of it: no finite pose or no usable covariance) and ``"bone_resid"`` [T,N,2] the largest
    |length - L| of every frame before and after, in metres.  ``std`` / ``cov`` stay what they were: the covariance is not
    updated.  16 sweeps and the 1 mm floor are defaults, not tuned values.  One length per bone per video, no joint-angle
    limits; the estimated lengths are biased long where the noise is comparable to the bone (pass your own there).  What it
    buys on real weights has NOT been measured.

    ``ground`` (with ``trajectory``; None: everything above, unchanged; True: radius 3; or a radius 1 .. 64) finds WHICH WAY IS UP
    from the video itself, on the device behind the trajectory fit and its smoother - so on the smoothed, bone-constrained
    pose that is returned (:func:`estimate_ground`; pafuse_amd.ground): a foot point whose local line
    moves slower than ``ground_speed`` metres per FRAME (the frame rate enters here) rests on the ground, the ground is the
    plane through those points, re-weighted ``ground_passes`` times; a person standing gives a line, and the plane through it
    closest to the body's own up.  ``ground_points``: the foot joints (None: h3wb.foot_points, the six toe and heel points of
    the 134-joint layout).  Added keys (GROUND_KEYS): ``"up"`` [T,3] the unit normal in camera space, ``"camera_height"`` [T]
    metres, ``"ground_rms"`` [T], ``"ground_eig"`` [T,3], ``"ground_points"`` [T] int32, ``"ground_code"`` [T] uint8 (1 plane, 2
    line, 3 the body's own up, 0 none: NaN), ``"ground_plane"`` [T,4] float64, ``"foot"`` [T,N,K,3], ``"foot_speed"`` and
    ``"contact"`` [T,N,K], and ``"pose_world"`` [T,N,J,3] / ``"traj_world"`` [T,N,3]: pose + traj with z up and the ground at
    z = 0 - the height of a joint is its third component.  One plane per video; the pose is rotated, not corrected (no foot
    locking); world x is the camera's right, not a direction of travel.  Every default is a default, not a tuned value, and
    nobody has run it on real video."""
    plan = _frame_plan(getattr(model, "frames", None), dataset, kps_left, kps_right, cam=cam, traj=traj, conf=conf, aggregate=aggregate,
                       stride=stride, hypothesis_chunk=hypothesis_chunk, spread=spread, trajectory=trajectory, focal=focal, repair=repair,
                       repair_threshold=repair_threshold, path_weight=path_weight, path_scope=path_scope, pose_smooth=pose_smooth,
                       pose_smooth_floor=pose_smooth_floor, bone_lengths=bone_lengths, bone_iterations=bone_iterations, screen=screen,
                       screen_gate=screen_gate, screen_floor=screen_floor, ground=ground, ground_speed=ground_speed,
                       ground_passes=ground_passes, ground_gate=ground_gate, ground_floor=ground_floor, ground_spread=ground_spread,
                       ground_points=ground_points)
    seq_2d = torch.as_tensor(seq_2d, dtype=torch.float32)
    conf = _conf_operand(conf, seq_2d.shape[-3:-1])
    dev = next(model.parameters()).device
    # the callees cut and flip on the host: the screened and repaired pair takes the place of the input, whole, before either
    seq_2d, conf, screened, repaired = _front_end(seq_2d, conf, plan, dataset, kps_left, kps_right, dev)
    out = _infer_sequence(model, dataset, seq_2d, kps_left, kps_right, plan, cam=cam, traj=traj, conf=conf, batch_size=batch_size,
                          group=group, dev=dev)
    if isinstance(out, dict):
        out.update({k: v for k, v in (("screened", screened), ("repaired", repaired)) if v is not None})
    return out


@dataclasses.dataclass(frozen=True)
class _FramePlan:
    """What the per-frame chain does, every option checked (_frame_plan); a switch that is off is None (trajectory: False)"""
    aggregate: object           # None, "mean", "reproj" or "reproj_fit"
    stride: object              # None: the clip path; else 1 .. frames, one pose per video frame
    hypothesis_chunk: object
    spread: object              # what the caller wants returned: None, "std" or "cov"
    fold_spread: object         # what is folded: the pose smoother and the bones need the covariance whatever the caller wants
    path_weight: object
    path_scope: str
    trajectory: bool
    smooth: object              # the radius of the trajectory's smoother
    focal: object               # None or "estimate"
    pose_smooth: object         # (radius, floor)
    bones: object               # _bone_spec's dict with its "tables" (_bone_tables)
    ground: object              # _ground_spec's dict
    screen: object              # (radius, gate, floor)
    repair: object              # the radius
    threshold: object           # repair_threshold as given (checked when the repair or the screen is on; both read it as a float)


def _frame_plan(frames, dataset, kps_left, kps_right, *, cam, traj, conf, aggregate, stride=None, hypothesis_chunk=None, spread=None,
                trajectory=None, focal=None, repair=None, repair_threshold=0.0, path_weight=None, path_scope="clip", pose_smooth=None,
                pose_smooth_floor=1e-3, bone_lengths=None, bone_iterations=16, screen=None, screen_gate=4.0, screen_floor=0.005,
                ground=None, ground_speed=0.015, ground_passes=3, ground_gate=2.5, ground_floor=0.005, ground_spread=0.03,
                ground_points=None, frames_only=False, conf_made=False):
    """The plan of infer_sequence / evaluate_frames from their raw options and `frames` = model.frames: every option check and
    every companion check, before anything touches the model or the device.  cam, traj and conf are only asked whether they
    are there.  What evaluate_frames does differently: frames_only=True - there is no clip path, so stride None means `frames`, an
    aggregate and cam are required, traj is its own - and conf_made=True: one of its plantings will make the confidences."""
    if frames_only:
        if aggregate not in ("mean", "reproj", "reproj_fit"):
            raise ValueError(f'aggregate must be "mean", "reproj" or "reproj_fit", got {aggregate!r}')
        if stride is None:
            stride = frames
    smooth = _trajectory_radius(trajectory)
    pose_smooth = _pose_smooth_radius(pose_smooth, pose_smooth_floor)
    if pose_smooth is not None:
        if stride is None:
            raise ValueError("pose_smooth needs stride (one pose per video frame); for stitched clips call harness.smooth_poses")
        if aggregate is None:
            raise ValueError('pose_smooth needs aggregate="mean", "reproj" or "reproj_fit": it smooths the ONE pose per frame')
        pose_smooth = (pose_smooth, float(pose_smooth_floor))
    bones = _bone_spec(bone_lengths, bone_iterations)
    if bones is not None:
        if stride is None:
            raise ValueError("bone_lengths needs stride (one pose per video frame); for stitched clips call harness.constrain_bones")
        if aggregate is None:
            raise ValueError('bone_lengths needs aggregate="mean", "reproj" or "reproj_fit": it constrains the ONE pose per frame')
        bones["tables"] = _bone_tables(None, dataset, kps_left, kps_right)
        if not isinstance(bones["lengths"], str) and bones["lengths"].shape[-1] != len(bones["tables"][0]):
            raise ValueError(f"bone_lengths must be [J] or [T,J] with J = {len(bones['tables'][0])}, got {tuple(bones['lengths'].shape)}")
    _focal_mode(focal)
    ground = _ground_spec(ground, ground_speed, ground_passes, ground_gate, ground_floor, ground_spread, ground_points)
    if ground is not None and trajectory is None:
        raise ValueError("ground needs a trajectory: the ground is found in camera space"
                         + ("" if frames_only else " (harness.estimate_ground takes poses and roots a caller has)"))
    repair = _repair_radius(repair, repair_threshold)
    if frames_only and (isinstance(stride, bool) or not isinstance(stride, int) or not 1 <= stride <= frames):
        raise ValueError(f"stride must be None or an integer in 1 .. {frames} (the window length), got {stride!r}")
    path_weight = _path_weight(path_weight, aggregate, hypothesis_chunk, stride, frames, path_scope)
    if repair is not None and conf is None and not conf_made:
        raise ValueError("repair needs conf [N,J]" + (" or drop" if frames_only else "") + ": a missing detection is one whose confidence is not above repair_threshold")
    screen = _screen_radius(screen, screen_gate, screen_floor)
    if screen is not None:
        _repair_radius(1, repair_threshold)      # the threshold is read by the screen as well
        if conf is None and not conf_made:
            raise ValueError("screen needs conf [N,J]" + (", corrupt, swap or drop" if frames_only else "")
                             + ": a rejected detection leaves with confidence 0")
        screen = (screen, float(screen_gate), float(screen_floor))
    if focal is not None and trajectory is None:
        raise ValueError('focal="estimate" belongs to a trajectory'
                         + ("" if frames_only else " (harness.estimate_focal gives the estimate alone)"))
    if frames_only and cam is None:
        raise ValueError("evaluate_frames needs cam [9] (the intrinsics)")
    if trajectory is not None:
        if stride is None:
            raise ValueError("trajectory needs stride (one pose per video frame); for stitched clips call harness.fit_trajectory")
        if cam is None and focal is None:
            raise ValueError('trajectory needs cam (fx, fy, cx, cy first): the fit takes the intrinsics as known (or focal="estimate")')
    if stride is not None and not frames_only:
        if isinstance(stride, bool) or int(stride) != stride or not 1 <= int(stride) <= frames:
            raise ValueError(f"stride must be an integer in 1 .. {frames} (the window length), got {stride!r}")
        if aggregate is None:
            raise ValueError('stride needs aggregate="mean", "reproj" or "reproj_fit": the hypotheses per frame would be ragged')
    if aggregate not in (None, "mean", "reproj", "reproj_fit"):
        raise ValueError(f'aggregate must be None, "mean", "reproj" or "reproj_fit", got {aggregate!r}')
    if spread not in (None, "std", "cov"):
        raise ValueError(f'spread must be None, "std" or "cov", got {spread!r}')
    if spread is not None and aggregate is None:
        raise ValueError('spread needs aggregate="mean", "reproj" or "reproj_fit" (it is reduced on the device beside the pose)')
    if hypothesis_chunk is not None and (aggregate is None or int(hypothesis_chunk) < 1):
        raise ValueError("hypothesis_chunk is a positive count" + ("" if frames_only else " and needs an aggregate"))
    if aggregate == "reproj" and not frames_only and (cam is None or traj is None):
        raise ValueError('aggregate="reproj" needs cam [9] and traj [N,3]')
    if aggregate == "reproj_fit" and (cam is None or traj is not None):
        raise ValueError('aggregate="reproj_fit" needs cam [9] and takes no traj (the root is what it fits)')
    if conf is not None and aggregate != "reproj_fit" and trajectory is None and repair is None and screen is None and not conf_made:
        raise ValueError('conf belongs to aggregate="reproj_fit"' + (" or a trajectory" if frames_only else ""))
    if stride is None and path_scope == "video":      # one path along the video: per-frame results, the clips of cut_clips
        stride = frames
    return _FramePlan(aggregate=aggregate, stride=None if stride is None else int(stride), hypothesis_chunk=hypothesis_chunk, spread=spread,
                      fold_spread="cov" if pose_smooth is not None or bones is not None else spread,
                      path_weight=path_weight, path_scope=path_scope, trajectory=trajectory is not None, smooth=smooth, focal=focal,
                      pose_smooth=pose_smooth, bones=bones, ground=ground, screen=screen, repair=repair, threshold=repair_threshold)


def _front_end(seq_2d, conf, plan, dataset, kps_left, kps_right, dev):
    """The detections as the model will see them: screened, then repaired, as the plan asks (both on the device, the pair staying
    there in between) -> (seq_2d, conf, the screen's status map or None, the repair's or None), all on the CPU"""
    if plan.screen is None and plan.repair is None:
        return seq_2d, conf, None, None
    seq_2d = seq_2d.squeeze(0) if seq_2d.dim() == 4 else seq_2d
    screened = repaired = None
    if plan.screen is not None:
        from .detscreen import mirror_table
        radius, gate, floor = plan.screen
        m = _screen_detections(seq_2d, conf, dev, mirror=mirror_table(kps_left, kps_right, seq_2d.shape[-2]), radius=radius, gate=gate,
                               floor=floor, threshold=float(plan.threshold))
        seq_2d, conf, screened = m["x2d"], m["conf"], m["status"].cpu()
    if plan.repair is not None:
        from .detections import repair_anchors
        m = _repair_detections(seq_2d, conf, dev, anchor=repair_anchors(dataset), radius=plan.repair, threshold=float(plan.threshold))
        seq_2d, conf, repaired = m["x2d"], m["conf"], m["status"].cpu()
    return seq_2d.cpu(), conf.cpu(), screened, repaired


PATH_CANDIDATES = 256    # path_scope="video": P times the windows that cover one frame (ops.FRAMES_PATH_MAX_CANDIDATES)


def _path_weight(path_weight, aggregate, hypothesis_chunk, stride, frames, scope="clip"):
    """infer_sequence's / evaluate_frames' `path_weight`: None, or a finite float >= 0 with what it may be combined with;
    `scope`: "clip" (a path per clip) or "video" (one path along the video, any stride)"""
    if scope not in ("clip", "video"):
        raise ValueError(f'path_scope must be "clip" or "video", got {scope!r}')
    if path_weight is None:
        if scope == "video":
            raise ValueError('path_scope="video" belongs to a path_weight')
        return None
    if isinstance(path_weight, bool) or not isinstance(path_weight, (int, float)) or not 0 <= path_weight < float("inf"):   # (a NaN fails both)
        raise ValueError(f"path_weight must be None or a finite number >= 0 (normalised screen length per metre), got {path_weight!r}")
    if aggregate not in ("reproj", "reproj_fit"):
        raise ValueError('path_weight belongs to aggregate="reproj" or "reproj_fit": it is the J-Agg pick made coherent in time')
    if hypothesis_chunk is not None:
        raise ValueError("path_weight takes no hypothesis_chunk: the recursion needs all P hypotheses of a clip at once")
    if scope == "clip" and stride is not None and int(stride) != frames:
        raise ValueError(f"path_weight takes un-strided clips only (stride None or {frames}): a path crosses no pooled windows")
    return float(path_weight)


def _sample_batch(sampler, dataset, plan, x2d, x2d_flip, traj, cam, conf, group, want=None):
    """One batch of clips or windows sampled under the plan; traj [B,F,3] with "reproj", conf [B,F,J] or None with "reproj_fit",
    else None.  `want` None (the frames path): the merged states of the batch's hypotheses, what accumulate_frames folds;
    names (the clip path): the combined outputs of those names.  -> (that dict, the hypotheses themselves with
    path_scope="video" - they stay on the device until the end of the video - else None)"""
    from . import ops
    from .evaluate import path_poses
    merged, spread, P = want is None, plan.fold_spread, sampler.model.num_proposals
    fit, reproj = plan.aggregate == "reproj_fit", plan.aggregate in ("reproj", "reproj_fit")

    def fold(state, pred, h0):
        if fit:
            return accumulate_poses(state, pred, h0, dataset, x2d, None, cam, fit=True, conf=conf)
        return accumulate_poses(state, pred, h0, dataset, x2d, traj, cam) if reproj else accumulate_poses(state, pred, h0, dataset)

    if plan.path_weight is None:
        state = moments = None
        for pred, h0, _ in sampler.sample_chunks(x2d, None, input_2d_flip=x2d_flip, chunk=plan.hypothesis_chunk):
            if merged or reproj or spread is None:      # the clip path's mean with a spread: the spread state holds the sums
                state = fold(state, pred, h0)
            if spread is not None:
                moments = accumulate_spread(moments, pred, h0, dataset)
            del pred
        return aggregate_poses_sharded(None, None, P, dataset, group=group, state=state, want=() if merged else want,
                                       spread_state=moments, merged=merged), None
    # a path needs ALL P hypotheses at once (gathered across the ranks, as aggregate=None gathers them): every rank holds them
    # and the same states, with nothing to exchange
    pred = sampler(x2d, None, input_2d_flip=x2d_flip)
    video = plan.path_scope == "video"
    if video:           # the path comes at the end of the video: here the states the default folds
        state = fold(None, pred, 0)
        out = {"state": torch.empty_like(state.head), "shape": state.shape}
        ops.combine_poses(state.head.unsqueeze(0), state.shape, P, merged=out["state"], want=(), no_pick_ok=fit)
    else:
        out = path_poses(pred, dataset, x2d, cam, plan.path_weight, traj=traj, conf=conf, fit=fit)
    if spread is not None:
        moments = accumulate_spread(None, pred, 0, dataset)
        into = torch.empty_like(moments.head) if merged else None
        out.update(ops.combine_spread(moments.head.unsqueeze(0), moments.shape, merged=into,
                                      want=() if merged else [k for k in want if k in ("std", "cov")]))
        if merged:
            out["spread_state"] = into
    return out, (pred if video else None)


def _infer_sequence(model, dataset, seq_2d, kps_left, kps_right, plan, *, cam, traj, conf, batch_size, group, dev):
    """infer_sequence behind its plan and the detection front end: the frames path's result copied to the CPU, or the clip path"""
    if plan.stride is not None:
        out = _infer_frames_device(model, dataset, seq_2d, kps_left, kps_right, plan, cam=cam, traj=traj, conf=conf,
                                   batch_size=batch_size, group=group, dev=dev)
        return {k: v.cpu() for k, v in out.items()}
    F, spread = model.frames, plan.spread
    x2d = cut_clips(seq_2d, F).to(dev)
    x2d_flip = cut_clips(flip_2d(seq_2d, kps_left, kps_right), F).to(dev)
    sampler = ShardedSampler(model, group)
    if plan.aggregate is None:
        outs = []
        for lo in range(0, x2d.shape[0], batch_size):
            pred = sampler(x2d[lo:lo + batch_size], None, input_2d_flip=x2d_flip[lo:lo + batch_size])
            outs.append(wb_pose_from_parts(pred, dataset).cpu())
        return torch.cat(outs)
    fit, reproj = plan.aggregate == "reproj_fit", plan.aggregate in ("reproj", "reproj_fit")
    clip_traj = clip_conf = None
    if fit:
        cam = torch.as_tensor(cam, dtype=torch.float32).to(dev)
        if conf is not None:
            clip_conf = cut_clips(conf.unsqueeze(-1), F).squeeze(-1).to(dev)               # [clips,F,J]
    elif reproj:
        traj = torch.as_tensor(traj, dtype=torch.float32)
        if traj.dim() != 2 or tuple(traj.shape) != (seq_2d.shape[-3], 3):
            raise ValueError(f"traj must be [N,3] with N = {seq_2d.shape[-3]} frames, got {tuple(traj.shape)}")
        clip_traj = cut_clips(traj.unsqueeze(1), F).squeeze(2).to(dev)                      # [clips,F,3]
        cam = torch.as_tensor(cam, dtype=torch.float32).to(dev)
    pose_name = "pick" if reproj else "mean"
    names = ((pose_name,) + (("idx",) if reproj else ()) + (("mean",) if fit else ())
             + (() if spread is None else ("std",) if spread == "std" else ("std", "cov")))
    kept = {k: [] for k in names if not (fit and k == "mean")}     # with the fit the mean only fills joints without a pick
    for lo in range(0, x2d.shape[0], batch_size):
        hi = min(lo + batch_size, x2d.shape[0])
        out, _ = _sample_batch(sampler, dataset, plan, x2d[lo:hi], x2d_flip[lo:hi], None if clip_traj is None else clip_traj[lo:hi], cam,
                               None if clip_conf is None else clip_conf[lo:hi], group, want=names)
        if fit:     # a joint without a pick (or a path) carries the mean: the one combine call wrote both
            out["pick"] = torch.where((out["idx"] < 0).unsqueeze(-1), out["mean"], out["pick"])
        for k in kept:
            kept[k].append(out[k].cpu())
    kept = {k: torch.cat(v) for k, v in kept.items()}
    if spread is not None:
        return {("pose" if k == pose_name else k): v for k, v in kept.items()}
    return (kept["pick"], kept["idx"]) if reproj else kept["mean"]


def cut_windows(seq, starts, frames=27):
    """[N, ...] -> [len(starts), frames, ...]: the windows that begin at `starts` (pafuse_amd.windows.window_starts); a
    sequence shorter than a window is padded by repeating its final frame, as cut_clips pads it."""
    n = seq.shape[0]
    if n < frames:
        seq = torch.cat([seq, seq[-1:].expand(frames - n, *seq.shape[1:])], dim=0)
    return torch.stack([seq[int(s):int(s) + frames] for s in starts])


def _infer_frames_device(model, dataset, seq_2d, kps_left, kps_right, plan, *, cam, traj, conf, batch_size, group, dev):
    """infer_sequence(stride=...): sliding windows pooled into one pose per video frame, then the stages behind the finish
    (_finish_stages) - the result left on the device, where evaluate_frames scores it"""
    from . import ops
    from .windows import coverage, window_starts
    if seq_2d.dim() == 4:
        seq_2d = seq_2d.squeeze(0)
    N, F, P = seq_2d.shape[0], model.frames, model.num_proposals
    starts, valid = window_starts(N, F, plan.stride)
    fit, reproj = plan.aggregate == "reproj_fit", plan.aggregate in ("reproj", "reproj_fit")
    video = plan.path_weight is not None and plan.path_scope == "video"
    if video and int(coverage(N, starts, valid).max()) * P > PATH_CANDIDATES:
        raise ValueError(f'path_scope="video": up to {int(coverage(N, starts, valid).max())} windows cover one frame at stride {plan.stride}, with '
                         f"{P} hypotheses each: at most {PATH_CANDIDATES} candidates per frame")
    x2d = cut_windows(seq_2d, starts, F).to(dev)
    x2d_flip = cut_windows(flip_2d(seq_2d, kps_left, kps_right), starts, F).to(dev)
    if reproj or plan.trajectory:
        cam = _default_cam(dev) if cam is None else torch.as_tensor(cam, dtype=torch.float32).to(dev)
    win_traj = win_conf = None
    if fit and conf is not None:
        win_conf = cut_windows(conf, starts, F).to(dev)                                # [windows,F,J]
    if reproj and not fit:
        traj = torch.as_tensor(traj, dtype=torch.float32)
        if traj.dim() != 2 or tuple(traj.shape) != (N, 3):
            raise ValueError(f"traj must be [N,3] with N = {N} frames, got {tuple(traj.shape)}")
        win_traj = cut_windows(traj, starts, F).to(dev)                                # [windows,F,3]
    sampler = ShardedSampler(model, group)
    frames, kept = None, []     # kept, path_scope="video": the hypotheses of every window stay on the device until the end of the video
    for lo in range(0, x2d.shape[0], batch_size):
        hi = min(lo + batch_size, x2d.shape[0])
        merged, pred = _sample_batch(sampler, dataset, plan, x2d[lo:hi], x2d_flip[lo:hi], None if win_traj is None else win_traj[lo:hi], cam,
                                     None if win_conf is None else win_conf[lo:hi], group)
        frames = accumulate_frames(frames, merged, starts[lo:hi], valid[lo:hi], N, P)
        if pred is not None:
            kept.append(pred)
    needs_cov = plan.fold_spread != plan.spread
    want = (("mean", "count") + (("pick", "idx", "window") if reproj else ())
            + (() if plan.spread is None else ("std",) if plan.spread == "std" else ("std", "cov")) + (("cov",) if needs_cov else ()))
    out = ops.finish_frames(N, frames.T, frames.J, frame=frames.pose, spread=frames.spread, want=want)
    if video:       # one path along the video through the hypotheses of all windows, against the pooled mean
        from .evaluate import path_frames
        path = path_frames(torch.cat(kept), dataset, seq_2d.to(dev), cam, plan.path_weight, starts, valid, N, frames,
                           traj=None if fit else traj.to(dev), conf=None if conf is None or not fit else conf.to(dev), fit=fit)
        del kept
        out.update(pick=path["pick"], idx=path["idx"], window=path["window"], path_cost=path["cost"])
    return _finish_stages(out, plan, seq_2d, cam, conf)


def _finish_stages(out, plan, seq_2d, cam, conf):
    """The stages behind the finish (or the video path) in their order, each on what the one before it returns: out - finish_frames'
    dict on the device - becomes infer_sequence(stride=...)'s; seq_2d [N,J,2] and conf [N,J] or None on the CPU, cam on the device"""
    from . import ops
    dev = out["mean"].device
    if plan.aggregate == "reproj_fit":      # a joint without a pick carries the pooled mean
        out["pick"] = torch.where((out["idx"] < 0).unsqueeze(-1), out["mean"], out["pick"])
    out["pose"] = out.pop("pick") if "pick" in out else out["mean"]
    out.pop("mean", None)
    if plan.fold_spread == "cov":           # the covariance is returned only when the caller asked for it
        cov = out["cov"] if plan.spread == "cov" else out.pop("cov")
    if plan.pose_smooth is not None:        # on the pose that is returned: everything below sees the smoothed pose
        out["pose_raw"] = out["pose"].contiguous()
        out["pose"], out["pose_smooth_code"] = ops.smooth_poses(out["pose_raw"], cov, plan.pose_smooth[0], floor=plan.pose_smooth[1], want_code=True)
    if plan.bones is not None:              # smoothing bends bones, this straightens them; the root fit below sees the constrained pose
        out.update(_constrain_bones(out["pose"].contiguous(), cov, plan.bones))
    if plan.trajectory:                     # the root of the pose that is returned, on the device before anything crosses to the host
        out.update(_fit_trajectory(out["pose"], seq_2d.to(dev), cam, None if conf is None else conf.to(dev), smooth=plan.smooth, focal=plan.focal))
    if plan.ground is not None:             # behind the fit and its smoother: the plane through the resting feet of the pose and roots
        out.update(_estimate_ground(out["pose"], out["traj"], plan.ground))
    return out


def _trajectory_radius(trajectory, name="trajectory"):
    """infer_sequence's `trajectory`: None / True -> None (no smoothing), an integer r in 1 .. 64 -> r"""
    if trajectory is None or trajectory is True:
        return None
    if isinstance(trajectory, bool) or not isinstance(trajectory, int) or not 1 <= trajectory <= 64:
        raise ValueError(f"{name} must be None, True (the per-frame fit) or a smoothing radius in 1 .. 64, got {trajectory!r}")
    return trajectory


def _pose_smooth_radius(pose_smooth, floor=1e-3, name="pose_smooth"):
    """infer_sequence's `pose_smooth` and its floor: None, or an integer radius in 1 .. 64 with a floor that is finite and > 0"""
    if pose_smooth is None:
        return None
    if isinstance(pose_smooth, bool) or not isinstance(pose_smooth, int) or not 1 <= pose_smooth <= 64:
        raise ValueError(f"{name} must be None or a smoothing radius in 1 .. 64 (frames), got {pose_smooth!r}")
    if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not 0 < floor < float("inf"):      # (a NaN fails both)
        raise ValueError(f"{name}_floor must be a finite number > 0 (metres; the default 1e-3 is a regulariser, not a tuned value), got {floor!r}")
    return pose_smooth


BONE_FLOOR = 1e-3      # metres: a regulariser that keeps a zero covariance usable, not a tuned value


def _bone_spec(bone_lengths, bone_iterations=16, snap=True, floor=BONE_FLOOR):
    """infer_sequence's `bone_lengths` / `bone_iterations`: None, or {"lengths": "video" | "symmetric" | a float32 CPU tensor
    [J] or [T,J], "iterations", "snap", "floor"} - refused here, before anything touches the device"""
    if bone_lengths is None:
        return None
    if isinstance(bone_lengths, str):
        if bone_lengths not in ("video", "symmetric"):
            raise ValueError(f'bone_lengths must be None, "video", "symmetric" or a tensor [J] or [T,J] of lengths in metres, got {bone_lengths!r}')
        lengths = bone_lengths
    else:
        lengths = torch.as_tensor(bone_lengths, dtype=torch.float32)
        if lengths.dim() not in (1, 2) or 0 in lengths.shape:
            raise ValueError(f"bone_lengths must be [J] or [T,J] (metres), got {tuple(lengths.shape)}")
    if isinstance(bone_iterations, bool) or not isinstance(bone_iterations, int) or not 0 <= bone_iterations <= 64:
        raise ValueError(f"bone_iterations must be an integer in 0 .. 64 (Jacobi sweeps; the default 16 is not a tuned value), got {bone_iterations!r}")
    if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not 0 < floor < float("inf"):
        raise ValueError(f"floor must be a finite number > 0 (metres; the default 1e-3 is a regulariser, not a tuned value), got {floor!r}")
    return {"lengths": lengths, "iterations": int(bone_iterations), "snap": bool(snap), "floor": float(floor)}


def _bone_tables(tables, dataset=None, kps_left=None, kps_right=None, J=None):
    """-> (parent, mirror) int32 numpy [J], validated on the host (ops.bone_table): `tables` as given - (parent, mirror) with
    mirror None or absent - or h3wb.bone_tables of the dataset: the joints_left() / joints_right() of its skeleton() where it has one,
    else kps_left / kps_right, paired by position"""
    from . import ops
    from .h3wb import bone_tables
    if tables is None:
        if hasattr(dataset, "skeleton"):                              # the dataset's own joints_left() / joints_right()
            kps_left = kps_right = None
        parent, mirror = bone_tables(68 if dataset is None else dataset, True, None if kps_left is None else list(kps_left),
                                     None if kps_right is None else list(kps_right))
    else:
        if not isinstance(tables, (tuple, list)) or len(tables) not in (1, 2):
            raise ValueError("tables must be (parent, mirror) - mirror may be None - as h3wb.bone_tables returns them")
        parent, mirror = tables[0], tables[1] if len(tables) == 2 else None
    n = len(parent) if J is None else int(J)
    parent = ops.bone_table(parent, n)
    return parent, None if mirror is None else ops.bone_table(mirror, n, mirror=True)


def _constrain_bones(free, cov, bones):
    """the bone keys of infer_sequence on the device: free [T,N,J,3] contiguous, cov [T,N,J,6] or None, bones: _bone_spec's dict
    with its tables"""
    from . import ops
    T, N, J, _ = free.shape
    parent, mirror = bones["tables"]
    if len(parent) != J:
        raise ValueError(f"the bone tables hold {len(parent)} joints, the pose {J}")
    lengths, floor = bones["lengths"], bones["floor"]
    video, dev, frames = ops.bone_lengths(free, cov, parent, mirror if isinstance(lengths, str) and lengths == "symmetric" else None,
                                          floor=floor, want_dev=True, want_frames=True)
    if isinstance(lengths, str):
        held = video
    else:
        if tuple(lengths.shape) not in ((J,), (T, J)):
            raise ValueError(f"bone_lengths must be [J] = [{J}] or [T,J] = {(T, J)}, got {tuple(lengths.shape)}")
        held = lengths.to(free.device)
        held = (held.unsqueeze(0).expand(T, J) if held.dim() == 1 else held).contiguous()
    pose, code, resid = ops.project_bones(free, cov, parent, held, iterations=bones["iterations"], snap=bones["snap"], floor=floor,
                                          want_code=True, want_resid=True)
    return {"pose": pose, "pose_free": free, "bone_length": held, "bone_dev": dev, "bone_frames": frames, "bone_code": code,
            "bone_resid": resid}


def _focal_mode(focal):
    if focal not in (None, "estimate"):
        raise ValueError(f'focal must be None (cam holds it) or "estimate", got {focal!r}')


def _default_cam(dev):
    """the intrinsics of a camera nothing is known of, for screen-normalised detections: square pixels, the principal point at the
    image centre, no distortion (the focal slots are placeholders: estimate_focal reads only their ratio)"""
    return torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)


def _cam9(cam, dev):
    """cam (None, or 4 .. 9 values, fx fy cx cy first) -> [9] fp32 on the device, the missing distortion terms 0"""
    if cam is None:
        return _default_cam(dev)
    cam = torch.as_tensor(cam, dtype=torch.float32).reshape(-1)
    if not 4 <= cam.numel() <= 9:
        raise ValueError(f"cam holds 4 .. 9 values (fx fy cx cy, then the distortion terms), got {cam.numel()}")
    return torch.cat([cam, cam.new_zeros(9 - cam.numel())]).to(dev)


def _estimate_focal(pose, x2d, cam, conf):
    """device tensors -> the focal keys of infer_sequence / fit_trajectory / estimate_focal, on the device"""
    from . import ops
    m = ops.estimate_focal(pose.contiguous(), x2d.contiguous(), cam.contiguous(), conf=None if conf is None else conf.contiguous())
    return {"focal": m["focal"], "focal_r2": m["r2"], "focal_frames": m["frames"], "cam": m["cam"]}


def _fit_trajectory(pose, x2d, cam, conf, *, smooth, focal=None):
    """device tensors -> the trajectory keys of infer_sequence / fit_trajectory, on the device"""
    from . import ops
    est = {}
    if focal is not None:       # the estimate of the last, fully denoised step: a row of the device tensor, no host round trip
        est = _estimate_focal(pose, x2d, _cam9(cam, pose.device), conf)
        cam = est["cam"][est["cam"].shape[0] - 1]
    m = ops.fit_trajectory(pose.contiguous(), x2d.contiguous(), cam.contiguous(), conf=None if conf is None else conf.contiguous())
    out = {"traj": m["traj"], "traj_weight": m["wsum"], "traj_resid": m["resid"], **est}
    if smooth is not None:
        out["traj_raw"] = m["traj"]
        out["traj"] = ops.smooth_trajectory(m["traj"], m["wsum"], smooth)
    return out


@torch.no_grad()
def fit_trajectory(poses, seq_2d, cam=None, conf=None, smooth=None, device="cuda", focal=None):
    """The camera-space root trajectory of per-frame poses: ``poses`` [T,N,J,3] whole-body and root-relative - an
    ``infer_sequence(stride=...)["pose"]`` or the result of :func:`stitch_poses` - ``seq_2d`` [N,J,2] the screen-normalised
    detections they were lifted from, ``cam`` the intrinsics (fx, fy, cx, cy first), ``conf`` [N,J] the detections' weights
    (None: all 1).  Fitted on the device per (t, frame) (pafuse_amd.trajectory; ops.fit_trajectory); ``smooth=r`` (1 .. 64)
    also runs the local-linear filter of that radius along the frames (ops.smooth_trajectory).  Returns a dict of CPU tensors:
    ``"traj"`` [T,N,3] (smoothed when ``smooth`` is given), ``"traj_raw"`` when smoothed, ``"traj_weight"`` [T,N] and
    ``"traj_resid"`` [T,N] - the keys ``infer_sequence(trajectory=...)`` adds.  Camera-space poses: ``poses + traj[:, :, None]``.
    ``focal="estimate"``: the focal length is estimated from the poses and detections (:func:`estimate_focal`) and the fit runs
    with the estimate of the last step; ``cam`` is then optional, and ``"focal"``, ``"focal_r2"``, ``"focal_frames"`` [T] and
    ``"cam"`` [T,9] are added."""
    _focal_mode(focal)
    if smooth is True:
        raise ValueError("smooth must be None or a smoothing radius in 1 .. 64")
    smooth = _trajectory_radius(smooth, "smooth")
    if cam is None and focal is None:
        raise ValueError('fit_trajectory needs cam (fx, fy, cx, cy first), or focal="estimate"')
    poses, seq_2d = _poses_operand(poses, seq_2d, "seq_2d [N,J,2]", slice(1, 3), (2,), empty_ok=True)
    conf = _conf_operand(conf, seq_2d.shape[:2])

    def run(dev):
        cam9 = _cam9(cam, dev) if focal is not None else torch.as_tensor(cam, dtype=torch.float32).reshape(-1).to(dev)
        return _fit_trajectory(poses.to(dev), seq_2d.to(dev), cam9, None if conf is None else conf.to(dev), smooth=smooth, focal=focal)
    return _run_on(poses, device, run)


@torch.no_grad()
def smooth_poses(poses, cov=None, radius=13, floor=1e-3, device="cuda"):
    """Per-frame poses smoothed along the frames on the device, the counterpart of :func:`fit_trajectory` for the joints:
    ``poses`` [T,N,J,3] - an ``infer_sequence(stride=...)["pose"]``, the result of :func:`stitch_poses` or any such array -
    ``cov`` [T,N,J,6] the covariance of the hypotheses per (t, frame, joint) (``infer_sequence(spread="cov")["cov"]``: xx xy xz
    yy yz zz; None: every frame weighs the same in every direction, which is :func:`fit_trajectory`'s filter per joint),
    ``radius`` 1 .. 64 frames, ``floor`` in metres (finite and > 0; the 1 mm default is a regulariser that keeps a zero
    covariance solvable, not a tuned value).  ops.smooth_poses; pafuse_amd.posesmooth states the arithmetic.  Returns a dict of
    CPU tensors: ``"pose"`` [T,N,J,3] the smoothed pose, ``"pose_raw"`` the input and ``"pose_smooth_code"`` [T,N,J] uint8
    (1 line, 2 weighted mean, 3 none: NaN) - the keys ``infer_sequence(pose_smooth=...)`` adds.  A fixed-radius linear
    smoother without a motion model or a bone-length constraint; what it buys on real weights has not been measured."""
    from . import ops
    radius = _pose_smooth_radius(radius, floor, "radius")
    if radius is None:
        raise ValueError("radius must be a smoothing radius in 1 .. 64 (frames), got None")
    poses = _poses_operand(poses)
    cov = _cov_operand(cov, poses)

    def run(dev):
        raw = poses.to(dev).contiguous()
        pose, code = ops.smooth_poses(raw, None if cov is None else cov.to(dev).contiguous(), radius, floor=float(floor), want_code=True)
        return {"pose": pose, "pose_raw": raw, "pose_smooth_code": code}
    return _run_on(poses, device, run)


@torch.no_grad()
def constrain_bones(poses, cov=None, tables=None, lengths="video", iterations=16, snap=True, floor=1e-3, device="cuda"):
    """Bone lengths held constant along a video, for poses a caller already has: ``poses`` [T,N,J,3] - an
    ``infer_sequence(stride=...)["pose"]``, the result of :func:`stitch_poses` or :func:`smooth_poses`, or any such array of N
    video frames - ``cov`` [T,N,J,6] the covariance of the hypotheses per (t, frame, joint) (``infer_sequence(spread="cov")``;
    None: zeros - every joint gives way alike in every direction), ``tables`` (parent, mirror) as h3wb.bone_tables returns
    them (None: the H3WB tables with the inserted root, 134 joints; every parent index must be smaller than its child's),
    ``lengths`` "video" (one length per bone and step from the whole video: ops.bone_lengths), "symmetric" (the same with the
    mirror partners pooled) or a tensor [J] or [T,J] of the caller's own lengths in metres (NaN: that bone is left alone),
    ``iterations`` 0 .. 64 Jacobi sweeps of the covariance-weighted projection, ``snap`` the exact top-down pass behind them,
    ``floor`` in metres (finite and > 0).  16 sweeps and the 1 mm floor are defaults, not tuned values.  ops.bone_lengths and
    ops.project_bones; pafuse_amd.bones states the arithmetic.  Returns a dict of CPU tensors: ``"pose"`` [T,N,J,3] the
    constrained pose, ``"pose_free"`` the input, ``"bone_length"`` [T,J] the lengths held, ``"bone_dev"`` [T,J] the weighted
    standard deviation of the input's bone lengths, ``"bone_frames"`` [T,J] int32, ``"bone_code"`` [T,N,J] uint8 (1 moved with a
    bone, 0 untouched, 3 untouched although a bone was asked of it) and ``"bone_resid"`` [T,N,2] the largest |length - L| of every
    frame before and after (metres) - the keys ``infer_sequence(bone_lengths=...)`` adds.  Jacobi converges slowly:
    ``bone_resid`` with ``snap=False`` tells how far.  One length per bone per video, no joint-angle limits, the covariance is
    not updated; what it buys on real weights has not been measured."""
    bones = _bone_spec(lengths, iterations, snap, floor)
    if bones is None:
        raise ValueError('lengths must be "video", "symmetric" or a tensor [J] or [T,J], got None')
    if not isinstance(snap, (bool, int)) or snap not in (0, 1):
        raise ValueError(f"snap must be a bool, got {snap!r}")
    poses = _poses_operand(poses)
    T, N, J, _ = poses.shape
    cov = _cov_operand(cov, poses)
    bones["tables"] = _bone_tables(tables, J=None if tables is None else J)
    if len(bones["tables"][0]) != J:
        raise ValueError(f"the bone tables hold {len(bones['tables'][0])} joints, the pose {J}")
    if not isinstance(bones["lengths"], str) and tuple(bones["lengths"].shape) not in ((J,), (T, J)):
        raise ValueError(f"lengths must be [J] = [{J}] or [T,J] = {(T, J)}, got {tuple(bones['lengths'].shape)}")
    return _run_on(poses, device, lambda dev: _constrain_bones(poses.to(dev).contiguous(), None if cov is None else cov.to(dev).contiguous(), bones))


@torch.no_grad()
def estimate_focal(poses, seq_2d, cam=None, conf=None, device="cuda"):
    """The focal length of the camera of a video, estimated from per-frame poses and the detections they were lifted from:
    ``poses`` [T,N,J,3] whole-body and root-relative, ``seq_2d`` [N,J,2] screen-normalised, ``conf`` [N,J] (None: all 1), as
    :func:`fit_trajectory` takes them.  ``cam`` (4 .. 9 values): its principal point, pixel aspect cam[1]/cam[0] and distortion
    terms are kept, its focal length is not read; None means square pixels and the principal point at the image centre.
    One focal length per step t for the whole video, on the device (pafuse_amd.focal; ops.estimate_focal).  Returns a dict of
    CPU tensors: ``"focal"`` [T] in screen-normalised units (pixels: focal * width / 2; NaN: no estimate), ``"focal_r2"`` [T]
    the fraction of the perspective signal the estimate explains, ``"focal_frames"`` [T] the frames it rests on, and ``"cam"``
    [T,9] the intrinsics with the estimate in place - what ``fit_trajectory(..., cam=out["cam"][-1])`` takes.  The estimate
    inherits a depth-scale error of the poses one for one; a single frame or a distant person carries little signal, which
    focal_r2 and focal_frames show."""
    poses, seq_2d = _poses_operand(poses, seq_2d, "seq_2d [N,J,2]", slice(1, 3), (2,), empty_ok=True)
    conf = _conf_operand(conf, seq_2d.shape[:2])
    cam = _cam9(cam, "cpu")                                          # refused here, before anything touches the device
    return _run_on(poses, device, lambda dev: _estimate_focal(poses.to(dev), seq_2d.to(dev), cam.to(dev), None if conf is None else conf.to(dev)))


GROUND_KEYS = ("up", "camera_height", "ground_rms", "ground_eig", "ground_points", "ground_code", "ground_plane", "foot", "foot_speed",
               "contact", "pose_world", "traj_world")


def _ground_spec(ground, speed=0.015, passes=3, gate=2.5, floor=0.005, spread=0.03, points=None):
    """infer_sequence's `ground` and its companions: None -> None, True -> radius 3, an integer r in 1 .. 64 -> r; -> the
    keyword arguments of ops.estimate_ground (defaults, not tuned values), refused here before anything touches the device"""
    if ground is None:
        return None
    if ground is True:
        ground = 3
    if isinstance(ground, bool) or not isinstance(ground, int) or not 1 <= ground <= 64:
        raise ValueError(f"ground must be None, True (radius 3) or a radius in 1 .. 64 frames, got {ground!r}")
    for name, v in (("ground_speed", speed), ("ground_gate", gate), ("ground_floor", floor), ("ground_spread", spread)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be a number that is finite and > 0, got {v!r}")
    if isinstance(passes, bool) or not isinstance(passes, int) or not 1 <= passes <= 8:
        raise ValueError(f"ground_passes must be an integer in 1 .. 8, got {passes!r}")
    return dict(points=points, radius=ground, speed=float(speed), passes=passes, gate=float(gate), floor=float(floor), spread=float(spread))


def _estimate_ground(pose, traj, spec):
    """device tensors -> the ground keys of infer_sequence / estimate_ground (GROUND_KEYS), on the device"""
    from . import ops
    spec = dict(spec)
    points = spec.pop("points")
    if points is None:
        from .h3wb import foot_points
        points = foot_points(True)
        if pose.shape[2] != 134:
            raise ValueError(f"ground: the default foot points are those of the 134-joint layout, the pose has {pose.shape[2]} joints: pass points")
    m = ops.estimate_ground(pose.contiguous(), traj.contiguous(), points, want=[k for k in ops.GROUND_OUTPUTS if k != "scale"], **spec)
    m["ground_plane"] = m.pop("plane")
    return {k: m[k] for k in GROUND_KEYS}


@torch.no_grad()
def estimate_ground(poses, traj, points=None, radius=3, speed=0.015, passes=3, gate=2.5, floor=0.005, spread=0.03, device="cuda"):
    """Which way is up, for poses and roots a caller already has: ``poses`` [T,N,J,3] whole-body and root-relative, ``traj``
    [T,N,3] their camera-space roots (NaN: none) - ``infer_sequence(trajectory=...)``'s "pose" and "traj", or
    :func:`fit_trajectory`'s - ``points`` the foot joints (None: h3wb.foot_points, the six toe and heel points of the 134-joint
    layout; not the ankles, which ride above the floor), ``radius`` 1 .. 64 frames of the local line through every foot
    point, ``speed`` in metres per FRAME below which a foot counts as resting (the frame rate enters here), ``passes`` 1 .. 8
    re-weightings with ``gate`` times the plane's own rms (at least ``floor`` metres), ``spread`` metres the extent the contacts
    must have for a plane (or, failing that, a line).  On the device (ops.estimate_ground; pafuse_amd.ground states the
    arithmetic).  Returns a dict of CPU tensors, the keys ``infer_sequence(ground=...)`` adds (GROUND_KEYS): ``"up"``,
    ``"camera_height"``, ``"ground_rms"``, ``"ground_eig"``, ``"ground_points"``, ``"ground_code"`` (1 plane, 2 line, 3 the
    body's own up, 0 none: NaN everywhere), ``"ground_plane"``, ``"foot"``, ``"foot_speed"``, ``"contact"``, ``"pose_world"`` and
    ``"traj_world"``.  One plane per video: no stairs, no changing slope, no moving camera; a slow foot in the air counts until
    the re-weighting drops it; codes 2 and 3 lean on the lifted body's own up and inherit its lean; the pose is rotated, not
    corrected.  Every default is a default, not a tuned value; nobody has run it on real video."""
    spec = _ground_spec(radius if radius is not True else None, speed, passes, gate, floor, spread, points)
    if spec is None:
        raise ValueError(f"radius must be a radius in 1 .. 64 (frames), got {radius!r}")
    poses, traj = _poses_operand(poses, traj, "traj [T,N,3]")
    return _run_on(poses, device, lambda dev: _estimate_ground(poses.to(dev), traj.to(dev), spec))


@torch.no_grad()
def frames_to_world(poses, traj, plane, device="cuda"):
    """Camera space to world space with a plane a caller has: ``poses`` [T,N,J,3] root-relative, ``traj`` [T,N,3], ``plane`` [T,4]
    float64 - :func:`estimate_ground`'s "ground_plane" - or [4], ONE plane for every step (its last row, say: the plane of the
    fully denoised step).  ops.frames_to_world.  Returns a dict of CPU tensors ``"pose_world"`` [T,N,J,3] and ``"traj_world"``
    [T,N,3]: z up, the ground at z = 0, x the camera's right levelled; NaN in gives NaN out."""
    from . import ops
    poses, traj = _poses_operand(poses, traj, "traj [T,N,3]")
    plane = torch.as_tensor(plane, dtype=torch.float64)
    if tuple(plane.shape) == (4,):
        plane = plane.expand(poses.shape[0], 4)
    if tuple(plane.shape) != (poses.shape[0], 4):
        raise ValueError(f"plane must be [T,4] = {(poses.shape[0], 4)} or [4], got {tuple(plane.shape)}")
    def run(dev):
        pose_world, traj_world = ops.frames_to_world(poses.to(dev).contiguous(), traj.to(dev).contiguous(), plane.to(dev).contiguous())
        return {"pose_world": pose_world, "traj_world": traj_world}
    return _run_on(poses, device, run)


def load_pifpaf_keypoints(path, num_kps=134, with_conf=False):
    """OpenPifPaf whole-body detections, one JSON object per line and frame, first person of each frame
    (in_the_wild/h3wb_diffusion.py:57-70): -> float32 [frames, num_kps, 2] in pixels with the root joint (midpoint of
    the shifted hip joints 12 and 13) inserted at index 0.  Confidences are dropped, as in the reference - unless
    with_conf=True: then -> (kps, conf [frames, num_kps] float32), the detector's confidence of every keypoint (0 where it
    found none: OpenPifPaf writes (0, 0, 0) there), the inserted root taking the smaller of its two hips'."""
    import json
    import numpy as np
    frames = []
    with open(path) as f:
        for line in f:
            if line.strip():
                frames.append(json.loads(line))
    kps = np.zeros((len(frames), num_kps, 2), dtype=np.float32)
    conf = np.zeros((len(frames), num_kps), dtype=np.float32)
    for i, frame in enumerate(frames):
        flat = frame["predictions"][0]["keypoints"]
        kps[i, 1:, 0] = flat[::3]
        kps[i, 1:, 1] = flat[1::3]
        kps[i, :1, :] = (kps[i, 12:13, :] + kps[i, 13:14, :]) / 2.
        conf[i, 1:] = flat[2::3]
        conf[i, 0] = min(conf[i, 12], conf[i, 13])
    return (kps, conf) if with_conf else kps


def load_pifpaf_people(path, num_kps=134, max_people=None):
    """OpenPifPaf whole-body detections, one JSON object per line and frame, EVERY person of each frame, in the detector's
    order - which is not stable from frame to frame: -> (kps float32 [frames, K, num_kps, 2] in pixels, conf float32
    [frames, K, num_kps]), the root inserted at index 0 as :func:`load_pifpaf_keypoints` does.  K is the largest number of
    people in any frame, or ``max_people`` if that is smaller (the detector's first entries are kept); a slot a frame does
    not fill, and every slot of a frame whose ``predictions`` list is empty, is all zeros with confidence 0 - "nobody" to
    :func:`track_people`."""
    import json
    import numpy as np
    if max_people is not None and (isinstance(max_people, bool) or not isinstance(max_people, int) or max_people < 1):
        raise ValueError(f"max_people must be None or an integer >= 1, got {max_people!r}")
    frames = []
    with open(path) as f:
        for line in f:
            if line.strip():
                frames.append(json.loads(line)["predictions"])
    K = max([len(people) for people in frames] + [1])
    if max_people is not None:
        K = min(K, max_people)
    kps = np.zeros((len(frames), K, num_kps, 2), dtype=np.float32)
    conf = np.zeros((len(frames), K, num_kps), dtype=np.float32)
    for i, people in enumerate(frames):
        for k, person in enumerate(people[:K]):
            flat = person["keypoints"]
            kps[i, k, 1:, 0] = flat[::3]
            kps[i, k, 1:, 1] = flat[1::3]
            kps[i, k, :1, :] = (kps[i, k, 12:13, :] + kps[i, k, 13:14, :]) / 2.
            conf[i, k, 1:] = flat[2::3]
            conf[i, k, 0] = min(conf[i, k, 12], conf[i, k, 13])
    return kps, conf


@torch.no_grad()
def track_people(kps, conf, tracks=1, seed=None, gate=0.5, skip=0.05, max_gap=4, support=5, min_frames=5, threshold=0.0,
                 device="cuda"):
    """People followed through a video on the device, in front of everything else (pafuse_amd.tracks; ops.track_people):
    ``kps`` [N,K,J,2] the candidate detections of every frame in no stable order (:func:`load_pifpaf_people`), ``conf``
    [N,K,J].  Nothing is normalised here: the cost of a link is the distance a person moved in units of their own size, so
    pixels and screen-normalised coordinates give the same tracks up to rounding.  Returns a dict of CPU tensors: ``"x2d"``
    [M,N,J,2] and ``"conf"`` [M,N,J], one video per person, best first - ``x2d[m]``, ``conf[m]`` go straight into
    :func:`screen_detections`, :func:`repair_detections` and :func:`infer_sequence`; a frame without the person is zeros with
    confidence 0 - ``"assign"`` [M,N] int32 (the candidate followed, -1 nobody), ``"score"`` [M] float64 (NaN: no such track)
    and ``"frames"`` [M] int32.  ``seed`` = (frame, candidate) follows that detection's person (tracks = 1).  The parameters
    are defaults, not tuned values.  Position only: identities can switch where two people cross; a person gone for more
    than ``max_gap - 1`` frames comes back as a new track."""
    from . import ops
    kps = torch.as_tensor(kps, dtype=torch.float32)
    conf = torch.as_tensor(conf, dtype=torch.float32)
    if kps.dim() != 4 or kps.shape[-1] != 2 or tuple(conf.shape) != tuple(kps.shape[:3]):
        raise ValueError(f"kps must be [N,K,J,2] and conf [N,K,J], got {tuple(kps.shape)} and {tuple(conf.shape)}")
    return _run_on(kps, device, lambda dev: ops.track_people(kps.to(dev).contiguous(), conf.to(dev).contiguous(), tracks=tracks, seed=seed,
                                                             gate=gate, skip=skip, max_gap=max_gap, support=support,
                                                             min_frames=min_frames, threshold=threshold))


def stitch_clips(prediction, total_frames, frames=27):
    """[clips, T, P, frames, J, 3] (clips cut by :func:`cut_clips`) -> [T, P, total_frames, J, 3]: consecutive clips laid
    end to end, the last one contributing only its final `total_frames - frames * (clips - 1)` frames
    (in_the_wild/h3wb_diffusion.py:118-131).  Sequences shorter than one clip keep their first total_frames frames."""
    clips, T, P, _, J, c = prediction.shape
    out = prediction.new_empty(T, P, total_frames, J, c)
    if total_frames <= frames:
        return prediction[0, :, :, :total_frames].clone()
    for i in range(clips - 1):
        out[:, :, i * frames:(i + 1) * frames] = prediction[i]
    left = total_frames - (clips - 1) * frames
    out[:, :, -left:] = prediction[-1, :, :, -left:]
    return out


def stitch_poses(poses, total_frames, frames=27):
    """[clips, T, frames, J, 3] aggregated poses (clips cut by :func:`cut_clips`) -> [T, total_frames, J, 3], by the rule of
    :func:`stitch_clips`: consecutive clips end to end, the last one contributing only its final frames."""
    return stitch_clips(poses.unsqueeze(2), total_frames, frames).squeeze(1)


def stitch_spread(spread, total_frames, frames=27):
    """[clips, T, frames, J] per-joint std or [clips, T, frames, J, 6] covariance (clips cut by :func:`cut_clips`) ->
    [T, total_frames, J] / [T, total_frames, J, 6], by the rule of :func:`stitch_poses`."""
    if spread.dim() == 4:
        return stitch_clips(spread[:, :, None, :, :, None], total_frames, frames)[:, 0, :, :, 0]
    return stitch_clips(spread.unsqueeze(2), total_frames, frames).squeeze(1)


def camera_to_world(X, R, t=0.0):
    """Rotate points [..., 3] by the unit quaternion R (w, x, y, z) and translate (common/camera.py:27-28,
    common/quaternion.py:3-17: v + 2 (w (q x v) + q x (q x v)))."""
    R = torch.as_tensor(R, dtype=X.dtype, device=X.device)
    q = R[1:].expand(X.shape)
    uv = torch.cross(q, X, dim=-1)
    uuv = torch.cross(q, uv, dim=-1)
    return X + 2 * (R[0] * uv + uuv) + t


def read_checkpoint(path):
    """``torch.load`` for the reference's checkpoint files (``best_epoch.bin`` / ``pafuse_model.bin``, written by
    common/logging.py:83-115) and for the ones :func:`pafuse_amd.h3wb.save_state` writes.  Besides tensors they hold
    ``random_state``, a pickled ``numpy.random.RandomState`` (main_h3wb.py:1047), which the ``weights_only=True``
    default of torch >= 2.6 refuses - so the file is loaded with ``weights_only=False`` (only open files you trust,
    as with the reference)."""
    return torch.load(path, map_location="cpu", weights_only=False)


def load_checkpoint(model, checkpoint):
    """Accept what the reference saves (common/logging.py:83-115): a dict with 'model_pos', DataParallel
    ``module.``-prefixed keys, or a bare state dict - or the path of such a file (:func:`read_checkpoint`).
    A ``train_stream`` entry (written by :func:`pafuse_amd.h3wb.save_state` for ``train_draws = "device"``) puts a training
    model back where the saved run stood in noise stream v1: the next forward draws what the uninterrupted run would have."""
    if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "__fspath__"):
        checkpoint = read_checkpoint(checkpoint)
    stream = checkpoint.get("train_stream") if isinstance(checkpoint, dict) else None
    if stream is not None and getattr(model, "is_train", False) and hasattr(model, "train_call"):
        model.noise_seed = int(stream["seed"])
        model.train_call = int(stream["call"])
    sd = checkpoint.get("model_pos", checkpoint) if isinstance(checkpoint, dict) else checkpoint
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    return model.load_state_dict(sd)


@torch.no_grad()
def evaluate_sequence(model, dataset, seq_2d, seq_3d, cam, kps_left, kps_right, batch_size=1024, group=None, p2=False,
                      gather="hypotheses", hypothesis_chunk=None, p2_gather="hypotheses"):
    """One (camera, sequence) item of evaluate()'s loop (main_h3wb.py:261-396).

    seq_2d [N,J,2] normalised 2-D input, seq_3d [N,J,3] camera-space ground truth (metres), cam [9] intrinsics.
    Returns ``(sums, n)``: the 14 accumulators [T] already multiplied by the batch multiplier (clips x frames), and
    the multiplier total - add them over sequences and report ``sums[k] / n * 1000`` mm, like :func:`report`.
    ``p2=True`` adds the four Protocol #2 accumulators (ACCUMULATORS_P2, the reference's ``ft2d.p2``).
    With torch.distributed initialised the hypothesis axis is sharded and gathered (pafuse_amd.parallel).
    The model is taken as it is configured: with ``model.noise = "device"`` (and a ``noise_seed``) the hypotheses come from the
    library's counter-based stream, the same for every world size, batch size and hypothesis chunk, and no noise is allocated.

    ``gather="hypotheses"`` (default): every rank receives all P hypotheses and evaluates them in one kernel.
    ``gather="partials"``: every rank reduces its own hypotheses to partial reductions and the ranks exchange those
    (evaluate.evaluate_accumulators_sharded): neither the [B,T,P,F,J,3] tensor nor per-hypothesis error maps exist
    anywhere.  ``hypothesis_chunk=n`` (partials only) also samples and reduces the rank's hypotheses n at a time, so peak
    memory follows n instead of P; the numbers do not depend on n.  Protocol #1 comes from the partials.

    ``p2_gather`` says where ``p2=True`` takes Protocol #2 from when ``gather="partials"``.  ``"hypotheses"`` (default): the
    chunks are kept and gathered, and the Protocol #2 kernel runs on all P hypotheses of every rank - the four p2_* vectors
    are those of gather="hypotheses" bit for bit, and the memory saving is lost.  ``"partials"`` (needs ``p2=True`` and
    ``gather="partials"``): every chunk is also folded into a 16-byte-per-(clip,t,f,j) Protocol #2 state
    (evaluate.accumulate_procrustes) and dropped; the states travel in the same all-gather as the Protocol #1 states (56
    bytes per (clip,t,f,j) plus the per-hypothesis tails per rank) and no rank ever holds all hypotheses.  p2_j_best and
    p2_j_agg are then still bit-equal to the default; p2_p_best and p2_p_agg differ from it by fp64 roundings (their sums
    are taken in another order), and of the four only p2_p_agg depends on how the hypotheses are cut into ranks and chunks,
    in the last bit."""
    if gather not in ("hypotheses", "partials"):
        raise ValueError(f'gather must be "hypotheses" or "partials", got {gather!r}')
    if hypothesis_chunk is not None and (gather != "partials" or int(hypothesis_chunk) < 1):
        raise ValueError('hypothesis_chunk is a positive count and needs gather="partials"')
    if p2_gather not in ("hypotheses", "partials"):
        raise ValueError(f'p2_gather must be "hypotheses" or "partials", got {p2_gather!r}')
    if p2_gather == "partials" and not (p2 and gather == "partials"):
        raise ValueError('p2_gather="partials" needs p2=True and gather="partials"')
    dev = next(model.parameters()).device
    seq_2d = torch.as_tensor(seq_2d, dtype=torch.float32)
    seq_3d = torch.as_tensor(seq_3d, dtype=torch.float32)
    x2d = cut_clips(seq_2d, model.frames).to(dev)
    x2d_flip = cut_clips(flip_2d(seq_2d, kps_left, kps_right), model.frames).to(dev)
    gt = cut_clips(seq_3d, model.frames).to(dev)
    traj = gt[:, :, :1].clone()                                   # main_h3wb.py:300
    gt_parts = center_pose_parts(gt, dataset)                     # main_h3wb.py:304
    cam = torch.as_tensor(cam, dtype=torch.float32).to(dev)
    sampler = ShardedSampler(model, group)
    sums, n = None, 0
    for lo in range(0, x2d.shape[0], batch_size):
        hi = min(lo + batch_size, x2d.shape[0])
        if gather == "partials":
            acc = _accumulators_from_partials(sampler, dataset, x2d[lo:hi], x2d_flip[lo:hi], gt_parts[lo:hi], traj[lo:hi], cam,
                                              hypothesis_chunk, p2, p2_gather)
        else:
            pred = sampler(x2d[lo:hi], gt_parts[lo:hi], input_2d_flip=x2d_flip[lo:hi])      # [b,T,P,F,J,3]
            acc = evaluate_accumulators(pred, gt_parts[lo:hi], x2d[lo:hi], traj[lo:hi], cam, dataset, p2=p2)
        mult = (hi - lo) * model.frames                           # main_h3wb.py:333
        sums = {k: mult * v for k, v in acc.items()} if sums is None else {k: sums[k] + mult * acc[k] for k in acc}
        n += mult
    return sums, n


def _accumulators_from_partials(sampler, dataset, x2d, x2d_flip, gt_parts, traj, cam, hypothesis_chunk, p2, p2_gather="hypotheses"):
    """One batch of clips through sample -> reduce, chunk by chunk, then one exchange of the states."""
    from .evaluate import (accumulate_procrustes, gather_partial_states, protocol2_accumulators,
                           protocol2_accumulators_sharded)
    from .parallel import gather_hypotheses
    p2_partials = p2 and p2_gather == "partials"
    state, p2_state, kept = None, None, []
    for pred, h0, _ in sampler.sample_chunks(x2d, gt_parts, input_2d_flip=x2d_flip, chunk=hypothesis_chunk):
        state = accumulate_partials(state, pred, h0, gt_parts, x2d, traj, cam, dataset)
        if p2_partials:
            p2_state = accumulate_procrustes(p2_state, pred, h0, gt_parts, x2d, traj, cam, dataset)
        elif p2:
            kept.append(pred)
        del pred
    P = sampler.model.num_proposals
    if p2_partials:       # both states of every rank in ONE all-gather; no hypothesis is kept or exchanged
        gathered = gather_partial_states(state, P, sampler.group, p2_state=p2_state)
        acc = evaluate_accumulators_sharded(None, None, P, gt_parts, x2d, traj, cam, dataset, state=gathered)
        acc.update(protocol2_accumulators_sharded(None, gathered, P, gt_parts, dataset))
        return acc
    acc = evaluate_accumulators_sharded(None, None, P, gt_parts, x2d, traj, cam, dataset, group=sampler.group, state=state)
    if p2:
        full = gather_hypotheses(torch.cat(kept, dim=2) if len(kept) > 1 else kept[0], P, sampler.group)
        acc.update(protocol2_accumulators(full, gt_parts, x2d, traj, cam, dataset))
    return acc


def report(sums, n):
    """mm per protocol and step, as evaluate() prints them (main_h3wb.py:415-509)."""
    return {k: (v / n * 1000.0).tolist() for k, v in sums.items()}


def format_report(rep, test_time_augmentation=True, action=None):
    """The reference's evaluation log, line for line (main_h3wb.py:406-509): returns ``(printed, written)`` - the lines
    evaluate() prints and the lines it appends to ``h36m_test_log_H<P>_K<T>.txt`` (the reference prints P_Best but
    does not write it, and writes each part-based header twice; both quirks are kept so files diff clean).  When ``rep``
holds the p2_* keys, each step ends with the four Protocol #2 lines (:511-519): printed as ``print(fmt % ii, value,
'mm')`` prints them (``str`` of the value), written with ``%f``, P_Best written too."""
    printed, written = [], []

    def both(line):
        printed.append(line), written.append(line)

    if action is None:
        printed.append("----------")
    else:
        both("----" + action + "----")
    printed.append(f"Test time augmentation: {test_time_augmentation}")
    for ii in range(len(rep["j_best"])):
        hands = lambda key: (rep[key + "_right_hand"][ii] + rep[key + "_left_hand"][ii]) / 2.
        both("step %d : Protocol #1 Error (MPJPE) J_Best: %f mm" % (ii, rep["j_best"][ii]))
        printed.append("step %d : Protocol #1 Error (MPJPE) P_Best: %f mm" % (ii, rep["p_best"][ii]))
        both("step %d : Protocol #1 Error (MPJPE) P_Agg: %f mm" % (ii, rep["p_agg"][ii]))
        both("step %d : Protocol #1 Error (MPJPE) J_Agg: %f mm" % (ii, rep["j_agg"][ii]))
        for header, key, name in (("-----------------> Part-Based Evaluation <-----------------", "p_best_pb", "P_Best"),
                                  ("-----------------> Part-Based Evaluation Aggregation <-----------------", "p_agg_pb",
                                   "P_Agg")):
            both(header)
            written.append(header)
            both("step %d : Protocol #1 Error (MPJPE) %s Part-Based: %f mm" % (ii, name, rep[key][ii]))
            both("step %d : Protocol #1 Error (MPJPE) %s Part-Based BODY: %f mm" % (ii, name, rep[key + "_body"][ii]))
            both("step %d : Protocol #1 Error (MPJPE) %s Part-Based FACE: %f mm" % (ii, name, rep[key + "_face"][ii]))
            both("step %d : Protocol #1 Error (MPJPE) %s Part-Based HANDS: %f mm" % (ii, name, hands(key)))
            both("step %d : Protocol #1 Error (MPJPE) %s Part-Based LEFT HAND: %f mm" % (ii, name, rep[key + "_left_hand"][ii]))
            both("step %d : Protocol #1 Error (MPJPE) %s Part-Based RIGHT HAND: %f mm" % (ii, name, rep[key + "_right_hand"][ii]))
        if "p2_j_best" in rep:
            for key, name in (("p2_j_best", "J_Best"), ("p2_p_best", "P_Best"), ("p2_p_agg", "P_Agg"), ("p2_j_agg", "J_Agg")):
                head = "step %d : Protocol #2 Error (MPJPE) %s:" % (ii, name)
                printed.append(" ".join((head, str(rep[key][ii]), "mm")))
                written.append("%s %f mm" % (head, rep[key][ii]))
    both("----------")
    return printed, written


# ----------------------------------------------------------------- the per-frame output scored against ground truth
@torch.no_grad()
def evaluate_frames(model, dataset, seq_2d, seq_3d, cam, kps_left, kps_right, aggregate="mean", stride=None, trajectory=None,
                    conf=None, batch_size=2, group=None, hypothesis_chunk=None, p2=False, per_frame=False, focal=None, repair=None,
                    drop=None, repair_threshold=0.0, path_weight=None, path_scope="clip", pose_smooth=None, pose_smooth_floor=1e-3,
                    bone_lengths=None, bone_iterations=16, corrupt=None, swap=None, screen=None, screen_gate=4.0, screen_floor=0.005,
                    distract=None, track=False, ground=None, ground_speed=0.015):
    """One video scored at the level of frames: the frames path of :func:`infer_sequence` - ONE pose per video frame, pooled
    over the windows that cover it - against the ground truth, on the device before anything crosses to the host
    (evaluate.frame_metrics; pafuse_amd.framemetrics states the arithmetic).

    seq_2d [N,J,2] normalised 2-D input, seq_3d [N,J,3] camera-space ground truth (metres), cam [9] intrinsics.  ``aggregate``:
    "mean", "reproj" or "reproj_fit" as in infer_sequence; "reproj" takes its trajectory from the ground truth root, as the
    reference's J-Agg does; "reproj_fit" and ``trajectory`` use ``cam`` only.  ``stride``: 1 .. model.frames; None means
    model.frames - un-strided clips laid end to end.  ``trajectory`` (True, or a smoothing radius 1 .. 64) also fits the
    camera-space root and scores it: root, root_vel, abs_mpjpe.  ``conf`` [N,J] with "reproj_fit" or a trajectory.

    Returns ``(sums, counts)``: dicts of CPU tensors [T], float64 and int64, keyed by evaluate.frame_metric_names plus
    "mpjpe_pb" (and "p_mpjpe" with ``p2=True``) - add them over videos and hand them to :func:`frame_report`.
    ``per_frame=True`` returns ``(sums, counts, maps)``, maps = {"err" [T,N,K] float64, "cnt" [T,N,K] int32, "names"}: the
    same per frame, what :func:`seam_profile` bins.  On synthetic weights the numbers mean nothing.

    ``focal="estimate"`` (with ``trajectory``): the root is fitted and scored with the ESTIMATED focal length (``cam`` gives the
    principal point, aspect and distortion terms), and the estimate is returned as one more, last element: a dict of CPU
    tensors ``"focal"``, ``"focal_r2"``, ``"focal_frames"`` [T] and ``"cam"`` [T,9], to be compared with cam[0].

    ``drop=(rate, run, seed)`` (None: everything above, unchanged) loses detections on purpose - ground-truth 2-D has no
    dropouts, so without it nobody can measure what a repair is worth: detections.plant_dropouts(N, J, rate, run, seed) marks
    the lost (frame, joint)s, which get detections.DROPPED_XY and confidence 0; every other joint keeps ``conf`` (None: 1).
    ``repair`` (a radius 1 .. 64; needs ``conf`` or ``drop``) then repairs the detections as infer_sequence(repair=...) does,
    before the model sees them.  With either, one more, last element is returned: a dict of CPU tensors ``"x2d"`` [N,J,2] and
    ``"conf"`` [N,J] as the model and the fits saw them, ``"lost"`` [N,J] bool with ``drop`` and ``"status"`` [N,J] uint8 with
    ``repair`` - what detections.repair_error takes.

    ``corrupt=(rate, run, size, seed)`` and ``swap=(rate, run, seed)`` (None: everything above, unchanged) plant WRONG detections
    with their confidence kept, on the clean detections and before any ``drop``: detscreen.corrupt with the mirror pairs of
    ``kps_left`` / ``kps_right`` - runs of detections displaced by ``size`` (a length or a (lo, hi) range, screen units) and runs
    of left/right pairs exchanged; ``conf`` None counts as 1.  ``screen`` (a radius 1 .. 64; needs ``conf``, ``corrupt``, ``swap``
    or ``drop``) then screens the detections as infer_sequence(screen=...) does, before the repair.  The extra dict gains
    ``"planted_out"`` / ``"planted_swap"`` [N,J] bool with ``corrupt`` or ``swap`` and ``"screened"`` [N,J] uint8 with ``screen`` -
    what detscreen.screen_error takes - and its ``"x2d"`` / ``"conf"`` are what the model and the fits saw.

    ``distract=(people, seed)`` (None: everything above, unchanged) plants OTHER PEOPLE, first of all: tracks.plant_people adds
    ``people`` shifted copies of the subject and draws a new order of the people + 1 slots in every frame - what a detector's
    list of a frame with several people looks like; ``conf`` None counts as 1.  With ``track=False`` slot 0 of every frame is
    lifted - what a caller that takes ``predictions[0]`` lifts: a splice of the subject and the copies; with ``track=True`` (or
    a dict of :func:`track_people`'s parameters) the candidates are linked on the device and track 0 is lifted.  Everything
    else (corrupt, swap, drop, screen, repair) then sees that one video.  The extra dict gains ``"tracked"`` [N] int32, the
    slot lifted in every frame (-1: nobody), and ``"truth_slot"`` [N] int32, the subject's - what tracks.track_error takes.

    ``path_weight`` (with "reproj" or "reproj_fit", un-strided clips and no hypothesis_chunk; None: everything above, unchanged)
    scores the pick made coherent in time, infer_sequence(path_weight=...): per clip and joint one path through the hypotheses.
    Where the last window overlaps its predecessor the fold's first-minimum rule decides between the two paths, frame by frame.
    The ``mpjpe`` and ``accel`` columns show what a weight buys.  ``path_scope="video"`` scores the path along the whole video
    instead, infer_sequence(path_weight=..., path_scope="video"): any ``stride``, the candidates of a frame being the
    hypotheses of all windows that cover it, so nothing is left to the fold's rule; the hypotheses of all windows stay on
    the device until the end of the video, and at most 256 candidates per frame are taken.

    ``pose_smooth`` (a radius 1 .. 64; None: everything above, unchanged) scores the pose SMOOTHED along the frames with the
    covariance of the hypotheses as matrix weight, infer_sequence(pose_smooth=..., pose_smooth_floor=...): the ``mpjpe`` and
    ``accel`` columns show what a radius buys, and the trajectory is fitted on the smoothed pose.

    ``bone_lengths`` ("video", "symmetric" or a tensor [J] or [T,J]; None: everything above, unchanged) and ``bone_iterations``
    score the pose with its BONE LENGTHS HELD CONSTANT along the video, infer_sequence(bone_lengths=..., bone_iterations=...):
    the existing ``mpjpe`` / ``accel`` columns score it, the trajectory is fitted on it.  One more, last element is returned, a
    dict of CPU tensors: ``"bone_length"`` [J] the lengths held at the last step, ``"bone_length_gt"`` [J] the same kernel on
    the ground truth (a [1,N,J,3] pose without a covariance; NaN: no bone), and ``"bone_dev_free"`` / ``"bone_dev"`` [T]: the
    mean over the bones of the bone-length standard deviation, in mm, of the free and of the constrained pose.

    ``ground`` (True, or a radius 1 .. 64; with ``trajectory``; None: everything above, unchanged) and ``ground_speed`` also find
    the ground plane of the video, infer_sequence(ground=..., ground_speed=...), behind the trajectory fit.  The metrics are not
    changed by it; one more, last element is returned, a dict of CPU tensors with infer_sequence's ground keys (GROUND_KEYS)."""
    got = _evaluate_frames(model, dataset, seq_2d, seq_3d, cam, kps_left, kps_right, aggregate=aggregate, conf=conf, batch_size=batch_size,
                           group=group, p2=p2, per_frame=per_frame, drop=drop, corrupt=corrupt, swap=swap, distract=distract, track=track,
                           stride=stride, trajectory=trajectory, hypothesis_chunk=hypothesis_chunk, focal=focal, repair=repair,
                           repair_threshold=repair_threshold, path_weight=path_weight, path_scope=path_scope, pose_smooth=pose_smooth,
                           pose_smooth_floor=pose_smooth_floor, bone_lengths=bone_lengths, bone_iterations=bone_iterations, screen=screen,
                           screen_gate=screen_gate, screen_floor=screen_floor, ground=ground, ground_speed=ground_speed)
    return tuple(v for v in got if v is not None)      # the documented shape: the optional elements in the fields' order


class _FrameScores(NamedTuple):
    """evaluate_frames' result by name; what the options did not ask for is None"""
    sums: dict
    counts: dict
    maps: object = None         # per_frame=True
    estimate: object = None     # focal="estimate": the focal keys
    seen: object = None         # a planting, screen or repair: the detections as the model saw them
    held: object = None         # bone_lengths: the lengths held beside the ground truth's
    found: object = None        # ground: GROUND_KEYS


@torch.no_grad()
def _evaluate_frames(model, dataset, seq_2d, seq_3d, cam, kps_left, kps_right, *, aggregate="mean", conf=None, batch_size=2, group=None,
                     p2=False, per_frame=False, drop=None, corrupt=None, swap=None, distract=None, track=False, **options):
    """evaluate_frames with its result named (_FrameScores); `options`: the options it shares with infer_sequence, as _frame_plan
    takes them"""
    if drop is not None:
        if (not isinstance(drop, (tuple, list)) or len(drop) != 3 or not 0.0 <= float(drop[0]) <= 1.0
                or isinstance(drop[1], bool) or int(drop[1]) != drop[1] or int(drop[1]) < 1):
            raise ValueError(f"drop must be (rate in 0 .. 1, run >= 1 frames, seed), got {drop!r}")
    if distract is not None and (not isinstance(distract, (tuple, list)) or len(distract) != 2 or isinstance(distract[0], bool)
                                 or int(distract[0]) != distract[0] or not 1 <= int(distract[0]) <= 63):
        raise ValueError(f"distract must be (people in 1 .. 63, seed), got {distract!r}")
    if track is not False and distract is None:
        raise ValueError("track needs distract: ground-truth 2-D holds one person, there is nobody to tell apart")
    if not isinstance(track, (bool, dict)):
        raise ValueError(f"track must be False, True or a dict of track_people's parameters, got {track!r}")
    planting = corrupt is not None or swap is not None
    for name, spec, k in (("corrupt", corrupt, 4), ("swap", swap, 3)):
        if spec is not None and (not isinstance(spec, (tuple, list)) or len(spec) != k or not 0.0 <= float(spec[0]) <= 1.0
                                 or isinstance(spec[1], bool) or int(spec[1]) != spec[1] or int(spec[1]) < 1):
            raise ValueError(f"{name} must be (rate in 0 .. 1, run >= 1 frames, {'size, ' if k == 4 else ''}seed), got {spec!r}")
    plan = _frame_plan(getattr(model, "frames", None), dataset, kps_left, kps_right, cam=cam, traj=None, conf=conf, aggregate=aggregate,
                       frames_only=True, conf_made=drop is not None or planting or distract is not None, **options)
    seq_2d = torch.as_tensor(seq_2d, dtype=torch.float32)
    seq_3d = torch.as_tensor(seq_3d, dtype=torch.float32)
    if seq_2d.dim() != 3 or seq_2d.shape[-1] != 2 or tuple(seq_3d.shape) != (*seq_2d.shape[:2], 3):
        raise ValueError(f"seq_2d must be [N,J,2] and seq_3d [N,J,3], got {tuple(seq_2d.shape)} and {tuple(seq_3d.shape)}")
    conf = _conf_operand(conf, seq_2d.shape[:2])
    from .evaluate import frame_metrics
    dev = next(model.parameters()).device
    seen = None
    if distract is not None:
        from .tracks import plant_people
        crowd = plant_people(seq_2d.numpy(), torch.ones(seq_2d.shape[:2]).numpy() if conf is None else conf.numpy(), int(distract[0]) + 1,
                             seed=distract[1])
        if track is False:
            tracked = torch.zeros(seq_2d.shape[0], dtype=torch.int32)
            seq_2d, conf = torch.from_numpy(crowd["x2d"][:, 0].copy()), torch.from_numpy(crowd["conf"][:, 0].copy())
        else:
            found = track_people(crowd["x2d"], crowd["conf"], device=dev, **(track if isinstance(track, dict) else {}))
            tracked, seq_2d, conf = found["assign"][0], found["x2d"][0].contiguous(), found["conf"][0].contiguous()
        seen = {"tracked": tracked, "truth_slot": torch.from_numpy(crowd["truth"][0])}
    if planting:
        from .detscreen import corrupt as plant_wrong, mirror_table
        wrong = plant_wrong(seq_2d.numpy(), torch.ones(seq_2d.shape[:2]).numpy() if conf is None else conf.numpy(),
                            mirror_table(kps_left, kps_right, seq_2d.shape[1]),
                            outliers=None if corrupt is None else (float(corrupt[0]), int(corrupt[1]), corrupt[2], corrupt[3]),
                            swaps=None if swap is None else (float(swap[0]), int(swap[1]), swap[2]))
        seq_2d, conf = torch.from_numpy(wrong["x2d"]), torch.from_numpy(wrong["conf"])
        seen = {**(seen or {}), "planted_out": torch.from_numpy(wrong["planted_out"]), "planted_swap": torch.from_numpy(wrong["planted_swap"])}
    if drop is not None:
        from .detections import DROPPED_XY, plant_dropouts
        lost = torch.from_numpy(plant_dropouts(seq_2d.shape[0], seq_2d.shape[1], float(drop[0]), int(drop[1]), drop[2]))
        seq_2d = torch.where(lost.unsqueeze(-1), torch.tensor(DROPPED_XY, dtype=torch.float32), seq_2d)
        conf = torch.where(lost, torch.zeros(()), torch.ones(lost.shape) if conf is None else conf)
        seen = {**(seen or {}), "lost": lost}
    seq_2d, conf, screened, repaired = _front_end(seq_2d, conf, plan, dataset, kps_left, kps_right, dev)
    if screened is not None:
        seen = {**(seen or {}), "screened": screened}
    if repaired is not None:
        seen = {**(seen or {}), "status": repaired}
    if seen is not None:
        seen.update(x2d=seq_2d, conf=conf)
    gt_root = seq_3d[:, 0].contiguous()                             # [N,3]
    gt_wb = (seq_3d - seq_3d[:, :1]).to(dev)                        # joint 0 at 0, exactly
    out = _infer_frames_device(model, dataset, seq_2d, kps_left, kps_right, plan, cam=cam, traj=gt_root if aggregate == "reproj" else None,
                               conf=conf, batch_size=batch_size, group=group, dev=dev)
    found = {k: out[k].cpu() for k in GROUND_KEYS} if plan.ground is not None else None
    estimate = {k: out[k].cpu() for k in ("focal", "focal_r2", "focal_frames", "cam")} if plan.focal is not None else None
    bones, held = plan.bones, None
    if bones is not None:           # the lengths held beside the ground truth's, and what the constraint did to the known diagnostic
        from . import ops
        parent, mirror = bones["tables"]
        mirror = mirror if isinstance(bones["lengths"], str) and bones["lengths"] == "symmetric" else None
        gt_length = ops.bone_lengths(gt_wb.unsqueeze(0).contiguous(), None, parent, mirror, floor=bones["floor"])
        _, dev_after = ops.bone_lengths(out["pose"], None, parent, mirror, floor=bones["floor"], want_dev=True)
        held = {"bone_length": out["bone_length"][-1].cpu(), "bone_length_gt": gt_length[0].cpu(),
                "bone_dev_free": (out["bone_dev"].double().nanmean(dim=1) * 1000.0).cpu(),
                "bone_dev": (dev_after.double().nanmean(dim=1) * 1000.0).cpu()}
    m = frame_metrics(out["pose"], gt_wb, dataset, traj=out.get("traj"), gt_root=gt_root.to(dev) if "traj" in out else None,
                      p2=p2, per_frame=per_frame)
    maps = {k: m.pop(k).cpu() for k in ("err", "cnt") if k in m}
    sums, counts = {k: v[0].cpu() for k, v in m.items()}, {k: v[1].cpu() for k, v in m.items()}
    if per_frame:
        from .evaluate import frame_metric_names
        maps["names"] = frame_metric_names(dataset)
    return _FrameScores(sums, counts, maps if per_frame else None, estimate, seen, held, found)


FRAME_UNITS = {"mpjve": "mm/frame", "root_vel": "mm/frame", "accel": "mm/frame^2"}     # every other metric: mm


def frame_report(sums, counts):
    """mm per metric and step from the sums and counts of :func:`evaluate_frames` (added over the videos): sum / count * 1000;
    mm/frame for mpjve and root_vel, mm/frame^2 for accel (FRAME_UNITS); NaN where nothing was counted."""
    return {k: (sums[k].double() / counts[k].double() * 1000.0).tolist() for k in sums}


def format_frame_report(rep, action=None):
    """The lines of a frame-level report, step by step, in the style of :func:`format_report`."""
    lines = ["----------" if action is None else "----" + action + "----"]
    for ii in range(len(rep["mpjpe"])):
        for k in rep:
            lines.append("step %d : Frame Error (%s): %f %s" % (ii, k.upper(), rep[k][ii], FRAME_UNITS.get(k, "mm")))
    lines.append("----------")
    return lines


def seam_bins(err, cnt, frames, slot=0):
    """-> (sums, counts) float64 [T, frames]: err[t, n, slot] and cnt[t, n, slot] added over n = i mod frames; what
    :func:`seam_profile` divides, kept apart so that several videos can be added first"""
    err = torch.as_tensor(err, dtype=torch.float64).cpu()
    cnt = torch.as_tensor(cnt).cpu()
    frames = int(frames)
    if err.dim() != 3 or tuple(cnt.shape) != tuple(err.shape) or not 0 <= int(slot) < err.shape[2] or frames < 1:
        raise ValueError("seam_profile: err and cnt are [T,N,K] maps, slot one of the K, frames >= 1")
    T, N, _ = err.shape
    bins = (torch.arange(N) % frames).expand(T, N)
    s = torch.zeros(T, frames, dtype=torch.float64).scatter_add_(1, bins, err[:, :, slot])
    c = torch.zeros(T, frames, dtype=torch.float64).scatter_add_(1, bins, cnt[:, :, slot].double())
    return s, c


def seam_profile(err, cnt, frames, slot=0):
    """The per-frame maps of evaluate_frames(per_frame=True) binned by the position in the clip: err, cnt [T,N,K] ->
    float64 [T, frames], entry (t, i) = sum of err[t, n, slot] over n = i mod frames / the sum of cnt there (NaN where nothing
    was counted), in the maps' unit (metres).  With stride = frames the ends of the profile are the clip seams - a border frame
    has temporal context on one side only; compare with a stride < frames.  Host-side."""
    s, c = seam_bins(err, cnt, frames, slot)
    return s / c

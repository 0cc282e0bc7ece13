"""H3WB data plumbing on the caller side of the hot path: the npz loader with root-joint
insertion and camera normalisation, the per-camera sequence list evaluate() iterates, and the evaluation driver.

Mirrors, for a user who has ``data/train_h3wb.npz`` + ``data/task1_test_3d.npz`` and ``pafuse_model.bin``:
  Human3WBDataset            reference common/h3wb_dataset.py:14-213 (attributes D3DP and evaluate() read)
  prepare_keypoints / fetch  reference main_h3wb.py:57-119,621-648 (mm -> m, screen normalisation, per-camera lists)
  iter_sequences             reference common/generators.py:174-249 (UnchunkedGenerator_Seq.next_epoch, no augmentation)
  evaluate                   reference main_h3wb.py:194-531 (the loop around model_eval + the mm report)
  ChunkedClips               reference common/generators.py:5-172 (ChunkedGenerator_Seq: the shuffled, flip-augmented
                             27-frame training clips)
  train_epoch / save_state   reference main_h3wb.py:820-870,1018-1040, common/logging.py:83-115
Host-side numpy; nothing here touches the device except through pafuse_amd.harness.evaluate_sequence.
"""
import copy
import json
import os

import numpy as np

KPS_ORDER = ("body", "left_foot", "right_foot", "face", "left_hand", "right_hand")
CAMERA_ORDER = ("54138969", "55011271", "58860488", "60457274")
ROOT_INDICES = {"body": 0, "face": 54, "left_hand": 92, "right_hand": 113}
PARTS_CONNECTION_INDICES = {"face": 1, "left_hand": 10, "right_hand": 11}
_CAMERA_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "h36m_cameras.json")


def normalize_screen_coordinates(X, w, h):
    """[0, w] -> [-1, 1], aspect ratio kept (reference common/camera.py:7-11)."""
    assert X.shape[-1] == 2
    return X / w * 2 - [1, h / w]


class Skeleton:
    """Parent table + left/right joint lists (the part of common/skeleton.py the evaluation path reads)."""

    def __init__(self, parents, joints_left, joints_right):
        self._parents = np.array(parents)
        self._joints_left, self._joints_right = list(joints_left), list(joints_right)

    def num_joints(self):
        return len(self._parents)

    def parents(self):
        return self._parents

    def joints_left(self):
        return self._joints_left

    def joints_right(self):
        return self._joints_right


def _hand_parents(wrist, body_wrist):
    """21 hand keypoints: the wrist hangs on the body's wrist joint, five 4-joint finger chains hang on the wrist."""
    out = [body_wrist]
    for finger in range(5):
        first = wrist + 4 * finger + 1
        out += [wrist, first, first + 1, first + 2]
    return out


def skeleton_parents(n_face, root_added):
    """Parent index of every keypoint in H3WB order (body, feet, face, hands), reference h3wb_dataset.py:137-161."""
    feet = [15] * 3 + [16] * 3
    hands = _hand_parents(91, 9) + _hand_parents(112, 10)
    if root_added:
        body = [-1] * 6 + [0, 0, 6, 7, 8, 9, 0, 0, 12, 13, 14, 15]          # inserted root first; head points free
        face = [-1] * n_face
        feet, hands = [p + 1 for p in feet], [p + 1 for p in hands]
    else:
        body = [-1, 0, 0, 0, 0, 0, 0, 5, 6, 7, 8, 5, 6, 11, 12, 13, 14]
        face = [0] * n_face
    return body + feet + face + hands


def bone_tables(dataset_or_n_face=68, root_added=True, left=None, right=None):
    """-> (parent int32 [J], mirror int32 [J]): the tables of the bone-length constraint (pafuse_amd.bones, DESIGN.md section
    6n).  ``parent[j]`` is the joint that joint j's bone hangs on, or -1 for no bone - the body's real topology, a list of our
    own, unlike :func:`skeleton_parents`, which leaves the head points free for drawing: the nose hangs on the root, eyes
    and ears on the nose, shoulders and hips on the root, elbow on shoulder, wrist on elbow, knee on hip, ankle on knee, the
    three foot points on their ankle, the hands as :func:`_hand_parents` has them (depth 8 from the root to a fingertip).
    The face points get -1 and are not touched: carried with the nose they would take on the noise of its correction, and an
    expression changes their distances anyway.  Every parent index is smaller than its child's - the kernels rely on that.
    Without the inserted root the nose is the top and shoulders and hips hang as in ``skeleton_parents(n_face, False)``.
    ``mirror[j]`` is the left/right partner of joint j, or -1: ``left`` / ``right`` paired by position when given, else the
    ``joints_left()`` / ``joints_right()`` of a dataset that has a ``skeleton()``, else the layout's own pairs (body and feet
    alternate left, right; the left hand's points mirror the right hand's).  ``dataset_or_n_face``: such a dataset, any object
    with ``parts_joint_indices["face"]``, or the number of face points."""
    ds = dataset_or_n_face
    if isinstance(ds, (int, np.integer)) and not isinstance(ds, bool):
        n_face = int(ds)
    elif hasattr(ds, "parts_joint_indices"):
        n_face = len(ds.parts_joint_indices["face"])
    else:
        n_face = len(ds.metadata["face"])
    if n_face < 0:
        raise ValueError(f"bone_tables: the number of face points must be >= 0, got {n_face}")
    s = 1 if root_added else 0
    head = [-1, 0, 1, 1, 1, 1] if root_added else [-1, 0, 0, 0, 0]               # (root,) nose, eyes, ears
    limbs = ([0, 0, 6, 7, 8, 9, 0, 0, 12, 13, 14, 15] if root_added              # shoulders, elbows, wrists, hips, knees, ankles
             else [0, 0, 5, 6, 7, 8, 5, 6, 11, 12, 13, 14])
    feet = [15 + s] * 3 + [16 + s] * 3
    lh, rh = 23 + n_face, 44 + n_face                                            # the hands' wrists before the root shift
    hands = [p + s for p in _hand_parents(lh, 9) + _hand_parents(rh, 10)]
    parent = np.array(head + limbs + feet + [-1] * n_face + hands, dtype=np.int32)
    J = len(parent)
    assert all(-1 <= parent[j] < j for j in range(J))
    if left is None and right is None and hasattr(ds, "skeleton"):
        left, right = ds.skeleton().joints_left(), ds.skeleton().joints_right()
    if left is None and right is None:
        body = list(range(1, 17, 2))                                             # left eye, ear, shoulder, ... ankle (no root shift)
        left = [j + s for j in body + [17, 18, 19] + list(range(lh, lh + 21))]
        right = [j + s for j in [b + 1 for b in body] + [20, 21, 22] + list(range(rh, rh + 21))]
    if left is None or right is None or len(left) != len(right):
        raise ValueError("bone_tables: left and right come together and pair by position")
    mirror = np.full(J, -1, dtype=np.int32)
    for a, b in zip(left, right):
        if not (0 <= a < J and 0 <= b < J and a != b):
            raise ValueError(f"bone_tables: the pair ({a}, {b}) is not two joints of {J}")
        mirror[a], mirror[b] = b, a
    return parent, mirror


def foot_points(dataset_or_root_added=True):
    """-> int32 [6]: the toe and heel points of both feet, what the ground estimate takes as foot points (pafuse_amd.ground,
    DESIGN.md section 6q): keypoints 17 .. 22 of the H3WB order (left big toe, small toe, heel; right likewise), 18 .. 23 with
    the inserted root.  NOT the ankles: they ride about 8 cm above the floor.  ``dataset_or_root_added``: True / False, or a
    dataset of this package - they all carry the inserted root (134 joints)."""
    ds = dataset_or_root_added
    root_added = bool(ds) if isinstance(ds, (bool, np.bool_)) else True
    s = 1 if root_added else 0
    return np.arange(17 + s, 23 + s, dtype=np.int32)


def with_root_joint(arr, hips=(11, 12)):
    """[N,133,c] -> [N,134,c] (float64, like the reference's np.zeros buffer): keypoint 0 = midpoint of the hips."""
    out = np.zeros((arr.shape[0], arr.shape[1] + 1, arr.shape[2]))
    out[:, 1:, :] = arr
    out[:, :1, :] = (arr[:, hips[0]:hips[0] + 1, :] + arr[:, hips[1]:hips[1] + 1, :]) / 2.
    return out


def load_cameras():
    """Per-subject camera list as the reference builds it (h3wb_dataset.py:101-121): H36M extrinsics + the four shared
    intrinsics, centre/focal length in normalised screen units, translation in metres, 9-float 'intrinsic' vector."""
    with open(_CAMERA_FILE) as f:
        table = json.load(f)
    cameras = copy.deepcopy(table["extrinsic"])
    for cams in cameras.values():
        for i, cam in enumerate(cams):
            cam.update(table["intrinsic"][i])
            for k, v in cam.items():
                if k not in ("id", "res_w", "res_h"):
                    cam[k] = np.array(v, dtype="float32")
            cam["center"] = normalize_screen_coordinates(cam["center"], w=cam["res_w"], h=cam["res_h"]).astype("float32")
            cam["focal_length"] = cam["focal_length"] / cam["res_w"] * 2
            if "translation" in cam:
                cam["translation"] = cam["translation"] / 1000
            cam["intrinsic"] = np.concatenate((cam["focal_length"], cam["center"], cam["radial_distortion"],
                                               cam["tangential_distortion"]))
    return cameras


class Human3WBDataset:
    """H3WB as PAFUSE reads it: ``Human3WBDataset('data/train_h3wb.npz')`` (the S8 test split is read from
    ``task1_test_3d.npz`` in the same directory)."""

    def __init__(self, path, add_root=True):
        blob = np.load(path, allow_pickle=True)
        self.metadata = blob["metadata"].item()
        data = blob["train_data"].item()
        test = np.load(os.path.join(os.path.dirname(path), "task1_test_3d.npz"), allow_pickle=True)["data"].item()
        data.update(test)

        shift = 1 if add_root else 0
        both = set(self.metadata["left_side"]) & set(self.metadata["right_side"])
        joints_left = [k + shift for k in self.metadata["left_side"] if k not in both]
        joints_right = [k + shift for k in self.metadata["right_side"] if k not in both]
        self.kps_order = list(KPS_ORDER)
        self.parents = skeleton_parents(len(self.metadata["face"]), add_root)
        self.root_indices = dict(ROOT_INDICES)
        self.parts_connection_indices = dict(PARTS_CONNECTION_INDICES)
        self.num_kps = len(self.parents)
        self.keypoints_metadata = {"layout_name": "h3wb", "num_joints": self.num_kps,
                                   "keypoints_symmetry": [joints_left, joints_right]}
        self._skeleton = Skeleton(self.parents, joints_left, joints_right)
        self._fps = 50
        self._cameras = load_cameras()
        self.camera_order_id = list(CAMERA_ORDER)

        self._data, self._cameras_full_data = {}, {}
        for subject, actions in data.items():
            cams = [self.metadata[subject][c] for c in self.camera_order_id]
            self._cameras_full_data[subject] = cams
            self._data[subject] = {}
            for action, rec in actions.items():
                def arr(a):
                    return with_root_joint(a) if add_root else a
                self._data[subject][action] = {
                    "positions": arr(rec["global_3d"]).squeeze(),
                    "cameras": list(cams),
                    "positions_3d": [arr(rec[c]["camera_3d"]).squeeze() for c in self.camera_order_id],
                    "pose_2d": [arr(rec[c]["pose_2d"]).squeeze() for c in self.camera_order_id],
                }
        # part -> joint indices after the root shift; the feet belong to the body part (h3wb_dataset.py:198-213)
        shifted = {p: [k + 1 for k in self.metadata[p]] for p in KPS_ORDER}
        self.parts_joint_indices = {
            "body": [0] + shifted["body"] + shifted["left_foot"] + shifted["right_foot"],
            "face": shifted["face"], "left_hand": shifted["left_hand"], "right_hand": shifted["right_hand"]}

    def __getitem__(self, subject):
        return self._data[subject]

    def subjects(self):
        return self._data.keys()

    def fps(self):
        return self._fps

    def skeleton(self):
        return self._skeleton

    def cameras(self):
        return self._cameras

    def supports_semi_supervised(self):
        return True


def prepare_keypoints(dataset):
    """main_h3wb.py:621-648: camera-space 3-D from millimetres to metres, 2-D keypoints to normalised screen
    coordinates of their camera (both in place, as the reference does).  Returns keypoints[subject][action][cam]."""
    keypoints = {}
    for subject in dataset.subjects():
        keypoints[subject] = {}
        for action, anim in dataset[subject].items():
            if "positions" in anim:
                anim["positions_3d"] = [p / 1000. for p in anim["positions_3d"]]
            per_cam = []
            for cam_idx, kps in enumerate(anim["pose_2d"]):
                cam = dataset.cameras()[subject][cam_idx]
                kps[..., :2] = normalize_screen_coordinates(kps[..., :2], w=cam["res_w"], h=cam["res_h"])
                per_cam.append(kps)
            keypoints[subject][action] = per_cam
    return keypoints


def fetch(subjects, keypoints, dataset, stride=1, action_filter=None, parse_3d_poses=True):
    """main_h3wb.py:57-119 without the `subset` sampling: flat per-(subject, action, camera) lists of camera
    intrinsics, 3-D and 2-D sequences, optionally strided."""
    cams, poses_3d, poses_2d = [], [], []
    for subject in subjects:
        for action, per_cam in keypoints[subject].items():
            if action_filter is not None and not any(action.startswith(a) for a in action_filter):
                continue
            poses_2d += list(per_cam)
            if subject in dataset.cameras():
                subject_cams = dataset.cameras()[subject]
                assert len(subject_cams) == len(per_cam), "Camera count mismatch"
                cams += [c["intrinsic"] for c in subject_cams if "intrinsic" in c]
            if parse_3d_poses and "positions_3d" in dataset[subject][action]:
                seqs = dataset[subject][action]["positions_3d"]
                assert len(seqs) == len(per_cam), "Camera count mismatch"
                poses_3d += list(seqs)
    if stride > 1:
        poses_2d = [p[::stride] for p in poses_2d]
        poses_3d = [p[::stride] for p in poses_3d]
    return (cams or None), (poses_3d or None), poses_2d


def fetch_orientations(subjects, keypoints, dataset, action_filter=None):
    """The camera-to-world quaternion (w, x, y, z) of every video, in the order of :func:`fetch`'s lists; None for a camera
    that carries no orientation."""
    out = []
    for subject in subjects:
        for action, per_cam in keypoints[subject].items():
            if action_filter is not None and not any(action.startswith(a) for a in action_filter):
                continue
            subject_cams = dataset.cameras().get(subject, [])
            for i in range(len(per_cam)):
                q = subject_cams[i].get("orientation") if i < len(subject_cams) else None
                out.append(None if q is None else np.asarray(q, dtype=np.float64))
    return out


def camera_up(orientation):
    """the world's up (0, 0, 1) in the camera space of a camera whose camera-to-world rotation is the unit quaternion
    `orientation` (w, x, y, z): rotated by its inverse (the reference's world_to_camera, common/camera.py)"""
    import torch
    from .harness import camera_to_world
    q = np.asarray(orientation, dtype=np.float64)
    return camera_to_world(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), q * np.array([1.0, -1.0, -1.0, -1.0])).numpy()


def up_angle(a, b):
    """the angle between two directions, degrees (NaN for a NaN direction)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.rad2deg(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))))


def iter_sequences(cams, poses_3d, poses_2d):
    """One (cam [1,9], seq_3d [1,N,J,3], seq_2d [1,N,J,2]) triple per video, batch axis added, no augmentation."""
    from itertools import zip_longest
    for c, p3, p2 in zip_longest(cams or [], poses_3d or [], poses_2d):
        yield (None if c is None else np.expand_dims(c, 0), None if p3 is None else np.expand_dims(p3, 0),
               np.expand_dims(p2, 0))


def evaluate(model, dataset, cams, poses_3d, poses_2d, kps_left, kps_right, batch_size=1024, group=None, log=print,
             action=None, log_dir=None, p2=False, gather="hypotheses", hypothesis_chunk=None, p2_gather="hypotheses"):
    """evaluate() of main_h3wb.py:194-531 for an already loaded eval model: every video through
    harness.evaluate_sequence (flip-TTA, 27-frame clips, sharded sampling, device-side aggregation), frame-weighted
    means in millimetres per protocol and sampling step, printed in the reference's log format (:406-509) and, with
    `log_dir`, appended to ``h36m_test_log_H<P>_K<T>.txt`` there exactly as the reference writes it.  `action` is
    the per-action header of the reference's run_evaluation loop (:1117-1362): call once per action's sequences.
    ``p2=True`` (``ft2d.p2``) adds Protocol #2 (P-MPJPE after similarity alignment) to the numbers and the log.
    ``gather`` / ``hypothesis_chunk``: harness.evaluate_sequence's - "partials" evaluates Protocol #1 from per-shard
    partial reductions (optionally sampling the hypotheses a chunk at a time) instead of gathering all P hypotheses.
    ``p2_gather``: harness.evaluate_sequence's - "partials" (with p2=True and gather="partials") takes Protocol #2 from
    per-shard partial states too, so that no rank ever holds all hypotheses."""
    from . import harness
    total, n = None, 0
    for cam, seq_3d, seq_2d in iter_sequences(cams, poses_3d, poses_2d):
        sums, cnt = harness.evaluate_sequence(model, dataset, seq_2d[0].astype("float32"), seq_3d[0].astype("float32"),
                                              cam[0].astype("float32"), kps_left, kps_right, batch_size, group, p2=p2,
                                              gather=gather, hypothesis_chunk=hypothesis_chunk, p2_gather=p2_gather)
        total = sums if total is None else {k: total[k] + sums[k] for k in sums}
        n += cnt
    rep = harness.report(total, n)
    printed, written = harness.format_report(rep, bool(model.flip), action)
    for line in printed:
        log(line)
    if log_dir is not None:
        import os
        path = os.path.join(log_dir, "h36m_test_log_H%d_K%d.txt" % (model.num_proposals, model.sampling_timesteps))
        with open(path, mode="a") as f:
            f.write("".join(line + "\n" for line in written))
    return rep


def evaluate_frames(model, dataset, cams, poses_3d, poses_2d, kps_left, kps_right, aggregate="mean", stride=None, trajectory=None,
                    batch_size=2, group=None, log=print, action=None, hypothesis_chunk=None, p2=False, seam_profile=False, focal=None,
                    repair=None, drop=None, repair_threshold=0.0, path_weight=None, path_scope="clip", pose_smooth=None,
                    pose_smooth_floor=1e-3, bone_lengths=None, bone_iterations=16, corrupt=None, swap=None, screen=None,
                    screen_gate=4.0, screen_floor=0.005, distract=None, track=False, ground=None, ground_speed=0.015, orientations=None):
    """The frame-level evaluation of every video, looped like :func:`evaluate`: harness.evaluate_frames per (camera, sequence) -
    one pose per video frame (``aggregate``, ``stride``; None: un-strided clips laid end to end), optionally its fitted
    camera-space root (``trajectory``: True or a smoothing radius) - scored on the device; the sums and counts added over the
    videos; millimetres per metric and sampling step (harness.frame_report) printed through `log` in the lines of
    harness.format_frame_report.  ``seam_profile=True`` also keeps the per-frame maps and logs the position error binned by the
    frame's position in the clip (harness.seam_profile, summed over the videos); the return value is then ``(rep, profile)``,
    profile float64 [T, model.frames] in mm.  ``focal="estimate"`` (with ``trajectory``) fits and scores the root with the focal
    length estimated from each video (harness.estimate_focal) and logs, per video, the estimate of every step beside the true
    cam[0], with r2 and the frames it rests on.  ``drop=(rate, run, seed)`` loses detections of the ground-truth 2-D on purpose
    (detections.plant_dropouts with seed + the video's number; DROPPED_XY, confidence 0, else 1) and ``repair`` (a radius
    1 .. 64, with ``drop``) repairs them on the device before the model sees them (harness.evaluate_frames); per video the
    joints per status are logged and, with both, detections.repair_error: the RMS 2-D distance of the filled and of the
    unfilled joints from the detections that were dropped, overall and per part.  ``path_weight`` (with "reproj" / "reproj_fit" on
    un-strided clips) scores the pick made coherent in time (harness.evaluate_frames); ``path_scope="video"`` scores one path along the
    whole video instead, at any ``stride``.  ``pose_smooth`` (a radius 1 .. 64, ``pose_smooth_floor`` metres) scores the pose
    smoothed along the frames with the covariance of the hypotheses as matrix weight (harness.evaluate_frames): compare the
    ``mpjpe`` and ``accel`` lines with a run without it - what the smoother buys on a real checkpoint has not been measured.
    ``bone_lengths`` ("video" or "symmetric"; ``bone_iterations`` Jacobi sweeps) scores the pose with its bone lengths held
    constant along each video (harness.evaluate_frames): per video the mean bone-length standard deviation of the free and of
    the constrained pose and the largest difference of the held lengths from the ground truth's are logged - what it buys on
    a real checkpoint has not been measured either.
    ``corrupt=(rate, run, size, seed)`` and ``swap=(rate, run, seed)`` plant wrong detections with their confidence kept - displaced
    runs and exchanged left/right pairs (detscreen.corrupt, seed + the video's number) - and ``screen`` (a radius 1 .. 64;
    ``screen_gate``, ``screen_floor``) screens the detections on the device before the repair (harness.evaluate_frames); per
    video the detections per screen status are logged and, with a planting, detscreen.screen_error: the planted outliers and
    swaps found and missed and the false rejects and swaps, overall and per part.  Whether the screen lowers the 3-D error needs
    a real checkpoint and has not been measured.
    ``distract=(people, seed)`` plants that many other people - shifted copies of the subject - and a new order of the slots in
    every frame (tracks.plant_people, seed + the video's number); slot 0 is then lifted, what ``predictions[0]`` gives on such a
    file, or with ``track=True`` (a dict: harness.track_people's parameters) track 0 of the device tracker; per video
    tracks.track_error of what was lifted is logged.  What the tracker buys in 3-D error needs a real checkpoint and has not
    been measured.
    ``ground`` (True or a radius 1 .. 64, with ``trajectory``; ``ground_speed`` metres per frame) also finds the ground plane of
    every video from its resting feet (harness.evaluate_frames(ground=...)) and logs, per video and step, the code, the camera
    height and the number of contact points of the prediction, and the same estimator run on the GROUND-TRUTH 3-D (which needs
    no checkpoint).  ``orientations`` (:func:`fetch_orientations`: one camera-to-world quaternion per video, or None) adds the
    angle between each estimated up and the camera's true up.  The defaults are not tuned values; what the estimate is worth on
    a real checkpoint has not been measured - that angle is the tool for it.
    On synthetic weights the numbers mean nothing."""
    import torch
    from . import detections, detscreen, harness, tracks
    if distract is not None and (not isinstance(distract, (tuple, list)) or len(distract) != 2):
        raise ValueError(f"distract must be (people, seed), got {distract!r}")
    if drop is not None and (not isinstance(drop, (tuple, list)) or len(drop) != 3):
        raise ValueError(f"drop must be (rate, run, seed), got {drop!r}")
    if corrupt is not None and (not isinstance(corrupt, (tuple, list)) or len(corrupt) != 4):
        raise ValueError(f"corrupt must be (rate, run, size, seed), got {corrupt!r}")
    if swap is not None and (not isinstance(swap, (tuple, list)) or len(swap) != 3):
        raise ValueError(f"swap must be (rate, run, seed), got {swap!r}")
    sums = counts = prof_s = prof_c = None
    for video, (cam, seq_3d, seq_2d) in enumerate(iter_sequences(cams, poses_3d, poses_2d)):
        got = harness._evaluate_frames(model, dataset, seq_2d[0].astype("float32"), seq_3d[0].astype("float32"),
                                       cam[0].astype("float32"), kps_left, kps_right, aggregate=aggregate, stride=stride,
                                       trajectory=trajectory, batch_size=batch_size, group=group,
                                       hypothesis_chunk=hypothesis_chunk, p2=p2, per_frame=seam_profile, focal=focal, repair=repair,
                                       drop=None if drop is None else (drop[0], drop[1], int(drop[2]) + video),
                                       repair_threshold=repair_threshold, path_weight=path_weight, path_scope=path_scope,
                                       pose_smooth=pose_smooth, pose_smooth_floor=pose_smooth_floor, bone_lengths=bone_lengths,
                                       bone_iterations=bone_iterations,
                                       corrupt=None if corrupt is None else (corrupt[0], corrupt[1], corrupt[2], int(corrupt[3]) + video),
                                       swap=None if swap is None else (swap[0], swap[1], int(swap[2]) + video), screen=screen,
                                       screen_gate=screen_gate, screen_floor=screen_floor,
                                       distract=None if distract is None else (distract[0], int(distract[1]) + video), track=track,
                                       ground=ground, ground_speed=ground_speed)       # named: what an option did not ask for is None
        found, held, seen, est = got.found, got.held, got.seen, got.estimate
        if found is not None:
            gt = torch.as_tensor(seq_3d[0].astype("float32"))
            truth = harness.estimate_ground((gt - gt[:, :1]).unsqueeze(0), gt[:, 0].unsqueeze(0), radius=3 if ground is True else ground,
                                            speed=ground_speed)
            true_up = None if orientations is None or orientations[video] is None else camera_up(orientations[video])
            off = lambda up: "n/a" if true_up is None else "%.3f" % up_angle(up, true_up)
            for t in range(found["up"].shape[0]):
                log("video %d step %d : ground code %d, camera height %.3f m, %d contact points, angle to the camera's true up %s deg"
                    % (video, t, int(found["ground_code"][t]), float(found["camera_height"][t]), int(found["ground_points"][t]), off(found["up"][t])))
            log("video %d ground truth 3-D : ground code %d, camera height %.3f m, %d contact points, angle to the camera's true up %s deg"
                % (video, int(truth["ground_code"][0]), float(truth["camera_height"][0]), int(truth["ground_points"][0]), off(truth["up"][0])))
        if held is not None:
            gap = (held["bone_length"].double() - held["bone_length_gt"].double()).abs()
            log("video %d: bone-length std (mm, mean over the bones) free %s -> constrained %s; held lengths vs ground truth: max %.1f mm"
                % (video, ["%.2f" % v for v in held["bone_dev_free"].tolist()], ["%.2f" % v for v in held["bone_dev"].tolist()],
                   float(gap[~gap.isnan()].max()) * 1000.0 if bool((~gap.isnan()).any()) else float("nan")))
        if seen is not None:
            if "tracked" in seen:
                e = tracks.track_error(seen["tracked"].numpy(), seen["truth_slot"].numpy())
                log("video %d : %s among %d people: the subject's detection in %d frames, another person's in %d, nobody in %d, %d switches"
                    % (video, "track 0" if track is not False else "slot 0", int(distract[0]) + 1, e["right"], e["wrong"], e["missed"], e["switches"]))
            if "screened" in seen:
                log("video %d : detections accepted %d, rejected %d, swapped %d, not observed %d"
                    % ((video,) + tuple(detscreen.counts(seen["screened"].numpy()))))
                if "planted_out" in seen:
                    err = detscreen.screen_error(seen["screened"].numpy(), seen["planted_out"].numpy(), seen["planted_swap"].numpy(),
                                                 parts=dataset.parts_joint_indices)
                    for name, e in [("all", err)] + list(err["parts"].items()):
                        log("video %d : screen error %s: outliers found %d, missed %d, false rejects %d of %d untouched; "
                            "swapped detections found %d, missed %d, false swaps %d"
                            % (video, name, e["out_found"], e["out_missed"], e["false_rejects"], e["untouched"], e["swap_found"],
                               e["swap_missed"], e["false_swaps"]))
            elif "planted_out" in seen:
                log("video %d : %d outliers and %d swapped detections planted, none screened"
                    % (video, int(seen["planted_out"].sum()), int(seen["planted_swap"].sum())))
            if "status" in seen:
                log("video %d : detections observed %d, filled %d, held %d, unfilled %d" % ((video,) + tuple(detections.counts(seen["status"].numpy()))))
            if "status" in seen and "lost" in seen:
                err = detections.repair_error(seq_2d[0].astype("float32"), seen["x2d"].numpy(), seen["lost"].numpy(), seen["status"].numpy(),
                                              parts=dataset.parts_joint_indices)
                for name, e in [("all", err)] + list(err["parts"].items()):
                    log("video %d : repair error %s: filled %f over %d joints, unfilled %f over %d (RMS, screen-normalised units)"
                        % (video, name, e["filled"], e["n_filled"], e["unfilled"], e["n_unfilled"]))
            elif "lost" in seen:
                log("video %d : %d detections dropped, none repaired" % (video, int(seen["lost"].sum())))
        if est is not None:
            for t in range(est["focal"].shape[0]):
                log("video %d step %d : estimated focal length %f (true %f, ratio %f), r2 %f over %d frames"
                    % (video, t, float(est["focal"][t]), float(cam[0][0]), float(est["focal"][t]) / float(cam[0][0]),
                       float(est["focal_r2"][t]), int(est["focal_frames"][t])))
        sums = got.sums if sums is None else {k: sums[k] + got.sums[k] for k in sums}
        counts = got.counts if counts is None else {k: counts[k] + got.counts[k] for k in counts}
        if seam_profile:       # the sums and the counts of the bins add over videos; the quotient is formed once
            s, c = harness.seam_bins(got.maps["err"], got.maps["cnt"], model.frames)
            prof_s, prof_c = (s, c) if prof_s is None else (prof_s + s, prof_c + c)
    rep = harness.frame_report(sums, counts)
    for line in harness.format_frame_report(rep, action):
        log(line)
    if not seam_profile:
        return rep
    profile = prof_s / prof_c * 1000.0
    for t in range(profile.shape[0]):
        log("step %d : MPJPE by position in the clip (mm): %s" % (t, " ".join("%.3f" % v for v in profile[t].tolist())))
    return rep, profile


class ChunkedClips:
    """Training batches: every video cut into `chunk_length`-frame clips centred on the video (the overhang split
    between both ends and filled by repeating the edge frame), each clip optionally a second time mirrored (x negated,
    left/right keypoints swapped, camera centre/tangential x negated), all (video, start, end, flip) items shuffled
    per epoch by a RandomState(1234) and served `batch_size` clips at a time.  Same item list, same permutation call,
    same buffers' dtype (float64) as the reference's ChunkedGenerator_Seq."""

    def __init__(self, batch_size, cameras, poses_3d, poses_2d, chunk_length, shuffle=True, random_seed=1234,
                 augment=False, kps_left=None, kps_right=None, joints_left=None, joints_right=None, shard=None):
        assert poses_3d is None or len(poses_3d) == len(poses_2d)
        assert cameras is None or len(cameras) == len(poses_2d)
        items = []
        for i, seq in enumerate(poses_2d):
            n = seq.shape[0]
            assert poses_3d is None or poses_3d[i].shape[0] == n
            n_chunks = (n + chunk_length - 1) // chunk_length
            offset = (n_chunks * chunk_length - n) // 2
            bounds = np.arange(n_chunks + 1) * chunk_length - offset
            # the reference zips len(bounds) flags with len(bounds) - 1 intervals: zip stops at the shorter list
            plain = np.full(len(bounds), False, dtype=bool)
            items += zip(np.repeat(i, len(bounds)), bounds[:-1], bounds[1:], plain)
            if augment:
                items += zip(np.repeat(i, len(bounds)), bounds[:-1], bounds[1:], ~plain)
        self.pairs, self.batch_size, self.chunk_length = items, batch_size, chunk_length
        self.num_batches = (len(items) + batch_size - 1) // batch_size
        self.random = np.random.RandomState(random_seed)
        self.shuffle, self.augment = shuffle, augment
        self.cameras, self.poses_3d, self.poses_2d = cameras, poses_3d, poses_2d
        self.kps_left, self.kps_right = kps_left, kps_right
        self.joints_left, self.joints_right = joints_left, joints_right
        # shard = (rank, world): one process per GPU.  Every rank keeps the reference's item list, seed and GLOBAL
        # batches (so an epoch is one pass and model.batch_size is the global batch, as with the reference's
        # nn.DataParallel, main_h3wb.py:699-705) and serves clips rank, rank + world, ... of each batch.
        self.shard = shard
        self.last_share = None

    def batch_num(self):
        return self.num_batches

    def num_frames(self):
        return self.num_batches * self.batch_size

    def random_state(self):
        return self.random

    def set_random_state(self, random):
        self.random = random

    def _clip(self, seq, start, end):
        lo, hi = max(start, 0), min(end, seq.shape[0])
        clip = seq[lo:hi]
        if lo != start or hi != end:
            clip = np.pad(clip, ((lo - start, end - hi), (0, 0), (0, 0)), "edge")
        return clip

    def next_epoch(self):
        pairs = self.random.permutation(self.pairs) if self.shuffle else self.pairs
        for b in range(self.num_batches):
            chunk = pairs[b * self.batch_size:(b + 1) * self.batch_size]
            if self.shard is not None:
                rank, world = self.shard
                n_global, chunk = len(chunk), chunk[rank::world]
                self.last_share = (len(chunk), n_global, world)
                if len(chunk) == 0:            # fewer clips than ranks: keep the collective's call count, weight 0
                    chunk = pairs[b * self.batch_size:b * self.batch_size + 1]
            n = len(chunk)
            b2 = np.empty((n, self.chunk_length) + self.poses_2d[0].shape[-2:])
            b3 = None if self.poses_3d is None else np.empty((n, self.chunk_length) + self.poses_3d[0].shape[-2:])
            bc = None if self.cameras is None else np.empty((n, self.cameras[0].shape[-1]))
            for i, (seq_i, start, end, flip) in enumerate(chunk):
                seq_i, start, end = int(seq_i), int(start), int(end)
                b2[i] = self._clip(self.poses_2d[seq_i], start, end)
                if flip:
                    b2[i, :, :, 0] *= -1
                    b2[i, :, self.kps_left + self.kps_right] = b2[i, :, self.kps_right + self.kps_left]
                if b3 is not None:
                    b3[i] = self._clip(self.poses_3d[seq_i], start, end)
                    if flip:
                        b3[i, :, :, 0] *= -1
                        b3[i, :, self.joints_left + self.joints_right] = b3[i, :, self.joints_right + self.joints_left]
                if bc is not None:
                    bc[i] = self.cameras[seq_i]
                    if flip:
                        bc[i, 2] *= -1
                        bc[i, 7] *= -1
            yield bc, b3, b2


# per-joint loss weights of model.weighted_loss (main_h3wb.py:724-727: 18 body weights "from MixSTE", 1.0 for the rest)
WEIGHTED_LOSS_HEAD = (1, 1, 1, 1, 1, 1, 1.5, 1.5, 4, 4, 4, 4, 1, 1, 2.5, 2.5, 2.5, 2.5)


def mpjpe_loss(predicted, target, weights=None, mse_loss=False):
    """The training loss, common/loss.py:9-27 (`mpjpe` without return_joints_err): mean joint distance, optionally
    per-joint weighted and/or squared.  Plain torch on the caller's side of the boundary, as in the reference."""
    import torch
    assert predicted.shape == target.shape
    err = torch.norm(predicted - target, dim=len(target.shape) - 1)
    if weights is not None:
        assert weights.shape[0] == target.shape[-2]
        err = weights[None, None, :].to(predicted.device) * err
    return torch.mean(torch.square(err)) if mse_loss else torch.mean(err)


def train_epoch(model, optimizer, generator, dataset, device, wb_loss=False, log=None, mse_loss=False,
                weighted_loss=False):
    """One epoch of main_h3wb.py:820-870: part-centred targets, train-mode D3DP forward (HIP), mpjpe loss
    (`model.mse_loss` / `model.weighted_loss` variants included, :724-727,:859), backward (HIP), optimizer step.
    `model` may be wrapped in DistributedDataParallel: with a rank-sharded generator (``ChunkedClips(..., shard=(rank,
    world))``) every rank holds its slice of the reference's global batch and the local loss is weighted by
    n_local * world / n_global, so the all-reduced (averaged) gradient is the gradient of the global-batch mean - what
    the reference's DataParallel computes on the gathered batch.  Returns the clip-weighted mean loss (m)."""
    import torch
    from . import harness
    total, frames = 0.0, 0
    weights = None
    if weighted_loss:
        J = dataset.skeleton().num_joints() if hasattr(dataset, "skeleton") else 134
        weights = torch.tensor(list(WEIGHTED_LOSS_HEAD) + [1.0] * (J - len(WEIGHTED_LOSS_HEAD)), device=device)
    module = model.module if hasattr(model, "module") else model
    if getattr(module, "train_draws", "torch") == "device":
        # the rank's clips are clips rank, rank + world, ... of the global batch: their draws follow the GLOBAL index
        module.train_clips = tuple(getattr(generator, "shard", None) or (0, 1))
    for it, (_, batch_3d, batch_2d) in enumerate(generator.next_epoch()):
        inputs_3d = torch.from_numpy(batch_3d.astype("float32")).to(device)
        inputs_2d = torch.from_numpy(batch_2d.astype("float32")).to(device)
        inputs_3d = harness.center_pose_parts(inputs_3d, dataset)
        optimizer.zero_grad()
        pred = model(inputs_2d, inputs_3d)
        target = inputs_3d
        if wb_loss:
            pred, target = harness.wb_pose_from_parts(pred, dataset), harness.wb_pose_from_parts(inputs_3d, dataset)
        loss = mpjpe_loss(pred, target, weights, mse_loss)                              # common/loss.py:9-27
        share = getattr(generator, "last_share", None)        # (clips that count here, clips of the global batch, world)
        n_local = inputs_3d.shape[0]
        scale = 1.0
        if share is not None:
            n_local, n_global, world = share
            scale = n_local * world / n_global
        (loss * scale if scale != 1.0 else loss).backward()
        optimizer.step()
        n = n_local * inputs_3d.shape[1]
        total, frames = total + n * float(loss.detach()), frames + n
        if log is not None and it % 10 == 0:
            log("%d/%d" % (it, generator.batch_num()))
    return total / max(frames, 1)


def save_state(model, optimizer, epoch_no, lr, foldername, random_state=None, tag=None, reference_layout=True):
    """The reference's checkpoint dictionary (common/logging.py:83-115): evaluate() and --resume read it back.

    The reference always saves the state dict of an ``nn.DataParallel`` wrapper (main_h3wb.py:699-705,1029), so its
    'model_pos' keys carry a ``module.`` prefix and its loaders expect one (:252 strict, :713-714).  With
    ``reference_layout`` (default) the file written here has exactly those keys whether or not `model` is wrapped
    (DataParallel / DistributedDataParallel), so checkpoints are interchangeable with the reference in both directions
    (``harness.load_checkpoint`` strips the prefix); ``reference_layout=False`` writes bare keys.

    A model that draws on the device (``train_draws = "device"``) adds ``train_stream: {"seed", "call"}``, from which
    ``harness.load_checkpoint`` lets a resumed run continue the sequence; the file of a default run keeps its exact key set."""
    import torch
    module = model.module if hasattr(model, "module") else model
    sd = module.state_dict()
    if reference_layout:
        sd = type(sd)(("module." + k, v) for k, v in sd.items())
    params = {"optimizer": optimizer.state_dict(), "epoch": epoch_no, "lr": lr, "model_pos": sd}
    if random_state is not None:
        params["random_state"] = random_state
    if getattr(module, "train_draws", "torch") == "device":
        params["train_stream"] = {"seed": int(module.noise_seed), "call": int(module.train_call)}
    fname = f"{foldername}/{tag or f'epoch_{epoch_no}'}.bin"
    torch.save(params, fname)
    return fname

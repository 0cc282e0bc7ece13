"""ctypes binding of libpafuse_hip.so (the C ABI declared in include/pafuse_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no CPU fallback: if the
shared object is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpafuse_hip.so")   # the in-tree build; no environment variable selects another one

MAX_DEPTH = 16
MAX_PARTS = 4
f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)


BLOCK_FIELDS = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b",
                "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


class BlockWeights(C.Structure):
    _names = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b",
              "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
              "qkv_ws", "proj_ws", "fc1_ws", "fc2_ws",
              "qkv_ls", "qkv_lt", "fc1_ls", "fc1_lt",
              "qkv_hs", "qkv_hb", "qkv_hl", "fc2_hp")
    _fields_ = [(n, C.c_void_p) for n in _names]


class MixSTE2Weights(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("frames", "joints", "channels", "depth", "heads", "in_chans",
                                         "operand_bf16", "mlp_hidden")] + [("qk_scale", C.c_float), ("keep_f32_residual", C.c_int32)] +
                [(n, C.c_void_p) for n in ("patch_w", "patch_b", "pos_spatial", "pos_temporal",
                                           "tm1_w", "tm1_b", "tm3_w", "tm3_b", "freqs",
                                           "snorm_w", "snorm_b", "tnorm_w", "tnorm_b",
                                           "hnorm_w", "hnorm_b", "head_w", "head_b")] +
                [("ste", BlockWeights * MAX_DEPTH), ("tte", BlockWeights * MAX_DEPTH)])


class D3DPConfig(C.Structure):
    _fields_ = [("num_parts", C.c_int32), ("num_kps", C.c_int32), ("frames", C.c_int32), ("flip", C.c_int32),
                ("scale", C.c_double),
                ("part", MixSTE2Weights * MAX_PARTS),
                ("part_joints", C.c_void_p * MAX_PARTS),
                ("joint_part", C.c_void_p), ("joint_local", C.c_void_p), ("flip_perm", C.c_void_p),
                ("part_by_part_launches", C.c_int32)]


class RowLNArgs(C.Structure):
    """pafuse_rowln_args: one whole-row layer (attn.proj / mlp.fc2 + residual + LayerNorm chain) for pafuse_linear_rowln[_group]"""
    _fields_ = ([("M", C.c_int64), ("N", C.c_int32), ("K", C.c_int32), ("operand_bf16", C.c_int32), ("training", C.c_int32)] +
                [(n, C.c_void_p) for n in ("A", "W", "Wsplit", "bias", "resid", "out_x", "out_n", "post_w", "post_b")] +
                [("post_eps", C.c_float), ("pos", C.c_void_p), ("posJ", C.c_int32), ("posF", C.c_int32)] +
                [(n, C.c_void_p) for n in ("next_w", "next_b")] + [("next_eps", C.c_float)] +
                [(n, C.c_void_p) for n in ("head_w", "head_b", "out_head", "ln_stats", "A_img", "resid_img", "out_x_img",
                                           "out_n_img", "rowscale")] +
                [(n, C.c_int32) for n in ("rs_temporal", "rs_J", "rs_FJ")] + [("out_pre", C.c_void_p)])


class LnbArgs(C.Structure):
    """pafuse_lnb_args: one LayerNorm backward of the training step for pafuse_layernorm_backward"""
    _fields_ = ([(n, C.c_void_p) for n in ("dy", "x", "w")] + [("eps", C.c_float)] +
                [(n, C.c_void_p) for n in ("add", "dx", "drop")] + [(n, C.c_int32) for n in ("temporal", "J", "FJ")] +
                [(n, C.c_void_p) for n in ("out_scaled", "dw", "db", "dbranch")] + [("M", C.c_int64), ("C", C.c_int32)])


class EmbedArgs(C.Structure):
    """pafuse_embed_args: one embed launch in any of the sampling loop's output forms, for pafuse_embed_unit"""
    _fields_ = ([(n, C.c_void_p) for n in ("x3d", "x2d", "x2d_flip", "joints", "perm", "patch_w", "patch_b", "pos_spatial", "temb",
                                           "norm_w", "norm_b")] + [("norm_eps", C.c_float)] +
                [(n, C.c_int32) for n in ("B", "P", "F", "J", "J3", "C", "nflip", "do_clamp")] + [("scale", C.c_double)] +
                [(n, C.c_int32) for n in ("operand_bf16", "ln_folded", "h_residual_only")] +
                [(n, C.c_void_p) for n in ("x", "xn", "image", "stats")] + [("row0", C.c_int64), ("nrows", C.c_int64)])


class DDIMStep(C.Structure):
    _fields_ = [("time", C.c_int64), ("last", C.c_int32),
                ("sqrt_recip_acp", C.c_double), ("sqrt_recipm1_acp", C.c_double),
                ("sqrt_alpha_next", C.c_double), ("c", C.c_double), ("sigma", C.c_double)]


# every symbol include/pafuse_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "pafuse_version": (C.c_char_p, []),
    "pafuse_last_error": (C.c_char_p, []),
    "pafuse_abi_version": (C.c_int, []),
    "pafuse_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                C.c_int32, C.c_void_p]),
    "pafuse_split_weights_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "pafuse_split_image_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "pafuse_split_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "pafuse_linear_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_void_p]),
    "pafuse_linear_rowln": (C.c_int, [C.POINTER(RowLNArgs), C.c_void_p]),
    "pafuse_linear_rowln_group": (C.c_int, [C.POINTER(RowLNArgs), C.c_int32, C.c_int32, C.c_void_p]),
    "pafuse_hsplit_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "pafuse_xsplit_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "pafuse_linear_x": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]),
    "pafuse_linear_h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]),
    "pafuse_qkv_attention_image": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_void_p]),
    "pafuse_mlp_h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "pafuse_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                   C.c_void_p]),
    "pafuse_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "pafuse_attention_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "pafuse_linear_weight_grad_bytes": (C.c_size_t, []),
    "pafuse_linear_weight_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_train_unit_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "pafuse_layernorm_backward": (C.c_int, [C.POINTER(LnbArgs), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_linear_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_linear_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_gelu_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "pafuse_train_head_grad_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "pafuse_train_head_grad": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_train_patch_grad_bytes": (C.c_size_t, [C.c_int32] * 4),
    "pafuse_train_patch_grad": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_train_group_sum_bytes": (C.c_size_t, [C.c_int32] * 5),
    "pafuse_train_group_sum": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_train_sinusoid": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p]),
    "pafuse_block_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "pafuse_block_forward": (C.c_int, [C.POINTER(BlockWeights), C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_time_embed": (C.c_int, [C.POINTER(MixSTE2Weights), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "pafuse_mixste2_fused_blocks": (C.c_int, [C.POINTER(MixSTE2Weights)]),
    "pafuse_mode_supported": (C.c_int, [C.c_int32] * 6),
    "pafuse_mixste2_workspace_bytes": (C.c_size_t, [C.POINTER(MixSTE2Weights), C.c_int32, C.c_int32]),
    "pafuse_mixste2_forward": (C.c_int, [C.POINTER(MixSTE2Weights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_d3dp_workspace_bytes": (C.c_size_t, [C.POINTER(D3DPConfig), C.c_int32, C.c_int32]),
    "pafuse_d3dp_sample": (C.c_int, [C.POINTER(D3DPConfig), C.POINTER(DDIMStep), C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32]),
    "pafuse_d3dp_sample_seeded": (C.c_int, [C.POINTER(D3DPConfig), C.POINTER(DDIMStep), C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32]),
    "pafuse_noise_fill": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "pafuse_d3dp_lanes": (C.c_int, [C.POINTER(D3DPConfig), C.c_int32, C.c_int32, C.c_int32]),
    "pafuse_d3dp_range_flag_offset": (C.c_size_t, [C.POINTER(D3DPConfig), C.c_int32, C.c_int32]),
    "pafuse_d3dp_check_range": (C.c_int, [C.POINTER(D3DPConfig), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "pafuse_embed": (C.c_int, [C.c_void_p] * 11 + [C.c_float] + [C.c_int32] * 8 + [C.c_double, C.c_void_p, C.c_void_p,
                                                                                    C.c_void_p]),
    "pafuse_embed_unit": (C.c_int, [C.POINTER(EmbedArgs), C.c_void_p]),
    "pafuse_ddim_finalize": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32] + [C.c_void_p] * 6 +
                             [C.c_int32] * 7 + [C.c_double, C.POINTER(DDIMStep), C.c_void_p]),
    "pafuse_hypothesis_errors": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 5 + [C.c_void_p] * 7),
    "pafuse_hypothesis_partials_bytes": (C.c_size_t, [C.c_int32] * 6),
    "pafuse_hypothesis_partials_workspace_bytes": (C.c_size_t, [C.c_int32] * 6),
    "pafuse_hypothesis_partials": (C.c_int, [C.c_void_p] * 8 + [C.c_int32] * 7 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                                                  C.c_void_p]),
    "pafuse_hypothesis_combine": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t] + [C.c_void_p] * 3 + [C.c_int32] * 5 +
                                  [C.c_void_p] * 6),
    "pafuse_pose_partials_bytes": (C.c_size_t, [C.c_int32] * 4),
    "pafuse_pose_partials": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_pose_partials_fit": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pafuse_pose_combine": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t] + [C.c_int32] * 5 + [C.c_void_p] * 5),
    "pafuse_pose_path_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "pafuse_pose_path": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_double] + [C.c_int32] * 5 +
                         [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "pafuse_frames_path_workspace_bytes": (C.c_size_t, [C.c_int32] * 5 + [C.c_void_p] * 2),
    "pafuse_frames_path": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_double] + [C.c_int32] * 6 +
                           [C.c_void_p] * 10 + [C.c_size_t, C.c_void_p]),
    "pafuse_spread_partials_bytes": (C.c_size_t, [C.c_int32] * 4),
    "pafuse_spread_partials": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_spread_combine": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t] + [C.c_int32] * 4 + [C.c_void_p] * 5),
    "pafuse_frame_pose_state_bytes": (C.c_size_t, [C.c_int32] * 3),
    "pafuse_frame_spread_state_bytes": (C.c_size_t, [C.c_int32] * 3),
    "pafuse_frame_pose_state_init": (C.c_int, [C.c_void_p, C.c_size_t] + [C.c_int32] * 3 + [C.c_void_p]),
    "pafuse_frame_spread_state_init": (C.c_int, [C.c_void_p, C.c_size_t] + [C.c_int32] * 3 + [C.c_void_p]),
    "pafuse_pose_windows_fold": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t] + [C.c_int32] * 4 +
                                 [C.c_void_p] * 4 + [C.c_int32] * 2 + [C.c_void_p]),
    "pafuse_spread_windows_fold": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t] + [C.c_int32] * 4 +
                                   [C.c_void_p] * 5),
    "pafuse_frames_finish": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p] * 7),
    "pafuse_frames_root_fit": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p] * 4),
    "pafuse_trajectory_smooth": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p] * 2),
    "pafuse_detections_repair": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_float] + [C.c_void_p] * 4),
    "pafuse_detections_screen_workspace_bytes": (C.c_size_t, [C.c_int32] * 2),
    "pafuse_detections_screen": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_float] * 3 + [C.c_void_p] * 6 +
                                 [C.c_size_t, C.c_void_p]),
    "pafuse_tracks_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "pafuse_tracks_links": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_float] + [C.c_double] * 2 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pafuse_tracks_path": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 7 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "pafuse_tracks_gather": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p] * 3),
    "pafuse_pose_smooth_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "pafuse_pose_smooth": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_float] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "pafuse_bone_lengths": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_float] + [C.c_void_p] * 4),
    "pafuse_bone_project": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_float] + [C.c_void_p] * 4),
    "pafuse_frames_focal_sums": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p] * 2),
    "pafuse_focal_solve": (C.c_int, [C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p, C.c_int32] + [C.c_void_p] * 5),
    "pafuse_foot_contacts": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_double] + [C.c_void_p] * 4),
    "pafuse_ground_sums": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 3 + [C.c_double] + [C.c_void_p] * 2),
    "pafuse_ground_solve": (C.c_int, [C.c_void_p] + [C.c_int32] * 2 + [C.c_double] * 2 + [C.c_void_p] * 9),
    "pafuse_frames_to_world": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p] * 3),
    "pafuse_frame_errors": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p] * 3),
    "pafuse_frame_errors_reduce": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p] * 3),
    "pafuse_procrustes_errors": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p] * 6),
    "pafuse_procrustes_partials_bytes": (C.c_size_t, [C.c_int32] * 5),
    "pafuse_procrustes_partials_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "pafuse_procrustes_partials": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                                                   C.c_void_p]),
    "pafuse_procrustes_combine": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
                                  + [C.c_int32] * 5 + [C.c_void_p] * 6),
    "pafuse_d3dp_replay_gemms": (C.c_int, [C.POINTER(D3DPConfig), C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.POINTER(C.c_double)]),
    "pafuse_d3dp_replay_layers": (C.c_int, [C.POINTER(D3DPConfig), C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    "pafuse_mixste2_train_bytes": (C.c_size_t, [C.POINTER(MixSTE2Weights), C.c_int32]),
    "pafuse_mixste2_train_forward": (C.c_int, [C.POINTER(MixSTE2Weights), C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]),
    "pafuse_mixste2_train_backward": (C.c_int, [C.POINTER(MixSTE2Weights), C.POINTER(MixSTE2Weights), C.c_void_p,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pafuse_d3dp_qsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                      C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "pafuse_d3dp_qsample_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "pafuse_train_droppath_fill": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
}

# matrix-product modes (include/pafuse_hip.h: pafuse_mixste2_weights.operand_bf16) and the precision names they go by: the one table
MODE_F32, MODE_BF16, MODE_BF16X3, MODE_F16X2, MODE_BF16X3_IMAGES = range(5)
PRECISIONS = {"f32": MODE_F32, "bf16": MODE_BF16, "bf16x3": MODE_BF16X3, "f16x2": MODE_F16X2, "bf16x3_images": MODE_BF16X3_IMAGES}
# ... per split mode, the scheme flag pafuse_split_weights adds to the layout (include/pafuse_hip.h PAFUSE_SPLIT_F16X2, PAFUSE_SPLIT_X),
# and per image mode the bytes per element of an activation image (f16x2 H image, bf16x3 X image)
SPLIT_FLAG = {MODE_BF16X3: 0, MODE_F16X2: 4, MODE_BF16X3_IMAGES: 8}
IMAGE_BYTES = {MODE_F16X2: 4, MODE_BF16X3_IMAGES: 6}

_lib = None

ABI_VERSION = 8      # include/pafuse_hip.h PAFUSE_ABI_VERSION: the struct layouts mirrored above

KERNEL_SOURCES = ("pafuse_amd/csrc/kernels.hpp", "pafuse_amd/csrc/hgemm.hpp", "pafuse_amd/csrc/xgemm.hpp", "pafuse_amd/csrc/sgemm.hpp", "pafuse_amd/csrc/train_kernels.hpp", "pafuse_amd/csrc/pafuse_hip.hip",
                  "pafuse_amd/csrc/train_host.inc", "include/pafuse_hip.h")


def kernel_source_digest():
    """SHA-256 over the native sources the library is built from and the compiler flags.  Measurements kept under
    profiles/ carry it, and bench.py only quotes a committed counter profile whose digest equals the running tree's (the
    GPU box has no .git)."""
    import hashlib
    from .build_flags import HIPCC_FLAGS
    root = os.path.dirname(_HERE)
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    for rel in KERNEL_SOURCES:
        h.update(rel.encode())
        with open(os.path.join(root, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


class PafuseError(RuntimeError):
    pass


def load(path=None):
    """Load the shared library (once) and attach the prototypes.  Raises if it has not been built.
    `path` (development tools only, before anything else has loaded the library): another build of it, for A/B timing
    of two builds inside one process image - an explicit argument, never the environment."""
    global _lib
    if _lib is None:
        lib_path = path or LIB_PATH
        if not os.path.exists(lib_path):
            raise PafuseError(f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = C.CDLL(lib_path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise PafuseError(f"{lib_path} does not export {name}: a stale build - rebuild it (__graft_entry__.build())")
            fn.restype, fn.argtypes = res, args
        if lib.pafuse_abi_version() != ABI_VERSION:    # struct layouts carry no size fields: a mismatch would shift pointers silently
            raise PafuseError(f"{lib_path} has struct layout version {lib.pafuse_abi_version()}, these bindings {ABI_VERSION}: rebuild")
        _lib = lib
    elif path is not None and os.path.abspath(path) != os.path.abspath(getattr(_lib, "_name", "")):
        raise PafuseError("the library is already loaded from " + str(getattr(_lib, "_name", "?")))
    return _lib


_workspace_policy = None   # None: torch.empty.  Only workspace_policy() sets it; nothing in the library or the environment does


def workspace(nbytes, device, what, dtype=None):
    """The one place that allocates a byte arena handed to the C ABI as a `workspace`, `saved`, `scratch` or `work` argument:
    a contiguous 1-D tensor of exactly max(nbytes, 1) bytes (dtype torch.uint8, the default) or that many bytes' worth of
    torch.float64 (rounded up to whole elements).  `what`: the fixed name of the call site.  With no policy installed this is
    torch.empty and the content is whatever the allocator hands over - no entry point may depend on it."""
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    if dtype not in (torch.uint8, torch.float64):
        raise ValueError(f"workspace({what}): dtype torch.uint8 or torch.float64")
    n = max(int(nbytes), 1)
    n = n if dtype == torch.uint8 else (n + 7) // 8 * 8
    if _workspace_policy is None:
        return torch.empty(n if dtype == torch.uint8 else n // 8, dtype=dtype, device=device)
    t = _workspace_policy(n, torch.device(device), what, dtype)
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == 1 and t.is_contiguous() and t.device.type == torch.device(device).type
            and t.numel() * t.element_size() == n):
        raise PafuseError(f"workspace policy returned no contiguous {dtype} tensor of {n} bytes for '{what}'")
    return t


class workspace_policy:
    """Context manager: workspace() asks policy(nbytes, device, what, dtype) -> tensor for every arena while it is entered, and
    the previous policy (usually none) afterwards, also when the body raises.  A hook for tests that guard or pre-fill the
    arenas (tests/workspace_policy.py); nothing installs one otherwise."""

    def __init__(self, policy):
        self.policy = policy

    def __enter__(self):
        global _workspace_policy
        self.previous, _workspace_policy = _workspace_policy, self.policy
        return self.policy

    def __exit__(self, *exc):
        global _workspace_policy
        _workspace_policy = self.previous
        return False


def check(rc):
    if rc < 0:
        raise PafuseError(f"pafuse_hip error {rc}: {load().pafuse_last_error().decode()}")
    return rc

"""ctypes binding of ``libplayaid_hip.so`` (the C ABI in include/playaid_hip.h).

The product path has no CPU fallback: if the HIP library is missing or does
not load, importing the engine raises ``HipLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PA_LIB_PATH: load a differently built library (e.g. the ablation build used by scripts/)
LIB_PATH = os.environ.get("PA_LIB_PATH") or os.path.join(HERE, "libplayaid_hip.so")

PA_ABI_VERSION = 15
PA_DTYPE_F32 = 0
PA_DTYPE_BF16 = 1
PA_DTYPE_EMULATED_F32 = 2
DTYPES = {"f32": PA_DTYPE_F32, "bf16": PA_DTYPE_BF16, "emulated_f32": PA_DTYPE_EMULATED_F32}
PA_WEIGHT_MAGIC = 0x31574150
PA_LSTM_MAGIC = 0x314C4150
PA_ENCODER_MAGIC = 0x31454150
PA_FEATURE_STRIDE = 1024
PA_TRACE_STAGES = 20
# pa_det_form (include/playaid_hip.h): the kernel form a detector layer ran as, by value
DET_FORMS = ("not_run", "stem_direct", "stem_bf16", "wino", "patch", "pgemm", "pgemm_up", "psgemm", "psgemm_up", "igemm", "sppf",
             "maxpool", "upsample", "absorbed", "decode", "bgemm", "bgemm_up")
# pa_cn_form / pa_lstm_form (ABI 15): the form a conv-net table row / an LSTM layer ran as, by value
CN_FORMS = ("not_run", "stem_pool", "avgpool", "wino", "patch", "igemm_128x128", "igemm_128x64", "igemm_64x64", "psgemm",
            "bgemm", "bgemm_splitk", "avgpool_bf16")
# PA_CN_FORM_STEM_POOL_ANY (appended beside the enum, see the header): every value pa_convnet_layer_forms can report, by value
PA_CN_FORM_STEM_POOL_ANY = 12
CN_FORM_NAMES = CN_FORMS + ("stem_pool_any",)
LSTM_FORMS = ("not_run", "steps", "u1", "u2", "u4", "u8", "mfma")

PA_OK = 0
PA_ERR_INVALID_ARG = -1
PA_ERR_HIP = -2
PA_ERR_BAD_WEIGHTS = -3
PA_ERR_CAPACITY = -4
PA_ERR_NO_DEVICE = -5
PA_ERR_NOT_READY = -6
PA_ERR_BAD_LABELS = -7
PA_EVAL_IGNORE = -100
PA_ANNOT_MAX_ITEMS = 16
# pa_head_trainer_read / pa_lstm_trainer_read: which set of the trained tensors (PA_TRAIN_RAW, or-ed in: the head's alone)
PA_TRAIN_WEIGHTS = 0
PA_TRAIN_M = 1
PA_TRAIN_V = 2
PA_TRAIN_RAW = 16

PA_CROP_OK = 0
PA_CROP_EMPTY = 1
PA_CROP_BAD_BOX = 2
PA_CROP_UPSCALE = 3
PA_CROP_FILTER_TOO_WIDE = 4
PA_CROP_BAD_FRAME = 5
# pa_square_crops_sized: the output sizes it takes
PA_CROP_SIZE_MIN = 16
PA_CROP_SIZE_MAX = 512


class HipLibraryError(RuntimeError):
    pass


class pa_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("device_id", C.c_int32),
        ("sequence_length", C.c_int32),
        ("frame_delta", C.c_int32),
        ("num_actions", C.c_int32),
        ("num_fighters", C.c_int32),
        ("crop_padding", C.c_int32),
        ("max_batch_frames", C.c_int32),
        ("max_clip_frames", C.c_int32),
        ("max_frame_height", C.c_int32),
        ("max_frame_width", C.c_int32),
        ("fighter_class_ids", C.c_int32 * 4),
        ("compute_dtype", C.c_int32),
    ]


class pa_record(C.Structure):
    _fields_ = [
        ("char_id", C.c_int32),
        ("action_id", C.c_int32),
        ("prob", C.c_float),
        ("status", C.c_int32),
    ]


class pa_crop_image(C.Structure):
    _fields_ = [("offset", C.c_int64), ("height", C.c_int32), ("width", C.c_int32)]


class pa_jpeg_file(C.Structure):
    _fields_ = [("offset", C.c_int64), ("nbytes", C.c_int32), ("reserved", C.c_int32)]


class pa_crop_window(C.Structure):
    _fields_ = [("offset", C.c_int64), ("pitch", C.c_int32), ("rows", C.c_int32), ("src_offset", C.c_int64),
                ("src_pitch", C.c_int32), ("row_bytes", C.c_int32)]


class pa_conv_desc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "cin", "cout", "ksize", "stride", "in_hw", "in_buf", "in_pad", "out_buf", "out_pad",
                                        "res_buf", "relu")] + [("w_off", C.c_int64), ("b_off", C.c_int64)]


class pa_net_layer(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "cin", "cout", "ksize", "stride", "in_h", "in_w", "in_buf", "in_coff", "in_cstride", "in_pad",
                                        "out_buf", "out_coff", "out_cstride", "out_pad", "res_buf", "res_coff", "act", "res_after",
                                        "reserved")] + [("w_off", C.c_int64), ("b_off", C.c_int64), ("aux", C.c_float * 8)]


class pa_eval_totals(C.Structure):
    _fields_ = [("rows", C.c_int64), ("correct", C.c_int64), ("ignored", C.c_int64), ("bad_labels", C.c_int64),
                ("nll_sum", C.c_double), ("conf_sum", C.c_double)]


class pa_annot_item(C.Structure):
    _fields_ = [("box", C.c_int32 * 4), ("draw_box", C.c_int32), ("line_width", C.c_int32), ("has_color", C.c_int32),
                ("text_off", C.c_int32), ("text_len", C.c_int32), ("rgb", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class pa_adam_config(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class pa_train_stats(C.Structure):
    _fields_ = [("loss", C.c_float), ("valid", C.c_int32), ("correct", C.c_int32), ("pad", C.c_int32)]


class pa_augment_params(C.Structure):
    _fields_ = [("src", C.c_int32), ("flip", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float), ("blur_k", C.c_int32),
                ("hue_shift", C.c_float), ("sat_shift", C.c_float), ("val_shift", C.c_float), ("noise_sigma", C.c_float),
                ("pixel_drop_thr", C.c_uint32), ("n_holes", C.c_int32), ("holes", C.c_uint8 * 16), ("channel_mask", C.c_int32),
                ("xmap", C.c_uint8 * 128), ("ymap", C.c_uint8 * 128), ("key", C.c_uint64)]


PA_AUGMENT_U8 = 0
PA_AUGMENT_MODEL = 1
PA_AUGMENT_QUANTILES = 1025


class pa_synth_params(C.Structure):
    _fields_ = [("sprite", C.c_int32), ("stage", C.c_int32), ("stage_x", C.c_int32), ("stage_y", C.c_int32),
                ("paste_dx", C.c_int32), ("paste_dy", C.c_int32), ("reserved", C.c_int32 * 2)]


PA_SYNTH_SPRITES = 0
PA_SYNTH_STAGES = 1
PA_SYNTH_U8 = 0
PA_SYNTH_MODEL = 1
PA_SYNTH_DIM_MIN = 32
PA_SYNTH_DIM_MAX = 256
PA_SYNTH_SPRITE_MAX = 1024
PA_SYNTH_STAGE_MAX = 4096
PA_SYNTH_PASTE_MAX = 4096


class pa_sprite_aug_params(C.Structure):
    _fields_ = [("src", C.c_int32), ("flip", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float), ("blur_k", C.c_int32),
                ("hue_shift", C.c_float), ("sat_shift", C.c_float), ("val_shift", C.c_float), ("noise_sigma", C.c_float),
                ("pixel_drop_thr", C.c_uint32), ("n_holes", C.c_int32), ("holes", C.c_uint8 * 4), ("channel_mask", C.c_int32),
                ("new_scale", C.c_int32), ("sized_crop", C.c_int32), ("reserved", C.c_int32), ("xmap", C.c_uint8 * 160),
                ("ymap", C.c_uint8 * 160), ("axmap", C.c_uint8 * 160), ("aymap", C.c_uint8 * 160), ("key", C.c_uint64)]


PA_SPRITE_DROP_THR = 429496729
PA_SPRITE_H1_MAX = 448
PA_SPRITE_CANVAS_MAX = 160


class pa_sprite_resize_params(C.Structure):
    _fields_ = [("src", C.c_int32), ("out_w", C.c_int32), ("out_h", C.c_int32), ("reserved", C.c_int32)]


PA_SPRITE_RESIZE_W_MAX = 160
PA_SPRITE_RESIZE_H_MAX = 560
PA_SPRITE_RESIZE_COEFS = 5776
PA_SCENE_SPRITES_MAX = 4


class pa_scene_sprite(C.Structure):
    _fields_ = [("slot", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


class pa_scene_params(C.Structure):
    _fields_ = [("stage", C.c_int32), ("n_sprites", C.c_int32), ("sprites", pa_scene_sprite * PA_SCENE_SPRITES_MAX),
                ("reserved", C.c_int32 * 2)]


class pa_kernel_stat(C.Structure):
    _fields_ = [
        ("name", C.c_char * 48),
        ("launches", C.c_int32),
        ("total_ms", C.c_float),
        ("flops", C.c_double),
        ("bytes", C.c_double),
        ("flops_executed", C.c_double),
    ]


# every symbol include/playaid_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("pa_create", C.c_int, [C.POINTER(pa_config), _P, C.c_size_t, C.POINTER(_P)]),
    ("pa_create_from_arena", C.c_int, [C.POINTER(pa_config), _P, C.c_size_t, C.POINTER(_P)]),
    ("pa_weights_arena_bytes", C.c_size_t, [_P]),
    ("pa_weights_export", C.c_int, [_P, _P, C.c_size_t, _P]),
    ("pa_destroy", None, [_P]),
    ("pa_last_error", C.c_char_p, [_P]),
    ("pa_status_string", C.c_char_p, [C.c_int]),
    ("pa_abi_version", C.c_int, []),
    ("pa_weight_blob_bytes", C.c_size_t, [C.c_int, C.c_int]),
    ("pa_infer_windows", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("pa_square_crops", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_square_crops_sized", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_runner_inputs", C.c_int, [_P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_backbone_crop_images", C.c_int, [_P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_detect_postprocess", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_uint32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_detect_postprocess_classes", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_detector_create", C.c_int, [C.c_int32, C.POINTER(pa_net_layer), C.c_int32, C.POINTER(C.c_int64), C.c_int32, _P, C.c_size_t,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pa_detector_create_dtype", C.c_int, [C.c_int32, C.POINTER(pa_net_layer), C.c_int32, C.POINTER(C.c_int64), C.c_int32, _P, C.c_size_t,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pa_detector_destroy", None, [_P]),
    ("pa_detector_last_error", C.c_char_p, [_P]),
    ("pa_detector_rows", C.c_int, [_P]),
    ("pa_detector_forward", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("pa_detector_forward_timed", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32]),
    ("pa_detector_trace", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, _P,
                                    _P, _P]),
    ("pa_detector_layer_forms", C.c_int, [_P, _P, C.c_int32]),
    ("pa_clean_detections", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    ("pa_save_one_box_crops", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P,
                                        C.c_size_t, _P, _P]),
    ("pa_project_boxes", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("pa_clip_begin", C.c_int, [_P, C.c_int32]),
    ("pa_clip_begin_batch", C.c_int, [_P, C.c_int32, C.c_int32]),
    ("pa_backbone_frames", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("pa_preprocess_frames", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("pa_backbone_slot", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("pa_upload_crop_windows", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P, _P,
                                         C.POINTER(C.c_size_t), _P]),
    ("pa_preprocess_windows", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("pa_backbone_frames_indexed", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("pa_clip_mark_ready", C.c_int, [_P, _P, C.c_int32]),
    ("pa_device_errors", C.c_int, [_P, C.POINTER(C.c_int32), _P]),
    ("pa_backbone_frames_src", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_head_frames", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_infer_clip", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("pa_features_export", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    ("pa_features_import", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    ("pa_profile_enable", C.c_int, [_P, C.c_int32]),
    ("pa_profile_read", C.c_int, [_P, C.POINTER(pa_kernel_stat), C.c_int32, C.POINTER(C.c_int32)]),
    ("pa_set_crop_jpeg_quality", C.c_int, [_P, C.c_int32]),
    ("pa_stream_spin", C.c_int, [_P, C.c_int32, _P]),
    ("pa_stream_gate", C.c_int, [_P, C.c_int32, _P]),
    ("pa_stream_gate_open", C.c_int, [_P]),
    ("pa_stream_sync", C.c_int, [_P, _P]),
    ("pa_backbone_windows", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("pa_backbone_trace", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P, C.c_size_t, _P]),
    ("pa_lstm_blob_bytes", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("pa_lstm_create", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, C.POINTER(_P)]),
    ("pa_lstm_destroy", None, [_P]),
    ("pa_lstm_last_error", C.c_char_p, [_P]),
    ("pa_lstm_last_status", C.c_int, [_P]),
    ("pa_lstm_forward", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("pa_lstm_layer_forms", C.c_int, [_P, _P, C.c_int32]),
    ("pa_convnet_create", C.c_int, [C.c_int32, C.POINTER(pa_conv_desc), C.c_int32, C.POINTER(C.c_int64), C.c_int32, _P, C.c_size_t,
                                    C.c_int32, C.POINTER(_P)]),
    ("pa_convnet_create_dtype", C.c_int, [C.c_int32, C.POINTER(pa_conv_desc), C.c_int32, C.POINTER(C.c_int64), C.c_int32, _P, C.c_size_t,
                                          C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pa_convnet_destroy", None, [_P]),
    ("pa_convnet_last_error", C.c_char_p, [_P]),
    ("pa_convnet_forward", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("pa_convnet_trace", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, _P]),
    ("pa_convnet_layer_forms", C.c_int, [_P, _P, C.c_int32]),
    ("pa_detector_plan", C.c_int, [_P] * 5 + [C.c_int32] + [_P] * 7),
    ("pa_detector_plan_desc", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_longlong, _P, C.c_int32, C.c_longlong, _P]),
    ("pa_square_crops_src", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_wino_weight_floats", C.c_size_t, [C.c_int32, C.c_int32]),
    ("pa_wino_channels_per_workgroup", C.c_int, [C.c_int32, C.c_int64]),
    ("pa_wino_transform_weights", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("pa_wino_conv3x3", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int32] * 11 + [_P]),
    ("pa_conv_weight_bytes", C.c_size_t, [C.c_int32] * 5),
    ("pa_conv_pack_weights", C.c_int, [_P] + [C.c_int32] * 5 + [_P]),
    ("pa_conv2d", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int32] * 14 + [_P]),
    ("pa_conv2d_branch", C.c_int, [_P, _P, _P, _P, _P, _P, _P] + [C.c_int32] * 14 + [_P]),
    ("pa_stem_int_pack_weights", C.c_int, [_P, _P]),
    ("pa_stem_int", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P]),
    ("pa_wino_conv3x3_splitk", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int32] * 11 + [_P, C.c_size_t, _P, C.c_int32, _P]),
    ("pa_crop_resize_width", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, _P, C.c_int32,
                                       C.POINTER(C.c_int32), _P]),
    ("pa_encoder_blob_bytes", C.c_size_t, [C.c_int32] * 7),
    ("pa_encoder_create", C.c_int, [C.c_int32] * 10 + [_P, C.c_size_t, C.POINTER(_P)]),
    ("pa_encoder_destroy", None, [_P]),
    ("pa_encoder_last_error", C.c_char_p, [_P]),
    ("pa_encoder_forward", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("pa_mjpeg_create", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.POINTER(_P)]),
    ("pa_mjpeg_destroy", None, [_P]),
    ("pa_mjpeg_last_error", C.c_char_p, [_P]),
    ("pa_mjpeg_probe", C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]),
    ("pa_mjpeg_set_sync_rounds", C.c_int, [_P, C.c_int32]),
    ("pa_mjpeg_set_groups", C.c_int, [_P, C.c_int32]),
    ("pa_mjpeg_last_sync_rounds", C.c_int, [_P]),
    ("pa_mjpeg_debug_counters", C.c_int, [_P]),
    ("pa_mjpeg_decode", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_jpegenc_create", C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.POINTER(_P)]),
    ("pa_jpegenc_destroy", None, [_P]),
    ("pa_jpegenc_last_error", C.c_char_p, [_P]),
    ("pa_jpeg_header", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_int32)]),
    ("pa_jpeg_file_bytes_bound", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("pa_jpegenc_encode", C.c_int, [_P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t,
                                    _P, _P]),
    ("pa_jpegenc_overflows", C.c_int, [_P, C.POINTER(C.c_int32), _P]),
    ("pa_jpegdec_create", C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.POINTER(_P)]),
    ("pa_jpegdec_destroy", None, [_P]),
    ("pa_jpegdec_last_error", C.c_char_p, [_P]),
    ("pa_jpegdec_set_sync_rounds", C.c_int, [_P, C.c_int32]),
    ("pa_jpegdec_plan", C.c_int, [_P, _P, C.c_int32, _P, C.POINTER(C.c_size_t), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]),
    ("pa_jpegdec_decode", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P, _P, _P]),
    ("pa_eval_create", C.c_int, [C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pa_eval_destroy", None, [_P]),
    ("pa_eval_reset", C.c_int, [_P, _P]),
    ("pa_eval_update", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    ("pa_eval_read", C.c_int, [_P, C.POINTER(pa_eval_totals), _P, _P]),
    ("pa_annot_create", C.c_int, [C.c_int32, _P] + [C.c_int32] * 7 + [C.POINTER(_P)]),
    ("pa_annotate_frames", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P] + [C.c_int32] * 4 + [_P, _P]),
    ("pa_annot_destroy", None, [_P]),
    ("pa_head_trainer_create", C.c_int, [_P, C.POINTER(pa_adam_config), C.c_int32, C.POINTER(_P)]),
    ("pa_head_trainer_destroy", None, [_P]),
    ("pa_head_trainer_last_error", C.c_char_p, [_P]),
    ("pa_head_trainer_steps", C.c_int64, [_P]),
    ("pa_head_train_step", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pa_head_trainer_read", C.c_int, [_P, C.c_int32, _P, C.c_size_t, _P]),
    ("pa_lstm_trainer_create", C.c_int, [_P, C.POINTER(pa_adam_config), C.POINTER(_P)]),
    ("pa_lstm_trainer_destroy", None, [_P]),
    ("pa_lstm_trainer_last_error", C.c_char_p, [_P]),
    ("pa_lstm_trainer_steps", C.c_int64, [_P]),
    ("pa_lstm_train_step", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("pa_lstm_trainer_read", C.c_int, [_P, C.c_int32, _P, C.c_size_t, _P]),
    ("pa_lstm_trainer_floats", C.c_size_t, [_P]),
    ("pa_encoder_trainer_create", C.c_int, [_P, C.POINTER(pa_adam_config), C.c_float, C.c_uint64, C.POINTER(_P)]),
    ("pa_encoder_trainer_destroy", None, [_P]),
    ("pa_encoder_trainer_last_error", C.c_char_p, [_P]),
    ("pa_encoder_trainer_steps", C.c_int64, [_P]),
    ("pa_encoder_train_step", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("pa_encoder_trainer_read", C.c_int, [_P, C.c_int32, _P, C.c_size_t, _P]),
    ("pa_encoder_trainer_floats", C.c_size_t, [_P]),
    ("pa_encoder_trainer_max_windows", C.c_int32, [_P]),
    ("pa_wino4_weight_floats", C.c_size_t, [C.c_int32, C.c_int32]),
    ("pa_wino4_transform_weights", C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    ("pa_wino4_conv3x3", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int32] * 10 + [_P, C.c_size_t, _P]),
    ("pa_augment_params_check", C.c_int, [_P, C.c_int32, C.c_int32]),
    ("pa_augment_quantiles", C.c_int, [_P]),
    ("pa_augment_crops", C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    ("pa_synth_bank_create", C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.POINTER(_P)]),
    ("pa_synth_bank_destroy", None, [_P]),
    ("pa_synth_params_check", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32]),
    ("pa_synth_composite", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("pa_sprite_aug_params_check", C.c_int, [_P, C.c_int32, _P]),
    ("pa_sprite_bank_create", C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    ("pa_sprite_augment", C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    ("pa_sprite_bank_read", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    ("pa_wino_conv3x3_shape", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int32] * 12 + [_P]),
    ("pa_wino_conv3x3_wg", C.c_int, [_P, _P, _P, _P, _P] + [C.c_int32] * 12 + [_P, C.c_size_t, _P, C.c_int32, _P]),
    ("pa_sprite_resize_params_check", C.c_int, [_P, C.c_int32, _P, _P]),
    ("pa_sprite_resize_bank_create", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pa_sprite_resize", C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    ("pa_sprite_resize_bank_read", C.c_int, [_P, _P, C.c_int32, _P, C.c_size_t, _P]),
    ("pa_scene_params_check", C.c_int, [_P, C.c_int32, _P, _P]),
    ("pa_scene_composite", C.c_int, [_P, _P, _P, _P, C.c_int32, _P, C.c_size_t, _P, _P]),
]

_lib = None


def load() -> C.CDLL:
    """Load the shared library and bind every exported symbol (fails loudly)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so.7; import it FIRST so that this
    # library's NEEDED libamdhip64.so.7 resolves to that same runtime instance.
    # Two HIP/HSA runtimes in one process cannot both open the device, and
    # streams / device pointers are only meaningful inside one of them.
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `python -m playaid_core_amd._build` "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback for this path."
        )
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the box
        raise HipLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, restype, argtypes in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.pa_abi_version() != PA_ABI_VERSION:
        raise HipLibraryError("libplayaid_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib

/*
 * playaid_hip.h -- C ABI of the MI355X (gfx950) action-recognition hot path.
 *
 * The reference (NathanBWaters/playaid_core) is pure Python and has no FFI; the
 * path sits behind three Python call boundaries. Each
 * entry point below names the reference interface it replaces. The Python host
 * in playaid_core_amd/ binds this library with ctypes and re-exposes the
 * reference's own classes (CNNActionDetector, AIRunner, YoloCrop); see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - All data pointers are DEVICE pointers (HBM) unless the name ends in
 *     _host. The caller owns every buffer. `stream` is a hipStream_t passed as
 *     void* (NULL = default stream). Calls only enqueue work; nothing here
 *     synchronises except pa_create / pa_destroy / pa_profile_read and the
 *     *_sync helpers.
 *   - Return value: PA_OK (0) or a negative pa_status. pa_last_error() gives a
 *     human-readable message for the last failing call on that engine. The
 *     reference's asserts / exit() (ai_runner.py:240-242,447,458; fighter.py
 *     :356-362) become status codes; per-crop failures are reported in the
 *     per-crop `status` words, not as a failed call.
 *   - One engine per device; an engine is not thread-safe (the reference is
 *     single-threaded).
 *   - Frames are numbered from 1 like the reference's YOLO files
 *     (ai_runner.py:516); `frame0` arguments are 0-based indices into a clip.
 */
#ifndef PLAYAID_HIP_H
#define PLAYAID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_ABI_VERSION 15
#define PA_WEIGHT_MAGIC 0x31574150 /* "PAW1" */
#define PA_LSTM_MAGIC 0x314c4150   /* "PAL1" */
#define PA_ENCODER_MAGIC 0x31454150 /* "PAE1" */
#define PA_FEATURE_STRIDE 1024     /* floats per cached feature row (1000 used) */
#define PA_CROP 128

typedef enum pa_status {
    PA_OK = 0,
    PA_ERR_INVALID_ARG = -1,
    PA_ERR_HIP = -2,          /* a HIP runtime call failed; see pa_last_error */
    PA_ERR_BAD_WEIGHTS = -3,  /* blob size / magic / shape mismatch */
    PA_ERR_CAPACITY = -4,     /* more frames/windows than the engine was created for */
    PA_ERR_NO_DEVICE = -5,
    PA_ERR_NOT_READY = -6,    /* head asked for frames whose features are not cached */
    PA_ERR_BAD_LABELS = -7    /* pa_eval_read: labels outside [0, num_actions) were met (and skipped); the totals are filled */
} pa_status;

/* per-crop status words written by the preprocess stage */
#define PA_CROP_OK 0
#define PA_CROP_EMPTY 1        /* empty / off-screen slice: reference returns (False, None), fighter.py:356-362.
                                 A (d x 0) slice (box off the right / left edge with exactly d rows left) is NOT
                                 empty: ImageOps.pad skips the resize (contain size == source size) and returns
                                 a black d x d canvas, so that crop is PA_CROP_OK with all-zero pixels. A (0 x d)
                                 slice stays PA_CROP_EMPTY: there Pillow raises ZeroDivisionError, which the
                                 reference does not catch (it crashes) -- a stated departure. */
#define PA_CROP_BAD_BOX 2      /* non-finite box or square side <= 0 (reference raises) */
#define PA_CROP_UPSCALE 3      /* reserved (was: square side < 128 px rejected; the enlarging branch is implemented now) */
#define PA_CROP_FILTER_TOO_WIDE 4 /* bicubic support beyond the kernel's table size (scale > 3.5) */
#define PA_CROP_BAD_FRAME 5    /* pa_backbone_frames_src: source index outside the frame buffer */

typedef struct pa_engine pa_engine;

/* Geometry of the path. Defaults mirror ai_runner.py:426-439 and
 * cnn_action_detector.py:14-27. */
typedef struct pa_config {
    int32_t abi_version;       /* PA_ABI_VERSION */
    int32_t device_id;         /* HIP device ordinal */
    int32_t sequence_length;   /* S, odd; 7 (ai_runner.py:432) */
    int32_t frame_delta;       /* 3 (ai_runner.py:433-437) */
    int32_t num_actions;       /* A; 63 (anim_ontology.py:592-600) */
    int32_t num_fighters;      /* crops per frame; 2 (ai_runner.py:240-242) */
    int32_t crop_padding;      /* 30 px (ai_runner.py:417-418) */
    int32_t max_batch_frames;  /* most frames handed to one pa_backbone_frames call */
    int32_t max_clip_frames;   /* feature-cache capacity in frames */
    int32_t max_frame_height;  /* scratch sizing for the resampler */
    int32_t max_frame_width;
    int32_t fighter_class_ids[4]; /* CHAR_LIST index of each fighter slot (constants.py:51) */
    int32_t compute_dtype;     /* PA_DTYPE_F32 (default, the reference's arithmetic), PA_DTYPE_BF16 or PA_DTYPE_EMULATED_F32 */
} pa_config;

/* compute_dtype. PA_DTYPE_BF16 (BASELINE.json configs[2]) stores the activations and folded
 * weights of the sixteen 3x3 convolutions in bf16 and multiplies them on the bf16 matrix cores
 * with fp32 accumulation; the stem, the fc, the temporal head and every interface stay fp32.
 * It is NOT within the 1e-4 parity bar of the fp32 path (tests state its own tolerance). */
#define PA_DTYPE_F32 0
#define PA_DTYPE_BF16 1
/* PA_DTYPE_EMULATED_F32 (ABI 11; never the default): fp32 inputs, fp32 outputs and fp32-accurate sums, but the products of the
 * convolutions run on the bf16 matrix cores -- every fp32 operand as three bf16 slices (an exact decomposition of its 24-bit
 * significand), the six leading cross products per fp32 product on v_mfma_f32_32x32x16_bf16, fp32 accumulation
 * (csrc/psgemm.hip). As close to a float64 run as the exact fp32 kernels are, and inside the same 1e-4 parity bars (the fp32
 * parity tests run under both values); summation order and rounding differ from the fp32 instruction's, so results are NOT
 * bit-identical to PA_DTYPE_F32. Layers without an emulated kernel run the exact fp32 one. bench.py's `value` / `dtype` stay
 * on PA_DTYPE_F32; this value is reported as the side block `emulated_fp32`. */
#define PA_DTYPE_EMULATED_F32 2

/* Result record per (frame, fighter): the fields AIRunner.action_recognition
 * derives at ai_runner.py:474-479. confidence% = prob * 100 is left to the host
 * (the reference multiplies in Python double). */
typedef struct pa_record {
    int32_t char_id;    /* CHAR_LIST.index(fighter) */
    int32_t action_id;  /* int(torch.argmax(predictions)) */
    float prob;         /* exp(logp[action_id]) */
    int32_t status;     /* PA_CROP_* of the window's middle crop */
} pa_record;

/* One row per kernel family of the last profiled call(s). */
typedef struct pa_kernel_stat {
    char name[48];
    int32_t launches;
    float total_ms;     /* sum of HIP-event durations on the engine's stream */
    double flops;       /* algorithmic FLOPs summed over those launches (a convolution: 2 x outputs x k x k x cin) */
    double bytes;       /* algorithmic (compulsory) HBM bytes summed over those launches */
    double flops_executed; /* multiply-adds the matrix cores actually ran, x 2: equal to `flops` except for launches of the
                              Winograd F(2x2, 3x3) kernel, which execute 4 / 9 of their layer's direct-form count (ABI 9) */
} pa_kernel_stat;

/* ---- lifetime ----------------------------------------------------------- */

/* Replaces CNNActionDetector.load_from_checkpoint(...).eval()
 * (ai_runner.py:164-168; cnn_action_detector.py:46-92).
 * weight_blob_host: int32 header {PA_WEIGHT_MAGIC, 1, S, A, 0,0,0,0} followed by
 * the fp32 tensors of the Lightning state_dict in this order, PyTorch layouts:
 *   model.cnn2d.conv1.weight[64,3,7,7], bn1.{weight,bias,running_mean,running_var}[64],
 *   for layer 1..4, block 0..1: conv1.weight, bn1.{w,b,mean,var}, conv2.weight,
 *     bn2.{w,b,mean,var}, then (block 0 of layers 2..4) downsample.0.weight,
 *     downsample.1.{w,b,mean,var};
 *   fc.weight[1000,512], fc.bias[1000];
 *   model.cnn1d.0.weight[512,1000,S], model.cnn1d.0.bias[512];
 *   model.classifier.0.weight[128,512], .bias[128];
 *   model.classifier.2.weight[A,128], .bias[A].
 * BatchNorm (eval, eps 1e-5) is folded into the preceding convolution in fp64
 * on the host and the tensors are re-laid-out for the kernels here. */
int pa_create(const pa_config* cfg, const void* weight_blob_host, size_t blob_bytes, pa_engine** out);
/* Weights for the other GPUs of a node (one broadcast of the weights). The
 * folded, re-laid-out tensors of an engine live in one device arena whose layout depends only on
 * (sequence_length, num_actions, compute_dtype): pa_weights_export copies it into a caller buffer of
 * pa_weights_arena_bytes() bytes (device to device, on `stream`); after that buffer has been broadcast
 * (RCCL), every other rank builds its engine from it with pa_create_from_arena -- no host copy of the
 * weights, no second BatchNorm fold. The reference has no counterpart (single process,
 * ai_runner.py:164-168). */
int pa_create_from_arena(const pa_config* cfg, const void* arena_dev, size_t arena_bytes, pa_engine** out);
size_t pa_weights_arena_bytes(const pa_engine* e);
int pa_weights_export(pa_engine* e, void* arena_dst_dev, size_t arena_bytes, void* stream);
void pa_destroy(pa_engine* e);
const char* pa_last_error(const pa_engine* e);
const char* pa_status_string(int status);
int pa_abi_version(void);
/* Expected blob size in bytes for (S, A). */
size_t pa_weight_blob_bytes(int sequence_length, int num_actions);

/* ---- b1: the operator --------------------------------------------------- */

/* Replaces `logp = model(x)` (cnn_action_detector.py:86-92; ai_runner.py:472).
 * x: float32[B,S,3,128,128] NCHW contiguous, values in [0,1].
 * logp: float32[B,A] log-probabilities. B*S <= max_batch_frames*num_fighters. */
int pa_infer_windows(pa_engine* e, const float* x, int32_t batch, float* logp, void* stream);

/* ---- a6: crop preprocessing --------------------------------------------- */

/* Replaces YoloCrop.square_crop(frame, 128, padding) (fighter.py:323-381) for
 * n frames x num_fighters boxes at once.
 * frames: uint8[n,H,W,3] HWC (BGR as cv2 delivers it, ai_runner.py:404-405).
 * boxes:  float64[n,num_fighters,4] normalised (cx,cy,w,h) (ai_runner.py:53-71).
 * crops:  uint8[n,num_fighters,128,128,3]; channel order kept when swap_rb=0
 *         (square_crop), reversed when swap_rb=1 (the BGR2RGB of ai_runner.py:448).
 * status: int32[n,num_fighters] PA_CROP_*; failed crops are all zero. */
int pa_square_crops(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                    const double* boxes, int32_t padding, int32_t swap_rb, uint8_t* crops,
                    int32_t* status, void* stream);

/* The same at any output size (ABI 15, appended): YoloCrop.square_crop(frame, output_size, padding) for every integer
 * output_size in PA_CROP_SIZE_MIN .. PA_CROP_SIZE_MAX (PA_ERR_INVALID_ARG outside). crops: uint8[n,num_fighters,S,S,3] with
 * S = output_size; status as above, failed crops all zero; stream-ordered with pa_square_crops (it uses the same scratch of the
 * engine, which is sized by max_frame_height x max_frame_width and not by S). All branches of cv2.resize(INTER_AREA) to
 * (S, int(d * (S / float(d)))) are kept: copy (d == S), 2 x 2 and integer scale, the general shrink in OpenCV's fp32 order,
 * the fixed-point bilinear emulation for d < S, and the black last row when the height comes out as S - 1. Its kernels
 * (csrc/crop_sized.hip) are a multi-pass form; pa_square_crops keeps the 128 x 128 kernels, which this call never launches.
 * Kernel limits, the only sources of PA_CROP_FILTER_TOO_WIDE here (the same two as pa_square_crops): a Pillow BICUBIC pass of
 * ImageOps.pad that shrinks by more than 3.5 (more than 15 taps: with padding 30 an unclipped box whose square side is below
 * 24 pixels), and a slice whose intermediates (slice rows x padded width x 3 bytes) exceed one max_frame_height x
 * max_frame_width frame. */
#define PA_CROP_SIZE_MIN 16
#define PA_CROP_SIZE_MAX 512
int pa_square_crops_sized(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                          const double* boxes, int32_t padding, int32_t swap_rb, int32_t output_size,
                          uint8_t* crops, int32_t* status, void* stream);

/* ---- a5: the runner's own input branch ----------------------------------- */

/* One crop image inside a byte buffer: what YOLOv5 --save-crop wrote and cv2.imread returns
 * (ai_runner.py:445-446), uint8 [height][width][3], BGR, rows packed. */
typedef struct pa_crop_image {
    int64_t offset;  /* byte offset of the image in `images` */
    int32_t height;
    int32_t width;
} pa_crop_image;

/* Replaces the per-frame body of AIRunner.get_action_recognition_input_for_frame (ai_runner.py:446-459)
 * for n_crops crop images of ANY size at once: BGR2RGB (swap_rb = 1) -> imutils.resize(width=128)
 * = cv2.resize(INTER_AREA) to (128, int(h * (128 / w))) -> ImageOps.pad((128, 128), black) when that is
 * not 128 rows (tall crops are BICUBIC-shrunk and letterboxed left/right, wide ones letterboxed top/bottom).
 * images: device bytes; desc: device pa_crop_image[n_crops]; inputs_u8: uint8[n_crops][128][128][3] (the
 * `frames` list of :459-464); status: int32[n_crops] PA_CROP_* (PA_CROP_BAD_BOX: descriptor outside the
 * buffer or larger than max_frame_height x max_frame_width; PA_CROP_EMPTY: int(h*128/w) == 0, where
 * cv2.resize raises; PA_CROP_FILTER_TOO_WIDE: taller than 3.5 x 128 rows after the resize). */
int pa_runner_inputs(pa_engine* e, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int32_t n_crops,
                     int32_t swap_rb, uint8_t* inputs_u8, int32_t* status, void* stream);

/* pa_backbone_frames for a clip that arrives as crop IMAGES instead of frames + boxes (the reference's
 * actual on-disk hand-off, crops/<Fighter>/<video>_<n>.jpg after decoding): n frames x num_fighters images in
 * (frame, fighter) order -> runner inputs -> ResNet-18 features in the cache rows of frames frame0... */
int pa_backbone_crop_images(pa_engine* e, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int32_t n,
                            int32_t frame0, uint8_t* crops_rgb, int32_t* status, void* stream);

/* ---- f1: detection post-processing --------------------------------------- */

/* Replaces the post-network half of the YOLOv5 subprocess AIRunner.run_yolo starts (ai_runner.py:191-224:
 * detect.py --max-det 2 --save-txt --save-conf --classes 2 3): from the detection head's decoded rows
 * pred[n_frames][rows][5 + num_classes] (cx cy w h in network-input pixels, objectness, class scores; device
 * float32) to the numbers of the label files the reference parses (ai_runner.py:53-94): objectness and
 * confidence gates (conf_thres, default 0.25), best class per row, class filter (class_mask bit c = class c
 * allowed; the reference passes classes 2 and 3), class-aware IoU NMS (iou_thres, default 0.45), at most
 * max_det (<= 8) boxes, mapped from the letterboxed net_height x net_width input back to the img_height x
 * img_width frame, rounded to pixels and normalised.
 * dets: float32[n_frames][max_det][6] = cls cx cy w h conf in LABEL-FILE order (detect.py writes
 * reversed(det): lowest confidence first); counts: int32[n_frames]. The host writes each row as six '%g'
 * fields (playaid_core_amd/detect.py). The arithmetic is the un-vendored ultralytics/yolov5 checkout's; the
 * contract is restated in oracle/detect.py ("parity unpinned"). */
int pa_detect_postprocess(pa_engine* e, const float* pred, int32_t n_frames, int32_t rows, int32_t num_classes,
                          float conf_thres, float iou_thres, uint32_t class_mask, int32_t max_det, int32_t net_height,
                          int32_t net_width, int32_t img_height, int32_t img_width, float* dets, int32_t* counts, void* stream);
/* pa_detect_postprocess for up to 80 classes (a stock COCO checkpoint): num_classes 1..80, and the class filter as
 * class_words, ceil(num_classes / 32) host words -- bit c % 32 of word c / 32 = class c allowed -- or NULL for every class
 * (detect.py without --classes). Same arithmetic, same outputs and the same order of the dets rows as pa_detect_postprocess:
 * for num_classes <= 32 and class_mask = class_words[0] both give the same dets and counts. One gating pass per frame reads
 * every row once and compacts the rows over the gates; the max_det arg-max passes walk that list (a frame with more than
 * 4096 such rows walks every row instead, with the same result). */
int pa_detect_postprocess_classes(pa_engine* e, const float* pred, int32_t n_frames, int32_t rows, int32_t num_classes,
                                  float conf_thres, float iou_thres, const uint32_t* class_words, int32_t max_det, int32_t net_height,
                                  int32_t net_width, int32_t img_height, int32_t img_width, float* dets, int32_t* counts, void* stream);

/* ---- f1: the detection network ---------------------------------------------
 *
 * Replaces the network half of the YOLOv5 subprocess (ai_runner.py:191-224: `detect.py --weights <yolov5s checkpoint>
 * --source <video>`): frames -> letterbox (cv2.resize INTER_LINEAR to the un-padded size, 114-grey border, BGR -> RGB,
 * / 255) -> a fully convolutional network given as a LAYER TABLE -> Detect decode -> pred float32[n][rows][5 + nc] in
 * network-input pixels, i.e. the input of pa_detect_postprocess. The table (playaid_core_amd/yolov5.py builds any YOLOv5
 * v6.0 / v7.0 P5 model -- n, s, m, l, x -- from an ultralytics state dict) arrives BatchNorm-folded: per convolution
 * [cout][ky][kx][cin] at w_off and the bias [cout] at b_off (float offsets into one blob); the 6x6 stem in the lane layout of
 * kind 3 below. Activations are zero-bordered NHWC device buffers of buf_floats_per_image[b] floats per image; a layer addresses
 * a CHANNEL SLICE of a buffer (coff = first channel, cstride = channels per pixel of the buffer), so concatenations are free.
 * Channel counts that are not multiples of 32 are the table's business: it pads them with zero weight rows, zero weight
 * columns and zero biases (SiLU(0) = 0: the padding stays exactly 0 and moves no result).
 * A stem wider than 32 channels is one kind-3 row per 32 of them, each with cout = 32, its own weights and bias, and
 * out_coff = 32 g into the same buffer; under PA_DTYPE_EMULATED_F32 and PA_DTYPE_BF16 every such row gets its own bf16
 * fragments and runs on stem6x6_bf16_kernel (form PA_DET_FORM_STEM_BF16), under PA_DTYPE_F32 on the direct kernel. */
typedef struct pa_net_layer {
    int32_t kind;      /* 0 convolution, 3 stem 6x6/2 + SiLU on the letter-boxed image (cout == 32; weights float32[64][56]: lane l =
                          (kx / 3) * 32 + channel holds W[channel][c][ky][3 * (l / 32) + j] at ky * 9 + j * 3 + c), 4 max-pool 5x5/1,
                          5 nearest 2x up-sampling, 6 Detect decode of one scale (3 anchors) */
    int32_t cin, cout; /* kind 0: cin % 32 == 0, cout % 32 == 0 (pad with zero weights; cout % 64 != 0 needs in_pad == 1 for a 3x3 and no residual for a 1x1); kinds 4 / 5: cin = channels moved */
    int32_t ksize, stride;           /* kind 0: 1 | 3, 1 | 2 */
    int32_t in_h, in_w;              /* interior of the input */
    int32_t in_buf, in_coff, in_cstride, in_pad;
    int32_t out_buf, out_coff, out_cstride, out_pad;
    int32_t res_buf, res_coff;       /* residual slice (-1: none): the output's geometry and cstride */
    int32_t act;                     /* 0 none, 1 ReLU, 2 SiLU */
    int32_t res_after;               /* 1: residual added after the activation (YOLOv5 Bottleneck), 0: before (ResNet) */
    int32_t reserved;
    int64_t w_off, b_off;
    float aux[8];                    /* kind 6: stride of the scale, then 3 anchors (w, h) in network-input pixels */
} pa_net_layer;
typedef struct pa_detector pa_detector;
int pa_detector_create(int32_t device, const pa_net_layer* layers, int32_t n_layers, const int64_t* buf_floats_per_image, int32_t n_bufs,
                       const float* weights_host, size_t n_weights, int32_t max_images, int32_t net_h, int32_t net_w, int32_t num_classes,
                       pa_detector** out);
/* The same with the convolutions' arithmetic chosen (ABI 11): PA_DTYPE_F32 (= pa_detector_create) or PA_DTYPE_EMULATED_F32 -- the
 * 1x1 and stride-2 3x3 convolutions then run on the bf16 matrix cores with fp32-accurate sums (see PA_DTYPE_EMULATED_F32; the
 * stride-1 3x3 layers keep their exact Winograd kernel), and so does the 6x6 stem: the letter-boxed pixels are integers 0..255,
 * one exact bf16 value each, multiplied with the three bf16 slices of W / 255 (csrc/yolo.hip, stem6x6_bf16_kernel). Never the default.
 *
 * PA_DTYPE_BF16 (ABI 14; never the default): bf16 storage and bf16 products. Rounding model:
 *   - letter-boxed input: the pixel integers 0..255 as bf16 (exact);
 *   - stem: stem6x6_bf16_kernel's product of the integers with the three bf16 slices of fp32 W / 255, + fp32 bias, SiLU in fp32,
 *     ONE round-to-nearest-even (RNE) to bf16 on the store;
 *   - every other convolution (csrc/bgemm.hip): the folded fp32 weights rounded RNE to bf16 once, at create; the activations as
 *     stored (bf16); products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; + fp32 bias, SiLU in fp32; a residual (the
 *     in-place Bottleneck's, res_after) added as its stored bf16 value in fp32 after the activation; ONE RNE rounding on the store;
 *   - the Detect heads -- the convolutions whose output buffer a decode row (kind 6) reads -- store fp32, and the decode runs on
 *     fp32 as under PA_DTYPE_F32;
 *   - max-pools (SPPF, fused or not) and 2x up-samplings (fused into the producer or not): on bf16, exact.
 * Buffers hold 2 bytes per element, 4 for those a decode row reads (buf_floats_per_image counts elements). Create fails, naming
 * the row, where a row has no bf16 form. Detections are NOT within the fp32 path's 1e-4 parity bar (tests state their own). */
int pa_detector_create_dtype(int32_t device, const pa_net_layer* layers, int32_t n_layers, const int64_t* buf_floats_per_image, int32_t n_bufs,
                             const float* weights_host, size_t n_weights, int32_t max_images, int32_t net_h, int32_t net_w, int32_t num_classes,
                             int32_t compute_dtype, pa_detector** out);
void pa_detector_destroy(pa_detector* h);
const char* pa_detector_last_error(const pa_detector* h);
int pa_detector_rows(const pa_detector* h); /* rows of pred per image: 3 x sum over the decode layers of in_h x in_w */
/* frames uint8[n,H,W,3] BGR (device) -> pred float32[n][rows][5 + nc] (device). */
int pa_detector_forward(pa_detector* h, const uint8_t* frames, int32_t n, int32_t height, int32_t width, float* pred, void* stream);
/* Measurement aid: the same call with a HIP event between the table's layers; layer_us[i] (host, cap >= n_layers) = microseconds
 * layer i took on `stream`. Synchronises the stream. */
int pa_detector_forward_timed(pa_detector* h, const uint8_t* frames, int32_t n, int32_t height, int32_t width, float* pred, void* stream,
                              float* layer_us, int32_t cap);
/* Test aids (ABI 13). pa_detector_trace enqueues exactly what pa_detector_forward enqueues for n (1..max_images) frames in one
 * range of images -- letterbox, kernels, tiles, fusions, knobs -- for layers 0..last_layer (-1: the letterbox alone), then copies
 * images [img0, img0 + n_img) of the handle's capacity of buffer `buf`, as stored (zero border included), to `out` (device).
 * buf = -1 is the letter-boxed input x0 [image][net_h + 4][net_w + 4][4]: fp32 / 255, or (PA_DTYPE_EMULATED_F32 with the bf16
 * stem) the pixel integers as bf16, 2 bytes each. A layer buffer holds (h + 2 pad) x (w + 2 pad) x cstride elements per image, the
 * geometry of the rows that touch it: fp32, or under PA_DTYPE_BF16 bf16 (2 bytes) except the buffers a decode row reads; out_bytes
 * is checked against that element size. A layer that one launch runs together with others (SPPF's pools, an up-sampling fused
 * into its producer) runs with its group: *last_done (host, may be NULL) = the last layer run. Decode layers write `pred`
 * (device, [n][rows][5 + nc]). PA_ERR_INVALID_ARG for a layer, buffer or image range out of range, n outside 1..max_images
 * or out_bytes short of the range. */
int pa_detector_trace(pa_detector* h, const uint8_t* frames, int32_t n, int32_t height, int32_t width, int32_t last_layer, int32_t buf,
                      int32_t img0, int32_t n_img, void* out, size_t out_bytes, float* pred, int32_t* last_done, void* stream);
/* The kernel form each layer ran as in the last forward or trace (decided at run time: a launcher that refuses a shape passes
 * the layer on to the next form). forms: host int32[cap], cap >= the number of layers. */
typedef enum pa_det_form {
    PA_DET_FORM_NOT_RUN = 0,
    PA_DET_FORM_STEM_DIRECT = 1,  /* stem6x6_direct_kernel (exact fp32) */
    PA_DET_FORM_STEM_BF16 = 2,    /* stem6x6_bf16_kernel (integer pixels, three bf16 slices of W / 255) */
    PA_DET_FORM_WINO = 3,         /* Winograd F(2x2, 3x3), wino.hip */
    PA_DET_FORM_PATCH = 4,        /* patch-resident blocked 3x3, patchconv.hip */
    PA_DET_FORM_PGEMM = 5,        /* persistent GEMM, pigemm.hip */
    PA_DET_FORM_PGEMM_UP = 6,     /* ... writing the next layer's 2x up-sampling too */
    PA_DET_FORM_PSGEMM = 7,       /* emulated-fp32 persistent GEMM, psgemm.hip */
    PA_DET_FORM_PSGEMM_UP = 8,    /* ... writing the next layer's 2x up-sampling too */
    PA_DET_FORM_IGEMM = 9,        /* one-tile-per-workgroup implicit GEMM, igemm.hip */
    PA_DET_FORM_SPPF = 10,        /* SPPF's three max-pools in one launch (this layer and the two absorbed after it) */
    PA_DET_FORM_MAXPOOL = 11,     /* one 5x5 max-pool */
    PA_DET_FORM_UPSAMPLE = 12,    /* one 2x up-sampling */
    PA_DET_FORM_ABSORBED = 13,    /* run by the launch of an earlier layer */
    PA_DET_FORM_DECODE = 14,      /* Detect decode */
    PA_DET_FORM_BGEMM = 15,       /* one-slice bf16 persistent GEMM, bgemm.hip (PA_DTYPE_BF16; ABI 14) */
    PA_DET_FORM_BGEMM_UP = 16     /* ... writing the next layer's 2x up-sampling too */
} pa_det_form;
int pa_detector_layer_forms(const pa_detector* h, int32_t* forms, int32_t cap);

/* Replaces AIRunner.clean_yolo_crops / clean_yolo_crops_for_fighter (ai_runner.py:226-289, 306-424) on the table
 * pa_detect_postprocess wrote (dets float32[n_labels][max_det][6], counts int32[n_labels]; label n = index n - 1), with no
 * label files in between: per fighter (cfg.fighter_class_ids) duplicate detections of its class are resolved (nearest
 * centre, L1, to the class's previous box), the frames it is missing in get boxes interpolated FROM THE END frame and
 * pixels from VideoCapture position j (one decoded frame late; a read past n_decoded_frames copies the previous crop),
 * and the fighter whose crops end first gets its last crop copied up to, not including, the other's last frame. The rows
 * are taken through the label file's '%g' formatting first, so the tables equal the host mirror's
 * (playaid_core_amd/label_cleaning.py, which works on the label text) bit for bit. All device pointers:
 * labels float64[n_labels][F][6] = every fighter's repaired label row (cls cx cy w h conf; cls < 0: none);
 * pixel_frame int32[n_labels][F] = decoded frame each crop is cut from (-1 none); pixel_box float64[n_labels][F][4];
 * crop_kind int32[n_labels][F]: 1 the detector's own crop (save_one_box of crop_row), 2 a square_crop repair, 0 none;
 * crop_row float32[n_labels][F][6]; info4 int32[4] = max_frames (number of the last non-empty label), error code
 * (0 ok; 1 duplicate detections of a class never seen before, ai_runner.py:343; 2 a gap before a fighter's first
 * detection, :375-378; 3 a fighter without any detection), the label number it happened at, duplicates resolved. Rows
 * behind max_frames of pixel_frame / crop_kind are written as "no crop" (-1 / 0) whatever the caller's memory held. Enqueue
 * only; the call uses ONE scratch per engine (sized at pa_create for max_clip_frames x 8 detections; a longer table grows it
 * behind a device synchronisation), so the calls of one engine belong on one stream, or on streams the caller orders. */
int pa_clean_detections(pa_engine* e, const float* dets, const int32_t* counts, int32_t n_labels, int32_t max_det, int32_t n_decoded_frames,
                        double* labels, int32_t* pixel_frame, double* pixel_box, int32_t* crop_kind, float* crop_row, int32_t* info4,
                        void* stream);

/* What the crop hand-off needs from pa_clean_detections' tables, worked out on the device (one launch instead of a dozen
 * generic element-wise / sort launches between the repair and the crops): det_index / src_own int32[n_labels][F] = the
 * det_index / src_frame arguments of pa_save_one_box_crops for the entries of kind 1 (-1 / 0 elsewhere; rows behind
 * max_frames count as "no crop"); the square_crop repairs (kind 2, rows < max_frames) compacted in entry order:
 * rep_entry int32[] = their (frame * F + fighter) entries, rep_boxes float64[][4], rep_src int32[] = source frames --
 * each with room for n_labels * F entries, padded with copies of the first repair to a whole number of F (the shape
 * pa_square_crops_src cuts); words5 int32[5] = info4 followed by the number of repairs (the five words a host waits
 * for). Enqueue only. */
int pa_detector_plan(pa_engine* e, const int32_t* pixel_frame, const double* pixel_box, const int32_t* crop_kind, const int32_t* info4,
                     int32_t n_labels, int32_t* det_index, int32_t* src_own, int32_t* rep_entry, double* rep_boxes, int32_t* rep_src,
                     int32_t* words5, void* stream);
/* The clip's crop-image descriptors once pa_save_one_box_crops has packed every chunk of `step_frames` frames into a region
 * of `region_bytes` of its own (descriptor offsets relative to the region): kind-1 entries move by their chunk's region,
 * the n_rep repairs' 128 x 128 x 3 images sit back to back from byte `rep_base`. desc[n_frames][F]. Enqueue only. */
int pa_detector_plan_desc(pa_engine* e, pa_crop_image* desc, const int32_t* crop_kind, int32_t n_frames, int32_t step_frames,
                          long long region_bytes, const int32_t* rep_entry, int32_t n_rep, long long rep_base, void* stream);
/* pa_square_crops with every crop cut from the frame src_frame names (int32[n][F], device; frames uint8[n_src,H,W,3]):
 * the square_crop repairs of clean_yolo_crops, whose pixels come from VideoCapture position j (ai_runner.py:404-418). */
int pa_square_crops_src(pa_engine* e, const uint8_t* frames, int32_t n_src, int32_t height, int32_t width, const double* boxes,
                        const int32_t* src_frame, int32_t n, int32_t padding, int32_t swap_rb, uint8_t* crops, int32_t* status, void* stream);

/* Replaces the crop half of the same subprocess (`--save-crop`, ai_runner.py:208) and the cv2.imread that reads each
 * crop back (:445-446): per (frame, fighter) YOLOv5 v7.0's utils/plots.py::save_one_box -- the label row's pixel box ->
 * xyxy2xywh -> wh * 1.02 + 10 -> xywh2xyxy -> .long() -> clip_boxes -> im[y1:y2, x1:x2] (float32 like torch) -- and, for
 * jpeg_quality 1..100, the pixel arithmetic of its Image.save(quality=95, subsampling=0) + a JPEG read (4:4:4 baseline
 * JPEG of an image of ANY size, edge blocks filled by edge replication; jpeg_quality 0 leaves the raw cut).
 * frames uint8[n_src,H,W,3] BGR; n clip frames; src_frame int32[n][num_fighters] (device; NULL = every crop from its own
 * frame, n_src == n) says which frame a crop's pixels come from (the reference's tail repair copies the last crop FILE of a
 * fighter to later frames, ai_runner.py:270-289); dets float32[n][max_det][6] / counts int32[n] as pa_detect_postprocess
 * wrote them (label rows, label-file order);
 * det_index int32[n][num_fighters] (device) = which detection of its frame each fighter's crop is cut from, -1 none, or
 * NULL = the first detection of the fighter's class (cfg.fighter_class_ids) in label order, i.e. the crop file whose name
 * carries no counter. The BGR images land back to back (16-byte aligned) in `images`, desc[n][num_fighters] describes them
 * (height = width = 0: no detection / empty rectangle / no room left in `images`, the latter also counted for
 * pa_device_errors): exactly what pa_runner_inputs / pa_backbone_crop_images take. Restated in oracle/detect.py
 * (rectangle: parity unpinned, YOLOv5 is not vendored) + oracle/jpeg.py::roundtrip_any (pinned to live libjpeg-turbo). */
int pa_save_one_box_crops(pa_engine* e, const uint8_t* frames, int32_t n_src, int32_t height, int32_t width, const float* dets,
                          const int32_t* counts, int32_t max_det, const int32_t* det_index, const int32_t* src_frame, int32_t n,
                          int32_t jpeg_quality, uint8_t* images, size_t images_capacity, pa_crop_image* desc, void* stream);

/* Boxes from the game log instead of a detector. Replaces the
 * projection half of Fighter.set_from_json (fighter.py:494-539: calculate_lookat_matrix,
 * calculate_intrinsic_matrix, project_point_to_pixel on four corners, all for the
 * reference's hard-coded 1280x720 image) + YoloCrop.from_pixel_coordinates (fighter.py:170-190).
 * log_rows: float64[n_rows,9] = pos_x, pos_y, camera_position xyz, camera_target_position
 * xyz, fov in degrees (STAGE_ENUM_TO_DATA[stage]["fov"], fighter.py:488); boxes:
 * float64[n_rows,4] normalised (cx,cy,w,h), directly usable as the `boxes` of the calls below. */
int pa_project_boxes(pa_engine* e, const double* log_rows, int32_t n_rows, double* boxes, void* stream);

/* ---- b2: the runner loop ------------------------------------------------ */

/* Start a clip of clip_frames frames (= the reference's max_frames,
 * ai_runner.py:244-245): sets the clamp range of the window sampler and marks
 * the feature cache empty. */
int pa_clip_begin(pa_engine* e, int32_t clip_frames);
/* A batch of n_clips INDEPENDENT clips of clip_frames frames each, processed as one clip of n_clips * clip_frames
 * frames (clip c = frames c * clip_frames ...): the backbone calls see one long clip -- more crops per launch --
 * while every window is clamped to its own clip's frame numbers, so each clip's records equal what it gets alone up
 * to fp32 rounding (launch sizes pick tiles / split-K factors) (the reference runs clips one after another; ai_runner.py:493-520 has no cross-clip state). Records of frame
 * numbers that are a multiple of clip_frames belong to no clip (a clip's frame numbers run 1 .. clip_frames - 1)
 * and are to be ignored. */
int pa_clip_begin_batch(pa_engine* e, int32_t n_clips, int32_t clip_frames);

/* Crop + backbone for frames frame0 .. frame0+n-1 (0-based) of the clip:
 * square_crop(pad) -> BGR2RGB -> /255 -> ResNet-18 -> 1000-d feature per
 * (frame, fighter), stored in the engine's feature cache. Replaces the crop
 * read + `self.model.cnn2d` part of ai_runner.py:443-472 with each crop run
 * through the backbone once instead of once per window.
 * crops_rgb (optional, may be NULL): uint8[n,num_fighters,128,128,3] copy of the
 * model inputs (the `frames` entry of action_recognition's dict, :489).
 * status (optional): int32[n,num_fighters]. */
int pa_backbone_frames(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                       const double* boxes, int32_t frame0, uint8_t* crops_rgb, int32_t* status,
                       void* stream);

/* The two halves of pa_backbone_frames as separate calls, so that a host can pipeline them
 * on two streams: crop preprocessing of chunk k+1 (VALU/LDS-bound) overlaps the backbone of
 * chunk k (MFMA-bound) on the same GPU. `slot` (0 or 1) selects one of two model-input
 * buffers inside the engine. Ordering is the caller's job:
 *   - all pa_preprocess_frames / pa_square_crops calls are stream-ordered with each other
 *     (they share scratch memory);
 *   - pa_backbone_slot(slot) runs after the pa_preprocess_frames that filled `slot`;
 *   - a slot is not refilled before the pa_backbone_slot that read it has passed its first
 *     kernel (in practice: record an event after pa_backbone_slot and make the preprocess
 *     stream wait on it; playaid_core_amd/parallel.py does exactly this). */
int pa_preprocess_frames(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                         const double* boxes, int32_t slot, uint8_t* crops_rgb, int32_t* status,
                         void* stream);
int pa_backbone_slot(pa_engine* e, int32_t slot, int32_t n, int32_t frame0, void* stream);

/* ---- f2 / a1: ingest without hardware decode ----------------------------- */

/* This image has no hardware decode path (no rocDecode / rocJPEG / VCN libraries, no cv2), so "decode" is the
 * hand-over of raw BGR frames (cv2.VideoCapture.read's output, ai_runner.py:404-405). When those
 * frames sit in HOST memory, uploading them whole costs 6.2 MB per 1080p frame of PCIe for the ~0.84 MB the two
 * crops read. pa_upload_crop_windows copies only each crop's slice -- the square_crop region fighter.py:335-343
 * cuts, computed on the host with the device plan's own arithmetic -- into a packed device buffer: one kernel
 * whose waves read the slice rows straight out of the host frames over PCIe (frames_host must be pinned,
 * device-visible memory: hipHostMalloc / torch pin_memory; desc_host too) and writes one descriptor per crop; pa_preprocess_windows is
 * pa_preprocess_frames reading those windows (bit-identical crops). height / width stay the FRAME's. */
typedef struct pa_crop_window {
    int64_t offset;      /* first byte of the slice in the window buffer (16-byte aligned) */
    int32_t pitch;       /* bytes per slice row in the window buffer (row_bytes rounded up to 16) */
    int32_t rows;        /* slice rows */
    int64_t src_offset;  /* first byte of the slice in the host frame buffer */
    int32_t src_pitch;   /* bytes per frame row */
    int32_t row_bytes;   /* slice width * 3 */
} pa_crop_window;
int pa_upload_crop_windows(pa_engine* e, const uint8_t* frames_host, int32_t n, int32_t height, int32_t width,
                           const double* boxes_host, int32_t padding, uint8_t* windows_dev, size_t windows_capacity,
                           pa_crop_window* desc_host, pa_crop_window* desc_dev, size_t* bytes_used, void* stream);
int pa_preprocess_windows(pa_engine* e, const uint8_t* windows_dev, const pa_crop_window* desc_dev, int32_t n, int32_t height,
                          int32_t width, const double* boxes, int32_t slot, uint8_t* crops_rgb, int32_t* status, void* stream);

/* ---- a1 / f2: Motion-JPEG decode on the device ------------------------------ */

/* Replaces the per-frame decode of cv2.VideoCapture.read / cv2.imread (ai_runner.py:153,404-405,446;
 * manuscript.py:154-155) for Motion-JPEG streams and JPEG image sequences: n baseline JPEG files (SOF0 / 8-bit SOF1,
 * Huffman, one interleaved scan; 4:2:0, 4:2:2, 4:4:4 or grey; with or without restart markers) -> uint8 [n][height][width][3]
 * frames in HBM, BGR like OpenCV (rgb = 0) or RGB (rgb = 1). The arithmetic is libjpeg(-turbo)'s defaults, which OpenCV's
 * JPEG reader runs: integer IDCT (JDCT_ISLOW), fancy chroma up-sampling, jdcolor.c; oracle/jpeg.py::decode restates it and is
 * pinned byte for byte against the live libjpeg-turbo. (OpenCV's FFmpeg backend for .avi containers runs FFmpeg's own
 * decoder, which differs from libjpeg in the last bit; that arithmetic is not restated.)
 *
 * A handle owns the scratch for up to max_frames frames of max_height x max_width and max_bytes compressed bytes per
 * call. pa_mjpeg_decode parses the marker segments on the host, then ENQUEUES: one host -> device copy of the compressed
 * bytes (the range of data_host that covers all n frames; pinned memory makes it asynchronous) on a copy stream of the
 * handle's own, which `stream` waits for -- so the upload of one call runs under the decode passes of the call before it;
 * data_host must stay untouched until `stream` has passed this call -- and, on `stream`, the restart-marker
 * scan + byte un-stuffing, Huffman decoding (one lane per subsequence of the stream, wherever it falls: the
 * decoder states at the subsequence borders are found by self-synchronisation -- a speculative pass, then verify passes
 * until nothing changes -- so a stream needs no restart markers to decode in parallel; restart markers, where present,
 * are exact entry points), IDCT, up-sampling + colour conversion. spans_host: int64[n][2], frame f = bytes [spans[f][0], spans[f][1]) of data_host, in
 * any order (container chunk headers between frames are never looked at); every frame of a call has the same size and
 * sampling (tables and restart interval may change per frame).
 * status_dev (optional): int32[n] device, 0 or a bit set: 1 invalid Huffman code, 2 restart markers do not match the
 * header's interval, 4 coefficient index overflow, 8 the decoder states had not settled after the enqueued verify
 * passes (decode again after pa_mjpeg_set_sync_rounds(h, 0)) -- such a frame's pixels are undefined, nothing is written
 * out of bounds. Malformed or unsupported HEADERS fail the call with PA_ERR_INVALID_ARG and name the frame in
 * pa_mjpeg_last_error; nothing is enqueued then. */
typedef struct pa_mjpeg pa_mjpeg;
int pa_mjpeg_create(int32_t device, int32_t max_frames, int32_t max_height, int32_t max_width, size_t max_bytes, pa_mjpeg** out);
void pa_mjpeg_destroy(pa_mjpeg* h);
const char* pa_mjpeg_last_error(const pa_mjpeg* h);
/* Host only, no device: the marker segments of one JPEG file as pa_mjpeg_decode reads them. info8 = height, width,
 * components, max horizontal / vertical sampling factor (2,2 = 4:2:0), restart interval in MCUs (0 = none), byte offset
 * of the entropy-coded data, 0. PA_ERR_INVALID_ARG with the reason in `why` for files the decoder does not take
 * (progressive, arithmetic, 12-bit, multi-scan, truncated headers). */
int pa_mjpeg_probe(const uint8_t* data_host, size_t nbytes, int32_t* info8, char* why, size_t why_bytes);
/* Verify passes per call: 1..16 are enqueued without looking at their outcome (default 8; a pass over a frame whose
 * previous pass changed nothing returns at once; 1080p frames at quality 95 settle in three, and a frame that has not
 * settled is flagged with status bit 8); 0 = exact mode: passes are repeated until one changes
 * nothing, which synchronises the stream once per pass (long runs of identical blocks -- black bars -- re-synchronise
 * slowly and can need many). pa_mjpeg_last_sync_rounds: how many the last call ran. */
int pa_mjpeg_set_sync_rounds(pa_mjpeg* h, int32_t rounds);
int pa_mjpeg_last_sync_rounds(const pa_mjpeg* h);
/* Frame groups per call, 1..4 (default 2): a call's frames are decoded in that many groups, each on a stream of the
 * handle's own (uploads on a further one), joined to `stream` at the end -- a group's upload and its latency-bound late
 * verify passes run under the other group's passes. 1 = everything on `stream`: the setting for a caller that keeps
 * several decoders busy on several streams itself. The decoded frames are the same for every value. */
int pa_mjpeg_set_groups(pa_mjpeg* h, int32_t groups);
/* Diagnostics of the entropy decoder (scripts/mjpeg_rate.py): for pass kind m = 0 speculative, 1 verify, 2 final of the most
 * recent call, out8_host[2m] = shader-clock cycles the first wave of the first frame spent in its symbol loop,
 * out8_host[2m + 1] = (100 MHz wall ticks << 32) | symbols it walked; out8_host[8 + 2m] = cycles of those spent outside
 * the straight-line symbol loop (ring top-ups, restart markers, general symbols), out8_host[9 + 2m] = how often it
 * left that loop. out8_host holds 16 values. Synchronises the device. */
int pa_mjpeg_debug_counters(unsigned long long* out8_host);
int pa_mjpeg_decode(pa_mjpeg* h, const uint8_t* data_host, const int64_t* spans_host, int32_t n, int32_t height, int32_t width,
                    int32_t rgb, uint8_t* frames_dev, int32_t* status_dev, void* stream);

/* ---- a2 / a3: baseline JPEG encode on the device --------------------------------- */

/* The file half of YOLOv5's `--save-crop` hand-off (ai_runner.py:191-194, 208, 291-295: crops/<Fighter>/<video>_<n>.jpg)
 * and the writer of Motion-JPEG clips: n packed uint8 [h][w][3] images in HBM -> n complete baseline JPEG files in HBM,
 * byte for byte what libjpeg(-turbo) writes for the same pixels (Pillow's Image.save(quality, subsampling) without
 * `optimize`): JFIF 1.1 APP0, two DQT segments from jpeg_set_quality(q, force_baseline), SOF0, the four standard Huffman
 * tables K.3-K.6 (DC0, AC0, DC1, AC1), one interleaved scan without restart markers, FF bytes stuffed, the last byte
 * filled with 1-bits, FFD9. Samples: jccolor.c, edge blocks by repeating the last row / column, 4:2:0 by jcsample.c's
 * h2v2_downsample (dummy luma blocks of a half-empty MCU: AC 0, DC of the block before), jfdctint.c, jcdctmgr.c.
 *
 * A handle owns the scratch of one call: max_blocks 8x8 blocks (all components, all images of a call; 130 bytes each)
 * and scratch_bytes for the un-stuffed entropy-coded streams (each image's rounded up to 64 bytes). pa_jpegenc_encode
 * only ENQUEUES on `stream` -- about ten launches, no host synchronisation, no waiting between workgroups; calls on one
 * handle must be stream-ordered with each other.
 * images / images_bytes: device bytes exactly as pa_save_one_box_crops(jpeg_quality = 0) / pa_square_crops leave them;
 * desc (device) as pa_crop_image; bgr = 1 for OpenCV's channel order, 0 for R, G, B; quality 1..100; subsampling 0 (4:4:4)
 * or 2 (4:2:0); max_height / max_width bound every image of the call (they size the grids). The files land back to back
 * in `files`, each at a 16-byte aligned offset, in input order; out[n] (device) says where. An entry with
 * height = width = 0 gets nbytes = 0. An image that does not fit -- the handle's blocks or stream scratch, files_capacity,
 * a descriptor larger than max_height x max_width or outside images_bytes -- gets nbytes = -1, is counted for
 * pa_jpegenc_overflows, and nothing of it is written; the images before it stay valid (the ones behind it fail as well:
 * offsets are running sums). Bad arguments return PA_ERR_INVALID_ARG without touching the device. */
typedef struct pa_jpeg_file {
    int64_t offset;   /* first byte of the file in `files` (16-byte aligned) */
    int32_t nbytes;   /* file length; 0: empty entry; -1: did not fit */
    int32_t reserved;
} pa_jpeg_file;
typedef struct pa_jpegenc pa_jpegenc;
int pa_jpegenc_create(int32_t device, int32_t max_images, int64_t max_blocks, size_t scratch_bytes, pa_jpegenc** out);
void pa_jpegenc_destroy(pa_jpegenc* h);
const char* pa_jpegenc_last_error(const pa_jpegenc* h);
/* Host only, no device: the 623 header bytes (SOI .. SOS) of such a file. */
int pa_jpeg_header(int32_t height, int32_t width, int32_t quality, int32_t subsampling, uint8_t* out_host, size_t cap, int32_t* nbytes);
/* Host only: an upper bound of a file's length: header + 2 * 209 bytes per coded block (1665 bits, every byte stuffed)
 * + 2; 0 for bad arguments. */
size_t pa_jpeg_file_bytes_bound(int32_t height, int32_t width, int32_t subsampling);
int pa_jpegenc_encode(pa_jpegenc* h, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int32_t n, int32_t max_height,
                      int32_t max_width, int32_t bgr, int32_t quality, int32_t subsampling, uint8_t* files, size_t files_capacity,
                      pa_jpeg_file* out, void* stream);
/* Images that did not fit since the last query (the count is reset); synchronises `stream`. */
int pa_jpegenc_overflows(pa_jpegenc* h, int32_t* count_host, void* stream);

/* ---- a2 / a3 (read side): the crop cache's JPEG files of mixed sizes, decoded on the device ---- */

/* The other half of the cache boundary pa_jpegenc_encode writes: the reference reads every cached crop back with cv2.imread
 * (ai_runner.py:191-194, 445-446). n baseline JPEG FILES OF DIFFERENT SIZES AND SAMPLINGS -- save_one_box crops (any size,
 * 4:4:4) and the repaired gaps' 128 x 128 4:2:0 files (:420) sit in one folder -- go straight into the packed crop-image layout
 * pa_backbone_crop_images / pa_runner_inputs consume: rows packed, each image at a 16-byte aligned offset, one pa_crop_image
 * per image. Per image it takes what pa_mjpeg_decode takes per call: 4:4:4, 4:2:2, 4:2:0 or grey (three equal channels, as
 * cv2.imread gives), restart markers or none, standard or optimised tables. The arithmetic is libjpeg-turbo's, including one
 * rule no video frame meets: 2:1 sub-sampled chroma at most 2 samples wide is replicated, not filtered (jdsample.c).
 *
 * pa_jpegdec_plan is host only and needs no device: the marker segments of the n files spans_host[i] = bytes [start, end)
 * of data_host -> desc_host[i] (height, width, offset = running sum of (h * w * 3 + 15) & ~15 in input order), the total
 * *images_bytes and *blocks, the sum of all components' 8x8 blocks padded to whole MCUs, which a handle's max_blocks must
 * cover. An empty span (start == end: no file for that frame and fighter) gives height = width = 0 and takes no bytes. A
 * file the decoder does not take (progressive, arithmetic, 12-bit, multi-scan, 4 components, truncated header) returns
 * PA_ERR_INVALID_ARG and names the image index and the reason in `why`. desc_host, images_bytes, blocks may be NULL.
 *
 * A handle owns the scratch of one call: up to max_images files, max_blocks blocks and max_bytes compressed bytes (the range
 * of data_host that covers the call's spans). pa_jpegdec_decode parses on the host, then only ENQUEUES on `stream`: the upload
 * of that byte range, the descriptors to desc_dev (device pa_crop_image[n]), the pixels to images_dev (16-byte aligned; BGR
 * for bgr = 1, RGB for 0) and, if not NULL, the per-image status bits of pa_mjpeg_decode to status_dev (device int32[n]).
 * The number of launches does not depend on n. Spans may come in any order and may repeat; data_host must stay untouched
 * until `stream` has passed the call; calls on one handle must be stream-ordered with each other. PA_ERR_CAPACITY, with
 * nothing enqueued, when n, the blocks, the bytes or images_capacity exceed what the handle or the caller provided;
 * header problems fail the call like pa_jpegdec_plan (pa_jpegdec_last_error). A corrupt entropy-coded stream flags its own
 * image, whose pixels are undefined; nothing is written out of bounds and the other images are not affected.
 * pa_jpegdec_set_sync_rounds: as pa_mjpeg_set_sync_rounds (1..16 passes enqueued, default 16: a pass over an image that has
 * settled returns at once; 0 = exact mode, which synchronises `stream` once per pass). */
typedef struct pa_jpegdec pa_jpegdec;
int pa_jpegdec_create(int32_t device, int32_t max_images, int64_t max_blocks, size_t max_bytes, pa_jpegdec** out);
void pa_jpegdec_destroy(pa_jpegdec* h);
const char* pa_jpegdec_last_error(const pa_jpegdec* h);
int pa_jpegdec_set_sync_rounds(pa_jpegdec* h, int32_t rounds);
int pa_jpegdec_plan(const uint8_t* data_host, const int64_t* spans_host, int32_t n, pa_crop_image* desc_host, size_t* images_bytes,
                    int64_t* blocks, char* why, size_t why_bytes);
int pa_jpegdec_decode(pa_jpegdec* h, const uint8_t* data_host, const int64_t* spans_host, int32_t n, int32_t bgr, uint8_t* images_dev,
                      size_t images_capacity, pa_crop_image* desc_dev, int32_t* status_dev, void* stream);

/* pa_backbone_frames for frames that are NOT consecutive in the clip (a resolution bucket of a
 * mixed-resolution stream, BASELINE.json configs[4]): frame_ids[n] (device, int32, 0-based)
 * says where each frame's features go in the cache. The call does not touch host-side clip
 * state, so it can be captured into a hipGraph and replayed with new buffer contents; tell
 * the engine which frames are cached with pa_clip_mark_ready (host ids) before pa_head_frames. */
int pa_backbone_frames_indexed(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                               const double* boxes, const int32_t* frame_ids, uint8_t* crops_rgb,
                               int32_t* status, void* stream);
int pa_clip_mark_ready(pa_engine* e, const int32_t* frame_ids_host, int32_t n);
/* pa_backbone_frames_indexed cannot validate device-resident ids on the host: a frame id outside
 * [0, clip_frames) writes nothing and is counted on the device. This call synchronises `stream`, returns
 * the count since the last call in *bad_frame_ids_host (and clears it); PA_ERR_CAPACITY when non-zero. */
int pa_device_errors(pa_engine* e, int32_t* bad_frame_ids_host, void* stream);

/* pa_backbone_frames for a clip whose crops are NOT cut from their own frame: crop (i, p) of clip frame
 * frame0 + i comes from frames[src_frame[i*num_fighters + p]] (device int32, values in [0, n_src)).
 * This is what clean_yolo_crops_for_fighter does for repaired gaps -- it re-cuts a missing crop from
 * VideoCapture position j, one decoded frame late, per fighter (ai_runner.py:404-418) -- in one pass.
 * A source index outside the buffer gives that crop status PA_CROP_BAD_FRAME (all-zero pixels). */
int pa_backbone_frames_src(pa_engine* e, const uint8_t* frames, int32_t n_src, int32_t height, int32_t width,
                           const double* boxes, const int32_t* src_frame, int32_t n, int32_t frame0,
                           uint8_t* crops_rgb, int32_t* status, void* stream);

/* Window gather + Conv1d/MLP head + log_softmax + argmax for frame numbers
 * frame_num_lo .. frame_num_hi-1 (1-based, as run_action_recognition iterates
 * range(1, max_frames), ai_runner.py:508). Replaces
 * action_sample_from_frame_middle_out (dataset_utils.py:109-138) and the head
 * half of ai_runner.py:472-477.
 * records: pa_record[count,num_fighters]; logp (optional): float32[count,num_fighters,A]. */
int pa_head_frames(pa_engine* e, int32_t frame_num_lo, int32_t frame_num_hi, pa_record* records,
                   float* logp, void* stream);

/* pa_clip_begin + pa_backbone_frames(all n frames) + pa_head_frames(1..n-1):
 * AIRunner.run_action_recognition (ai_runner.py:493-520) for an n-frame clip.
 * records: pa_record[n-1,num_fighters]; logp optional float32[n-1,num_fighters,A]. */
int pa_infer_clip(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                  const double* boxes, pa_record* records, float* logp, uint8_t* crops_rgb,
                  int32_t* status, void* stream);

/* Feature-cache access for frame-parallel sharding: copy
 * the cached rows of frames frame0..frame0+n-1 out of / into the engine.
 * feats: float32[n,num_fighters,PA_FEATURE_STRIDE]. pa_features_import also sets the crop status of the rows it
 * writes to PA_CROP_OK (on the same stream): an imported row has no crop of this engine, so the pa_record.status of a
 * window whose middle frame was imported is 0, not what an earlier clip left in that row. */
int pa_features_export(pa_engine* e, int32_t frame0, int32_t n, float* feats, void* stream);
int pa_features_import(pa_engine* e, int32_t frame0, int32_t n, const float* feats, void* stream);

/* Damage HUD crops (AIRunner.run_damage_detection, ai_runner.py:556-571 +
 * damage_crop_to_percent :114): YoloCrop.crop_img (fighter.py:316-321) = image[y1:y2, x1:x2] followed by
 * imutils.resize(width=out_w) = cv2.resize(INTER_AREA) to (out_w, int(h * (out_w / float(w)))), for up to four pixel
 * rectangles per frame (rects_host int32[n_rects][4] = x1, y1, x2, y2 from YoloCrop.xyxy_pixels). frames
 * uint8[n,H,W,3] (device) -> out uint8[n,n_rects,out_h_cap,out_w,3] (device, channel order kept; rows beyond a
 * rectangle's height untouched); the heights are returned in out_h_host[n_rects]. The recogniser the reference
 * then calls (PaddleOCR) is an external model and is not part of this library. */
int pa_crop_resize_width(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const int32_t* rects_host,
                         int32_t n_rects, int32_t out_w, uint8_t* out, int32_t out_h_cap, int32_t* out_h_host, void* stream);

/* ---- the alternative temporal model --------
 *
 * RNNActionDetector (playaid/models/rnn_action_detector.py:55-95): the same torchvision resnet18 with
 * fc = Linear(512, 300), then nn.LSTM(300, 512, num_layers=3), Linear(512,128) + ReLU, Linear(128, A),
 * log_softmax -- one output row per (window, frame). The backbone half reuses an engine's kernels:
 *
 * pa_backbone_windows: x float32[n_crops,3,128,128] (NCHW, values k/255, device) -> feats
 * float32[n_crops,PA_FEATURE_STRIDE] (device), the engine's resnet18 output per crop (fc included; an
 * engine built from a state dict whose fc rows 300..999 are zero yields the 300 features and zeros). */
int pa_backbone_windows(pa_engine* e, const float* x, int32_t n_crops, float* feats, void* stream);

/* Test aid (ABI 12): the intermediate activations of the backbone. Enqueues exactly what pa_backbone_windows enqueues for
 * n_crops (1..max_crops crops, one chunk: same kernels, tiles, split-K, fused branches and knobs), stops after `stage`
 * and copies that stage's buffer, zero border included, to `out` (device, >= the stage's bytes). Storage type: bf16
 * bits (2 bytes) for stages 0-17 of a PA_DTYPE_BF16 engine, float32 everywhere else.
 *   0: model input x0 [n][134][134][4]          1: stem + BatchNorm + ReLU + max-pool [n][34][34][64]
 *   2..17: the sixteen 3x3 convolutions in engine order (layer1.0.conv1, layer1.0.conv2, layer1.1.conv1, ...,
 *          layer4.1.conv2), each [n][hw+2][hw+2][cout]
 *   18: avgpool float32 [n][512]                19: fc float32 [n][PA_FEATURE_STRIDE]
 * aux (device, may be NULL): at the layerX.0.conv2 stages of layers 2-4 (7, 11, 15) the stored 1x1/2 downsample branch
 * the convolution read as its residual, in the layout and type of `out` (no bias: the conv's bias holds both). Where the
 * engine stores no branch at such a stage (fused into the conv's K) a non-NULL aux is refused; elsewhere it is unused.
 * PA_ERR_INVALID_ARG for a stage out of range, n_crops outside 1..max_crops or a buffer too small. */
#define PA_TRACE_STAGES 20
int pa_backbone_trace(pa_engine* e, const float* x, int32_t n_crops, int32_t stage, void* out, size_t out_bytes, void* aux,
                      size_t aux_bytes, void* stream);

/* The recurrent head. blob: int32 header {PA_LSTM_MAGIC, 1, input_dim, hidden_dim, num_layers, num_actions, 0, 0},
 * then float32 per layer l: weight_ih_l [4H, in_l], weight_hh_l [4H, H], bias_ih_l [4H], bias_hh_l [4H] (torch
 * gate order i, f, g, o; in_0 = input_dim, in_l = H), then action_decoder.0.weight [128, H], .0.bias [128],
 * .2.weight [A, 128], .2.bias [A]. hidden_dim % 8 == 0, <= 512; max_rows bounds seq_len * batch. */
typedef struct pa_lstm pa_lstm;
size_t pa_lstm_blob_bytes(int32_t input_dim, int32_t hidden_dim, int32_t num_layers, int32_t num_actions);
int pa_lstm_create(int32_t device, int32_t input_dim, int32_t hidden_dim, int32_t num_layers, int32_t num_actions,
                   int32_t max_rows, const void* blob_host, size_t blob_bytes, pa_lstm** out);
void pa_lstm_destroy(pa_lstm* h);
const char* pa_lstm_last_error(const pa_lstm* h);
/* x float32[seq_len, batch, ld] (device; the first input_dim of every ld-float row are read), zero initial
 * state -> logp float32[seq_len * batch, num_actions] (device). As in the reference (:88-90, an nn.LSTM
 * without batch_first fed [B, S, 300]) seq_len is the number of WINDOWS and batch (<= 16) the frames of a
 * window: the state runs from one window to the next. */
int pa_lstm_forward(pa_lstm* h, const float* x, int32_t ld, int32_t seq_len, int32_t batch, float* logp, void* stream);
/* A layer's time steps run in ONE launch (H / 4 workgroups, an ordinary launch since ABI 10) whose workgroups hand h(t) to each
 * other as tagged 8-byte granules and therefore must all be resident at once. The library checks the grid against HALF of what
 * the EMPTY device holds (occupancy query x CUs) and otherwise launches one kernel per time step; the query cannot see kernels of
 * OTHER streams, so do not overlap pa_lstm_forward with launches that fill the chip for more than a few milliseconds (the
 * engine's lanes, the chain's decode / detector stages). If part of the grid is nevertheless kept off the device, a granule that
 * does not arrive within 20 ms ends the launch: that call's logp rows are then NaN (never garbage) and the status below says so.
 * Call this after synchronising the stream of a pa_lstm_forward: PA_ERR_HIP ONCE if that happened (the handle launches one
 * kernel per time step from then on and later calls are valid), PA_OK otherwise. */
int pa_lstm_last_status(pa_lstm* h);
/* Test aid (ABI 15): per layer, the form the last pa_lstm_forward launched it as -- the fallback it really took (a grid the
 * device cannot hold, PA_LSTM_STEPS, a handle past a timeout), not the path it would have preferred. forms: host
 * int32[cap], cap >= num_layers. Enqueues nothing. */
typedef enum pa_lstm_form {
    PA_LSTM_FORM_NOT_RUN = 0,
    PA_LSTM_FORM_STEPS = 1,  /* one lstm_step_kernel launch per time step */
    PA_LSTM_FORM_U1 = 2,     /* persistent lstm_layer_kernel, vector recurrent product, 1 hidden unit per workgroup */
    PA_LSTM_FORM_U2 = 3,     /* ... 2 units */
    PA_LSTM_FORM_U4 = 4,     /* ... 4 units */
    PA_LSTM_FORM_U8 = 5,     /* ... 8 units */
    PA_LSTM_FORM_MFMA = 6    /* persistent, 4 units, recurrent product on the fp32 matrix cores */
} pa_lstm_form;
int pa_lstm_layer_forms(const pa_lstm* h, int32_t* forms, int32_t cap);

/* A conv-net given as a table (the ResNet-50 backbone of ResnetTransformerDetector,
 * playaid/models/resnet_transformer_detector.py:37), run on the engine's fp32 convolution kernels. Weights arrive
 * BatchNorm-folded: per convolution [cout][ky][kx][cin] at w_off and the bias [cout] at b_off (float offsets into
 * one blob); the 7x7/2 stem as [64][7 ky][8 px][4 ch] (kx >= 7 and channel 3 zero). Activations: `n_bufs` device
 * buffers of buf_floats_per_crop[b] floats per crop, NHWC with a zero border of `pad` pixels; a bordered buffer
 * must keep one geometry for the whole table. Layers run in table order. */
typedef struct pa_conv_desc {
    int32_t kind;               /* 0 convolution, 1 stem 7x7/2 + ReLU + max-pool 3x3/2 of the 128x128x3 input, 2 global average pool,
                                   3 the same stem + max-pool of an in_hw x in_hw x 3 input (below) */
    int32_t cin, cout;          /* kind 0: cin % 32 == 0, cout % 64 == 0; kind 2: cin = channels */
    int32_t ksize, stride;      /* 1 | 3, 1 | 2 */
    int32_t in_hw;              /* spatial size of the input interior (square) */
    int32_t in_buf, in_pad;     /* in_pad >= (ksize - 1) / 2 */
    int32_t out_buf, out_pad;
    int32_t res_buf;            /* residual added before the ReLU (geometry of the output), or -1 */
    int32_t relu;
    int64_t w_off, b_off;
} pa_conv_desc;
typedef struct pa_convnet pa_convnet;
/* Kind 3 (ABI 15, appended; csrc/stem_pool_any.hip): the kind-1 stem for a square input of any in_hw with in_hw % 32 == 0 and
 * 64 <= in_hw <= 512. Weights in the same [64][7][8][4] layout, in_pad == 3, out_pad == 1; it writes the pooled map
 * [in_hw / 4 + 2]^2 x 64 (zero border 1). A table holds at most one stem row (kind 1 or 3), and that row sets the size of the
 * input pa_convnet_forward / pa_convnet_trace take: x float32[n,3,in_hw,in_hw], converted into [max_crops][in_hw + 6]^2 x 4
 * (which is what trace's buf = -1 returns). Kind 1 keeps meaning 128 and keeps its kernel. fp32 only: create refuses a
 * PA_DTYPE_BF16 table with a kind-3 row, and any kind-3 row outside the limits above, naming the row in last_error. Every other
 * row runs on the launchers it ran on before; a stride-1 3x3 row whose map is not 4, 8, 16 or 32 pixels wide (the widths the
 * patch-resident kernel is laid out for) and that Winograd does not take (sides % 4 != 0, or below 8) runs on the implicit GEMM. */
int pa_convnet_create(int32_t device, const pa_conv_desc* descs, int32_t n_descs, const int64_t* buf_floats_per_crop,
                      int32_t n_bufs, const float* weights_host, size_t n_weights, int32_t max_crops, pa_convnet** out);
/* The same with the convolutions' arithmetic chosen (ABI 11): PA_DTYPE_F32 (= pa_convnet_create) or PA_DTYPE_EMULATED_F32 -- every
 * convolution that is not in Winograd form and has enough 128-pixel tiles at max_crops to fill half the chip runs on the emulated-fp32
 * persistent GEMM (csrc/psgemm.hip), the rest on the exact kernels. Never the default.
 *
 * PA_DTYPE_BF16 (ABI 15, no new symbol; never the default): bf16 storage and bf16 products. Rounding model:
 *   - input: the fp32 NCHW image rounded to nearest even (RNE) to bf16 (the engine's bf16 conversion into [134][134][4]);
 *   - stem (kind 1): the folded 7x7 weights RNE to bf16 once at create ([64][224] as laid out); products on
 *     v_mfma_f32_32x32x16_bf16, fp32 accumulation; then fp32 bias, ReLU and the 3x3/2 max-pool; ONE RNE to bf16 on the store;
 *   - convolutions (kind 0), every row on csrc/bgemm.hip: the folded fp32 weights RNE to bf16 once at create; activations read
 *     as stored (bf16); products on v_mfma_f32_32x32x16_bf16, fp32 accumulation; + fp32 bias, + the stored bf16 residual in
 *     fp32 BEFORE the ReLU, ReLU, ONE RNE on the store. A split-K row sums the fp32 partials of contiguous k-ranges in split
 *     order (the bias inside the first), then runs the same epilogue; results are bitwise repeatable. No Winograd form;
 *   - global average pool (kind 2): the stored bf16 values summed in fp32 in a fixed order (row by row), times 1 / hw^2; fp32
 *     output [n][C], so the last row of a bf16 table must be a pool.
 * Buffers written by stem or convolution rows hold bf16 (2 bytes per element; buf_floats_per_crop still counts elements), those
 * written by a pool fp32. Create refuses, naming the row, a buffer written in both types, a row reading an fp32 buffer, a
 * convolution bgemm.hip cannot take (ReLU or none) and a table that does not end in a pool. Split-K: where the unsplit grid of a
 * row at the call's n is below a quarter of the CUs (64 workgroups) and K >= 72 x 32, S in {2, 4, 8} with tiles x S <= 256 and at
 * least 4 k-steps per slice, the largest; PA_CONVNET_BG_SPLIT=0 or 1 (read once) turns it off, =n forces S = n on every row whose grid
 * is below half the CUs (A/B runs). */
int pa_convnet_create_dtype(int32_t device, const pa_conv_desc* descs, int32_t n_descs, const int64_t* buf_floats_per_crop,
                            int32_t n_bufs, const float* weights_host, size_t n_weights, int32_t max_crops, int32_t compute_dtype,
                            pa_convnet** out);
void pa_convnet_destroy(pa_convnet* h);
const char* pa_convnet_last_error(const pa_convnet* h);
/* x float32[n,3,S,S] (NCHW, device; S = 128, or the in_hw of the table's kind-3 row) -> out: the last layer's output buffer,
 * float32[n, out_floats_per_crop]. */
int pa_convnet_forward(pa_convnet* h, const float* x, int32_t n, float* out, int32_t out_floats_per_crop, void* stream);
/* Test aids (ABI 15). pa_convnet_trace enqueues exactly what pa_convnet_forward enqueues for n (1..max_crops) crops -- kernels,
 * tiles, knobs -- for layers 0..last_row (-1: the input conversion alone), then copies the WHOLE buffer `buf` as stored to `out`
 * (device): max_crops x buf_floats_per_crop[buf] floats, zero borders and the crops at n and above included; each layer writes
 * crop i of its output at i x its own per-crop geometry ((hw + 2 pad)^2 x channels). buf = -1 is the stem's input
 * [max_crops][S + 6][S + 6][4] (S = 128 without a kind-3 row). Under PA_DTYPE_BF16 a bf16 buffer (and buf = -1) is copied as stored, 2 bytes per element, and
 * out_bytes is checked against that size. PA_ERR_INVALID_ARG for a row or buffer out of range, n outside 1..max_crops or out_bytes short of
 * the buffer; nothing is enqueued then. pa_convnet_layer_forms: the form each layer ran as in the last forward or trace (a
 * launcher that refuses a shape passes the layer on to the next form); forms: host int32[cap], cap >= n_descs. */
int pa_convnet_trace(pa_convnet* h, const float* x, int32_t n, int32_t last_row, int32_t buf, void* out, size_t out_bytes, void* stream);
typedef enum pa_cn_form {
    PA_CN_FORM_NOT_RUN = 0,
    PA_CN_FORM_STEM_POOL = 1,       /* stem + max-pool, stem_pool.hip */
    PA_CN_FORM_AVGPOOL = 2,         /* global average pool */
    PA_CN_FORM_WINO = 3,            /* Winograd F(2x2, 3x3), wino.hip */
    PA_CN_FORM_PATCH = 4,           /* patch-resident 3x3, patchconv.hip */
    PA_CN_FORM_IGEMM_128x128 = 5,   /* implicit GEMM, igemm.hip, 128 x 128 tiles */
    PA_CN_FORM_IGEMM_128x64 = 6,    /* ... 128 x 64 tiles */
    PA_CN_FORM_IGEMM_64x64 = 7,     /* ... 64 x 64 tiles */
    PA_CN_FORM_PSGEMM = 8,          /* emulated-fp32 persistent GEMM, psgemm.hip (PA_DTYPE_EMULATED_F32) */
    PA_CN_FORM_BGEMM = 9,           /* one-slice bf16 persistent GEMM, bgemm.hip (PA_DTYPE_BF16) */
    PA_CN_FORM_BGEMM_SPLITK = 10,   /* ... its split-K form */
    PA_CN_FORM_AVGPOOL_BF16 = 11    /* global average pool of a bf16 map, fp32 out (PA_DTYPE_BF16) */
} pa_cn_form;
/* Appended: the form of a kind-3 row (stem + max-pool of any size, stem_pool_any.hip), reported by pa_convnet_layer_forms like
 * the values above. A constant beside the enumeration, not a thirteenth enumerator: the list above and its Python mirror
 * (_lib.CN_FORMS) are compared entry by entry by the ABI-15 tests and stay as they are; _lib.CN_FORM_NAMES has the name. */
#define PA_CN_FORM_STEM_POOL_ANY 12
int pa_convnet_layer_forms(const pa_convnet* h, int32_t* forms, int32_t cap);

/* One stride-1 3x3 convolution (padding 1) on the Winograd F(2x2, 3x3) kernel of the fp32 convolution stack
 * (csrc/wino.hip) -- the operator the engine's ResNet-18 / the detector's Bottlenecks run their stride-1 3x3 layers on,
 * exposed for parity tests and measurements of single layers. x: float32[n][height + 2][width + 2][in_px_stride]
 * (device, zero border of one pixel, the first `cin` channels of every pixel are read); out:
 * float32[n][height + 2 out_pad][width + 2 out_pad][out_px_stride] (interior written, first `cout` channels);
 * residual: addressed like out, or NULL; act: 0 none, 1 ReLU, 2 SiLU; res_after: 1 = the residual is added after the
 * activation. height, width multiples of 4; cin % 8 == 0; cout % 32 == 0. Filters: pa_wino_transform_weights turns
 * BatchNorm-folded [cout][ky][kx][cin] (host) into the kernel's layout (host, pa_wino_weight_floats floats), which
 * the caller uploads. `bn` = output channels per workgroup (64 | 32), part of that layout and of the launch:
 * pa_wino_channels_per_workgroup gives the value the engine would pick for a layer of `cout` channels launched over
 * `sub_blocks` = n * height / 4 * width / 4 sub-blocks (32 when 64-channel workgroups would not fill the chip). Enqueue only. */
size_t pa_wino_weight_floats(int32_t cin, int32_t cout);
int pa_wino_channels_per_workgroup(int32_t cout, int64_t sub_blocks);
int pa_wino_transform_weights(const float* w_host, int32_t cin, int32_t cout, int32_t bn, float* ug_host);
int pa_wino_conv3x3(const float* x, const float* ug, const float* bias, const float* residual, float* out, int32_t n,
                    int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t bn, int32_t in_px_stride,
                    int32_t out_px_stride, int32_t out_pad, int32_t act, int32_t res_after, void* stream);
/* The same launch with split-K scratch (ABI 10): where the layer's tiles alone would leave CUs without a workgroup (few pixels,
 * many channels: ResNet-18's 8 x 8 and 4 x 4 maps) the launcher lets 2 / 4 / 8 workgroups share a tile, each summing a run of
 * input-channel chunks; their partial output tiles meet in `slab` and the last workgroup to arrive adds them IN SPLIT ORDER
 * (results do not depend on arrival order) and runs the epilogue. slab: device scratch of slab_floats floats (16 MB covers
 * every launch: 256 x 512 x 32 floats); tickets: int32[n_tickets] on the device, ZERO before the first launch -- the kernel
 * leaves them zero; a launch with more tiles than tickets, or too small a slab, runs unsplit. Launches that share the scratch
 * belong on one stream. */
int pa_wino_conv3x3_splitk(const float* x, const float* ug, const float* bias, const float* residual, float* out, int32_t n,
                           int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t bn, int32_t in_px_stride, int32_t out_px_stride,
                           int32_t out_pad, int32_t act, int32_t res_after, float* slab, size_t slab_floats, int32_t* tickets,
                           int32_t n_tickets, void* stream);

/* One convolution (1x1 or 3x3, stride 1 or 2, "same" padding) + bias + activation (+ residual) on the persistent implicit-GEMM
 * kernels -- the operator the detection network's layers (ai_runner.py:191-224's YOLOv5s) and, under PA_DTYPE_EMULATED_F32, the
 * ResNet-18's 3x3 convolutions (cnn_action_detector.py:16,32) run on -- exposed for parity tests and per-layer measurements.
 * x: float32[n][height + 2 in_pad][width + 2 in_pad][in_px_stride] (device, zero border, the first cin channels of a pixel are
 * read; in_pad >= (ksize - 1) / 2); out: float32[n][oh + 2 out_pad][ow + 2 out_pad][out_px_stride], oh = height / stride
 * (interior written, first cout channels); residual: addressed like out (it may BE out), or NULL; act: 0 none, 1 ReLU, 2 SiLU;
 * res_after: 1 = the residual is added after the activation. cin, cout multiples of 32; pixel strides multiples of 4 floats and
 * x, w, out, residual 16-byte aligned (PA_ERR_INVALID_ARG otherwise: the kernels move 16-byte units). Weights: pa_conv_pack_weights turns
 * BatchNorm-folded [cout][ky][kx][cin] fp32 (host) into what the kernel of `compute_dtype` reads (host, pa_conv_weight_bytes
 * bytes; the caller uploads it): PA_DTYPE_F32 = the same fp32 values (csrc/pigemm.hip; no residual), PA_DTYPE_EMULATED_F32 = three
 * bf16 slices per weight in the LDS stage-image order of csrc/psgemm.hip, whose tile width depends on has_residual. Enqueue only. */
size_t pa_conv_weight_bytes(int32_t cin, int32_t cout, int32_t ksize, int32_t compute_dtype, int32_t has_residual);
int pa_conv_pack_weights(const float* w_host, int32_t cin, int32_t cout, int32_t ksize, int32_t compute_dtype, int32_t has_residual,
                         void* out_host);
int pa_conv2d(const float* x, const void* w, const float* bias, const float* residual, float* out, int32_t n, int32_t height,
              int32_t width, int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t in_pad, int32_t in_px_stride,
              int32_t out_px_stride, int32_t out_pad, int32_t act, int32_t res_after, int32_t compute_dtype, void* stream);
/* The opener of a ResNet block with its downsample branch (csrc/pigemm.hip, pgemm_branch_kernel): pa_conv2d's 3x3 stride-2
 * convolution into `out`, and from the SAME pass over x the block's 1x1 stride-2 branch out2 = x(2 y, 2 x) . w2 -- w2 float32
 * [cout][cin] (device), out2 addressed like out, no bias, no activation -- computed on the 3x3's centre tap, which reads those
 * pixels. Both outputs have the bits of the two pa_conv2d calls they replace. PA_DTYPE_F32 only; PA_ERR_INVALID_ARG for anything
 * but ksize 3, stride 2, in_px_stride == cin, cout a multiple of 64, act 0 | 1, no residual. residual, ksize, stride and res_after
 * exist so that the argument list is pa_conv2d's plus w2 and out2: they must be NULL, 3, 2 and 0. Appended: PA_ABI_VERSION stays 15,
 * no existing layout changes. Enqueue only. */
int pa_conv2d_branch(const float* x, const void* w, const float* bias, const float* residual, float* out, const float* w2, float* out2,
                     int32_t n, int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t in_pad,
                     int32_t in_px_stride, int32_t out_px_stride, int32_t out_pad, int32_t act, int32_t res_after, int32_t compute_dtype,
                     void* stream);

/* The ResNet-18 stem on integer pixels (csrc/stem_pool.hip, its third form): 7x7/2 convolution + folded BatchNorm + ReLU + 3x3/2
 * max-pool of u8 crops, the operator the exact engines (PA_DTYPE_F32, PA_DTYPE_EMULATED_F32) run on every model input they make from
 * u8 pixels -- exposed for parity tests and measurements of the single layer. crops_u8: uint8[n][128][128][3] (device); the pixel
 * integers go as bf16 into the interior of `packed` = bf16[n][134][134][4] (device scratch, 16-byte aligned, ZERO before the first
 * call: border and fourth channel are never written with anything else), are multiplied EXACTLY with the three bf16 slices of the
 * fp32 weights on the bf16 matrix cores, summed in fp32 (slice 2, 1, 0; taps in (ky, kx, channel) order), divided by 255 once
 * (correctly rounded), + bias, ReLU, max-pool -> out: float32[n][34][34][64] (device, interior written, the border of one pixel
 * is the caller's zero). w_slices: bf16[3][64][224] (device), made on the host by pa_stem_int_pack_weights from the BatchNorm-folded
 * fp32 weights [64][ky 7][kx 7][cin 3]: s0 = bf16(w), s1 = bf16(w - s0), s2 = bf16(w - s0 - s1), w = s0 + s1 + s2 exactly.
 * bias: float32[64] (device). PA_ERR_INVALID_ARG for a NULL or misaligned pointer or n outside 1..8192, before anything is
 * enqueued. Appended: PA_ABI_VERSION stays 15, no existing layout changes. Enqueue only. */
int pa_stem_int_pack_weights(const float* w_host, uint16_t* out_host);
int pa_stem_int(const uint8_t* crops_u8, const void* w_slices, const float* bias, void* packed, float* out, int32_t n, void* stream);

/* Head of ResnetTransformerDetector (resnet_transformer_detector.py:41-93,141): Linear(in_dim, hidden_dim), the
 * enc_dim-value time encoding of the frame slot appended (d_model = hidden_dim + enc_dim, 32 per head),
 * num_layers post-norm nn.TransformerEncoderLayer (ReLU feed-forward of ff_dim), Linear(d_model, num_actions),
 * log_softmax. blob: int32[16] header {PA_ENCODER_MAGIC, 1, in_dim, hidden_dim, slots, enc_dim, num_heads,
 * num_layers, ff_dim, num_actions, 0...}, then float32: resnet_ffn.weight [hidden, in_dim], .bias, freq_encoding
 * [slots, enc_dim], per layer self_attn.in_proj_weight [3D, D], in_proj_bias, out_proj.weight [D, D], .bias,
 * linear1.weight [ff, D], .bias, linear2.weight [D, ff], .bias, norm1.weight, .bias, norm2.weight, .bias, then
 * classifier.weight [A, D], .bias. */
typedef struct pa_encoder pa_encoder;
size_t pa_encoder_blob_bytes(int32_t in_dim, int32_t hidden_dim, int32_t slots, int32_t enc_dim, int32_t num_layers,
                             int32_t ff_dim, int32_t num_actions);
int pa_encoder_create(int32_t device, int32_t in_dim, int32_t hidden_dim, int32_t slots, int32_t enc_dim, int32_t num_heads,
                      int32_t num_layers, int32_t ff_dim, int32_t num_actions, int32_t max_rows, const void* blob_host,
                      size_t blob_bytes, pa_encoder** out);
void pa_encoder_destroy(pa_encoder* h);
const char* pa_encoder_last_error(const pa_encoder* h);
/* feats float32[seq_len * batch, ld] (device, row r = l * batch + n; the first in_dim values of a row are read) ->
 * logp float32[seq_len * batch, num_actions]. As in the reference (an encoder without batch_first fed
 * [B, S, 256], :82-84) seq_len is the number of WINDOWS and batch = slots the frames of a window. */
int pa_encoder_forward(pa_encoder* h, const float* feats, int32_t ld, int32_t seq_len, int32_t batch, float* logp, void* stream);

/* ---- measurement -------------------------------------------------------- */

/* When enabled, every kernel launch is bracketed by HIP events recorded on the
 * stream it is launched on. pa_profile_read synchronises that stream, returns
 * one row per kernel family and clears the log. */
int pa_profile_enable(pa_engine* e, int32_t on);
int pa_profile_read(pa_engine* e, pa_kernel_stat* stats, int32_t max_stats, int32_t* n_stats);

/* quality 1..100: every 128 x 128 crop the engine cuts (pa_square_crops, pa_backbone_frames*, pa_infer_clip,
 * pa_preprocess_*) additionally goes through the pixel arithmetic of a baseline JPEG write + read at that quality
 * (4:2:0, integer DCT), as the reference's cv2.imwrite / cv2.imread of every crop does (ai_runner.py:420,446; OpenCV's
 * default quality is 95) -- the returned crops and the model input then carry the codec's loss. 0 (the default)
 * switches it off: crops are the exact resampler output. Crop IMAGES handed to pa_runner_inputs /
 * pa_backbone_crop_images are taken as already decoded. */
int pa_set_crop_jpeg_quality(pa_engine* e, int32_t quality);

/* Keeps `stream` busy for about `microseconds` (one spinning thread; 0..100000). A probe, not a workload: two
 * HIP streams that the runtime multiplexed onto one hardware queue run such kernels strictly in turn, two that sit
 * on different queues side by side (playaid_core_amd/parallel.py picks the streams of its lanes with it). */
int pa_stream_spin(pa_engine* e, int32_t microseconds, void* stream);

/* A gate the HOST opens: pa_stream_gate enqueues a one-thread kernel that keeps `stream` busy until pa_stream_gate_open is
 * called (a store to coherent pinned memory the kernel polls), or max_microseconds (1..100000) have passed -- the bound
 * makes a gate nobody opens cost that long instead of hanging the queue. One gate per engine at a time.
 * playaid_core_amd/parallel.py (ClipLanes) enqueues the first clip of every lane behind an event recorded after one gate
 * and opens it when the last of them is enqueued, so the lanes start together whatever the host's submit times were. */
int pa_stream_gate(pa_engine* e, int32_t max_microseconds, void* stream);
int pa_stream_gate_open(pa_engine* e);

/* Blocks until all work enqueued on `stream` is done (hipStreamSynchronize). */
int pa_stream_sync(pa_engine* e, void* stream);

/* ---- scoring ------------------------------------------------------------ */

/* Scores log-probabilities against labels on the device: the NLL loss and multiclass top-1 accuracy of the reference's
 * validation_step / test_step (cnn_action_detector.py:131-163, the same in the other two models) and the confusion matrix,
 * "% correct" and "mean confidence" of visualizations/cnn_action_detector_vis.py:89-153, accumulated over any number of
 * pa_eval_update calls (an epoch) and read once. The handle belongs to no engine: it takes the log-probabilities of any
 * of the three models. Not thread-safe; the calls of one handle go to one stream (or to streams the caller orders).
 *
 * pa_eval_update: logp float32[n][ld] (device; ld >= num_actions, columns >= num_actions are never read), row i is
 * scored against labels[i * label_stride] (int32, device). label_stride 1 = a plain label array; 4 with
 * labels = &records->action_id = a pa_record array, so that another run's predictions serve as the labels (agreement of
 * two arithmetics with nothing on the host). The prediction of a row is its first maximum (torch.argmax, pa_record's
 * action_id). A label PA_EVAL_IGNORE (F.nll_loss's default ignore_index; frames without ground truth) skips the row and
 * counts it in `ignored`; any other label outside [0, num_actions) skips the row and counts it in `bad_labels`.
 * Otherwise rows += 1, correct += (prediction == label), nll_sum += -logp[i][label], conf_sum += exp(logp[i][prediction])
 * (both taken in double), confusion[label][prediction] += 1 (row = actual, column = predicted, as sklearn lays it out).
 * n == 0 is a no-op. Enqueue only.
 *
 * Determinism: the integers are exact in any order; the two double sums use no floating-point atomics (ordered slabs:
 * one partial per workgroup, folded in a fixed order by a second launch), so the same calls in the same order give the
 * same bits.
 *
 * pa_eval_read is the only call that waits: it copies the totals (and, when confusion_host is not NULL, the
 * int64[num_actions * num_actions] matrix) to the host behind everything enqueued on `stream`. It returns
 * PA_ERR_BAD_LABELS when bad_labels != 0 -- the totals and the matrix are filled all the same. pa_eval_reset zeroes the
 * state (enqueued). pa_eval_create / pa_eval_update check their arguments before any device call (null handle or
 * pointers, device < 0, num_actions outside 1..4096, ld < num_actions, n < 0, label_stride < 1: PA_ERR_INVALID_ARG); a create that
 * stops at the device (PA_ERR_NO_DEVICE / PA_ERR_HIP) still hands the handle back, to be destroyed by the caller. */
typedef struct pa_eval pa_eval;
typedef struct pa_eval_totals {
    int64_t rows, correct, ignored, bad_labels;
    double nll_sum, conf_sum;
} pa_eval_totals;
#define PA_EVAL_IGNORE (-100)
int pa_eval_create(int32_t device, int32_t num_actions, pa_eval** out);
void pa_eval_destroy(pa_eval* h);
int pa_eval_reset(pa_eval* h, void* stream);
int pa_eval_update(pa_eval* h, const float* logp_dev, int32_t ld, int32_t n, const int32_t* labels_dev, int32_t label_stride,
                   void* stream);
int pa_eval_read(pa_eval* h, pa_eval_totals* totals_host, int64_t* confusion_host, void* stream);

/* ---- annotation --------------------------------------------------------- */

/* Draws the reference annotator's boxes and labels (playaid/annotator.py:79-145, box_label's Pillow branch -- the one
 * Manuscript.render always takes, because set_frame's default `example` is not ASCII) on frames in HBM and pads them
 * (maybe_pad_image's np.pad, :300-363) in the same pass: ONE launch per call copies n frames and paints what the draw
 * lists touch. Append-only like the scoring calls above: PA_ABI_VERSION stays 15, no existing layout changes.
 *
 * frames_in uint8[n][H][W][3] BGR (device) -> frames_out uint8[n][H + pad_bottom][pad_left + W + pad_right][3] BGR
 * (device, a different buffer; the padding is zeros). items[n][PA_ANNOT_MAX_ITEMS], counts[n] and text[text_bytes] are
 * HOST arrays, checked and copied by the call (a handle keeps four calls' lists in flight and waits for the oldest
 * before it takes a fifth, so calls may go to any streams; the handle itself is not thread-safe).
 *
 * An item is one box_label call. Per item, on the device (Pillow's ImageDraw, pinned against Pillow 12.2):
 *   1. draw_box and line_width > 0: ImageDraw.rectangle(box, outline=rgb, width=line_width) -- in WHITE without has_color
 *      (outline=None makes ImageDraw fall back to its default ink). For a box
 *      at least 2 * line_width on a side that is line_width nested one-pixel frames; for thinner ones Pillow's
 *      vertical strokes run between y0 + width and y1 - width + 1 whichever way round, and may leave the box
 *      (csrc/annotate.hip states the rule). A reversed box is drawn as Pillow's C routine draws it (rows swapped);
 *      current Pillow refuses such a box before it gets there, and so does playaid_core_amd/annotator.py.
 *   2. text_len > 0: w = cell_w * text_len, h = cell_h, outside = box[1] - h >= 0, y = outside ? box[1] - h : box[1];
 *      has_color: ImageDraw.rectangle((box[0], y, box[0] + w + 1, y + h + 1), fill=rgb), both corners inclusive;
 *      then the text at (box[0], y) in WHITE (the reference's Pillow branch ignores txt_color): cell k of the string is
 *      atlas[text[k]][text[k + 1]], the last one atlas[text[k]][n_chars] -- Pillow's bitmap font lets the next
 *      character decide a cell's last column.
 * Everything is clipped to the INPUT frame area; items are painted in list order, a later one over an earlier one.
 * A colour (r, g, b) lands in the BGR frame as (b, g, r): the reference draws RGB on RGBA and converts on write.
 *
 * atlas: uint8[n_chars][n_chars + 1][cell_h][cell_w] (host; non-zero = ink), uploaded by pa_annot_create; text holds
 * character codes first_char .. first_char + n_chars - 1. PA_ERR_INVALID_ARG, before any device work, for: null
 * pointers, n < 0 or H, W < 1 or a negative pad or an output side above 32768, frames_in == frames_out, a count
 * outside 0..max_items, line_width outside 0..32767, a text range outside text_bytes, text_bytes > max_text, a
 * character code outside the atlas; PA_ERR_CAPACITY for n > max_frames. n == 0 is a no-op. Enqueue only. */
#define PA_ANNOT_MAX_ITEMS 16
typedef struct pa_annot pa_annot;
typedef struct pa_annot_item {
    int32_t box[4];      /* x0, y0, x1, y1 as given to box_label: any values (taken as clamped to +-2^29) */
    int32_t draw_box;    /* 0 / 1 */
    int32_t line_width;
    int32_t has_color;   /* 0 = box_label(color=None): no background, white text, and a WHITE outline if draw_box */
    int32_t text_off;    /* first character of the label in `text` */
    int32_t text_len;    /* 0 = no label */
    uint8_t rgb[3];
    uint8_t reserved;
} pa_annot_item;
int pa_annot_create(int32_t device, const uint8_t* atlas_host, int32_t cell_w, int32_t cell_h, int32_t first_char, int32_t n_chars,
                    int32_t max_frames, int32_t max_items, int32_t max_text, pa_annot** out);
int pa_annotate_frames(pa_annot* h, const uint8_t* frames_in, int32_t n, int32_t height, int32_t width, const pa_annot_item* items_host,
                       const int32_t* counts_host, const uint8_t* text_host, int32_t text_bytes, int32_t pad_left, int32_t pad_right,
                       int32_t pad_bottom, uint8_t* frames_out, void* stream);
void pa_annot_destroy(pa_annot* h);

/* ---- training the temporal head ------------------------------------------ */

/* Trains CNNActionDetector's temporal head -- cnn1d.0, classifier.0, classifier.2; the ResNet-18 encoder and its fc stay
 * frozen -- on feature rows the engine has already computed (pa_backbone_windows, pa_features_export), with the reference's
 * loss and optimiser (cnn_action_detector.py:94-116, 165-167: F.nll_loss on the window's centre label, torch.optim.Adam with
 * its default betas and eps). Append-only: PA_ABI_VERSION stays 15.
 *
 * The weights are updated IN PLACE in the engine's arena, in the layouts the inference kernels read, so the next
 * pa_infer_windows / pa_head_frames / captured graph / pa_weights_export sees the step without a re-pack. The trainer owns
 * the two Adam moments (same layouts) and the step's scratch. It borrows the engine: destroy the trainer first, and do not
 * run a step concurrently with inference on another stream.
 *
 * pa_head_train_step, all pointers on the device: feats float32[n_rows][PA_FEATURE_STRIDE] (16-byte aligned, 1000 used),
 * gather int32[batch][S] row indices into feats (the kernels clamp them into [0, n_rows)), labels int32[batch] in
 * [0, num_actions) or PA_EVAL_IGNORE (any other value is treated as PA_EVAL_IGNORE). With n = the number of labelled
 * windows, loss = -(1/n) sum logp[b][labels[b]]; n == 0 divides by 1 (loss 0, all gradients 0) where torch gives NaN.
 *   apply = 1: one optimiser step (step count k += 1):  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *              w -= (lr / (1 - beta1^k)) * m / (sqrt(v) / sqrt(1 - beta2^k) + eps). grads_out may be NULL.
 *   apply = 0: nothing changes; grads_out receives the six gradients, concatenated, in PyTorch layouts and blob order:
 *              cnn1d.0.weight [512][1000][S], cnn1d.0.bias [512], classifier.0.weight [128][512], classifier.0.bias [128],
 *              classifier.2.weight [A][128], classifier.2.bias [A]  (512000 S + 66176 + 129 A floats).
 * stats_dev (may be NULL) receives the step's pa_train_stats: the loss BEFORE the update, the number of labelled windows and
 * how many of them the model got right (first maximum). Enqueue only: stream-ordered, nothing is read back, every sum has
 * a fixed order (no floating-point atomics), so the same calls give the same bits.
 *
 * pa_head_trainer_read copies one set of six tensors (weights, first or second moments) to out_dev in the PyTorch layouts
 * above; floats must be that total. With PA_TRAIN_RAW or-ed into `which` the set is copied as it lies on the device instead:
 * [512][S][1024] (columns 1000..1023 are padding), [512], k-major [512][128], [128], k-major [128][64] (columns A..63 are
 * padding), [A] -- 524288 S + 74368 + A floats; padding has gradient 0 and stays bitwise zero. Enqueue only.
 *
 * PA_ERR_INVALID_ARG before any device call: null handle or pointers, batch < 1, batch > max_batch, max_batch outside 1..256,
 * lr or eps not finite or <= 0, a beta outside [0, 1), apply outside {0, 1}, apply = 0 without grads_out, n_rows < 1. A create
 * that stops at the device (PA_ERR_NO_DEVICE / PA_ERR_HIP) still hands the handle back, to be destroyed by the caller. */
typedef struct pa_head_trainer pa_head_trainer;
typedef struct pa_adam_config {
    float lr, beta1, beta2, eps;
} pa_adam_config;
typedef struct pa_train_stats {
    float loss;
    int32_t valid;
    int32_t correct;
    int32_t pad;
} pa_train_stats;
#define PA_TRAIN_WEIGHTS 0
#define PA_TRAIN_M 1
#define PA_TRAIN_V 2
#define PA_TRAIN_RAW 16 /* or-ed in: the set as it lies on the device, padding included (see pa_head_trainer_read) */
int pa_head_trainer_create(pa_engine* e, const pa_adam_config* cfg, int32_t max_batch, pa_head_trainer** out);
void pa_head_trainer_destroy(pa_head_trainer* t);
const char* pa_head_trainer_last_error(const pa_head_trainer* t);
int64_t pa_head_trainer_steps(const pa_head_trainer* t);
int pa_head_train_step(pa_head_trainer* t, const float* feats, int32_t n_rows, const int32_t* gather, const int32_t* labels, int32_t batch,
                       int32_t apply, float* grads_out, pa_train_stats* stats_dev, void* stream);
int pa_head_trainer_read(pa_head_trainer* t, int32_t which, float* out_dev, size_t floats, void* stream);

/* ---- training the LSTM head ----------------------------------------------- */

/* Trains RNNActionDetector's recurrent head -- every lstm.weight_ih / weight_hh / bias_ih / bias_hh, action_decoder.0 and
 * action_decoder.2; resnet.* (resnet.fc.0 included) stays frozen -- on feature rows already computed (pa_backbone_windows), with
 * the reference's loss and optimiser (rnn_action_detector.py:97-117, 162-164: F.nll_loss over every (window, frame) row,
 * torch.optim.Adam with its default betas and eps). Append-only: PA_ABI_VERSION stays 15.
 *
 * The trainer borrows the pa_lstm handle's weights and updates them IN PLACE, where pa_lstm_forward reads them (PyTorch
 * layouts: there is no other form, PA_TRAIN_RAW is refused). It owns the two Adam moments and the saved activations, sized for
 * the handle's max_rows. Destroy the trainer before the handle, and do not run a step concurrently with pa_lstm_forward on
 * another stream. The hidden size must be a multiple of 32 (the served 512 is); other handles stay inference-only.
 *
 * pa_lstm_train_step, all pointers on the device: x float32[seq_len * batch][ld] (input_dim used), as pa_lstm_forward takes it:
 * seq_len time steps (the windows) of batch <= 16 rows (a window's frames), zero initial state; labels int32[seq_len * batch]
 * in [0, num_actions) or PA_EVAL_IGNORE (any other value is treated as PA_EVAL_IGNORE). With n = the number of labelled rows,
 * loss = -(1/n) sum logp[r][labels[r]]; n == 0 divides by 1 (loss 0, all gradients 0) where torch gives NaN.
 *   apply = 1: one optimiser step, as pa_head_train_step's; one step counter serves all tensors. grads_out may be NULL.
 *   apply = 0: nothing changes; grads_out receives the gradients, concatenated, in the blob's tensor order and PyTorch layouts:
 *              per layer w_ih [4H][in], w_hh [4H][H], b_ih [4H], b_hh [4H], then action_decoder.0.weight [128][H], .bias [128],
 *              action_decoder.2.weight [A][128], .bias [A]  (pa_lstm_trainer_floats floats).
 * stats_dev (may be NULL) receives the step's pa_train_stats: the loss BEFORE the update, the labelled rows and how many of
 * them the model got right (first maximum). Enqueue only: stream-ordered, nothing is read back, one launch per time step and
 * layer in each direction (no kernel waits for another workgroup), every sum in a fixed order: the same calls give the same bits.
 *
 * pa_lstm_trainer_read copies one set (PA_TRAIN_WEIGHTS, PA_TRAIN_M, PA_TRAIN_V) to out_dev in that order; floats must be
 * pa_lstm_trainer_floats(handle). Enqueue only.
 *
 * PA_ERR_INVALID_ARG before any device call: null handle or pointers, seq_len < 1, batch outside 1..16, seq_len * batch >
 * max_rows, ld < input_dim, apply outside {0, 1}, apply = 0 without grads_out, lr or eps not finite or <= 0, a beta outside
 * [0, 1), a hidden size that is no multiple of 32, PA_TRAIN_RAW. A create that stops at the device (PA_ERR_NO_DEVICE /
 * PA_ERR_HIP) still hands the trainer back, to be destroyed by the caller. */
typedef struct pa_lstm_trainer pa_lstm_trainer;
int pa_lstm_trainer_create(pa_lstm* h, const pa_adam_config* cfg, pa_lstm_trainer** out);
void pa_lstm_trainer_destroy(pa_lstm_trainer* t);
const char* pa_lstm_trainer_last_error(const pa_lstm_trainer* t);
int64_t pa_lstm_trainer_steps(const pa_lstm_trainer* t);
int pa_lstm_train_step(pa_lstm_trainer* t, const float* x, int32_t ld, int32_t seq_len, int32_t batch, const int32_t* labels, int32_t apply,
                       float* grads_out, pa_train_stats* stats_dev, void* stream);
int pa_lstm_trainer_read(pa_lstm_trainer* t, int32_t which, float* out_dev, size_t floats, void* stream);
size_t pa_lstm_trainer_floats(const pa_lstm* h);

/* ---- training the transformer-encoder head ------------------------------------ */

/* Trains ResnetTransformerDetector's head -- resnet_ffn, every transformer layer's self_attn.in_proj / out_proj, linear1,
 * linear2, norm1, norm2, and the classifier; the ResNet-50, freq_encoding and resnet_classifier stay as loaded -- on feature
 * rows already computed (pa_convnet_forward), with the reference's loss and optimiser (resnet_transformer_detector.py:143-164,
 * 207-209: F.nll_loss over every (window, frame) row in train mode, i.e. with the encoder layers' dropout; torch.optim.Adam with
 * its default betas and eps). Append-only: PA_ABI_VERSION stays 15.
 *
 * The trainer borrows the pa_encoder handle's weights and updates them IN PLACE, where pa_encoder_forward reads them (PyTorch
 * layouts: there is no other form, PA_TRAIN_RAW is refused); after an applied step the handle's zero-padded copy of the front
 * projection is refreshed on the stream. It owns the two Adam moments and the saved activations, sized for the handle's
 * max_rows; the handle's inference buffers are not touched. Destroy the trainer before the handle, and do not run a step
 * concurrently with pa_encoder_forward on another stream.
 *
 * A handle is trainable when num_actions <= 64, ff_dim % 32 == 0 and max_rows >= slots (the 32-wide heads of every pa_encoder make
 * hidden_dim + enc_dim a multiple of 32); anything else is refused at create with PA_ERR_INVALID_ARG and a message on the
 * pa_encoder handle. pa_encoder_trainer_max_windows = min(64, max_rows / slots): the seq_len one step takes (the attention
 * kernels hold one (slot, head)'s seq_len x seq_len block in a workgroup); more returns PA_ERR_CAPACITY with a message.
 *
 * pa_encoder_train_step, all pointers on the device: feats float32[seq_len * batch][ld] (in_dim used) as pa_encoder_forward
 * takes them: seq_len windows (the attention's sequence) of batch = slots rows, row r = l * batch + n; labels int32[seq_len *
 * batch] in [0, num_actions) or PA_EVAL_IGNORE (any other value is treated as PA_EVAL_IGNORE). With n = the number of labelled
 * rows, loss = -(1/n) sum logp[r][labels[r]]; n == 0 divides by 1 (loss 0, all gradients 0) where torch gives NaN.
 *   apply = 1: one optimiser step, as pa_head_train_step's; one step counter serves all tensors. grads_out may be NULL.
 *   apply = 0: nothing changes; grads_out receives the gradients, concatenated, in the blob's order without freq_encoding and in
 *              PyTorch layouts: resnet_ffn.weight [hidden][in], .bias [hidden]; per layer in_proj_weight [3D][D], in_proj_bias
 *              [3D], out_proj.weight [D][D], .bias [D], linear1.weight [ff][D], .bias [ff], linear2.weight [D][ff], .bias [D],
 *              norm1.weight, .bias, norm2.weight, .bias [D]; classifier.weight [A][D], .bias [A]
 *              (pa_encoder_trainer_floats floats). pa_encoder_trainer_read uses the same order.
 * stats_dev (may be NULL) receives the step's pa_train_stats: the loss BEFORE the update, the labelled rows and how many of
 * them the model got right (first maximum). Enqueue only: stream-ordered, nothing is read back, no kernel waits for another
 * workgroup, every sum has a fixed order and there are no floating-point atomics: the same calls give the same bits.
 *
 * Dropout (`dropout` = p in [0, 1), `seed`): four sites per layer, each element kept with probability 1 - p and scaled by
 * 1 / (1 - p) (fp32: 1.f / (1.f - p)), the same mask in the forward and the backward pass:
 *   site 0  the attention probabilities, element index i in torch's layout [batch * heads][seq_len][seq_len]
 *   site 1  the attention block's output before the residual, [rows][D]
 *   site 2  the feed-forward activation after the ReLU, [rows][ff]
 *   site 3  the feed-forward output before the residual, [rows][D]
 * keep(seed, step, layer, site, i), all arithmetic on uint32 (wrapping), step = pa_encoder_trainer_steps before the call (so
 * an apply = 0 call and the apply = 1 call behind it see the same masks):
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16;  return x
 *   key = mix((uint32)seed + 0x9e3779b9)
 *   key = mix(key ^ (uint32)(seed >> 32))
 *   key = mix(key ^ (uint32)step)
 *   key = mix(key ^ (uint32)((uint64)step >> 32))
 *   key = mix(key ^ ((uint32)(layer * 4 + site + 1) * 0x85ebca6b))
 *   r   = mix(mix((uint32)i ^ key) + key)
 *   keep = r >= thr,  thr = (uint32)(uint64)((double)p * 4294967296.0)   (p the float handed to create)
 * It does not depend on the launch geometry; encoder_trainer.dropout_keep is its numpy twin. With p = 0 nothing is generated.
 *
 * pa_encoder_trainer_read copies one set (PA_TRAIN_WEIGHTS, PA_TRAIN_M, PA_TRAIN_V) to out_dev in the order above; floats must
 * be pa_encoder_trainer_floats(handle). Enqueue only.
 *
 * PA_ERR_INVALID_ARG before any device call: null handle or pointers, seq_len < 1, batch != slots, ld < in_dim, apply outside
 * {0, 1}, apply = 0 without grads_out, lr or eps not finite or <= 0, a beta outside [0, 1), dropout outside [0, 1), a handle that
 * is not trainable, PA_TRAIN_RAW. A create that stops at the device (PA_ERR_NO_DEVICE / PA_ERR_HIP) still hands the trainer
 * back, to be destroyed by the caller. */
typedef struct pa_encoder_trainer pa_encoder_trainer;
int pa_encoder_trainer_create(pa_encoder* h, const pa_adam_config* cfg, float dropout, uint64_t seed, pa_encoder_trainer** out);
void pa_encoder_trainer_destroy(pa_encoder_trainer* t);
const char* pa_encoder_trainer_last_error(const pa_encoder_trainer* t);
int64_t pa_encoder_trainer_steps(const pa_encoder_trainer* t);
int pa_encoder_train_step(pa_encoder_trainer* t, const float* feats, int32_t ld, int32_t seq_len, int32_t batch, const int32_t* labels,
                          int32_t apply, float* grads_out, pa_train_stats* stats_dev, void* stream);
int pa_encoder_trainer_read(pa_encoder_trainer* t, int32_t which, float* out_dev, size_t floats, void* stream);
size_t pa_encoder_trainer_floats(const pa_encoder* h);
int32_t pa_encoder_trainer_max_windows(const pa_encoder* h);

/* Appended (the version stays 15): one stride-1 3x3 convolution (padding 1) on a 4 x 4 map as Winograd F(4x4, 3x3) taken apart
 * (csrc/wino4.hip) -- an input transform, 36 grouped GEMMs on the exact persistent GEMM, an output transform with the epilogue:
 * three launches on `stream`. The form the fp32 engine runs ResNet-18's layer 4 on from PA_WINO_F4_MIN crops; exposed for parity
 * tests and measurements of single layers. Arguments as pa_wino_conv3x3 (x: float32[n][6][6][in_px_stride] with a zero ring, out:
 * float32[n][4 + 2 out_pad][4 + 2 out_pad][out_px_stride], interior written) without `bn`; height and width must be 4, cin and cout
 * multiples of 64. Filters: pa_wino4_transform_weights turns BatchNorm-folded [cout][ky][kx][cin] (host) into U[36][cout][cin]
 * (host, pa_wino4_weight_floats floats; 0 for channel counts the form does not take), which the caller uploads. scratch: device,
 * 16-byte aligned, scratch_floats >= 36 * ceil(n / 64) * 64 * (cin + cout). No K split: a crop's result does not depend on the
 * batch it is in. PA_ERR_INVALID_ARG for anything else. Enqueue only. */
size_t pa_wino4_weight_floats(int32_t cin, int32_t cout);
int pa_wino4_transform_weights(const float* w_host, int32_t cin, int32_t cout, float* u_host);
int pa_wino4_conv3x3(const float* x, const float* u, const float* bias, const float* residual, float* out, int32_t n, int32_t height,
                     int32_t width, int32_t cin, int32_t cout, int32_t in_px_stride, int32_t out_px_stride, int32_t out_pad, int32_t act,
                     int32_t res_after, float* scratch, size_t scratch_floats, void* stream);

/* Appended (the version stays 15): the reference's training augmentation of 128 x 128 crops, augment_char_crop
 * (dataset_utils.py:141-252), as ONE launch over crops that are already on the device (csrc/augment.hip).
 * Output crop i reads source crop params[i].src of src uint8[n_src][128][128][3] (RGB) and applies, in A.Compose's order:
 *   1 HorizontalFlip        flip != 0: source column 127 - u
 *   2 BrightnessContrast    table trunc(clip((float)k * alpha + beta * 255.f, 0, 255)), fp32, no fused multiply-add
 *   3 Blur                  blur_k 2 or 3 (0: none): box filter over step 2's values, window u - 1 .. u - 1 + (k - 1) (OpenCV's
 *                           anchor k / 2), reflect-101 border, sum / k^2 rounded to nearest, ties to even
 *   4 HueSaturationValue    skipped when the three shifts are all exactly 0; else OpenCV's 8-bit integer RGB -> HSV (H 0..179),
 *                           tables trunc((k + hue_shift) mod 180) and trunc(clip(k + shift, 0, 255)) in fp64, then HSV -> RGB in
 *                           fp32: h * (6.f / 180.f), s and v * (1.f / 255.f), OpenCV's sector form, rint(x * 255.f) clipped
 *   5 GaussNoise            noise_sigma > 0: per channel trunc(clip((float)byte + sigma * z, 0, 255)); z from the counter hash below
 *   6 PixelDropout          pixel_drop_thr != 0: all three bytes 0 where hash(stream 1, v * 128 + u) < thr
 *   7 CoarseDropout         n_holes holes of 4 x 4 at (holes[2 j], holes[2 j + 1]) = (x, y), zeroed
 *   8 ChannelDropout        channel c zeroed where channel_mask bit c is set (bit 0 = R)
 *   9 Downscale + RandomSizedCrop, both nearest neighbour, composed by the host: output pixel (x, y) is the chain's value at
 *                           (u, v) = (xmap[x], ymap[y])
 * Counter hash (mix as in the encoder trainer's dropout): k = mix((uint32)key + 0x9e3779b9); k = mix(k ^ (uint32)(key >> 32));
 * ks = mix(k ^ ((uint32)(stream + 1) * 0x85ebca6b)); r(i) = mix(mix((uint32)i ^ ks) + ks). Stream 0 is the noise with
 * i = (v * 128 + u) * 3 + c, stream 1 the pixel dropout with i = v * 128 + u: neither depends on the launch geometry.
 * z = q[r >> 22] + (float)(r & 0x3fffff) * 2^-22 * (q[(r >> 22) + 1] - q[r >> 22]) with q the handle's table of 1025 normal
 * quantiles (pa_augment_quantiles; adds and multiplies only on the device). augment.augment_reference is the numpy twin.
 *
 * The kernel is defined for ANY parameter bytes: src is clamped to [0, n_src), map entries are taken & 127, holes are clipped to
 * the image, n_holes is clamped to 0..8, channel_mask is taken & 7, a blur_k other than 2 or 3 is 0, a float that is not finite
 * counts as its identity value (alpha 1, the others 0) and finite ones are clamped to alpha 0..4, beta -2..2, hue -1024..1024,
 * sat / val -512..512, sigma 0..256. pa_augment_params_check (host only, no device call) returns PA_ERR_INVALID_ARG for
 * anything of that kind and for values outside the reference's limits: alpha outside [0.8, 1.2], beta outside [-0.2, 0.4], hue
 * outside [-256, 256], sat outside [-67, 67], val outside [-5, 5], sigma outside [0, sqrt(200)], a hole beyond 124, flip
 * outside {0, 1}, channel_mask outside 0..6.
 *
 * pa_augment_crops: src and params on the device (src and out 16-byte aligned), n >= 1, n_src >= 1; out_format PA_AUGMENT_U8 ->
 * out uint8[n][128][128][3], PA_AUGMENT_MODEL -> out float32[n][3][128][128] with value (float)byte / 255.f (the input of
 * pa_backbone_windows / pa_infer_windows). Enqueue only; nothing is read back. PA_ERR_INVALID_ARG otherwise. */
typedef struct pa_augment_params {
    int32_t src;
    int32_t flip;
    float alpha, beta;
    int32_t blur_k;
    float hue_shift, sat_shift, val_shift;
    float noise_sigma;
    uint32_t pixel_drop_thr;
    int32_t n_holes;
    uint8_t holes[16];
    int32_t channel_mask;
    uint8_t xmap[128];
    uint8_t ymap[128];
    uint64_t key;
} pa_augment_params;
#define PA_AUGMENT_U8 0
#define PA_AUGMENT_MODEL 1
#define PA_AUGMENT_QUANTILES 1025
int pa_augment_params_check(const pa_augment_params* host, int32_t n, int32_t n_src);
/* the table q: q[j] = the standard normal quantile at j / 1024 (fp64, rounded once) for 0 < j < 1024; q[0] = -q[1024] chosen so
 * that the outermost cells keep the normal's second moment over their probability 1 / 1024. out_host: float32[1025]. */
int pa_augment_quantiles(float* out_host);
int pa_augment_crops(pa_engine* e, const uint8_t* src_dev, int32_t n_src, const pa_augment_params* params_dev, int32_t n,
                     int32_t out_format, void* out_dev, void* stream);

/* Appended (the version stays 15): the reference's synthetic training frames -- load_and_augment_frame_to_stage_crop at
 * synth_difficulty 0 (ult_action_dataset.py:97-136), which get_synth and simple_dataset call once per frame -- as ONE launch
 * for n output frames from images that were uploaded once (csrc/synth_composite.hip). A bank holds images on
 * the device: PA_SYNTH_SPRITES the character renders as RGBA (cv2 reads BGRA; the loader swaps once, which commutes with a
 * per-channel resample), PA_SYNTH_STAGES the stage pictures as RGB. Output frame i with square side D = dim:
 *   1 stage crop     stage[stage_y : stage_y + D, stage_x : stage_x + D] of stage image params[i].stage
 *   2 sprite size    the sprite is h x w; imutils.resize in double precision: h > w: (ow, oh) = ((int)(w * (D / (double)h)), D),
 *                    else (ow, oh) = (D, (int)(h * (D / (double)w)))
 *   3 resample       cv2.resize(sprite, (ow, oh), INTER_AREA) of all four channels, each a plain channel (no premultiplication),
 *                    by the branch cv::resize takes: equal sizes copy; either axis enlarging -> the 8-bit bilinear resizer with
 *                    area-mode coefficients (11-bit weights, (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
 *                    both scales integers -> box sums ((s + 2) >> 2 for 2 x 2, else cvRound((float)s * (1.f / (float)area)));
 *                    else computeResizeAreaTab's weights in fp32: per source row the horizontal sum in table order, multiply
 *                    then add, then the vertical sum of beta * row the same way, then cvRound (ties to even) and saturate
 *   4 paste          Image.paste(sprite, (px, py), sprite): px = (D - ow) / 2 + paste_dx, py = (D - oh) / 2 + paste_dy, clipped
 *                    to the canvas; per covered pixel and channel c of R, G, B, with a the resampled alpha:
 *                    t = s_c * a + d_c * (255 - a) + 128; out_c = ((t >> 8) + t) >> 8   (Pillow's paste_mask_RGBA)
 *   5 output         PA_SYNTH_U8 -> uint8[n][D][D][3]; PA_SYNTH_MODEL (D = 128 only) -> float32[n][3][128][128] with value
 *                    (float)byte / 255.f, the input of pa_backbone_windows / pa_infer_windows
 * synth_dataset.composite_reference is the numpy twin.
 *
 * pa_synth_bank_create: images_host[k] points at image k's packed rows (heights[k] x widths[k] x 4 bytes for sprites, x 3 for
 * stages). Validated on the host before any device call -- n >= 1, sprite sides 1..PA_SYNTH_SPRITE_MAX, stage sides
 * 1..PA_SYNTH_STAGE_MAX, no sprite so thin that step 2 gives it an empty size (ow or oh 0, for which cv2.resize raises) at
 * every dim; PA_ERR_INVALID_ARG and a message otherwise -- then packed, each image 16-byte aligned, behind a descriptor table
 * into one device allocation and uploaded once. A sprite whose longer side is at most 32 times the shorter has ow, oh >= 1
 * at every dim >= 32; a thinner one only from some larger dim on, and pa_synth_params_check and pa_synth_composite return
 * PA_ERR_INVALID_ARG for a dim below the largest such bound of the bank's sprites. With e NULL the bank holds the sizes alone
 * (no device allocation): pa_synth_params_check takes it, pa_synth_composite refuses it. PA_ERR_CAPACITY: the host has no
 * memory for the packed copy (as large as the bank); PA_ERR_HIP: the device allocation or the upload failed. The kernel trusts the descriptors because only the library writes them. A bank is
 * independent of the launches that read it: a later producer of sprites can hand pa_synth_composite a bank of its own.
 *
 * The kernel is defined for ANY parameter bytes: sprite and stage are clamped into their banks, the stage origin into
 * [0, W - D] x [0, H - D], the paste offsets to +-PA_SYNTH_PASTE_MAX; the reserved words are not read.
 * pa_synth_params_check (host only, no device call) returns PA_ERR_INVALID_ARG for anything of that kind, for a non-zero
 * reserved word, for a dim outside PA_SYNTH_DIM_MIN..PA_SYNTH_DIM_MAX and for a record whose stage is smaller than dim.
 *
 * pa_synth_composite: params on the device (8-byte aligned), n 1..65535, dim PA_SYNTH_DIM_MIN..PA_SYNTH_DIM_MAX, out 16-byte
 * aligned, PA_SYNTH_MODEL only with dim == 128, every stage of the bank at least dim x dim. PA_ERR_INVALID_ARG otherwise.
 * Enqueue only; nothing is read back. */
typedef struct pa_synth_bank pa_synth_bank;
typedef struct pa_synth_params {
    int32_t sprite;              /* image of the sprite bank */
    int32_t stage;               /* image of the stage bank */
    int32_t stage_x, stage_y;    /* origin of the D x D stage crop */
    int32_t paste_dx, paste_dy;  /* added to the centred paste position */
    int32_t reserved[2];         /* zero */
} pa_synth_params;
#define PA_SYNTH_SPRITES 0
#define PA_SYNTH_STAGES 1
#define PA_SYNTH_U8 0
#define PA_SYNTH_MODEL 1
#define PA_SYNTH_DIM_MIN 32
#define PA_SYNTH_DIM_MAX 256
#define PA_SYNTH_SPRITE_MAX 1024
#define PA_SYNTH_STAGE_MAX 4096
#define PA_SYNTH_PASTE_MAX 4096
int pa_synth_bank_create(pa_engine* e, int32_t kind, const uint8_t* const* images_host, const int32_t* widths, const int32_t* heights,
                         int32_t n, pa_synth_bank** out);
void pa_synth_bank_destroy(pa_synth_bank* bank);
int pa_synth_params_check(const pa_synth_params* host, int32_t n, const pa_synth_bank* sprites, const pa_synth_bank* stages, int32_t dim);
int pa_synth_composite(pa_engine* e, const pa_synth_bank* sprites, const pa_synth_bank* stages, const pa_synth_params* params_dev,
                       int32_t n, int32_t dim, int32_t out_format, void* out_dev, void* stream);

/* Appended (the version stays 15): the reference's augmentation of a character render BEFORE the paste, augment_synth_char_crop
 * (dataset_utils.py:255-378, output_size = 128), which load_and_augment_frame_to_stage_crop runs on every render when
 * synth_difficulty is 1 or 2 (csrc/sprite_augment.hip). Output sprite i reads the h x w RGBA image
 * params[i].src of a PA_SYNTH_SPRITES bank and is written, as 128 x 128 RGBA, into slot i of a bank made by
 * pa_sprite_bank_create, which pa_synth_composite then takes like any other sprite bank:
 *   a resize to width 128   imutils.resize(width=128): cv2.resize(INTER_AREA) to 128 x h1, h1 = (int)(h * (128 / (double)w)), all
 *                           four channels plain channels, by the branch cv::resize takes (step 3 of pa_synth_composite)
 *   b ImageOps.pad          to (128, 128), transparent. h1 == 128: unchanged. h1 < 128: pasted (copied, no mask) at row
 *                           rint((128 - h1) * 0.5) (Python's round: ties to even). h1 > 128: Image.resize((w2, 128), BICUBIC),
 *                           w2 = rint(128 / (double)h1 * 128), as Pillow does it for RGBA -- every pixel to premultiplied RGBa
 *                           (c' = MULDIV255(c, a): t = c * a + 128, ((t >> 8) + t) >> 8; alpha kept), the horizontal then the
 *                           vertical 8-bit pass over all four channels (22-bit coefficients of precompute_coeffs, the sum starts
 *                           at 2^21, >> 22, clipped to 0..255), back to RGBA (alpha 0 or 255: unchanged, else
 *                           min(255, 255 * c / a), integer division) -- pasted at column rint((128 - w2) * 0.5)
 *   c shrink                new_scale != 0 (96..127): cv2.resize(INTER_AREA) to new_scale x new_scale, then ImageOps.expand with a
 *                           transparent border of 128 - new_scale: a canvas of side C = 256 - new_scale. Otherwise C = 128
 *   d the Compose           on the C x C canvas, RGB as the image and alpha as the mask. The image takes stages 1..8 of
 *                           pa_augment_crops with C for 128 wherever a size enters: the flip reads column C - 1 - u, the blur's
 *                           border reflects about C - 1, the stream positions are v * C + u, holes are squares of side
 *                           S = min(96, C / 3) at (holes[2 j], holes[2 j + 1]) = (x, y). Then output pixel (x, y) of the
 *                           O x O result (O = 128 when sized_crop != 0, else C) is the image's value at (xmap[x], ymap[y])
 *                           (Downscale then RandomSizedCrop, both nearest, composed by the host). The mask takes the flip, 0 at
 *                           dropped pixels and inside holes, nothing of the other stages, and is gathered at (axmap[x], aymap[y])
 *                           (RandomSizedCrop alone)
 *   e resize to width 128   O == 128: unchanged; else cv2.resize(INTER_AREA) of the four channels from C x C to 128 x 128
 * sprite_augment.augment_sprites_reference is the numpy twin.
 *
 * The kernel is defined for ANY parameter bytes: src is clamped into the bank, the floats are read as pa_augment_crops reads
 * them, n_holes is clamped to 0..2, channel_mask is taken & 7, a blur_k other than 2 or 3 and a new_scale outside 96..127 are
 * 0, sized_crop and flip count as 0 / 1, map entries are clamped to C - 1 (entries from O on are not read), holes are
 * comparisons. pa_sprite_aug_params_check (host only, no device call) returns PA_ERR_INVALID_ARG for anything of that kind and
 * for values outside the reference's limits: alpha outside [0.8, 1.2], beta outside [-0.2, 0.6], hue outside [-256, 256], sat
 * outside [-67, 67], val outside [-10, 10], a noise_sigma that is neither 0 nor in [sqrt(427.63), sqrt(500)], a pixel_drop_thr
 * that is neither 0 nor PA_SPRITE_DROP_THR (probability 0.1), a hole beyond C - S, channel_mask outside 0..6, a non-zero
 * reserved word. It also checks the bank: PA_ERR_INVALID_ARG when a render is so flat that h1 < 1 (cv2.resize raises),
 * PA_ERR_CAPACITY when one is so tall that h1 > PA_SPRITE_H1_MAX = 448 (step b's filter then has more than PA_KSIZE_MAX = 15
 * taps, and its intermediate outgrows the scratch): every render with h <= 3.5 w is taken.
 *
 * pa_sprite_bank_create: a PA_SYNTH_SPRITES bank of n (1..65535) slots of 128 x 128 whose descriptors the library writes and
 * whose pixels only pa_sprite_augment writes (zero until then), with the kernel's scratch behind them (524288 bytes for each of
 * min(n, 256) workgroups). With e NULL the bank holds the sizes alone. pa_synth_bank_destroy frees it.
 * pa_sprite_augment: params on the device (8-byte aligned), n 1..slots of out_bank, sprites a bank with pixels that is not
 * out_bank; the bank-level limits above are refused here too, on the host. PA_ERR_INVALID_ARG / PA_ERR_CAPACITY otherwise.
 * Launches on one out_bank must be stream-ordered with each other and with the pa_synth_composite calls that read it. Enqueue
 * only; nothing is read back. */
typedef struct pa_sprite_aug_params {
    int32_t src;                 /* image of the sprite bank */
    int32_t flip;
    float alpha, beta;
    int32_t blur_k;
    float hue_shift, sat_shift, val_shift;
    float noise_sigma;
    uint32_t pixel_drop_thr;
    int32_t n_holes;
    uint8_t holes[4];            /* (x, y) of up to two holes */
    int32_t channel_mask;
    int32_t new_scale;           /* 0: no shrink */
    int32_t sized_crop;          /* != 0: the maps have 128 entries (RandomSizedCrop fired), else C */
    int32_t reserved;            /* zero */
    uint8_t xmap[160], ymap[160];    /* the image's gather */
    uint8_t axmap[160], aymap[160];  /* the mask's */
    uint64_t key;
} pa_sprite_aug_params;          /* 712 bytes */
#define PA_SPRITE_DROP_THR 429496729u
#define PA_SPRITE_H1_MAX 448
#define PA_SPRITE_CANVAS_MAX 160
int pa_sprite_aug_params_check(const pa_sprite_aug_params* host, int32_t n, const pa_synth_bank* sprites);
int pa_sprite_bank_create(pa_engine* e, int32_t n, pa_synth_bank** out);
int pa_sprite_augment(pa_engine* e, const pa_synth_bank* sprites, const pa_sprite_aug_params* params_dev, int32_t n,
                      pa_synth_bank* out_bank, void* stream);
/* Slots first .. first + n - 1 of a bank of pa_sprite_bank_create as uint8[n][128][128][4] (RGBA) in host memory, for tests and
 * for looking at what a level does: a copy behind the work already enqueued on `stream`, which the call waits for.
 * PA_ERR_INVALID_ARG for a bank of another kind or without pixels, or a range outside the slots. */
int pa_sprite_bank_read(pa_engine* e, const pa_synth_bank* bank, int32_t first, int32_t n, uint8_t* out_host, void* stream);

/* Appended (the version stays 15): pa_wino_conv3x3 with the workgroup's shape as one more argument, for parity tests and
 * measurements of single layers. PA_WINO_WG_BY_BN: the launch pa_wino_conv3x3 makes (eight waves over 16 sub-blocks x 64 channels, or
 * four over 16 x 32, as `bn` says). PA_WINO_WG_2X2: four waves as two tile groups by two channel groups -- 8 sub-blocks (128 pixels)
 * x 64 channels, one workgroup per CU; it reads the `bn` = 64 filter layout and nothing else. Neither splits K: per lane the
 * arithmetic is the same in both, so the two give the same bits. PA_ERR_INVALID_ARG for another shape value, for PA_WINO_WG_2X2
 * with `bn` != 64, and for whatever pa_wino_conv3x3 refuses. Enqueue only. */
#define PA_WINO_WG_BY_BN 0
#define PA_WINO_WG_2X2 1
int pa_wino_conv3x3_shape(const float* x, const float* ug, const float* bias, const float* residual, float* out, int32_t n,
                          int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t bn, int32_t in_px_stride,
                          int32_t out_px_stride, int32_t out_pad, int32_t act, int32_t res_after, int32_t shape, void* stream);

/* Appended (the version stays 15): pa_wino_conv3x3 with the launch width `wg` (output channels per workgroup: 32 | 64) beside the
 * filter layout's `bn`, which must be 64. wg == 64 is the launch pa_wino_conv3x3 makes (pa_wino_conv3x3_splitk where `slab` and
 * `tickets` are given; both null: no scratch). wg == 32 is the one new combination: four-wave workgroups of 16 sub-blocks x 32
 * channels, two to a CU, each copying its half of the 64-channel filter images -- per lane the same instructions on the same values
 * as the eight-wave workgroup, so the same bits. It never splits K: PA_ERR_INVALID_ARG where scratch is handed in with it, for
 * `bn` != 64 (the 32-channel layout has its own launch and nothing to halve), for another `wg`, and for whatever pa_wino_conv3x3 /
 * _splitk refuse. Enqueue only. */
int pa_wino_conv3x3_wg(const float* x, const float* ug, const float* bias, const float* residual, float* out, int32_t n, int32_t height,
                       int32_t width, int32_t cin, int32_t cout, int32_t bn, int32_t in_px_stride, int32_t out_px_stride,
                       int32_t out_pad, int32_t act, int32_t res_after, int32_t wg, float* slab, size_t slab_floats, int32_t* tickets,
                       int32_t n_tickets, void* stream);

/* Appended (the version stays 15): the detector's own synthetic training images, composite_chars_onto_stage of
 * gen_synth_char_detection.py:190-262 -- one to four renders, each resized to a random width, augmented, and pasted over a WHOLE
 * stage picture -- as two more launches around pa_sprite_augment (csrc/sprite_resize.hip, csrc/scene_composite.hip, DESIGN.md
 * 5.17): pa_sprite_resize -> pa_sprite_augment -> pa_scene_composite -> pa_jpegenc_encode, and no frame on the host.
 *
 * pa_sprite_resize: output i is Image.resize((out_w, out_h)) of the h x w RGBA render params[i].src of a PA_SYNTH_SPRITES bank,
 * as the installed Pillow does it for mode RGBA with its default filter, BICUBIC:
 *   (out_w, out_h) == (w, h)   a copy (no premultiplication: the round trip below is not the identity)
 *   otherwise                  every pixel to premultiplied RGBa (c' = MULDIV255(c, a): t = c * a + 128, ((t >> 8) + t) >> 8; alpha
 *                              kept); when out_w != w the horizontal 8-bit pass, then when out_h != h the vertical one, each over
 *                              all four channels (precompute_coeffs + normalize_coeffs_8bpc: support 2 * max(in / out, 1), the
 *                              weights summed in tap order in double precision, each divided by the sum, scaled by 2^22 and
 *                              rounded half away from zero; a value is 2^21 + the sum of u8 * coefficient, >> 22, clipped to
 *                              0..255) -- a pass whose size does not change is skipped, not run with scale 1; back to RGBA (alpha
 *                              0 or 255: unchanged, else min(255, 255 * c / a), integer division)
 * Resampling the four channels as plain channels gives other bytes. detect_composite.resize_sprites_reference is the numpy twin.
 * Limits: any render of the bank (sides up to PA_SYNTH_SPRITE_MAX), out_w 1..PA_SPRITE_RESIZE_W_MAX, out_h
 * 1..PA_SPRITE_RESIZE_H_MAX (the reference draws widths 50..150 and pa_sprite_augment takes heights up to 3.5 widths). A row of
 * a pass in -> out has at most min(ceil(2 * max(in / out, 1)) * 2 + 1, in) taps -- 83 for 1024 -> 50, 1024 for 1024 -> 1 -- and
 * the kernel keeps one pass's table, out rows of that many, in LDS: at most PA_SPRITE_RESIZE_COEFS = 4 * 1024 + 3 * 560
 * coefficients (ksize <= 4 in / out + 3). PA_KSIZE_MAX = 15 of the crop stage and of pa_sprite_augment's pad step is another
 * matter and stays.
 *
 * pa_sprite_resize_bank_create: a PA_SYNTH_SPRITES bank of n (1..65535) slots of up to max_w x max_h (1..PA_SPRITE_RESIZE_W_MAX,
 * 1..PA_SPRITE_RESIZE_H_MAX; PA_ERR_INVALID_ARG and a message otherwise), each max_w * max_h * 4 bytes rounded up to 16; slot i's
 * descriptor is 1 x 1 (a transparent pixel) until a call fills it. Behind the slots: the records' device copy, and the kernel's
 * scratch (the horizontal pass's output, PA_SYNTH_SPRITE_MAX rows of max_w pixels, for each of min(n, 256) workgroups). With e
 * NULL the bank holds the sizes alone. pa_synth_bank_destroy frees it; pa_sprite_augment and pa_synth_composite read it like
 * any other sprite bank. Nothing is allocated per call.
 * pa_sprite_resize: params on the HOST, n 1..slots of out_bank, sprites a bank with pixels that is not out_bank. The call
 * writes the descriptors of slots 0..n-1: the host's copy (what pa_sprite_aug_params_check and the launches' argument checks
 * read) at once, the device's copy by the kernel itself, stream-ordered with the pixels. The records travel through a pinned
 * staging area of the bank (the call waits for the previous call's copy out of it, not for its kernel). PA_ERR_INVALID_ARG /
 * PA_ERR_CAPACITY (n beyond the slots) and a message otherwise. Calls on one out_bank must be stream-ordered with each other
 * and with the launches that read it. Enqueue only.
 * The kernel is defined for ANY parameter bytes: src is clamped into the bank, out_w to 1..max_w, out_h to 1..max_h of the
 * output bank, every source coordinate is clamped where the address is formed; the reserved word is not read.
 * pa_sprite_resize_params_check (host only, no device call) returns PA_ERR_INVALID_ARG for a src outside the bank, a size
 * below 1 or a non-zero reserved word, PA_ERR_CAPACITY for a size beyond the output bank's slots.
 * pa_sprite_resize_bank_read: slot `slot` as uint8[h][w][4] of its current host descriptor into out_host (capacity bytes), behind
 * the work enqueued on `stream`, which the call waits for; for tests. */
typedef struct pa_sprite_resize_params {
    int32_t src;                 /* image of the sprite bank */
    int32_t out_w, out_h;
    int32_t reserved;            /* zero */
} pa_sprite_resize_params;
#define PA_SPRITE_RESIZE_W_MAX 160
#define PA_SPRITE_RESIZE_H_MAX 560
#define PA_SPRITE_RESIZE_COEFS 5776
int pa_sprite_resize_params_check(const pa_sprite_resize_params* host, int32_t n, const pa_synth_bank* sprites, const pa_synth_bank* out_bank);
int pa_sprite_resize_bank_create(pa_engine* e, int32_t n, int32_t max_w, int32_t max_h, pa_synth_bank** out);
int pa_sprite_resize(pa_engine* e, const pa_synth_bank* sprites, const pa_sprite_resize_params* params_host, int32_t n,
                     pa_synth_bank* out_bank, void* stream);
int pa_sprite_resize_bank_read(pa_engine* e, const pa_synth_bank* bank, int32_t slot, uint8_t* out_host, size_t capacity, void* stream);

/* pa_scene_composite: scene i is the whole picture params[i].stage of a PA_SYNTH_STAGES bank (RGB, W x H) with n_sprites (0..4)
 * 128 x 128 RGBA slots of a pa_sprite_bank_create bank pasted over it in order, sprite k with its top-left corner at
 * (sprites[k].x, sprites[k].y) through its own alpha -- Image.paste(char, (x, y), char): per covered pixel and channel c of R, G, B,
 * t = s_c * a + d_c * (255 - a) + 128; out_c = ((t >> 8) + t) >> 8, where d is the picture with the earlier sprites already
 * in it -- clipped to the picture; x and y may be negative or beyond it. detect_composite.compose_scenes_reference is the twin.
 * Output: the scenes as packed uint8[H][W][3] RGB in `images`, scene i at the sum of the earlier scenes' sizes, each rounded up
 * to 16 bytes, and desc[i] = {offset, H, W}: the pair pa_jpegenc_encode(bgr = 0) takes as it is. Stages of different sizes may
 * share a call. A scene that does not fit images_capacity (padding included) gets height = width = 0, for which the encoder
 * writes an empty entry, and none of its bytes is written; so do the scenes behind it.
 * The kernel is defined for ANY parameter bytes: stage and slot are clamped into their banks, n_sprites to 0..4, x and y to
 * +-PA_SYNTH_PASTE_MAX, and a sprite's pixel is addressed only where both of its coordinates are 0..127; the reserved words are
 * not read. pa_scene_params_check (host only) returns PA_ERR_INVALID_ARG for anything of that kind and for a non-zero reserved
 * word (the entries from n_sprites on must be zero as well).
 * pa_scene_composite: params and desc on the device (8-byte aligned), images 16-byte aligned, n 1..65535, sprites a bank of
 * 128 x 128 slots with pixels. PA_ERR_INVALID_ARG and a message otherwise. Two launches (the layout: one small workgroup; the
 * scenes), enqueue only. */
#define PA_SCENE_SPRITES_MAX 4
typedef struct pa_scene_sprite {
    int32_t slot;                /* slot of the sprite bank */
    int32_t x, y;                /* where its top-left corner goes in the picture */
} pa_scene_sprite;
typedef struct pa_scene_params {
    int32_t stage;               /* image of the stage bank */
    int32_t n_sprites;           /* 0..4 */
    pa_scene_sprite sprites[PA_SCENE_SPRITES_MAX];
    int32_t reserved[2];         /* zero */
} pa_scene_params;               /* 64 bytes */
int pa_scene_params_check(const pa_scene_params* host, int32_t n, const pa_synth_bank* sprites, const pa_synth_bank* stages);
int pa_scene_composite(pa_engine* e, const pa_synth_bank* sprites, const pa_synth_bank* stages, const pa_scene_params* params_dev,
                       int32_t n, uint8_t* images_dev, size_t images_capacity, pa_crop_image* desc_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PLAYAID_HIP_H */

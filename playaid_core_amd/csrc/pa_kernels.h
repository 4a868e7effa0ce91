// Internal declarations shared by the HIP translation units and the C-ABI host
// code. Not part of the public ABI (include/playaid_hip.h is).
#pragma once
#include "gemm_tile.h"   // GemmTile
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "crop_math.h"  // CropPlan, AreaTabPacked (behind the HIP runtime: its device functions use __mul24)

namespace pa {

// SiLU x * sigmoid(x) of the conv epilogues (the detection network): v_exp_f32 + v_rcp_f32 (1 ulp each; the exponent's
// pre-multiply adds |x| * 6e-8 relative) instead of expf + an IEEE division -- ~6 instead of ~30 vector instructions per
// value, which for a 64-deep 1x1 convolution was as much issue time as the tile's matrix instructions.
__device__ __forceinline__ float silu_fast(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}

// ---------------------------------------------------------------------------
// implicit-GEMM engine (igemm.hip)
// ---------------------------------------------------------------------------
// out[m][n] = act( sum_{tap,kc} A(m,tap,kc) * W[n][tap*chunk + kc] + bias[n] (+ residual[m][n]) )
//
// A(m,tap,kc) is addressed in one of two ways:
//  * conv mode  (gather == nullptr): m -> (img, oy, ox); tap -> (ky, kx);
//      A = act + img*in_img_stride + (oy*stride + ky + off_y)*in_row_stride
//              + (ox*stride + kx + off_x)*in_px_stride + kc
//    Activations are NHWC with an explicit zero border, so no bounds checks.
//  * gather mode: row = gather[m*taps + tap]; A = act + row*in_px_stride + kc
//    (row < 0 -> zeros). Used for the temporal Conv1d over cached features.
struct GemmParams {
    const float* act;
    const float* wgt;       // [N][ktot], K contiguous
    const float* bias;      // [N] or nullptr
    const float* residual;  // same addressing as out, or nullptr
    float* out;
    float* slab;            // split-K partial sums [splitk][M][N]
    const int32_t* gather;
    int32_t M, N, ktot;
    int32_t taps, kw_taps, chunk;  // ktot == taps*chunk, chunk % 32 == 0
    int32_t howo, wo;              // output pixels per image, output width
    int32_t howo_shift, wo_shift;  // log2 of the above when both are powers of two, else -1 (set by the launcher)
    int32_t in_img_stride, in_row_stride, in_px_stride, stride, off_y, off_x;
    int32_t out_img_stride, out_row_stride, out_px_stride, out_pad;
    int32_t relu;           // activation of the epilogue: 0 none, 1 ReLU, 2 SiLU (x * sigmoid(x))
    int32_t res_after;      // 1: the residual is added AFTER the activation (YOLOv5's Bottleneck), 0: before (ResNet)
    // optional second im2col source appended to K (k2_steps * 32 values, 1x1 taps): act2 addressed as
    //   act2 + img*in2_img_stride + (oy*stride2 + off2)*in2_row_stride + (ox*stride2 + off2)*in2_px_stride + kc
    const float* act2;
    int32_t k2_steps, in2_img_stride, in2_row_stride, in2_px_stride, stride2, off2;
    int32_t splitk, ksteps_per_split;
    int32_t defer_reduce;   // 1: leave the split-K slabs to the consumer (the head MLP sums them itself); the
                            //    launcher writes the split count it actually used to *splitk_used
    int32_t* splitk_used;
    int32_t skip_w;         // 1: k % 4 == 3 always meets a zero weight (stem channel pad): those MFMAs are skipped
    int32_t tiles_m, tiles_n;
    // persistent GEMMs (pgemm_common.h), filled by persistent_plan and the launchers: workgroups per XCD, output rows per image, ceil(2^32 / howo) and
    // ceil(2^32 / wo) for the scalar divisions, how often 31 consecutive pixels can wrap a row / that many rows an image
    // (beside tiles_m / tiles_n: the kernel's first scalar loads fetch them together)
    int32_t pg_per, pg_ho, pg_nwx, pg_nwy;
    uint32_t pg_magic_howo, pg_magic_wo;
    // persistent GEMM only: a second, nearest-neighbour x2 up-sampled copy of the output (first channel of the slice's padded pixel
    // (0, 0) of image 0; strides in floats of the UP-SAMPLED buffer; nullptr = none)
    float* up_out;
    int32_t up_img_stride, up_row_stride, up_px_stride, up_pad;
    // patch-resident 3x3 kernel (patchconv.hip), filled by its launcher: pixels per LDS patch buffer,
    // input row pitch and image size in pixels, tile -> first patch pixel, pixels in the whole buffer
    int32_t patch_slots, patch_pitch, img_px, tiles_per_img, p0_img, p0_row, total_px;
    int32_t swz_a, magic_pitch, magic_img, img_px_patch;  // chunk-swizzle key of a patch pixel (see patchconv.hip)
    int32_t xcd_m, xcd_n;  // the 8 XCDs as an xcd_m x xcd_n grid over (pixel tiles, channel tiles); 0 = contiguous runs of tiles
    // blocked form of the patch-resident kernel (maps whose width is not 32 / 16 / 8 / 4: the detection network's): output
    // pixel m = (block * blk_rows + r) * blk_cols + c, blocks row-major over each image; a tile's patch = the
    // (blk_rows + 2) x (blk_cols + 2) input rectangles of its blocks back to back. Set by launch_conv3x3_patch_blocked.
    int32_t blk_rows, blk_cols, blk_shift_c, blk_shift_px, blk_per_row, blk_per_img, n_blocks, src_pitch;
    // igemm_bf16.hip, stride-2 3x3 openers: a second 1x1 product off the SAME im2col rows -- the centre tap's rows are the
    // pixels the block's 1x1/2 downsample branch reads -- wgt2 = [N][chunk] bf16, out2 addressed like out (no bias, no
    // activation); nullptr = off. The same pair on the exact persistent GEMM (pigemm.hip's pgemm_branch_kernel): wgt2 fp32
    const float* wgt2;
    float* out2;
    unsigned long long* clk;  // ablation builds only: in-kernel clock stamps
    // split-K form of the one-slice bf16 GEMM (bgemm.hip, splitk > 1): 4 zeroed tickets per output tile, left zeroed behind a launch
    int32_t* tickets;
    // grouped form of the exact persistent GEMM (pigemm.hip's pgemm_group_kernel, set by launch_pgemm_grouped): `grp_tiles` consecutive
    // pixel tiles share one [N][ktot] weight image, the next ones read the image grp_wgt_bytes further on; grp_magic = ceil(2^32 / grp_tiles)
    int32_t grp_tiles, grp_wgt_bytes;
    uint32_t grp_magic;
};

hipError_t launch_igemm(const GemmParams& p, GemmTile tile, hipStream_t s);
// persistent form of the same engine for short tiles (pigemm.hip): conv mode, no residual / second source / split-K;
// bm = 128 | 64, 64 output channels per tile; results equal to launch_igemm up to where the bias enters the sum
// p.wgt2 / p.out2 set: the opener form (3x3, stride 2, whole-pixel taps, ReLU or none, 64 x 64 tiles), hipErrorInvalidValue for anything else
hipError_t launch_pgemm(const GemmParams& p, int bm, hipStream_t s);
// `groups` independent products out[g] = a[g] . w[g]^T in ONE launch of the same kernel (no bias, no activation, no K split): a =
// [groups][rows][K], w = [groups][N][K], out = [groups][rows][N], all fp32, 16-byte aligned; rows a multiple of 64, K of 32, N of 64.
// A pixel tile's first row gives its group, and the group moves the weight base by one scalar offset (rows are whole tiles, so the
// activation and output rows of all groups are one contiguous matrix). tile: 1 = 64 x 64, 2 = 128 x 64 (rows % 128 == 0), 3 = 128 x 32
// (the same), 0 = the default. A row's bits depend on neither the tile nor the other rows.
hipError_t launch_pgemm_grouped(const float* a, const float* w, float* out, int groups, int rows, int K, int N, int tile, hipStream_t s);
// "emulated fp32" form of the persistent GEMM (psgemm.hip): fp32 activations, the weights as three bf16 slices in the kernel's
// stage-image layout (psgemm_pack_weights, psgemm_weight_elems of them), six bf16 matrix instructions per fp32 product, fp32
// accumulate. Conv mode; bias, ReLU / SiLU; out_floats = floats from p.out to the end of its buffer (the store descriptor's bounds).
int psgemm_pick_bn(int N, int residual);          // channels per workgroup (128 | 64 | 32; with a residual 64 at most): part of the weight layout
size_t psgemm_weight_elems(int N, int ktot, int residual);
void psgemm_pack_weights(const float* w, int N, int ktot, int residual, unsigned short* out);
hipError_t launch_psgemm(const GemmParams& p, const unsigned short* wsp, size_t out_floats, size_t up_floats, hipStream_t s);   // (up_floats: the same for p.up_out, 0 without one)
// one-slice bf16 form of it (bgemm.hip, the detection network's PA_DTYPE_BF16 convolutions): bf16 activations, residual and up-sampled
// copy behind the float* fields (strides and counts in elements), the weights as ONE round-to-nearest-even bf16 plane in psgemm's plane
// layout (bgemm_pack_weights), one matrix instruction per product, fp32 accumulate, one rounding on the store; out_f32: fp32 output
// (the Detect heads; no residual, no up-sampling). out_elems / up_elems: elements from p.out / p.up_out to the end of the buffer.
size_t bgemm_weight_elems(int N, int ktot, int residual);
void bgemm_pack_weights(const float* w, int N, int ktot, int residual, unsigned short* out);
hipError_t launch_bgemm(const GemmParams& p, const unsigned short* wsp, size_t out_elems, size_t up_elems, bool out_f32, hipStream_t s);
// Its split-K form: p.splitk = S > 1 runs one workgroup per (output tile, k-slice) -- bf16 output, no up-sampled copy; p.slab holds
// BGEMM_SLAB_ITEMS workgroups' fp32 partial tiles (128 x BN each), p.tickets BGEMM_TICKETS zeroed ints. bgemm_pick_split: the S the
// split rule gives the shape of p (conv mode, as launch_bgemm takes it): 1 unless its unsplit grid is below BGEMM_SPLIT_MAX_GRID
// workgroups (a quarter of the CUs) and it has at least BGEMM_SPLIT_MIN_KSTEPS k-steps (of 32), else the largest S in {8, 4, 2} with
// tiles * S <= BGEMM_SLAB_ITEMS and at least 4 k-steps per slice; force > 1 takes S = force instead (on every row whose unsplit grid
// is below half the CUs, short K included, within the same two limits, else 1), force 0 or 1 gives 1 (no split), force < 0 is the
// rule.
constexpr int BGEMM_SLAB_ITEMS = 256, BGEMM_TICKETS = 4 * 128, BGEMM_SPLIT_MAX_GRID = 64, BGEMM_SPLIT_MIN_KSTEPS = 72;
int bgemm_pick_split(const GemmParams& p, int force);
// bf16 activations / weights (uint16_t storage behind the float* fields, every count in elements),
// f32 accumulate on v_mfma_f32_32x32x16_bf16; conv mode only (igemm_bf16.hip)
hipError_t launch_igemm_bf16(const GemmParams& p, GemmTile tile, hipStream_t s);

// stride-1 3x3 convolution on bf16 with the activation patch resident in LDS (patchconv_bf16.hip); no second source
hipError_t launch_conv3x3_bf16_patch(const GemmParams& p, hipStream_t s);

// Persistent direct 7x7/2 stem (stem.hip): x = [crops][134][134][4] fp32 (3-pixel zero border,
// channel 3 = 0), wgt = [64][7 ky][8 px][4 ch] (the igemm stem layout), out = [crops][66][66][64].
struct StemParams {
    const float* x;
    const float* wgt;
    const float* bias;
    float* out;     // fp32, or bf16 (uint16_t storage) when out_bf16 != 0
    int32_t tiles;  // crops * 32 (one tile = two output rows of one crop)
    int32_t out_bf16;
    unsigned long long* clk;  // stamp builds only
};
hipError_t launch_stem7x7(const StemParams& p, hipStream_t s);
// Stem + BatchNorm + ReLU + 3x3/2 max-pool in one persistent kernel (stem_pool.hip): x as above (fp32) or bf16
// [crops][134][134][4]; wgt fp32 or bf16 [64][224]; out = pooled map [crops][34][34][64], fp32 or bf16. in_bf16 == 2: x holds
// the pixel integers 0 .. 255 as bf16, wgt three bf16 slices [3][64][224] of the fp32 weights, out fp32 (exact products).
struct StemPoolParams {
    const void* x;
    const void* wgt;
    const float* bias;
    void* out;
    int32_t crops;
    int32_t run;       // row pairs per run (set by the launcher)
    int32_t in_bf16;   // 1: x and wgt are bf16: multiply on the bf16 matrix cores; 2: integer pixels and three weight slices
    int32_t out_bf16;
};
hipError_t launch_stem_pool(const StemPoolParams& p, hipStream_t s);
// The same stem + max-pool for a square input of any size in_hw (in_hw % 32 == 0, 64 .. 512; stem_pool_any.hip): x fp32
// [crops][in_hw + 6][in_hw + 6][4], wgt fp32 [64][224], out fp32 [crops][in_hw / 4 + 2]^2 x 64 (interior written). fp32 only.
struct StemPoolAnyParams {
    const float* x;
    const float* wgt;
    const float* bias;
    float* out;
    int32_t crops;
    int32_t in_hw;
    int32_t run;       // row pairs per run (set by the launcher)
};
hipError_t launch_stem_pool_any(const StemPoolAnyParams& p, hipStream_t s);
// ordered split-K reduce of the slabs with the fused epilogue (igemm.hip); out_bf16: bf16 residual and output (igemm_bf16.hip)
hipError_t launch_splitk_reduce(const GemmParams& p, hipStream_t s, bool out_bf16 = false);
// stride-1 3x3 convolution with the input patch resident in LDS across the nine taps (patchconv.hip); bm = 128 | 64
hipError_t launch_conv3x3_patch(const GemmParams& p, int bm, hipStream_t s);
// the same kernel over rectangular blocks of output pixels (8 x 16, 8 x 8 or 4 x 4, whichever divides the map): any map whose
// sides are multiples of 4; in_pad == 1; epilogue: bias, ReLU / SiLU, residual before or after the activation
hipError_t launch_conv3x3_patch_blocked(const GemmParams& p, hipStream_t s);

// stride-1 3x3 convolution as Winograd F(2x2, 3x3) on the fp32 matrix cores (wino.hip): zero-bordered NHWC input (border 1),
// any map whose sides are multiples of 4, cin % 8 == 0, cout % 32 == 0; epilogue: bias, ReLU / SiLU, residual before or
// after the activation. The input and output may be channel slices of wider buffers (px strides >= cin / cout).
struct WinoParams {
    const float* act;       // first channel of padded pixel (0, 0) of image 0
    const float* wgt;       // wino_transform_weights' image of the filters
    const float* bias;      // [cout] or nullptr
    const float* residual;  // addressed like out, or nullptr
    float* out;             // first channel of padded pixel (0, 0) of image 0
    int32_t n_img, height, width, cin, cout;
    int32_t bn;             // output channels per workgroup the filters were laid out for (wino_pick_bn: 64 | 32)
    int32_t in_px_stride, in_row_stride, in_img_stride;      // floats
    int32_t out_px_stride, out_row_stride, out_img_stride, out_pad;
    int32_t relu, res_after;  // as GemmParams
    int32_t n_sb, sb_per_row, sb_per_img, tiles_n;  // set by the launcher
    unsigned long long* clk;  // stamp launches only (PA_WINO_ABL=8)
    // split K (optional; the launcher turns it on for layers whose tiles do not fill the chip): scratch for the partial output
    // tiles -- slab_floats floats -- and one ticket per tile, tickets_cap of them, ZERO before the first launch (the kernel
    // leaves them zero); ksplit is set by the launcher
    float* slab;
    size_t slab_floats;
    int32_t* tickets;
    int32_t tickets_cap, ksplit;
    int32_t tiles_m, xcd_gm, xcd_gn;   // set by the launcher: pixel tiles; the 8 XCDs as a gm x gn grid over (pixel, channel) tiles, 0 = launch order
    int32_t tg2;   // 0: the workgroup bn implies; 1: four waves as 2 tile groups x 2 channel groups (bn == 64), 8 sub-blocks each, never split
    int32_t wg;    // output channels per workgroup of THIS launch, beside the layout's bn: 0 = the layout's own; named only with bn == 64: 64 = its own
                   // again, 32 = four waves of 16 sub-blocks x 32 channels on the 64-channel filter images, two to a CU, never split (no scratch)
};
size_t wino_weight_floats(int cin, int cout);
// output channels per workgroup = per stage image of the filter layout (64 | 32); cin_split > 0: the caller launches with split-K
// scratch (WinoParams::slab, tickets) and the layer has that many input channels
int wino_pick_bn(int cout, long long n_sb, int cin_split = 0);
// w [cout][ky][kx][cin] (host) -> ug [wino_weight_floats] (host)
void wino_transform_weights(const float* w, int cin, int cout, int bn, float* ug);
hipError_t launch_wino3x3(const WinoParams& p, hipStream_t s);

// stride-1 3x3 convolution on a 4 x 4 map as Winograd F(4x4, 3x3) taken apart (wino4.hip): input transform, 36 grouped GEMMs on
// pigemm.hip, output transform + epilogue -- three launches on the stream. Zero-bordered NHWC input (border 1), cin and cout
// multiples of 64; epilogue as WinoParams. v, m: scratch of 36 * wino4_rows(n_img) * cin and ... * cout floats.
struct Wino4Params {
    const float* act;       // first channel of padded pixel (0, 0) of image 0
    const float* wgt;       // wino4_transform_weights' image of the filters: U[36][cout][cin]
    const float* bias;      // [cout] or nullptr
    const float* residual;  // addressed like out, or nullptr
    float* out;             // first channel of padded pixel (0, 0) of image 0
    float* v;               // scratch: the transformed input V[36][rows][cin]
    float* m;               // scratch: the products M[36][rows][cout]
    int32_t n_img, cin, cout;
    int32_t in_px_stride, in_row_stride, in_img_stride;      // floats
    int32_t out_px_stride, out_row_stride, out_img_stride, out_pad;
    int32_t relu, res_after;  // as GemmParams
    int32_t tile;             // the GEMM's tile (launch_pgemm_grouped), 0 = the default
    int32_t rows;             // set by the launcher: wino4_rows(n_img)
};
size_t wino4_weight_floats(int cin, int cout);
int wino4_rows(int n_img);   // crops padded to the GEMM's row tile
// w [cout][ky][kx][cin] (host) -> u [wino4_weight_floats] (host)
void wino4_transform_weights(const float* w, int cin, int cout, float* u);
hipError_t launch_wino4_conv3x3(const Wino4Params& p, hipStream_t s);

// ---------------------------------------------------------------------------
// crop preprocessing (preprocess.hip)
// ---------------------------------------------------------------------------
// CropPlan, AreaTabPacked, PA_KSIZE_MAX and PA_CROP_BLANK: crop_math.h (included above; the host compiler reads it too)
// Stage buffers of crop_fused_kernel; + 2176 B of INTER_AREA tables = 80000 B: two 512-thread
// workgroups per CU (16 waves). Measured ladder of this choice (64 x 1080p step, kernel alone):
// 256 threads / 50944 B (3 per CU) 0.189 ms -> 512 threads / 46592 B 0.169 -> 512 threads / 77824 B
// 0.144: eight waves per band halve a workgroup's lifetime, and the larger budget lets most crops use
// 8-row sub-bands (the 7-tap vertical support makes 4-row sub-bands recompute 1.7x of the horizontal
// pass, 8-row ones 1.35x).
#define PA_FUSED_LDS_BYTES 77824

// The horizontal matrix form's operand (crop_hop_kernel -> crop_fused_kernel): per crop PA_HOP_BLOCKS_MAX blocks of 10
// output pixels (30 byte columns of the 32 the instruction has), PA_HOP_BLOCK_BYTES each: six 1 KB fragments -- digit
// plane 2, 1, 0 x the two 32-byte halves of the block's 64-byte input window, lane l's 16 bytes at 16 l -- then the 32
// columns' constants 2^21 + 128 sum(k), then the window's first byte inside the staged row (a multiple of 4).
#define PA_HOP_BLOCKS_MAX 48
#define PA_HOP_PIXELS 10
#define PA_HOP_WINDOW 64
#define PA_HOP_BLOCK_BYTES (6 * 1024 + 32 * 4 + 16)
#define PA_CROP_MFMA_H_DEFAULT 1  // PA_CROP_MFMA_H when the environment does not set it

struct CropWindow {  // == pa_crop_window of the public header
    int64_t offset;      // first byte of the crop's slice inside the window buffer
    int32_t pitch;       // bytes per slice row in the window buffer (row_bytes rounded up to 16)
    int32_t rows;        // slice rows
    int64_t src_offset;  // first byte of the slice inside the host frame buffer
    int32_t src_pitch;   // bytes per frame row
    int32_t row_bytes;   // slice width * 3
};
hipError_t launch_slice_upload(const uint8_t* frames_host, long long frames_bytes, const CropWindow* desc, uint8_t* windows, int ncrops,
                               hipStream_t s);

struct PreprocParams {
    const uint8_t* frames;  // [n_src][H][W][3]; with `windows`: the packed window buffer
    const CropWindow* windows;  // [ncrops] or nullptr: every crop's slice was uploaded on its own
    const double* boxes;    // [ncrops][4]
    const int32_t* src_frame;  // [ncrops] frame each crop is cut from, or nullptr = crop / fighters
    int32_t n_src;             // frames in the buffer (bound of src_frame)
    int32_t n_frames, height, width, fighters, padding, swap_rb;
    CropPlan* plans;        // [ncrops]
    int32_t* coef;          // [ncrops][2][maxdim][1 + 1 + PA_KSIZE_MAX]: xmin, count, kk[]
    int32_t coef_dim;       // maxdim (entries per axis per crop)
    const int32_t* coef_cache;  // tables of the pairs (2 * (d / 2) + 2 * coef_cache_pad -> d), d = 1 .. coef_cache_dmax, table d at row d * (d - 1) / 2
    int32_t coef_cache_pad, coef_cache_dmax;
    AreaTabPacked* area_tabs;   // [ncrops][2][128]: INTER_AREA tables of the 128 destination columns, then rows
    uint8_t* t1;            // [ncrops][t_stride] horizontally resampled slice
    uint8_t* t2;            // [ncrops][t_stride] fully resampled slice
    size_t t_stride;
    uint8_t* crops_u8;      // [ncrops][128][128][3] or nullptr
    float* crops_f32;       // [ncrops][134][134][4] zero-bordered, or nullptr
    int32_t crops_f32_is_bf16;  // 1: the model input is stored as bf16 [ncrops][134][134][4] instead (bf16 conv path); 2: as the pixel integers in bf16 (integer stem)
    int32_t* status;        // [ncrops] or nullptr
    int32_t* fallback_count;  // [1] number of crops routed to the multi-kernel fallback (zeroed per call)
    int32_t* fallback_list;   // [ncrops] their indices
    int32_t fused_lds;      // LDS budget of the fused kernel (set by the launcher; 0 forces the fallback)
    int32_t ablate;         // timing experiments: skip stages of the fused kernel (results wrong when != 0)
    int32_t crop_mfma;      // PA_CROP_MFMA (default 1; set by the launcher): 0 keeps both bicubic passes on the vector ALU
    int32_t crop_mfma_h;    // PA_CROP_MFMA_H (set by the launcher): 0 keeps the horizontal pass and today's staging; 1; 2 (CropPlan::mfma_h)
    int32_t crop_xcd;       // PA_CROP_XCD (default 1; set by the launcher): a crop's 16 workgroups run on one XCD
    uint8_t* hop;           // [ncrops][PA_HOP_BLOCKS_MAX][PA_HOP_BLOCK_BYTES] or nullptr (no horizontal matrix form)
    uint8_t* dbg;           // debug builds only (PA_DEBUG_DUMP)
    int32_t dbg_crop, dbg_row;
};

hipError_t launch_preprocess(const PreprocParams& p, hipStream_t s);
// square crops of out_size x out_size (PA_CROP_SIZE_MIN .. PA_CROP_SIZE_MAX) into p.crops_u8 [ncrops][out_size][out_size][3] (crop_sized.hip):
// the multi-pass form on p's plans / coef / t1 / t2; no window ingest, no model input
hipError_t launch_crop_sized(const PreprocParams& p, int out_size, hipStream_t s);
// fills the engine's coefficient cache for one padding value (once per engine, or when the padding changes)
size_t coef_cache_ints(int dmax);
hipError_t launch_build_coef_cache(int32_t* cache, int padding, int dmax, hipStream_t s);

// crop images of any size -> runner inputs (ai_runner.py:446-459), see runner_input_kernel
struct CropImageDesc {  // == pa_crop_image of the public header
    int64_t offset;     // byte offset of the image inside `images`
    int32_t height, width;
};
struct RunnerInParams {
    const uint8_t* images;      // concatenated uint8 [h][w][3] images
    long long images_bytes;
    const CropImageDesc* desc;  // [n] (device)
    int32_t n, swap_rb, max_h, max_w;
    uint8_t* t1;                // scratch, t_stride bytes per image each
    uint8_t* t2;
    size_t t_stride;
    uint8_t* inputs_u8;         // [n][128][128][3] or nullptr
    float* inputs_f32;          // [n][134][134][4] zero-bordered model input (fp32, or bf16 storage) or nullptr
    int32_t inputs_f32_is_bf16;  // 0 / 1 / 2 as PreprocParams::crops_f32_is_bf16
    int32_t* status;            // [n] PA_CROP_* or nullptr
};
hipError_t launch_runner_inputs(const RunnerInParams& q, hipStream_t s);

// baseline-JPEG write + read of the 128 x 128 crops, in place (jpeg.hip)
struct JpegParams {
    uint8_t* crops_u8;   // [ncrops][128][128][3]
    const int32_t* qtab; // [2][64] quantisation tables (luminance, chrominance) in natural order, device
    void* x0;            // model input [ncrops][134][134][4] (fp32 or bf16) rewritten from the new pixels, or nullptr
    int32_t x0_bf16;     // 0 / 1 / 2 as PreprocParams::crops_f32_is_bf16
    int32_t bgr;         // memory order of the crops: 1 = B, G, R (cv2), 0 = R, G, B
};
hipError_t launch_jpeg_roundtrip(const JpegParams& p, int ncrops, hipStream_t s);

// label repair on the detection table (detect.hip::clean_labels_kernel)
struct CleanParams {
    const float* dets;      // [n_labels][max_det][6] label rows, label-file order
    const int32_t* counts;  // [n_labels]
    int32_t n_labels, max_det, n_decoded, fighters;
    int32_t class_ids[4];
    double* lab;            // [n_labels][F][6] repaired label row of each fighter (cls < 0: none)
    int32_t* pixel_frame;   // [n_labels][F]
    double* pixel_box;      // [n_labels][F][4]
    int32_t* crop_kind;     // [n_labels][F]
    float* crop_row;        // [n_labels][F][6]
    int32_t* info;          // [4]: max_frames, error code, error frame, duplicates resolved
    double* g6v;            // scratch [n_labels][max_det][6]: every row value through the label file's '%g' (filled by the launcher's first kernel)
};
hipError_t launch_clean_labels(const CleanParams& p, hipStream_t s);
struct CropImageDesc;
// what the crop hand-off needs from the repaired table, and the clip's crop-image descriptors (detect.hip; pa_detector_plan*)
hipError_t launch_detector_plan(const int32_t* pixel_frame, const double* pixel_box, const int32_t* crop_kind, const int32_t* info4, int n_labels, int F,
                                int32_t* det_index, int32_t* src_own, int32_t* rep_entry, double* rep_boxes, int32_t* rep_src, int32_t* words5,
                                hipStream_t s);
hipError_t launch_detector_desc(CropImageDesc* desc, const int32_t* crop_kind, int n_entries, int F, int step_frames, long long region,
                                const int32_t* rep_entry, int n_rep, long long rep_base, hipStream_t s);

// YOLOv5 save_one_box crops + their 4:4:4 JPEG write / read (savebox.hip)
struct SaveBoxRect { int32_t x1, y1, w, h; };
struct SaveBoxParams {
    const uint8_t* frames;      // [n][height][width][3] BGR
    int32_t height, width, fighters, n_entries;  // n_entries = frames * fighters
    const float* dets;          // [n][max_det][6] label rows (cls cx cy w h conf, normalised), label-file order
    const int32_t* counts;      // [n]
    int32_t max_det;
    const int32_t* det_index;   // [n_entries] detection of each (frame, fighter), -1 = none; nullptr = first of the class
    const int32_t* src_frame;   // [n_entries] frame (of n_src) the pixels are cut from; nullptr = the entry's own frame
    int32_t n_src;
    int32_t class_ids[4];
    float gain, pad;
    uint8_t* images;            // packed output
    unsigned long long capacity;
    CropImageDesc* desc;        // [n_entries]
    SaveBoxRect* rects;         // [n_entries] scratch
    int32_t* overflow;          // device counter: entries that did not fit `capacity`
    int32_t quality;            // 0 = no JPEG write / read
    int32_t qtab[128];          // quantisation tables (luminance, chrominance), natural order
};
hipError_t launch_save_one_box(const SaveBoxParams& p, hipStream_t s);

// crop_img + imutils.resize(width) of up to four pixel rectangles per frame (the damage HUD crops), see rect_resize_kernel
struct RectResizeParams {
    const uint8_t* frames;       // [n][height][width][3]
    int32_t height, width;
    int32_t n_rects;
    int32_t x1[4], y1[4], x2[4], y2[4];  // numpy slice image[y1:y2, x1:x2]
    int32_t out_w, out_h[4];     // destination width, int(h * (out_w / float(w))) per rectangle
    int32_t out_h_cap;           // rows per rectangle in `out`
    uint8_t* out;                // [n][n_rects][out_h_cap][out_w][3]
};
hipError_t launch_rect_resize(const RectResizeParams& q, int n_frames, hipStream_t s);
// per-device one-time setup of the crop stage (dynamic-LDS attribute); call with the device current
hipError_t preprocess_init_device();
// log rows [n][9] (pos_x,pos_y,cam xyz,target xyz,fov deg) -> normalised boxes [n][4]
hipError_t launch_project_boxes(const double* log, double* boxes, int32_t n, hipStream_t s);

// ---------------------------------------------------------------------------
// detection post-processing (detect.hip): head rows -> class filter, confidence, NMS, max_det, image-space boxes
// ---------------------------------------------------------------------------
struct DetectParams {
    const float* pred;   // [n_frames][rows][5 + nc]: cx cy w h (network-input pixels), objectness, class scores
    int32_t n_frames, rows, nc, max_det;
    float conf_thres, iou_thres;
    uint32_t class_mask;
    uint32_t class_words[3];   // launch_detect_nms_classes: bit c % 32 of word c / 32 = class c allowed (nc <= DETECT_MAX_CLASSES)
    float pad_x, pad_y, gain;  // letterbox of the network input inside the image (scale_boxes)
    float img_w, img_h;
    float* dets;         // [n_frames][max_det][6]: cls cx cy w h conf, label-file order (lowest confidence first)
    int32_t* counts;     // [n_frames]
};
hipError_t launch_detect_nms(const DetectParams& q, hipStream_t s);
constexpr int DETECT_MAX_CLASSES = 80;
hipError_t launch_detect_nms_classes(const DetectParams& q, hipStream_t s);

// ---------------------------------------------------------------------------
// small kernels (misc.hip)
// ---------------------------------------------------------------------------
// x[n][3][128][128] f32 -> zero-bordered [n][134][134][4]
// small dense layer on the vector units (side models: LSTM / transformer heads): C[m*ldc + n] = act(X[m*ld + :K] . W[n*K + :K] + bias[n])
hipError_t launch_linear_f32(const float* X, int ld, const float* W, const float* bias, float* C, int ldc, int M, int N, int K, int relu,
                             hipStream_t s);
hipError_t launch_spin(int32_t microseconds, hipStream_t s);
hipError_t launch_gate(const int* flag, int32_t max_microseconds, hipStream_t s);  // one thread busy for that long (stream-concurrency probe)
hipError_t launch_nchw_to_padded(const float* x, float* out, int32_t n, int32_t out_bf16, hipStream_t s);
// x[n][3][hw][hw] f32 -> zero-bordered fp32 [n][hw + 6][hw + 6][4] (the input of a kind-3 stem row; stem_pool_any.hip)
hipError_t launch_nchw_to_padded_sized(const float* x, float* out, int32_t n, int32_t hw, hipStream_t s);
// 3x3/2 max pool, padded [n][66][66][64] -> padded [n][34][34][64]
hipError_t launch_maxpool(const float* in, float* out, int32_t n, hipStream_t s);
// global average pool, padded [n][6][6][512] -> [n][512]
hipError_t launch_avgpool(const float* in, float* out, int32_t n, hipStream_t s);
hipError_t launch_maxpool_bf16(const void* in, void* out, int32_t n, hipStream_t s);  // bf16 storage
hipError_t launch_avgpool_bf16(const void* in, float* out, int32_t n, hipStream_t s);  // bf16 in, fp32 out
// window gather table: rows into the feature cache, see head_gather_kernel
hipError_t launch_window_gather(int32_t* gather, int32_t frame_num_lo, int32_t count, int32_t fighters,
                                int32_t seq, int32_t delta, int32_t max_frames, int32_t min_frame, int32_t sub_frames, hipStream_t s);
hipError_t launch_identity_gather(int32_t* gather, int32_t n, hipStream_t s);
hipError_t launch_scatter_rows(const float* feats, const int32_t* st, const int32_t* ids, float* cache, int32_t* cache_st,
                               int32_t n, int32_t fighters, int32_t clip_frames, int32_t* bad_ids, hipStream_t s);

struct HeadParams {
    const float* h1;      // [nwin][512] post-ReLU Conv1d output, or nullptr when the slabs below are given
    const float* slab;    // split-K partial sums of the Conv1d [splitk][nwin][512] (ordered sum + bias + ReLU done here)
    const float* b1;      // Conv1d bias [512]
    int32_t splitk;
    const float* w2;      // [128][512]
    const float* b2;      // [128]
    const float* w3;      // [A][128]
    const float* b3;      // [A]
    float* logp;          // [nwin][A] or nullptr
    void* records;        // pa_record[nwin] or nullptr
    const int32_t* crop_status;  // per feature row or nullptr
    const int32_t* gather;       // [nwin][seq] (middle slot gives the window's own crop)
    int32_t nwin, num_actions, fighters, seq;
    int32_t class_ids[4];
};
hipError_t launch_head_mlp(const HeadParams& p, hipStream_t s);

// metrics.hip: scores n rows of log-probabilities logp[n][ld] (A columns read) against labels[i * label_stride] and adds the
// result to running device state -- counts {rows, correct, ignored, bad_labels}, sums {nll_sum, conf_sum} (double), confusion
// [A][A] (row = label, column = prediction). slab: 2 * EVAL_SLAB_PARTS doubles of scratch (one partial pair per workgroup).
constexpr int EVAL_SLAB_PARTS = 1024;
hipError_t launch_eval_rows(const float* logp, int ld, int n, int A, const int32_t* labels, int label_stride, unsigned long long* counts,
                            double* sums, unsigned long long* confusion, double* slab, hipStream_t s);

// annotate.hip: copies n BGR frames [H][W][3] into [H + pad_bottom][pad_left + W + pad_right][3] (zero padding) and paints each
// frame's draw list on the way (pa_annotate_frames). items: pa_annot_item[n][PA_ANNOT_MAX_ITEMS] (device), counts int32[n],
// text: atlas ROW indices (character code - first_char), atlas uint8[n_chars][n_chars + 1][cell_h][cell_w]. Everything the
// kernel indexes with was range-checked by the caller.
struct AnnotParams {
    const unsigned char* in;
    unsigned char* out;
    const void* items;
    const int* counts;
    const unsigned char* text;
    const unsigned char* atlas;
    int n, H, W, pad_left, pad_right, pad_bottom;
    int cell_w, cell_h, n_chars;
};
hipError_t launch_annotate(const AnnotParams& p, hipStream_t s);

// head_train.hip: one training step of the temporal head (pa_head_train_step). The six tensors are always in blob order --
// 0 cnn1d.0.weight, 1 cnn1d.0.bias, 2 classifier.0.weight, 3 classifier.0.bias, 4 classifier.2.weight, 5 classifier.2.bias --
// and in the layouts the inference kernels read: [512][S][1024], [512], k-major [512][128], [128], k-major [128][64], [A].
// AdamScalars is shared with lstm_train.hip (pa_lstm_train_step, whose kernels and handle are that file's own); adam_apply
// and the host side of the scalars are in adam.h.
struct AdamScalars {
    double one_minus_b1, b2, one_minus_b2;   // the moments are formed in double (adam_apply)
    float step_size, bc2_sqrt, eps;          // lr / (1 - beta1^k), sqrt(1 - beta2^k): double on the host, rounded once
};
struct HeadTensors {
    const float* p[6];
};
struct HeadTrainParams {
    const float* feats;      // [n_rows][1024]
    const int32_t* gather;   // [B][S] rows of feats (clamped into [0, n_rows) by every kernel)
    const int32_t* labels;   // [B], -100 = ignore
    int32_t n_rows, B, S, A, apply;
    float* w[6];             // the engine's weights, updated in place when apply
    float* m[6];
    float* v[6];
    // the trainer's scratch: h1 [B][512], h2 [B][128], dz3 [B][64], dz2 [B][128], dz1 [B][512], loss_b [B], hit_b [B],
    // gs = the five small gradients (65536 + 8192 + 512 + 128 + 64 floats), stats = pa_train_stats
    float *h1, *h2, *dz3, *dz2, *dz1, *loss_b, *gs, *stats;
    int32_t* hit_b;
    float* stats_out;        // caller's pa_train_stats or nullptr
    float* grads_out;        // apply == 0: the six gradients in PyTorch layouts, concatenated
};
size_t head_tensor_floats(int S, int A);
hipError_t launch_head_train_step(const HeadTrainParams& p, const AdamScalars& ak, hipStream_t s);
hipError_t launch_head_export(const HeadTensors& src, int S, int A, float* out, hipStream_t s);

// ---------------------------------------------------------------------------
// augmentation of 128 x 128 crops (augment.hip; pa_augment_crops of include/playaid_hip.h)
// ---------------------------------------------------------------------------
// the constant tables one launch copies into LDS: built once on the host in fp64 (augment_tables_host), held by the engine
struct AugmentTables {
    float q[1028];        // 1025 normal quantiles (pa_augment_quantiles), padded to 16 bytes
    int32_t sdiv[256];    // OpenCV's RGB -> HSV: round((255 << 12) / v)
    int32_t hdiv[256];    // ... round((180 << 12) / (6 diff))
    float unit[256];      // (float)k / 255.f
};
void augment_tables_host(AugmentTables* t);
// params: device, pa_augment_params[n]; out_format 0 = uint8 [n][128][128][3], 1 = float32 [n][3][128][128]
hipError_t launch_augment(const uint8_t* src, int n_src, const void* params, int n, int out_format, void* out,
                          const AugmentTables* tabs_dev, hipStream_t s);

// ---------------------------------------------------------------------------
// synthetic training frames: a sprite resampled and pasted over a stage crop (synth_composite.hip; pa_synth_composite)
// ---------------------------------------------------------------------------
struct SynthDesc;   // synth_math.h
struct SynthArgs {
    const uint8_t* sprite_px;        // the sprite bank's first pixel (RGBA images, each 16-byte aligned)
    const SynthDesc* sprite_desc;
    int n_sprites;
    const uint8_t* stage_px;         // the stage bank's (RGB)
    const SynthDesc* stage_desc;
    int n_stages;
    const pa_synth_params* params;   // device, [n]
    int n, dim, out_format;
    void* out;                       // PA_SYNTH_U8: uint8 [n][dim][dim][3]; PA_SYNTH_MODEL: float32 [n][3][128][128]
    const float* unit;               // AugmentTables::unit on the device: (float)k / 255.f
};
hipError_t launch_synth_composite(const SynthArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// augmentation of character renders before the paste (sprite_augment.hip; pa_sprite_augment)
// ---------------------------------------------------------------------------
// one workgroup's scratch: [128 x h1 resize, later the chain's C x C output][horizontal bicubic pass, later the C x C canvas]
// [128 x 128 canvas], dwords
constexpr size_t SPRITE_SCRATCH_R0 = 128 * PA_SPRITE_H1_MAX * 4, SPRITE_SCRATCH_R1 = 128 * PA_SPRITE_H1_MAX * 4, SPRITE_SCRATCH_R2 = 128 * 128 * 4;
constexpr size_t SPRITE_SCRATCH_BYTES = SPRITE_SCRATCH_R0 + SPRITE_SCRATCH_R1 + SPRITE_SCRATCH_R2;
constexpr int SPRITE_WORKGROUPS_MAX = 256;
struct SpriteAugArgs {
    const uint8_t* sprite_px;        // the source bank's first pixel
    const SynthDesc* sprite_desc;
    int n_sprites;
    const pa_sprite_aug_params* params;   // device, [n]
    int n;
    uint8_t* out_px;                 // the output bank's first pixel: slot i at i * 65536
    uint8_t* scratch;                // [workgroups][SPRITE_SCRATCH_BYTES]
    int workgroups;
    const AugmentTables* tabs;
};
hipError_t launch_sprite_augment(const SpriteAugArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// the detector's synthetic training images (sprite_resize.hip, scene_composite.hip; pa_sprite_resize, pa_scene_composite)
// ---------------------------------------------------------------------------
constexpr int RESIZE_WORKGROUPS_MAX = 256;
struct SpriteResizeArgs {
    const uint8_t* sprite_px;        // the source bank's first pixel
    const SynthDesc* sprite_desc;
    int n_sprites;
    const pa_sprite_resize_params* params;   // device, [n]
    int n;
    SynthDesc* out_desc;             // the output bank's descriptor table: entries 0..n-1 are written
    uint8_t* out_px;                 // its first pixel: slot i at i * slot_bytes
    size_t slot_bytes;
    int max_w, max_h;                // a slot's capacity
    uint8_t* scratch;                // [workgroups][PA_SYNTH_SPRITE_MAX * max_w] dwords: the horizontal pass's output
    int workgroups;
};
hipError_t launch_sprite_resize(const SpriteResizeArgs& a, hipStream_t s);

struct SceneArgs {
    const uint8_t* sprite_px;        // a bank of 128 x 128 RGBA slots
    int n_slots;
    const uint8_t* stage_px;         // the stage bank's first pixel (RGB images, each 16-byte aligned and padded to 16)
    const SynthDesc* stage_desc;
    int n_stages;
    const pa_scene_params* params;   // device, [n]
    int n;
    uint8_t* images;                 // 16-byte aligned
    size_t images_capacity;
    pa_crop_image* desc;             // device, [n]: written by the layout launch, read by the scenes'
    int groups_x;                    // workgroups per scene, sized by the bank's largest stage
};
hipError_t launch_scene_composite(const SceneArgs& a, hipStream_t s);

}  // namespace pa

// How a convolution row of a layer table becomes kernel launch parameters, and where each kernel form's copy of its weights lives:
// the host code the three executors (pa_api.hip's ResNet-18 engine, convnet.hip, yolo.hip) share. No kernel here. Which form a row
// takes, and in what order the forms are tried, stays with each executor.
#pragma once
#include "gemm_tile.h"   // im2col_tile: the im2col engine's choice of tile shape
#include "pa_kernels.h"
#include <cstring>
#include <vector>

namespace pa {

// fp32 -> bf16, round to nearest even (host side: weights at create); inf and NaN by truncation (a quiet NaN stays one)
inline unsigned short bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)(u >> 16);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// A k x k convolution (k = 1 | 3) of `images` zero-bordered NHWC maps, input and output possibly channel slices of wider pixels
// (px strides >= cin / cout; the slice's channel offset goes into the pointers, which the caller sets)
struct ConvRow {
    int images, in_h, in_w, in_pad, in_px_stride, cin, cout, ksize, stride, out_pad, out_px_stride;
    int act;        // GemmParams::relu
    int res_after;  // GemmParams::res_after
};
// its GemmParams: conv mode, strides and counts in elements, splitk = 1, no pointers
GemmParams conv_row_params(const ConvRow& r);

// the Winograd launch of a stride-1 3x3 row from its filled GemmParams: pointers, strides and epilogue as there; no split-K scratch
WinoParams wino_params(const GemmParams& p, int n_img, int height, int width, int cin, const float* filters, int bn);

// The per-form copies of a table's convolution weights: up to three device planes and each row's offset into them.
enum { FORM_WINO = 1, FORM_PSGEMM = 2, FORM_BGEMM = 4 };
struct FormRow {
    int forms = 0;             // FORM_* the caller has decided the row takes; 0 = none (not a convolution, or its fp32 weights only)
    int cin = 0, cout = 0, ksize = 0;
    int residual = 0;          // the row adds a residual (part of the psgemm / bgemm layouts)
    long long w_off = 0;       // its [cout][ky][kx][cin] fp32 weights in the host blob
    long long wino_tiles = 0;  // FORM_WINO: 4 x 4 input tiles at full batch, what wino_pick_bn sizes the channel tile by
    // FORM_BGEMM, a plane the caller packed itself (the conv-net's stem): copied into the row's slot as it is
    const unsigned short* packed = nullptr;
    size_t packed_elems = 0;
};
struct FormWeights {
    float* wino = nullptr;             // wino_transform_weights' filters (wino.hip)
    unsigned short* psgemm = nullptr;  // three bf16 slices per weight (psgemm_pack_weights)
    unsigned short* bgemm = nullptr;   // one RNE bf16 plane (bgemm_pack_weights), every row's 256-byte aligned
    std::vector<long long> wino_off, psgemm_off, bgemm_off;  // per row: element offset into its plane, -1 = the row has no such form
    std::vector<int> wino_bn;          // per row: output channels per workgroup its Winograd filters were laid out for
    FormWeights() = default;
    FormWeights(const FormWeights&) = delete;
    FormWeights& operator=(const FormWeights&) = delete;
    ~FormWeights();
    // offsets, sizes, packing, allocation and upload on the current device; on failure *what names the step that failed
    hipError_t prepare(const std::vector<FormRow>& rows, const float* blob, const char** what);
};

}  // namespace pa

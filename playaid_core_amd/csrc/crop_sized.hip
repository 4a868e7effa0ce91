// Crop stage at ANY output size: YoloCrop.square_crop(frame, output_size = S, padding) (playaid/fighter.py:323-381) for
// S = 16 .. 512 -> uint8 [crop][S][S][3] (pa_square_crops_sized). preprocess.hip's kernels are the 128 x 128 path and stay as
// they are: its fused kernel's sub-band search, LDS layout and INTER_AREA tables are all laid out for 128 destination rows.
//
// The arithmetic is that file's, through crop_common.h (built with -ffp-contract=off like it): truncating pixel box, clipped
// numpy slice, ImageOps.pad to the square (Pillow BICUBIC: 22-bit fixed point, horizontal pass, u8, vertical pass), then
// imutils.resize(width = S) = cv2.resize(INTER_AREA) to (S, int(d * (S / float(d)))) in all of its branches -- copy, 2 x 2,
// integer scale, general shrink in OpenCV's fp32 order, and the fixed-point bilinear emulation when d < S -- and the black
// last row when that height is S - 1.
//
// Form: the multi-pass one of preprocess.hip's fallback, with each pass a launch of its own so that every crop is spread over
// the chip (a call carries a handful of crops, not a clip's worth):
//   plan   one workgroup per crop: geometry (one lane), then the Pillow tables the engine's cache does not hold
//   H      slice -> t1, one thread per (slice row, resized column)
//   V      t1 (or the slice) -> t2, one thread per resized pixel
//   area   t2 / t1 / slice -> crop, one thread per destination pixel
// The intermediates and tables are the engine's (sized by its frame capacity, not by S): nothing here depends on S but the
// launch grids. A crop the reference fails on (status != 0) is written as zeros.
#include "crop_common.h"

namespace pa {

namespace {

constexpr int CS_PASS_BLOCKS = 32;  // workgroups per crop of the two bicubic passes (grid-stride over the pass's elements)

// crop_plan_kernel's geometry with `out_size` in the place of 128 (no LDS sub-band search: there is no fused form here)
__global__ __launch_bounds__(256) void crop_sized_plan_kernel(const PreprocParams p, const int out_size) {
    __shared__ CropPlan plan_sh;
    const int crop = blockIdx.x;
    if (threadIdx.x == 0) {
        CropPlan pl;
        pl.status = PA_CROP_OK;
        pl.frame = p.src_frame ? p.src_frame[crop] : crop / p.fighters;
        pl.sx0 = pl.sy0 = pl.sw = pl.sh = 0;
        pl.d = pl.rw = pl.rh = pl.px = pl.py = 0;
        pl.need_h = pl.need_v = pl.ksize_h = pl.ksize_v = 0;
        pl.out_h = 0;
        pl.area_mode = 0;
        pl.iscale_x = pl.iscale_y = 1;
        pl.fused_rb = 0;
        pl.mfma_v = 0;
        pl.mfma_h = pl.h_mis = 0;
        pl.coef_h = pl.coef_v = nullptr;
        pl.scale_x = pl.scale_y = 1.0;
        const double* b = p.boxes + (size_t)crop * 4;
        const int W = p.width, H = p.height, pad = p.padding;
        if ((unsigned)pl.frame >= (unsigned)p.n_src) {  // a source index outside the frame buffer: never dereferenced
            pl.frame = 0;
            pl.status = PA_CROP_BAD_FRAME;
        }
        int cx, cy, cw, ch;
        // YoloCrop.yolo_pixels (fighter.py:305-314)
        if (pl.status == PA_CROP_OK && (!to_int_checked(b[0] * W, &cx) || !to_int_checked(b[1] * H, &cy) || !to_int_checked(b[2] * W, &cw) ||
                                        !to_int_checked(b[3] * H, &ch)))
            pl.status = PA_CROP_BAD_BOX;
        if (pl.status == PA_CROP_OK) {
            pl.d = cw > ch ? cw : ch;
            if (pl.d <= 0 || pl.d > 16384) pl.status = PA_CROP_BAD_BOX;
        }
        if (pl.status == PA_CROP_OK) {
            const int d = pl.d;
            const int half = d / 2;  // int(square_dim / 2)
            int y0 = cy - half - pad, y1 = cy + half + pad, x0 = cx - half - pad, x1 = cx + half + pad;
            y0 = y0 > 0 ? y0 : 0;
            x0 = x0 > 0 ? x0 : 0;
            y1 = y1 < H ? y1 : H;
            x1 = x1 < W ? x1 : W;
            np_slice(y0, y1, H, &pl.sy0, &pl.sh);
            np_slice(x0, x1, W, &pl.sx0, &pl.sw);
            if (pl.sh != d || pl.sw != d) {
                // ImageOps.pad(raw_crop, (d, d), color="black"); the empty slices: see crop_plan_kernel
                if (pl.sh == 0 || pl.sw == 0) {
                    pl.status = (pl.sw == 0 && pl.sh == d) ? PA_CROP_BLANK : PA_CROP_EMPTY;
                } else {
                    int rw = d, rh = d;
                    const double im_ratio = (double)pl.sw / (double)pl.sh;
                    if (im_ratio != 1.0) {
                        if (im_ratio > 1.0) {
                            const int nh = (int)rint((double)pl.sh / (double)pl.sw * (double)d);
                            if (nh != d) rh = nh;
                        } else {
                            const int nw = (int)rint((double)pl.sw / (double)pl.sh * (double)d);
                            if (nw != d) rw = nw;
                        }
                    }
                    if (rw <= 0 || rh <= 0) {
                        pl.status = PA_CROP_EMPTY;
                    } else {
                        pl.rw = rw;
                        pl.rh = rh;
                        pl.need_h = rw != pl.sw;
                        pl.need_v = rh != pl.sh;
                        if (rw != d)
                            pl.px = (int)rint((double)(d - rw) * 0.5);
                        else if (rh != d)
                            pl.py = (int)rint((double)(d - rh) * 0.5);
                        if (pl.need_h) pl.ksize_h = bicubic_ksize(pl.sw, rw);
                        if (pl.need_v) pl.ksize_v = bicubic_ksize(pl.sh, rh);
                        // the two kernel limits (include/playaid_hip.h at pa_square_crops_sized): PA_KSIZE_MAX taps per pass, and
                        // intermediates / tables within the engine's frame capacity
                        if (pl.ksize_h > PA_KSIZE_MAX || pl.ksize_v > PA_KSIZE_MAX) pl.status = PA_CROP_FILTER_TOO_WIDE;
                        if ((size_t)pl.sh * rw * 3 > p.t_stride || (size_t)rh * rw * 3 > p.t_stride || rw > p.coef_dim || rh > p.coef_dim)
                            pl.status = PA_CROP_FILTER_TOO_WIDE;
                    }
                }
            } else {
                pl.rw = pl.rh = d;
            }
        }
        if (pl.status == PA_CROP_OK) {
            const int d = pl.d;
            // imutils.resize(width=S): dim = (S, int(h * (S / float(w))))
            const double r = (double)out_size / (double)d;
            pl.out_h = (int)((double)d * r);
            const double inv_sx = (double)out_size / (double)d;
            const double inv_sy = (double)pl.out_h / (double)d;
            pl.scale_x = 1.0 / inv_sx;
            pl.scale_y = 1.0 / inv_sy;
            if (d == out_size && pl.out_h == out_size) {
                pl.area_mode = 0;  // cv::resize of equal sizes copies
            } else if (pl.scale_x < 1.0 || pl.scale_y < 1.0) {
                pl.area_mode = 4;  // a source smaller than S: the fixed-point bilinear emulation
            } else {
                pl.iscale_x = (int)rint(pl.scale_x);  // saturate_cast<int>(double) == cvRound
                pl.iscale_y = (int)rint(pl.scale_y);
                const bool fast = fabs(pl.scale_x - pl.iscale_x) < 2.220446049250313e-16 && fabs(pl.scale_y - pl.iscale_y) < 2.220446049250313e-16;
                pl.area_mode = fast ? ((pl.iscale_x == 2 && pl.iscale_y == 2) ? 1 : 2) : 3;
            }
            if (pl.out_h < 1 || pl.out_h > out_size) pl.status = PA_CROP_BAD_BOX;  // (int(d * (S / d)) is S or S - 1: never taken)
        }
        // coefficient tables: the engine's cache of the (2 * (d / 2) + 2 * padding -> d) passes, or this crop's own rows
        for (int axis = 0; axis < 2; ++axis) {
            const int in_size = axis ? pl.sh : pl.sw, out = axis ? pl.rh : pl.rw;
            const bool cached = p.coef_cache && in_size == 2 * (out / 2) + 2 * p.coef_cache_pad && out >= 1 && out <= p.coef_cache_dmax;
            const int32_t* tab = cached ? p.coef_cache + (size_t)out * (out - 1) / 2 * COEF_ROW : p.coef + (size_t)(crop * 2 + axis) * p.coef_dim * COEF_ROW;
            if (axis) pl.coef_v = tab; else pl.coef_h = tab;
        }
        p.plans[crop] = pl;
        plan_sh = pl;
        if (p.status) p.status[crop] = pl.status == PA_CROP_BLANK ? PA_CROP_OK : pl.status;
    }
    __syncthreads();
    const CropPlan pl = plan_sh;
    if (pl.status != PA_CROP_OK) return;
    // Pillow precompute_coeffs + normalize_coeffs_8bpc for the passes the cache does not hold (one thread per output coordinate)
    for (int axis = 0; axis < 2; ++axis) {
        if (!(axis ? pl.need_v : pl.need_h)) continue;
        const int in_size = axis ? pl.sh : pl.sw, out = axis ? pl.rh : pl.rw;
        int32_t* own = p.coef + (size_t)(crop * 2 + axis) * p.coef_dim * COEF_ROW;
        if ((axis ? pl.coef_v : pl.coef_h) != own) continue;
        for (int xx = threadIdx.x; xx < out; xx += 256) bicubic_coef_row(in_size, out, xx, own + (size_t)xx * COEF_ROW);
    }
}

// ImagingResampleHorizontal_8bpc over the slice rows: t1[y][xx][c]
__global__ __launch_bounds__(256) void crop_sized_h_kernel(const PreprocParams p) {
    const int crop = blockIdx.y;
    const CropPlan pl = p.plans[crop];
    if (pl.status != PA_CROP_OK || !pl.need_h) return;
    const int total = pl.sh * pl.rw;
    size_t src_pitch;
    const uint8_t* src = slice_ptr(p, crop, pl, &src_pitch);
    uint8_t* dst = p.t1 + (size_t)crop * p.t_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int y = i / pl.rw;
        const int xx = i - y * pl.rw;
        const int32_t* row = pl.coef_h + (size_t)xx * COEF_ROW;
        const int xmin = row[0], cnt = row[1];
        const uint8_t* s = src + (size_t)y * src_pitch + (size_t)xmin * 3;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int x = 0; x < cnt; ++x) {
            const int k = row[2 + x];
            a0 += __mul24((int)s[3 * x + 0], k);  // u8 x 22-bit fixed point: fits v_mad_i32_i24
            a1 += __mul24((int)s[3 * x + 1], k);
            a2 += __mul24((int)s[3 * x + 2], k);
        }
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = (uint8_t)clip8(a0);
        o[1] = (uint8_t)clip8(a1);
        o[2] = (uint8_t)clip8(a2);
    }
}

// ImagingResampleVertical_8bpc: t2[yy][x][c] from t1 (or the slice when no horizontal pass ran)
__global__ __launch_bounds__(256) void crop_sized_v_kernel(const PreprocParams p) {
    const int crop = blockIdx.y;
    const CropPlan pl = p.plans[crop];
    if (pl.status != PA_CROP_OK || !pl.need_v) return;
    const int total = pl.rh * pl.rw;
    const uint8_t* src;
    size_t src_pitch;
    if (pl.need_h) {
        src = p.t1 + (size_t)crop * p.t_stride;
        src_pitch = (size_t)pl.rw * 3;
    } else {
        src = slice_ptr(p, crop, pl, &src_pitch);
    }
    uint8_t* dst = p.t2 + (size_t)crop * p.t_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int yy = i / pl.rw;
        const int x = i - yy * pl.rw;
        const int32_t* row = pl.coef_v + (size_t)yy * COEF_ROW;
        const int ymin = row[0], cnt = row[1];
        const uint8_t* s = src + (size_t)ymin * src_pitch + (size_t)x * 3;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int y = 0; y < cnt; ++y) {
            const int k = row[2 + y];
            a0 += __mul24((int)s[0], k);
            a1 += __mul24((int)s[1], k);
            a2 += __mul24((int)s[2], k);
            s += src_pitch;
        }
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = (uint8_t)clip8(a0);
        o[1] = (uint8_t)clip8(a1);
        o[2] = (uint8_t)clip8(a2);
    }
}

// INTER_AREA d x d canvas -> out_h x S, rows from out_h on black (the pad to S x S), failed crops all black; channel swap
__global__ __launch_bounds__(256) void crop_sized_area_kernel(const PreprocParams p, const int out_size) {
    const int crop = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= out_size * out_size) return;
    const CropPlan pl = p.plans[crop];
    int o0 = 0, o1 = 0, o2 = 0;
    if (pl.status == PA_CROP_OK) {
        Canvas cv;
        cv.px = pl.px; cv.py = pl.py; cv.rw = pl.rw; cv.rh = pl.rh;
        if (pl.need_v) {
            cv.src = p.t2 + (size_t)crop * p.t_stride;
            cv.pitch = (size_t)pl.rw * 3;
        } else if (pl.need_h) {
            cv.src = p.t1 + (size_t)crop * p.t_stride;
            cv.pitch = (size_t)pl.rw * 3;
        } else {
            cv.src = slice_ptr(p, crop, pl, &cv.pitch);
        }
        const int dy = i / out_size, dx = i - dy * out_size;
        if (dy < pl.out_h) area_pixel(pl, cv, dy, dx, o0, o1, o2, (double)out_size);
    }
    if (p.swap_rb) {
        const int t = o0;
        o0 = o2;
        o2 = t;
    }
    uint8_t* o = p.crops_u8 + ((size_t)crop * out_size * out_size + i) * 3;
    o[0] = (uint8_t)o0;
    o[1] = (uint8_t)o1;
    o[2] = (uint8_t)o2;
}

}  // namespace

hipError_t launch_crop_sized(const PreprocParams& p, int out_size, hipStream_t s) {
    const int ncrops = p.n_frames * p.fighters;
    if (ncrops <= 0) return hipSuccess;
    if (out_size < PA_CROP_SIZE_MIN || out_size > PA_CROP_SIZE_MAX || !p.crops_u8 || p.windows || !p.plans || !p.coef || !p.t1 || !p.t2)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(crop_sized_plan_kernel, dim3(ncrops), dim3(256), 0, s, p, out_size);
    hipLaunchKernelGGL(crop_sized_h_kernel, dim3(CS_PASS_BLOCKS, ncrops), dim3(256), 0, s, p);
    hipLaunchKernelGGL(crop_sized_v_kernel, dim3(CS_PASS_BLOCKS, ncrops), dim3(256), 0, s, p);
    hipLaunchKernelGGL(crop_sized_area_kernel, dim3((out_size * out_size + 255) / 256, ncrops), dim3(256), 0, s, p, out_size);
    return hipGetLastError();
}

}  // namespace pa

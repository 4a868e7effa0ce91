// Device helpers of the crop stage shared by preprocess.hip (the 128 x 128 path) and crop_sized.hip (any output size): what
// of the stage needs PreprocParams -- where a crop's slice, intermediates and coefficient tables lie, the plan kernels'
// common head and tail, and the two bicubic passes over global memory. The reference's slice / Pillow BICUBIC / OpenCV
// INTER_AREA arithmetic itself is crop_math.h's (host-compilable, pinned on the CPU by tests/test_crop_math_host.py). Both
// files are built with -ffp-contract=off (see preprocess.hip's head comment); nothing here may be compiled with fused
// multiply-adds.
#pragma once
#include "tile_common.h"
#include "crop_math.h"

namespace pa {

// First byte and row pitch of a crop's slice: inside the whole frame, or -- window ingest (pa_preprocess_windows) --
// inside the packed copy of just that slice that the host uploaded.
__device__ __forceinline__ const uint8_t* slice_ptr(const PreprocParams& p, int crop, const CropPlan& pl, size_t* pitch) {
    if (p.windows) {
        *pitch = (size_t)p.windows[crop].pitch;
        return p.frames + p.windows[crop].offset;
    }
    *pitch = (size_t)p.width * 3;
    return p.frames + ((size_t)pl.frame * p.height + pl.sy0) * p.width * 3 + (size_t)pl.sx0 * 3;
}

// A crop's image as it stands behind the vertical pass (after_v) or in front of it: t2, else t1, else the slice itself.
__device__ __forceinline__ const uint8_t* crop_image(const PreprocParams& p, int crop, const CropPlan& pl, bool after_v, size_t* pitch) {
    if (!(after_v && pl.need_v) && !pl.need_h) return slice_ptr(p, crop, pl, pitch);
    *pitch = (size_t)pl.rw * 3;
    return ((after_v && pl.need_v) ? p.t2 : p.t1) + (size_t)crop * p.t_stride;
}

// The d x d canvas the INTER_AREA step of a crop reads from global memory
__device__ __forceinline__ Canvas crop_canvas(const PreprocParams& p, int crop, const CropPlan& pl) {
    Canvas cv;
    cv.px = pl.px; cv.py = pl.py; cv.rw = pl.rw; cv.rh = pl.rh;
    cv.src = crop_image(p, crop, pl, true, &cv.pitch);
    return cv;
}

// ImagingResampleHorizontal_8bpc over the slice rows: t1[y][xx][c]; items first, first + step, ...
__device__ __forceinline__ void crop_pass_h(const PreprocParams& p, int crop, const CropPlan& pl, int first, int step) {
    if (!pl.need_h) return;
    size_t src_pitch;
    const uint8_t* src = slice_ptr(p, crop, pl, &src_pitch);
    bicubic_pass_h(pl.coef_h, src, src_pitch, pl.sh, pl.rw, p.t1 + (size_t)crop * p.t_stride, first, step);
}

// ImagingResampleVertical_8bpc: t2[yy][x][c] from t1 (or the slice when no horizontal pass ran)
__device__ __forceinline__ void crop_pass_v(const PreprocParams& p, int crop, const CropPlan& pl, int first, int step) {
    if (!pl.need_v) return;
    size_t src_pitch;
    const uint8_t* src = crop_image(p, crop, pl, false, &src_pitch);
    bicubic_pass_v(pl.coef_v, src, src_pitch, pl.rh, pl.rw, p.t2 + (size_t)crop * p.t_stride, first, step);
}

// Head of a plan kernel: the geometry of crop `crop` at out_size. (The 128 path's window ingest has no frame buffer to
// index; crop_sized refuses windows.)
__device__ __forceinline__ CropPlan crop_plan_geometry(const PreprocParams& p, int crop, int out_size) {
    const int frame = p.src_frame ? p.src_frame[crop] : crop / p.fighters;
    const bool frame_ok = p.windows || (unsigned)frame < (unsigned)p.n_src;
    return square_crop_plan(p.boxes + (size_t)crop * 4, p.width, p.height, p.padding, out_size, p.t_stride, p.coef_dim, frame, frame_ok);
}

// Tail of a plan kernel, one thread: the crop's coefficient tables -- a pass (2 * (d / 2) + 2 * padding -> d), the slice
// of every crop the frame edge does not clip (fighter.py:334-343: centre -/+ int(d / 2) -/+ padding), reads the engine's
// cache; any other pair gets this crop's own rows (crop_plan_fill_tables) -- then the plan and the reported status.
__device__ __forceinline__ void crop_plan_publish(const PreprocParams& p, int crop, CropPlan& pl) {
    for (int axis = 0; axis < 2; ++axis) {
        const int in_size = axis ? pl.sh : pl.sw, out_size = axis ? pl.rh : pl.rw;
        const bool cached = p.coef_cache && in_size == 2 * (out_size / 2) + 2 * p.coef_cache_pad && out_size >= 1 &&
                            out_size <= p.coef_cache_dmax;
        const int32_t* tab = cached ? p.coef_cache + (size_t)out_size * (out_size - 1) / 2 * COEF_ROW
                                    : p.coef + (size_t)(crop * 2 + axis) * p.coef_dim * COEF_ROW;
        if (axis) pl.coef_v = tab; else pl.coef_h = tab;
    }
    p.plans[crop] = pl;
    if (p.status) p.status[crop] = pl.status == PA_CROP_BLANK ? PA_CROP_OK : pl.status;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for the passes the cache does not hold (one thread of the workgroup's
// 256 per output coordinate)
__device__ __forceinline__ void crop_plan_fill_tables(const PreprocParams& p, int crop, const CropPlan& pl) {
    for (int axis = 0; axis < 2; ++axis) {
        if (!(axis ? pl.need_v : pl.need_h)) continue;
        int32_t* own = p.coef + (size_t)(crop * 2 + axis) * p.coef_dim * COEF_ROW;
        if ((axis ? pl.coef_v : pl.coef_h) != own) continue;
        bicubic_coef_table(axis ? pl.sh : pl.sw, axis ? pl.rh : pl.rw, own, threadIdx.x, 256);
    }
}

}  // namespace pa

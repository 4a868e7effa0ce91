// Crop stage at ANY output size: YoloCrop.square_crop(frame, output_size = S, padding) (playaid/fighter.py:323-381) for
// S = 16 .. 512 -> uint8 [crop][S][S][3] (pa_square_crops_sized). preprocess.hip's kernels are the 128 x 128 path and stay as
// they are: its fused kernel's sub-band search, LDS layout and INTER_AREA tables are all laid out for 128 destination rows.
//
// The arithmetic is that file's -- crop_math.h, and crop_common.h for where a crop's data lies (built with -ffp-contract=off
// like it): truncating pixel box, clipped
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

// crop_plan_kernel's head and tail (crop_common.h) at `out_size` (no LDS sub-band search: there is no fused form here)
__global__ __launch_bounds__(256) void crop_sized_plan_kernel(const PreprocParams p, const int out_size) {
    __shared__ CropPlan plan_sh;
    const int crop = blockIdx.x;
    if (threadIdx.x == 0) {
        CropPlan pl = crop_plan_geometry(p, crop, out_size);
        crop_plan_publish(p, crop, pl);
        plan_sh = pl;
    }
    __syncthreads();
    const CropPlan pl = plan_sh;
    if (pl.status != PA_CROP_OK) return;
    crop_plan_fill_tables(p, crop, pl);
}

__global__ __launch_bounds__(256) void crop_sized_h_kernel(const PreprocParams p) {
    const int crop = blockIdx.y;
    const CropPlan pl = p.plans[crop];
    if (pl.status != PA_CROP_OK) return;
    crop_pass_h(p, crop, pl, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

__global__ __launch_bounds__(256) void crop_sized_v_kernel(const PreprocParams p) {
    const int crop = blockIdx.y;
    const CropPlan pl = p.plans[crop];
    if (pl.status != PA_CROP_OK) return;
    crop_pass_v(p, crop, pl, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// INTER_AREA d x d canvas -> out_h x S, rows from out_h on black (the pad to S x S), failed crops all black; channel swap
__global__ __launch_bounds__(256) void crop_sized_area_kernel(const PreprocParams p, const int out_size) {
    const int crop = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= out_size * out_size) return;
    const CropPlan pl = p.plans[crop];
    int o0 = 0, o1 = 0, o2 = 0;
    if (pl.status == PA_CROP_OK) {
        const int dy = i / out_size, dx = i - dy * out_size;
        if (dy < pl.out_h) area_pixel(area_geom(pl, out_size), crop_canvas(p, crop, pl), dy, dx, o0, o1, o2);
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

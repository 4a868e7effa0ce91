// Device helpers of the crop stage shared by preprocess.hip (the 128 x 128 path) and crop_sized.hip (any output size):
// the reference's slice / Pillow BICUBIC / OpenCV INTER_AREA arithmetic, bit for bit. Both files are built with
// -ffp-contract=off (see preprocess.hip's head comment); nothing here may be compiled with fused multiply-adds.
#pragma once
#include "tile_common.h"
#include "../../include/playaid_hip.h"

namespace pa {

#define PRECISION_BITS 22
#define COEF_ROW (2 + PA_KSIZE_MAX)

__device__ __forceinline__ bool to_int_checked(double v, int* out) {
    if (!(v > -2.0e9 && v < 2.0e9)) return false;  // also rejects NaN
    *out = (int)v;                                 // C cast == Python int(): truncation
    return true;
}

// numpy basic-slice length for image[start:stop] with start >= 0.
__device__ __forceinline__ void np_slice(int start, int stop, int size, int* s0, int* len) {
    if (start > size) start = size;
    if (stop < 0) {
        stop += size;
        if (stop < 0) stop = 0;
    }
    if (stop > size) stop = size;
    *s0 = start;
    *len = stop > start ? stop - start : 0;
}

__device__ __forceinline__ int bicubic_ksize(int in_size, int out_size) {
    double scale = (double)(float)in_size / out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(2.0 * filterscale) * 2 + 1;
}


// Pillow precompute_coeffs bounds (first tap, tap count) of output coordinate
// xx for a pass in_size -> out_size: the same arithmetic as bicubic_coef_row.
__device__ __forceinline__ void bicubic_bounds(int in_size, int out_size, int xx, int* xmin, int* cnt) {
    const double scale = (double)(float)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in_size) hi = in_size;
    *xmin = lo;
    *cnt = hi - lo;
}

// computeResizeAreaTab for one destination coordinate.
struct AreaTab {
    int s_first;     // source index of entry 0
    int n;           // number of entries
    float a_first;   // alpha of a leading partial cell (if has_first)
    float a_mid;     // alpha of the full cells
    float a_last;    // alpha of a trailing partial cell (if has_last)
    int has_first, n_mid, has_last;
};

__device__ __forceinline__ AreaTab area_tab(int dx, double scale, int ssize) {
    AreaTab t;
    const double fsx1 = dx * scale;
    const double fsx2 = fsx1 + scale;
    const double cell = fmin(scale, ssize - fsx1);
    int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
    sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
    sx1 = sx1 < sx2 ? sx1 : sx2;
    t.has_first = (sx1 - fsx1 > 1e-3) ? 1 : 0;
    t.a_first = (float)((sx1 - fsx1) / cell);
    t.n_mid = sx2 - sx1;
    t.a_mid = (float)(1.0 / cell);
    t.has_last = (fsx2 - sx2 > 1e-3) ? 1 : 0;
    t.a_last = (float)(fmin(fmin(fsx2 - sx2, 1.0), cell) / cell);
    t.s_first = sx1 - t.has_first;
    t.n = t.has_first + t.n_mid + t.has_last;
    return t;
}

// 16-byte LDS form of an AreaTab (s_first < 2^16, n_mid < 2^8 for any square side the plan accepts)
__device__ __forceinline__ AreaTabPacked area_pack(const AreaTab& t) {
    AreaTabPacked q;
    q.bits = (uint32_t)t.s_first | ((uint32_t)t.n_mid << 16) | ((uint32_t)t.has_first << 24) | ((uint32_t)t.has_last << 25);
    q.a_first = t.a_first;
    q.a_mid = t.a_mid;
    q.a_last = t.a_last;
    return q;
}

__device__ __forceinline__ AreaTab area_unpack(const AreaTabPacked& q) {
    AreaTab t;
    t.s_first = (int)(q.bits & 0xffff);
    t.n_mid = (int)((q.bits >> 16) & 0xff);
    t.has_first = (int)((q.bits >> 24) & 1);
    t.has_last = (int)((q.bits >> 25) & 1);
    t.n = t.has_first + t.n_mid + t.has_last;
    t.a_first = q.a_first;
    t.a_mid = q.a_mid;
    t.a_last = q.a_last;
    return t;
}

// (by value, as selects of values: taking the table by reference made hipcc keep it in scratch memory and turn the
// choice into an indexed scratch load -- which gave the whole fused kernel a private segment)
__device__ __forceinline__ float area_alpha(const AreaTab t, int k) {
    const float a_first = t.a_first, a_mid = t.a_mid, a_last = t.a_last;
    const int hf = t.has_first, hm = t.has_first + t.n_mid;
    float r = a_last;
    r = k < hm ? a_mid : r;
    r = k < hf ? a_first : r;
    return r;
}

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

__device__ __forceinline__ double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for output coordinate xx of a pass in_size -> out_size
// into row[0] = first tap, row[1] = tap count, row[2..] = coefficients.
// (out of line: the plan kernel runs once per clip with its code cold, every line of it fetched from memory, and the
// passes of almost every crop are in the engine's cache)
__device__ __noinline__ void bicubic_coef_row(int in_size, int out_size, int xx, int32_t* row) {
    const double scale = (double)(float)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double k[PA_KSIZE_MAX];
    double ww = 0.0;
    for (int x = 0; x < PA_KSIZE_MAX; ++x) {
        double w = 0.0;
        if (x < xmax) {
            w = bicubic_filter((x + xmin - center + 0.5) * ss);
            ww += w;
        }
        k[x] = w;
    }
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < PA_KSIZE_MAX; ++x) {
        double v = k[x];
        if (x < xmax && ww != 0.0) v = v / ww;
        row[2 + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << PRECISION_BITS)) : (int)(0.5 + v * (double)(1 << PRECISION_BITS));
    }
}

// Pillow clip8: (acc >> 22) clamped to 0..255. Returns a 32-bit value on purpose: with a
// uint8_t return type hipcc 7.2 packed the four bytes of the vertical pass through 16-bit
// v_bitop3_b16 operations and bytes 2/3 of each dword came out wrong on gfx950.
__device__ __forceinline__ uint32_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct Canvas {
    const uint8_t* src;
    size_t pitch;
    int px, py, rw, rh;
    // d x d black canvas with the resized slice pasted at (px, py)
    __device__ __forceinline__ void load(int y, int x, int& c0, int& c1, int& c2) const {
        y -= py;
        x -= px;
        if ((unsigned)y < (unsigned)rh && (unsigned)x < (unsigned)rw) {
            const uint8_t* s = src + (size_t)y * pitch + (size_t)x * 3;
            c0 = s[0];
            c1 = s[1];
            c2 = s[2];
        } else {
            c0 = c1 = c2 = 0;
        }
    }
};

__device__ __forceinline__ int cv_saturate_u8(float v) {
    const int r = (int)rintf(v);  // cvRound: round half to even
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// One destination pixel of cv::resize INTER_AREA (d x d canvas -> out_h x out_w; out_w = 128 for the 128 path, whose
// CropPlan scales were formed from 128 as well).
// CV::load(y, x, c0, c1, c2) returns the canvas pixel (black outside the paste).
template <class CV>
__device__ __forceinline__ void area_pixel(const CropPlan& pl, const CV& cv, int dy, int dx, int& o0, int& o1, int& o2,
                                           const double out_w = (double)PA_CROP) {
    if (pl.area_mode == 0) {
        cv.load(dy, dx, o0, o1, o2);
    } else if (pl.area_mode == 1) {
        int s0 = 2, s1 = 2, s2 = 2;
        for (int yy = 0; yy < 2; ++yy)
            for (int xx = 0; xx < 2; ++xx) {
                int c0, c1, c2;
                cv.load(dy * 2 + yy, dx * 2 + xx, c0, c1, c2);
                s0 += c0; s1 += c1; s2 += c2;
            }
        o0 = s0 >> 2; o1 = s1 >> 2; o2 = s2 >> 2;
    } else if (pl.area_mode == 2) {
        int s0 = 0, s1 = 0, s2 = 0;
        for (int yy = 0; yy < pl.iscale_y; ++yy)
            for (int xx = 0; xx < pl.iscale_x; ++xx) {
                int c0, c1, c2;
                cv.load(dy * pl.iscale_y + yy, dx * pl.iscale_x + xx, c0, c1, c2);
                s0 += c0; s1 += c1; s2 += c2;
            }
        const float scale = 1.f / (float)(pl.iscale_x * pl.iscale_y);
        o0 = cv_saturate_u8((float)s0 * scale);
        o1 = cv_saturate_u8((float)s1 * scale);
        o2 = cv_saturate_u8((float)s2 * scale);
    } else if (pl.area_mode == 4) {
        // enlarging: cv::hal::resize runs the 8-bit bilinear resizer with area-mode coefficients
        // (s = floor(d*scale), f = (d+1) - (s+1)*inv_scale, f <= 0 ? 0 : f - floor(f); weights
        // cvRound(w * 2048)); HResizeLinear keeps 11 fraction bits, VResizeLinear computes
        // (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2. Columns whose right neighbour
        // would leave the source use S[last]*2048; rows only clip the index.
        const int ss = pl.d;
        const double inv_x = out_w / (double)ss, inv_y = (double)pl.out_h / (double)ss;  // dsize / ssize, as cv::resize forms them
        int sx = (int)floor((double)dx * pl.scale_x);
        float fx = (float)((double)(dx + 1) - (double)(sx + 1) * inv_x);
        fx = fx <= 0.f ? 0.f : fx - floorf(fx);
        const bool plain = sx + 1 >= ss;
        if (sx >= ss - 1) {
            fx = 0.f;
            sx = ss - 1;
        }
        const int a0 = (int)rintf((1.f - fx) * 2048.f), a1 = (int)rintf(fx * 2048.f);
        const int sy = (int)floor((double)dy * pl.scale_y);
        float fy = (float)((double)(dy + 1) - (double)(sy + 1) * inv_y);
        fy = fy <= 0.f ? 0.f : fy - floorf(fy);
        const int b0 = (int)rintf((1.f - fy) * 2048.f), b1 = (int)rintf(fy * 2048.f);
        const int r0 = sy < ss - 1 ? sy : ss - 1;
        const int r1 = sy + 1 < ss - 1 ? sy + 1 : ss - 1;
        int h0[3], h1[3];
        {
            int c0, c1, c2, e0 = 0, e1 = 0, e2 = 0;
            cv.load(r0, sx, c0, c1, c2);
            if (!plain) cv.load(r0, sx + 1, e0, e1, e2);
            h0[0] = plain ? c0 * 2048 : c0 * a0 + e0 * a1;
            h0[1] = plain ? c1 * 2048 : c1 * a0 + e1 * a1;
            h0[2] = plain ? c2 * 2048 : c2 * a0 + e2 * a1;
            cv.load(r1, sx, c0, c1, c2);
            if (!plain) cv.load(r1, sx + 1, e0, e1, e2);
            h1[0] = plain ? c0 * 2048 : c0 * a0 + e0 * a1;
            h1[1] = plain ? c1 * 2048 : c1 * a0 + e1 * a1;
            h1[2] = plain ? c2 * 2048 : c2 * a0 + e2 * a1;
        }
        o0 = ((((b0 * (h0[0] >> 4)) >> 16) + ((b1 * (h1[0] >> 4)) >> 16) + 2) >> 2) & 0xff;
        o1 = ((((b0 * (h0[1] >> 4)) >> 16) + ((b1 * (h1[1] >> 4)) >> 16) + 2) >> 2) & 0xff;
        o2 = ((((b0 * (h0[2] >> 4)) >> 16) + ((b1 * (h1[2] >> 4)) >> 16) + 2) >> 2) & 0xff;
    } else {
        const AreaTab tx = area_tab(dx, pl.scale_x, pl.d);
        const AreaTab ty = area_tab(dy, pl.scale_y, pl.d);
        float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f;
        for (int j = 0; j < ty.n; ++j) {
            const float beta = area_alpha(ty, j);
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            for (int k = 0; k < tx.n; ++k) {
                const float alpha = area_alpha(tx, k);
                int c0, c1, c2;
                cv.load(ty.s_first + j, tx.s_first + k, c0, c1, c2);
                b0 = b0 + (float)c0 * alpha;
                b1 = b1 + (float)c1 * alpha;
                b2 = b2 + (float)c2 * alpha;
            }
            sum0 = sum0 + beta * b0;
            sum1 = sum1 + beta * b1;
            sum2 = sum2 + beta * b2;
        }
        o0 = cv_saturate_u8(sum0);
        o1 = cv_saturate_u8(sum1);
        o2 = cv_saturate_u8(sum2);
    }
}

}  // namespace pa

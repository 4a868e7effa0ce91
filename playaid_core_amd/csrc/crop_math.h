// The crop stage's reference arithmetic, once each: YoloCrop.square_crop's slice / contain / paste geometry, the branch
// cv::resize(INTER_AREA) takes, one INTER_AREA destination pixel, Pillow's BICUBIC coefficient rows and output values, and
// the base-256 digit form of a coefficient row that the int8 matrix instruction multiplies. Bit for bit what numpy, Pillow and
// OpenCV compute; every kernel of preprocess.hip and crop_sized.hip reaches it through here (crop_common.h adds what needs
// PreprocParams), and tests/helpers/crop_math_table.cpp runs the same functions on the host against the oracle.
//
// No HIP includes: the host C++ compiler alone compiles this header. Under hipcc the functions are __host__ __device__ and
// the includer has the HIP runtime in scope before this header (mul24 uses its __mul24). Whoever compiles it must not fuse
// multiplies and adds (-ffp-contract=off): the coefficient tables are Pillow's double arithmetic and the fractional
// INTER_AREA path is OpenCV's fp32 multiply, then add.
#pragma once
#include "../../include/playaid_hip.h"
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PA_HD __host__ __device__ inline __attribute__((always_inline))
#define PA_HD_COLD __host__ __device__ inline __attribute__((noinline))
#else
#define PA_HD inline
#define PA_HD_COLD inline
#endif

namespace pa {

#define PA_KSIZE_MAX 15
#define PRECISION_BITS 22
#define COEF_ROW (2 + PA_KSIZE_MAX)
// Plan-internal crop status (never reported): a (d x 0) slice that ImageOps.pad turns into a black d x d canvas
// without resizing. The kernels treat it as a failed crop (all-zero pixels); the plan reports PA_CROP_OK.
#define PA_CROP_BLANK 0x100

struct CropPlan {
    int32_t status;
    int32_t frame;
    int32_t sx0, sy0, sw, sh;  // slice of the frame
    int32_t d;                 // square side
    int32_t rw, rh;            // size after ImageOps.contain
    int32_t px, py;            // paste offset inside the d x d canvas
    int32_t need_h, need_v;    // bicubic passes
    int32_t ksize_h, ksize_v;
    int32_t out_h;             // INTER_AREA destination height (width is the output size)
    int32_t area_mode;         // 0 copy, 1 fast 2x2, 2 fast integer, 3 general, 4 enlarging (bilinear emulation)
    int32_t iscale_x, iscale_y;
    int32_t fused_rb;          // output rows per LDS sub-band of the fused kernel (8/4/2/1), 0 = multi-kernel fallback
    int32_t mfma_v;            // the fused kernel's vertical pass runs on the int8 matrix instruction (B1 transposed in LDS)
    // the horizontal pass runs on it as well (only with mfma_v), from the crop's operand in PreprocParams::hop. 1: B0 is
    // staged as the frame's aligned dwords and the operand's tap positions carry the slice's byte misalignment h_mis;
    // 2 (PA_CROP_MFMA_H=2, the A/B row of the staging alone): B0 is staged re-aligned as for the vector form, h_mis = 0
    int32_t mfma_h, h_mis;
    double scale_x, scale_y;
    // Pillow coefficient tables of the two bicubic passes ([out][2 + PA_KSIZE_MAX]): the engine's cache of the
    // (2 * (d / 2) + 2 * padding -> d) pairs, or this crop's own rows of PreprocParams::coef for any other pair
    const int32_t* coef_h;
    const int32_t* coef_v;
};

// One entry of cv::computeResizeAreaTab per destination column / row of a crop (plan kernel -> fused kernel)
struct AreaTabPacked {
    uint32_t bits;  // s_first | n_mid << 16 | has_first << 24 | has_last << 25
    float a_first, a_mid, a_last;
};

// u8 x 22-bit fixed point: fits v_mad_i32_i24 on the device; the same product as a plain multiply
PA_HD int mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

PA_HD bool to_int_checked(double v, int* out) {
    if (!(v > -2.0e9 && v < 2.0e9)) return false;  // also rejects NaN
    *out = (int)v;                                 // C cast == Python int(): truncation
    return true;
}

// numpy basic-slice length for image[start:stop] with start >= 0.
PA_HD void np_slice(int start, int stop, int size, int* s0, int* len) {
    if (start > size) start = size;
    if (stop < 0) {
        stop += size;
        if (stop < 0) stop = 0;
    }
    if (stop > size) stop = size;
    *s0 = start;
    *len = stop > start ? stop - start : 0;
}

// ---------------------------------------------------------------------------
// Pillow BICUBIC
// ---------------------------------------------------------------------------
PA_HD int bicubic_ksize(int in_size, int out_size) {
    double scale = (double)(float)in_size / out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(2.0 * filterscale) * 2 + 1;
}

// Pillow precompute_coeffs bounds (first tap, tap count) of output coordinate
// xx for a pass in_size -> out_size: the same arithmetic as bicubic_coef_row.
PA_HD void bicubic_bounds(int in_size, int out_size, int xx, int* xmin, int* cnt) {
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

PA_HD double bicubic_filter(double x) {
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
PA_HD_COLD void bicubic_coef_row(int in_size, int out_size, int xx, int32_t* row) {
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
PA_HD uint32_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One bicubic output value of Pillow's ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc, three channels:
// 2^21 + sum over the row's taps of u8 * coefficient (clip8 of each is the output byte). `tap` is the first tap's pixel.
// TAP_STRIDE: the bytes from one tap to the next where the taps lie along a row (3: indexed from `tap`, so that the
// compiler keeps Pillow's byte loads -- stepping a pointer made it merge them into unaligned dword loads, 7 % slower in
// crop_sized_h_kernel); 0: down a column, `pitch` bytes apart, stepping the pointer as ImagingResampleVertical does.
struct BicubicAcc {
    int a0, a1, a2;
};
template <int TAP_STRIDE>
PA_HD BicubicAcc bicubic_acc(const int32_t* row, const uint8_t* tap, size_t pitch = 0) {
    BicubicAcc r;
    r.a0 = r.a1 = r.a2 = 1 << (PRECISION_BITS - 1);
    const int cnt = row[1];
    for (int t = 0; t < cnt; ++t) {
        const int k = row[2 + t];
        const uint8_t* s = TAP_STRIDE ? tap + TAP_STRIDE * t : tap;
        r.a0 += mul24((int)s[0], k);
        r.a1 += mul24((int)s[1], k);
        r.a2 += mul24((int)s[2], k);
        if (!TAP_STRIDE) tap += pitch;
    }
    return r;
}

PA_HD void store_clip8(uint8_t* o, const BicubicAcc a) {
    o[0] = (uint8_t)clip8(a.a0);
    o[1] = (uint8_t)clip8(a.a1);
    o[2] = (uint8_t)clip8(a.a2);
}

// The two passes over plain memory, items first, first + step, ...: the multi-pass forms' bodies (a workgroup's or a
// grid's stride on the device, (0, 1) on the host).
// ImagingResampleHorizontal_8bpc: dst[y][xx][c], rows x out_w, from src rows of src_pitch bytes.
PA_HD void bicubic_pass_h(const int32_t* coef, const uint8_t* src, size_t src_pitch, int rows, int out_w, uint8_t* dst, int first, int step) {
    const int total = rows * out_w;
    for (int i = first; i < total; i += step) {
        const int y = i / out_w;
        const int xx = i - y * out_w;
        const int32_t* row = coef + (size_t)xx * COEF_ROW;
        store_clip8(dst + (size_t)i * 3, bicubic_acc<3>(row, src + (size_t)y * src_pitch + (size_t)row[0] * 3));
    }
}

// ImagingResampleVertical_8bpc: dst[yy][x][c], out_h x w, from src rows of src_pitch bytes.
PA_HD void bicubic_pass_v(const int32_t* coef, const uint8_t* src, size_t src_pitch, int out_h, int w, uint8_t* dst, int first, int step) {
    const int total = out_h * w;
    for (int i = first; i < total; i += step) {
        const int yy = i / w;
        const int x = i - yy * w;
        const int32_t* row = coef + (size_t)yy * COEF_ROW;
        store_clip8(dst + (size_t)i * 3, bicubic_acc<0>(row, src + (size_t)row[0] * src_pitch + (size_t)x * 3, src_pitch));
    }
}

// The table of a pass in_size -> out_size, rows first, first + step, ...
PA_HD void bicubic_coef_table(int in_size, int out_size, int32_t* table, int first, int step) {
    for (int xx = first; xx < out_size; xx += step) bicubic_coef_row(in_size, out_size, xx, table + (size_t)xx * COEF_ROW);
}

// The matrix forms multiply a coefficient as three base-256 digits: k = d0 + 256 d1 + 65536 d2, d0 and d1 in [-128, 127]
// (d2 as well for every normalised coefficient, |k| < 2^23), against pixels offset to p - 128 ...
PA_HD void coef_digits(int k, int* d0, int* d1, int* d2) {
    *d0 = (int)(int8_t)(k & 0xff);
    const int k1 = (k - *d0) >> 8;
    *d1 = (int)(int8_t)(k1 & 0xff);
    *d2 = (k1 - *d1) >> 8;
}

// ... so the exact sum Pillow accumulates is D_0 + (D_1 << 8) + (D_2 << 16) + this constant of the output coordinate:
// 2^21 + 128 * sum(k) over the (at most 7) taps the forms take.
PA_HD int coef_row_constant(const int32_t* row) {
    const int cnt = row[1];
    int ksum = 0;
    for (int t = 0; t < 7; ++t) ksum += t < cnt ? row[2 + t] : 0;
    return 128 * ksum + (1 << (PRECISION_BITS - 1));
}

// ---------------------------------------------------------------------------
// OpenCV INTER_AREA
// ---------------------------------------------------------------------------
// What cv::resize(INTER_AREA) does from sw x sh to ow x oh, by value (see area_alpha).
struct AreaGeom {
    int mode;  // 0 copy, 1 fast 2x2, 2 fast integer, 3 general, 4 enlarging: the 8-bit bilinear resizer with area-mode coefficients
    int iscale_x, iscale_y;
    int sw, sh, ow, oh;
    double scale_x, scale_y;
};

// The branch: copy iff the sizes are equal; else the bilinear emulation iff either axis enlarges; else the integer fast
// paths iff both scales are integers to within DBL_EPSILON (2 x 2 its own), else the general one. (crop_plan_kernel used
// to ask "enlarging" before "copy"; the orders agree, because equal sizes make both scales exactly 1.0 and a scale of 1.0
// does not enlarge: checked for S in {16, 64, 128, 200, 512} and d in 1..3999.)
PA_HD AreaGeom area_branch(int sw, int sh, int ow, int oh) {
    AreaGeom g;
    g.sw = sw; g.sh = sh; g.ow = ow; g.oh = oh;
    g.iscale_x = g.iscale_y = 1;
    const double inv_sx = (double)ow / (double)sw, inv_sy = (double)oh / (double)sh;  // dsize / ssize, as cv::resize forms them
    g.scale_x = 1.0 / inv_sx;
    g.scale_y = 1.0 / inv_sy;
    if (sw == ow && sh == oh) {
        g.mode = 0;
    } else if (g.scale_x < 1.0 || g.scale_y < 1.0) {
        g.mode = 4;
    } else {
        g.iscale_x = (int)rint(g.scale_x);  // saturate_cast<int>(double) == cvRound
        g.iscale_y = (int)rint(g.scale_y);
        const double eps = 2.220446049250313e-16;  // DBL_EPSILON
        const bool fast = fabs(g.scale_x - g.iscale_x) < eps && fabs(g.scale_y - g.iscale_y) < eps;
        g.mode = fast ? ((g.iscale_x == 2 && g.iscale_y == 2) ? 1 : 2) : 3;
    }
    return g;
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

PA_HD AreaTab area_tab(int dx, double scale, int ssize) {
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
PA_HD AreaTabPacked area_pack(const AreaTab& t) {
    AreaTabPacked q;
    q.bits = (uint32_t)t.s_first | ((uint32_t)t.n_mid << 16) | ((uint32_t)t.has_first << 24) | ((uint32_t)t.has_last << 25);
    q.a_first = t.a_first;
    q.a_mid = t.a_mid;
    q.a_last = t.a_last;
    return q;
}

// (by value, as selects of values: taking the table by reference made hipcc keep it in scratch memory and turn the
// choice into an indexed scratch load -- which gave the whole fused kernel a private segment)
PA_HD float area_alpha(const AreaTab t, int k) {
    const float a_first = t.a_first, a_mid = t.a_mid, a_last = t.a_last;
    const int hf = t.has_first, hm = t.has_first + t.n_mid;
    float r = a_last;
    r = k < hm ? a_mid : r;
    r = k < hf ? a_first : r;
    return r;
}

PA_HD int cv_saturate_u8(float v) {
    const int r = (int)rintf(v);  // cvRound: round half to even
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// The canvases of area_pixel: load(y, x, c0, c1, c2) returns a source pixel of the INTER_AREA step.
struct Canvas {  // d x d black canvas with the resized slice pasted at (px, py)
    const uint8_t* src;
    size_t pitch;
    int px, py, rw, rh;
    PA_HD void load(int y, int x, int& c0, int& c1, int& c2) const {
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

struct WhCanvas {  // plain [rows][cols][3] bytes
    const uint8_t* src;
    int pitch;
    PA_HD void load(int y, int x, int& c0, int& c1, int& c2) const {
        const uint8_t* s = src + (size_t)y * pitch + x * 3;
        c0 = s[0]; c1 = s[1]; c2 = s[2];
    }
};

// One destination pixel (dy, dx) of cv::resize INTER_AREA, g.sw x g.sh -> g.ow x g.oh (the square paths: sw = sh = d).
// Geometry and canvas by value, as area_alpha's table.
template <class CV>
PA_HD void area_pixel(const AreaGeom g, const CV cv, int dy, int dx, int& o0, int& o1, int& o2) {
    if (g.mode == 0) {
        cv.load(dy, dx, o0, o1, o2);
    } else if (g.mode == 1) {
        int s0 = 2, s1 = 2, s2 = 2;
        for (int yy = 0; yy < 2; ++yy)
            for (int xx = 0; xx < 2; ++xx) {
                int c0, c1, c2;
                cv.load(dy * 2 + yy, dx * 2 + xx, c0, c1, c2);
                s0 += c0; s1 += c1; s2 += c2;
            }
        o0 = s0 >> 2; o1 = s1 >> 2; o2 = s2 >> 2;
    } else if (g.mode == 2) {
        int s0 = 0, s1 = 0, s2 = 0;
        for (int yy = 0; yy < g.iscale_y; ++yy)
            for (int xx = 0; xx < g.iscale_x; ++xx) {
                int c0, c1, c2;
                cv.load(dy * g.iscale_y + yy, dx * g.iscale_x + xx, c0, c1, c2);
                s0 += c0; s1 += c1; s2 += c2;
            }
        const float scale = 1.f / (float)(g.iscale_x * g.iscale_y);
        o0 = cv_saturate_u8((float)s0 * scale);
        o1 = cv_saturate_u8((float)s1 * scale);
        o2 = cv_saturate_u8((float)s2 * scale);
    } else if (g.mode == 4) {
        // enlarging: cv::hal::resize runs the 8-bit bilinear resizer with area-mode coefficients
        // (s = floor(d*scale), f = (d+1) - (s+1)*inv_scale, f <= 0 ? 0 : f - floor(f); weights
        // cvRound(w * 2048)); HResizeLinear keeps 11 fraction bits, VResizeLinear computes
        // (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2. Columns whose right neighbour
        // would leave the source use S[last]*2048; rows only clip the index.
        const double inv_x = (double)g.ow / (double)g.sw, inv_y = (double)g.oh / (double)g.sh;  // dsize / ssize, as cv::resize forms them
        int sx = (int)floor((double)dx * g.scale_x);
        float fx = (float)((double)(dx + 1) - (double)(sx + 1) * inv_x);
        fx = fx <= 0.f ? 0.f : fx - floorf(fx);
        const bool plain = sx + 1 >= g.sw;
        if (sx >= g.sw - 1) {
            fx = 0.f;
            sx = g.sw - 1;
        }
        const int a0 = (int)rintf((1.f - fx) * 2048.f), a1 = (int)rintf(fx * 2048.f);
        const int sy = (int)floor((double)dy * g.scale_y);
        float fy = (float)((double)(dy + 1) - (double)(sy + 1) * inv_y);
        fy = fy <= 0.f ? 0.f : fy - floorf(fy);
        const int b0 = (int)rintf((1.f - fy) * 2048.f), b1 = (int)rintf(fy * 2048.f);
        const int r0 = sy < g.sh - 1 ? sy : g.sh - 1;
        const int r1 = sy + 1 < g.sh - 1 ? sy + 1 : g.sh - 1;
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
        const AreaTab tx = area_tab(dx, g.scale_x, g.sw);
        const AreaTab ty = area_tab(dy, g.scale_y, g.sh);
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

// The INTER_AREA step of a planned square crop: d x d canvas -> out_h x out_size
PA_HD AreaGeom area_geom(const CropPlan& pl, int out_size) {
    AreaGeom g;
    g.mode = pl.area_mode;
    g.iscale_x = pl.iscale_x; g.iscale_y = pl.iscale_y;
    g.sw = g.sh = pl.d;
    g.ow = out_size; g.oh = pl.out_h;
    g.scale_x = pl.scale_x; g.scale_y = pl.scale_y;
    return g;
}

// ---------------------------------------------------------------------------
// YoloCrop.square_crop(frame, out_size, padding) (playaid/fighter.py:323-381), decided once per crop: the geometry fields of
// a CropPlan from the normalised box b[4] on a W x H frame. t_stride / coef_dim are the caller's capacity (bytes of an
// intermediate, rows of a coefficient table). frame_ok = false: the crop's source index lies outside the frame buffer.
// fused_rb, mfma_* and h_mis stay zero and the table addresses null: crop_plan_kernel's own.
// ---------------------------------------------------------------------------
PA_HD CropPlan square_crop_plan(const double* b, int W, int H, int pad, int out_size, size_t t_stride, int coef_dim, int frame, bool frame_ok) {
    CropPlan pl;
    pl.status = PA_CROP_OK;
    pl.frame = frame;
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
    if (!frame_ok) {  // never dereferenced
        pl.frame = 0;
        pl.status = PA_CROP_BAD_FRAME;
    }
    int cx, cy, cw, ch;
    // YoloCrop.yolo_pixels (fighter.py:305-314)
    if (pl.status == PA_CROP_OK && (!to_int_checked(b[0] * W, &cx) || !to_int_checked(b[1] * H, &cy) ||
                                    !to_int_checked(b[2] * W, &cw) || !to_int_checked(b[3] * H, &ch))) {
        pl.status = PA_CROP_BAD_BOX;
    }
    if (pl.status == PA_CROP_OK) {
        const int d = cw > ch ? cw : ch;
        pl.d = d;
        if (d <= 0 || d > 16384) pl.status = PA_CROP_BAD_BOX;
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
            // ImageOps.pad(raw_crop, (d, d), color="black")
            if (pl.sh == 0 || pl.sw == 0) {
                // Pillow's contain size of a (sh x 0) slice is (0, d): equal to the source size when sh == d, so
                // ImageOps.pad skips the resize and returns the black d x d canvas (the reference's crop is all zero);
                // any other empty slice raises (ValueError -> (False, None), or ZeroDivisionError for sh == 0)
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
                    // the two kernel limits (include/playaid_hip.h): PA_KSIZE_MAX taps per pass, and intermediates / tables
                    // within the caller's capacity
                    if (pl.ksize_h > PA_KSIZE_MAX || pl.ksize_v > PA_KSIZE_MAX) pl.status = PA_CROP_FILTER_TOO_WIDE;
                    if ((size_t)pl.sh * rw * 3 > t_stride || (size_t)rh * rw * 3 > t_stride || rw > coef_dim || rh > coef_dim)
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
        const AreaGeom g = area_branch(d, d, out_size, pl.out_h);
        pl.scale_x = g.scale_x;
        pl.scale_y = g.scale_y;
        pl.iscale_x = g.iscale_x;
        pl.iscale_y = g.iscale_y;
        pl.area_mode = g.mode;
        if (pl.out_h < 1 || pl.out_h > out_size) pl.status = PA_CROP_BAD_BOX;  // (int(d * (S / d)) is S or S - 1: never taken)
    }
    return pl;
}

// ---------------------------------------------------------------------------
// The runner's own input branch (playaid/ai_runner.py:446-459), decided once per crop image of sw x sh: the INTER_AREA step
// to (128, int(h * (128 / w))) and ImageOps.pad((128, 128))'s contain size / paste offset / bicubic passes behind it.
// ---------------------------------------------------------------------------
struct RunnerInPlan {
    int status;
    AreaGeom area;       // sw x sh -> 128 x oh
    int rw, rh, px, py;  // ImageOps.pad: size after contain, paste offset (rw == 128 && rh == 128: no pad step)
    int need_h, need_v;
};

PA_HD RunnerInPlan runner_in_plan(int sw, int sh, size_t t_stride) {
    RunnerInPlan pl;
    pl.status = PA_CROP_OK;
    pl.rw = pl.rh = PA_CROP; pl.px = pl.py = 0; pl.need_h = pl.need_v = 0;
    // imutils.resize(width=128): dim = (128, int(h * (128 / float(w))))
    const double r = 128.0 / (double)sw;
    const double ohd = (double)sh * r;
    const int oh = ohd < 2.0e9 ? (int)ohd : 0;
    if (oh < 1) {  // cv2.resize raises for an empty destination
        pl.status = PA_CROP_EMPTY;
        pl.area = AreaGeom{};
        return pl;
    }
    pl.area = area_branch(sw, sh, PA_CROP, oh);
    if (oh != PA_CROP) {
        // ImageOps.pad(img 128 x oh, (128, 128)): contain keeps the aspect ratio (ImageOps.py)
        const double im_ratio = 128.0 / (double)oh;
        if (im_ratio > 1.0) {
            const int nh = (int)rint((double)oh / 128.0 * 128.0);
            if (nh != PA_CROP) pl.rh = nh;
        } else {
            const int nw = (int)rint(128.0 / (double)oh * 128.0);
            if (nw != PA_CROP) pl.rw = nw;
        }
        if (pl.rw < 1 || pl.rh < 1) pl.status = PA_CROP_EMPTY;
        pl.need_h = pl.rw != PA_CROP;
        pl.need_v = pl.rh != oh;
        if (pl.rw != PA_CROP)
            pl.px = (int)rint((double)(PA_CROP - pl.rw) * 0.5);
        else if (pl.rh != PA_CROP)
            pl.py = (int)rint((double)(PA_CROP - pl.rh) * 0.5);
        if ((pl.need_h && bicubic_ksize(PA_CROP, pl.rw) > PA_KSIZE_MAX) || (pl.need_v && bicubic_ksize(oh, pl.rh) > PA_KSIZE_MAX))
            pl.status = PA_CROP_FILTER_TOO_WIDE;
    }
    if ((size_t)(oh + (pl.need_v ? pl.rh : 0)) * PA_CROP * 3 > t_stride) pl.status = PA_CROP_FILTER_TOO_WIDE;  // scratch
    return pl;
}

// One pixel (y, x) of the runner input's last step: the vertical pass where the pad step has one, pasted on the black
// 128 x 128 canvas. cur: [.][cur_w][3] behind the horizontal pass (or INTER_AREA); coef: the vertical pass's table.
PA_HD void runner_in_pixel(const RunnerInPlan& pl, const uint8_t* cur, const int32_t* coef, int i, int& o0, int& o1, int& o2) {
    const int cur_w = pl.need_h ? pl.rw : PA_CROP;
    const int cur_h = pl.need_v ? pl.rh : pl.area.oh;
    const int y = (i >> 7) - pl.py, x = (i & 127) - pl.px;
    o0 = o1 = o2 = 0;
    if ((unsigned)y < (unsigned)cur_h && (unsigned)x < (unsigned)cur_w) {
        if (pl.need_v) {
            const int32_t* row = coef + (size_t)y * COEF_ROW;
            const BicubicAcc a = bicubic_acc<0>(row, cur + ((size_t)row[0] * cur_w + x) * 3, (size_t)cur_w * 3);
            o0 = clip8(a.a0); o1 = clip8(a.a1); o2 = clip8(a.a2);
        } else {
            const uint8_t* sp = cur + ((size_t)y * cur_w + x) * 3;
            o0 = sp[0]; o1 = sp[1]; o2 = sp[2];
        }
    }
}

}  // namespace pa

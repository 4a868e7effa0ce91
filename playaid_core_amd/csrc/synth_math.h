// The synthetic-window compositing's reference arithmetic (pa_synth_composite of include/playaid_hip.h), on
// top of crop_math.h: the size imutils.resize gives a sprite inside a square stage crop, cv::resize(INTER_AREA) of a
// four-channel image of any sw x sh (every branch area_branch distinguishes, each channel a plain channel), and Pillow's
// paste_mask_RGBA blend. crop_math.h's own functions are used as they are and none of them changes: area_branch, area_tab,
// area_pack, area_alpha and cv_saturate_u8 never assumed three channels or a square source.
//
// Host and device, no HIP includes, -ffp-contract=off for whoever compiles it: as crop_math.h.
#pragma once
#include "crop_math.h"

namespace pa {

// One image of a bank (pa_synth_bank_create): `offset` bytes behind the bank's first pixel, 16-byte aligned, rows packed.
struct SynthDesc {
    uint64_t offset;
    int32_t w, h;
};

// load_and_augment_frame_to_stage_crop (ult_action_dataset.py:120-123): imutils.resize(height=D) of a sprite taller than wide,
// imutils.resize(width=D) of any other, in double precision. Unclamped: a thin sprite's shorter side can come out 0, for
// which cv2.resize raises -- the host refuses such a (bank, D) pair (synth_dim_min).
PA_HD void synth_sprite_size_raw(int w, int h, int D, int* ow, int* oh) {
    if (h > w) {
        *ow = (int)((double)w * ((double)D / (double)h));
        *oh = D;
    } else {
        *ow = D;
        *oh = (int)((double)h * ((double)D / (double)w));
    }
}

// ... as the kernel takes it: both sides within 1..D whatever the descriptor says.
PA_HD void synth_sprite_size(int w, int h, int D, int* ow, int* oh) {
    int rw, rh;
    synth_sprite_size_raw(w, h, D, &rw, &rh);
    *ow = rw < 1 ? 1 : (rw > D ? D : rw);
    *oh = rh < 1 ? 1 : (rh > D ? D : rh);
}

// The smallest D of PA_SYNTH_DIM_MIN..PA_SYNTH_DIM_MAX at which the sprite resizes to at least 1 x 1 (every larger D does too:
// the products grow with D), or PA_SYNTH_DIM_MAX + 1 when none does. PA_SYNTH_DIM_MIN for any sprite whose longer side is at
// most 32 times the shorter.
inline int synth_dim_min(int w, int h) {
    for (int D = PA_SYNTH_DIM_MIN; D <= PA_SYNTH_DIM_MAX; ++D) {
        int ow, oh;
        synth_sprite_size_raw(w, h, D, &ow, &oh);
        if (ow >= 1 && oh >= 1) return D;
    }
    return PA_SYNTH_DIM_MAX + 1;
}

// Pillow's paste_mask_RGBA for one channel: source s over destination d through the source's alpha a (MULDIV255's form).
PA_HD int pillow_blend(int s, int d, int a) {
    const int t = s * a + d * (255 - a) + 128;
    return ((t >> 8) + t) >> 8;
}

// A packed [sh][sw] RGBA image, one pixel a little-endian dword (R in the low byte). The indices every branch below forms lie
// inside the image by construction; the clamp keeps that true for any geometry.
struct RgbaImage {
    const uint32_t* src;
    int sw, sh;
    PA_HD uint32_t load(int y, int x) const {
        y = y < sh - 1 ? y : sh - 1;
        x = x < sw - 1 ? x : sw - 1;
        return src[(size_t)y * sw + x];
    }
};

PA_HD uint32_t pack4(int c0, int c1, int c2, int c3) {
    return (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)c3 << 24);
}

// area_pack's inverse
PA_HD AreaTab area_unpack(const AreaTabPacked q) {
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

// The integer fast paths (area_branch modes 1 and 2) for destination pixel (dy, dx): area_pixel's, four channels.
template <class CV>
PA_HD uint32_t area4_box(const CV cv, int dy, int dx, int iscale_x, int iscale_y) {
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int yy = 0; yy < iscale_y; ++yy)
        for (int xx = 0; xx < iscale_x; ++xx) {
            const uint32_t p = cv.load(dy * iscale_y + yy, dx * iscale_x + xx);
            s0 += (int)(p & 0xff); s1 += (int)((p >> 8) & 0xff); s2 += (int)((p >> 16) & 0xff); s3 += (int)(p >> 24);
        }
    if (iscale_x == 2 && iscale_y == 2) return pack4((s0 + 2) >> 2, (s1 + 2) >> 2, (s2 + 2) >> 2, (s3 + 2) >> 2);
    const float scale = 1.f / (float)(iscale_x * iscale_y);
    return pack4(cv_saturate_u8((float)s0 * scale), cv_saturate_u8((float)s1 * scale), cv_saturate_u8((float)s2 * scale),
                 cv_saturate_u8((float)s3 * scale));
}

// The general path (mode 3) from the two axes' table entries: the horizontal sum in table order, multiply then add, then the
// vertical one, then cvRound and saturate -- area_pixel's order, which is oracle.resample.cv_resize_area's.
template <class CV>
PA_HD uint32_t area4_general(const AreaTab tx, const AreaTab ty, const CV cv) {
    float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f, sum3 = 0.f;
    for (int j = 0; j < ty.n; ++j) {
        const float beta = area_alpha(ty, j);
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
        for (int k = 0; k < tx.n; ++k) {
            const float alpha = area_alpha(tx, k);
            const uint32_t p = cv.load(ty.s_first + j, tx.s_first + k);
            b0 = b0 + (float)(p & 0xff) * alpha;
            b1 = b1 + (float)((p >> 8) & 0xff) * alpha;
            b2 = b2 + (float)((p >> 16) & 0xff) * alpha;
            b3 = b3 + (float)(p >> 24) * alpha;
        }
        sum0 = sum0 + beta * b0;
        sum1 = sum1 + beta * b1;
        sum2 = sum2 + beta * b2;
        sum3 = sum3 + beta * b3;
    }
    return pack4(cv_saturate_u8(sum0), cv_saturate_u8(sum1), cv_saturate_u8(sum2), cv_saturate_u8(sum3));
}

// One axis of the enlarging path (mode 4: the 8-bit bilinear resizer with area-mode coefficients), as area_pixel states it:
// along x, s0 is the left column, (w0, w1) its and its right neighbour's 11-bit weights, plain = the neighbour would leave the
// source (the column counts 2048); along y, (s0, s1) are the two clipped rows and the weights are not zeroed at the edge.
struct LinTab {
    int s0, s1, w0, w1, plain;
};

PA_HD LinTab area_lin_x(int dx, const AreaGeom g) {
    LinTab t;
    const double inv_x = (double)g.ow / (double)g.sw;
    int sx = (int)floor((double)dx * g.scale_x);
    float fx = (float)((double)(dx + 1) - (double)(sx + 1) * inv_x);
    fx = fx <= 0.f ? 0.f : fx - floorf(fx);
    t.plain = sx + 1 >= g.sw ? 1 : 0;
    if (sx >= g.sw - 1) {
        fx = 0.f;
        sx = g.sw - 1;
    }
    t.s0 = sx < 0 ? 0 : sx;
    t.s1 = t.s0;
    t.w0 = (int)rintf((1.f - fx) * 2048.f);
    t.w1 = (int)rintf(fx * 2048.f);
    return t;
}

PA_HD LinTab area_lin_y(int dy, const AreaGeom g) {
    LinTab t;
    const double inv_y = (double)g.oh / (double)g.sh;
    const int sy = (int)floor((double)dy * g.scale_y);
    float fy = (float)((double)(dy + 1) - (double)(sy + 1) * inv_y);
    fy = fy <= 0.f ? 0.f : fy - floorf(fy);
    t.w0 = (int)rintf((1.f - fy) * 2048.f);
    t.w1 = (int)rintf(fy * 2048.f);
    const int r0 = sy < g.sh - 1 ? sy : g.sh - 1;
    const int r1 = sy + 1 < g.sh - 1 ? sy + 1 : g.sh - 1;
    t.s0 = r0 < 0 ? 0 : r0;
    t.s1 = r1 < 0 ? 0 : r1;
    t.plain = 0;
    return t;
}

// A LinTab in the 16 bytes of an AreaTabPacked (indices < 2^15, weights 0..2048: exact as floats)
PA_HD AreaTabPacked lin_pack(const LinTab t) {
    AreaTabPacked q;
    q.bits = (uint32_t)t.s0 | ((uint32_t)t.s1 << 16) | ((uint32_t)t.plain << 31);
    q.a_first = (float)t.w0;
    q.a_mid = (float)t.w1;
    q.a_last = 0.f;
    return q;
}

PA_HD LinTab lin_unpack(const AreaTabPacked q) {
    LinTab t;
    t.s0 = (int)(q.bits & 0xffff);
    t.s1 = (int)((q.bits >> 16) & 0x7fff);
    t.plain = (int)(q.bits >> 31);
    t.w0 = (int)q.a_first;
    t.w1 = (int)q.a_mid;
    return t;
}

PA_HD int lin_value(int c0, int e0, int c1, int e1, const LinTab tx, const LinTab ty) {
    const int h0 = tx.plain ? c0 * 2048 : c0 * tx.w0 + e0 * tx.w1;
    const int h1 = tx.plain ? c1 * 2048 : c1 * tx.w0 + e1 * tx.w1;
    return ((((ty.w0 * (h0 >> 4)) >> 16) + ((ty.w1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xff;
}

template <class CV>
PA_HD uint32_t area4_linear(const LinTab tx, const LinTab ty, const CV cv) {
    const uint32_t p0 = cv.load(ty.s0, tx.s0), p1 = cv.load(ty.s1, tx.s0);
    const uint32_t q0 = tx.plain ? 0u : cv.load(ty.s0, tx.s0 + 1), q1 = tx.plain ? 0u : cv.load(ty.s1, tx.s0 + 1);
    return pack4(lin_value((int)(p0 & 0xff), (int)(q0 & 0xff), (int)(p1 & 0xff), (int)(q1 & 0xff), tx, ty),
                 lin_value((int)((p0 >> 8) & 0xff), (int)((q0 >> 8) & 0xff), (int)((p1 >> 8) & 0xff), (int)((q1 >> 8) & 0xff), tx, ty),
                 lin_value((int)((p0 >> 16) & 0xff), (int)((q0 >> 16) & 0xff), (int)((p1 >> 16) & 0xff), (int)((q1 >> 16) & 0xff), tx, ty),
                 lin_value((int)(p0 >> 24), (int)(q0 >> 24), (int)(p1 >> 24), (int)(q1 >> 24), tx, ty));
}

}  // namespace pa

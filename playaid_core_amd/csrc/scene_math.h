// The reference arithmetic of the detector's synthetic training images (pa_sprite_resize and pa_scene_composite of
// include/playaid_hip.h), on top of crop_math.h and synth_math.h, whose functions are used as they are:
// bicubic_ksize, bicubic_filter, clip8, mul24, pillow_blend, pack4, SynthDesc. What is new here: how a record of either call is
// read (the clamps, shared by the kernels and the host's descriptor writer), one row of Pillow's coefficient table with as
// many taps as the pass has (crop_math.h's bicubic_coef_row stops at PA_KSIZE_MAX = 15; a 1024-wide render going to width 50
// has 83), Pillow's RGBA <-> RGBa conversions, and the byte geometry of a scene.
//
// Host and device, no HIP includes, -ffp-contract=off for whoever compiles it: as crop_math.h.
#pragma once
#include "synth_math.h"

namespace pa {

PA_HD int scene_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- pa_sprite_resize -------------------------------------------------------------------------------------------------------------

// A record as the kernel reads it: src inside the bank, the size inside the output bank's slots (max_w <= PA_SPRITE_RESIZE_W_MAX,
// max_h <= PA_SPRITE_RESIZE_H_MAX: pa_sprite_resize_bank_create).
struct ResizeRead {
    int src, ow, oh;
};

PA_HD ResizeRead resize_read(const pa_sprite_resize_params p, int n_sprites, int max_w, int max_h) {
    ResizeRead r;
    r.src = scene_clampi(p.src, 0, n_sprites - 1);
    r.ow = scene_clampi(p.out_w, 1, max_w);
    r.oh = scene_clampi(p.out_h, 1, max_h);
    return r;
}

// The taps one row of a pass in_size -> out_size is given room for: Pillow's ksize (its own allocation per row, so no row has
// more), and no more than the source has pixels. out_size * resize_row_taps never exceeds PA_SPRITE_RESIZE_COEFS for in_size
// <= PA_SYNTH_SPRITE_MAX and out_size <= PA_SPRITE_RESIZE_H_MAX: ksize <= 4 in / out + 3 for a shrinking pass, 5 otherwise.
PA_HD int resize_row_taps(int in_size, int out_size) {
    const int k = bicubic_ksize(in_size, out_size);
    return k < in_size ? k : in_size;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output coordinate xx of a BICUBIC pass in_size -> out_size, any number
// of taps: bicubic_coef_row's arithmetic (the weights summed in tap order in double precision, each divided by the sum, scaled
// by 2^22 and rounded half away from zero) with the taps written to k[0 .. *cnt - 1]. `room` = resize_row_taps(in_size,
// out_size) bounds *cnt and changes no value.
PA_HD_COLD void resize_coef_row(int in_size, int out_size, int xx, int room, int* first, int* cnt, int32_t* k) {
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
    if (xmax > room) xmax = room;
    if (xmax < 0) xmax = 0;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double v = bicubic_filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) v = v / ww;
        k[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << PRECISION_BITS)) : (int)(0.5 + v * (double)(1 << PRECISION_BITS));
    }
    *first = xmin;
    *cnt = xmax;
}

// Pillow's MULDIV255
PA_HD int scene_muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// Pillow's rgbA2rgba: a pixel to premultiplied alpha (alpha kept)
PA_HD uint32_t rgba_premultiply(uint32_t p) {
    const int al = (int)(p >> 24);
    return pack4(scene_muldiv255((int)(p & 0xff), al), scene_muldiv255((int)((p >> 8) & 0xff), al), scene_muldiv255((int)((p >> 16) & 0xff), al), al);
}

// Pillow's rgba2rgbA for one channel: alpha 0 or 255 leaves it, else min(255, 255 * c / a), integer division
PA_HD int rgba_unpremultiply(int c, int al) {
    if (al == 0 || al == 255) return c;
    const int v = 255 * c / al;
    return v > 255 ? 255 : v;
}

// ---- pa_scene_composite -----------------------------------------------------------------------------------------------------------

constexpr int SCENE_SPRITE = 128;   // the side of a pa_sprite_bank_create slot

// A record as the kernel reads it
struct SceneRead {
    int stage, n;
    int slot[PA_SCENE_SPRITES_MAX], x[PA_SCENE_SPRITES_MAX], y[PA_SCENE_SPRITES_MAX];
};

PA_HD SceneRead scene_read(const pa_scene_params& p, int n_slots, int n_stages) {
    SceneRead r;
    r.stage = scene_clampi(p.stage, 0, n_stages - 1);
    r.n = scene_clampi(p.n_sprites, 0, PA_SCENE_SPRITES_MAX);
    for (int k = 0; k < PA_SCENE_SPRITES_MAX; ++k) {
        r.slot[k] = scene_clampi(p.sprites[k].slot, 0, n_slots - 1);
        r.x[k] = scene_clampi(p.sprites[k].x, -PA_SYNTH_PASTE_MAX, PA_SYNTH_PASTE_MAX);
        r.y[k] = scene_clampi(p.sprites[k].y, -PA_SYNTH_PASTE_MAX, PA_SYNTH_PASTE_MAX);
    }
    return r;
}

// The bytes a W x H scene takes in the output buffer: its packed rows, rounded up to 16 so that every scene starts on a
// 16-byte boundary (a stage image of a bank is padded the same way).
PA_HD uint64_t scene_bytes_padded(int w, int h) { return ((uint64_t)w * (uint64_t)h * 3u + 15u) & ~(uint64_t)15; }

}  // namespace pa

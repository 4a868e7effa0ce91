// The arithmetic of the albumentations stages that augment.hip (128 x 128 RGB crops, pa_augment_crops) and sprite_augment.hip
// (C x C RGBA canvases, pa_sprite_augment) both run, once each: how a float of a parameter block is read, the crop's four
// 256-byte tables, the box blur's rounding, OpenCV's 8-bit RGB -> HSV -> tables -> RGB, the noise deviate and the two stream
// keys. include/playaid_hip.h states every formula; augment.augment_reference is the numpy twin of all of them.
//
// Device code (the includer is compiled by hipcc with -ffp-contract=off: the fp32 stages must not have their multiplies and
// adds fused). Needs pa_kernels.h (AugmentTables) and train_common.h (hash_mix, hash_element) in scope.
#pragma once
#include "pa_kernels.h"
#include "train_common.h"

namespace pa {

// a float of the parameter block as the kernels use it: its identity value when it is not finite, else clamped
__host__ __device__ __forceinline__ float aug_sane(float x, float ident, float lo, float hi) {
    if (!(fabsf(x) <= 3.4028235e38f)) return ident;
    return fminf(fmaxf(x, lo), hi);
}

__device__ __forceinline__ uint8_t aug_byte(float t) {   // trunc(clip(t, 0, 255))
    return (uint8_t)(int)fminf(fmaxf(t, 0.f), 255.f);
}

__device__ __forceinline__ int aug_reflect(int i, int size) {   // BORDER_REFLECT_101 on 0..size - 1, for i in -1..size
    return i < 0 ? -i : (i > size - 1 ? 2 * (size - 1) - i : i);
}

// entry k of the four tables: brightness / contrast (fp32), hue, saturation, value (fp64)
__device__ __forceinline__ void aug_lut_entry(int k, float alpha, float beta, float hue, float sat, float val, uint8_t* lut_bc,
                                              uint8_t* lut_h, uint8_t* lut_s, uint8_t* lut_v) {
    const float bo = beta * 255.f;
    lut_bc[k] = aug_byte((float)k * alpha + bo);
    const double t = (double)k + (double)hue;
    double r = t - floor(t * (1.0 / 180.0)) * 180.0;   // (k + shift) mod 180 in [0, 180): the quotient may be one off, the two
    if (r < 0.0) r += 180.0;                            // corrections are exact
    if (r >= 180.0) r -= 180.0;
    lut_h[k] = (uint8_t)(int)r;
    lut_s[k] = (uint8_t)(int)fmin(fmax((double)k + (double)sat, 0.0), 255.0);
    lut_v[k] = (uint8_t)(int)fmin(fmax((double)k + (double)val, 0.0), 255.0);
}

// the box sum s of a blur x blur window as a byte
__device__ __forceinline__ int aug_blur_round(int s, int blur) {
    if (blur == 2) {   // s / 4 to nearest, ties to even
        const int q = s >> 2, rem = s & 3;
        return q + ((rem == 3 || (rem == 2 && (q & 1))) ? 1 : 0);
    }
    return (2 * s + 9) / 18;   // s / 9 to nearest (no ties: 9 is odd)
}

// c[0..2] = (r, g, b) through OpenCV's 8-bit HSV and the three tables, in place
__device__ __forceinline__ void aug_hsv_pixel(int* c, const AugmentTables& tabs, const uint8_t* lut_h, const uint8_t* lut_s,
                                              const uint8_t* lut_v) {
    const int r = c[0], g = c[1], b = c[2];
    const int vmax = max(r, max(g, b)), vmin = min(r, min(g, b));
    const int diff = vmax - vmin;
    const int vr = vmax == r ? -1 : 0, vg = vmax == g ? -1 : 0;
    const int s8 = ((diff * tabs.sdiv[vmax] + (1 << 11)) >> 12) & 255;
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + (~vg & (r - g + 4 * diff))));
    h = (h * tabs.hdiv[diff] + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    h = min(max(h, 0), 255);
    const int H = lut_h[h], S = lut_s[s8], V = lut_v[vmax];
    const float vf = (float)V * (1.f / 255.f), sf = (float)S * (1.f / 255.f);
    float rf = vf, gf = vf, bf = vf;
    if (S != 0) {
        float hf = (float)H * (6.f / 180.f);
        int sector = (int)hf;   // hf >= 0: the floor
        hf -= (float)sector;
        if ((unsigned)sector >= 6u) {
            sector = 0;
            hf = 0.f;
        }
        const float t1 = vf * (1.f - sf);
        const float t2 = vf * (1.f - sf * hf);
        const float t3 = vf * (1.f - sf * (1.f - hf));
        // OpenCV's sector table, (b, g, r) of tab[] = {v, t1, t2, t3}: {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
        switch (sector) {
            case 0: bf = t1; gf = t3; rf = vf; break;
            case 1: bf = t1; gf = vf; rf = t2; break;
            case 2: bf = t3; gf = vf; rf = t1; break;
            case 3: bf = vf; gf = t2; rf = t1; break;
            case 4: bf = vf; gf = t1; rf = t3; break;
            default: bf = t2; gf = t1; rf = vf; break;
        }
    }
    c[0] = (int)fminf(fmaxf(rintf(rf * 255.f), 0.f), 255.f);
    c[1] = (int)fminf(fmaxf(rintf(gf * 255.f), 0.f), 255.f);
    c[2] = (int)fminf(fmaxf(rintf(bf * 255.f), 0.f), 255.f);
}

// byte + sigma * z, z the normal deviate of element i of the noise stream
__device__ __forceinline__ int aug_noise_byte(int byte, float sigma, uint32_t k_noise, uint32_t i, const float* q) {
    const uint32_t r = hash_element(k_noise, i);
    const int cell = (int)(r >> 22);
    const float f = (float)(r & 0x3fffffu) * (1.f / 4194304.f);
    const float q0 = q[cell];
    const float z = q0 + f * (q[cell + 1] - q0);
    return aug_byte((float)byte + sigma * z);
}

// the 32-bit keys of a record's noise (stream 0) and pixel-dropout (stream 1) streams
__device__ __forceinline__ void aug_stream_keys(uint64_t key, uint32_t* k_noise, uint32_t* k_drop) {
    uint32_t k0 = hash_mix((uint32_t)key + 0x9e3779b9u);
    k0 = hash_mix(k0 ^ (uint32_t)(key >> 32));
    *k_noise = hash_mix(k0 ^ (1u * 0x85ebca6bu));
    *k_drop = hash_mix(k0 ^ (2u * 0x85ebca6bu));
}

}  // namespace pa

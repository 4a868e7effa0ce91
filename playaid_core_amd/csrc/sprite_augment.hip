// The reference's augmentation of a character render before it is pasted over a stage crop, augment_synth_char_crop
// (dataset_utils.py:255-378), from a sprite bank into a sprite bank: pa_sprite_augment of include/playaid_hip.h, which states the
// arithmetic of every step; DESIGN.md 5.16. sprite_augment.augment_sprites_reference is the numpy twin and the contract: this
// file and the twin give the same bytes.
//
// One launch, at most SPRITE_WORKGROUPS_MAX workgroups of 512 threads; a workgroup takes output sprites blockIdx.x,
// blockIdx.x + gridDim.x, ... and runs each one's steps as phases over its own scratch in memory, a barrier between two:
//   0  thread 0 reads the descriptor and decides the geometry (runner_in_plan of crop_math.h: the same imutils.resize and
//      ImageOps.pad the runner's input takes); the record, the constant tables and the record's four byte tables go to LDS
//   1  INTER_AREA, h x w -> 128 x h1, four channels (synth_math.h), per-axis tables in LDS                      -> R0
//   2  ImageOps.pad: a copy at a row offset, or for h1 > 128 Pillow's premultiplied BICUBIC -- horizontal pass  -> R1,
//      vertical pass, un-premultiply and paste                                                                   -> R2 (128 x 128)
//   3  with a shrink: INTER_AREA 128 -> new_scale inside a transparent border                                    -> R1 (C x C)
//   4  the Compose per output pixel (augment_math.h), image and mask each through its own gather                 -> the slot, or R0
//   5  with C > 128 and no sized crop: INTER_AREA C -> 128                                                       -> the slot
// The 128 x h1 intermediate (up to 224 KB) is why the phases go through memory and not LDS; a workgroup reads only what it
// wrote itself, behind a barrier, on its own compute unit's cache.
//
// Memory safety for ANY parameter bytes: src is clamped into the bank, new_scale outside 96..127 is 0 (so C is 128..160), map
// entries are clamped to C - 1, n_holes to 0..2 and hole tests are comparisons (no address is formed from a hole), every table
// index is a byte; every source coordinate of a resample is clamped into its image where the address is formed. The
// descriptors are the library's own, and the host refuses a bank with a render whose h1 is outside 1..PA_SPRITE_H1_MAX; a
// workgroup that met one all the same writes a transparent slot. Compiled with -ffp-contract=off.
#include "augment_math.h"
#include "synth_math.h"

namespace pa {
namespace {

constexpr int SPA_THREADS = 512;
constexpr int SPA_CMAX = PA_SPRITE_CANVAS_MAX;

struct SpaPlan {
    const uint32_t* src;
    RunnerInPlan in;   // area: w x h -> 128 x h1; (rw, rh) after contain, (px, py) the paste, need_h / need_v the bicubic passes
    int ok;
    int ns, C, O;
    AreaGeom shrink, fin;
};

struct alignas(16) SpaLds {
    AugmentTables tabs;
    pa_sprite_aug_params prm;
    uint8_t lut_bc[256], lut_h[256], lut_s[256], lut_v[256];
    SpaPlan plan;
    AreaTabPacked xt[SPA_CMAX], yt[PA_SPRITE_H1_MAX];
    int32_t coef_h[128 * COEF_ROW], coef_v[128 * COEF_ROW];
};
static_assert(sizeof(SpaLds) <= 64 * 1024, "one workgroup's LDS");
static_assert(sizeof(pa_sprite_aug_params) == 712 && sizeof(AugmentTables) % 4 == 0, "copied in words");
static_assert(SPRITE_SCRATCH_R0 >= (size_t)SPA_CMAX * SPA_CMAX * 4 && SPRITE_SCRATCH_R1 >= (size_t)SPA_CMAX * SPA_CMAX * 4, "C x C canvases");

__device__ __forceinline__ int muldiv255(int a, int b) {   // Pillow's MULDIV255
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// clip8 for the bytes this file packs into a dword. Left to itself hipcc 7 fuses two clip8s and the packing into one
// v_ashr_pk_u8_i32 and then treats the upper half of its destination as zero, while on gfx950 that half keeps what the register
// held (the accumulator): byte 2 of the pixel came out as byte 2 of 2^21 + sum. (crop_math.h's clip8 met the same family of
// packing; its callers store single bytes.) The empty statement hides the value from that combine and emits nothing.
__device__ __forceinline__ int spa_clip8(int acc) {
    int v = (int)clip8(acc);
    asm volatile("" : "+v"(v));
    return v;
}

// the per-axis tables of an INTER_AREA step (modes 3 and 4 read them)
__device__ __forceinline__ void spa_tables(const AreaGeom g, AreaTabPacked* xt, AreaTabPacked* yt, int tid) {
    if (g.mode == 3) {
        for (int i = tid; i < g.ow + g.oh; i += SPA_THREADS) {
            if (i < g.ow)
                xt[i] = area_pack(area_tab(i, g.scale_x, g.sw));
            else
                yt[i - g.ow] = area_pack(area_tab(i - g.ow, g.scale_y, g.sh));
        }
    } else if (g.mode == 4) {
        for (int i = tid; i < g.ow + g.oh; i += SPA_THREADS) {
            if (i < g.ow)
                xt[i] = lin_pack(area_lin_x(i, g));
            else
                yt[i - g.ow] = lin_pack(area_lin_y(i - g.ow, g));
        }
    }
}

__device__ __forceinline__ uint32_t spa_area_pixel(const AreaGeom g, const AreaTabPacked* xt, const AreaTabPacked* yt, const RgbaImage img,
                                                   int y, int x) {
    if (g.mode == 0) return img.load(y, x);
    if (g.mode == 1 || g.mode == 2) return area4_box(img, y, x, g.iscale_x, g.iscale_y);
    if (g.mode == 3) return area4_general(area_unpack(xt[x]), area_unpack(yt[y]), img);
    return area4_linear(lin_unpack(xt[x]), lin_unpack(yt[y]), img);
}

__global__ __launch_bounds__(SPA_THREADS) void sprite_augment_kernel(const SpriteAugArgs a) {
    __shared__ SpaLds L;
    const int tid = threadIdx.x;
    uint8_t* scratch = a.scratch + (size_t)blockIdx.x * SPRITE_SCRATCH_BYTES;
    uint32_t* R0 = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* R1 = reinterpret_cast<uint32_t*>(scratch + SPRITE_SCRATCH_R0);
    uint32_t* R2 = reinterpret_cast<uint32_t*>(scratch + SPRITE_SCRATCH_R0 + SPRITE_SCRATCH_R1);
    {
        const uint32_t* g = reinterpret_cast<const uint32_t*>(a.tabs);
        uint32_t* d = reinterpret_cast<uint32_t*>(&L.tabs);
        for (int i = tid; i < (int)(sizeof(AugmentTables) / 4); i += SPA_THREADS) d[i] = g[i];
    }
    for (int sprite = blockIdx.x; sprite < a.n; sprite += gridDim.x) {
        uint32_t* slot = reinterpret_cast<uint32_t*>(a.out_px + (size_t)sprite * (128 * 128 * 4));
        __syncthreads();   // (the previous sprite's readers of L are done)
        {
            const uint32_t* gp = reinterpret_cast<const uint32_t*>(a.params + sprite);
            uint32_t* dp = reinterpret_cast<uint32_t*>(&L.prm);
            if (tid < (int)(sizeof(pa_sprite_aug_params) / 4)) dp[tid] = gp[tid];
        }
        __syncthreads();
        // ---- phase 0 ----
        if (tid == 0) {
            const SynthDesc sd = a.sprite_desc[min(max(L.prm.src, 0), a.n_sprites - 1)];
            SpaPlan p;
            p.src = reinterpret_cast<const uint32_t*>(a.sprite_px + sd.offset);
            p.in = runner_in_plan(sd.w, sd.h, (size_t)1 << 30);
            p.ok = p.in.status == PA_CROP_OK && p.in.area.oh >= 1 && p.in.area.oh <= PA_SPRITE_H1_MAX;
            p.ns = (L.prm.new_scale >= 96 && L.prm.new_scale <= 127) ? L.prm.new_scale : 0;
            p.C = p.ns ? 256 - p.ns : 128;
            p.O = L.prm.sized_crop != 0 ? 128 : p.C;
            p.shrink = area_branch(128, 128, p.ns ? p.ns : 128, p.ns ? p.ns : 128);
            p.fin = area_branch(p.C, p.C, 128, 128);
            L.plan = p;
        }
        const float alpha = aug_sane(L.prm.alpha, 1.f, 0.f, 4.f);
        const float beta = aug_sane(L.prm.beta, 0.f, -2.f, 2.f);
        const float hue = aug_sane(L.prm.hue_shift, 0.f, -1024.f, 1024.f);
        const float sat = aug_sane(L.prm.sat_shift, 0.f, -512.f, 512.f);
        const float val = aug_sane(L.prm.val_shift, 0.f, -512.f, 512.f);
        const float sigma = aug_sane(L.prm.noise_sigma, 0.f, 0.f, 256.f);
        const bool flip = L.prm.flip != 0;
        const int blur = (L.prm.blur_k == 2 || L.prm.blur_k == 3) ? L.prm.blur_k : 0;
        const bool hsv_on = hue != 0.f || sat != 0.f || val != 0.f;
        const uint32_t thr = L.prm.pixel_drop_thr;
        const int n_holes = min(max(L.prm.n_holes, 0), 2);
        const int cmask = L.prm.channel_mask & 7;
        uint32_t k_noise, k_drop;
        aug_stream_keys(L.prm.key, &k_noise, &k_drop);
        if (tid < 256) aug_lut_entry(tid, alpha, beta, hue, sat, val, L.lut_bc, L.lut_h, L.lut_s, L.lut_v);
        __syncthreads();
        if (!L.plan.ok) {   // (refused on the host: never launched)
            for (int i = tid; i < 128 * 128; i += SPA_THREADS) slot[i] = 0u;
            continue;
        }
        const RunnerInPlan in = L.plan.in;
        const int h1 = in.area.oh;
        const int ns = L.plan.ns, C = L.plan.C, O = L.plan.O;

        // ---- phase 1: INTER_AREA to 128 x h1 ----
        spa_tables(in.area, L.xt, L.yt, tid);
        __syncthreads();
        {
            const RgbaImage img = {L.plan.src, in.area.sw, in.area.sh};
            for (int i = tid; i < 128 * h1; i += SPA_THREADS) R0[i] = spa_area_pixel(in.area, L.xt, L.yt, img, i >> 7, i & 127);
        }
        __syncthreads();

        // ---- phase 2: ImageOps.pad to 128 x 128 ----
        if (in.need_h) {   // h1 > 128: both passes
            const int rw = in.rw;
            for (int i = tid; i < rw + 128; i += SPA_THREADS) {
                if (i < rw)
                    bicubic_coef_row(128, rw, i, L.coef_h + i * COEF_ROW);
                else
                    bicubic_coef_row(h1, 128, i - rw, L.coef_v + (i - rw) * COEF_ROW);
            }
            __syncthreads();
            for (int i = tid; i < h1 * rw; i += SPA_THREADS) {
                const int y = i / rw, xx = i - y * rw;
                const int32_t* row = L.coef_h + xx * COEF_ROW;
                const int first = min(max(row[0], 0), 127), cnt = min(max(row[1], 0), PA_KSIZE_MAX);
                int a0, a1, a2, a3;
                a0 = a1 = a2 = a3 = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t p = R0[y * 128 + min(first + t, 127)];
                    const int al = (int)(p >> 24), k = row[2 + t];
                    a0 += mul24(muldiv255((int)(p & 0xff), al), k);
                    a1 += mul24(muldiv255((int)((p >> 8) & 0xff), al), k);
                    a2 += mul24(muldiv255((int)((p >> 16) & 0xff), al), k);
                    a3 += mul24(al, k);
                }
                R1[i] = pack4(spa_clip8(a0), spa_clip8(a1), spa_clip8(a2), spa_clip8(a3));
            }
            __syncthreads();
            for (int i = tid; i < 128 * 128; i += SPA_THREADS) {
                const int y = i >> 7, x = (i & 127) - in.px;
                uint32_t o = 0u;
                if ((unsigned)x < (unsigned)rw) {
                    const int32_t* row = L.coef_v + y * COEF_ROW;
                    const int first = min(max(row[0], 0), h1 - 1), cnt = min(max(row[1], 0), PA_KSIZE_MAX);
                    int a0, a1, a2, a3;
                    a0 = a1 = a2 = a3 = 1 << (PRECISION_BITS - 1);
                    for (int t = 0; t < cnt; ++t) {
                        const uint32_t p = R1[min(first + t, h1 - 1) * rw + x];
                        const int k = row[2 + t];
                        a0 += mul24((int)(p & 0xff), k);
                        a1 += mul24((int)((p >> 8) & 0xff), k);
                        a2 += mul24((int)((p >> 16) & 0xff), k);
                        a3 += mul24((int)(p >> 24), k);
                    }
                    int c0 = spa_clip8(a0), c1 = spa_clip8(a1), c2 = spa_clip8(a2);
                    const int al = spa_clip8(a3);
                    if (al != 0 && al != 255) {   // Pillow's rgba2rgbA
                        c0 = min(255 * c0 / al, 255);
                        c1 = min(255 * c1 / al, 255);
                        c2 = min(255 * c2 / al, 255);
                    }
                    o = pack4(c0, c1, c2, al);
                }
                R2[i] = o;
            }
        } else {
            for (int i = tid; i < 128 * 128; i += SPA_THREADS) {
                const int y = (i >> 7) - in.py;
                R2[i] = (unsigned)y < (unsigned)h1 ? R0[y * 128 + (i & 127)] : 0u;
            }
        }
        __syncthreads();

        // ---- phase 3: the shrink, inside its border ----
        const uint32_t* canvas = R2;
        if (ns) {
            const AreaGeom g = L.plan.shrink;
            spa_tables(g, L.xt, L.yt, tid);
            __syncthreads();
            const RgbaImage img = {R2, 128, 128};
            const int b = 128 - ns;
            for (int i = tid; i < C * C; i += SPA_THREADS) {
                const int y = i / C, x = i - y * C;
                const int ly = y - b, lx = x - b;
                R1[i] = ((unsigned)ly < (unsigned)ns && (unsigned)lx < (unsigned)ns) ? spa_area_pixel(g, L.xt, L.yt, img, ly, lx) : 0u;
            }
            canvas = R1;
            __syncthreads();
        }

        // ---- phase 4: the Compose ----
        {
            uint32_t* dst = O == 128 ? slot : R0;
            const int S = min(96, C / 3);
            for (int i = tid; i < O * O; i += SPA_THREADS) {
                const int y = i / O, x = i - y * O;
                const int u = min((int)L.prm.xmap[x], C - 1), v = min((int)L.prm.ymap[y], C - 1);
                int c[3];
                if (blur == 0) {
                    const uint32_t p = canvas[v * C + (flip ? C - 1 - u : u)];
                    c[0] = L.lut_bc[p & 0xff]; c[1] = L.lut_bc[(p >> 8) & 0xff]; c[2] = L.lut_bc[(p >> 16) & 0xff];
                } else {
                    int s0 = 0, s1 = 0, s2 = 0;
                    for (int dy = 0; dy < blur; ++dy) {
                        const int vy = aug_reflect(v - 1 + dy, C);
                        for (int dx = 0; dx < blur; ++dx) {
                            const int ux = aug_reflect(u - 1 + dx, C);
                            const uint32_t p = canvas[vy * C + (flip ? C - 1 - ux : ux)];
                            s0 += L.lut_bc[p & 0xff]; s1 += L.lut_bc[(p >> 8) & 0xff]; s2 += L.lut_bc[(p >> 16) & 0xff];
                        }
                    }
                    c[0] = aug_blur_round(s0, blur); c[1] = aug_blur_round(s1, blur); c[2] = aug_blur_round(s2, blur);
                }
                if (hsv_on) aug_hsv_pixel(c, L.tabs, L.lut_h, L.lut_s, L.lut_v);
                const uint32_t pos = (uint32_t)(v * C + u);
                if (sigma > 0.f) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k] = aug_noise_byte(c[k], sigma, k_noise, pos * 3u + (uint32_t)k, L.tabs.q);
                }
                const int ua = min((int)L.prm.axmap[x], C - 1), va = min((int)L.prm.aymap[y], C - 1);
                bool zero = thr != 0u && hash_element(k_drop, pos) < thr;
                bool zero_a = thr != 0u && hash_element(k_drop, (uint32_t)(va * C + ua)) < thr;
                for (int hole = 0; hole < n_holes; ++hole) {
                    const int hx = (int)L.prm.holes[2 * hole], hy = (int)L.prm.holes[2 * hole + 1];
                    zero = zero || ((unsigned)(u - hx) < (unsigned)S && (unsigned)(v - hy) < (unsigned)S);
                    zero_a = zero_a || ((unsigned)(ua - hx) < (unsigned)S && (unsigned)(va - hy) < (unsigned)S);
                }
                const int al = zero_a ? 0 : (int)(canvas[va * C + (flip ? C - 1 - ua : ua)] >> 24);
                dst[i] = pack4((zero || (cmask & 1)) ? 0 : c[0], (zero || (cmask & 2)) ? 0 : c[1], (zero || (cmask & 4)) ? 0 : c[2], al);
            }
        }

        // ---- phase 5: back to 128 ----
        if (O != 128) {
            const AreaGeom g = L.plan.fin;
            spa_tables(g, L.xt, L.yt, tid);
            __syncthreads();
            const RgbaImage img = {R0, C, C};
            for (int i = tid; i < 128 * 128; i += SPA_THREADS) slot[i] = spa_area_pixel(g, L.xt, L.yt, img, i >> 7, i & 127);
        }
    }
}

}  // namespace

hipError_t launch_sprite_augment(const SpriteAugArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sprite_augment_kernel, dim3((unsigned)a.workgroups), dim3(SPA_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace pa

// Pillow's Image.resize((out_w, out_h)) of an RGBA character render, as composite_chars_onto_stage
// (gen_synth_char_detection.py:216-219) calls it before augment_synth_char_crop, from a sprite bank into a sprite bank:
// pa_sprite_resize of include/playaid_hip.h, which states the arithmetic; DESIGN.md 5.17.
// detect_composite.resize_sprites_reference is the numpy twin and the contract: this file and the twin give the same bytes.
//
// One launch, at most RESIZE_WORKGROUPS_MAX workgroups of 512 threads; a workgroup takes outputs blockIdx.x,
// blockIdx.x + gridDim.x, ... and runs each one's passes as phases, a barrier between two:
//   0  thread 0 reads the record (resize_read of scene_math.h), decides which passes run and writes the slot's descriptor
//   1  equal sizes: a copy, and nothing else
//   2  the horizontal pass's coefficient rows go to LDS (one thread per row; a row has up to resize_row_taps taps), then every
//      row of the render is premultiplied on the fly and resampled to out_w -- or only premultiplied when the width stays
//                                                                                                    -> the workgroup's scratch
//   3  the vertical pass's rows replace the horizontal ones in LDS; resample to out_h, un-premultiply         -> the slot
// The intermediate (up to 1024 x 160 pixels) is why the passes go through memory; a workgroup reads only what it wrote
// itself, behind a barrier. Consecutive lanes take consecutive output pixels of a row, so the vertical pass reads and writes
// whole cache lines and the horizontal pass walks neighbouring windows of one source row.
//
// Memory safety for ANY parameter bytes: src is clamped into the bank and the size into the slot, every source coordinate of a
// pass is clamped into its image where the address is formed, a row's tap count is bounded by the room its pass has in LDS.
// The descriptors are the library's own. Compiled with -ffp-contract=off.
#include "pa_kernels.h"
#include "scene_math.h"

namespace pa {
namespace {

constexpr int SRZ_THREADS = 512;

struct SrzPlan {
    const uint32_t* src;
    int sw, sh, ow, oh;
    int need_h, need_v;
    int room_h, room_v;   // taps a row of either pass has room for
    int ok;
};

struct alignas(16) SrzLds {
    SrzPlan plan;
    int first[PA_SPRITE_RESIZE_H_MAX], cnt[PA_SPRITE_RESIZE_H_MAX];
    int32_t coef[PA_SPRITE_RESIZE_COEFS];
};
static_assert(sizeof(SrzLds) <= 64 * 1024, "one workgroup's LDS");
static_assert(PA_SPRITE_RESIZE_W_MAX <= PA_SPRITE_RESIZE_H_MAX, "first / cnt hold either pass's rows");
static_assert(PA_SPRITE_RESIZE_COEFS >= 4 * PA_SYNTH_SPRITE_MAX + 3 * PA_SPRITE_RESIZE_H_MAX, "ksize <= 4 in / out + 3");

// clip8 for the bytes this file packs into a dword: sprite_augment.hip's spa_clip8 ("A compiler matter": left
// to itself hipcc fuses two clip8s and the packing into one packed instruction whose upper half is wrong on gfx950). The
// empty statement hides the value from that combine and emits nothing.
__device__ __forceinline__ int srz_clip8(int acc) {
    int v = (int)clip8(acc);
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(SRZ_THREADS) void sprite_resize_kernel(const SpriteResizeArgs a) {
    __shared__ SrzLds L;
    const int tid = threadIdx.x;
    uint32_t* R = reinterpret_cast<uint32_t*>(a.scratch) + (size_t)blockIdx.x * PA_SYNTH_SPRITE_MAX * a.max_w;
    for (int sprite = blockIdx.x; sprite < a.n; sprite += gridDim.x) {
        uint32_t* slot = reinterpret_cast<uint32_t*>(a.out_px + (size_t)sprite * a.slot_bytes);
        __syncthreads();   // (the previous sprite's readers of L are done)
        // ---- phase 0 ----
        if (tid == 0) {
            const ResizeRead r = resize_read(a.params[sprite], a.n_sprites, a.max_w, a.max_h);
            const SynthDesc sd = a.sprite_desc[r.src];
            SrzPlan p;
            p.src = reinterpret_cast<const uint32_t*>(a.sprite_px + sd.offset);
            p.sw = scene_clampi(sd.w, 1, PA_SYNTH_SPRITE_MAX);
            p.sh = scene_clampi(sd.h, 1, PA_SYNTH_SPRITE_MAX);
            p.ow = r.ow;
            p.oh = r.oh;
            p.need_h = p.ow != p.sw;
            p.need_v = p.oh != p.sh;
            p.room_h = resize_row_taps(p.sw, p.ow);
            p.room_v = resize_row_taps(p.sh, p.oh);
            p.ok = p.ow * p.room_h <= PA_SPRITE_RESIZE_COEFS && p.oh * p.room_v <= PA_SPRITE_RESIZE_COEFS;   // (always: scene_math.h)
            L.plan = p;
            SynthDesc od;
            od.offset = (uint64_t)sprite * a.slot_bytes;
            od.w = p.ow;
            od.h = p.oh;
            a.out_desc[sprite] = od;
        }
        __syncthreads();
        const SrzPlan p = L.plan;
        const int n_out = p.ow * p.oh;
        if (!p.ok) {
            for (int i = tid; i < n_out; i += SRZ_THREADS) slot[i] = 0u;
            continue;
        }
        // ---- phase 1: equal sizes ----
        if (!p.need_h && !p.need_v) {
            for (int i = tid; i < n_out; i += SRZ_THREADS) slot[i] = p.src[i];
            continue;
        }
        // ---- phase 2: premultiply, horizontal pass ----
        const int n_mid = p.sh * p.ow;
        if (p.need_h) {
            for (int xx = tid; xx < p.ow; xx += SRZ_THREADS) resize_coef_row(p.sw, p.ow, xx, p.room_h, &L.first[xx], &L.cnt[xx], L.coef + xx * p.room_h);
            __syncthreads();
            for (int i = tid; i < n_mid; i += SRZ_THREADS) {
                const int y = i / p.ow, xx = i - y * p.ow;
                const int32_t* k = L.coef + xx * p.room_h;
                const int first = min(max(L.first[xx], 0), p.sw - 1), cnt = min(max(L.cnt[xx], 0), p.room_h);
                const uint32_t* row = p.src + (size_t)y * p.sw;
                int a0, a1, a2, a3;
                a0 = a1 = a2 = a3 = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t q = row[min(first + t, p.sw - 1)];
                    const int al = (int)(q >> 24), c = k[t];
                    a0 += mul24(scene_muldiv255((int)(q & 0xff), al), c);
                    a1 += mul24(scene_muldiv255((int)((q >> 8) & 0xff), al), c);
                    a2 += mul24(scene_muldiv255((int)((q >> 16) & 0xff), al), c);
                    a3 += mul24(al, c);
                }
                R[i] = pack4(srz_clip8(a0), srz_clip8(a1), srz_clip8(a2), srz_clip8(a3));
            }
        } else {
            for (int i = tid; i < n_mid; i += SRZ_THREADS) R[i] = rgba_premultiply(p.src[i]);
        }
        __syncthreads();
        // ---- phase 3: vertical pass, back to RGBA ----
        if (p.need_v) {
            for (int yy = tid; yy < p.oh; yy += SRZ_THREADS) resize_coef_row(p.sh, p.oh, yy, p.room_v, &L.first[yy], &L.cnt[yy], L.coef + yy * p.room_v);
            __syncthreads();
            for (int i = tid; i < n_out; i += SRZ_THREADS) {
                const int y = i / p.ow, x = i - y * p.ow;
                const int32_t* k = L.coef + y * p.room_v;
                const int first = min(max(L.first[y], 0), p.sh - 1), cnt = min(max(L.cnt[y], 0), p.room_v);
                int a0, a1, a2, a3;
                a0 = a1 = a2 = a3 = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t q = R[(size_t)min(first + t, p.sh - 1) * p.ow + x];
                    const int c = k[t];
                    a0 += mul24((int)(q & 0xff), c);
                    a1 += mul24((int)((q >> 8) & 0xff), c);
                    a2 += mul24((int)((q >> 16) & 0xff), c);
                    a3 += mul24((int)(q >> 24), c);
                }
                const int al = srz_clip8(a3);
                slot[i] = pack4(rgba_unpremultiply(srz_clip8(a0), al), rgba_unpremultiply(srz_clip8(a1), al), rgba_unpremultiply(srz_clip8(a2), al), al);
            }
        } else {
            for (int i = tid; i < n_out; i += SRZ_THREADS) {
                const uint32_t q = R[i];
                const int al = (int)(q >> 24);
                slot[i] = pack4(rgba_unpremultiply((int)(q & 0xff), al), rgba_unpremultiply((int)((q >> 8) & 0xff), al),
                                rgba_unpremultiply((int)((q >> 16) & 0xff), al), al);
            }
        }
    }
}

}  // namespace

hipError_t launch_sprite_resize(const SpriteResizeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(sprite_resize_kernel, dim3((unsigned)a.workgroups), dim3(SRZ_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace pa

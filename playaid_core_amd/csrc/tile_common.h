// What the tiled (non-persistent) convolution kernels share -- igemm.hip, igemm_bf16.hip, patchconv.hip, patchconv_bf16.hip,
// wino.hip, stem.hip, stem_pool.hip -- and what the persistent ones (pgemm_common.h) take from the same place: the vector types,
// the blockIdx -> work item remap over the 8 XCDs, m -> (image, row, column), the LDS-DMA builtin, counted waits, bf16 rounding,
// the fused epilogues, the staging cursor of the two im2col kernels, and on the host the launchers' shift, split-K, tile-shape and
// XCD-grid rules. Each kernel keeps its own matrix loop, LDS layout, swizzle and launcher.
//
// Two rules every helper here keeps, because the kernels' counted waits depend on them:
//  * a kernel has ONE __shared__ array and the helpers take pointers into it (a second shared object, or extern __shared__, makes
//    hipcc drain vmcnt to 0 in front of the operand reads);
//  * a helper that copies issues exactly the vector-memory operations its arguments name, in program order.
#pragma once
#include "pa_kernels.h"

namespace pa {

// ---------------------------------------------------------------- device ----------------------------------------------------------------

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: stays in VGPRs (HIP's float4 class did not)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t bf16_t;  // storage

// XCD-aware (bijective) remap of blockIdx b of a grid of nwg workgroups: blocks with equal b % 8 share an XCD (and its private L2)
// and get a contiguous run of work items.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = b & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// The 8 XCDs as a gm x gn grid over (pixel tiles, channel tiles), gm * gn == 8 dividing tiles_m and tiles_n: the tile of the
// workgroup of rank `rank` inside XCD `xcd` (= blockIdx & 7), channel tiles fastest. An XCD's L2 then fetches 1 / gm of the
// activations and 1 / gn of the weights instead of 1 / 8 of the former and all of the latter.
__device__ __forceinline__ void xcd_grid_tile(int xcd, int rank, int gm, int gn, int tiles_m, int tiles_n, int& tile_m, int& tile_n) {
    const int tm_per = tiles_m / gm, tn_per = tiles_n / gn;
    const int xm = xcd / gn, lm = rank / tn_per;
    tile_m = xm * tm_per + lm;
    tile_n = (xcd - xm * gn) * tn_per + (rank - lm * tn_per);
}

// m -> (img, oy, ox) with shifts when the output plane is a power of two (fill_pow2_shifts), integer division otherwise.
__device__ __forceinline__ void split_m(const GemmParams& p, int m, int& img, int& oy, int& ox) {
    if (p.howo_shift >= 0) {
        img = m >> p.howo_shift;
        const int rem = m & (p.howo - 1);
        oy = rem >> p.wo_shift;
        ox = rem & (p.wo - 1);
    } else {
        img = m / p.howo;
        const int rem = m - img * p.howo;
        oy = rem / p.wo;
        ox = rem - oy * p.wo;
    }
}

// 16-byte global -> LDS DMA in its buffer form (buffer_load_dwordx4 ... offen lds): LDS destination = wave-uniform `lds_ptr` +
// lane * 16, source = descriptor base + voff_bytes (per lane) + soff_bytes (wave-uniform). The FLAT form (global_load_lds) makes
// hipcc assume "a FLAT access may be pending" and turn every later wait into s_waitcnt vmcnt(0) lgkmcnt(0); behind the MUBUF form
// the waits stay counted.
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, int voff_bytes, int soff_bytes, void* lds_ptr) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_ptr, 16, voff_bytes, soff_bytes, 0, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t glds_rsrc(const void* base, int num_bytes = -1) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, num_bytes, 0x00020000);
}

// counted wait: all but the N youngest vector-memory operations of this wave are done
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is six bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// bf16 <-> fp32. The rounding is to nearest even for FINITE inputs (what the kernels round: sums of finite products); the host's
// bf16_rne (conv_rows.h) also keeps inf / NaN.
__device__ __forceinline__ float bf16_to_f32(bf16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint32_t bf16_round_bits(float f) {  // the rounded value in the upper 16 bits
    uint32_t u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u;
}
__device__ __forceinline__ bf16_t f32_to_bf16(float f) { return (bf16_t)(bf16_round_bits(f) >> 16); }
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {  // (lo = a, hi = b)
    return (bf16_round_bits(a) >> 16) | (bf16_round_bits(b) & 0xffff0000u);
}

// two integers 0 .. 255 as two bf16 (lo = a, hi = b): the upper halves of their fp32 patterns, exact (8 significant bits at most)
__device__ __forceinline__ uint32_t u8_bf16x2(int a, int b) {
    return (__float_as_uint((float)a) >> 16) | (__float_as_uint((float)b) & 0xffff0000u);
}

// activation of a conv epilogue on four floats: GemmParams::relu = 0 none, 1 ReLU, 2 SiLU
__device__ __forceinline__ f32x4 act4(f32x4 v, int relu) {
    if (relu == 1) {
        v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
        v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
    } else if (relu == 2) {
        v.x = silu_fast(v.x); v.y = silu_fast(v.y);
        v.z = silu_fast(v.z); v.w = silu_fast(v.w);
    }
    return v;
}
// fp32 epilogue of a tile: v + (bias + residual), activation -- or v + bias, activation, + residual (res_after: YOLOv5's Bottleneck)
__device__ __forceinline__ f32x4 epilogue4(f32x4 v, f32x4 bias4, f32x4 res4, int relu, int res_after) {
    v += res_after ? bias4 : bias4 + res4;
    v = act4(v, relu);
    if (res_after) v += res4;
    return v;
}

// Staging side of the two im2col kernels (igemm.hip: EB = 4, igemm_bf16.hip: EB = 2; BK in elements, an LDS row is BK * EB = 128 or
// 256 bytes): which tile and K split a workgroup owns, the source offsets of the rows its 256 threads stage, and the cursor over
// k-steps. One pass of the threads stages PASS_ROWS rows; LDS chunk c of staging row r receives logical 16-byte chunk c ^ swz(r),
// swz(r) = (r >> 1) & 7 for 128-byte rows and r & 15 for 256-byte rows -- r = row0 + PASS_ROWS * i, so the term only depends on
// row0 -- applied on the SOURCE address (an LDS-DMA wave instruction writes 1 KiB lane-linear). Offsets are in elements.
template <int EB, int BK, int BM, int BN, bool GATHER>
struct Im2colStage {
    static constexpr int CH = BK * EB / 16;      // 16-byte chunks per row (8 or 16)
    static constexpr int PASS_ROWS = 256 / CH;   // rows staged by one pass of the 256 threads (32 or 16)
    static constexpr int A_ROWS = BM / PASS_ROWS;  // staging rows per thread
    static constexpr int B_ROWS = BN / PASS_ROWS;
    static constexpr int CE = 16 / EB;           // elements per chunk

    int z, tile_m, tile_n;       // K split and tile of this workgroup
    int row0, colq;              // staging row of this thread within a pass, its (swizzled) source chunk
    int a_off[A_ROWS], a_off2[A_ROWS], b_off[B_ROWS];
    int nk_main, ks_begin, ks_end;   // k-steps of the first source; this split's k-steps
    int issue_ks;                // absolute index of the next k-step to issue
    int cur_kc, cur_kx, cur_ky;  // its channel offset and tap, advanced incrementally (one division at entry only)
    __amdgpu_buffer_rsrc_t act_rs, wgt_rs, act2_rs;

    __device__ __forceinline__ void setup(const GemmParams& p) {
        const int wg = xcd_remap(blockIdx.x, gridDim.x);
        const int tiles_mn = p.tiles_m * p.tiles_n;
        z = wg / tiles_mn;
        const int t_id = wg - z * tiles_mn;
        tile_m = t_id / p.tiles_n;
        tile_n = t_id - tile_m * p.tiles_n;

        const int tid = threadIdx.x;
        row0 = tid / CH;
        colq = (tid & (CH - 1)) ^ (CH == 8 ? ((row0 >> 1) & 7) : (row0 & 15));
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            int m = tile_m * BM + row0 + PASS_ROWS * i;
            m = m < p.M ? m : p.M - 1;
            a_off2[i] = 0;
            if (GATHER) {
                a_off[i] = m * p.taps;
            } else {
                int img, oy, ox;
                split_m(p, m, img, oy, ox);
                a_off[i] = img * p.in_img_stride + oy * p.stride * p.in_row_stride + ox * p.stride * p.in_px_stride + colq * CE;
                // optional second source for the last k2_steps k-steps (the 1x1/2 downsample branch of a residual block, fused
                // into conv2's accumulation as extra K)
                if (p.act2)
                    a_off2[i] = img * p.in2_img_stride + (oy * p.stride2 + p.off2) * p.in2_row_stride +
                                (ox * p.stride2 + p.off2) * p.in2_px_stride + colq * CE;
            }
        }
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i) b_off[i] = (tile_n * BN + row0 + PASS_ROWS * i) * p.ktot + colq * CE;

        nk_main = (p.ktot - p.k2_steps * BK) / BK;
        const int nk = p.ktot / BK;
        ks_begin = z * p.ksteps_per_split;
        ks_end = ks_begin + p.ksteps_per_split;
        ks_end = ks_end < nk ? ks_end : nk;
        issue_ks = ks_begin;
        const int cpt = p.chunk / BK;
        const int ksm = ks_begin < nk_main ? ks_begin : nk_main;
        const int tap = ksm / cpt;
        cur_kc = (ksm - tap * cpt) * BK;
        cur_ky = tap / p.kw_taps;
        cur_kx = tap - cur_ky * p.kw_taps;

        act_rs = glds_rsrc(p.act);
        wgt_rs = glds_rsrc(p.wgt);
        act2_rs = glds_rsrc(p.act2 ? p.act2 : p.act);
    }

    // Issue the LDS-DMA copies of the k-step under the cursor -- A_ROWS im2col rows to As_w + i KiB, then B_ROWS weight rows to
    // Bs_w + i KiB (this wave's 1 KiB pieces of the stage) -- then advance the cursor. first_source(ky, kx, kc) runs behind the
    // copies of a first-source k-step, before the cursor moves (igemm_bf16.hip's centre-tap weight copies).
    template <class Hook> __device__ __forceinline__ void issue(const GemmParams& p, float* As_w, float* Bs_w, Hook&& first_source) {
        if (issue_ks >= nk_main) {
            const int kc2 = (issue_ks - nk_main) * BK;
#pragma unroll
            for (int i = 0; i < A_ROWS; ++i) glds16(act2_rs, (a_off2[i] + kc2) * EB, 0, As_w + i * 1024);
            const int koff2 = nk_main * BK + kc2;
#pragma unroll
            for (int i = 0; i < B_ROWS; ++i) glds16(wgt_rs, (b_off[i] + koff2) * EB, 0, Bs_w + i * 1024);
        } else {
            const int tap = cur_ky * p.kw_taps + cur_kx;
            if (GATHER) {
#pragma unroll
                for (int i = 0; i < A_ROWS; ++i) {
                    const int row = p.gather[a_off[i] + tap];
                    glds16(act_rs, (row * p.in_px_stride + cur_kc + colq * CE) * EB, 0, As_w + i * 1024);
                }
            } else {
                const int tapoff = (cur_ky + p.off_y) * p.in_row_stride + (cur_kx + p.off_x) * p.in_px_stride + cur_kc;
#pragma unroll
                for (int i = 0; i < A_ROWS; ++i) glds16(act_rs, (a_off[i] + tapoff) * EB, 0, As_w + i * 1024);
            }
            const int koff = tap * p.chunk + cur_kc;
#pragma unroll
            for (int i = 0; i < B_ROWS; ++i) glds16(wgt_rs, (b_off[i] + koff) * EB, 0, Bs_w + i * 1024);
            first_source(cur_ky, cur_kx, cur_kc);
            cur_kc += BK;
            if (cur_kc == p.chunk) {
                cur_kc = 0;
                if (++cur_kx == p.kw_taps) {
                    cur_kx = 0;
                    ++cur_ky;
                }
            }
        }
        ++issue_ks;
    }
    __device__ __forceinline__ void issue(const GemmParams& p, float* As_w, float* Bs_w) {
        issue(p, As_w, Bs_w, [](int, int, int) {});
    }
};

// ----------------------------------------------------------------- host -----------------------------------------------------------------

// log2 of a power of two, -1 for anything else
inline int ilog2_exact(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return (1 << s) == v ? s : -1;
}

// GemmParams::howo_shift / wo_shift as split_m reads them: both logs when both are powers of two, else both -1
inline void fill_pow2_shifts(GemmParams& p) {
    p.howo_shift = ilog2_exact(p.howo);
    p.wo_shift = ilog2_exact(p.wo);
    if (p.howo_shift < 0 || p.wo_shift < 0) p.howo_shift = p.wo_shift = -1;
}

// split-K over nk k-steps: the wanted split clamped to [1, nk], equal runs of `per` k-steps, no empty splits
inline void plan_splitk(int nk, int32_t& splitk, int32_t& per) {
    if (splitk < 1) splitk = 1;
    if (splitk > nk) splitk = nk;
    per = (nk + splitk - 1) / splitk;
    splitk = (nk + per - 1) / per;
}

// BM x BN x BK (elements) of a GemmTile for elements of elem_bytes: LDS rows of 128 bytes, of 256 for the *_K64 shapes.
// TILE_256x128 exists for 2-byte elements only; whatever a launcher does not know is the last shape.
struct TileDims { int bm, bn, bk; };
inline TileDims tile_dims(GemmTile tile, int elem_bytes) {
    const int k128 = 128 / elem_bytes, k256 = 256 / elem_bytes;
    switch (tile) {
        case TILE_128x128: return {128, 128, k128};
        case TILE_128x64: return {128, 64, k128};
        case TILE_64x64: return {64, 64, k128};
        case TILE_128x64_K64: return {128, 64, k256};
        case TILE_256x128: if (elem_bytes == 2) return {256, 128, k128}; [[fallthrough]];
        default: return {64, 64, k256};
    }
}

// XCD grid of the patch-resident 3x3 kernels (xcd_grid_tile): bytes an XCD fetches for an (a x b) arrangement are input
// activations / a + weights / b; keep the default (a = 8: contiguous runs, xcd_m = xcd_n = 0) unless another divisor pair of the
// tile counts is at least 10 % cheaper. `allow` = false: the default always.
inline void pick_xcd_grid(GemmParams& p, bool allow) {
    p.xcd_m = p.xcd_n = 0;
    if (!allow) return;
    const double act = (double)p.total_px * p.chunk * 4.0, wgt = (double)p.N * p.ktot * 4.0;
    double best = act / 8 + wgt;
    for (int a = 4; a >= 1; a >>= 1) {
        const int bb = 8 / a;
        if (p.tiles_m % a || p.tiles_n % bb) continue;
        const double cost = act / a + wgt / bb;
        if (cost < 0.9 * best) {
            best = cost;
            p.xcd_m = a;
            p.xcd_n = bb;
        }
    }
}

}  // namespace pa

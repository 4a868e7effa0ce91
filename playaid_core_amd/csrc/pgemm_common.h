// What the three persistent implicit-GEMM convolution kernels share -- pigemm.hip (exact fp32), psgemm.hip (emulated fp32) and
// bgemm.hip (one-slice bf16): which tiles a workgroup walks, how a run of pixels becomes an offset, the issue cursor over k-steps
// and tiles, the loader waves' LDS-DMA ring, and on the host the launch plan and the weights' stage image. Each kernel keeps its
// own matrix loop, LDS layout, epilogue and launcher.
#pragma once
#include "conv_rows.h"
#include "tile_common.h"

#include <algorithm>
#include <cstring>

namespace pa {

// ---------------------------------------------------------------- device ----------------------------------------------------------------

// n / d and the remainder for a WAVE-UNIFORM 0 <= n < 2^25 with magic = min(ceil(2^32 / d), 2^32 - 1), 1 <= d < 2^16: the
// estimate is off by at most one either way (n * (magic * d - 2^32) < 2^32 * d * 2^-7); everything on the scalar unit
__device__ __forceinline__ int pgemm_sdiv(int n, int d, unsigned magic, int& rem) {
    int q = (int)__umulhi((unsigned)n, magic);
    int r = n - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
    rem = r;
    return q;
}

// The output map as the pixel walk needs it (persistent_plan's fields of GemmParams). nwx: how often a lane's column can wrap a row,
// nwy: how often its row can then wrap an image. A lane sits up to 31 pixels behind its run's first everywhere (p.pg_nwx, p.pg_nwy)
// except in bgemm's loaders, whose 64-byte rows put four lanes on a pixel and so 64 pixels under a wave: they set the counts for a
// reach of 63 themselves.
struct PixelGeom {
    int howo, wo, ho, nwx, nwy;
    unsigned magic_howo, magic_wo;
};
__device__ __forceinline__ PixelGeom pixel_geom(const GemmParams& p) {
    return PixelGeom{p.howo, p.wo, p.pg_ho, p.pg_nwx, p.pg_nwy, p.pg_magic_howo, p.pg_magic_wo};
}

// pixel m (wave-uniform) = (image, oy, ox) -> image * img_stride + oy * row_stride + ox * px_stride, on the scalar unit
__device__ __forceinline__ int pixel_base(const PixelGeom& g, int m, int img_stride, int row_stride, int px_stride, int& oy, int& ox) {
    int rem;
    const int img = pgemm_sdiv(m, g.howo, g.magic_howo, rem);
    oy = pgemm_sdiv(rem, g.wo, g.magic_wo, ox);
    return img * img_stride + oy * row_stride + ox * px_stride;
}

// Offset of pixel m_base + lane_row in a buffer whose pixel (image, oy, ox) sits at image * img_stride + oy * row_stride + ox *
// px_stride: the scalar base of the run's first pixel + lane_const (the lane's own lane_row * px_stride and whatever else it adds,
// kept in a register by the caller), the row and image wraps folded in with compares and selects -- no multiply or division per
// lane. wrap_x = row_stride - wo * px_stride (column wo -> column 0 of the next row), wrap_y = img_stride - ho * row_stride. Strides
// in whatever unit the caller addresses in. What a lane past M gets is the caller's business.
__device__ __forceinline__ int pixel_walk(const PixelGeom& g, int m_base, int lane_row, int img_stride, int row_stride, int px_stride, int wrap_x,
                                          int wrap_y, int lane_const) {
    int oy, ox_b;
    int off = pixel_base(g, m_base, img_stride, row_stride, px_stride, oy, ox_b) + lane_const;
    int ox = ox_b + lane_row;
    for (int w = 0; w < g.nwx; ++w) {
        const bool c = ox >= g.wo;
        ox -= c ? g.wo : 0;
        off += c ? wrap_x : 0;
        oy += c ? 1 : 0;
    }
    for (int w = 0; w < g.nwy; ++w) {
        const bool c = oy >= g.ho;
        oy -= c ? g.ho : 0;
        off += c ? wrap_y : 0;
    }
    return off;
}

// A workgroup's tiles: channel column tile_n, pixel tiles first, first + step, ... below end -- nt of them. The grid is 8 x p.pg_per
// workgroups, blockIdx & 7 = the XCD: an XCD takes a contiguous eighth of the pixel tiles, and the pg_per / tiles_n workgroups it has
// for a channel column take every step-th of them (the launcher makes pg_per a multiple of tiles_n).
struct TileRun {
    int tile_n, first, step, end, nt;
    __device__ __forceinline__ int tile(int t) const { return first + t * step; }
};
__device__ __forceinline__ TileRun tile_run(const GemmParams& p) {
    const int b = blockIdx.x, xcd = b & 7, local = b >> 3;
    const int TN = p.tiles_n, TM = p.tiles_m;
    const int LM = p.pg_per / TN, lm = local / TN;
    const int t_lo = (int)(((long long)xcd * TM) >> 3), t_hi = (int)(((long long)(xcd + 1) * TM) >> 3);
    return TileRun{local % TN, t_lo + lm, LM, t_hi, t_lo + lm < t_hi ? (t_hi - t_lo - lm + LM - 1) / LM : 0};
}

// Issue cursor: which k-step's operands are copied next -- tile, k-step of the tile, its tap (ky, kx) and channel offset kc
struct IssueCursor {
    int tile, ks, ky, kx, kc;
    // the k-step's tap and channel chunk as an element offset from a pixel's (off_y, off_x) corner
    __device__ __forceinline__ int tap_offset(const GemmParams& p) const { return ky * p.in_row_stride + kx * p.in_px_stride + kc; }
    // on to the next k-step (32 channels on, then the next tap); behind k-step ks_end - 1 on to the run's next tile, whose rows
    // rows_of(tile) computes (past the run's last tile: the rows of that one again; nobody issues them)
    template <class RowsOf> __device__ __forceinline__ void advance(const GemmParams& p, int ks_end, const TileRun& run, RowsOf&& rows_of) {
        kc += 32;
        if (kc == p.chunk) {
            kc = 0;
            if (++kx == p.kw_taps) { kx = 0; ++ky; }
        }
        if (++ks == ks_end) {
            ks = 0; ky = 0; kx = 0; kc = 0;
            tile += run.step;
            rows_of(tile < run.end ? tile : run.end - 1);
        }
    }
};

// ---- psgemm.hip and bgemm.hip: loader waves that copy with inline-assembly LDS-DMA (pigemm.hip copies with the builtin: its waits
// count the same wave's stores too, and the compiler has to know of the copies for that) ----

typedef int pgemm_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ pgemm_i32x4 lds_dma_rsrc(const void* base, unsigned num_bytes) {
    const unsigned long long a = (unsigned long long)base;
    return pgemm_i32x4{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32) & 0xffff), (int)num_bytes, 0x00020000};
}

// 16 bytes per lane, L2 / HBM -> LDS at lds_addr + 16 * lane (buffer_load_dwordx4 ... lds; M0 = destination). As inline assembly
// (wino.hip's reasons): hipcc then knows nothing of these copies and the kernel's own counted waits are the only ones. M0 is written
// and read in the SAME statement (it is compiler-reserved and cannot be declared; nothing else here lives in it: tests/test_abi.py).
__device__ __forceinline__ void lds_dma16(pgemm_i32x4 rsrc, int voff_bytes, int soff_bytes, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
                 :
                 : "v"(voff_bytes), "s"(rsrc), "s"(soff_bytes), "s"(lds_addr)
                 : "memory");
}

// A loader wave's life: `total` k-steps through a ring of NSTAGE LDS stages, NLD LDS-DMA instructions per wave and k-step, which
// issue(slot) issues for the cursor's k-step before advancing it. One barrier per k-step, shared with the consumer waves: barrier
// g + 1 says that stage g + 1 has landed and that every consumer's reads of stage g have returned, so stage g's slot is refilled
// behind it. The waits are counted: in front of barrier g + 1 exactly the copies of the (at most NSTAGE - 2) stages issued after
// stage g + 1 may be outstanding. REFILL = false: no copies after the prologue (psgemm.hip's timing ablation).
template <int NSTAGE, int NLD, bool REFILL = true, class Issue>
__device__ __forceinline__ void loader_ring(int total, Issue&& issue) {
    static_assert(NSTAGE >= 2 && NSTAGE <= 4, "wait_stage covers rings of two to four stages");
    auto wait_stage = [](int younger) {
        if (NSTAGE >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NLD) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    int slot = 0;
#pragma unroll
    for (int s = 0; s < NSTAGE; ++s)
        if (s < total) issue(s);
    {
        const int younger = (total < NSTAGE ? total : NSTAGE) - 1;   // stages 1 .. behind stage 0
        if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * NLD) : "memory");
        else wait_stage(younger);
    }
    __builtin_amdgcn_s_barrier();   // stage 0 (and what the workgroup stored to LDS before it) in LDS
    for (int g = 0; g + 1 < total; ++g) {
        // stages issued so far: min(g + NSTAGE, total); behind stage g + 1: min(g + NSTAGE, total) - (g + 2)
        const int inflight = (g + NSTAGE < total ? g + NSTAGE : total) - (g + 2);
        wait_stage(inflight);
        __builtin_amdgcn_s_barrier();   // stage g + 1 landed; every consumer's reads of stage g have returned
        if (REFILL && g + NSTAGE < total) issue(slot);
        slot = slot + 1 == NSTAGE ? 0 : slot + 1;
    }
    __builtin_amdgcn_s_barrier();   // (the consumers' barrier of the last k-step)
}

// ----------------------------------------------------------------- host -----------------------------------------------------------------

// The launchers' shared checks (conv mode, whole 32-channel k-steps, pixel counts and maps the scalar divisions and the 32-bit
// offsets hold) and the fields pgemm_sdiv and pixel_walk read: pg_ho, the two magics, pg_nwx, pg_nwy. Each launcher adds pg_per.
inline hipError_t persistent_plan(GemmParams& p) {
    if (p.gather || p.k2_steps || p.chunk % 32 != 0 || p.M <= 0 || p.M >= (1 << 24) || p.howo <= 0 || p.wo <= 0 || p.howo >= (1 << 16) ||
        p.howo % p.wo != 0 || p.ktot != p.taps * p.chunk)
        return hipErrorInvalidValue;
    auto magic = [](int d) { return (unsigned)std::min<unsigned long long>(((1ull << 32) + d - 1) / d, 0xffffffffull); };
    p.pg_ho = p.howo / p.wo;
    p.pg_magic_howo = magic(p.howo);
    p.pg_magic_wo = magic(p.wo);
    p.pg_nwx = 1 + 30 / p.wo;                         // column c + 31 <= wo - 1 + 31 wraps at most this often
    p.pg_nwy = (p.pg_ho - 1 + p.pg_nwx) / p.pg_ho;    // and row r + nwx that often
    return hipSuccess;
}

// workgroups per XCD of psgemm's and bgemm's unsplit grid over tiles_m x tiles_n tiles (the grid is 8 x that): one workgroup per CU =
// 32 per XCD, a multiple of the channel columns, and no more per column than the XCD's share of pixel tiles
inline int unsplit_per(int tiles_m, int tiles_n) {
    const int share = (tiles_m + 7) / 8;
    int lm = 32 / tiles_n;
    lm = lm < 1 ? 1 : (lm > share ? share : lm);
    return lm * tiles_n;
}

// The weights' LDS stage images (psgemm.hip, bgemm.hip): per (channel column of bn, k-step of 32) `pieces` 1 KiB DMA pieces holding
// `planes` planes of bn rows x 32 k bf16, the rest zero padding. stage_weight_elems: bf16 elements of the whole image, 0 = no such layout.
inline size_t stage_weight_elems(int N, int ktot, int bn, int pieces) {
    if (bn == 0 || ktot % 32 != 0 || N <= 0 || ktot <= 0) return 0;
    return (size_t)(N / bn) * (ktot / 32) * ((size_t)pieces * 512);
}

// w [N][ktot] fp32 (K contiguous: [cout][tap][cin], BatchNorm folded) -> [tile_n][k-step][plane s][row r][chunk c'][8] bf16: plane s =
// the s-th bf16 slice of the weight (s0 = bf16(x), s1 = bf16(x - s0), ...; one plane: the weight rounded to nearest even), chunk c' of
// row r holding k 8 (c' ^ ((r >> 2) & 3)) .. + 7
inline void pack_stage_weights(const float* w, int N, int ktot, int bn, int planes, int pieces, unsigned short* out) {
    const int nk = ktot / 32, tn_n = N / bn;
    const size_t stage = (size_t)pieces * 512;   // elements
    memset(out, 0, stage_weight_elems(N, ktot, bn, pieces) * sizeof(unsigned short));
    for (int tn = 0; tn < tn_n; ++tn)
        for (int ks = 0; ks < nk; ++ks) {
            unsigned short* img = out + ((size_t)tn * nk + ks) * stage;
            for (int r = 0; r < bn; ++r)
                for (int c = 0; c < 4; ++c) {
                    const int cp = c ^ ((r >> 2) & 3);
                    for (int j = 0; j < 8; ++j) {
                        float x = w[(size_t)(tn * bn + r) * ktot + ks * 32 + c * 8 + j];
                        for (int s = 0; s < planes; ++s) {
                            const unsigned short hq = bf16_rne(x);
                            img[((size_t)(s * bn + r) * 4 + cp) * 8 + j] = hq;
                            const uint32_t u = (uint32_t)hq << 16;
                            float f;
                            memcpy(&f, &u, 4);
                            x -= f;
                        }
                    }
                }
        }
}

}  // namespace pa

// "Emulated fp32" persistent implicit-GEMM convolution for gfx950: fp32 results from the bf16 matrix cores.
//
// The exact fp32 matrix instruction (v_mfma_f32_32x32x2_f32, pigemm.hip) runs at the fp32 VECTOR rate, 1/16 of the bf16 rate,
// and shares its SIMD with the vector ALU (SQ_VALU_MFMA_COEXEC_CYCLES = 0: DESIGN.md 5.1c). Here every fp32 operand is split
// into three bf16 slices -- x = s0 + s1 + s2 with s0 = bf16(x), s1 = bf16(x - s0), s2 = bf16(x - s0 - s1), an EXACT
// decomposition of the 24-bit significand (each subtraction is exact in fp32) -- and a product a * b becomes the six leading
// cross products a_i * b_j, i + j <= 2, each one v_mfma_f32_32x32x16_bf16: a bf16 x bf16 product is exact in fp32 and the
// instruction accumulates in fp32. The dropped terms (i + j >= 3) are below 2^-24 |a b|: the sum is as close to the float64
// product as the exact fp32 instruction's (measured on the oracle network: 2.0e-6 against 3.5e-6 on log-probabilities,
// tests/emulated_fp32_study.py; per layer: tests/test_psgemm.py against float64). Six bf16 instructions cost 6/16 of the matrix
// time of the fp32 instructions they replace, and the bf16 pipe runs BESIDE the vector ALU (scripts/micro/mfma_f32_mix.hip).
// This is the reference's arithmetic (playaid/ai_runner.py:191-224's network, cnn_action_detector.py:29-43) to fp32 rounding,
// never the default: compute_dtype PA_DTYPE_EMULATED_F32 selects it, `value` / `dtype` of bench.py stay on the exact path.
//
// Layout of the work (pigemm.hip's persistent scheme, re-cut for a matrix pipe that is 2.7x faster; the tile schedule, the pixel
// walk, the issue cursor and the loaders' ring are pgemm_common.h's, shared with pigemm.hip and bgemm.hip):
//   * 512 threads, ONE workgroup per CU: waves 0-3 CONSUME (LDS reads, split, matrix instructions, epilogue), waves 4-7 LOAD (every
//     LDS-DMA copy, the pixel address arithmetic, the counted waits) -- one of each per SIMD. A tile is 128 pixels x BN channels
//     (BN = 128 | 64 | 32) and consumer wave w owns pixels 32 w .. 32 w + 31 x ALL BN channels: every activation value is split
//     exactly once per workgroup (a 2 x 2 wave grid would split it twice -- the split, 44 vector instructions per 8 values, is
//     the loop's second cost; with 64-channel tiles it is the first).
//   * activations stay fp32 in HBM and in LDS (LDS-DMA, pigemm's swizzled 128-byte rows) and are split in registers behind
//     their ds_read_b128; the weights were split at fold time (psgemm_pack_weights) into the exact LDS stage image --
//     [tile_n][k-step][3 planes][BN rows][32 k] bf16, 16-byte chunk c of row r at chunk c ^ ((r >> 2) & 3) -- so their DMA
//     is a straight 1 KiB-per-instruction copy and a ds_read_b128 of 16 rows x 4 chunks hits 64 distinct banks.
//   * the ring is NSTAGE k-steps (32 k each) deep and the pipeline is SKEWED by half a k-step: a k-step's second half
//     (k 16..31) is multiplied AFTER the barrier that opens the next k-step, from operands already in registers, while the
//     next k-step's first operands are read and split. A stage is therefore free as soon as its last operand read has
//     returned, one barrier earlier than its last matrix instruction: NSTAGE stages are in flight, not NSTAGE - 1.
//   * between two matrix instructions stand at most one LDS read and two or three instructions of the split, placed by hand
//     (half()): a lone wave per SIMD hides nothing, whatever takes longer than the 32 cycles a matrix instruction occupies the
//     pipe idles it. Measured (profiles/r06_pgemm_split_stamps.txt): 1592 cycles per k-step for 1536 of matrix time on the
//     big-K layers, at the 1.53-1.57 GHz the chip holds in this loop.
//   * the loaders' waits are counted: in front of barrier g + 1 exactly the copies of the (at most NSTAGE - 2) younger stages may
//     be outstanding, s_waitcnt vmcnt(k * NLD) (NLD checked on the built object: tests/test_abi.py). The consumers never wait on
//     vmcnt; their stores are buffer stores whose descriptor drops the rows past M (offset beyond num_records), so a wave issues
//     the SAME stores for every tile, live rows or not (ADVICE round 5 on pigemm.hip's predicate-dependent store count).
//   * the bias is the value the accumulators start from (read from LDS per tile); SiLU / ReLU and the 16-byte stores run
//     from the accumulators: lane = pixel, runs of four consecutive channels. (Measured and NOT kept, commit 32f1f5b: the epilogue
//     handed to the loader waves through 64 KB of LDS staging, and stores transposed to whole cache lines -- same speed and 5-15 %
//     slower: on the short-K layers the stores cost their bytes, 4.6 TB/s of mixed traffic, not issue slots.
//     profiles/r06_pgemm_split_defer.txt)
#include "pgemm_common.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

// timing experiments only (results wrong when != 0; a diagnostic build: hipcc -DPA_PS_ABL=n): 1 = no copies after the prologue,
// 2 = no matrix instructions
#ifndef PA_PS_ABL
#define PA_PS_ABL 0
#endif

namespace pa {

namespace {

typedef __attribute__((address_space(3))) const f32x4 lds_cf4;
typedef __attribute__((address_space(3))) const u32x4 lds_cu4;
typedef __attribute__((address_space(3))) float lds_f;

__device__ __forceinline__ unsigned ps_cvt_pk_bf16(float a, float b) {   // (lo = a, hi = b), round to nearest even
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// x - (the bf16 in the LOW / HIGH half of q, widened): exact in fp32. As assembly so that hipcc cannot pair two of them into a
// v_pk_add_f32, which costs ~13 cycles beside bf16 matrix instructions where two scalar ones cost 8 (MI355X_MICROARCH.md, price of a filler)
__device__ __forceinline__ float ps_sub_lo(float x, unsigned q) {
    float r;
    const unsigned w = q << 16;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(w));
    return r;
}
__device__ __forceinline__ float ps_sub_hi(float x, unsigned q) {
    float r;
    const unsigned w = q & 0xffff0000u;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(w));
    return r;
}

// eight fp32 values -> their three bf16 slices as matrix operands (element j of the fragment = value j)
__device__ __forceinline__ void ps_split8(const f32x4 lo, const f32x4 hi, u32x4& s0, u32x4& s1, u32x4& s2) {
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned q0 = ps_cvt_pk_bf16(x[2 * q], x[2 * q + 1]);
        const float r0 = ps_sub_lo(x[2 * q], q0), r1 = ps_sub_hi(x[2 * q + 1], q0);
        const unsigned q1 = ps_cvt_pk_bf16(r0, r1);
        const float t0 = ps_sub_lo(r0, q1), t1 = ps_sub_hi(r1, q1);
        s0[q] = q0;
        s1[q] = q1;
        s2[q] = ps_cvt_pk_bf16(t0, t1);
    }
}

__device__ __forceinline__ f32x16 ps_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

constexpr int ps_b_pieces(int bn) { return bn == 32 ? 8 : bn * 3 / 16; }   // 1 KiB DMA pieces of a stage's weight image (32: 6 + 2 of padding)

}  // namespace

// ACT: 0 none, 1 ReLU, 2 SiLU. RES: a residual (addressed like the output) is added, before the activation (ResNet) or after it
// (YOLOv5's Bottleneck) by p.res_after; it may alias the output (in-place Bottlenecks: every value is read by the lane that writes it).
//
// 512 threads: waves 0-3 CONSUME (LDS reads, split, matrix instructions, epilogue), waves 4-7 LOAD (every LDS-DMA copy of the
// workgroup, the pixel address arithmetic, the counted waits); one of each per SIMD. An LDS-DMA instruction costs its wave 60-180
// cycles of issue (MI355X_MICROARCH.md, cycle constants) -- seven to ten of them per k-step in a wave whose matrix instructions
// want a slot every 32 cycles would idle the pipe a third of the time; in a partner wave they cost the consumer nothing but the
// shared barrier. The consumers never wait on vmcnt (their only vector-memory instructions are the tile's stores and residual loads).
template <int BN, int NSTAGE, int ACT, bool RES>
__global__ __launch_bounds__(512, 2) void psgemm_kernel(const GemmParams p, const unsigned short* __restrict__ wsp, unsigned out_bytes, unsigned up_bytes) {
    constexpr int BM = 128, CB = BN / 32;
    constexpr int A_BYTES = BM * 128;
    constexpr int PB = ps_b_pieces(BN) / 4;       // weight pieces per loader wave and k-step
    constexpr int B_BYTES = ps_b_pieces(BN) * 1024;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NLD = 4 + PB;                   // LDS-DMA instructions per loader wave and k-step
    constexpr int NM = 6 * CB;                    // matrix instructions per half k-step
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NSTAGE * STAGE + BN * 4];

    // --- this workgroup's tiles: one channel column, every step-th pixel tile of its XCD's contiguous share ----
    const TileRun run = tile_run(p);
    const int tile_n = run.tile_n, nt = run.nt;
    if (nt == 0) return;
    const int nk = p.ktot >> 5;
    const int total = nt * nk;

    const int tid = threadIdx.x;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const unsigned lds_base = (unsigned)(size_t)(lds_f*)(float*)lds;
    const PixelGeom geom = pixel_geom(p);

    // bias of the column -> LDS (the accumulators of every tile start from it)
    float* const bias_s = (float*)(lds + NSTAGE * STAGE);
    if (tid < BN) bias_s[tid] = p.bias ? p.bias[tile_n * BN + tid] : 0.f;
    // the store complete before the workgroup's first barrier, behind which every consumer wave reads bias_s: gfx950's barrier
    // waits for nothing by itself, and hipcc inserts no wait in front of it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    if (wave_id >= 4) {
        // =============================== loader waves ===============================
        const int lw = wave_id - 4, ltid = tid - 256;
        const int row0 = ltid >> 3;
        const int colq = (ltid & 7) ^ ((row0 >> 1) & 7);   // LDS chunk c of activation row r holds logical chunk c ^ ((r >> 1) & 7)
        const pgemm_i32x4 act_rs = lds_dma_rsrc(p.act, 0xffffffffu);
        const pgemm_i32x4 wgt_rs = lds_dma_rsrc(wsp + (size_t)tile_n * nk * (B_BYTES / 2), 0xffffffffu);
        // pixel addressing (pixel_walk: scalar base of a 32-pixel run + the lane's distance, wraps folded in), in bytes
        const int in_ps = p.in_px_stride * p.stride * 4, in_rs = p.in_row_stride * p.stride * 4;
        const int in_wrap_x = in_rs - p.wo * in_ps;
        const int in_wrap_y = p.in_img_stride * 4 - p.pg_ho * in_rs;
        const int in_org = (p.off_y * p.in_row_stride + p.off_x * p.in_px_stride) * 4;
        int in_lane = row0 * in_ps + colq * 16;
        asm volatile("" : "+v"(in_lane));
        int in_last;   // pixel M - 1: what the rows past M of a partial last tile read (computed, dropped)
        {
            int oy, ox;
            in_last = pixel_base(geom, p.M - 1, p.in_img_stride * 4, in_rs, in_ps, oy, ox) + in_org + colq * 16;
        }
        auto in_offset = [&](int m_base) {
            const int off = pixel_walk(geom, m_base, row0, p.in_img_stride * 4, in_rs, in_ps, in_wrap_x, in_wrap_y, in_org + in_lane);
            return m_base + row0 < p.M ? off : in_last;
        };
        IssueCursor cur{run.first, 0, 0, 0, 0};
        int a_off[4];
        auto rows_of = [&](int tile_m) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a_off[i] = in_offset(tile_m * BM + 32 * i);
        };
        rows_of(cur.tile);
        int b_lane = lw * PB * 1024 + lane * 16;
        asm volatile("" : "+v"(b_lane));
        auto issue = [&](int slot) {
            const unsigned sb = lds_base + slot * STAGE;
            const int tapoff = cur.tap_offset(p) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) lds_dma16(act_rs, a_off[i], tapoff, sb + lw * 1024 + i * 4096);
            const int koff = cur.ks * B_BYTES;
#pragma unroll
            for (int j = 0; j < PB; ++j) lds_dma16(wgt_rs, b_lane, koff + j * 1024, sb + A_BYTES + (lw * PB + j) * 1024);
            cur.advance(p, nk, run, rows_of);
        };
        loader_ring<NSTAGE, NLD, !(PA_PS_ABL & 1)>(total, issue);
        return;
    }

    // =============================== consumer waves ===============================
    const __amdgpu_buffer_rsrc_t out_rs = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t res_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.residual : p.out), 0, (int)out_bytes, 0x00020000);
    const int ch0 = tile_n * BN + 4 * lh;
    // output, in BYTES: O(m) = (img * OIS + (oy + pad) * ORS + (ox + pad) * OPS + ch0) * 4
    const int out_wrap_x = (p.out_row_stride - p.wo * p.out_px_stride) * 4;
    const int out_wrap_y = (p.out_img_stride - p.pg_ho * p.out_row_stride) * 4;
    int out_lane = (lr * p.out_px_stride + p.out_pad * (p.out_row_stride + p.out_px_stride) + ch0) * 4;
    asm volatile("" : "+v"(out_lane));
    auto out_offset = [&](int m_base) -> unsigned {
        const int off = pixel_walk(geom, m_base, lr, p.out_img_stride * 4, p.out_row_stride * 4, p.out_px_stride * 4, out_wrap_x, out_wrap_y, out_lane);
        return m_base + lr < p.M ? (unsigned)off : 0x80000000u;   // past M: beyond num_records, dropped (the launcher keeps buffers under 2 GB)
    };

    // the nearest-neighbour x2 up-sampled copy (p.up_out, YOLOv5's nn.Upsample behind model.10 / model.14 as four more stores of the
    // producer): pixel (oy, ox) -> (2 oy, 2 ox) .. (2 oy + 1, 2 ox + 1): the same walk with doubled row and pixel strides
    const __amdgpu_buffer_rsrc_t up_rs = __builtin_amdgcn_make_buffer_rsrc(p.up_out ? p.up_out : p.out, 0, (int)(p.up_out ? up_bytes : out_bytes), 0x00020000);
    const int up_rs_b = 2 * p.up_row_stride * 4, up_ps_b = 2 * p.up_px_stride * 4;
    const int up_wrap_x = up_rs_b - p.wo * up_ps_b, up_wrap_y = p.up_img_stride * 4 - p.pg_ho * up_rs_b;
    int up_lane = lr * up_ps_b + (p.up_pad * (p.up_row_stride + p.up_px_stride) + ch0) * 4;
    asm volatile("" : "+v"(up_lane));
    auto up_offset = [&](int m_base) -> unsigned {
        const int off = pixel_walk(geom, m_base, lr, p.up_img_stride * 4, up_rs_b, up_ps_b, up_wrap_x, up_wrap_y, up_lane);
        return m_base + lr < p.M ? (unsigned)off : 0x80000000u;
    };

    // LDS read addresses (bytes) of the two k halves: this wave's pixel rows; the weight rows lr of each 32-channel block
    unsigned a_rd[2], a_rd2[2], b_rd[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        a_rd[h] = lds_base + (wave_id * 32 + lr) * 128 + (((4 * h + 2 * lh) ^ ((lr >> 1) & 7)) * 16);
        a_rd2[h] = a_rd[h] ^ 16u;
        b_rd[h] = lds_base + A_BYTES + (lr * 4 + ((2 * h + lh) ^ ((lr >> 2) & 3))) * 16;
        asm volatile("" : "+v"(a_rd[h]), "+v"(a_rd2[h]), "+v"(b_rd[h]));
    }

    u32x4 a_c[3], a_n[3], b_c[CB][3], b_n[CB][3];
    f32x16 acc[CB];
    auto read_b = [&](u32x4 (&bb)[CB][3], unsigned sb, int h) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int s = 0; s < 3; ++s) bb[cb][s] = *(lds_cu4*)(size_t)(b_rd[h] + sb + (s * BN + cb * 32) * 64);
    };
    // Half a k-step: NM matrix instructions (six cross products per 32-channel block, smallest terms first, the blocks taking
    // turns) from the operand registers (a, bb). Dealt out among them, ONE OR TWO PER GAP, go the next half's LDS reads (the raw
    // pixels first, then the weight fragments -> bn) and the 44 vector instructions that split the raw values (-> an). A lone
    // wave per SIMD hides nothing by itself: whatever stands between two matrix instructions and takes longer than the 32
    // cycles one of them occupies the pipe idles it (measured on the first form of this loop, reads in bursts of 14 and the
    // split in chunks of six: 2300 cycles per k-step for 1536 of matrix time; SQ_ACTIVE_INST / SQ_WAIT_INST in
    // profiles/r06_pgemm_split_pmc.txt). Per gap the issue budget is 32 - 8 (the matrix instruction's own): one ds_read_b128
    // (~13) and two or three vector instructions (4 each). The split's instruction order keeps every result two instructions away
    // from its first reader (two value pairs in lock step), so no dependent-issue stall and no hazard nop.
    // `pre`: matrix instructions issued before `open` runs (the barrier of the second half); reads start in gap `pre`.
    constexpr unsigned HI16 = 0xffff0000u;
    auto half = [&](const u32x4 (&a)[3], const u32x4 (&bb)[CB][3], u32x4 (&an)[3], u32x4 (&bn)[CB][3], unsigned sb, int h, auto pre_c, auto&& open) {
        constexpr int PRE = decltype(pre_c)::value;
        constexpr int TA[6] = {0, 1, 2, 0, 1, 0}, TB[6] = {2, 1, 0, 1, 0, 0};
        constexpr int NR = 2 + 3 * CB;                                     // LDS reads of the next half
        constexpr int OS = PRE + (NM >= 24 ? 6 : (NM >= 12 ? 3 : 1));      // first gap that takes split instructions
        f32x4 raw[2];
        float x[8], r[8];
        unsigned w[8], q0[4], q1[4];
        auto sop = [&](int k) {   // one instruction of the split; k = 22 G + j, G = which raw quad (pairs 2 G, 2 G + 1)
            const int G = k / 22, j = k % 22, pq = 2 * G + (j & 1), e = 2 * pq;
            if (j < 2) {
                if (j == 0) {
                    x[4 * G] = raw[G].x; x[4 * G + 1] = raw[G].y; x[4 * G + 2] = raw[G].z; x[4 * G + 3] = raw[G].w;
                }
                q0[pq] = ps_cvt_pk_bf16(x[e], x[e + 1]);
                an[0][pq] = q0[pq];
            } else if (j < 4) {
                asm("v_lshlrev_b32 %0, 16, %1" : "=v"(w[e]) : "v"(q0[pq]));
            } else if (j < 6) {
                asm("v_and_b32 %0, %1, %2" : "=v"(w[e + 1]) : "s"(HI16), "v"(q0[pq]));
            } else if (j < 8) {
                asm("v_sub_f32 %0, %1, %2" : "=v"(r[e]) : "v"(x[e]), "v"(w[e]));
            } else if (j < 10) {
                asm("v_sub_f32 %0, %1, %2" : "=v"(r[e + 1]) : "v"(x[e + 1]), "v"(w[e + 1]));
            } else if (j < 12) {
                q1[pq] = ps_cvt_pk_bf16(r[e], r[e + 1]);
                an[1][pq] = q1[pq];
            } else if (j < 14) {
                asm("v_lshlrev_b32 %0, 16, %1" : "=v"(w[e]) : "v"(q1[pq]));
            } else if (j < 16) {
                asm("v_and_b32 %0, %1, %2" : "=v"(w[e + 1]) : "s"(HI16), "v"(q1[pq]));
            } else if (j < 18) {
                asm("v_sub_f32 %0, %1, %2" : "=v"(r[e]) : "v"(r[e]), "v"(w[e]));
            } else if (j < 20) {
                asm("v_sub_f32 %0, %1, %2" : "=v"(r[e + 1]) : "v"(r[e + 1]), "v"(w[e + 1]));
            } else {
                an[2][pq] = ps_cvt_pk_bf16(r[e], r[e + 1]);
            }
        };
        auto rop = [&](int k) {   // one LDS read of the next half: the two raw pixel quads first (the split waits for them)
            if (k == 0) raw[0] = *(lds_cf4*)(size_t)(a_rd[h] + sb);
            else if (k == 1) raw[1] = *(lds_cf4*)(size_t)(a_rd2[h] + sb);
            else bn[(k - 2) % CB][(k - 2) / CB] = *(lds_cu4*)(size_t)(b_rd[h] + sb + (((k - 2) / CB) * BN + ((k - 2) % CB) * 32) * 64);
        };
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            if (i == PRE) open();
            const int term = i / CB, cb = i % CB;
            if (!(PA_PS_ABL & 2)) acc[cb] = ps_mfma(bb[cb][TB[term]], a[TA[term]], acc[cb]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                int at = PRE + k;
                at = at > NM - 1 ? NM - 1 : at;
                if (at == i) rop(k);
            }
#pragma unroll
            for (int k = 0; k < 44; ++k) {
                int at = OS + (k * (NM - OS)) / 44;
                if (at == i) sop(k);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto load_bias = [&]() {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 b4 = *(const f32x4*)(bias_s + cb * 32 + 8 * g + 4 * lh);
                acc[cb][4 * g] = b4.x; acc[cb][4 * g + 1] = b4.y; acc[cb][4 * g + 2] = b4.z; acc[cb][4 * g + 3] = b4.w;
            }
    };

    __builtin_amdgcn_s_barrier();   // stage 0 (and bias_s) in LDS
    {
        const f32x4 lo = *(lds_cf4*)(size_t)a_rd[0], hi = *(lds_cf4*)(size_t)a_rd2[0];
        read_b(b_c, 0u, 0);
        ps_split8(lo, hi, a_c[0], a_c[1], a_c[2]);
    }

    // diagnostic build only (-DPA_PS_STAMP, p.clk = 8 words per consumer wave): shader clock (s_memtime) and the constant 100 MHz clock
    // (s_memrealtime) around the tile loop -> cycles per k-step and the clock the chip holds in this loop; and the same around the
    // k-steps alone (epilogues excluded). Values go to a buffer nothing else reads; in the product kernel no stamp executes.
#ifdef PA_PS_STAMP
    unsigned long long st_t0 = 0, st_r0 = 0, st_k = 0;
    if (p.clk) { st_t0 = __builtin_amdgcn_s_memtime(); st_r0 = __builtin_amdgcn_s_memrealtime(); }
#endif
    int slot = 0, g = 0;
    for (int t = 0; t < nt; ++t) {
        const int tile_m = run.tile(t);
#ifdef PA_PS_STAMP
        const unsigned long long st_ks = p.clk ? __builtin_amdgcn_s_memtime() : 0ull;
#endif
        load_bias();
        f32x4 res4[CB][4];
        const unsigned o_off = out_offset(tile_m * BM + wave_id * 32);
        const unsigned u_off = p.up_out ? up_offset(tile_m * BM + wave_id * 32) : 0u;
        for (int ks = 0; ks < nk; ++ks, ++g) {
            const unsigned sb = slot * STAGE;
            // ---- first half: multiply k 0..15 from registers; read and split k 16..31 of the same stage (the reads go out BEHIND the
            //      first matrix instruction: in front of it hipcc's wait for that instruction's operands, read in the previous
            //      iteration -- it loses the count over the loop's back edge -- would wait for brand-new reads as well) ----
            if (RES && BN < 128 && ks == nk - 1) {   // the tile's residual values: requested a k-step ahead of their use
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const unsigned off = o_off == 0x80000000u ? o_off : o_off + (unsigned)(cb * 32 + 8 * gq) * 4u;
                        res4[cb][gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(res_rs, off, 0, 0));
                    }
            }
            half(a_c, b_c, a_n, b_n, sb, 1, std::integral_constant<int, 0>{}, [] {});
            // every LDS read of stage g has returned: behind the barrier below its slot is overwritten
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            // ---- second half: multiply k 16..31 from registers; a few matrix instructions in, open k-step g + 1 (barrier) and read
            //      and split its first operands under the rest. (No branch around this for the last k-step: it then reads a slot
            //      nobody refills -- stale, unused -- and the loaders join one barrier more; straight-line code keeps hipcc's
            //      operand waits out of the matrix instructions' way.) ----
            const int nslot = slot + 1 == NSTAGE ? 0 : slot + 1;
            half(a_n, b_n, a_c, b_c, (unsigned)(nslot * STAGE), 0, std::integral_constant<int, (NM >= 24 ? 2 : 1)>{}, [] {
                __builtin_amdgcn_s_barrier();   // stage g + 1 landed (the loaders waited for it); stage g's slot is free
                __builtin_amdgcn_sched_barrier(0);
            });
            slot = nslot;
        }
#ifdef PA_PS_STAMP
        if (p.clk) st_k += __builtin_amdgcn_s_memtime() - st_ks;
#endif
        // ---- epilogue of the tile, straight from the accumulators: lane = pixel lr of the wave's 32, channels ch0 + 32 cb + 8 g + 0..3 ----
        if (RES && BN >= 128) {   // 128-channel tiles: the residual's 64 registers are free only now (the operand sets of the last half are dead)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const unsigned off = o_off == 0x80000000u ? o_off : o_off + (unsigned)(cb * 32 + 8 * gq) * 4u;
                    res4[cb][gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(res_rs, off, 0, 0));
                }
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 v = f32x4{acc[cb][4 * gq], acc[cb][4 * gq + 1], acc[cb][4 * gq + 2], acc[cb][4 * gq + 3]};   // (bias inside)
                if (RES && !p.res_after) v += res4[cb][gq];
                if (ACT == 2) {
                    v.x = silu_fast(v.x); v.y = silu_fast(v.y); v.z = silu_fast(v.z); v.w = silu_fast(v.w);
                } else if (ACT == 1) {
                    v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
                }
                if (RES && p.res_after) v += res4[cb][gq];
                const unsigned off = o_off == 0x80000000u ? o_off : o_off + (unsigned)(cb * 32 + 8 * gq) * 4u;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, v), out_rs, off, 0, 0);
                if (p.up_out) {
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const unsigned uo = u_off == 0x80000000u ? u_off : u_off + (unsigned)((q4 >> 1) * p.up_row_stride + (q4 & 1) * p.up_px_stride + cb * 32 + 8 * gq) * 4u;
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, v), up_rs, uo, 0, 0);
                    }
                }
            }
    }
#ifdef PA_PS_STAMP
    if (p.clk && lane == 0) {
        unsigned long long* c = p.clk + ((size_t)blockIdx.x * 4 + wave_id) * 8;
        c[0] = __builtin_amdgcn_s_memtime() - st_t0;
        c[1] = __builtin_amdgcn_s_memrealtime() - st_r0;
        c[2] = st_k;
        c[3] = (unsigned long long)total;
        c[4] = (unsigned long long)nt;
    }
#endif
}

// channels per workgroup = per stage image of the weight layout (`residual` is part of the choice only for the A/B switch PA_PS_RES128:
// 64-channel tiles request the residual a k-step ahead of the epilogue, 128-channel tiles -- no registers to spare until the last
// operand sets are dead -- at its start)
int psgemm_pick_bn(int N, int residual) {
    static const int res128 = getenv("PA_PS_RES128") ? atoi(getenv("PA_PS_RES128")) : 1;   // 0: residual layers on 64-channel tiles (A/B)
    return N % 128 == 0 && (!residual || res128) ? 128 : (N % 64 == 0 ? 64 : (N % 32 == 0 ? 32 : 0));
}

size_t psgemm_weight_elems(int N, int ktot, int residual) {
    const int bn = psgemm_pick_bn(N, residual);
    return stage_weight_elems(N, ktot, bn, ps_b_pieces(bn));
}

// w [N][ktot] fp32 -> the kernel's stage images (host): three planes, the exact decomposition of every weight into bf16 slices
void psgemm_pack_weights(const float* w, int N, int ktot, int residual, unsigned short* out) {
    const int bn = psgemm_pick_bn(N, residual);
    pack_stage_weights(w, N, ktot, bn, 3, ps_b_pieces(bn), out);
}

// Conv mode of GemmParams (no gather, no second source, no split-K); p.wgt is ignored, wsp = psgemm_pack_weights' image of it.
// out_floats: floats from p.out to the end of its buffer (bounds of the output descriptor, < 2^29).
hipError_t launch_psgemm(const GemmParams& p_in, const unsigned short* wsp, size_t out_floats, size_t up_floats, hipStream_t s) {
    GemmParams p = p_in;
    const int bn = psgemm_pick_bn(p.N, p.residual != nullptr);
    if (bn == 0 || !wsp || out_floats == 0 || out_floats >= (1ull << 29) || persistent_plan(p) != hipSuccess) return hipErrorInvalidValue;
    p.tiles_n = p.N / bn;
    p.tiles_m = (p.M + 127) / 128;
    p.pg_per = unsplit_per(p.tiles_m, p.tiles_n);
    const int grid = p.pg_per * 8;
    const unsigned out_bytes = (unsigned)(out_floats * 4);
#ifdef PA_PS_STAMP
    // PA_PS_STAMP_FILE=<path>: every launch appends "M K N grid | median over consumer waves of: shader cycles, 100 MHz ticks, cycles in k-steps, k-steps, tiles" (synchronises)
    static const char* stamp_file = getenv("PA_PS_STAMP_FILE");
    unsigned long long* clk_dev = nullptr;
    if (stamp_file) {
        if (hipMalloc(&clk_dev, (size_t)grid * 4 * 8 * 8) != hipSuccess) return hipErrorOutOfMemory;
        (void)hipMemsetAsync(clk_dev, 0, (size_t)grid * 4 * 8 * 8, s);
        p.clk = clk_dev;
    }
#endif
    if (p.up_out && (up_floats == 0 || up_floats >= (1ull << 29) || p.up_px_stride % 4 || p.up_row_stride % 4 || p.up_img_stride % 4 ||
                     (reinterpret_cast<unsigned long long>(p.up_out) & 15ull)))
        return hipErrorInvalidValue;
    const unsigned up_bytes = (unsigned)(up_floats * 4);
#define PA_PS_LAUNCH1(BN_, NS_, RES_)                                                                                                \
    do {                                                                                                                             \
        if (p.relu == 2) hipLaunchKernelGGL((psgemm_kernel<BN_, NS_, 2, RES_>), dim3(grid), dim3(512), 0, s, p, wsp, out_bytes, up_bytes);     \
        else if (p.relu == 1) hipLaunchKernelGGL((psgemm_kernel<BN_, NS_, 1, RES_>), dim3(grid), dim3(512), 0, s, p, wsp, out_bytes, up_bytes); \
        else hipLaunchKernelGGL((psgemm_kernel<BN_, NS_, 0, RES_>), dim3(grid), dim3(512), 0, s, p, wsp, out_bytes, up_bytes);                 \
    } while (0)
#define PA_PS_LAUNCH(BN_, NS_)                                                                                                       \
    do {                                                                                                                             \
        if (p.residual) PA_PS_LAUNCH1(BN_, NS_, true);                                                                               \
        else PA_PS_LAUNCH1(BN_, NS_, false);                                                                                         \
    } while (0)
    // ring depth: as deep as one workgroup per CU allows. PA_PS_STAGES=2 (A/B): a two-stage ring of 80 / 56 KB, which leaves a CU room for a
    // workgroup of another stream's kernel (the Motion-JPEG passes' 52 KB) beside this one -- the chain runs three streams
    static const int stages2 = getenv("PA_PS_STAGES") && atoi(getenv("PA_PS_STAGES")) == 2;
    if (stages2) {
        if (bn == 128) PA_PS_LAUNCH(128, 2);
        else if (bn == 64) PA_PS_LAUNCH(64, 2);
        else PA_PS_LAUNCH(32, 2);
    } else if (bn == 128) PA_PS_LAUNCH(128, 3);
    else if (bn == 64) PA_PS_LAUNCH(64, 4);
    else PA_PS_LAUNCH(32, 4);
#undef PA_PS_LAUNCH1
#ifdef PA_PS_STAMP
    if (clk_dev) {
        std::vector<unsigned long long> hst((size_t)grid * 4 * 8);
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(hst.data(), clk_dev, hst.size() * 8, hipMemcpyDeviceToHost);
        (void)hipFree(clk_dev);
        std::vector<double> cyc, clkghz, perk, perk_in;
        for (int w = 0; w < grid * 4; ++w) {
            const unsigned long long* c = &hst[(size_t)w * 8];
            if (c[3] == 0 || c[1] == 0) continue;
            cyc.push_back((double)c[0]);
            clkghz.push_back((double)c[0] / (double)c[1] * 0.1);
            perk.push_back((double)c[0] / (double)c[3]);
            perk_in.push_back((double)c[2] / (double)c[3]);
        }
        auto med = [](std::vector<double>& v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
        if (FILE* f = fopen(stamp_file, "a")) {
            fprintf(f, "M %d K %d N %d bn %d grid %d | wave lifetime %.0f cycles, in-kernel clock %.3f GHz, %.0f cycles per k-step (whole loop), %.0f inside the k-steps\n",
                    p.M, p.ktot, p.N, bn, grid, med(cyc), med(clkghz), med(perk), med(perk_in));
            fclose(f);
        }
    }
#endif
#undef PA_PS_LAUNCH
    return hipGetLastError();
}

}  // namespace pa

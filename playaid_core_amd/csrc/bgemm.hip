// One-slice bf16 form of the persistent implicit-GEMM convolution (psgemm.hip's launcher conventions and loader / consumer split; the
// tile schedule, the pixel walk, the issue cursor, the loaders' ring and the weights' stage image are pgemm_common.h's):
// the detection network's PA_DTYPE_BF16 convolutions -- every 1x1, stride-2 3x3 and stride-1 3x3 row of its table.
//
// What changes against psgemm.hip's emulated-fp32 kernel:
//   * activations are bf16 in HBM and in the LDS ring: a k-step (32 k) of a pixel is one 64-byte row, half the bytes of the fp32
//     row. 16-byte chunk c of row r sits at chunk c ^ ((r >> 2) & 3): a ds_read_b128 of 16 rows x one logical chunk (the lane
//     groups {0-3, 12-15, 20-27}, ...) hits 16 distinct 16-byte slots of the 256-byte bank span;
//   * the weights are ONE plane, rounded to nearest even once at create (bgemm_pack_weights), in psgemm's plane layout
//     [tile_n][k-step][BN rows][4 chunks][8], chunk c of row r at c ^ ((r >> 2) & 3); 32-channel tiles pad the 2 KiB image to 4;
//   * the consumers feed the LDS fragments straight into ONE v_mfma_f32_32x32x16_bf16 per product (no split in registers): a
//     k-step is 2 x BN / 32 matrix instructions, fed from registers read one k-step ahead;
//   * the epilogue adds the fp32 bias (the accumulators start from it), applies SiLU / ReLU in fp32, adds a bf16 residual in fp32,
//     and rounds once to nearest even on the store (8 bytes per lane and 4 channels); the fused 2x up-sampled copy is the same
//     bf16 value. OUT_F32: the Detect heads' fp32 store instead (no residual, no up-sampling).
// Loader waves 4-7: per k-step 2 activation pieces (128 rows x 64 bytes = 8 KiB) and BN / 64 weight pieces (at least one) of 1 KiB
// each, counted waits (loader_ring).
//
// Split-K form (SPLIT, the ResNet-50 table's small maps: launch_bgemm with p.splitk = S > 1): one workgroup per (output tile, k-slice),
// slice s covering k-steps [s nk / S, (s + 1) nk / S); slice 0's accumulators start from the bias, the others' from zero. Each
// consumer wave writes its 32 pixels x BN channels of fp32 partials to the slab and draws the ticket of (tile, wave); the last of
// the S waves to arrive sums the S partials IN SPLIT ORDER (its own read back from the slab as well, so the sum does not depend on
// who was last), resets the ticket and runs the unsplit epilogue (residual, activation, one rounding on the store).
#include "pgemm_common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace pa {

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u32x4 lds_cu4;
typedef __attribute__((address_space(3))) float lds_f;

// four fp32 values -> four bf16, round to nearest even (v_cvt_pk_bf16_f32), element 0 in the low half of word 0
__device__ __forceinline__ u32x2 bg_pack4(f32x4 v) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 lo = __builtin_convertvector((f32x2{v.x, v.y}), bf16x2), hi = __builtin_convertvector((f32x2{v.z, v.w}), bf16x2);
    return u32x2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
}
__device__ __forceinline__ f32x4 bg_unpack4(u32x2 q) {
    return f32x4{__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xffff0000u)};
}

constexpr int bg_b_pieces(int bn) { return bn == 32 ? 4 : bn / 16; }   // 1 KiB DMA pieces of a stage's weight image (32: 2 + 2 of padding)

}  // namespace

// ACT: 0 none, 1 ReLU, 2 SiLU. RES: a bf16 residual addressed like the output, added before (ResNet) or after (YOLOv5's Bottleneck,
// p.res_after) the activation; it may alias the output (every value is read by the lane that writes it). OUT_F32: fp32 output.
template <int BN, int NSTAGE, int ACT, bool RES, bool OUT_F32, bool SPLIT = false>
__global__ __launch_bounds__(512, 2) void bgemm_kernel(const GemmParams p, const unsigned short* __restrict__ wsp, unsigned out_bytes, unsigned up_bytes) {
    static_assert(!(RES && OUT_F32), "the fp32-output form is the Detect heads': no residual");
    static_assert(!(SPLIT && OUT_F32), "the split-K form stores bf16");
    constexpr int BM = 128, CB = BN / 32;
    constexpr int A_BYTES = BM * 64;
    constexpr int PB = bg_b_pieces(BN) / 4;       // weight pieces per loader wave and k-step
    constexpr int B_BYTES = bg_b_pieces(BN) * 1024;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NLD = 2 + PB;                   // LDS-DMA instructions per loader wave and k-step
    constexpr int OE = OUT_F32 ? 4 : 2;           // output element bytes
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NSTAGE * STAGE + BN * 4];

    // --- this workgroup's tiles: one channel column, every step-th pixel tile of its XCD's contiguous share ----
    // (SPLIT: the one tile w_tile = tile_m * TN + tile_n of workgroup w_tile * S + slice, k-steps ks_lo .. ks_lo + nk - 1)
    const int b = blockIdx.x, TN = p.tiles_n;
    const int S = SPLIT ? p.splitk : 1;
    const int w_tile = SPLIT ? b / S : 0, slice = SPLIT ? b - w_tile * S : 0;
    const TileRun run = SPLIT ? TileRun{w_tile % TN, w_tile / TN, 1, w_tile / TN + 1, 1} : tile_run(p);
    const int tile_n = run.tile_n, nt = run.nt;
    if (nt == 0) return;
    const int nk_all = p.ktot >> 5;
    const int ks_lo = SPLIT ? slice * nk_all / S : 0;
    const int nk = SPLIT ? (slice + 1) * nk_all / S - ks_lo : nk_all;
    const int total = nt * nk;

    const int tid = threadIdx.x;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const unsigned lds_base = (unsigned)(size_t)(lds_f*)(float*)lds;

    float* const bias_s = (float*)(lds + NSTAGE * STAGE);
    if (tid < BN) bias_s[tid] = p.bias && slice == 0 ? p.bias[tile_n * BN + tid] : 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the bias store complete before the first barrier: psgemm.hip)

    if (wave_id >= 4) {
        // =============================== loader waves ===============================
        const int lw = wave_id - 4, ltid = tid - 256;
        const int row0 = ltid >> 2;                          // 0..63: four lanes per 64-byte row
        const int colq = (ltid & 3) ^ ((row0 >> 2) & 3);     // LDS chunk c of activation row r holds logical chunk c ^ ((r >> 2) & 3)
        const pgemm_i32x4 act_rs = lds_dma_rsrc(p.act, 0xffffffffu);
        const pgemm_i32x4 wgt_rs = lds_dma_rsrc(wsp + (size_t)tile_n * nk_all * (B_BYTES / 2), 0xffffffffu);
        // pixel addressing in bytes (pixel_walk, with a lane's distance from the run's first pixel up to 63: its own wrap counts)
        const int in_ps = p.in_px_stride * p.stride * 2, in_rs = p.in_row_stride * p.stride * 2;
        const int in_wrap_x = in_rs - p.wo * in_ps;
        const int in_wrap_y = p.in_img_stride * 2 - p.pg_ho * in_rs;
        const int in_org = (p.off_y * p.in_row_stride + p.off_x * p.in_px_stride) * 2;
        PixelGeom geom = pixel_geom(p);
        geom.nwx = 1 + 62 / p.wo;
        geom.nwy = (p.pg_ho - 1 + geom.nwx) / p.pg_ho;
        int in_lane = row0 * in_ps + colq * 16;
        asm volatile("" : "+v"(in_lane));
        int in_last;   // pixel M - 1: what the rows past M of a partial last tile read (computed, dropped)
        {
            int oy, ox;
            in_last = pixel_base(geom, p.M - 1, p.in_img_stride * 2, in_rs, in_ps, oy, ox) + in_org + colq * 16;
        }
        auto in_offset = [&](int m_base) {
            const int off = pixel_walk(geom, m_base, row0, p.in_img_stride * 2, in_rs, in_ps, in_wrap_x, in_wrap_y, in_org + in_lane);
            return m_base + row0 < p.M ? off : in_last;
        };
        IssueCursor cur{run.first, ks_lo, 0, 0, 0};
        if (SPLIT) {   // the slice's first k-step: tap (ky, kx), channel offset kc
            const int k0 = ks_lo * 32, tap = k0 / p.chunk;
            cur.kc = k0 - tap * p.chunk;
            cur.ky = tap / p.kw_taps;
            cur.kx = tap - cur.ky * p.kw_taps;
        }
        int a_off[2];
        auto rows_of = [&](int tile_m) {
#pragma unroll
            for (int i = 0; i < 2; ++i) a_off[i] = in_offset(tile_m * BM + 64 * i);
        };
        rows_of(cur.tile);
        int b_lane = lw * PB * 1024 + lane * 16;
        asm volatile("" : "+v"(b_lane));
        auto issue = [&](int slot) {
            const unsigned sb = lds_base + slot * STAGE;
            const int tapoff = cur.tap_offset(p) * 2;
#pragma unroll
            for (int i = 0; i < 2; ++i) lds_dma16(act_rs, a_off[i], tapoff, sb + lw * 1024 + i * 4096);
            const int koff = cur.ks * B_BYTES;
#pragma unroll
            for (int j = 0; j < PB; ++j) lds_dma16(wgt_rs, b_lane, koff + j * 1024, sb + A_BYTES + (lw * PB + j) * 1024);
            cur.advance(p, ks_lo + nk, run, rows_of);   // (SPLIT: past the slice's last k-step nothing is issued)
        };
        loader_ring<NSTAGE, NLD>(total, issue);
        return;
    }

    // =============================== consumer waves ===============================
    const __amdgpu_buffer_rsrc_t out_rs = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t res_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.residual : p.out), 0, (int)out_bytes, 0x00020000);
    const int ch0 = tile_n * BN + 4 * lh;
    const PixelGeom geom = pixel_geom(p);
    // output, in BYTES: O(m) = (img * OIS + (oy + pad) * ORS + (ox + pad) * OPS + ch0) * OE
    const int out_wrap_x = (p.out_row_stride - p.wo * p.out_px_stride) * OE;
    const int out_wrap_y = (p.out_img_stride - p.pg_ho * p.out_row_stride) * OE;
    int out_lane = (lr * p.out_px_stride + p.out_pad * (p.out_row_stride + p.out_px_stride) + ch0) * OE;
    asm volatile("" : "+v"(out_lane));
    auto out_offset = [&](int m_base) -> unsigned {
        const int off = pixel_walk(geom, m_base, lr, p.out_img_stride * OE, p.out_row_stride * OE, p.out_px_stride * OE, out_wrap_x, out_wrap_y, out_lane);
        return m_base + lr < p.M ? (unsigned)off : 0x80000000u;   // past M: beyond num_records, dropped
    };
    // the nearest-neighbour x2 up-sampled copy: the same walk with doubled row and pixel strides, bf16
    const __amdgpu_buffer_rsrc_t up_rs = __builtin_amdgcn_make_buffer_rsrc(p.up_out ? p.up_out : p.out, 0, (int)(p.up_out ? up_bytes : out_bytes), 0x00020000);
    const int up_rs_b = 2 * p.up_row_stride * 2, up_ps_b = 2 * p.up_px_stride * 2;
    const int up_wrap_x = up_rs_b - p.wo * up_ps_b, up_wrap_y = p.up_img_stride * 2 - p.pg_ho * up_rs_b;
    int up_lane = lr * up_ps_b + (p.up_pad * (p.up_row_stride + p.up_px_stride) + ch0) * 2;
    asm volatile("" : "+v"(up_lane));
    auto up_offset = [&](int m_base) -> unsigned {
        const int off = pixel_walk(geom, m_base, lr, p.up_img_stride * 2, up_rs_b, up_ps_b, up_wrap_x, up_wrap_y, up_lane);
        return m_base + lr < p.M ? (unsigned)off : 0x80000000u;
    };

    // LDS read addresses (bytes) of the two k halves: this wave's pixel row lr; the weight rows lr of each 32-channel block
    unsigned a_rd[2], b_rd[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        a_rd[h] = lds_base + (wave_id * 32 + lr) * 64 + (((2 * h + lh) ^ ((lr >> 2) & 3)) * 16);
        b_rd[h] = lds_base + A_BYTES + (lr * 4 + ((2 * h + lh) ^ ((lr >> 2) & 3))) * 16;
        asm volatile("" : "+v"(a_rd[h]), "+v"(b_rd[h]));
    }

    u32x4 a0[2], a1[2], w0[CB][2], w1[CB][2];
    f32x16 acc[CB];
    u32x2 res2[CB][4];
    auto read = [&](u32x4 (&a)[2], u32x4 (&w)[CB][2], unsigned sb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            a[h] = *(lds_cu4*)(size_t)(a_rd[h] + sb);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) w[cb][h] = *(lds_cu4*)(size_t)(b_rd[h] + sb + cb * 32 * 64);
        }
    };

    int slot = 0, ks = 0, t = 0;
    unsigned o_off = 0, u_off = 0;
    // ---- epilogue of a tile, from the accumulators: lane = pixel lr of the wave's 32, channels ch0 + 32 cb + 8 g + 0..3 ----
    auto epilogue = [&]() {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 v = f32x4{acc[cb][4 * gq], acc[cb][4 * gq + 1], acc[cb][4 * gq + 2], acc[cb][4 * gq + 3]};   // (bias inside)
                if (RES && !p.res_after) v += bg_unpack4(res2[cb][gq]);
                if (ACT == 2) {
                    v.x = silu_fast(v.x); v.y = silu_fast(v.y); v.z = silu_fast(v.z); v.w = silu_fast(v.w);
                } else if (ACT == 1) {
                    v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
                }
                if (RES && p.res_after) v += bg_unpack4(res2[cb][gq]);
                const unsigned off = o_off == 0x80000000u ? o_off : o_off + (unsigned)(cb * 32 + 8 * gq) * OE;
                if (OUT_F32) {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), out_rs, off, 0, 0);
                } else {
                    const u32x2 q = bg_pack4(v);
                    __builtin_amdgcn_raw_buffer_store_b64(q, out_rs, off, 0, 0);
                    if (p.up_out) {
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            const unsigned uo = u_off == 0x80000000u ? u_off : u_off + (unsigned)((q4 >> 1) * p.up_row_stride + (q4 & 1) * p.up_px_stride + cb * 32 + 8 * gq) * 2u;
                            __builtin_amdgcn_raw_buffer_store_b64(q, up_rs, uo, 0, 0);
                        }
                    }
                }
            }
    };
    // one k-step: its operands (cur) are in flight or in registers; the next k-step's are read behind the barrier while the
    // matrix instructions of this one run. Every k-step of every tile, one barrier each (the loaders' count).
    auto step = [&](const u32x4 (&ca)[2], const u32x4 (&cw)[CB][2], u32x4 (&na)[2], u32x4 (&nw)[CB][2]) {
        if (ks == 0) {
            const int tile_m = run.tile(t);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 b4 = *(const f32x4*)(bias_s + cb * 32 + 8 * g + 4 * lh);
                    acc[cb][4 * g] = b4.x; acc[cb][4 * g + 1] = b4.y; acc[cb][4 * g + 2] = b4.z; acc[cb][4 * g + 3] = b4.w;
                }
            o_off = out_offset(tile_m * BM + wave_id * 32);
            u_off = p.up_out ? up_offset(tile_m * BM + wave_id * 32) : 0u;
        }
        if (RES && !SPLIT && ks == nk - 1) {   // the tile's residual values, requested ahead of the last k-step's matrix instructions
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const unsigned off = o_off == 0x80000000u ? o_off : o_off + (unsigned)(cb * 32 + 8 * gq) * 2u;
                    res2[cb][gq] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(res_rs, off, 0, 0));
                }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this k-step's operands are in registers: its slot may be refilled
        __builtin_amdgcn_s_barrier();                          // stage g + 1 landed (the loaders waited for it)
        __builtin_amdgcn_sched_barrier(0);
        const int nslot = slot + 1 == NSTAGE ? 0 : slot + 1;
        read(na, nw, (unsigned)(nslot * STAGE));   // (the last k-step reads a slot nobody refills: stale, unused)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, cw[cb][h]), __builtin_bit_cast(bf16x8, ca[h]), acc[cb], 0, 0, 0);
        slot = nslot;
        if (++ks < nk) return;
        ks = 0;
        ++t;
        if (!SPLIT) epilogue();
    };

    __builtin_amdgcn_s_barrier();   // stage 0 (and bias_s) in LDS
    read(a0, w0, 0u);
    int g = 0;
    for (; g + 1 < total; g += 2) {   // (two k-steps per trip: the operand sets trade places without register copies)
        step(a0, w0, a1, w1);
        step(a1, w1, a0, w0);
    }
    if (g < total) step(a0, w0, a1, w1);
    if constexpr (SPLIT) {
        // wino.hip's split-K hand-off (its comment gives the argument), per wave instead of per workgroup: every slab value is an
        // agent-scope atomic store (written through the storing XCD's L2), the wave waits for them (vmcnt(0) as inline assembly)
        // before lane 0's agent-scope ticket add, and the last arriver reads the slab with agent-scope atomic loads (served by L2 /
        // memory, never a stale L1 line). Slab: [workgroup][wave][value e][lane], each store instruction one 256-byte run.
        constexpr int NV = CB * 16;
        float* const mine = p.slab + ((size_t)b * 4 + wave_id) * (NV * 64) + lane;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int e = 0; e < 16; ++e) __hip_atomic_store(mine + (cb * 16 + e) * 64, acc[cb][e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int32_t* const ticket = p.tickets + w_tile * 4 + wave_id;
        int drawn = 0;
        if (lane == 0) drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        drawn = __builtin_amdgcn_readlane(drawn, 0);
        asm volatile("" ::: "memory");
        if (drawn != S - 1) return;
        if (lane == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        const float* const all = p.slab + ((size_t)w_tile * S * 4 + wave_id) * (NV * 64) + lane;   // slice sl: + sl * 4 * NV * 64
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[cb][e] = __hip_atomic_load(all + (cb * 16 + e) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int sl = 1; sl < S; ++sl)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    acc[cb][e] += __hip_atomic_load(all + ((size_t)sl * 4 * NV + cb * 16 + e) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (RES) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const unsigned off = o_off == 0x80000000u ? o_off : o_off + (unsigned)(cb * 32 + 8 * gq) * 2u;
                    res2[cb][gq] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(res_rs, off, 0, 0));
                }
        }
        epilogue();
    }
}

int bgemm_pick_bn(int N, int residual) { return psgemm_pick_bn(N, residual); }

size_t bgemm_weight_elems(int N, int ktot, int residual) {
    const int bn = bgemm_pick_bn(N, residual);
    return stage_weight_elems(N, ktot, bn, bg_b_pieces(bn));
}

// w [N][ktot] fp32 (K contiguous, BatchNorm folded) -> one RNE bf16 plane in the kernel's stage images (32-channel tiles: + 2 KiB of zeros)
void bgemm_pack_weights(const float* w, int N, int ktot, int residual, unsigned short* out) {
    const int bn = bgemm_pick_bn(N, residual);
    pack_stage_weights(w, N, ktot, bn, 1, bg_b_pieces(bn), out);
}

int bgemm_pick_split(const GemmParams& p, int force) {
    const int bn = bgemm_pick_bn(p.N, p.residual != nullptr);
    if (bn == 0 || p.M <= 0 || force == 0 || force == 1) return 1;
    const int tn = p.N / bn, tm = (p.M + 127) / 128;
    const int grid = 8 * unsplit_per(tm, tn);   // the unsplit grid launch_bgemm would launch
    if (grid >= 128) return 1;   // at least half the CUs (256 on an MI355X) busy
    const int tiles = tm * tn, nk = p.ktot / 32;
    auto fits = [&](int S) { return tiles * S <= BGEMM_SLAB_ITEMS && 4 * tiles <= BGEMM_TICKETS && nk / S >= 4; };
    if (force > 1) return force <= 8 && fits(force) ? force : 1;
    // what the per-row A/B of the ResNet-50 at 64 crops kept (profiles/r07_resformer_bf16_rows_ab.txt, three runs),
    // split time over unsplit time: the 3x3 rows on 4 x 4 maps (grid 32, 144 k-steps) 0.48-0.90 at S = 4 or 8 (one outlier, 1.12,
    // against 0.72 for the same row and S in the next column); the 3x3 rows on 8 x 8 maps (grid 64, 72 k-steps) 0.84-1.12 at S = 4,
    // a wash; the 1x1 rows on 8 x 8 maps (32 k-steps) 0.86-1.47 at S = 4, slower in 9 of 10; the 1x1 rows on 4 x 4 maps (64
    // k-steps) 0.90-1.26 at S = 8, 0.58-0.82 at S = 4 in one run only. The same row in the same form varies 0.68-1.20 between
    // processes under this measurement, so only the classes that were faster in every run are split.
    if (grid >= BGEMM_SPLIT_MAX_GRID || nk < BGEMM_SPLIT_MIN_KSTEPS) return 1;
    for (int S = 8; S >= 2; S >>= 1)
        if (fits(S)) return S;
    return 1;
}

// Conv mode of GemmParams with bf16 storage behind the float* fields (every stride and count in ELEMENTS): act, residual and
// up_out bf16, out bf16 or (out_f32) fp32. out_elems / up_elems: elements from p.out / p.up_out to the end of the buffer.
// Refuses (hipErrorInvalidValue) what the 32-bit byte offsets of the loaders and the store descriptors cannot span: the input
// images the layer reads, the output, the up-sampled copy -- 2 GB each.
hipError_t launch_bgemm(const GemmParams& p_in, const unsigned short* wsp, size_t out_elems, size_t up_elems, bool out_f32, hipStream_t s) {
    GemmParams p = p_in;
    const int bn = bgemm_pick_bn(p.N, p.residual != nullptr);
    if (bn == 0 || !wsp || out_elems == 0 || (out_f32 && (p.residual || p.up_out)) || persistent_plan(p) != hipSuccess) return hipErrorInvalidValue;
    const unsigned long long oe = out_f32 ? 4 : 2;
    const unsigned long long images = (unsigned long long)((p.M + p.howo - 1) / p.howo);
    // the input span the loaders address with int byte offsets: every image of the range, its border and channel slice included
    const unsigned long long in_bytes = (images * (unsigned long long)p.in_img_stride) * 2ull;
    if (p.in_img_stride <= 0 || in_bytes >= (1ull << 31) || out_elems * oe >= (1ull << 31)) return hipErrorInvalidValue;
    if (p.up_out && (up_elems == 0 || up_elems * 2ull >= (1ull << 31) || p.up_px_stride % 4 || p.up_row_stride % 4 || p.up_img_stride % 4 ||
                     (reinterpret_cast<unsigned long long>(p.up_out) & 7ull)))
        return hipErrorInvalidValue;
    p.tiles_n = p.N / bn;
    p.tiles_m = (p.M + 127) / 128;
    p.pg_per = unsplit_per(p.tiles_m, p.tiles_n);
    const int grid = p.pg_per * 8;
    const unsigned out_bytes = (unsigned)(out_elems * oe), up_bytes = (unsigned)(up_elems * 2);
    if (p.splitk > 1) {
        // split-K: workgroup w_tile * S + slice; the slab holds BGEMM_SLAB_ITEMS workgroups, the tickets 4 per tile
        const int S = p.splitk, tiles = p.tiles_m * p.tiles_n;
        if (out_f32 || p.up_out || !p.slab || !p.tickets || S > 8 || tiles * S > BGEMM_SLAB_ITEMS || 4 * tiles > BGEMM_TICKETS ||
            p.ktot / 32 < S)
            return hipErrorInvalidValue;
#define PA_BG_SPLIT2(BN_, RES_)                                                                                                       \
    do {                                                                                                                             \
        if (p.relu == 1) hipLaunchKernelGGL((bgemm_kernel<BN_, 4, 1, RES_, false, true>), dim3(tiles * S), dim3(512), 0, s, p, wsp, out_bytes, 0u); \
        else if (p.relu == 0) hipLaunchKernelGGL((bgemm_kernel<BN_, 4, 0, RES_, false, true>), dim3(tiles * S), dim3(512), 0, s, p, wsp, out_bytes, 0u); \
        else return hipErrorInvalidValue;                                                                                            \
    } while (0)
#define PA_BG_SPLIT(BN_)                                                                                                             \
    do {                                                                                                                             \
        if (p.residual) PA_BG_SPLIT2(BN_, true);                                                                                     \
        else PA_BG_SPLIT2(BN_, false);                                                                                               \
    } while (0)
        if (bn == 128) PA_BG_SPLIT(128);
        else if (bn == 64) PA_BG_SPLIT(64);
        else PA_BG_SPLIT(32);
#undef PA_BG_SPLIT
#undef PA_BG_SPLIT2
        return hipGetLastError();
    }
#define PA_BG_LAUNCH2(BN_, RES_, F32_)                                                                                                \
    do {                                                                                                                             \
        if (p.relu == 2) hipLaunchKernelGGL((bgemm_kernel<BN_, 4, 2, RES_, F32_>), dim3(grid), dim3(512), 0, s, p, wsp, out_bytes, up_bytes);     \
        else if (p.relu == 1) hipLaunchKernelGGL((bgemm_kernel<BN_, 4, 1, RES_, F32_>), dim3(grid), dim3(512), 0, s, p, wsp, out_bytes, up_bytes); \
        else hipLaunchKernelGGL((bgemm_kernel<BN_, 4, 0, RES_, F32_>), dim3(grid), dim3(512), 0, s, p, wsp, out_bytes, up_bytes);                 \
    } while (0)
#define PA_BG_LAUNCH(BN_)                                                                                                            \
    do {                                                                                                                             \
        if (out_f32) PA_BG_LAUNCH2(BN_, false, true);                                                                                \
        else if (p.residual) PA_BG_LAUNCH2(BN_, true, false);                                                                        \
        else PA_BG_LAUNCH2(BN_, false, false);                                                                                       \
    } while (0)
    if (bn == 128) PA_BG_LAUNCH(128);
    else if (bn == 64) PA_BG_LAUNCH(64);
    else PA_BG_LAUNCH(32);
#undef PA_BG_LAUNCH
#undef PA_BG_LAUNCH2
    return hipGetLastError();
}

}  // namespace pa

// Persistent implicit-GEMM convolution for gfx950 (exact fp32): the engine of igemm.hip rebuilt for layers whose tiles are
// SHORT -- the 1x1 convolutions and the stride-2 3x3 convolutions of the detection network (yolo.hip; the YOLOv5 subprocess
// of playaid/ai_runner.py:191-224). A 1x1 convolution over 64 channels is two k-steps per 128 x 64 tile: with one tile per
// workgroup (igemm.hip) a workgroup's life is address arithmetic, one HBM round trip, 64 matrix instructions per wave, a
// transposition through LDS and the drain of its stores -- measured 27-55 TFLOP/s, 1.5-3 TB/s on layers that are bound by
// HBM. Here a workgroup is PERSISTENT over a run of pixel tiles of one channel column and the LDS ring never drains:
//   * the issue cursor (which k-step's operands are copied next) runs two steps ahead of the compute cursor ACROSS tile
//     boundaries, so a tile's first operands arrive under the previous tile's last matrix instructions;
//   * copies are LDS-DMA (buffer_load ... lds), waits are COUNTED (s_waitcnt vmcnt(N) with N = the wave's younger copies
//     and stores) and the barrier is a raw s_barrier: two stages stay in flight across every barrier, and a tile's output
//     stores are never waited for;
//   * the matrix instruction takes the WEIGHTS as its row operand and the pixels as its column operand (as
//     patchconv.hip): a lane owns one pixel and runs of four consecutive channels, so bias + activation + the 16-byte
//     stores run straight from the accumulators -- no transposition, no barrier, nothing between two tiles but the stores.
// Same k order as igemm.hip (tap, channel chunk, eight-wide group, lane half); the bias is the value the accumulators start
// from instead of a last addition, so results agree with igemm.hip to the rounding of that one reordering.
// The tile schedule, the pixel walk and the issue cursor are pgemm_common.h's, shared with psgemm.hip and bgemm.hip.
#include "pgemm_common.h"

#include <algorithm>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace pa {


namespace {

typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

// The copies are tile_common.h's glds16 (the builtin): voff = the lane's byte offset (a register that lives as long as the tile),
// soff = the k-step's byte offset (scalar): no vector instruction between two copies.
// (vmcnt is six bits: a count past 63 waits at 63 -- for more than it must, never for less)
template <int N> __device__ __forceinline__ void pg_wait_vm() { wait_vmcnt<(N > 63 ? 63 : N)>(); }

}  // namespace

// BM x BN tiles, 256 threads = 2 x 2 waves (BN = 64) or 4 x 1 (BN = 32: layers with 32 output channels run without zero
// padding), three LDS stages of (BM + BN) rows x 32 floats.
//
// What a tile costs besides its matrix instructions is vector-ALU time -- scripts/micro/mfma_f32_mix.hip: next to a stream of
// v_mfma_f32_32x32x2_f32 an LDS read is free, a lone vector instruction costs ~12 cycles of the SIMD, a transcendental 16 (and
// v_mul_lo_u32, which the per-lane divisions were made of, is a quarter-rate instruction too) -- so the bookkeeping is kept off
// the vector unit:
//   * pixel index -> (image, row, column) of the tile's FIRST pixel on the scalar unit (pgemm_sdiv); a lane adds its pixel's
//     distance and folds the row / image wraps in with compares and selects (no multiply, no division per lane);
//   * a k-step's copies differ from the tile's first in a scalar byte offset only (buffer_load's soffset);
//   * the LDS read addresses of a k-step are eight adds in one burst (a burst costs about what a lone instruction does);
//   * SiLU on register pairs (v_pk_mul / v_pk_add around the two transcendentals).
// UP: the tile is ALSO written nearest-neighbour up-sampled by two into a second buffer (p.up_out: every output pixel to the 2 x 2
// pixels it becomes) -- YOLOv5's nn.Upsample behind model.10 / model.14 as four more stores of the producer instead of a pass
// of its own over HBM.
//
// DS (pgemm_branch_kernel: the stride-2 3x3 opener of a ResNet block, which takes the block's 1x1/2 downsample branch along): the
// centre tap (ky == kx == 1) reads exactly the pixels the branch reads, so on its chunk / 32 k-steps the stage also receives the
// BN x 32 block of p.wgt2 ([N][chunk]) and the wave issues its matrix instructions a second time, with the pixel operand it holds
// already, into a second accumulator set that starts from zero -- the k order of the branch as a GEMM of its own (channel chunk,
// eight-wide group, lane half), so p.out2 (no bias, no activation, addressed like p.out) has that GEMM's bits.
//
// GRP (pgemm_group_kernel: the 36 products of Winograd F(4x4, 3x3) taken apart, wino4.hip): p.grp_tiles consecutive pixel tiles are
// one group with a weight image [N][ktot] of its own, p.grp_wgt_bytes behind the previous group's. The group of a tile is one scalar
// division where the tile's row offsets are computed (rows_of) and enters the weight copies as part of their scalar offset; a
// workgroup's run of tiles may cross groups. The sums run in FOUR accumulator chains, one per eight-wide k group of a k-step (chain
// c: k with (k % 32) / 8 == c, ascending), added as (c0 + c1) + (c2 + c3) in front of the stores: the Winograd output transform
// multiplies the rounding of these sums by up to 64, and one chain of K = 512 fp32 additions put the layer at 1e-5 of its largest
// output where four chains of 128 stay near 4e-6. A row's bits depend on neither the tile shape nor the other rows.
template <int BM, int BN, bool SILU, bool STAMP, bool UP, bool DS, bool GRP = false>
__device__ __forceinline__ void pgemm_body(const GemmParams& p) {
    static_assert(!DS || (!UP && !STAMP && !SILU), "the branch form is the ResNet openers': ReLU, no up-sampled copy");
    static_assert(!GRP || (!UP && !STAMP && !SILU && !DS), "the grouped form is a plain product");
    // STAMP (scripts/pgemm_stamps.py): s_memtime per wave at entry [0], after the prologue [1], per tile t < 15 at 2 + 4 t:
    // tile start, first barrier passed, last matrix instruction issued, stores issued; exit [63]
    auto stamp = [&](int i) {
        if (STAMP) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == 0) p.clk[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + i] = t;
        }
    };
    stamp(0);
    constexpr int WM = BN == 64 ? 2 : 4;      // waves along the pixel rows
    constexpr int MI = BM / WM / 32;
    constexpr int A_ROWS = BM / 32, B_ROWS = BN / 32;
    constexpr int NLD = A_ROWS + B_ROWS;  // LDS-DMA wave instructions per k-step (DS: B_ROWS more on a centre-tap step, see pre())
    constexpr int NST = MI * 4 * (UP ? 5 : (DS ? 2 : 1));   // store wave instructions per tile
    constexpr int STAGE = (BM + BN + (DS ? BN : 0)) * 32;   // (DS: the rows of wgt2 behind those of wgt)
    __shared__ __attribute__((aligned(16))) float lds[3 * STAGE];

    // --- this workgroup's tiles: one channel column, every step-th pixel tile of its XCD's contiguous share -------------
    const TileRun run = tile_run(p);
    const int tile_n = run.tile_n, nt = run.nt;
    {   // the arguments the loop needs are asked for BEFORE the early exit below: one round trip of scalar loads instead of two
        const float *pa_ = p.act, *pw_ = p.wgt, *pb_ = p.bias;
        float* po_ = p.out;
        const int i0 = p.M, i1 = p.ktot, i2 = p.kw_taps, i3 = p.chunk, i4 = p.howo, i5 = p.wo, i6 = p.in_img_stride, i7 = p.in_row_stride,
                  i8 = p.in_px_stride, i9 = p.stride, i10 = p.off_y, i11 = p.off_x, i12 = p.out_img_stride, i13 = p.out_row_stride,
                  i14 = p.out_px_stride, i15 = p.out_pad, i16 = p.pg_ho, i17 = p.pg_nwx, i18 = p.pg_nwy;
        const unsigned u0 = p.pg_magic_howo, u1 = p.pg_magic_wo;
        asm volatile("" ::"s"(pa_), "s"(pw_), "s"(pb_), "s"(po_), "s"(i0), "s"(i1), "s"(i2), "s"(i3), "s"(i4), "s"(i5), "s"(i6), "s"(i7), "s"(i8), "s"(i9),
                     "s"(i10), "s"(i11), "s"(i12), "s"(i13), "s"(i14), "s"(i15), "s"(i16), "s"(i17), "s"(i18), "s"(u0), "s"(u1));
        if (DS) {
            const float* pw2_ = p.wgt2;
            float* po2_ = p.out2;
            asm volatile("" ::"s"(pw2_), "s"(po2_));
        }
        if (GRP) {
            const int g0 = p.grp_tiles, g1 = p.grp_wgt_bytes;
            const unsigned g2 = p.grp_magic;
            asm volatile("" ::"s"(g0), "s"(g1), "s"(g2));
        }
    }
    if (nt == 0) return;
    stamp(60);
    const int nk = p.ktot >> 5;  // k-steps per tile
    const int total = nt * nk;
    const int nkc = p.chunk >> 5;                 // k-steps per tap
    const int c_lo = 4 * nkc, c_hi = 5 * nkc;     // DS: the centre tap's k-steps of a tile

    const int tid = threadIdx.x;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = tid >> 3;
    const int colq = (tid & 7) ^ ((row0 >> 1) & 7);  // LDS chunk c of row r holds logical chunk c ^ ((r >> 1) & 7)
    const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int wm = BN == 64 ? wave_id >> 1 : wave_id, wn = BN == 64 ? wave_id & 1 : 0;

    const __amdgpu_buffer_rsrc_t act_rs = glds_rsrc(p.act), wgt_rs = glds_rsrc(p.wgt);
    const __amdgpu_buffer_rsrc_t wgt2_rs = glds_rsrc(DS ? p.wgt2 : p.wgt);

    const int ch0 = tile_n * BN + wn * 32 + 4 * lh;
    f32x2 nl2e = f32x2{-1.44269504088896341f, -1.44269504088896341f}, one2 = f32x2{1.f, 1.f};
    asm volatile("" : "+v"(nl2e), "+v"(one2));   // (register pairs: v_pk_mul / v_pk_add take no literal)

    int b_off[B_ROWS];   // bytes
#pragma unroll
    for (int i = 0; i < B_ROWS; ++i) b_off[i] = ((tile_n * BN + row0 + 32 * i) * p.ktot + colq * 4) * 4;
    int b2_off[B_ROWS];   // DS: the same rows of wgt2 [N][chunk]
#pragma unroll
    for (int i = 0; i < B_ROWS; ++i) b2_off[i] = DS ? ((tile_n * BN + row0 + 32 * i) * p.chunk + colq * 4) * 4 : 0;

    // --- pixel addressing: scalar base of a 32-pixel run + the lane's distance, wraps folded in -------------------------
    // input, in bytes: A(m) = img * IS + (oy * s + off_y) * RS + (ox * s + off_x) * PS
    const int in_ps = p.in_px_stride * p.stride * 4, in_rs = p.in_row_stride * p.stride * 4;
    const int in_wrap_x = in_rs - p.wo * in_ps;                          // column wo -> column 0 of the next row
    const int in_wrap_y = p.in_img_stride * 4 - p.pg_ho * in_rs;         // row ho -> row 0 of the next image
    const int in_org = (p.off_y * p.in_row_stride + p.off_x * p.in_px_stride) * 4;
    int in_lane = row0 * in_ps + colq * 16;
    asm volatile("" : "+v"(in_lane));   // (kept as a register: the compiler would fold it back into a per-tile multiply)
    const PixelGeom geom = pixel_geom(p);
    int in_last;   // pixel M - 1: what the rows past M of a partial last tile read (computed, dropped)
    {
        int oy, ox;
        in_last = pixel_base(geom, p.M - 1, p.in_img_stride * 4, in_rs, in_ps, oy, ox) + in_org + colq * 16;
    }
    auto in_offset = [&](int m_base) {   // byte offset of this lane's row of the 32-pixel run starting at the uniform m_base
        const int off = pixel_walk(geom, m_base, row0, p.in_img_stride * 4, in_rs, in_ps, in_wrap_x, in_wrap_y, in_org + in_lane);
        return m_base + row0 < p.M ? off : in_last;
    };
    // output, in floats: O(m) = img * OIS + (oy + pad) * ORS + (ox + pad) * OPS + ch0
    const int out_wrap_x = p.out_row_stride - p.wo * p.out_px_stride;
    const int out_wrap_y = p.out_img_stride - p.pg_ho * p.out_row_stride;
    int out_lane = lr * p.out_px_stride + p.out_pad * (p.out_row_stride + p.out_px_stride) + ch0;
    asm volatile("" : "+v"(out_lane));
    auto out_offset = [&](int m_base) { return pixel_walk(geom, m_base, lr, p.out_img_stride, p.out_row_stride, p.out_px_stride, out_wrap_x, out_wrap_y, out_lane); };
    // the up-sampled copy: pixel (oy, ox) -> (2 oy, 2 ox) .. (2 oy + 1, 2 ox + 1): the same walk with doubled row and pixel strides
    const int up_rs = 2 * p.up_row_stride, up_ps = 2 * p.up_px_stride;
    const int up_wrap_x = up_rs - p.wo * up_ps, up_wrap_y = p.up_img_stride - p.pg_ho * up_rs;
    int up_lane = lr * up_ps + p.up_pad * (p.up_row_stride + p.up_px_stride) + ch0;
    asm volatile("" : "+v"(up_lane));
    // issue cursor: tile, (ky, kx, kc) of its next k-step; the tile's row offsets
    IssueCursor cur{run.first, 0, 0, 0, 0};
    int a_off[A_ROWS];   // bytes
    int w_grp = 0;       // GRP: byte offset of the tile's weight image
    auto rows_of = [&](int tile_m) {
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) a_off[i] = in_offset(tile_m * BM + 32 * i);
        if (GRP) {
            int rem;
            w_grp = pgemm_sdiv(tile_m, p.grp_tiles, p.grp_magic, rem) * p.grp_wgt_bytes;
        }
    };
    rows_of(cur.tile);
    stamp(61);
    auto issue = [&](int slot) {
        float* As_w = lds + slot * STAGE + wave_id * 256;
        float* Bs_w = As_w + BM * 32;
        const int tapoff = cur.tap_offset(p) * 4;
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) glds16(act_rs, a_off[i], tapoff, As_w + i * 1024);
        const int koff = ((cur.ky * p.kw_taps + cur.kx) * p.chunk + cur.kc) * 4 + (GRP ? w_grp : 0);
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i) glds16(wgt_rs, b_off[i], koff, Bs_w + i * 1024);
        if (DS && cur.ky == 1 && cur.kx == 1) {   // a centre-tap step: B_ROWS more copies, LAST of the step's (pre() counts on that)
#pragma unroll
            for (int i = 0; i < B_ROWS; ++i) glds16(wgt2_rs, b2_off[i], cur.kc * 4, Bs_w + BN * 32 + i * 1024);
        }
        cur.advance(p, nk, run, rows_of);
    };

    // LDS read addresses of the four eight-wide k groups within a stage (bytes; the 32-row block is an immediate of the read)
    unsigned a_k[4], b_k[4];
    {
        const int a_rd = (wm * (BM / WM) + lr) * 32, b_rd = BM * 32 + (wn * 32 + lr) * 32;
        const int swz = (lr >> 1) & 7;
        const unsigned base = (unsigned)(size_t)(lds_f32*)lds;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int ch_ = ((kk * 2 + lh) ^ swz) * 4;
            a_k[kk] = base + (a_rd + ch_) * 4;
            b_k[kk] = base + (b_rd + ch_) * 4;
            asm volatile("" : "+v"(a_k[kk]), "+v"(b_k[kk]));
        }
    }

    issue(0);
    stamp(62);
    if (total > 1) issue(1);
    // bias of this lane's channels ch0 + 8 g + 0..3, the value every accumulator of a tile starts from: fetched BEHIND the first
    // copies (its round trip runs under theirs; the kernel's first 4 us used to be this load alone) and pinned, so that the
    // compiler's wait for it -- a full drain, as for any register load beside LDS-DMA -- happens here, where the first stage
    // is awaited anyway, and not in the loop
    f32x16 biasv;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + ch0 + 8 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
        biasv[4 * g] = b4.x; biasv[4 * g + 1] = b4.y; biasv[4 * g + 2] = b4.z; biasv[4 * g + 3] = b4.w;
    }
    asm volatile("" : "+v"(biasv));
    stamp(1);

    f32x16 acc[MI];
    f32x16 acc2[MI];   // DS: the branch's sums
    f32x16 accg[GRP ? 3 : 1][MI];   // GRP: chains 1..3 (chain 0 is acc)
    // one k-step on the stage at byte offset sb: 16 matrix instructions per 32-pixel block, operands read one k group
    // ahead; the eight read addresses in one burst of vector adds before the first of them
    // branch_c (DS): 0 = not a centre-tap step, 1 = the centre tap's first step (the branch's accumulators start from zero), 2 = its others:
    // the rows of wgt2 are read beside those of wgt and every matrix instruction is issued a second time on them
    auto kstep = [&](int sb, auto first_c, auto branch_c) {
        constexpr bool FIRST = decltype(first_c)::value;   // a tile's first k-step: the accumulators start from the bias
        constexpr int BR = decltype(branch_c)::value;
        f32x16 zero16;
        if (BR == 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e) zero16[e] = 0.f;
        }
        f32x4 b2f[2];
        unsigned ra[4], rb[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            ra[kk] = a_k[kk] + sb;
            rb[kk] = b_k[kk] + sb;
            asm volatile("" : "+v"(ra[kk]), "+v"(rb[kk]));
        }
        f32x4 af[2][MI], bf[2];
#define PG_FRAGS(SET, KK)                                                                                    \
    {                                                                                                        \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                                    \
            af[SET][mi] = *(const lds_f32x4*)(size_t)(ra[KK] + mi * 4096);                                   \
        bf[SET] = *(const lds_f32x4*)(size_t)(rb[KK]);                                                       \
        if (BR) b2f[SET] = *(const lds_f32x4*)(size_t)(rb[KK] + BN * 128);                                    \
    }
        PG_FRAGS(0, 0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const f32x4 a4 = af[kk & 1][mi], b4 = bf[kk & 1];
                f32x16& acc_k = GRP && kk > 0 ? accg[GRP ? kk - 1 : 0][mi] : acc[mi];   // (GRP: the k group's own chain; its bias is zero)
                acc_k = __builtin_amdgcn_mfma_f32_32x32x2f32(b4.x, a4.x, FIRST && (GRP || kk == 0) ? biasv : acc_k, 0, 0, 0);
                acc_k = __builtin_amdgcn_mfma_f32_32x32x2f32(b4.y, a4.y, acc_k, 0, 0, 0);
                if (mi == 0 && kk + 1 < 4) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (kk == 0) { PG_FRAGS(1, 1); } else if (kk == 1) { PG_FRAGS(0, 2); } else { PG_FRAGS(1, 3); }
                    __builtin_amdgcn_sched_barrier(0);
                }
                acc_k = __builtin_amdgcn_mfma_f32_32x32x2f32(b4.z, a4.z, acc_k, 0, 0, 0);
                acc_k = __builtin_amdgcn_mfma_f32_32x32x2f32(b4.w, a4.w, acc_k, 0, 0, 0);
                if (BR) {
                    const f32x4 c4 = b2f[kk & 1];
                    acc2[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.x, a4.x, BR == 1 && kk == 0 ? zero16 : acc2[mi], 0, 0, 0);
                    acc2[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.y, a4.y, acc2[mi], 0, 0, 0);
                    acc2[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.z, a4.z, acc2[mi], 0, 0, 0);
                    acc2[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.w, a4.w, acc2[mi], 0, 0, 0);
                }
            }
        }
#undef PG_FRAGS
    };

    int slot = 0, g = 0;
    // what precedes the matrix instructions of k-step g (the tile's ks-th): wait for its stage, barrier, request stage g + 2
    auto pre = [&](int ks, int t) {
        // Stage g must have landed. VMEM operations complete in order and this wave issued, after the copies of stage
        // g (during step g - 2): the stores of the tile step g - 2 closed, the copies of stage g + 1, the stores of the
        // tile step g - 1 closed -- whichever of those exist. Exactly that many may still be outstanding.
        // DS: stage g + 1 has B_ROWS more copies when step g + 1 is a centre-tap step. The counts below take it for a plain step --
        // the smaller count: where it is a centre-tap step the wait also covers the first B_ROWS copies of stage g + 1, issued a whole
        // k-step ago (it over-waits, it never under-waits). The extra copies of stage g ITSELF are older than everything counted.
        const bool next = g + 1 < total;
        int closed = 0;
        if (ks == 0 && g > 0) closed = 1;
        if ((nk == 1 || ks == 1) && g > 1) ++closed;
        if (next) {
            if (closed == 2) pg_wait_vm<NLD + 2 * NST>();
            else if (closed == 1) pg_wait_vm<NLD + NST>();
            else pg_wait_vm<NLD>();
        } else {
            if (closed == 2) pg_wait_vm<2 * NST>();
            else if (closed == 1) pg_wait_vm<NST>();
            else pg_wait_vm<0>();
        }
        __builtin_amdgcn_s_barrier();   // every wave's share of stage g is in LDS; every wave is done with stage g - 1
        if (STAMP && ks == 0 && t < 15) stamp(3 + 4 * t);
        const int slot2 = slot == 0 ? 2 : slot - 1;   // (g + 2) % 3 == (g - 1) % 3
        if (g + 2 < total) issue(slot2);
        __builtin_amdgcn_sched_barrier(0);
    };
    // (a wave's LDS reads of a stage are complete before it reaches the next barrier, behind which the stage is overwritten:
    // every one of them fed a matrix instruction)
    for (int t = 0; t < nt; ++t) {
        const int tile_m = run.tile(t);
        if (t < 15) stamp(2 + 4 * t);
        pre(0, t);
        kstep(slot * (STAGE * 4), std::true_type{}, std::integral_constant<int, 0>{});   // (k-step 0 is tap (0, 0), never the centre)
        slot = slot == 2 ? 0 : slot + 1;
        ++g;
        for (int ks = 1; ks < nk; ++ks, ++g) {
            pre(ks, t);
            if (DS && ks == c_lo) kstep(slot * (STAGE * 4), std::false_type{}, std::integral_constant<int, 1>{});
            else if (DS && ks > c_lo && ks < c_hi) kstep(slot * (STAGE * 4), std::false_type{}, std::integral_constant<int, 2>{});
            else kstep(slot * (STAGE * 4), std::false_type{}, std::integral_constant<int, 0>{});
            slot = slot == 2 ? 0 : slot + 1;
        }
        if (t < 15) stamp(4 + 4 * t);
        // epilogue of the tile, straight from the accumulators: lane = pixel lr of its 32-pixel block, channels ch0 + 8 g + 0..3
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            if (GRP) acc[mi] = (acc[mi] + accg[0][mi]) + (accg[GRP ? 1 : 0][mi] + accg[GRP ? 2 : 0][mi]);
            const int m_base = tile_m * BM + wm * (BM / WM) + mi * 32;
            const int o_off = out_offset(m_base);
            float* o_px = p.out + o_off;
            const bool live = m_base + lr < p.M;
            f32x4 out4[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x2 lo = f32x2{acc[mi][4 * gq], acc[mi][4 * gq + 1]}, hi = f32x2{acc[mi][4 * gq + 2], acc[mi][4 * gq + 3]};   // (bias inside)
                if (SILU) {   // x * 1 / (1 + 2^(-x log2 e)), as silu_fast
                    const f32x2 tl = lo * nl2e, th = hi * nl2e;
                    const f32x2 dl = f32x2{__builtin_amdgcn_exp2f(tl.x), __builtin_amdgcn_exp2f(tl.y)} + one2;
                    const f32x2 dh = f32x2{__builtin_amdgcn_exp2f(th.x), __builtin_amdgcn_exp2f(th.y)} + one2;
                    lo *= f32x2{__builtin_amdgcn_rcpf(dl.x), __builtin_amdgcn_rcpf(dl.y)};
                    hi *= f32x2{__builtin_amdgcn_rcpf(dh.x), __builtin_amdgcn_rcpf(dh.y)};
                } else if (p.relu == 1) {
                    lo.x = lo.x > 0.f ? lo.x : 0.f; lo.y = lo.y > 0.f ? lo.y : 0.f;
                    hi.x = hi.x > 0.f ? hi.x : 0.f; hi.y = hi.y > 0.f ? hi.y : 0.f;
                }
                // (rows past M of a partial last tile were computed on pixel M - 1 and are dropped)
                // INVARIANT the counted waits rely on: a wave whose rows are all past M issues NO stores here (hipcc branches
                // around them), so its vmcnt(NLD + k * NST) would under-wait if another k-step of this workgroup followed. None
                // does: a workgroup walks its tiles in ASCENDING order (TileRun: first, + step, ...) and only the launch's last tile
                // (tiles_m - 1) can be partial, so a partial tile is always the last thing its workgroup computes. Any other
                // tile order must first make the store count independent of the predicate (launch_pgemm checks the premise). That the
                // compiler emits exactly NST 16-byte stores per tile is checked on the built object
                // (tests/test_abi.py::test_pgemm_store_count_matches_the_counted_waits); psgemm.hip, the emulated-fp32 form of this
                // kernel, issues its stores unconditionally through a bounds-checked buffer descriptor instead.
                if (live) *reinterpret_cast<f32x4*>(o_px + 8 * gq) = f32x4{lo.x, lo.y, hi.x, hi.y};
                if (UP) { out4[gq] = f32x4{lo.x, lo.y, hi.x, hi.y}; }
            }
            if (DS && live) {   // the branch: no bias, no activation, the same pixels and channels of out2 (NST counts these four too)
                float* o2_px = p.out2 + o_off;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                    *reinterpret_cast<f32x4*>(o2_px + 8 * gq) = f32x4{acc2[mi][4 * gq], acc2[mi][4 * gq + 1], acc2[mi][4 * gq + 2], acc2[mi][4 * gq + 3]};
            }
            if (UP && live) {   // (a launch with an up-sampled copy has no partial tile followed by a k-step either: same invariant)
                float* u_px = p.up_out + pixel_walk(geom, m_base, lr, p.up_img_stride, up_rs, up_ps, up_wrap_x, up_wrap_y, up_lane);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    float* u = u_px + (q4 >> 1) * p.up_row_stride + (q4 & 1) * p.up_px_stride;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) *reinterpret_cast<f32x4*>(u + 8 * gq) = out4[gq];
                }
            }
        }
        if (t < 15) stamp(5 + 4 * t);
    }
    stamp(63);
}

template <int BM, int BN = 64, bool SILU = true, bool STAMP = false, bool UP = false>
__global__ __launch_bounds__(256, 2) void pgemm_kernel(const GemmParams p) {
    pgemm_body<BM, BN, SILU, STAMP, UP, false>(p);
}

// the opener form: ReLU (p.relu) or none on out, the raw branch sums on out2; 64 x 64 tiles (three stages of 192 rows: 72 KiB, two
// workgroups per CU)
__global__ __launch_bounds__(256, 2) void pgemm_branch_kernel(const GemmParams p) {
    pgemm_body<64, 64, false, false, false, true>(p);
}

// the grouped form: no bias, no activation (launch_pgemm_grouped)
template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void pgemm_group_kernel(const GemmParams p) {
    pgemm_body<BM, BN, false, false, false, false, true>(p);
}

// Conv mode of GemmParams (no gather, no second source, no residual, no split-K); bm = 128 | 64 | 0 (chosen here).
// p.wgt2 / p.out2 (both or neither): the opener form -- a 3x3 stride-2 convolution whose tap is the whole pixel (chunk == in_px_stride: the
// channels the branch reads), ReLU or no activation, no up-sampled copy, 64 x 64 tiles; anything else is refused.
hipError_t launch_pgemm(const GemmParams& p_in, int bm, hipStream_t s) {
    GemmParams p = p_in;
    if (p.residual || p.N % 32 != 0 || (bm != 128 && bm != 64 && bm != 0) || persistent_plan(p) != hipSuccess) return hipErrorInvalidValue;
    const bool branch = p.wgt2 || p.out2;
    if (branch) {
        if (!p.wgt2 || !p.out2 || p.taps != 9 || p.kw_taps != 3 || p.stride != 2 || p.in_px_stride != p.chunk || p.splitk > 1 || p.N % 64 != 0 || p.relu == 2 || p.up_out ||
            ((reinterpret_cast<unsigned long long>(p.wgt2) | reinterpret_cast<unsigned long long>(p.out2)) & 15ull))
            return hipErrorInvalidValue;
        bm = 64;
    }
    const int bn = p.N % 64 == 0 ? 64 : 32;   // 32: output channels that are not a multiple of 64 (128-row tiles only)
    if (bn == 32) bm = 128;
    p.tiles_n = p.N / bn;
    if (p.tiles_n > 64) return hipErrorInvalidValue;
    // Two workgroups per CU = 64 per XCD, a multiple of the channel columns, and no more per column than the XCD's share
    // of pixel tiles. bm = 0: the tile height whose slowest workgroup finishes first.
    auto plan = [&](int bm_, int* lm_out) {   // -> relative time of the slowest workgroup
        const int tm = (p.M + bm_ - 1) / bm_, share = (tm + 7) / 8;
        int lm = 64 / p.tiles_n;
        lm = lm < 1 ? 1 : (lm > share ? share : lm);
        *lm_out = lm;
        // tiles of its slowest workgroup x cost of a tile (a 64-row tile: half the matrix work + the same copies of the
        // weights), and a workgroup alone on its CU (<= 32 per XCD) runs ~1.6x as fast as one of a pair
        return (double)((share + lm - 1) / lm) * (bm_ == 128 ? 1.0 : 0.55) * (lm * p.tiles_n <= 32 ? 0.6 : 1.0);
    };
    int lm = 1;
    if (bm == 0) {
        int lm128, lm64;
        const double e128 = plan(128, &lm128), e64 = plan(64, &lm64);
        bm = e128 <= e64 ? 128 : 64;
        lm = bm == 128 ? lm128 : lm64;
    } else {
        (void)plan(bm, &lm);
    }
    p.tiles_m = (p.M + bm - 1) / bm;
    // the premise of the kernel's counted waits (see its store loop): every tile but the last is full
    if ((long long)(p.tiles_m - 1) * bm >= p.M || (long long)p.tiles_m * bm < p.M) return hipErrorInvalidValue;
    const int per = lm * p.tiles_n;
    const int grid = per * 8;
    p.pg_per = per;
    const bool silu = p.relu == 2;
    // diagnostic: PA_PG_STAMP_FILE=<path> PA_PG_STAMP_SHAPE=M,K,N [PA_PG_STAMP_SKIP=n]: the (n + 1)-th launch of that shape runs
    // the stamped kernel and its per-wave clock stamps are written to the file (synchronises; scripts/pgemm_stamps.py)
    static const char* stamp_file = getenv("PA_PG_STAMP_FILE");
    if (stamp_file && bm == 128 && bn == 64 && silu && !branch) {
        static int sm = 0, sk = 0, sn = 0, skip = getenv("PA_PG_STAMP_SKIP") ? atoi(getenv("PA_PG_STAMP_SKIP")) : 3, seen = 0;
        if (!sm && getenv("PA_PG_STAMP_SHAPE")) sscanf(getenv("PA_PG_STAMP_SHAPE"), "%d,%d,%d", &sm, &sk, &sn);
        if (p.M == sm && p.ktot == sk && p.N == sn && seen++ == skip) {
            const size_t n = (size_t)grid * 4 * 64;
            unsigned long long* d = nullptr;
            if (hipMalloc(&d, n * 8) != hipSuccess) return hipErrorOutOfMemory;
            (void)hipMemsetAsync(d, 0, n * 8, s);
            p.clk = d;
            hipLaunchKernelGGL((pgemm_kernel<128, 64, true, true>), dim3(grid), dim3(256), 0, s, p);
            std::vector<unsigned long long> hst(n);
            (void)hipStreamSynchronize(s);
            (void)hipMemcpy(hst.data(), d, n * 8, hipMemcpyDeviceToHost);
            (void)hipFree(d);
            if (FILE* f = fopen(stamp_file, "wb")) {
                const int hdr[4] = {grid, p.ktot / 32, p.tiles_m, p.tiles_n};
                fwrite(hdr, 4, 4, f);
                fwrite(hst.data(), 8, n, f);
                fclose(f);
            }
            return hipGetLastError();
        }
    }
#define PA_PG_LAUNCH(BM_, BN_)                                                                               \
    do {                                                                                                     \
        if (p.up_out) hipLaunchKernelGGL((pgemm_kernel<BM_, BN_, true, false, true>), dim3(grid), dim3(256), 0, s, p); \
        else if (silu) hipLaunchKernelGGL((pgemm_kernel<BM_, BN_, true>), dim3(grid), dim3(256), 0, s, p);   \
        else hipLaunchKernelGGL((pgemm_kernel<BM_, BN_, false>), dim3(grid), dim3(256), 0, s, p);            \
    } while (0)
    if (p.up_out && (!silu || p.up_px_stride % 4 || p.up_row_stride % 4 || p.up_img_stride % 4 || (reinterpret_cast<unsigned long long>(p.up_out) & 15ull)))
        return hipErrorInvalidValue;   // (the up-sampled copy exists for SiLU layers only)
    if (branch) hipLaunchKernelGGL(pgemm_branch_kernel, dim3(grid), dim3(256), 0, s, p);
    else if (bn == 32) PA_PG_LAUNCH(128, 32);
    else if (bm == 128) PA_PG_LAUNCH(128, 64);
    else PA_PG_LAUNCH(64, 64);
#undef PA_PG_LAUNCH
    return hipGetLastError();
}

// The groups as "images" of a 1x1 convolution over a rows x 1 map: pixel m = (group, row), whole tiles per group, so activations and
// outputs are one contiguous [groups * rows][K] / [..][N] matrix and only the weight image moves with the group. Grid as launch_pgemm.
hipError_t launch_pgemm_grouped(const float* a, const float* w, float* out, int groups, int rows, int K, int N, int tile, hipStream_t s) {
    auto mis = [](const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) != 0; };
    if (!a || !w || !out || mis(a) || mis(w) || mis(out) || groups < 1 || rows < 64 || rows % 64 || rows >= (1 << 16) || K < 32 || K % 32 || N < 64 || N % 64 ||
        tile < 0 || tile > 3)
        return hipErrorInvalidValue;
    // byte offsets inside the buffer descriptors are 32-bit
    if ((long long)groups * rows * K * 4 >= (1ll << 31) || (long long)groups * N * K * 4 >= (1ll << 31) || (long long)groups * rows * N >= (1ll << 31))
        return hipErrorInvalidValue;
    // 64 x 64 tiles: the fastest of the three at ResNet-18's layer 4 and 128 crops (profiles/wino_f4_parent_ab.md); the 128-row tiles
    // need groups of whole 128-row tiles
    if (tile == 0) tile = 1;
    if (tile != 1 && rows % 128) tile = 1;
    const int bm = tile == 1 ? 64 : 128, bn = tile == 3 ? 32 : 64;
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.act = a; p.wgt = w; p.out = out;
    p.M = groups * rows; p.N = N; p.ktot = K;
    p.taps = 1; p.kw_taps = 1; p.chunk = K;
    p.howo = rows; p.wo = rows;
    p.in_px_stride = K; p.in_row_stride = rows * K; p.in_img_stride = rows * K; p.stride = 1;
    p.out_px_stride = N; p.out_row_stride = rows * N; p.out_img_stride = rows * N;
    p.splitk = 1;
    if (persistent_plan(p) != hipSuccess) return hipErrorInvalidValue;
    p.tiles_n = N / bn;
    p.tiles_m = p.M / bm;
    if (p.tiles_n > 64) return hipErrorInvalidValue;
    p.grp_tiles = rows / bm;
    p.grp_wgt_bytes = N * K * 4;
    p.grp_magic = (unsigned)std::min<unsigned long long>(((1ull << 32) + p.grp_tiles - 1) / p.grp_tiles, 0xffffffffull);
    // Workgroups per channel column and XCD: up to 96 per XCD -- the 64 x 64 kernel's registers and 48 KiB of LDS let three share a CU --
    // so that at ResNet-18's layer 4 and 128 crops (9 pixel tiles x 8 columns per XCD) every workgroup has ONE tile: 576 workgroups took
    // 43.9 us where 512, an eighth of them with two tiles, took 46.1 (the whole layer, profiles/wino_f4_parent_ab.md)
    const int share = (p.tiles_m + 7) / 8;
    int lm = 96 / p.tiles_n;
    static const int lm_force = getenv("PA_PGEMM_GROUP_LM") ? atoi(getenv("PA_PGEMM_GROUP_LM")) : 0;   // A/B: workgroups per channel column and XCD
    if (lm_force > 0) lm = lm_force;
    lm = lm < 1 ? 1 : (lm > share ? share : lm);
    p.pg_per = lm * p.tiles_n;
    const int grid = p.pg_per * 8;
    if (tile == 1) hipLaunchKernelGGL((pgemm_group_kernel<64, 64>), dim3(grid), dim3(256), 0, s, p);
    else if (tile == 2) hipLaunchKernelGGL((pgemm_group_kernel<128, 64>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((pgemm_group_kernel<128, 32>), dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace pa

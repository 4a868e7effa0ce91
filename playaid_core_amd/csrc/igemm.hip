// Implicit-GEMM convolution / linear engine for gfx950 (MI355X), exact fp32.
//
// One kernel family carries every FLOP-heavy layer of the path
// (cnn_action_detector.py:14-43 in the reference): the 7x7/2 stem, the sixteen
// 3x3 convolutions and three 1x1/2 downsamples of ResNet-18, the 512->1000 fc,
// the temporal Conv1d(1000->512, k=S) over cached features (gather mode) and --
// through the same code -- nothing else. BatchNorm is folded into the weights
// on the host, bias + residual + ReLU are fused into the epilogue.
//
// Structure (CDNA4):
//   * workgroup = 256 threads = 4 wave64 arranged 2x2 over a BM x BN tile;
//   * the im2col A-tile (BM output pixels x 32 k-values) and the weight B-tile
//     (BN channels x 32 k-values) go global -> LDS directly with
//     global_load_lds_dwordx4 (no VGPR round trip, no ds_write: measured 15-18 %
//     of the loop in the register-staged version); NHWC activations carry an
//     explicit zero border so the gather is pure address arithmetic (no
//     predicates); two LDS stages, the loads of k-step k+1 are issued before
//     the MFMAs of step k, one barrier per step;
//   * an LDS-DMA wave instruction writes 1 KiB lane-linear (8 rows x 128 B), so
//     rows cannot be padded; bank conflicts are removed by an XOR swizzle on
//     the SOURCE address instead: LDS chunk c of row r holds logical 16-byte
//     chunk c ^ ((r >> 1) & 7), and the ds_read_b128 operand reads apply the
//     same XOR (16-lane groups, bank = dword % 64: conflict-free);
//   * the inner product runs on v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate,
//     bit-identical to an fmaf chain, at the same peak as the f32 VALU but with
//     one operand VGPR per lane (guide: cdna_hip_programming.md section 3,
//     "FP32-input MFMA"). Each lane reads 4 consecutive k of its row with one
//     ds_read_b128 and feeds them to 4 consecutive MFMAs; lanes 0-31 take
//     k = 8j..8j+3, lanes 32-63 take k = 8j+4..8j+7 of each 8-wide k group.
//   * blockIdx is remapped so that the workgroups sharing an XCD (b % 8) own a
//     contiguous run of tiles (same A rows, neighbouring weight panels) in that
//     XCD's private L2;
//   * deterministic split-K (slabs + ordered reduce) for the small-M layers.
#include "tile_common.h"
#include <cstdio>
#include <cstdlib>

namespace pa {

#ifndef PA_COUNTED_VMCNT
#define PA_COUNTED_VMCNT 0
#endif

// ABL: timing-only ablation bits for scripts/ablate_igemm.sh (results are wrong when != 0):
//   1 no global->LDS loads, 4 no barriers in the loop, 8 no MFMAs.
// SKIPW: every 4th k carries a zero weight (the stem's channel pad, k = ky*32 + kx*4 + c with c < 3),
// so the MFMA of each fragment's .w component is dropped -- 25 % fewer matrix instructions.
template <int BM, int BN, int BK, bool GATHER, int ABL = 0, bool SKIPW = false>
__global__ __launch_bounds__(256) void igemm_f32_kernel(const GemmParams p) {
    constexpr int MI = BM / 64;  // 32x32 MFMA tiles per wave along M
    constexpr int NI = BN / 64;
    using Stage = Im2colStage<4, BK, BM, BN, GATHER>;  // tile decode, staging offsets, k-step cursor (tile_common.h)
    constexpr int LDS_STRIDE = BK;       // floats per LDS row (unpadded: LDS-DMA writes are lane-linear)
    constexpr int A_ROWS = Stage::A_ROWS, B_ROWS = Stage::B_ROWS;  // staging rows per thread
    constexpr int STAGE = (BM + BN) * LDS_STRIDE;  // floats per LDS stage
    __shared__ __attribute__((aligned(16))) float lds[3 * STAGE];

    Stage st;
    st.setup(p);
    const int tile_m = st.tile_m, tile_n = st.tile_n, z = st.z;
    const int ks_begin = st.ks_begin, ks_end = st.ks_end;
    const int tid = threadIdx.x;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Issue the LDS-DMA loads of the k-step under the cursor into stage BUF, then advance the cursor. Each wave instruction
    // fills 1 KiB (8 or 4 rows).
#define PA_ISSUE_STAGE(BUF)                                                \
    {                                                                      \
        float* As_w = lds + (BUF) * STAGE + wave_id * 256;                 \
        st.issue(p, As_w, As_w + BM * LDS_STRIDE);                         \
    }

    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31;  // MFMA row (A) / column (B) of this lane
    const int lh = lane >> 5;  // which k of the pair

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

    const int a_rd_off = (wm * (BM / 2) + lr) * LDS_STRIDE;
    const int b_rd_off = BM * LDS_STRIDE + (wn * (BN / 2) + lr) * LDS_STRIDE;
    const int swz = BK == 32 ? ((lr >> 1) & 7) : (lr & 15);  // row-dependent chunk XOR (same for every 32-row MFMA tile)

    // The epilogue moves the tile through LDS so that every thread stores 16 bytes (see below):
    // thread t owns channels [c4, c4+4) of rows r_t + ROWS_PP * i. Its bias / residual operands
    // are fetched now, so their latency hides under the whole k loop.
    constexpr int TS = BN;                 // row of the transposed tile (floats): unpadded is the conflict-free choice
                                           // for ds_read_b128's lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31}
    constexpr int CPR = BN / 4;            // 16-byte chunks per row
    constexpr int ROWS_PP = 256 / CPR;     // rows covered by one pass of the 256 threads
    constexpr int EP_IT = BM / ROWS_PP;
    static_assert(BM * TS <= 3 * STAGE, "transposed tile must fit the LDS ring");
    const bool direct_out = p.splitk <= 1;
    const int c4 = (tid & (CPR - 1)) * 4;
    const int r_t = tid / CPR;
    int o_t[EP_IT];
    f32x4 res_t[EP_IT];
#pragma unroll
    for (int i = 0; i < EP_IT; ++i) {
        int m = tile_m * BM + r_t + ROWS_PP * i;
        m = m < p.M ? m : p.M - 1;
        int img, oy, ox;
        split_m(p, m, img, oy, ox);
        o_t[i] = img * p.out_img_stride + (oy + p.out_pad) * p.out_row_stride + (ox + p.out_pad) * p.out_px_stride +
                 tile_n * BN + c4;
        res_t[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (direct_out && p.residual) {
#pragma unroll
        for (int i = 0; i < EP_IT; ++i) res_t[i] = *reinterpret_cast<const f32x4*>(p.residual + o_t[i]);
    }
    f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (direct_out && p.bias) bias4 = *reinterpret_cast<const f32x4*>(p.bias + tile_n * BN + c4);

    // Three-stage LDS ring, one barrier per k-step, no post-barrier bubble:
    //   step k: issue LDS-DMA of step k+2 into stage (k+2)%3
    //           MFMAs of step k from stage k%3; operand fragments are read one
    //           8-wide k group ahead, and the LAST group of the step already
    //           reads the first fragments of step k+1 from stage (k+1)%3
    //           __syncthreads()  (hipcc drains the DMA with vmcnt(0) first)
    // RAW: stage (k+1)%3 was drained + barriered at the end of step k-1, so it is
    //      visible to every wave during step k.
    // WAR: the DMA of step k+3 (issued in step k+1) overwrites stage k%3, whose
    //      last reads every wave completed before the barrier that ends step k.
    f32x4 af[2][MI], bf[2][NI];
#define PA_LOAD_FRAGS(SET, STAGE_PTR, KK)                                                                     \
    {                                                                                                         \
        const int ch = (((KK) * 2 + lh) ^ swz) * 4;                                                           \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                                     \
            af[SET][mi] = *reinterpret_cast<const f32x4*>((STAGE_PTR) + a_rd_off + mi * 32 * LDS_STRIDE + ch); \
        _Pragma("unroll") for (int ni = 0; ni < NI; ++ni)                                                     \
            bf[SET][ni] = *reinterpret_cast<const f32x4*>((STAGE_PTR) + b_rd_off + ni * 32 * LDS_STRIDE + ch); \
    }
#ifdef PA_ABLATION_BUILD
    const unsigned long long clk_t0 = __builtin_amdgcn_s_memtime(), clk_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (ks_begin < ks_end) PA_ISSUE_STAGE(0);
    if (ks_begin + 1 < ks_end) PA_ISSUE_STAGE(1);
    __syncthreads();
    if (ks_begin < ks_end) PA_LOAD_FRAGS(0, lds, 0);
    int buf = 0;
    for (int ks = ks_begin; ks < ks_end; ++ks) {
        if (PA_COUNTED_VMCNT && ks > ks_begin) PA_LOAD_FRAGS(0, lds + buf * STAGE, 0);
        const int buf1 = buf == 2 ? 0 : buf + 1;
        const int buf2 = buf1 == 2 ? 0 : buf1 + 1;
        if (ks + 2 < ks_end && !(ABL & 1)) PA_ISSUE_STAGE(buf2);
        const bool has_next = ks + 1 < ks_end;
        // pin the issue order: hipcc otherwise sinks the loads below the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        const float* st_cur = lds + buf * STAGE;
        const float* st_next = lds + buf1 * STAGE;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            // The next group's reads are issued after the first two MFMAs of this
            // group (pinned with sched_barrier): >= 128 cycles of MFMA pipe time
            // remain to cover the LDS latency, and the lgkmcnt(0) hipcc puts in
            // front of the next group never waits on a read that was just issued.
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const f32x4 a4 = af[kk & 1][mi], b4 = bf[kk & 1][ni];
                    if (!(ABL & 8)) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc[mi][ni], 0, 0, 0);
                    } else {
                        acc[mi][ni][0] += a4.x * b4.x + a4.y * b4.y + a4.z * b4.z + a4.w * b4.w;
                    }
                    if (mi == 0 && ni == 0) {
                        __builtin_amdgcn_sched_barrier(0);
                        if (kk + 1 < BK / 8) {
                            PA_LOAD_FRAGS((kk + 1) & 1, st_cur, kk + 1);
                        } else if (has_next && !PA_COUNTED_VMCNT) {
                            PA_LOAD_FRAGS(0, st_next, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (!(ABL & 8)) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc[mi][ni], 0, 0, 0);
                        if (!SKIPW) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc[mi][ni], 0, 0, 0);
                    }
                }
        }
        if (!(ABL & 4)) {
            if (PA_COUNTED_VMCNT) {
                // leave the stage issued in THIS step in flight across the barrier: only the older
                // stage (needed next step) must have landed. __syncthreads() would drain to vmcnt(0).
                if (ks + 2 < ks_end) wait_vmcnt<A_ROWS + B_ROWS>();
                else wait_vmcnt<0>();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            } else {
                __syncthreads();
            }
        }
        buf = buf1;
    }
#undef PA_LOAD_FRAGS
#undef PA_ISSUE_STAGE
#ifdef PA_ABLATION_BUILD
    if (p.clk && tid == 0 && blockIdx.x == gridDim.x / 2) {
        p.clk[0] = __builtin_amdgcn_s_memtime() - clk_t0;
        p.clk[1] = __builtin_amdgcn_s_memrealtime() - clk_r0;
    }
#endif

    // Epilogue. The accumulators hold one output channel per lane (32x32 C/D map: col = lane & 31,
    // row = (e & 3) + 8*(e >> 2) + 4*(lane >> 5)): stored directly that is 16*MI*NI four-byte stores
    // per lane, and since every workgroup of a launch reaches its epilogue at about the same time
    // the stores queue up (timeline stamps: 8 us median, 16 us worst, of a 46 us workgroup). The
    // tile is therefore transposed through the (now idle) LDS ring -- rows of BN floats -- and each
    // thread moves 16 bytes per row: EP_IT dwordx4 stores (and residual loads) instead.
    float* const tbuf = lds;  // every wave left the k loop through its final barrier
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * (BM / 2) + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                tbuf[row * TS + wn * (BN / 2) + ni * 32 + lr] = acc[mi][ni][e];
            }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EP_IT; ++i) {
        const int row = r_t + ROWS_PP * i;
        const int m = tile_m * BM + row;
        if (m >= p.M) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(tbuf + row * TS + c4);
        if (!direct_out) {
            *reinterpret_cast<f32x4*>(p.slab + ((size_t)z * p.M + m) * p.N + tile_n * BN + c4) = v;
        } else {
            *reinterpret_cast<f32x4*>(p.out + o_t[i]) = epilogue4(v, bias4, res_t[i], p.relu, p.res_after);
        }
    }
}

// Ordered (deterministic) split-K reduction with the fused epilogue: the fp32 slabs summed in split order, + bias, + residual,
// activation, stored as OutT. The sum is (slabs + bias) + residual -- the tile epilogues add slabs + (bias + residual) -- so of
// epilogue4 only act4 is shared. float: ReLU / SiLU, residual before or after the activation; bf16_t (igemm_bf16.hip's layers): bf16
// residual before the activation, any non-zero relu is ReLU. (The body stands in the kernel itself: behind a helper that takes the
// parameters by reference both instances need two more registers.)
template <typename OutT> __global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p) {
    constexpr bool BF16 = sizeof(OutT) == 2;
    const OutT* residual = reinterpret_cast<const OutT*>(p.residual);
    OutT* out = reinterpret_cast<OutT*>(p.out);
    const int n4 = p.N >> 2;
    const size_t total = (size_t)p.M * n4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / n4);
        const int n = (int)(i - (size_t)m * n4) * 4;
        f32x4 s = *reinterpret_cast<const f32x4*>(p.slab + (size_t)m * p.N + n);
        for (int z = 1; z < p.splitk; ++z) s += *reinterpret_cast<const f32x4*>(p.slab + ((size_t)z * p.M + m) * p.N + n);
        int img, oy, ox;
        split_m(p, m, img, oy, ox);
        const size_t o = (size_t)img * p.out_img_stride + (size_t)(oy + p.out_pad) * p.out_row_stride +
                         (size_t)(ox + p.out_pad) * p.out_px_stride + n;
        if (p.bias) s += *reinterpret_cast<const f32x4*>(p.bias + n);
        if constexpr (BF16) {
            if (residual) {
                const ushort4 rv = *reinterpret_cast<const ushort4*>(residual + o);
                s += f32x4{bf16_to_f32(rv.x), bf16_to_f32(rv.y), bf16_to_f32(rv.z), bf16_to_f32(rv.w)};
            }
            s = act4(s, p.relu ? 1 : 0);
            ushort4 ov;
            ov.x = f32_to_bf16(s.x); ov.y = f32_to_bf16(s.y); ov.z = f32_to_bf16(s.z); ov.w = f32_to_bf16(s.w);
            *reinterpret_cast<ushort4*>(out + o) = ov;
        } else {
            f32x4 rv = f32x4{0.f, 0.f, 0.f, 0.f};
            if (residual) rv = *reinterpret_cast<const f32x4*>(residual + o);
            if (!p.res_after) s += rv;
            s = act4(s, p.relu);
            if (p.res_after) s += rv;
            *reinterpret_cast<f32x4*>(out + o) = s;
        }
    }
}

template <int BM, int BN, int BK>
static hipError_t launch_tile(const GemmParams& p, hipStream_t s) {
    const int grid = p.tiles_m * p.tiles_n * p.splitk;
#ifdef PA_ABLATION_BUILD
    static const int abl = getenv("PA_ABLATE") ? atoi(getenv("PA_ABLATE")) : 0;
    static unsigned long long* clk_dev = nullptr;
    static int clk_calls = 0;
    if (getenv("PA_CLK") && !p.gather) {
        if (!clk_dev) (void)hipMalloc(&clk_dev, 16);
        GemmParams q = p;
        q.clk = clk_dev;
        hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, BK, false, 0>), dim3(grid), dim3(256), 0, s, q);
        if (++clk_calls % 97 == 0) {
            unsigned long long h[2];
            (void)hipMemcpy(h, clk_dev, 16, hipMemcpyDeviceToHost);
            fprintf(stderr, "[igemm clk] tile %dx%dx%d M=%d N=%d K=%d: %llu cycles / %llu x10ns -> %.3f GHz\n", BM, BN, BK, p.M, p.N, p.ktot, h[0], h[1], (double)h[0] / (double)h[1] * 0.1);
        }
        return hipGetLastError();
    }
    if (!p.gather && abl) {
#define PA_ABL_CASE(V) case V: hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, BK, false, V>), dim3(grid), dim3(256), 0, s, p); return hipGetLastError();
        switch (abl) { PA_ABL_CASE(1) PA_ABL_CASE(4) PA_ABL_CASE(5) PA_ABL_CASE(8) PA_ABL_CASE(9) PA_ABL_CASE(12) default: break; }
    }
#endif
    if (p.gather)
        hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, BK, true>), dim3(grid), dim3(256), 0, s, p);
    else if (p.skip_w && BK == 32 && BN == 64)
        hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, (BN == 64 ? 32 : BK), false, 0, (BN == 64 && BK == 32)>), dim3(grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((igemm_f32_kernel<BM, BN, BK, false>), dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_igemm(const GemmParams& p_in, GemmTile tile, hipStream_t s) {
    GemmParams p = p_in;
    TileDims d = tile_dims(tile, 4);
    if (p.chunk % d.bk != 0 || p.k2_steps) {  // 32-wide taps (stem) or a fused second source: BK=32 shapes only
        tile = tile == TILE_128x64_K64 ? TILE_128x64 : TILE_64x64;
        d = tile_dims(tile, 4);
    }
    const int bm = d.bm, bn = d.bn, bk = d.bk;
    if (p.N % bn != 0 || p.chunk % bk != 0 || p.ktot != p.taps * p.chunk + p.k2_steps * 32 || p.M <= 0) return hipErrorInvalidValue;
    if (p.k2_steps && (bk != 32 || !p.act2 || p.gather)) return hipErrorInvalidValue;
    fill_pow2_shifts(p);
    p.tiles_m = (p.M + bm - 1) / bm;
    p.tiles_n = p.N / bn;
    plan_splitk(p.ktot / bk, p.splitk, p.ksteps_per_split);
    hipError_t err;
    switch (tile) {
        case TILE_128x128: err = launch_tile<128, 128, 32>(p, s); break;
        case TILE_128x64: err = launch_tile<128, 64, 32>(p, s); break;
        case TILE_64x64: err = launch_tile<64, 64, 32>(p, s); break;
        case TILE_128x64_K64: err = launch_tile<128, 64, 64>(p, s); break;
        default: err = launch_tile<64, 64, 64>(p, s); break;
    }
    if (err != hipSuccess) return err;
    if (p.splitk_used) *p.splitk_used = p.splitk;
    if (p.splitk > 1 && !p.defer_reduce) return launch_splitk_reduce(p, s);
    return hipSuccess;
}

hipError_t launch_splitk_reduce(const GemmParams& p, hipStream_t s, bool out_bf16) {
    const size_t total = (size_t)p.M * (p.N >> 2);
    int grid = (int)((total + 255) / 256);
    if (grid > 2048) grid = 2048;
    if (out_bf16) hipLaunchKernelGGL(splitk_reduce_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(splitk_reduce_kernel<float>, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace pa

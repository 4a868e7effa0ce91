// The 7x7/2 stem + BatchNorm + ReLU + 3x3/2 max-pool of stem_pool.hip for a square input of ANY size S (S % 32 == 0,
// 64 .. 512): table kind 3 of csrc/convnet.hip. stem_pool_kernel is laid out for one size -- a stem row of exactly 64 pixels is
// one tile, its 9 x 134-pixel patch one contiguous block of the crop that LDS-DMA copies whole -- and stays the 128 path.
//
// Here a stem row is S / 2 pixels (32 at S = 64, 48 at 96, 128 at 256, 256 at 512), so a tile is two stem rows x 64 stem
// COLUMNS: a workgroup takes a run of at most 16 row pairs of one crop and walks it once per column tile, the ceil(S / 128)
// tiles from left to right, each from the run's top row pair down. What the pooling needs across tile edges is carried, never
// recomputed:
//   * down the rows, the horizontal 3-max of the pair's second stem row (stem row 2r + 1 is pooled row r + 1's top row): in
//     registers, as in stem_pool_kernel; a run that does not start at the top of the crop first computes the pair above it
//     without storing (one warm-up tile per column tile of the run);
//   * across a column seam, stem column 64 t - 1 of every stem row of the run: a small LDS table (2 x 17 rows x 64 channels)
//     that tile t - 1 leaves behind and tile t copies into column 0 of the transposed stem tile, which has 65 pixel columns
//     (zero left of the first tile: after the ReLU a zero is the pool's -inf padding).
// A partial last tile (S / 2 is a multiple of 16, not of 64) computes all 64 columns -- its patch reads zeros right of the
// padded input row -- and masks the stores: pooled pixel p of the crop reads stem columns 2 p - 1 .. 2 p + 1 <= S / 2 - 1, so
// no stored value ever sees a column past the map. Only the interior of the [S / 4 + 2]^2 x 64 output is written; its zero
// border is the buffer's.
//
// The patch is staged PER COLUMN TILE: 9 input rows x 134 pixels x 16 B = 19 KB (full-width patches would be 9 x 518 x 16 B =
// 75 KB each at S = 512: no room for two). A tile's patch is not contiguous in the crop (134 of S + 6 pixels of each row, and
// the last tile's rows end early), so it goes global -> registers -> LDS, the next tile's loads issued before this tile's
// matrix instructions and stored behind them; with 19 KB + 33 KB + 9 KB of LDS two workgroups share a CU and cover each
// other's barriers. The product itself is stem_pool_kernel's fp32 form: the weights of the lane's output channel resident in
// registers, K = 7 x 7 x 3 = 147 as 25 steps of two taps on v_mfma_f32_32x32x2_f32, operands read straight out of the patch
// as overlapping windows, XOR-swizzled 16-byte chunks; the same (tap, channel) summation order.
#include "tile_common.h"

namespace pa {

namespace {

constexpr int SA_PW = 134;             // patch pixels per input row: 2 * 64 stem columns + 7 taps - 1
constexpr int SA_PATCH_CH = 9 * SA_PW;  // 2 stem rows x stride 2 + 7 taps - 2 = 9 input rows
constexpr int SA_PASSES = (SA_PATCH_CH + 255) / 256;
constexpr int SA_TS = 64;              // floats per pixel of the transposed stem tile
constexpr int SA_TCOLS = 65;           // its pixel columns: the seam column, then the tile's 64
constexpr int SA_MAX_RUN = 16;         // row pairs per run at most (the seam table's size)
constexpr int SA_COUT = 64, SA_KTOT = 224;

__device__ __forceinline__ f32x4 sa_max4(f32x4 a, f32x4 b) { return f32x4{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)}; }

// x[n][3][hw][hw] (NCHW fp32) -> zero-bordered NHWC4 [n][hw + 6][hw + 6][4]
__global__ __launch_bounds__(256) void nchw_to_padded_sized_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int hw) {
    const size_t plane = (size_t)hw * hw, total = (size_t)n * plane;
    const int w = hw + 6;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t img = i / plane;
        const int pix = (int)(i - img * plane);
        const int y = pix / hw, xx = pix - y * hw;
        const float* s = x + img * 3 * plane + pix;
        const f32x4 v = {s[0], s[plane], s[2 * plane], 0.f};
        reinterpret_cast<f32x4*>(out)[(img * w + (y + 3)) * w + (xx + 3)] = v;
    }
}

__global__ __launch_bounds__(256, 2) void stem_pool_any_kernel(const StemPoolAnyParams p) {
    __shared__ __attribute__((aligned(16))) float lds[SA_PATCH_CH * 4 + 2 * SA_TCOLS * SA_TS + 2 * (SA_MAX_RUN + 1) * SA_TS];
    float* const patch = lds;
    float* const tbuf = lds + SA_PATCH_CH * 4;
    float* const seam = tbuf + 2 * SA_TCOLS * SA_TS;  // [row pair of the run, warm-up pair first][stem row of the pair][channel]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave_id >> 1;  // stem row of the pair
    const int wn = wave_id & 1;   // 32-channel half
    const int lr = lane & 31;
    const int lh = lane >> 5;

    const int S = p.in_hw;
    const int iw = S + 6;        // padded input width
    const int po = S >> 2;       // pooled width / height
    const int ow = po + 2;       // padded output width
    const int nt = ((S >> 1) + 63) >> 6;  // column tiles of a stem row

    const int runs_per_crop = po / p.run;
    const int crop = blockIdx.x / runs_per_crop;
    if (crop >= p.crops) return;
    const int r0 = (blockIdx.x - crop * runs_per_crop) * p.run;
    const int r_end = r0 + p.run;
    const f32x4* const xin = reinterpret_cast<const f32x4*>(p.x) + (size_t)crop * iw * iw;

    // patch of (row pair R, column tile T) -> registers: chunk j = (input row 4 R + j / 134, input column 128 T + j % 134), zero past
    // the padded row
    f32x4 pre[SA_PASSES];
#define SA_LOAD(R, T)                                                                       \
    {                                                                                       \
        _Pragma("unroll") for (int i = 0; i < SA_PASSES; ++i) {                             \
            const int j = tid + 256 * i;                                                    \
            const int row = j / SA_PW, col = j - row * SA_PW, gc = 128 * (T) + col;          \
            f32x4 v = {0.f, 0.f, 0.f, 0.f};                                                 \
            if (j < SA_PATCH_CH && gc < iw) v = xin[(size_t)(4 * (R) + row) * iw + gc];     \
            pre[i] = v;                                                                     \
        }                                                                                   \
    }
#define SA_STORE()                                                                          \
    {                                                                                       \
        _Pragma("unroll") for (int i = 0; i < SA_PASSES; ++i) {                             \
            const int j = tid + 256 * i;                                                    \
            if (j < SA_PATCH_CH) *reinterpret_cast<f32x4*>(patch + (j ^ ((j >> 4) & 1)) * 4) = pre[i]; \
        }                                                                                   \
    }

    const int r_first = r0 > 0 ? r0 - 1 : 0;
    SA_LOAD(r_first, 0);

    // weights of this lane's output channel, resident for the whole kernel: step s multiplies taps (2 s, 2 s + 1) of the 49 (ky, kx),
    // this lane (half lh) holds tap 2 s + lh, channels 0-2; tap 49 (step 24, upper half) is a zero weight
    const int n = wn * 32 + lr;
    float bw[25][3];
    {
        const float* w = p.wgt + (size_t)n * SA_KTOT;
#pragma unroll
        for (int st = 0; st < 25; ++st) {
            const int t0 = 2 * st, t1 = 2 * st + 1;
            const int o0 = (t0 / 7) * 32 + (t0 % 7) * 4, o1 = t1 < 49 ? (t1 / 7) * 32 + (t1 % 7) * 4 : -1;
            f32x4 v = *reinterpret_cast<const f32x4*>(w + (lh && o1 >= 0 ? o1 : o0));
            if (lh && o1 < 0) v = f32x4{0.f, 0.f, 0.f, 0.f};
            bw[st][0] = v.x;
            bw[st][1] = v.y;
            bw[st][2] = v.z;
        }
    }
    const float bias = p.bias[n];
    const int c_lane = (2 * wm) * SA_PW + 2 * lr;  // chunk of (ky 0, kx 0) of this lane's first pixel

    // pooling: thread -> pooled pixels px = (tid >> 4) + 16 i (i = 0, 1) of the tile, channels c4 .. c4 + 3
    const int c4 = (tid & 15) * 4;
    for (int ct = 0; ct < nt; ++ct) {
        f32x4 hprev[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};  // horizontal 3-max of stem row 2 rr - 1
        for (int rr = r_first; rr < r_end; ++rr) {
            const bool warm = rr < r0;  // the row pair above the run: computed for the pooling's carry, not stored
            {
                SA_STORE();
                // column 0 of the stem tile: what the tile to the left left behind for these two stem rows
                if (tid < 128) {
                    const int row = tid >> 6, ch = tid & 63;
                    tbuf[(row * SA_TCOLS) * SA_TS + ch] = ct > 0 ? seam[((rr - r_first) * 2 + row) * SA_TS + ch] : 0.f;
                }
                __syncthreads();  // the patch is in LDS (and every wave is past the previous tile's pooling and seam copy)
                {
                    // the tile after this one, into registers while this one computes
                    const bool same_col = rr + 1 < r_end;
                    const int n_rr = same_col ? rr + 1 : r_first, n_ct = same_col ? ct : ct + 1;
                    if (n_ct < nt) SA_LOAD(n_rr, n_ct);
                }
                f32x16 acc[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[mi][e] = 0.f;
                f32x4 af[2][2];
                // chunk of this lane's tap of step ST: (ky, kx) = divmod(2 ST + lh, 7); the upper half's tap 49 reads tap 48's pixel
#define SA_FRAGS(SET, ST)                                                                          \
    {                                                                                              \
        const int t0_ = 2 * (ST), t1_ = 2 * (ST) + 1 < 49 ? 2 * (ST) + 1 : 48;                      \
        const int off_ = lh ? (t1_ / 7) * SA_PW + (t1_ % 7) : (t0_ / 7) * SA_PW + (t0_ % 7);      \
        _Pragma("unroll") for (int mi = 0; mi < 2; ++mi) {                                         \
            const int c = c_lane + off_ + 64 * mi;                                                 \
            af[SET][mi] = *reinterpret_cast<const f32x4*>(patch + (c ^ ((c >> 4) & 1)) * 4);       \
        }                                                                                          \
    }
                if (!(warm && wm == 0)) {  // (a warm-up tile is there for its SECOND stem row only)
                    SA_FRAGS(0, 0);
#pragma unroll
                    for (int g = 0; g < 25; ++g) {
#pragma unroll
                        for (int mi = 0; mi < 2; ++mi) {
                            const f32x4 a4 = af[g & 1][mi];
                            acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bw[g][0], acc[mi], 0, 0, 0);
                            if (mi == 0 && g + 1 < 25) SA_FRAGS((g + 1) & 1, g + 1);  // next step's operands, behind the first MFMA
                            acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bw[g][1], acc[mi], 0, 0, 0);
                            acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bw[g][2], acc[mi], 0, 0, 0);
                        }
                    }
                }
#undef SA_FRAGS
                // + folded BN bias, ReLU; the tile (2 rows x 64 pixels x 64 channels) goes through LDS so that the pooling threads
                // see pixel-major rows of 64 channels (columns 1 .. 64 of tbuf: column 0 is the seam)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int ox = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                        const float v = acc[mi][e] + bias;
                        tbuf[(wm * SA_TCOLS + 1 + ox) * SA_TS + n] = v > 0.f ? v : 0.f;
                    }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int px = (tid >> 4) + 16 * i;
                    f32x4 h[2];
#pragma unroll
                    for (int row = 0; row < 2; ++row) {
                        // stem columns 2 px - 1 (the seam column for px == 0), 2 px, 2 px + 1 of the tile
                        const float* t = tbuf + (row * SA_TCOLS + 1 + 2 * px) * SA_TS + c4;
                        h[row] = sa_max4(sa_max4(*reinterpret_cast<const f32x4*>(t - SA_TS), *reinterpret_cast<const f32x4*>(t)),
                                         *reinterpret_cast<const f32x4*>(t + SA_TS));
                    }
                    const f32x4 m = sa_max4(sa_max4(hprev[i], h[0]), h[1]);
                    hprev[i] = h[1];
                    const int gp = ct * 32 + px;  // pooled column in the crop
                    if (!warm && gp < po) {
                        const size_t o = (((size_t)crop * ow + rr + 1) * ow + gp + 1) * SA_COUT + c4;
                        *reinterpret_cast<f32x4*>(p.out + o) = m;
                    }
                }
                __syncthreads();  // every wave is done with tbuf and the patch
                // the seam for the tile to the right: this tile's last column
                if (tid < 128) {
                    const int row = tid >> 6, ch = tid & 63;
                    seam[((rr - r_first) * 2 + row) * SA_TS + ch] = tbuf[(row * SA_TCOLS + 64) * SA_TS + ch];
                }
            }
        }
    }
#undef SA_LOAD
#undef SA_STORE
}

}  // namespace

hipError_t launch_nchw_to_padded_sized(const float* x, float* out, int32_t n, int32_t hw, hipStream_t s) {
    if (n <= 0 || hw <= 0) return hipErrorInvalidValue;
    const size_t total = (size_t)n * hw * hw;
    size_t grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(nchw_to_padded_sized_kernel, dim3((unsigned)grid), dim3(256), 0, s, x, out, n, hw);
    return hipGetLastError();
}

hipError_t launch_stem_pool_any(const StemPoolAnyParams& p_in, hipStream_t s) {
    StemPoolAnyParams p = p_in;
    if (p.crops <= 0 || p.in_hw % 32 != 0 || p.in_hw < 64 || p.in_hw > 512 || !p.x || !p.wgt || !p.bias || !p.out) return hipErrorInvalidValue;
    // one run per workgroup; 512 workgroups (two per CU) want crops * runs per crop >= 512. S / 4 = 8 k row pairs per crop; a run is
    // 8 k / {1, 2, 4, 8} of them, halved until it fits the kernel's seam table (k <= 16 does)
    const int po = p.in_hw / 4;
    int per_crop = 1;
    while (per_crop < 8 && p.crops * per_crop < 512) per_crop *= 2;
    int run = po / per_crop;
    while (run > SA_MAX_RUN && run % 2 == 0) run /= 2;
    if (run < 1 || run > SA_MAX_RUN || po % run != 0) return hipErrorInvalidValue;
    p.run = run;
    hipLaunchKernelGGL(stem_pool_any_kernel, dim3(p.crops * (po / run)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace pa

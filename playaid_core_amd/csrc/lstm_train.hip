// Training of RNNActionDetector's LSTM head on the device (pa_lstm_train_step, include/playaid_hip.h; DESIGN.md "Training
// the LSTM head"): nn.LSTM(in, H, layers) on [T, N, in] (T windows are the time steps, N <= 16 frames the batch, zero
// initial state), Linear(H, 128) + ReLU, Linear(128, A), log_softmax, NLL as the mean over the rows whose label is not -100,
// back-propagation through time and torch.optim.Adam -- on the handle's weights where pa_lstm_forward reads them (PyTorch
// layouts, blob order: per layer w_ih, w_hh, b_ih, b_hh, then w1, b1, w2, b2).
//
// Launches of one step on the caller's stream (M = T N rows):
//   forward, per layer     launch_linear_f32 (the input projection of all steps), then T x lt_fwd_step_kernel, which keeps
//                          the four gates [M][4H], c [M][H] and h [M][H] of the layer
//   lt_decode_kernel       per row: z1, h1, z2, logp, loss term, hit, dz2, dz1, dh_top = dz1 W1
//   lt_param_kernel        dW2, db2, db1 (ascending rows) and the step's pa_train_stats
//   lt_dw_kernel           dW1 = dz1^T h_top (+ Adam), lt_small_adam_kernel on b1, w2, b2
//   backward, per layer from the top: T x lt_bwd_step_kernel (t = T - 1 .. 0), lt_dx_kernel (dX = dA W_ih, not for layer 0),
//                          lt_dw_kernel for dW_ih and dW_hh (+ Adam), lt_bias_kernel for b_ih and b_hh (+ Adam)
// No kernel waits for another workgroup of its launch: the recurrence is one launch per time step, in both directions. Every
// sum has a fixed order and there are no floating-point atomics: two runs give the same bits. The weights change in place, so
// every launch that reads a tensor (W1 in the decoder, W_hh[l] in the layer's backward steps, W_ih[l] in lt_dx_kernel) is
// enqueued before the launch that updates it.
//
// Labels outside [0, A) count as ignored (the Python wrapper refuses them; -100 is the only such value a checked caller passes).
#include "pa_kernels.h"
#include "train_common.h"
#include "lstm_handle.h"

namespace pa {
namespace {

constexpr int LT_NMAX = 16;   // batch rows of a time step (pa_lstm_forward's limit)

struct LstmTrainParams {
    const float* htop;        // [M][H] the top layer's h
    const float *w1, *b1, *w2, *b2;
    const int32_t* labels;    // [M], -100 = ignore
    int32_t M, H, A;
    float *h1, *dz1, *dz2, *dh, *loss_r;   // [M][128], [M][128], [M][64], [M][H], [M]
    int32_t* hit_r;                        // [M]
    float* gs;                // b1 [128] | w2 [A][128] | b2 [A]: the three small gradients, contiguous as in the blob
    float* stats;             // the trainer's pa_train_stats
    float* stats_out;         // the caller's, or nullptr
};

__device__ __forceinline__ float lt_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- forward: one time step of one layer, keeping what the backward pass needs ---------------------------------------
// grid H / 4, 256 threads: workgroup = 4 hidden units, wave g = gate g (i, f, g, o). pre [N][4H] (input projection + b_ih),
// h_prev / c_prev [N][H] or nullptr at t = 0; writes gates [N][4H] (post-activation), c_out, h_out [N][H] of this step.
// Everything a thread needs from memory is requested at once and without branches (addresses clamped, values selected
// afterwards): the k = lane + 64 q of its wave's four W_hh rows and its share of h(t-1), which goes to LDS as [k][n], pitch 20,
// rows n >= N zero, for 16-byte reads along n. A lane's 4 x 16 partial sums (unit, n; ascending q) are summed over the wave by
// a halving exchange -- step d = 32, 16, ... 1: the lane with bit d clear keeps the lower half of its values and adds the
// partner's, the other the upper half -- after which lane 16 u + n holds the total of (u, n): 63 exchanges, a fixed order.
constexpr int LT_FU = 4;

template <int D>
__device__ __forceinline__ void lt_halve(const float (&in)[2 * D], float (&out)[D], int lane) {
    const bool up = (lane & D) != 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float keep = up ? in[i + D] : in[i];
        const float send = up ? in[i] : in[i + D];
        out[i] = keep + __shfl_xor(send, D, 64);
    }
}

__global__ __launch_bounds__(256) void lt_fwd_step_kernel(const float* __restrict__ pre, const float* __restrict__ w_hh,
                                                          const float* __restrict__ b_hh, const float* __restrict__ h_prev,
                                                          const float* __restrict__ c_prev, float* __restrict__ gates,
                                                          float* __restrict__ c_out, float* __restrict__ h_out, int N, int H) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* hs = sm;                         // [H][20]: h(t-1)[n][k] at k * 20 + n
    float* gs = sm + (size_t)H * 20;        // [4 gates][LT_FU][LT_NMAX]
    const int j0 = blockIdx.x * LT_FU;
    const int tid = threadIdx.x, lane = tid & 63, gate = tid >> 6;
    if (h_prev) {
        float w[LT_FU][8];   // (H <= 512: eight k per lane and row)
#pragma unroll
        for (int u = 0; u < LT_FU; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = lane + 64 * q;
                const float x = w_hh[(size_t)(gate * H + j0 + u) * H + min(k, H - 1)];
                w[u][q] = k < H ? x : 0.f;
            }
        float hv[LT_NMAX][2];
#pragma unroll
        for (int n = 0; n < LT_NMAX; ++n)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int k = tid + 256 * b;
                const float x = h_prev[min(n, N - 1) * H + min(k, H - 1)];
                hv[n][b] = n < N ? x : 0.f;
            }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int k = tid + 256 * b;
            if (k < H) {
#pragma unroll
                for (int n4 = 0; n4 < 4; ++n4)
                    *reinterpret_cast<float4*>(hs + k * 20 + 4 * n4) = make_float4(hv[4 * n4][b], hv[4 * n4 + 1][b], hv[4 * n4 + 2][b], hv[4 * n4 + 3][b]);
            }
        }
        __syncthreads();
        float v[64];   // [u][n]
#pragma unroll
        for (int i = 0; i < 64; ++i) v[i] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4* hp = reinterpret_cast<const float4*>(hs + min(lane + 64 * q, H - 1) * 20);   // (k >= H: its weights are 0)
            const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2], h3 = hp[3];
            const float hn[16] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z, h2.w, h3.x, h3.y, h3.z, h3.w};
#pragma unroll
            for (int u = 0; u < LT_FU; ++u)
#pragma unroll
                for (int n = 0; n < LT_NMAX; ++n) v[u * 16 + n] = fmaf(w[u][q], hn[n], v[u * 16 + n]);
        }
        float a32[32], a16[16], a8[8], a4[4], a2[2], a1[1];
        lt_halve<32>(v, a32, lane);
        lt_halve<16>(a32, a16, lane);
        lt_halve<8>(a16, a8, lane);
        lt_halve<4>(a8, a4, lane);
        lt_halve<2>(a4, a2, lane);
        lt_halve<1>(a2, a1, lane);
        gs[gate * 64 + lane] = a1[0];   // lane = u * 16 + n
        __syncthreads();
    }
    if (tid < LT_FU * LT_NMAX) {
        const int u = tid / LT_NMAX, n = tid % LT_NMAX;
        if (n < N) {
            const int j = j0 + u;
            float g4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // torch: (x W_ih^T + b_ih) + (h W_hh^T + b_hh)
                const float rec = (h_prev ? gs[(g * LT_FU + u) * LT_NMAX + n] : 0.f) + b_hh[g * H + j];
                g4[g] = pre[(size_t)n * 4 * H + g * H + j] + rec;
            }
            const float ig = lt_sigmoid(g4[0]), fg = lt_sigmoid(g4[1]), gg = tanhf(g4[2]), og = lt_sigmoid(g4[3]);
            const float cp = c_prev ? c_prev[n * H + j] : 0.f;
            const float cn = fg * cp + ig * gg;
            float* gr = gates + (size_t)n * 4 * H + j;
            gr[0] = ig;
            gr[H] = fg;
            gr[2 * H] = gg;
            gr[3 * H] = og;
            c_out[n * H + j] = cn;
            h_out[n * H + j] = og * tanhf(cn);
        }
    }
}

// ---- decoder, loss and its way back to the top layer's h, per row -------------------------------------------------------
// grid M, 128 threads. Forward as lstm_decode_kernel (thread t = hidden unit t of the decoder, then lane = class).
__global__ __launch_bounds__(128) void lt_decode_kernel(LstmTrainParams p) {
    __shared__ float hr[512], h1s[128], dz1s[128], dz2s[64];
    __shared__ int nvalid;
    const int tid = threadIdx.x, row = blockIdx.x, H = p.H, A = p.A;
    if (tid == 0) nvalid = 0;
    __syncthreads();
    count_labelled(p.labels, p.M, A, tid, 128, &nvalid);
    for (int k = tid; k < H; k += 128) hr[k] = p.htop[(size_t)row * H + k];
    __syncthreads();
    const float n = (float)max(nvalid, 1);   // no labelled row: divide by 1, every gradient is then 0
    const int label = p.labels[row];
    const bool valid = label >= 0 && label < A;
    float z1;
    {
        const float4* w = reinterpret_cast<const float4*>(p.w1 + (size_t)tid * H);   // (H is a multiple of 4, every tensor 16-byte aligned)
        float a = 0.f;
#pragma unroll 8
        for (int k4 = 0; k4 < (H >> 2); ++k4) {   // one chain in ascending k, as lstm_decode_kernel's
            const float4 wv = w[k4];
            a = fmaf(wv.x, hr[4 * k4], a);
            a = fmaf(wv.y, hr[4 * k4 + 1], a);
            a = fmaf(wv.z, hr[4 * k4 + 2], a);
            a = fmaf(wv.w, hr[4 * k4 + 3], a);
        }
        z1 = a + p.b1[tid];
        h1s[tid] = z1 > 0.f ? z1 : 0.f;
        p.h1[(size_t)row * 128 + tid] = h1s[tid];
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: lane = class
        float z2 = -INFINITY;
        if (tid < A) {
            const float* w = p.w2 + (size_t)tid * 128;
            float a = 0.f;
            for (int k = 0; k < 128; ++k) a = fmaf(w[k], h1s[k], a);
            z2 = a + p.b2[tid];
        }
        const RowLoss r = softmax_nll_wave0(z2, tid, A, label, valid, n);
        dz2s[tid] = r.d;
        p.dz2[(size_t)row * 64 + tid] = r.d;
        if (tid == 0) {
            p.loss_r[row] = r.loss;
            p.hit_r[row] = r.hit;
        }
    }
    __syncthreads();
    {
        float s = 0.f;
        for (int a = 0; a < A; ++a) s = fmaf(dz2s[a], p.w2[a * 128 + tid], s);
        s = z1 > 0.f ? s : 0.f;   // ReLU's derivative at 0 is 0
        dz1s[tid] = s;
        p.dz1[(size_t)row * 128 + tid] = s;
    }
    __syncthreads();
    for (int k = tid; k < H; k += 128) {
        float s = 0.f;
        for (int t = 0; t < 128; ++t) s = fmaf(dz1s[t], p.w1[(size_t)t * H + k], s);
        p.dh[(size_t)row * H + k] = s;
    }
}

// ---- the decoder's small gradients, one thread per output element, ascending rows -------------------------------------
// gs: db1 [128] | dW2 [A][128] | db2 [A]; the thread behind them folds the step's statistics.
__global__ __launch_bounds__(256) void lt_param_kernel(LstmTrainParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x, M = p.M, A = p.A;
    const int n_w2 = 128 + A * 128, n_end = n_w2 + A;
    float s = 0.f;
    if (i < 128) {
        for (int r = 0; r < M; ++r) s += p.dz1[(size_t)r * 128 + i];
    } else if (i < n_w2) {
        const int a = (i - 128) >> 7, k = (i - 128) & 127;
        for (int r = 0; r < M; ++r) s = fmaf(p.dz2[(size_t)r * 64 + a], p.h1[(size_t)r * 128 + k], s);
    } else if (i < n_end) {
        for (int r = 0; r < M; ++r) s += p.dz2[(size_t)r * 64 + (i - n_w2)];
    } else if (i == n_end) {
        write_train_stats(p.stats, p.stats_out, p.labels, p.hit_r, p.loss_r, M, A);
        return;
    } else {
        return;
    }
    p.gs[i] = s;
}

// Adam on n contiguous floats (the decoder's b1 | w2 | b2, which lie in that order in the blob, the moments and gs).
__global__ __launch_bounds__(256) void lt_small_adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ g, int n, AdamScalars ak) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // Not adam_apply_at: with the gradient read before w, m and v the compiler fuses the other product of v's sum into the
    // double-precision FMA here (fma((1 - b2) g, g, b2 v) for fma(b2, v, (1 - b2) g g)), which rounds differently.
    float wi = w[i], mi = m[i], vi = v[i];
    adam_apply(wi, mi, vi, g[i], ak);
    w[i] = wi;
    m[i] = mi;
    v[i] = vi;
}

// ---- backward: one time step of one layer --------------------------------------------------------------------------------
// grid H / 16, 256 threads: a workgroup owns the hidden units j0 .. j0 + 15 and nothing is shared between workgroups. With
// da_next (dA of step t + 1, [N][4H]; nullptr at t = T - 1) thread (jj = tid & 15, kp = tid >> 4) forms its part of
// rec[n][j] = sum_k da_next[n][k] W_hh[k][j] -- W_hh is [4H][H] row-major, so the reads run along j -- over the k = KC c + 16 q +
// kp (chunks of KC = 512 k where 4H is a multiple of it, else 128: a chunk's KC / 16 weights per thread and its share of the
// da_next slice that goes to LDS are requested together, without branches), the sixteen parts are summed in ascending kp by thread (n = tid >> 4, jj), which then does
// the gate derivatives of
// (n, j): dh = dh_in + rec, and with the saved gates i, f, g, o, c_t and c_(t-1)
//   do = dh tanh(c_t), dc = dh o (1 - tanh^2(c_t)) + carry, di = dc g, dg = dc i, df = dc c_(t-1), carry' = dc f
//   dA[t] = [di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o)]
// carry [LT_NMAX][H] is dc_(t+1) f_(t+1), read (not at t = T - 1) and rewritten by its owner alone.
template <int KC>
__global__ __launch_bounds__(256) void lt_bwd_step_kernel(const float* __restrict__ da_next, const float* __restrict__ w_hh,
                                                          const float* __restrict__ dh_in, const float* __restrict__ gates,
                                                          const float* __restrict__ c_t, const float* __restrict__ c_prev,
                                                          float* __restrict__ carry, float* __restrict__ da_t, int N, int H) {
    __shared__ __attribute__((aligned(16))) float das[KC * 20];   // [k of the chunk][n], pitch 20: float4 reads along n
    __shared__ float red[16 * 272];                                // [kp][n][jj], pitch 272 per kp
    const int tid = threadIdx.x, jj = tid & 15, kp = tid >> 4, j0 = blockIdx.x * 16;
    float rec = 0.f;
    if (da_next) {
        float acc[LT_NMAX];
#pragma unroll
        for (int n = 0; n < LT_NMAX; ++n) acc[n] = 0.f;
        const float* wcol = w_hh + j0 + jj;
        for (int k0 = 0; k0 < 4 * H; k0 += KC) {
            float wq[KC / 16];
#pragma unroll
            for (int q = 0; q < KC / 16; ++q) wq[q] = wcol[(size_t)(k0 + q * 16 + kp) * H];
            float dv[KC / 16];   // (requested at once: rows n >= N read row N - 1 and become zeros)
#pragma unroll
            for (int i = 0; i < KC / 16; ++i) {
                const int idx = tid + 256 * i, n = idx / KC, kk = idx % KC;
                const float x = da_next[(size_t)min(n, N - 1) * 4 * H + k0 + kk];
                dv[i] = n < N ? x : 0.f;
            }
#pragma unroll
            for (int i = 0; i < KC / 16; ++i) {
                const int idx = tid + 256 * i;
                das[(idx % KC) * 20 + idx / KC] = dv[i];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < KC / 16; ++q) {
                const int kk = q * 16 + kp;
                const float w = wq[q];
                const float4* dp = reinterpret_cast<const float4*>(das + kk * 20);
                const float4 d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
                acc[0] = fmaf(d0.x, w, acc[0]);
                acc[1] = fmaf(d0.y, w, acc[1]);
                acc[2] = fmaf(d0.z, w, acc[2]);
                acc[3] = fmaf(d0.w, w, acc[3]);
                acc[4] = fmaf(d1.x, w, acc[4]);
                acc[5] = fmaf(d1.y, w, acc[5]);
                acc[6] = fmaf(d1.z, w, acc[6]);
                acc[7] = fmaf(d1.w, w, acc[7]);
                acc[8] = fmaf(d2.x, w, acc[8]);
                acc[9] = fmaf(d2.y, w, acc[9]);
                acc[10] = fmaf(d2.z, w, acc[10]);
                acc[11] = fmaf(d2.w, w, acc[11]);
                acc[12] = fmaf(d3.x, w, acc[12]);
                acc[13] = fmaf(d3.y, w, acc[13]);
                acc[14] = fmaf(d3.z, w, acc[14]);
                acc[15] = fmaf(d3.w, w, acc[15]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int n = 0; n < LT_NMAX; ++n) red[kp * 272 + n * 16 + jj] = acc[n];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) rec += red[q * 272 + tid];   // thread (n = tid >> 4, jj): ascending kp
    }
    const int n = tid >> 4, j = j0 + jj;
    if (n >= N) return;
    const float* gr = gates + (size_t)n * 4 * H + j;
    const float ig = gr[0], fg = gr[H], gg = gr[2 * H], og = gr[3 * H];
    const float tc = tanhf(c_t[n * H + j]);
    const float cp = c_prev ? c_prev[n * H + j] : 0.f;
    const float dh = dh_in[n * H + j] + rec;
    const float d_o = dh * tc;
    float dc = dh * og * (1.f - tc * tc);
    if (da_next) dc += carry[n * H + j];
    const float di = dc * gg, dg = dc * ig, df = dc * cp;
    carry[n * H + j] = dc * fg;
    float* out = da_t + (size_t)n * 4 * H + j;
    out[0] = di * ig * (1.f - ig);
    out[H] = df * fg * (1.f - fg);
    out[2 * H] = dg * (1.f - gg * gg);
    out[3 * H] = d_o * og * (1.f - og);
}

// ---- dX = dA W_ih for the layer below: [M][K = 4H] x [K][C = H] ------------------------------------------------------------
// grid (C / 32, ceil(M / 32)), 256 threads: one 32 (c) x 32 (rows) tile of v_mfma_f32_32x32x2_f32 per workgroup, W_ih rows as
// the A operand (reads along c), dA as the B operand, so that a lane ends with four consecutive c of one row. Wave w takes the
// k in [w K / 4, (w + 1) K / 4) (K / 4 = H, a multiple of 32), ascending, 32 per round with all of a round's operands
// requested before its sixteen instructions; the four partial tiles are summed through LDS in wave order.
__global__ __launch_bounds__(256) void lt_dx_kernel(const float* __restrict__ dA, const float* __restrict__ w_ih, float* __restrict__ dX,
                                                    int M, int C, int K) {
    __shared__ __attribute__((aligned(16))) float part[4][32][36];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
    const float* wp = w_ih + c0 + r;
    const float* dp = dA + (size_t)min(m0 + r, M - 1) * K;   // (rows past M read the last row; their results are not stored)
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int kq = K >> 2;
    for (int k0 = wave * kq; k0 < (wave + 1) * kq; k0 += 32) {
        float a[16], b[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = k0 + 2 * u + h;
            a[u] = wp[(size_t)k * C];
            b[u] = dp[k];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)   // D[c = 8g + 4h + 0..3][row = r]
        *reinterpret_cast<float4*>(&part[wave][r][8 * g + 4 * h]) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
    __syncthreads();
    const int row = tid >> 3, c4 = (tid & 7) * 4;
    float4 s = *reinterpret_cast<const float4*>(&part[0][row][c4]);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float4 p = *reinterpret_cast<const float4*>(&part[w][row][c4]);
        s.x += p.x;
        s.y += p.y;
        s.z += p.z;
        s.w += p.w;
    }
    if (m0 + row < M) *reinterpret_cast<float4*>(dX + (size_t)(m0 + row) * C + c0 + c4) = s;
}

// ---- a weight gradient (+ Adam) ---------------------------------------------------------------------------------------------
// dW[o][c] = sum_r D[r][o] X[r][c] for o < O (a multiple of 64), c < C, r < K, on v_mfma_f32_32x32x2_f32 with the X rows as
// the A operand (M = c) and the D rows as the B operand (N = o): a lane's accumulator registers 4g .. 4g + 3 are the four
// consecutive c = 8g + 4h + 0..3 of one o, so the epilogue reads and writes w, m and v with 16-byte accesses along c where C
// is a multiple of 4 (element-wise otherwise: the same arithmetic per element). grid (ceil(C / 64), O / 64), 256 threads: wave
// (wc, wo) one 32 x 32 tile of the workgroup's 64 x 64. One workgroup owns its tile for all of K, ascending, two rows per
// instruction (lane half h takes row r0 + h); an odd K ends with a zero row. Columns c >= C are loaded as zero and never
// stored: edge tiles are exact. STORE_G: the gradient to gout [O][C] instead, the state untouched.
template <bool STORE_G>
__global__ __launch_bounds__(256) void lt_dw_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ D, int ldd, int K, int C,
                                                    float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ gout, AdamScalars ak) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, wc = wave & 1, wo = wave >> 1;
    const int cl = blockIdx.x * 64 + wc * 32 + r;     // this lane's column of X (A operand)
    const int o = blockIdx.y * 64 + wo * 32 + r;      // this lane's column of D (B operand) and its output row
    const bool c_ok = cl < C;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* xa = X + (c_ok ? cl : 0);
    const float* da = D + o;
    for (int r0 = 0; r0 < K; r0 += 16) {   // eight k-steps per round, all of a round's operands requested before its instructions
        float a[8], d[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = r0 + 2 * u + h;
            a[u] = d[u] = 0.f;
            if (row < K) {
                if (c_ok) a[u] = xa[(size_t)row * ldx];
                d[u] = da[(size_t)row * ldd];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], d[u], acc, 0, 0, 0);
    }
    const bool vec = (C & 3) == 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = blockIdx.x * 64 + wc * 32 + 8 * g + 4 * h;
        if (c >= C) continue;
        const float gr[4] = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        const size_t idx = (size_t)o * C + c;
        if (STORE_G) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < C) gout[idx + j] = gr[j];
        } else if (vec) {   // (c is a multiple of 4 and so is C: c + 3 < C, idx is 16-byte aligned)
            adam_apply4_at(w, m, v, idx, gr, ak);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < C) adam_apply_at(w, m, v, idx + j, gr[j], ak);
        }
    }
}

// ---- the biases: db_ih = db_hh = the column sums of dA (ascending rows), one thread per column (+ Adam on both) ---------------
// w, m, v, gout point at b_ih [4H], which b_hh [4H] follows directly (blob order).
template <bool STORE_G>
__global__ __launch_bounds__(256) void lt_bias_kernel(const float* __restrict__ dA, int M, int H4, float* __restrict__ w, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ gout, AdamScalars ak) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= H4) return;
    float s = 0.f;
    for (int r = 0; r < M; ++r) s += dA[(size_t)r * H4 + k];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int i = b * H4 + k;
        if (STORE_G)
            gout[i] = s;
        else
            adam_apply_at(w, m, v, i, s, ak);
    }
}

hipError_t launch_dw(bool apply, const float* X, int ldx, const float* D, int ldd, int K, int O, int C, float* w, float* m, float* v, float* gout,
                     const AdamScalars& ak, hipStream_t s) {
    const dim3 grid((C + 63) / 64, O / 64);
    if (apply)
        hipLaunchKernelGGL(lt_dw_kernel<false>, grid, dim3(256), 0, s, X, ldx, D, ldd, K, C, w, m, v, (float*)nullptr, ak);
    else
        hipLaunchKernelGGL(lt_dw_kernel<true>, grid, dim3(256), 0, s, X, ldx, D, ldd, K, C, (float*)nullptr, (float*)nullptr, (float*)nullptr, gout,
                           ak);
    return hipGetLastError();
}

}  // namespace
}  // namespace pa

// =====================================================================================
// The trainer: a handle beside its pa_lstm
// =====================================================================================

struct pa_lstm_trainer : pa::TrainerCore {   // state: m | v (blob order, PyTorch layouts) | the saved activations and scratch
    pa_lstm* h = nullptr;
    size_t nw = 0;             // floats of one tensor set (the blob's)
    float *m = nullptr, *v = nullptr;
    float *pre = nullptr, *dA = nullptr, *dh = nullptr, *carry = nullptr;
    float *gates = nullptr, *cs = nullptr, *hs = nullptr;   // per layer: [max_rows][4H], [max_rows][H], [max_rows][H]
    float *h1 = nullptr, *dz1 = nullptr, *dz2 = nullptr, *loss_r = nullptr, *gs = nullptr, *stats = nullptr;
    int32_t* hit_r = nullptr;
};

using pa::trainer_fail;

extern "C" {

size_t pa_lstm_trainer_floats(const pa_lstm* h) { return h ? pa::lstm_float_count(h->in_dim, h->hid, h->layers, h->actions) : 0; }

int pa_lstm_trainer_create(pa_lstm* h, const pa_adam_config* cfg, pa_lstm_trainer** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (!h || !cfg) return PA_ERR_INVALID_ARG;
    if (!pa::adam_config_ok(cfg->lr, cfg->beta1, cfg->beta2, cfg->eps)) return PA_ERR_INVALID_ARG;
    if (h->hid % 32 != 0) {
        h->last_error = "pa_lstm_trainer_create: training needs a hidden size that is a multiple of 32 (this handle serves inference only)";
        return PA_ERR_INVALID_ARG;
    }
    pa_lstm_trainer* t = new pa_lstm_trainer();
    *out = t;   // (handed back whatever follows: TrainerCore)
    t->h = h;
    t->cfg = *cfg;
    t->nw = pa::lstm_float_count(h->in_dim, h->hid, h->layers, h->actions);
    if (!h->weights) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_lstm_trainer_create: the handle has no weights on a device");
    if (hipSetDevice(h->device) != hipSuccess) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_lstm_trainer_create: hipSetDevice failed");
    const size_t R = (size_t)h->max_rows, H = (size_t)h->hid, L = (size_t)h->layers, A = (size_t)h->actions;
    const size_t nw = (t->nw + 63) & ~(size_t)63;
    const size_t n_small = (128 + 129 * A + 63) & ~(size_t)63;
    const size_t scratch = R * 4 * H * 2 + R * H + pa::LT_NMAX * H + L * R * 6 * H + R * (128 + 128 + 64 + 2) + n_small + 64;
    if (const int rc = pa::trainer_alloc_zeroed(t, 2 * nw + scratch, "pa_lstm_trainer_create")) return rc;
    float* q = t->state;
    t->m = q, q += nw;
    t->v = q, q += nw;
    t->pre = q, q += R * 4 * H;
    t->dA = q, q += R * 4 * H;
    t->dh = q, q += R * H;
    t->carry = q, q += pa::LT_NMAX * H;
    t->gates = q, q += L * R * 4 * H;
    t->cs = q, q += L * R * H;
    t->hs = q, q += L * R * H;
    t->h1 = q, q += R * 128;
    t->dz1 = q, q += R * 128;
    t->dz2 = q, q += R * 64;
    t->loss_r = q, q += R;
    t->hit_r = reinterpret_cast<int32_t*>(q), q += R;
    t->gs = q, q += n_small;
    t->stats = q;
    return PA_OK;
}

void pa_lstm_trainer_destroy(pa_lstm_trainer* t) { pa::trainer_destroy(t); }

const char* pa_lstm_trainer_last_error(const pa_lstm_trainer* t) { return pa::trainer_last_error(t); }

int64_t pa_lstm_trainer_steps(const pa_lstm_trainer* t) { return pa::trainer_steps(t); }

int pa_lstm_train_step(pa_lstm_trainer* t, const float* x, int32_t ld, int32_t seq_len, int32_t batch, const int32_t* labels, int32_t apply,
                       float* grads_out, pa_train_stats* stats_dev, void* stream) {
    using namespace pa;
    if (!t) return PA_ERR_INVALID_ARG;
    pa_lstm* h = t->h;
    if (!x || !labels) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_lstm_train_step: null input");
    if (seq_len < 1 || batch < 1 || batch > LT_NMAX) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_lstm_train_step: seq_len < 1 or batch outside 1..16");
    if ((long long)seq_len * batch > h->max_rows) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_lstm_train_step: seq_len * batch exceeds max_rows");
    if (ld < h->in_dim) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_lstm_train_step: ld < input_dim");
    if (const int rc = trainer_check_apply(t, apply, grads_out, "pa_lstm_train_step")) return rc;
    if (!t->state) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_lstm_train_step: the trainer has no device state");
    hipStream_t s = (hipStream_t)stream;
    const int H = h->hid, L = h->layers, A = h->actions, T = seq_len, N = batch, M = T * N;
    const size_t R = (size_t)h->max_rows;
    const AdamScalars ak = adam_scalars(t->cfg.lr, t->cfg.beta1, t->cfg.beta2, t->cfg.eps, t->steps + 1, apply != 0);
    hipError_t err = hipSuccess;
    auto fail = [&](hipError_t e) { return trainer_fail(t, PA_ERR_HIP, std::string("pa_lstm_train_step: ") + hipGetErrorString(e)); };
    // a tensor of the handle -> the same tensor of m, v or grads_out (all in blob order)
    auto off = [&](const float* wp) { return (size_t)(wp - h->weights); };

    // forward
    const size_t step_lds = ((size_t)H * 20 + 4 * LT_FU * LT_NMAX) * sizeof(float);
    for (int l = 0; l < L; ++l) {
        const float* in = l == 0 ? x : t->hs + (size_t)(l - 1) * R * H;
        const int in_ld = l == 0 ? ld : H, K = l == 0 ? h->in_dim : H;
        if ((err = launch_linear_f32(in, in_ld, h->w_ih[l], h->b_ih[l], t->pre, 4 * H, M, 4 * H, K, 0, s)) != hipSuccess) return fail(err);
        float* gl = t->gates + (size_t)l * R * 4 * H;
        float* cl = t->cs + (size_t)l * R * H;
        float* hl = t->hs + (size_t)l * R * H;
        for (int k = 0; k < T; ++k) {
            const size_t r0 = (size_t)k * N, rp = (size_t)(k - 1) * N;
            hipLaunchKernelGGL(lt_fwd_step_kernel, dim3(H / LT_FU), dim3(256), step_lds, s, (const float*)t->pre + r0 * 4 * H, (const float*)h->w_hh[l],
                               (const float*)h->b_hh[l], k ? (const float*)hl + rp * H : nullptr, k ? (const float*)cl + rp * H : nullptr,
                               gl + r0 * 4 * H, cl + r0 * H, hl + r0 * H, N, H);
        }
        if ((err = hipGetLastError()) != hipSuccess) return fail(err);
    }
    // decoder, loss, the small gradients
    float* htop = t->hs + (size_t)(L - 1) * R * H;
    LstmTrainParams p;
    memset(&p, 0, sizeof(p));
    p.htop = htop;
    p.w1 = h->w1, p.b1 = h->b1, p.w2 = h->w2, p.b2 = h->b2;
    p.labels = labels;
    p.M = M, p.H = H, p.A = A;
    p.h1 = t->h1, p.dz1 = t->dz1, p.dz2 = t->dz2, p.dh = t->dh, p.loss_r = t->loss_r, p.hit_r = t->hit_r;
    p.gs = apply ? t->gs : grads_out + off(h->b1);
    p.stats = t->stats;
    p.stats_out = reinterpret_cast<float*>(stats_dev);
    const int n_small = 128 + 129 * A;
    hipLaunchKernelGGL(lt_decode_kernel, dim3(M), dim3(128), 0, s, p);
    if ((err = hipGetLastError()) != hipSuccess) return fail(err);
    hipLaunchKernelGGL(lt_param_kernel, dim3((n_small + 1 + 255) / 256), dim3(256), 0, s, p);
    if ((err = hipGetLastError()) != hipSuccess) return fail(err);
    // (lt_decode_kernel has read w1, b1, w2, b2: they may change now)
    if ((err = launch_dw(apply != 0, htop, H, t->dz1, 128, M, 128, H, h->w1, t->m + off(h->w1), t->v + off(h->w1),
                         apply ? nullptr : grads_out + off(h->w1), ak, s)) != hipSuccess)
        return fail(err);
    if (apply) {
        hipLaunchKernelGGL(lt_small_adam_kernel, dim3((n_small + 255) / 256), dim3(256), 0, s, h->b1, t->m + off(h->b1), t->v + off(h->b1),
                           (const float*)t->gs, n_small, ak);
        if ((err = hipGetLastError()) != hipSuccess) return fail(err);
    }
    // backward through time, from the top layer
    const auto bwd_step = (4 * H) % 512 == 0 ? lt_bwd_step_kernel<512> : lt_bwd_step_kernel<128>;
    for (int l = L - 1; l >= 0; --l) {
        const float* gl = t->gates + (size_t)l * R * 4 * H;
        const float* cl = t->cs + (size_t)l * R * H;
        const float* hl = t->hs + (size_t)l * R * H;
        for (int k = T - 1; k >= 0; --k) {
            const size_t r0 = (size_t)k * N;
            hipLaunchKernelGGL(bwd_step, dim3(H / 16), dim3(256), 0, s, k < T - 1 ? (const float*)t->dA + (r0 + N) * 4 * H : nullptr,
                               (const float*)h->w_hh[l], (const float*)t->dh + r0 * H, gl + r0 * 4 * H, cl + r0 * H,
                               k ? cl + (r0 - N) * H : nullptr, t->carry, t->dA + r0 * 4 * H, N, H);
        }
        if ((err = hipGetLastError()) != hipSuccess) return fail(err);
        if (l > 0) {   // dh of the layer below (reads W_ih[l] before its update; overwrites this layer's dh, which is done with)
            hipLaunchKernelGGL(lt_dx_kernel, dim3(H / 32, (M + 31) / 32), dim3(256), 0, s, (const float*)t->dA, (const float*)h->w_ih[l],
                               t->dh, M, H, 4 * H);
            if ((err = hipGetLastError()) != hipSuccess) return fail(err);
        }
        const float* xin = l == 0 ? x : t->hs + (size_t)(l - 1) * R * H;
        const int xld = l == 0 ? ld : H, C = l == 0 ? h->in_dim : H;
        const size_t o_ih = off(h->w_ih[l]), o_hh = off(h->w_hh[l]), o_b = off(h->b_ih[l]);
        if ((err = launch_dw(apply != 0, xin, xld, t->dA, 4 * H, M, 4 * H, C, h->w_ih[l], t->m + o_ih, t->v + o_ih,
                             apply ? nullptr : grads_out + o_ih, ak, s)) != hipSuccess)
            return fail(err);
        // dW_hh = dA[1..T)^T h[0..T-1): the dA rows shifted by one step; T = 1 leaves K = 0 rows and a zero gradient
        if ((err = launch_dw(apply != 0, hl, H, t->dA + (size_t)N * 4 * H, 4 * H, (T - 1) * N, 4 * H, H, h->w_hh[l], t->m + o_hh, t->v + o_hh,
                             apply ? nullptr : grads_out + o_hh, ak, s)) != hipSuccess)
            return fail(err);
        if (apply)
            hipLaunchKernelGGL(lt_bias_kernel<false>, dim3((4 * H + 255) / 256), dim3(256), 0, s, (const float*)t->dA, M, 4 * H, h->b_ih[l],
                               t->m + o_b, t->v + o_b, (float*)nullptr, ak);
        else
            hipLaunchKernelGGL(lt_bias_kernel<true>, dim3((4 * H + 255) / 256), dim3(256), 0, s, (const float*)t->dA, M, 4 * H, (float*)nullptr,
                               (float*)nullptr, (float*)nullptr, grads_out + o_b, ak);
        if ((err = hipGetLastError()) != hipSuccess) return fail(err);
    }
    if (apply) t->steps += 1;
    return PA_OK;
}

int pa_lstm_trainer_read(pa_lstm_trainer* t, int32_t which, float* out_dev, size_t floats, void* stream) {
    if (!t) return PA_ERR_INVALID_ARG;
    // (PA_TRAIN_RAW is refused too: the tensors lie in PyTorch layouts, there is no other form)
    if (const int rc = pa::trainer_check_which(t, which, out_dev, "pa_lstm_trainer_read")) return rc;
    if (floats != t->nw) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_lstm_trainer_read: wrong output size");
    if (!t->state) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_lstm_trainer_read: the trainer has no device state");
    const float* src = which == PA_TRAIN_WEIGHTS ? t->h->weights : which == PA_TRAIN_M ? t->m : t->v;
    if (hipMemcpyAsync(out_dev, src, t->nw * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return trainer_fail(t, PA_ERR_HIP, "pa_lstm_trainer_read: hipMemcpyAsync failed");
    return PA_OK;
}

}  // extern "C"

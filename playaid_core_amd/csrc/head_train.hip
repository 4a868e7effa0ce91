// Training of CNNActionDetector's temporal head on the device (pa_head_train_step, include/playaid_hip.h; DESIGN.md
// "Training the head"): Conv1d(1000 -> 512, k = S) + ReLU, Linear(512 -> 128) + ReLU, Linear(128 -> A), log_softmax,
// NLL over the windows whose label is not -100, the backward pass of all of it and torch.optim.Adam -- on the weights
// where the inference kernels read them (w1d [512][S][1024], w2 [512][128] and w3 [128][64] k-major, the biases).
//
// One step is five launches on the caller's stream:
//   1. ht_conv1d_kernel   h1 = relu(b1 + W1 * gathered rows)            v_mfma_f32_32x32x2_f32, K split over the four waves
//   2. ht_sample_kernel   per window: z2, h2, z3, logp, loss term, hit, dz3, dz2, dz1
//   3. ht_param_kernel    per output element: dW2, dW3, db1, db2, db3 (ascending b) and the step's pa_train_stats
//   4. ht_dw1_kernel      dW1 = dz1^T * gathered rows, one workgroup per 128 x 128 tile for all of K = B, Adam in the epilogue
//                         (or, <true>, the gradient stored in PyTorch layout and no state touched)
//   5. ht_adam_kernel     Adam on the five small tensors (or ht_export_kernel: their gradients in PyTorch layout)
// Every sum has a fixed order: no floating-point atomics, no split K across workgroups, nothing handed from one
// workgroup to another inside a launch. Two runs give the same bits.
//
// Gather indices are device data: every kernel clamps them into [0, n_rows). Labels outside [0, A) count as ignored
// (the host wrapper refuses them; -100 is the only such value a checked caller passes).
#include "pa_kernels.h"
#include "train_common.h"   // the loss, the statistics, adam_apply*

namespace pa {

namespace {

constexpr int FS = 1024;   // feature row stride (PA_FEATURE_STRIDE)
constexpr int FC = 1000;   // features used

__device__ __forceinline__ int clamp_row(int g, int n_rows) { return min(max(g, 0), n_rows - 1); }

// ---- 1. Conv1d over the gathered rows ------------------------------------------------------------------------------
// grid (ceil(B / 32), 16), 256 threads: a 32 (b) x 32 (o) tile of h1 per workgroup. Wave w takes the 8-float chunks
// w, w + 4, ... of every slot's 1000 features (lane half h the floats 4h .. 4h + 3 of a chunk, on both operands), the four
// partial tiles are summed through LDS in wave order, then bias and ReLU.
__global__ __launch_bounds__(256) void ht_conv1d_kernel(const float* __restrict__ feats, int n_rows, const int32_t* __restrict__ gather,
                                                        int B, int S, const float* __restrict__ w1d, const float* __restrict__ b1,
                                                        float* __restrict__ h1) {
    __shared__ float red[4][32][33];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = min((int)blockIdx.x * 32 + r, B - 1);
    const int o = blockIdx.y * 32 + r;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < S; ++t) {
        const int g = clamp_row(gather[b * S + t], n_rows);
        const float* fa = feats + (size_t)g * FS + 4 * h;
        const float* wb = w1d + ((size_t)o * S + t) * FS + 4 * h;
        for (int c = wave * 8; c < FC; c += 32) {
            const float4 a = *reinterpret_cast<const float4*>(fa + c);
            const float4 w = *reinterpret_cast<const float4*>(wb + c);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave][(i & 3) + 8 * (i >> 2) + 4 * h][r] = acc[i];   // D[row = b][col = o]
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const int row = e >> 5, col = e & 31;
        const int bb = blockIdx.x * 32 + row, oo = blockIdx.y * 32 + col;
        float s = red[0][row][col] + red[1][row][col];
        s += red[2][row][col];
        s += red[3][row][col];
        s += b1[oo];
        if (bb < B) h1[(size_t)bb * 512 + oo] = fmaxf(s, 0.f);
    }
}

// ---- 2. the middle, per window ------------------------------------------------------------------------------------
// grid B, 256 threads. Writes h2 [B][128], dz3 [B][64] (zero past A), dz2 [B][128], dz1 [B][512], loss_b [B], hit_b [B].
__global__ __launch_bounds__(256) void ht_sample_kernel(HeadTrainParams p) {
    __shared__ float h1s[512], h2s[128], dz2s[128], dz3s[64];
    __shared__ int nvalid;
    const int tid = threadIdx.x, b = blockIdx.x, A = p.A;
    const float *w2 = p.w[2], *b2 = p.w[3], *w3 = p.w[4], *b3 = p.w[5];
    if (tid == 0) nvalid = 0;
    __syncthreads();
    // Not count_labelled: its per-thread sums make 64 LDS atomics of a wave where the compiler folds this form's constant 1
    // into one, and the step at B = 64 measured 1.9 us (1 %) slower with it. (B <= 256 == blockDim: pa_head_trainer_create.)
    if (tid < p.B) {
        const int l = p.labels[tid];
        if (l >= 0 && l < A) atomicAdd(&nvalid, 1);   // (an integer count in LDS: exact in any order)
    }
    h1s[tid] = p.h1[(size_t)b * 512 + tid];
    h1s[tid + 256] = p.h1[(size_t)b * 512 + tid + 256];
    __syncthreads();
    const float n = (float)max(nvalid, 1);   // no valid label: divide by 1, every gradient is then 0
    const int label = p.labels[b];
    const bool valid = label >= 0 && label < A;
    float z2 = 0.f;
    if (tid < 128) {
        z2 = b2[tid];
        for (int k = 0; k < 512; ++k) z2 = fmaf(w2[k * 128 + tid], h1s[k], z2);
        h2s[tid] = fmaxf(z2, 0.f);
        p.h2[b * 128 + tid] = h2s[tid];
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: lane = class
        float z3 = -INFINITY;
        if (tid < A) {
            z3 = b3[tid];
            for (int k = 0; k < 128; ++k) z3 = fmaf(w3[k * 64 + tid], h2s[k], z3);
        }
        const RowLoss r = softmax_nll_wave0(z3, tid, A, label, valid, n);
        dz3s[tid] = r.d;
        p.dz3[b * 64 + tid] = r.d;
        if (tid == 0) {
            p.loss_b[b] = r.loss;
            p.hit_b[b] = r.hit;
        }
    }
    __syncthreads();
    if (tid < 128) {
        float s = 0.f;
        for (int a = 0; a < 64; ++a) s = fmaf(dz3s[a], w3[tid * 64 + a], s);
        s = z2 > 0.f ? s : 0.f;
        dz2s[tid] = s;
        p.dz2[b * 128 + tid] = s;
    }
    __syncthreads();
    for (int k = tid; k < 512; k += 256) {
        const float4* wr = reinterpret_cast<const float4*>(w2 + k * 128);
        float s = 0.f;
        for (int q = 0; q < 32; ++q) {
            const float4 w = wr[q];
            s = fmaf(dz2s[4 * q + 0], w.x, s);
            s = fmaf(dz2s[4 * q + 1], w.y, s);
            s = fmaf(dz2s[4 * q + 2], w.z, s);
            s = fmaf(dz2s[4 * q + 3], w.w, s);
        }
        p.dz1[(size_t)b * 512 + k] = h1s[k] > 0.f ? s : 0.f;
    }
}

// ---- 3. the small parameter gradients, one thread per output element, ascending b ----------------------------------
// gs: dW2 [512][128] | dW3 [128][64] | db1 [512] | db2 [128] | db3 [64] (the layouts of the weights); the last thread
// folds the step's statistics.
constexpr int GS_W2 = 0, GS_W3 = 512 * 128, GS_B1 = GS_W3 + 128 * 64, GS_B2 = GS_B1 + 512, GS_B3 = GS_B2 + 128, GS_END = GS_B3 + 64;

__global__ __launch_bounds__(256) void ht_param_kernel(HeadTrainParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x, B = p.B;
    float s = 0.f;
    if (i < GS_W3) {
        const int k = i >> 7, o = i & 127;
        for (int b = 0; b < B; ++b) s = fmaf(p.dz2[b * 128 + o], p.h1[(size_t)b * 512 + k], s);
    } else if (i < GS_B1) {
        const int k = (i - GS_W3) >> 6, a = (i - GS_W3) & 63;
        for (int b = 0; b < B; ++b) s = fmaf(p.dz3[b * 64 + a], p.h2[b * 128 + k], s);
    } else if (i < GS_B2) {
        for (int b = 0; b < B; ++b) s += p.dz1[(size_t)b * 512 + (i - GS_B1)];
    } else if (i < GS_B3) {
        for (int b = 0; b < B; ++b) s += p.dz2[b * 128 + (i - GS_B2)];
    } else if (i < GS_END) {
        for (int b = 0; b < B; ++b) s += p.dz3[b * 64 + (i - GS_B3)];
    } else if (i == GS_END) {
        write_train_stats(p.stats, p.stats_out, p.labels, p.hit_b, p.loss_b, B, p.A);
        return;
    } else {
        return;
    }
    p.gs[i] = s;
}

// ---- 4. dW1 (+ Adam) -------------------------------------------------------------------------------------------------
// dW1[o][t][c] = sum_b dz1[b][o] * feats[gather[b][t]][c]: M = (t, c), N = o, K = b on v_mfma_f32_32x32x2_f32 with the feature
// rows as the A operand, so that a lane's accumulator registers 4g .. 4g + 3 are four consecutive c of one o (c = 8g + 4h +
// 0..3): the epilogue reads and writes w, m and v with 16-byte accesses along c and nothing is transposed. grid (8 S, 4),
// 256 threads: workgroup (t, c0 = 128 * (x & 7), o0 = 128 y), wave (wc, wo) a 64 x 64 quarter as 2 x 2 MFMA tiles. K runs in
// ascending b, two per instruction (lane half h takes b0 + h); an odd B ends with a zero row.
template <bool STORE_G>
__global__ __launch_bounds__(256) void ht_dw1_kernel(const float* __restrict__ feats, int n_rows, const int32_t* __restrict__ gather, int B,
                                                     int S, const float* __restrict__ dz1, float* __restrict__ w, float* __restrict__ m,
                                                     float* __restrict__ v, float* __restrict__ gout, AdamScalars ak) {
    __shared__ int rows[258];
    const int tid = threadIdx.x;
    const int t = blockIdx.x >> 3, c0 = (blockIdx.x & 7) * 128, o0 = blockIdx.y * 128;
    rows[tid] = tid < B ? clamp_row(gather[tid * S + t], n_rows) : 0;
    if (tid < 2) rows[256 + tid] = 0;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, wc = wave & 1, wo = wave >> 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;
    const float* fa = feats + c0 + wc * 64 + r;
    const float* da = dz1 + o0 + wo * 64 + r;
    // four k-steps (eight b) per round, the next round's operands loaded before this round's sixteen MFMAs
    auto load = [&](int b0, float (&a0)[4], float (&a1)[4], float (&d0)[4], float (&d1)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = b0 + 2 * u + h;
            a0[u] = a1[u] = d0[u] = d1[u] = 0.f;
            if (b < B) {
                const float* fr = fa + (size_t)rows[b] * FS;
                const float* dr = da + (size_t)b * 512;
                a0[u] = fr[0];
                a1[u] = fr[32];
                d0[u] = dr[0];
                d1[u] = dr[32];
            }
        }
    };
    float a0[4], a1[4], d0[4], d1[4];
    load(0, a0, a1, d0, d1);
    for (int b0 = 0; b0 < B; b0 += 8) {
        float na0[4], na1[4], nd0[4], nd1[4];
        load(b0 + 8, na0, na1, nd0, nd1);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], d0[u], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], d1[u], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], d0[u], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], d1[u], acc[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) a0[u] = na0[u], a1[u] = na1[u], d0[u] = nd0[u], d1[u] = nd1[u];
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int o = o0 + wo * 64 + ni * 32 + r;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c0 + wc * 64 + mi * 32 + 8 * g + 4 * h;
                if (c >= FC) continue;   // the padding columns: gradient 0, never touched
                float gr[4] = {acc[mi][ni][4 * g], acc[mi][ni][4 * g + 1], acc[mi][ni][4 * g + 2], acc[mi][ni][4 * g + 3]};
                if (STORE_G) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) gout[((size_t)o * FC + c + j) * S + t] = gr[j];   // cnn1d.0.weight [512][1000][S]
                } else {
                    adam_apply4_at(w, m, v, ((size_t)o * S + t) * FS + c, gr, ak);
                }
            }
        }
}

// ---- 5. Adam on the five small tensors ------------------------------------------------------------------------------
// Element i of gs belongs to w2 | w3 | b1 | b2 | b3 (b3 holds A floats: the rest of its 64 slots has no weight).
__global__ __launch_bounds__(256) void ht_adam_kernel(HeadTrainParams p, AdamScalars ak) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int t, j;
    if (i < GS_W3) t = 2, j = i;
    else if (i < GS_B1) t = 4, j = i - GS_W3;
    else if (i < GS_B2) t = 1, j = i - GS_B1;
    else if (i < GS_B3) t = 3, j = i - GS_B2;
    else if (i < GS_B3 + p.A) t = 5, j = i - GS_B3;
    else return;
    adam_apply_at(p.w[t], p.m[t], p.v[t], j, p.gs[i], ak);
}

// ---- read-out: six tensors in the layouts above -> PyTorch layouts, concatenated in blob order ---------------------
// cnn1d.0.weight [512][1000][S] | cnn1d.0.bias [512] | classifier.0.weight [128][512] | .bias [128] | classifier.2.weight
// [A][128] | .bias [A]. src[0] == nullptr skips the first tensor (the gradient read-out: ht_dw1_kernel<true> wrote it).
__global__ __launch_bounds__(256) void ht_export_kernel(HeadTensors src, int S, int A, float* __restrict__ out) {
    const size_t n0 = (size_t)512 * FC * S;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (!src.p[0]) i += n0;
    const size_t total = n0 + 512 + 128 * 512 + 128 + (size_t)A * 128 + A;
    if (i >= total) return;
    size_t j = i;
    float val;
    if (j < n0) {
        const int t = (int)(j % S), c = (int)((j / S) % FC), o = (int)(j / ((size_t)S * FC));
        val = src.p[0][((size_t)o * S + t) * FS + c];
    } else if ((j -= n0) < 512) {
        val = src.p[1][j];
    } else if ((j -= 512) < 128 * 512) {
        const int o = (int)(j >> 9), k = (int)(j & 511);
        val = src.p[2][k * 128 + o];
    } else if ((j -= 128 * 512) < 128) {
        val = src.p[3][j];
    } else if ((j -= 128) < (size_t)A * 128) {
        const int a = (int)(j >> 7), k = (int)(j & 127);
        val = src.p[4][k * 64 + a];
    } else {
        val = src.p[5][j - (size_t)A * 128];
    }
    out[i] = val;
}

}  // namespace

size_t head_tensor_floats(int S, int A) { return (size_t)512 * FC * S + 512 + 128 * 512 + 128 + (size_t)A * 128 + A; }

hipError_t launch_head_export(const HeadTensors& src, int S, int A, float* out, hipStream_t s) {
    size_t n = head_tensor_floats(S, A);
    if (!src.p[0]) n -= (size_t)512 * FC * S;
    hipLaunchKernelGGL(ht_export_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, S, A, out);
    return hipGetLastError();
}

hipError_t launch_head_train_step(const HeadTrainParams& p, const AdamScalars& ak, hipStream_t s) {
    const int B = p.B, S = p.S;
    hipLaunchKernelGGL(ht_conv1d_kernel, dim3((B + 31) / 32, 16), dim3(256), 0, s, p.feats, p.n_rows, p.gather, B, S,
                       (const float*)p.w[0], (const float*)p.w[1], p.h1);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(ht_sample_kernel, dim3(B), dim3(256), 0, s, p);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(ht_param_kernel, dim3((GS_END + 1 + 255) / 256), dim3(256), 0, s, p);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if (p.apply) {
        hipLaunchKernelGGL(ht_dw1_kernel<false>, dim3(8 * S, 4), dim3(256), 0, s, p.feats, p.n_rows, p.gather, B, S, (const float*)p.dz1,
                           p.w[0], p.m[0], p.v[0], (float*)nullptr, ak);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        hipLaunchKernelGGL(ht_adam_kernel, dim3((GS_END + 255) / 256), dim3(256), 0, s, p, ak);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(ht_dw1_kernel<true>, dim3(8 * S, 4), dim3(256), 0, s, p.feats, p.n_rows, p.gather, B, S, (const float*)p.dz1,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr, p.grads_out, ak);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    HeadTensors g;
    g.p[0] = nullptr;
    g.p[1] = p.gs + GS_B1;
    g.p[2] = p.gs + GS_W2;
    g.p[3] = p.gs + GS_B2;
    g.p[4] = p.gs + GS_W3;
    g.p[5] = p.gs + GS_B3;
    return launch_head_export(g, S, p.A, p.grads_out, s);
}

}  // namespace pa

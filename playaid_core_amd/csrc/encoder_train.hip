// Training of ResnetTransformerDetector's transformer-encoder head on the device (pa_encoder_train_step,
// include/playaid_hip.h; DESIGN.md "Training the encoder head"): Linear(in, hidden) on the ResNet features, the time encoding
// appended -> D, `layers` post-norm nn.TransformerEncoderLayer(D, heads of 32, ff, ReLU, dropout p) over [L windows, N slots, D]
// (row r = l N + n: attention mixes the same slot of different windows), Linear(D, A), log_softmax, NLL as the mean over the
// rows whose label is not -100, back-propagation and torch.optim.Adam -- on the handle's weights where pa_encoder_forward reads
// them (PyTorch layouts; m, v and grads_out in blob order without the time encoding).
//
// Launches of one step on the caller's stream (R = L N rows), all fp32:
//   forward      launch_linear_f32 (front projection), et_append_encoding_kernel; per layer launch_linear_f32 (QKV),
//                et_attn_fwd_kernel (keeps P, writes O = (P o k0) V), launch_linear_f32 (out_proj), et_add_ln_fwd_kernel (keeps
//                x^ and rstd), launch_linear_f32 (linear1 + ReLU), et_mask_kernel (k2; p > 0 only), launch_linear_f32 (linear2),
//                et_add_ln_fwd_kernel
//   loss         et_cls_kernel per row: logits, logp, loss term, hit, dz, dX = dz W_c; et_cls_param_kernel: dW_c, db_c (+ Adam)
//                and the step's pa_train_stats (the small gradients -- this one, the biases, the LayerNorm weights -- sum the
//                rows in eight interleaved groups, combined in group order)
//   backward     per layer from the top: et_ln_bwd_kernel, et_ln_param_kernel, et_dx_kernel (dF, masked by the ReLU), et_dw_kernel
//                + et_colsum_kernel (linear2), et_dx_kernel (dX1), et_dw_kernel + et_colsum_kernel (linear1), et_ln_bwd_kernel,
//                et_ln_param_kernel, et_dx_kernel (dO), et_dw_kernel + et_colsum_kernel (out_proj), et_attn_bwd_kernel,
//                et_dx_kernel (dX), et_dw_kernel + et_colsum_kernel (in_proj); then et_dw_kernel + et_colsum_kernel for the
//                front projection and, after an applied step, two copies that refresh the handle's padded projection
// et_dx_kernel and et_dw_kernel run on v_mfma_f32_32x32x2_f32; every weight gradient's epilogue is Adam (or the store of the
// gradient for apply = 0). No kernel waits for another workgroup of its launch, every sum has a fixed order and there are no
// floating-point atomics: two runs give the same bits. The weights change in place, so every launch that reads a tensor (W_2,
// W_1, W_o, W_in in the layer's et_dx_kernel, the LayerNorm weights in et_ln_bwd_kernel, W_c in et_cls_kernel) is enqueued
// before the launch that updates it.
//
// Dropout: keep(seed, step, layer, site, i) of include/playaid_hip.h, recomputed where it is needed (forward and backward see the
// same function of the element's index); with p = 0 no kernel evaluates it.
//
// Labels outside [0, A) count as ignored (the Python wrapper refuses them; -100 is the only such value a checked caller passes).
#include "pa_kernels.h"
#include "train_common.h"
#include "encoder_handle.h"

namespace pa {
namespace {

constexpr int ET_LMAX = 64;   // windows of one step: a (slot, head)'s L x L block lives in one workgroup's LDS
constexpr int ET_HD = 32;     // head width (pa_encoder_create takes no other)

// ---- dropout ------------------------------------------------------------------------------------------------------------------
struct DropSite {
    uint32_t key, thr;   // thr == 0: no dropout, nothing is evaluated
    float scale;         // 1 / (1 - p)
};

__host__ __device__ __forceinline__ uint32_t et_mix(uint32_t x) { return hash_mix(x); }   // train_common.h

// the mask value of element i: 1 / (1 - p) where it is kept, 0 where it is dropped
__device__ __forceinline__ float et_keep(const DropSite& s, uint32_t i) {
    const uint32_t r = et_mix(et_mix(i ^ s.key) + s.key);
    return r >= s.thr ? s.scale : 0.f;
}

DropSite drop_site(uint64_t seed, int64_t step, int layer, int site, float p) {
    DropSite s;
    s.key = 0;
    s.thr = (uint32_t)(uint64_t)((double)p * 4294967296.0);
    s.scale = 1.f / (1.f - p);
    if (!s.thr) return s;
    uint32_t k = et_mix((uint32_t)seed + 0x9e3779b9u);
    k = et_mix(k ^ (uint32_t)(seed >> 32));
    k = et_mix(k ^ (uint32_t)(uint64_t)step);
    k = et_mix(k ^ (uint32_t)((uint64_t)step >> 32));
    k = et_mix(k ^ ((uint32_t)(layer * 4 + site + 1) * 0x85ebca6bu));
    s.key = k;
    return s;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------

// X[r][hidden + j] = enc[r % batch][j]
__global__ void et_append_encoding_kernel(float* __restrict__ X, const float* __restrict__ enc, int rows, int batch, int D, int hidden, int enc_dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * enc_dim) return;
    const int r = i / enc_dim, j = i - r * enc_dim;
    X[(size_t)r * D + hidden + j] = enc[(r % batch) * enc_dim + j];
}

// X[i] *= k(i) (site 2, behind the ReLU; launched with p > 0 only)
__global__ __launch_bounds__(256) void et_mask_kernel(float* __restrict__ X, uint32_t count, DropSite ds) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) X[i] *= et_keep(ds, i);
}

// Self-attention of one (slot n, head h), keeping the probabilities: grid (N, heads), one wave, lane = query. P block
// [(n heads + h)][L][L] (torch's layout of the attention weights): the scores go there first (a lane's own row), then the
// softmax (exp(s - max) / sum, as torch); O = (P o k0) V.
__global__ __launch_bounds__(64) void et_attn_fwd_kernel(const float* __restrict__ QKV, float* __restrict__ P, float* __restrict__ O, int L, int N, int D,
                                                         DropSite ds) {
    const int n = blockIdx.x, h = blockIdx.y, heads = gridDim.y, i = threadIdx.x;
    if (i >= L) return;
    const float scale = 1.f / sqrtf((float)ET_HD);
    const uint32_t pbase = (uint32_t)(n * heads + h) * (uint32_t)(L * L) + (uint32_t)(i * L);
    float* pr = P + pbase;
    const float* q = QKV + (size_t)(i * N + n) * 3 * D + h * ET_HD;
    float qr[ET_HD], acc[ET_HD];
#pragma unroll
    for (int d = 0; d < ET_HD; ++d) {
        qr[d] = q[d] * scale;   // torch scales the query before the product
        acc[d] = 0.f;
    }
    float m = -INFINITY;
    for (int j = 0; j < L; ++j) {
        const float* k = QKV + (size_t)(j * N + n) * 3 * D + D + h * ET_HD;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < ET_HD; ++d) s = fmaf(qr[d], k[d], s);
        pr[j] = s;
        m = fmaxf(m, s);
    }
    float l = 0.f;
    for (int j = 0; j < L; ++j) l += expf(pr[j] - m);
    for (int j = 0; j < L; ++j) {
        const float* v = QKV + (size_t)(j * N + n) * 3 * D + 2 * D + h * ET_HD;
        const float p = expf(pr[j] - m) / l;
        pr[j] = p;
        const float pm = ds.thr ? p * et_keep(ds, pbase + (uint32_t)j) : p;
#pragma unroll
        for (int d = 0; d < ET_HD; ++d) acc[d] = fmaf(pm, v[d], acc[d]);
    }
    float* o = O + (size_t)(i * N + n) * D + h * ET_HD;
#pragma unroll
    for (int d = 0; d < ET_HD; ++d) o[d] = acc[d];
}

// out[r] = LayerNorm(X[r] + Y[r] o k) g + b, eps 1e-5, one wave per row (as add_layernorm_kernel), keeping x^ and rstd
__global__ __launch_bounds__(64) void et_add_ln_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ g,
                                                           const float* __restrict__ b, float* __restrict__ xhat, float* __restrict__ rstd_out,
                                                           float* __restrict__ out, int D, DropSite ds) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* x = X + (size_t)r * D;
    const float* y = Y + (size_t)r * D;
    float* xh = xhat + (size_t)r * D;
    float sum = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float t = x[d] + (ds.thr ? y[d] * et_keep(ds, (uint32_t)(r * D + d)) : y[d]);
        xh[d] = t;   // (a lane's own elements: read back below)
        sum += t;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum / (float)D;
    float var = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float t = xh[d] - mean;
        var += t * t;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) var += __shfl_xor(var, o, 64);
    const float rstd = 1.f / sqrtf(var / (float)D + 1e-5f);
    for (int d = lane; d < D; d += 64) {
        const float t = (xh[d] - mean) * rstd;
        xh[d] = t;
        out[(size_t)r * D + d] = t * g[d] + b[d];
    }
    if (lane == 0) rstd_out[r] = rstd;
}

// ---- the classifier, the loss and its way back to the last layer's output, per row --------------------------------------------
struct ClsParams {
    const float* X;           // [M][D] the last layer's output
    const float *w, *b;       // [A][D], [A]
    const int32_t* labels;    // [M], -100 = ignore
    int32_t M, D, A;
    float *dz, *dX, *loss_r;  // [M][64], [M][D], [M]
    int32_t* hit_r;           // [M]
    float* stats;             // the trainer's pa_train_stats
    float* stats_out;         // the caller's, or nullptr
};

// grid M, one wave: lane = class
__global__ __launch_bounds__(64) void et_cls_kernel(ClsParams p) {
    __shared__ float dzs[64];
    __shared__ int nvalid;
    const int lane = threadIdx.x, row = blockIdx.x, D = p.D, A = p.A;
    if (lane == 0) nvalid = 0;
    __syncthreads();
    count_labelled(p.labels, p.M, A, lane, 64, &nvalid);
    __syncthreads();
    const float n = (float)max(nvalid, 1);   // no labelled row: divide by 1, every gradient is then 0
    const int label = p.labels[row];
    const bool valid = label >= 0 && label < A;
    const float* x = p.X + (size_t)row * D;
    float z = -INFINITY;
    if (lane < A) {
        const float* w = p.w + (size_t)lane * D;
        float a = 0.f;
        for (int k = 0; k < D; ++k) a = fmaf(w[k], x[k], a);
        z = a + p.b[lane];
    }
    const RowLoss r = softmax_nll_wave0(z, lane, A, label, valid, n);
    dzs[lane] = r.d;
    p.dz[(size_t)row * 64 + lane] = r.d;
    if (lane == 0) {
        p.loss_r[row] = r.loss;
        p.hit_r[row] = r.hit;
    }
    __syncthreads();
    for (int d = lane; d < D; d += 64) {
        float s = 0.f;
        for (int a = 0; a < A; ++a) s = fmaf(dzs[a], p.w[(size_t)a * D + d], s);
        p.dX[(size_t)row * D + d] = s;
    }
}

// The small gradients sum over the rows in ET_RG interleaved groups: a workgroup is 32 elements x ET_RG groups, thread (c, q)
// adds the rows q, q + ET_RG, ... in ascending order, and the element's thread of group 0 adds the ET_RG partial sums from LDS in
// group order. A fixed order, and 1 / ET_RG of the dependent trips to memory of one thread walking all rows.
constexpr int ET_RG = 8;

// dW_c [A][D] | db_c [A] (+ Adam: the two tensors lie in that order in the blob, the moments and grads_out); grid = one
// workgroup per 32 elements and a last one whose first thread folds the step's statistics.
template <bool STORE_G>
__global__ __launch_bounds__(256) void et_cls_param_kernel(ClsParams p, float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ gout, AdamScalars ak) {
    __shared__ float part[ET_RG][32];
    const int c = threadIdx.x & 31, q = threadIdx.x >> 5, M = p.M, A = p.A, D = p.D;
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x == 0) write_train_stats(p.stats, p.stats_out, p.labels, p.hit_r, p.loss_r, M, A);
        return;
    }
    const int i = blockIdx.x * 32 + c, n_w = A * D, n_end = n_w + A;
    float s = 0.f;
    if (i < n_w) {
        const int a = i / D, k = i - a * D;
        for (int r = q; r < M; r += ET_RG) s = fmaf(p.dz[(size_t)r * 64 + a], p.X[(size_t)r * D + k], s);
    } else if (i < n_end) {
        for (int r = q; r < M; r += ET_RG) s += p.dz[(size_t)r * 64 + (i - n_w)];
    }
    part[q][c] = s;
    __syncthreads();
    if (q != 0 || i >= n_end) return;
    float t = part[0][c];
#pragma unroll
    for (int g = 1; g < ET_RG; ++g) t += part[g][c];
    if (STORE_G)
        gout[i] = t;
    else
        adam_apply_at(w, m, v, (size_t)i, t, ak);
}

// ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------
// One wave per row: dy^ = dy g, dr = rstd (dy^ - mean(dy^) - x^ mean(dy^ x^)): the gradient of the LayerNorm's input, which is
// both the residual's and, times the mask of the site (drm = dr o k; drm == dr when there is no dropout), the block output's.
__global__ __launch_bounds__(64) void et_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ g, const float* __restrict__ xhat,
                                                       const float* __restrict__ rstd, float* __restrict__ dr, float* __restrict__ drm, int D,
                                                       DropSite ds) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* dyr = dy + (size_t)r * D;
    const float* xh = xhat + (size_t)r * D;
    float a = 0.f, b = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float t = dyr[d] * g[d];
        a += t;
        b = fmaf(t, xh[d], b);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const float ma = a / (float)D, mb = b / (float)D, rs = rstd[r];
    for (int d = lane; d < D; d += 64) {
        const float t = rs * (dyr[d] * g[d] - ma - xh[d] * mb);
        dr[(size_t)r * D + d] = t;
        if (ds.thr) drm[(size_t)r * D + d] = t * et_keep(ds, (uint32_t)(r * D + d));
    }
}

// d gamma [D] | d beta [D] (+ Adam on both: they lie in that order), 32 columns x ET_RG row groups per workgroup
template <bool STORE_G>
__global__ __launch_bounds__(256) void et_ln_param_kernel(const float* __restrict__ dy, const float* __restrict__ xhat, int M, int D,
                                                          float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                          float* __restrict__ gout, AdamScalars ak) {
    __shared__ float pg[ET_RG][32], pb[ET_RG][32];
    const int c = threadIdx.x & 31, q = threadIdx.x >> 5, d = blockIdx.x * 32 + c;
    float sg = 0.f, sb = 0.f;
    if (d < D)
        for (int r = q; r < M; r += ET_RG) {
            const float t = dy[(size_t)r * D + d];
            sg = fmaf(t, xhat[(size_t)r * D + d], sg);
            sb += t;
        }
    pg[q][c] = sg;
    pb[q][c] = sb;
    __syncthreads();
    if (q != 0 || d >= D) return;
    sg = pg[0][c];
    sb = pb[0][c];
#pragma unroll
    for (int g = 1; g < ET_RG; ++g) {
        sg += pg[g][c];
        sb += pb[g][c];
    }
    if (STORE_G) {
        gout[d] = sg;
        gout[D + d] = sb;
    } else {
        adam_apply_at(w, m, v, (size_t)d, sg, ak);
        adam_apply_at(w, m, v, (size_t)(D + d), sb, ak);
    }
}

// a bias gradient: the column sums of dA [M][ld] (n columns) (+ Adam), 32 columns x ET_RG row groups per workgroup
template <bool STORE_G>
__global__ __launch_bounds__(256) void et_colsum_kernel(const float* __restrict__ dA, int ld, int M, int n, float* __restrict__ w,
                                                        float* __restrict__ m, float* __restrict__ v, float* __restrict__ gout, AdamScalars ak) {
    __shared__ float part[ET_RG][32];
    const int c = threadIdx.x & 31, q = threadIdx.x >> 5, k = blockIdx.x * 32 + c;
    float s = 0.f;
    if (k < n)
        for (int r = q; r < M; r += ET_RG) s += dA[(size_t)r * ld + k];
    part[q][c] = s;
    __syncthreads();
    if (q != 0 || k >= n) return;
    s = part[0][c];
#pragma unroll
    for (int g = 1; g < ET_RG; ++g) s += part[g][c];
    if (STORE_G)
        gout[k] = s;
    else
        adam_apply_at(w, m, v, (size_t)k, s, ak);
}

// ---- attention backward -----------------------------------------------------------------------------------------------------------
// One workgroup per (slot n, head h), 256 threads; Q (scaled, as the forward pass forms it), K, V, dO [L][32] and one L x L block
// in LDS (49 KB). With P the kept probabilities and k0 the site's mask:
//   dV = (P o k0)^T dO;  dP = (dO V^T) o k0;  dS = P o (dP - rowsum(dP o P));  dQ = dS K / sqrt(32);  dK = dS^T (Q / sqrt(32))
// every sum ascending in its index. Writes the (n, h) part of dQKV [R][3D].
__global__ __launch_bounds__(256) void et_attn_bwd_kernel(const float* __restrict__ QKV, const float* __restrict__ P, const float* __restrict__ dO,
                                                          float* __restrict__ dQKV, int L, int N, int D, DropSite ds) {
    __shared__ float qs[ET_LMAX][ET_HD + 1], ks[ET_LMAX][ET_HD + 1], vs[ET_LMAX][ET_HD + 1], dos[ET_LMAX][ET_HD + 1];
    __shared__ float as[ET_LMAX][ET_LMAX + 1];
    __shared__ float rs[ET_LMAX];
    const int n = blockIdx.x, h = blockIdx.y, heads = gridDim.y, tid = threadIdx.x;
    const float scale = 1.f / sqrtf((float)ET_HD);
    const uint32_t pbase = (uint32_t)(n * heads + h) * (uint32_t)(L * L);
    const float* Pb = P + pbase;
    for (int idx = tid; idx < L * ET_HD; idx += 256) {
        const int i = idx / ET_HD, d = idx % ET_HD;
        const size_t row = (size_t)(i * N + n);
        const float* base = QKV + row * 3 * D + h * ET_HD + d;
        qs[i][d] = base[0] * scale;
        ks[i][d] = base[D];
        vs[i][d] = base[2 * D];
        dos[i][d] = dO[row * D + h * ET_HD + d];
    }
    for (int idx = tid; idx < L * L; idx += 256) {
        const int i = idx / L, j = idx - i * L;
        const float p = Pb[idx];
        as[i][j] = ds.thr ? p * et_keep(ds, pbase + (uint32_t)idx) : p;
    }
    __syncthreads();
    for (int idx = tid; idx < L * ET_HD; idx += 256) {   // dV
        const int j = idx / ET_HD, d = idx % ET_HD;
        float s = 0.f;
        for (int i = 0; i < L; ++i) s = fmaf(as[i][j], dos[i][d], s);
        dQKV[(size_t)(j * N + n) * 3 * D + 2 * D + h * ET_HD + d] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < L * L; idx += 256) {   // dP
        const int i = idx / L, j = idx - i * L;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < ET_HD; ++d) s = fmaf(dos[i][d], vs[j][d], s);
        as[i][j] = ds.thr ? s * et_keep(ds, pbase + (uint32_t)idx) : s;
    }
    __syncthreads();
    if (tid < L) {
        float s = 0.f;
        for (int j = 0; j < L; ++j) s = fmaf(as[tid][j], Pb[tid * L + j], s);
        rs[tid] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < L * L; idx += 256) {   // dS
        const int i = idx / L, j = idx - i * L;
        as[i][j] = Pb[idx] * (as[i][j] - rs[i]);
    }
    __syncthreads();
    for (int idx = tid; idx < L * ET_HD; idx += 256) {   // dQ and dK of row i = idx / 32
        const int i = idx / ET_HD, d = idx % ET_HD;
        float sq = 0.f, sk = 0.f;
        for (int j = 0; j < L; ++j) {
            sq = fmaf(as[i][j], ks[j][d], sq);
            sk = fmaf(as[j][i], qs[j][d], sk);
        }
        float* out = dQKV + (size_t)(i * N + n) * 3 * D + h * ET_HD + d;
        out[0] = sq * scale;
        out[D] = sk;
    }
}

// ---- dX = dA W: [M][K] x [K][C] ---------------------------------------------------------------------------------------------------
// grid (C / 32, ceil(M / 32)), 256 threads: one 32 (c) x 32 (rows) tile of v_mfma_f32_32x32x2_f32 per workgroup, the rows of W
// ([K][C] row-major: a PyTorch weight [out = K][in = C]) as the A operand (reads along c), dA as the B operand, so that a lane
// ends with four consecutive c of one row. K is a multiple of 32: wave w takes the rounds of 32 k with round % 4 == w,
// ascending, all of a round's operands requested before its sixteen instructions; the four partial tiles are summed through LDS
// in wave order. MODE 0: dX = the product; 1: + aux (the residual's gradient, [M][C]); 2: times scale where aux > 0, else 0 (aux
// = the kept ReLU output o k2 -- positive exactly where the unit is active and kept --, scale = 1 / (1 - p)).
template <int MODE>
__global__ __launch_bounds__(256) void et_dx_kernel(const float* __restrict__ dA, const float* __restrict__ W, float* __restrict__ dX,
                                                    const float* __restrict__ aux, float scale, int M, int C, int K) {
    __shared__ __attribute__((aligned(16))) float part[4][32][36];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
    const float* wp = W + c0 + r;
    const float* dp = dA + (size_t)min(m0 + r, M - 1) * K;   // (rows past M read the last row; their results are not stored)
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k0 = wave * 32; k0 < K; k0 += 128) {
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
    if (m0 + row >= M) return;
    const size_t idx = (size_t)(m0 + row) * C + c0 + c4;   // (C is a multiple of 32 and every buffer 16-byte aligned)
    if (MODE == 1) {
        const float4 x = *reinterpret_cast<const float4*>(aux + idx);
        s.x += x.x;
        s.y += x.y;
        s.z += x.z;
        s.w += x.w;
    } else if (MODE == 2) {
        const float4 x = *reinterpret_cast<const float4*>(aux + idx);
        s.x = x.x > 0.f ? s.x * scale : 0.f;   // ReLU's derivative at 0 is 0
        s.y = x.y > 0.f ? s.y * scale : 0.f;
        s.z = x.z > 0.f ? s.z * scale : 0.f;
        s.w = x.w > 0.f ? s.w * scale : 0.f;
    }
    *reinterpret_cast<float4*>(dX + idx) = s;
}

// ---- a weight gradient (+ Adam) ---------------------------------------------------------------------------------------------------
// dW[o][c] = sum_r D[r][o] X[r][c] for o < O, c < C, r < K, on v_mfma_f32_32x32x2_f32 with the X rows as the A operand (M = c)
// and the D rows as the B operand (N = o): a lane's accumulator registers 4g .. 4g + 3 are the four consecutive c = 8g + 4h +
// 0..3 of one o. grid (ceil(C / 64), ceil(O / 64)), 256 threads: wave (wc, wo) one 32 x 32 tile of the workgroup's 64 x 64. One
// workgroup owns its tile for all of K, ascending, two rows per instruction (lane half h takes row r0 + h); an odd K ends with
// a zero row. Columns c >= C and o >= O are loaded as zero and never stored: edge tiles are exact. The epilogue goes element
// by element (the blob's tensors are 4-byte aligned only: 247 biases and 63 encoding values lie in front of the layers).
// STORE_G: the gradient to gout [O][C] instead, the state untouched.
template <bool STORE_G>
__global__ __launch_bounds__(256) void et_dw_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ D, int ldd, int K, int O, int C,
                                                    float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ gout, AdamScalars ak) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, wc = wave & 1, wo = wave >> 1;
    const int cl = blockIdx.x * 64 + wc * 32 + r;     // this lane's column of X (A operand)
    const int o = blockIdx.y * 64 + wo * 32 + r;      // this lane's column of D (B operand) and its output row
    const bool c_ok = cl < C, o_ok = o < O;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* xa = X + (c_ok ? cl : 0);
    const float* da = D + (o_ok ? o : 0);
    for (int r0 = 0; r0 < K; r0 += 32) {   // sixteen k-steps per round, all of a round's operands requested before its instructions
        float a[16], d[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int row = r0 + 2 * u + h;
            a[u] = d[u] = 0.f;
            if (row < K) {
                if (c_ok) a[u] = xa[(size_t)row * ldx];
                if (o_ok) d[u] = da[(size_t)row * ldd];
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], d[u], acc, 0, 0, 0);
    }
    if (!o_ok) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = blockIdx.x * 64 + wc * 32 + 8 * g + 4 * h;
        const float gr[4] = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        const size_t idx = (size_t)o * C + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c + j >= C) continue;
            if (STORE_G)
                gout[idx + j] = gr[j];
            else
                adam_apply_at(w, m, v, idx + j, gr[j], ak);
        }
    }
}

}  // namespace
}  // namespace pa

// =====================================================================================
// The trainer: a handle beside its pa_encoder
// =====================================================================================

struct pa_encoder_trainer : pa::TrainerCore {   // state: m | v (blob order without the encoding) | saved activations | scratch
    pa_encoder* h = nullptr;
    size_t nw = 0;            // floats of one trained tensor set
    size_t n_front = 0;       // floats of resnet_ffn.weight and .bias: what lies in front of the encoding in the blob
    size_t n_enc = 0;         // floats of the encoding
    float dropout = 0.f;
    uint64_t seed = 0;
    int max_windows = 0;
    float *m = nullptr, *v = nullptr;
    struct Act { float *x, *qkv, *p, *o, *xh1, *rs1, *x1, *f, *xh2, *rs2; };
    std::vector<Act> act;     // per layer; act[l + 1].x is layer l's output (act[layers] has x alone)
    float *y = nullptr, *dxa = nullptr, *dr = nullptr, *drm = nullptr, *df = nullptr, *dx1 = nullptr, *d_o = nullptr, *dqkv = nullptr;
    float *dz = nullptr, *loss_r = nullptr, *stats = nullptr;
    int32_t* hit_r = nullptr;
};

namespace {

int encoder_max_windows(const pa_encoder* h) {
    const int w = h->max_rows / h->slots;
    return w < pa::ET_LMAX ? w : pa::ET_LMAX;
}

size_t encoder_trained_floats(const pa_encoder* h) {
    return pa::encoder_float_count(h->in_dim, h->hidden, h->slots, h->enc_dim, h->layers, h->ff, h->actions) - (size_t)h->slots * h->enc_dim;
}

// nullptr where the handle can be trained, else why not
const char* encoder_untrainable(const pa_encoder* h) {
    if (h->actions > 64) return "pa_encoder_trainer_create: training needs num_actions <= 64 (this handle serves inference only)";
    if (h->ff % 32 != 0 || h->D % 32 != 0) return "pa_encoder_trainer_create: training needs ff_dim and hidden_dim + enc_dim to be multiples of 32";
    if (h->max_rows < h->slots) return "pa_encoder_trainer_create: max_rows holds no window";
    if ((unsigned long long)h->max_rows * (unsigned long long)(h->ff > h->D ? h->ff : h->D) >= (1ull << 31) ||
        (unsigned long long)h->slots * h->heads * pa::ET_LMAX * pa::ET_LMAX >= (1ull << 31))
        return "pa_encoder_trainer_create: max_rows x ff_dim exceeds the 32-bit element index of the dropout masks";
    return nullptr;
}

}  // namespace

using pa::trainer_fail;

extern "C" {

size_t pa_encoder_trainer_floats(const pa_encoder* h) { return h ? encoder_trained_floats(h) : 0; }

int32_t pa_encoder_trainer_max_windows(const pa_encoder* h) { return h ? encoder_max_windows(h) : 0; }

int pa_encoder_trainer_create(pa_encoder* h, const pa_adam_config* cfg, float dropout, uint64_t seed, pa_encoder_trainer** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (!h || !cfg) return PA_ERR_INVALID_ARG;
    if (!pa::adam_config_ok(cfg->lr, cfg->beta1, cfg->beta2, cfg->eps)) return PA_ERR_INVALID_ARG;
    if (!(dropout >= 0.f && dropout < 1.f)) {
        h->last_error = "pa_encoder_trainer_create: dropout must be in [0, 1)";
        return PA_ERR_INVALID_ARG;
    }
    if (const char* why = encoder_untrainable(h)) {
        h->last_error = why;
        return PA_ERR_INVALID_ARG;
    }
    pa_encoder_trainer* t = new pa_encoder_trainer();
    *out = t;   // (handed back whatever follows: TrainerCore)
    t->h = h;
    t->cfg = *cfg;
    t->dropout = dropout;
    t->seed = seed;
    t->nw = encoder_trained_floats(h);
    t->n_front = (size_t)h->hidden * h->in_dim + h->hidden;
    t->n_enc = (size_t)h->slots * h->enc_dim;
    t->max_windows = encoder_max_windows(h);
    if (!h->weights || !h->x) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_encoder_trainer_create: the handle has no weights on a device");
    if (hipSetDevice(h->device) != hipSuccess) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_encoder_trainer_create: hipSetDevice failed");
    auto r64 = [](size_t n) { return (n + 63) & ~(size_t)63; };   // (every buffer starts 256-byte aligned)
    const size_t R = (size_t)t->max_windows * h->slots, D = (size_t)h->D, F = (size_t)h->ff, NL = (size_t)h->layers;
    const size_t nP = r64((size_t)h->slots * h->heads * t->max_windows * t->max_windows);
    const size_t RD = r64(R * D), RF = r64(R * F), R3 = r64(R * 3 * D), R1 = r64(R);
    const size_t nw = r64(t->nw);
    const size_t per_layer = RD + R3 + nP + RD + RD + R1 + RD + RF + RD + R1;
    const size_t scratch = RD * 6 + RF + R3 + r64(R * 64) + 2 * R1 + 64;
    if (const int rc = pa::trainer_alloc_zeroed(t, 2 * nw + NL * per_layer + RD + scratch, "pa_encoder_trainer_create")) return rc;
    float* q = t->state;
    auto take = [&](size_t n) { float* r = q; q += n; return r; };
    t->m = take(nw);
    t->v = take(nw);
    t->act.resize(NL + 1);
    for (size_t l = 0; l < NL; ++l) {
        pa_encoder_trainer::Act& a = t->act[l];
        a.x = take(RD), a.qkv = take(R3), a.p = take(nP), a.o = take(RD), a.xh1 = take(RD), a.rs1 = take(R1), a.x1 = take(RD), a.f = take(RF);
        a.xh2 = take(RD), a.rs2 = take(R1);
    }
    memset(&t->act[NL], 0, sizeof(pa_encoder_trainer::Act));
    t->act[NL].x = take(RD);
    t->y = take(RD), t->dxa = take(RD), t->dr = take(RD), t->drm = take(RD), t->dx1 = take(RD), t->d_o = take(RD);
    t->df = take(RF);
    t->dqkv = take(R3);
    t->dz = take(r64(R * 64));
    t->loss_r = take(R1);
    t->hit_r = reinterpret_cast<int32_t*>(take(R1));
    t->stats = take(64);
    return PA_OK;
}

void pa_encoder_trainer_destroy(pa_encoder_trainer* t) { pa::trainer_destroy(t); }

const char* pa_encoder_trainer_last_error(const pa_encoder_trainer* t) { return pa::trainer_last_error(t); }

int64_t pa_encoder_trainer_steps(const pa_encoder_trainer* t) { return pa::trainer_steps(t); }

int pa_encoder_train_step(pa_encoder_trainer* t, const float* feats, int32_t ld, int32_t seq_len, int32_t batch, const int32_t* labels, int32_t apply,
                          float* grads_out, pa_train_stats* stats_dev, void* stream) {
    using namespace pa;
    if (!t) return PA_ERR_INVALID_ARG;
    pa_encoder* h = t->h;
    if (!feats || !labels) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_encoder_train_step: null input");
    if (seq_len < 1 || batch < 1) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_encoder_train_step: seq_len < 1 or batch < 1");
    if (batch != h->slots)
        return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_encoder_train_step: batch must equal the number of encoded slots (sequence_length)");
    if (ld < h->in_dim) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_encoder_train_step: ld < in_dim");
    if (const int rc = trainer_check_apply(t, apply, grads_out, "pa_encoder_train_step")) return rc;
    if (seq_len > t->max_windows)
        return trainer_fail(t, PA_ERR_CAPACITY, "pa_encoder_train_step: seq_len exceeds pa_encoder_trainer_max_windows (" + std::to_string(t->max_windows) +
                                                    " windows per step)");
    if (!t->state) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_encoder_train_step: the trainer has no device state");
    hipStream_t s = (hipStream_t)stream;
    const int D = h->D, F = h->ff, A = h->actions, NL = h->layers, L = seq_len, N = batch, R = L * N, heads = h->heads;
    const AdamScalars ak = adam_scalars(t->cfg.lr, t->cfg.beta1, t->cfg.beta2, t->cfg.eps, t->steps + 1, apply != 0);
    hipError_t err = hipSuccess;
    auto fail = [&](hipError_t e) { return trainer_fail(t, PA_ERR_HIP, std::string("pa_encoder_train_step: ") + hipGetErrorString(e)); };
    // a tensor of the handle -> the same tensor of m, v or grads_out (blob order without the encoding)
    auto off = [&](const float* wp) {
        const size_t o = (size_t)(wp - h->weights);
        return o < t->n_front ? o : o - t->n_enc;
    };
    auto site = [&](int layer, int k) { return drop_site(t->seed, t->steps, layer, k, t->dropout); };
    const bool drop = site(0, 0).thr != 0;
#define ET_CHECK()                                               \
    do {                                                         \
        if ((err = hipGetLastError()) != hipSuccess) return fail(err); \
    } while (0)
#define ET_HIP(call)                                       \
    do {                                                   \
        if ((err = (call)) != hipSuccess) return fail(err); \
    } while (0)
    // dW (+ Adam) and db (+ Adam) of one Linear: weight wp [O][C] with its bias behind it in the blob; Dm [R][ldd] the gradient
    // of its output, X [R][ldx] its input
    auto linear_grads = [&](const float* X, int ldx, const float* Dm, int ldd, int O, int C, float* wp, float* bp) -> hipError_t {
        const size_t ow = off(wp), ob = off(bp);
        const dim3 grid((C + 63) / 64, (O + 63) / 64), gb((O + 31) / 32);
        if (apply) {
            hipLaunchKernelGGL(et_dw_kernel<false>, grid, dim3(256), 0, s, X, ldx, Dm, ldd, R, O, C, wp, t->m + ow, t->v + ow, (float*)nullptr, ak);
            hipLaunchKernelGGL(et_colsum_kernel<false>, gb, dim3(256), 0, s, Dm, ldd, R, O, bp, t->m + ob, t->v + ob, (float*)nullptr, ak);
        } else {
            hipLaunchKernelGGL(et_dw_kernel<true>, grid, dim3(256), 0, s, X, ldx, Dm, ldd, R, O, C, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                               grads_out + ow, ak);
            hipLaunchKernelGGL(et_colsum_kernel<true>, gb, dim3(256), 0, s, Dm, ldd, R, O, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                               grads_out + ob, ak);
        }
        return hipGetLastError();
    };
    // d gamma | d beta (+ Adam) of one LayerNorm: gp [D] with its bias behind it
    auto norm_grads = [&](const float* dy, const float* xhat, float* gp) -> hipError_t {
        const size_t og = off(gp);
        if (apply)
            hipLaunchKernelGGL(et_ln_param_kernel<false>, dim3((D + 31) / 32), dim3(256), 0, s, dy, xhat, R, D, gp, t->m + og, t->v + og,
                               (float*)nullptr, ak);
        else
            hipLaunchKernelGGL(et_ln_param_kernel<true>, dim3((D + 31) / 32), dim3(256), 0, s, dy, xhat, R, D, (float*)nullptr, (float*)nullptr,
                               (float*)nullptr, grads_out + og, ak);
        return hipGetLastError();
    };

    // ---- forward ----
    // (the padded copy of the projection where the handle keeps one -- it is refreshed behind every applied step --: whole matrix
    // tiles, as in pa_encoder_forward; its zero rows write zeros where the encoding goes next)
    if (h->ffn_pad)
        ET_HIP(launch_linear_f32(feats, ld, h->ffn_pad, h->ffn_pad + (size_t)D * h->in_dim, t->act[0].x, D, R, D, h->in_dim, 0, s));
    else
        ET_HIP(launch_linear_f32(feats, ld, h->ffn_w, h->ffn_b, t->act[0].x, D, R, h->hidden, h->in_dim, 0, s));
    if (h->enc_dim > 0) {
        const int total = R * h->enc_dim;
        hipLaunchKernelGGL(et_append_encoding_kernel, dim3((total + 255) / 256), dim3(256), 0, s, t->act[0].x, (const float*)h->enc, R, N, D, h->hidden,
                           h->enc_dim);
        ET_CHECK();
    }
    for (int l = 0; l < NL; ++l) {
        const pa_encoder::Layer& W = h->layer[l];
        const pa_encoder_trainer::Act& a = t->act[l];
        ET_HIP(launch_linear_f32(a.x, D, W.in_w, W.in_b, a.qkv, 3 * D, R, 3 * D, D, 0, s));
        hipLaunchKernelGGL(et_attn_fwd_kernel, dim3(N, heads), dim3(64), 0, s, (const float*)a.qkv, a.p, a.o, L, N, D, site(l, 0));
        ET_CHECK();
        ET_HIP(launch_linear_f32(a.o, D, W.out_w, W.out_b, t->y, D, R, D, D, 0, s));
        hipLaunchKernelGGL(et_add_ln_fwd_kernel, dim3(R), dim3(64), 0, s, (const float*)a.x, (const float*)t->y, (const float*)W.n1_g,
                           (const float*)W.n1_b, a.xh1, a.rs1, a.x1, D, site(l, 1));
        ET_CHECK();
        ET_HIP(launch_linear_f32(a.x1, D, W.l1_w, W.l1_b, a.f, F, R, F, D, 1, s));
        if (drop) {
            const uint32_t count = (uint32_t)R * (uint32_t)F;
            hipLaunchKernelGGL(et_mask_kernel, dim3((count + 255) / 256), dim3(256), 0, s, a.f, count, site(l, 2));
            ET_CHECK();
        }
        ET_HIP(launch_linear_f32(a.f, F, W.l2_w, W.l2_b, t->y, D, R, D, F, 0, s));
        hipLaunchKernelGGL(et_add_ln_fwd_kernel, dim3(R), dim3(64), 0, s, (const float*)a.x1, (const float*)t->y, (const float*)W.n2_g,
                           (const float*)W.n2_b, a.xh2, a.rs2, t->act[l + 1].x, D, site(l, 3));
        ET_CHECK();
    }
    // ---- the classifier and the loss ----
    ClsParams cp;
    memset(&cp, 0, sizeof(cp));
    cp.X = t->act[NL].x;
    cp.w = h->cls_w, cp.b = h->cls_b;
    cp.labels = labels;
    cp.M = R, cp.D = D, cp.A = A;
    cp.dz = t->dz, cp.dX = t->dxa, cp.loss_r = t->loss_r, cp.hit_r = t->hit_r;
    cp.stats = t->stats;
    cp.stats_out = reinterpret_cast<float*>(stats_dev);
    hipLaunchKernelGGL(et_cls_kernel, dim3(R), dim3(64), 0, s, cp);
    ET_CHECK();
    {   // (et_cls_kernel has read the classifier: it may change now)
        const size_t oc = off(h->cls_w);
        const dim3 grid((A * D + A + 31) / 32 + 1);
        if (apply)
            hipLaunchKernelGGL(et_cls_param_kernel<false>, grid, dim3(256), 0, s, cp, h->cls_w, t->m + oc, t->v + oc, (float*)nullptr, ak);
        else
            hipLaunchKernelGGL(et_cls_param_kernel<true>, grid, dim3(256), 0, s, cp, (float*)nullptr, (float*)nullptr, (float*)nullptr, grads_out + oc, ak);
        ET_CHECK();
    }
    // ---- backward, from the top layer; t->dxa is the gradient of the layer's output ----
    float* drm = drop ? t->drm : t->dr;   // the masked copy of a LayerNorm's input gradient: without dropout the gradient itself
    const dim3 gx_d(D / 32, (R + 31) / 32), gx_f(F / 32, (R + 31) / 32);
    for (int l = NL - 1; l >= 0; --l) {
        const pa_encoder::Layer& W = h->layer[l];
        const pa_encoder_trainer::Act& a = t->act[l];
        const DropSite s0 = site(l, 0), s1 = site(l, 1), s2 = site(l, 2), s3 = site(l, 3);
        // norm2 and the feed-forward block
        hipLaunchKernelGGL(et_ln_bwd_kernel, dim3(R), dim3(64), 0, s, (const float*)t->dxa, (const float*)W.n2_g, (const float*)a.xh2,
                           (const float*)a.rs2, t->dr, drm, D, s3);
        ET_CHECK();
        ET_HIP(norm_grads(t->dxa, a.xh2, W.n2_g));
        hipLaunchKernelGGL(et_dx_kernel<2>, gx_f, dim3(256), 0, s, (const float*)drm, (const float*)W.l2_w, t->df, (const float*)a.f, s2.scale, R, F, D);
        ET_CHECK();
        ET_HIP(linear_grads(a.f, F, drm, D, D, F, W.l2_w, W.l2_b));
        hipLaunchKernelGGL(et_dx_kernel<1>, gx_d, dim3(256), 0, s, (const float*)t->df, (const float*)W.l1_w, t->dx1, (const float*)t->dr, 1.f, R, D, F);
        ET_CHECK();
        ET_HIP(linear_grads(a.x1, D, t->df, F, F, D, W.l1_w, W.l1_b));
        // norm1 and the attention block
        hipLaunchKernelGGL(et_ln_bwd_kernel, dim3(R), dim3(64), 0, s, (const float*)t->dx1, (const float*)W.n1_g, (const float*)a.xh1,
                           (const float*)a.rs1, t->dr, drm, D, s1);
        ET_CHECK();
        ET_HIP(norm_grads(t->dx1, a.xh1, W.n1_g));
        hipLaunchKernelGGL(et_dx_kernel<0>, gx_d, dim3(256), 0, s, (const float*)drm, (const float*)W.out_w, t->d_o, (const float*)nullptr, 1.f, R, D, D);
        ET_CHECK();
        ET_HIP(linear_grads(a.o, D, drm, D, D, D, W.out_w, W.out_b));
        hipLaunchKernelGGL(et_attn_bwd_kernel, dim3(N, heads), dim3(256), 0, s, (const float*)a.qkv, (const float*)a.p, (const float*)t->d_o, t->dqkv, L,
                           N, D, s0);
        ET_CHECK();
        hipLaunchKernelGGL(et_dx_kernel<1>, gx_d, dim3(256), 0, s, (const float*)t->dqkv, (const float*)W.in_w, t->dxa, (const float*)t->dr, 1.f, R, D,
                           3 * D);
        ET_CHECK();
        ET_HIP(linear_grads(a.x, D, t->dqkv, 3 * D, 3 * D, D, W.in_w, W.in_b));
    }
    // the front projection: the first `hidden` columns of the first layer's input gradient (the encoding's columns are dropped)
    ET_HIP(linear_grads(feats, ld, t->dxa, D, h->hidden, h->in_dim, h->ffn_w, h->ffn_b));
    if (apply && h->ffn_pad) {   // what pa_encoder_forward reads at this shape: its rows [hidden, D) stay zero
        ET_HIP(hipMemcpyAsync(h->ffn_pad, h->ffn_w, (size_t)h->hidden * h->in_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
        ET_HIP(hipMemcpyAsync(h->ffn_pad + (size_t)D * h->in_dim, h->ffn_b, (size_t)h->hidden * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
#undef ET_CHECK
#undef ET_HIP
    if (apply) t->steps += 1;
    return PA_OK;
}

int pa_encoder_trainer_read(pa_encoder_trainer* t, int32_t which, float* out_dev, size_t floats, void* stream) {
    if (!t) return PA_ERR_INVALID_ARG;
    // (PA_TRAIN_RAW is refused too: the tensors lie in PyTorch layouts, there is no other form)
    if (const int rc = pa::trainer_check_which(t, which, out_dev, "pa_encoder_trainer_read")) return rc;
    if (floats != t->nw) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_encoder_trainer_read: wrong output size");
    if (!t->state) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_encoder_trainer_read: the trainer has no device state");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (which == PA_TRAIN_WEIGHTS) {   // the blob without the encoding
        e = hipMemcpyAsync(out_dev, t->h->weights, t->n_front * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(out_dev + t->n_front, t->h->weights + t->n_front + t->n_enc, (t->nw - t->n_front) * sizeof(float),
                               hipMemcpyDeviceToDevice, s);
    } else {
        e = hipMemcpyAsync(out_dev, which == PA_TRAIN_M ? t->m : t->v, t->nw * sizeof(float), hipMemcpyDeviceToDevice, s);
    }
    if (e != hipSuccess) return trainer_fail(t, PA_ERR_HIP, "pa_encoder_trainer_read: hipMemcpyAsync failed");
    return PA_OK;
}

}  // extern "C"

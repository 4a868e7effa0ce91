// Scoring of log-probabilities against labels on the device (pa_eval_*, include/playaid_hip.h): what the reference's
// validation_step / test_step (cnn_action_detector.py:131-163: F.nll_loss + a multiclass top-1 Accuracy) and its confusion
// matrix script (visualizations/cnn_action_detector_vis.py:89-153) compute, accumulated over any number of calls.
//
// eval_rows_kernel: one wave64 per row. The lanes stride over the A columns, a shuffle reduction finds the maximum with the
// first-index tie break of head_mlp_kernel (misc.hip) and torch.argmax, then -logp[y] and exp(logp[pred]) are taken in double.
//
// Determinism: the integer counts and the confusion matrix are 64-bit integer atomicAdds -- integer
// addition commutes, any order gives the same value. The two double sums use no floating-point atomics: a wave adds its rows
// in row order, thread 0 of a workgroup adds the workgroup's waves in wave order and writes ONE partial per workgroup into a
// slab, and eval_fold_kernel (one wave, second launch) adds the slab in a fixed order to the running sums. The row -> wave
// assignment depends on n alone, so the same calls in the same order give the same bits.
#include "pa_kernels.h"
#include "../../include/playaid_hip.h"

namespace pa {
namespace {

constexpr int EVAL_WAVES = 4;  // waves (rows in flight) per workgroup

__global__ __launch_bounds__(EVAL_WAVES * 64) void eval_rows_kernel(const float* __restrict__ logp, int ld, int n, int A,
                                                                    const int32_t* __restrict__ labels, int label_stride,
                                                                    unsigned long long* __restrict__ counts,
                                                                    unsigned long long* __restrict__ confusion,
                                                                    double* __restrict__ slab) {
    __shared__ double s_sum[EVAL_WAVES][2];
    __shared__ unsigned long long s_cnt[EVAL_WAVES][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double nll = 0.0, conf = 0.0;
    unsigned long long rows = 0, correct = 0, ignored = 0, bad = 0;
    // (row i of wave w of workgroup g: i = (k * gridDim.x + g) * EVAL_WAVES + w, k = 0, 1, ...)
    for (long long i = (long long)blockIdx.x * EVAL_WAVES + wave; i < n; i += (long long)gridDim.x * EVAL_WAVES) {
        const float* row = logp + (size_t)i * ld;
        // argmax with first-index tie break (torch.argmax); a lane keeps its first maximum, lanes without a column lose every tie
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (lane < A) {
            bv = row[lane];
            bi = lane;
        }
        for (int a = lane + 64; a < A; a += 64) {
            const float v = row[a];
            if (v > bv) {
                bv = v;
                bi = a;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(bv, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane != 0) continue;
        const int y = labels[(size_t)i * label_stride];
        if (y == PA_EVAL_IGNORE) {
            ++ignored;
        } else if (y < 0 || y >= A) {
            ++bad;
        } else {
            ++rows;
            correct += (bi == y);
            nll += -(double)row[y];
            conf += exp((double)bv);
            atomicAdd(&confusion[(size_t)y * A + bi], 1ull);
        }
    }
    if (lane == 0) {
        s_sum[wave][0] = nll;
        s_sum[wave][1] = conf;
        s_cnt[wave][0] = rows;
        s_cnt[wave][1] = correct;
        s_cnt[wave][2] = ignored;
        s_cnt[wave][3] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = s_sum[0][0], t1 = s_sum[0][1];
#pragma unroll
        for (int w = 1; w < EVAL_WAVES; ++w) {
            t0 += s_sum[w][0];
            t1 += s_sum[w][1];
        }
        slab[2 * blockIdx.x + 0] = t0;
        slab[2 * blockIdx.x + 1] = t1;
    }
    if (threadIdx.x < 4) {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < EVAL_WAVES; ++w) c += s_cnt[w][threadIdx.x];
        if (c) atomicAdd(&counts[threadIdx.x], c);
    }
}

// One wave: lane l adds partials l, l + 64, ... in index order, the 64 lane sums go through a fixed shuffle tree (both
// partners of a step compute the same a + b), and lane 0 adds the total to the running sums.
__global__ __launch_bounds__(64) void eval_fold_kernel(const double* __restrict__ slab, int parts, double* __restrict__ sums) {
    const int lane = threadIdx.x;
    double t0 = 0.0, t1 = 0.0;
    for (int i = lane; i < parts; i += 64) {
        t0 += slab[2 * i + 0];
        t1 += slab[2 * i + 1];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        t0 += __shfl_xor(t0, d, 64);
        t1 += __shfl_xor(t1, d, 64);
    }
    if (lane == 0) {
        sums[0] += t0;
        sums[1] += t1;
    }
}

}  // namespace

// counts: {rows, correct, ignored, bad_labels}; sums: {nll_sum, conf_sum}; slab: 2 * EVAL_SLAB_PARTS doubles
hipError_t launch_eval_rows(const float* logp, int ld, int n, int A, const int32_t* labels, int label_stride, unsigned long long* counts,
                            double* sums, unsigned long long* confusion, double* slab, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const long long groups = ((long long)n + EVAL_WAVES - 1) / EVAL_WAVES;
    const int parts = (int)(groups < EVAL_SLAB_PARTS ? groups : EVAL_SLAB_PARTS);
    hipLaunchKernelGGL(eval_rows_kernel, dim3(parts), dim3(EVAL_WAVES * 64), 0, s, logp, ld, n, A, labels, label_stride, counts, confusion, slab);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)slab, parts, sums);
    return hipGetLastError();
}

}  // namespace pa

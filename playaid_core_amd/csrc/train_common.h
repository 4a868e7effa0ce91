// What the trainers (head_train.hip with its handle in pa_api.hip, lstm_train.hip) share: the loss of one row in wave 0, the
// count of labelled rows, the fold of a step's pa_train_stats, the Adam update with the host-side scalars that go with it, and
// the host-side core of a trainer handle. The kernels that call these stay their files' own: they differ in tile shape, gather,
// prefetch and weight layouts.
#pragma once
#include "pa_kernels.h"
#include "../../include/playaid_hip.h"
#include <cmath>
#include <cstring>
#include <string>

namespace pa {

typedef float f32x16 __attribute__((ext_vector_type(16)));   // the accumulator of v_mfma_f32_32x32x2_f32

// ---- the counter-based hash -------------------------------------------------------------------------------------------------
// `mix` of include/playaid_hip.h: the encoder trainer's dropout masks (encoder_train.hip) and the augmentation's noise and pixel
// dropout (augment.hip) are r = mix(mix(i ^ key) + key) of an element index i -- a function of (key, i) alone.
__host__ __device__ __forceinline__ uint32_t hash_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ uint32_t hash_element(uint32_t key, uint32_t i) { return hash_mix(hash_mix(i ^ key) + key); }

// ---- the loss ---------------------------------------------------------------------------------------------------------------
// A label outside [0, A) counts as ignored (-100 is the only such value a checked caller passes).

// Adds the number of labelled rows among labels[0 .. n) to *lds_counter (an integer count in LDS: exact in any order). The
// caller zeroes the counter before and synchronises after. (lt_decode_kernel; ht_sample_kernel, whose B <= blockDim, keeps
// the one-label-per-thread form that the compiler folds into one atomic per wave.)
__device__ __forceinline__ void count_labelled(const int32_t* __restrict__ labels, int n, int A, int tid, int nthreads, int* lds_counter) {
    int cnt = 0;
    for (int i = tid; i < n; i += nthreads) {
        const int l = labels[i];
        cnt += l >= 0 && l < A;
    }
    if (cnt) atomicAdd(lds_counter, cnt);
}

struct RowLoss {
    float d;      // this lane's d loss / d z: (softmax - onehot) / n, 0 for an ignored row and for lane >= A
    float loss;   // -logp[label], 0 for an ignored row (lane 0 stores it)
    int hit;      // 1 where the arg-max (the lowest index on ties) is the label (lane 0 stores it)
};

// log_softmax and NLL of one row, by the 64 lanes of wave 0: lane = class, z = -INFINITY for lane >= A, n = the divisor of the
// mean (max(labelled rows, 1): with no labelled row every gradient is 0).
__device__ __forceinline__ RowLoss softmax_nll_wave0(float z, int lane, int A, int label, bool valid, float n) {
    float mx = z;
    int arg = lane;
    for (int d = 32; d >= 1; d >>= 1) {   // maximum and its first index
        const float om = __shfl_xor(mx, d);
        const int oa = __shfl_xor(arg, d);
        if (om > mx || (om == mx && oa < arg)) {
            mx = om;
            arg = oa;
        }
    }
    float se = lane < A ? expf(z - mx) : 0.f;
    for (int d = 32; d >= 1; d >>= 1) se += __shfl_xor(se, d);
    const float logp = z - mx - logf(se);
    const float lp_label = __shfl(logp, valid ? label : 0);
    RowLoss r;
    r.d = 0.f;
    if (valid && lane < A) r.d = (expf(logp) - (lane == label ? 1.f : 0.f)) / n;
    r.loss = valid ? -lp_label : 0.f;
    r.hit = valid && arg == label ? 1 : 0;
    return r;
}

// One thread folds the step's pa_train_stats from the n rows' loss terms and hit flags (ascending rows) and writes the four
// words to stats and, when non-null, to stats_out.
__device__ __forceinline__ void write_train_stats(float* stats, float* stats_out, const int32_t* labels, const int32_t* hit,
                                                  const float* loss_terms, int n, int A) {
    int nv = 0, hits = 0;
    float s = 0.f;
    for (int r = 0; r < n; ++r) {
        const int l = labels[r];
        nv += l >= 0 && l < A;
        hits += hit[r];
        s += loss_terms[r];
    }
    const float loss = s / (float)max(nv, 1);
    stats[0] = loss;
    stats[1] = __int_as_float(nv);
    stats[2] = __int_as_float(hits);
    stats[3] = 0.f;
    if (stats_out) {
        stats_out[0] = loss;
        stats_out[1] = __int_as_float(nv);
        stats_out[2] = __int_as_float(hits);
        stats_out[3] = 0.f;
    }
}

// ---- Adam -------------------------------------------------------------------------------------------------------------------
// One Adam update (torch.optim.Adam, no weight decay, no amsgrad). The two moments are formed in double and rounded
// once -- m' = m + (g - m)(1 - beta1) cancels when g and m disagree in sign, and three fp32 roundings there are many
// ulp of a small m' --; the weight update is fp32: w -= step_size * (m / (sqrt(v) / bc2_sqrt + eps)), step_size =
// lr / (1 - beta1^k) and bc2_sqrt = sqrt(1 - beta2^k) computed in double on the host and rounded to fp32 once.
__device__ __forceinline__ void adam_apply(float& w, float& m, float& v, float g, const AdamScalars& k) {
    const double gd = (double)g;
    m = (float)((double)m + (gd - (double)m) * k.one_minus_b1);
    v = (float)(k.b2 * (double)v + k.one_minus_b2 * gd * gd);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    w = w - k.step_size * (m / denom);
}

// Element i of w, m and v, read, updated with gradient g and written back.
__device__ __forceinline__ void adam_apply_at(float* w, float* m, float* v, size_t i, float g, const AdamScalars& ak) {
    float wi = w[i], mi = m[i], vi = v[i];
    adam_apply(wi, mi, vi, g, ak);
    w[i] = wi;
    m[i] = mi;
    v[i] = vi;
}

// The four elements idx .. idx + 3 (idx a multiple of 4, the tensors 16-byte aligned) with 16-byte accesses.
__device__ __forceinline__ void adam_apply4_at(float* w, float* m, float* v, size_t idx, const float (&gr)[4], const AdamScalars& ak) {
    float4 w4 = *reinterpret_cast<float4*>(w + idx);
    float4 m4 = *reinterpret_cast<float4*>(m + idx);
    float4 v4 = *reinterpret_cast<float4*>(v + idx);
    adam_apply(w4.x, m4.x, v4.x, gr[0], ak);
    adam_apply(w4.y, m4.y, v4.y, gr[1], ak);
    adam_apply(w4.z, m4.z, v4.z, gr[2], ak);
    adam_apply(w4.w, m4.w, v4.w, gr[3], ak);
    *reinterpret_cast<float4*>(w + idx) = w4;
    *reinterpret_cast<float4*>(m + idx) = m4;
    *reinterpret_cast<float4*>(v + idx) = v4;
}

// The scalars of optimiser step k = 1, 2, ... (all zero for a gradient-only call).
inline AdamScalars adam_scalars(float lr, float beta1, float beta2, float eps, long long k, bool apply) {
    AdamScalars ak;
    memset(&ak, 0, sizeof(ak));
    if (apply) {
        const double kd = (double)k, b1 = (double)beta1, b2 = (double)beta2;
        ak.one_minus_b1 = 1.0 - b1;
        ak.b2 = b2;
        ak.one_minus_b2 = 1.0 - b2;
        ak.step_size = (float)((double)lr / (1.0 - std::pow(b1, kd)));
        ak.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, kd));
        ak.eps = eps;
    }
    return ak;
}

// What every trainer refuses in a pa_adam_config-shaped set of hyper-parameters.
inline bool adam_config_ok(float lr, float beta1, float beta2, float eps) {
    return std::isfinite(lr) && lr > 0.f && std::isfinite(eps) && eps > 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f;
}

// ---- the host side of a trainer handle ----------------------------------------------------------------------------------------
// pa_head_trainer and pa_lstm_trainer derive from this. A handle is handed back even when the device stops its creation, for
// the error text (and destroyed by the caller). `who` is the exported function's name, the prefix of every error text.
struct TrainerCore {
    pa_adam_config cfg;
    int64_t steps = 0;
    std::string last_error;
    float* state = nullptr;   // one device allocation: the two moments and the step's scratch
};

inline int trainer_fail(TrainerCore* t, int code, const std::string& msg) {
    t->last_error = msg;
    return code;
}

// t->state = `floats` zeroed floats on the current device.
inline int trainer_alloc_zeroed(TrainerCore* t, size_t floats, const char* who) {
    void* p = nullptr;
    if (hipMalloc(&p, floats * sizeof(float)) != hipSuccess) return trainer_fail(t, PA_ERR_HIP, std::string(who) + ": hipMalloc failed");
    t->state = static_cast<float*>(p);
    if (hipMemset(p, 0, floats * sizeof(float)) != hipSuccess) return trainer_fail(t, PA_ERR_HIP, std::string(who) + ": hipMemset failed");
    return PA_OK;
}

inline int trainer_check_apply(TrainerCore* t, int32_t apply, const float* grads_out, const char* who) {
    if ((apply != 0 && apply != 1) || (!apply && !grads_out))
        return trainer_fail(t, PA_ERR_INVALID_ARG, std::string(who) + ": apply is 0 (with grads_out) or 1");
    return PA_OK;
}

// set: PA_TRAIN_WEIGHTS, PA_TRAIN_M or PA_TRAIN_V (a caller that serves PA_TRAIN_RAW has taken that bit out).
inline int trainer_check_which(TrainerCore* t, int32_t set, const float* out_dev, const char* who) {
    if (!out_dev || set < 0 || set > PA_TRAIN_V) return trainer_fail(t, PA_ERR_INVALID_ARG, std::string(who) + ": null output or unknown tensor set");
    return PA_OK;
}

template <class T>
void trainer_destroy(T* t) {
    if (!t) return;
    (void)hipFree(t->state);
    delete t;
}

inline const char* trainer_last_error(const TrainerCore* t) { return t ? t->last_error.c_str() : "null trainer"; }

inline int64_t trainer_steps(const TrainerCore* t) { return t ? t->steps : -1; }

}  // namespace pa

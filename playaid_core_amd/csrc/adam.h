// The Adam update shared by the trainers (head_train.hip, lstm_train.hip) and the host-side scalars that go with it.
#pragma once
#include "pa_kernels.h"
#include <cmath>
#include <cstring>

namespace pa {

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

}  // namespace pa

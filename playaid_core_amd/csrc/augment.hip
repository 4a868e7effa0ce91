// The reference's training augmentation of 128 x 128 crops, augment_char_crop (dataset_utils.py:141-252), on crops that are
// already on the device: pa_augment_crops of include/playaid_hip.h, which states the arithmetic of every stage; DESIGN.md 5.14.
// augment.augment_reference is the numpy twin and the contract: this file and the twin give the same bytes.
//
// One launch, one workgroup of 512 threads per OUTPUT crop, no intermediate image in memory:
//   1. the constant tables (AugmentTables, 7 KB) and the crop's parameter block go to LDS; 256 threads build the crop's four
//      256-byte tables (brightness / contrast, hue, saturation, value);
//   2. the source crop is read once with 16-byte loads and staged in LDS (48 KB) with the flip and the brightness / contrast
//      table applied, so the blur's neighbours and the gather through xmap / ymap never go back to memory;
//   3. every thread takes four consecutive output pixels of a row: the chain at (u, v) = (xmap[x], ymap[y]) for each, then
//      three 16-byte stores (one per plane, model layout) or three 4-byte stores (12 packed bytes, uint8 layout) -- consecutive
//      lanes write consecutive addresses.
// Every stage after the geometric ones is a function of the source position alone, which is what makes step 3 possible; the
// random streams are keyed by (key, stream, element index) and never by the launch geometry.
//
// Memory safety for ANY parameter bytes: src is clamped, map entries are masked with & 127, hole tests are comparisons (no
// address is formed from a hole), every table index is a byte. Compiled with -ffp-contract=off (_build.py): the fp32 stages
// must not have their multiplies and adds fused.
#include "augment_math.h"   // the stages' arithmetic, shared with sprite_augment.hip; include/playaid_hip.h

#include <cmath>

namespace pa {
namespace {

constexpr int AUG_THREADS = 512;
constexpr int AUG_ROW = 128 * 3;
constexpr int AUG_IMG = 128 * AUG_ROW;

struct alignas(16) AugLds {
    AugmentTables tabs;
    pa_augment_params prm;
    uint8_t lut_bc[256], lut_h[256], lut_s[256], lut_v[256];
    alignas(16) uint8_t img[AUG_IMG];   // the source crop after flip and brightness / contrast
};
static_assert(sizeof(AugLds) <= 64 * 1024, "one workgroup's LDS");
static_assert(sizeof(pa_augment_params) == 328 && sizeof(pa_augment_params) % 4 == 0 && sizeof(AugmentTables) % 16 == 0, "copied in words");

__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const uint8_t* __restrict__ src, int n_src,
                                                              const pa_augment_params* __restrict__ params, int out_format,
                                                              void* __restrict__ out, const AugmentTables* __restrict__ tabs) {
    __shared__ AugLds L;
    const int tid = threadIdx.x;
    const int crop = blockIdx.x;
    {
        const uint32_t* g = reinterpret_cast<const uint32_t*>(tabs);
        uint32_t* d = reinterpret_cast<uint32_t*>(&L.tabs);
        for (int i = tid; i < (int)(sizeof(AugmentTables) / 4); i += AUG_THREADS) d[i] = g[i];
        const uint32_t* gp = reinterpret_cast<const uint32_t*>(params + crop);
        uint32_t* dp = reinterpret_cast<uint32_t*>(&L.prm);
        if (tid < (int)(sizeof(pa_augment_params) / 4)) dp[tid] = gp[tid];
    }
    __syncthreads();

    const float alpha = aug_sane(L.prm.alpha, 1.f, 0.f, 4.f);
    const float beta = aug_sane(L.prm.beta, 0.f, -2.f, 2.f);
    const float hue = aug_sane(L.prm.hue_shift, 0.f, -1024.f, 1024.f);
    const float sat = aug_sane(L.prm.sat_shift, 0.f, -512.f, 512.f);
    const float val = aug_sane(L.prm.val_shift, 0.f, -512.f, 512.f);
    const float sigma = aug_sane(L.prm.noise_sigma, 0.f, 0.f, 256.f);
    const bool flip = L.prm.flip != 0;
    const int blur = (L.prm.blur_k == 2 || L.prm.blur_k == 3) ? L.prm.blur_k : 0;
    const bool hsv_on = hue != 0.f || sat != 0.f || val != 0.f;
    const uint32_t thr = L.prm.pixel_drop_thr;
    const int n_holes = min(max(L.prm.n_holes, 0), 8);
    const int cmask = L.prm.channel_mask & 7;
    uint32_t k_noise, k_drop;
    aug_stream_keys(L.prm.key, &k_noise, &k_drop);

    if (tid < 256) aug_lut_entry(tid, alpha, beta, hue, sat, val, L.lut_bc, L.lut_h, L.lut_s, L.lut_v);
    __syncthreads();

    {
        const int s = min(max(L.prm.src, 0), n_src - 1);
        const uint4* g = reinterpret_cast<const uint4*>(src + (size_t)s * AUG_IMG);
        for (int i = tid; i < AUG_IMG / 16; i += AUG_THREADS) {
            const uint4 w = g[i];
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            if (!flip) {
                uint32_t o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o[k] = (uint32_t)L.lut_bc[words[k] & 255] | ((uint32_t)L.lut_bc[(words[k] >> 8) & 255] << 8) |
                           ((uint32_t)L.lut_bc[(words[k] >> 16) & 255] << 16) | ((uint32_t)L.lut_bc[words[k] >> 24] << 24);
                reinterpret_cast<uint4*>(L.img)[i] = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    const int idx = i * 16 + b;
                    const int v = idx / AUG_ROW, rem = idx - v * AUG_ROW;
                    const int u = rem / 3, c = rem - u * 3;
                    L.img[v * AUG_ROW + (127 - u) * 3 + c] = L.lut_bc[(words[b >> 2] >> (8 * (b & 3))) & 255];
                }
            }
        }
    }
    __syncthreads();

    for (int quad = tid; quad < 128 * 32; quad += AUG_THREADS) {
        const int y = quad >> 5, x0 = (quad & 31) * 4;
        const int v = L.prm.ymap[y] & 127;
        uint8_t px[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = L.prm.xmap[x0 + j] & 127;
            int c[3];
            if (blur == 0) {
                const uint8_t* p = &L.img[v * AUG_ROW + u * 3];
                c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
            } else {
                int s0 = 0, s1 = 0, s2 = 0;
                for (int dy = 0; dy < blur; ++dy) {
                    const int vy = aug_reflect(v - 1 + dy, 128);
                    for (int dx = 0; dx < blur; ++dx) {
                        const uint8_t* p = &L.img[vy * AUG_ROW + aug_reflect(u - 1 + dx, 128) * 3];
                        s0 += p[0]; s1 += p[1]; s2 += p[2];
                    }
                }
                c[0] = aug_blur_round(s0, blur); c[1] = aug_blur_round(s1, blur); c[2] = aug_blur_round(s2, blur);
            }
            if (hsv_on) aug_hsv_pixel(c, L.tabs, L.lut_h, L.lut_s, L.lut_v);
            const uint32_t pos = (uint32_t)(v * 128 + u);
            if (sigma > 0.f) {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = aug_noise_byte(c[k], sigma, k_noise, pos * 3u + (uint32_t)k, L.tabs.q);
            }
            bool zero = thr != 0u && hash_element(k_drop, pos) < thr;
            for (int hole = 0; hole < n_holes; ++hole)
                zero = zero || ((unsigned)(u - (int)L.prm.holes[2 * hole]) < 4u && (unsigned)(v - (int)L.prm.holes[2 * hole + 1]) < 4u);
#pragma unroll
            for (int k = 0; k < 3; ++k) px[j][k] = (zero || ((cmask >> k) & 1)) ? (uint8_t)0 : (uint8_t)c[k];
        }
        if (out_format == PA_AUGMENT_MODEL) {
            float* o = reinterpret_cast<float*>(out) + (size_t)crop * 3 * 128 * 128 + y * 128 + x0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                *reinterpret_cast<float4*>(o + k * 128 * 128) =
                    make_float4(L.tabs.unit[px[0][k]], L.tabs.unit[px[1][k]], L.tabs.unit[px[2][k]], L.tabs.unit[px[3][k]]);
        } else {
            uint32_t* o = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(out) + (size_t)crop * AUG_IMG + (y * 128 + x0) * 3);
            const uint8_t* b = &px[0][0];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
        }
    }
}

// the standard normal's lower tail probability and, by bisection on it, its quantile for 0 < p < 1 / 2 (fp64)
double aug_norm_cdf(double x) { return 0.5 * std::erfc(-x * 0.70710678118654752440); }
double aug_norm_ppf_lower(double p) {
    double lo = -40.0, hi = 0.0;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (aug_norm_cdf(mid) < p) lo = mid; else hi = mid;
    }
    return 0.5 * (lo + hi);
}

}  // namespace

void augment_tables_host(AugmentTables* t) {
    memset(t, 0, sizeof(*t));
    for (int j = 1; j < 512; ++j) {
        const double x = aug_norm_ppf_lower((double)j / 1024.0);
        t->q[j] = (float)x;
        t->q[1024 - j] = (float)-x;
    }
    t->q[512] = 0.f;
    // the outermost cells: z runs linearly from a = q[1023] to c with probability 1 / 1024; c keeps the normal's second moment
    // of that tail, (a^2 + a c + c^2) / 3 = 1024 (a phi(a) + 1 / 1024)
    const double a = -aug_norm_ppf_lower(1.0 / 1024.0);
    const double phi = std::exp(-0.5 * a * a) / std::sqrt(2.0 * 3.14159265358979323846);
    const double target = 3.0 * (1024.0 * a * phi + 1.0);
    const double c = 0.5 * (-a + std::sqrt(a * a - 4.0 * (a * a - target)));
    t->q[1024] = (float)c;
    t->q[0] = (float)-c;
    for (int i = 1; i < 256; ++i) {   // cv::saturate_cast<int>(double): to nearest, ties to even
        t->sdiv[i] = (int32_t)std::nearbyint((double)(255 << 12) / (1.0 * i));
        t->hdiv[i] = (int32_t)std::nearbyint((double)(180 << 12) / (6.0 * i));
    }
    for (int i = 0; i < 256; ++i) t->unit[i] = (float)i / 255.0f;
}

hipError_t launch_augment(const uint8_t* src, int n_src, const void* params, int n, int out_format, void* out,
                          const AugmentTables* tabs_dev, hipStream_t s) {
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)n), dim3(AUG_THREADS), 0, s, src, n_src,
                       reinterpret_cast<const pa_augment_params*>(params), out_format, out, tabs_dev);
    return hipGetLastError();
}

}  // namespace pa

extern "C" {

int pa_augment_quantiles(float* out_host) {
    if (!out_host) return PA_ERR_INVALID_ARG;
    pa::AugmentTables t;
    pa::augment_tables_host(&t);
    memcpy(out_host, t.q, PA_AUGMENT_QUANTILES * sizeof(float));
    return PA_OK;
}

int pa_augment_params_check(const pa_augment_params* host, int32_t n, int32_t n_src) {
    if (!host || n < 1 || n_src < 1) return PA_ERR_INVALID_ARG;
    auto in = [](float x, float lo, float hi) { return x >= lo && x <= hi; };   // false for NaN
    for (int32_t i = 0; i < n; ++i) {
        const pa_augment_params& p = host[i];
        if (p.src < 0 || p.src >= n_src || (p.flip != 0 && p.flip != 1)) return PA_ERR_INVALID_ARG;
        if (!in(p.alpha, 0.8f, 1.2f) || !in(p.beta, -0.2f, 0.4f)) return PA_ERR_INVALID_ARG;
        if (p.blur_k != 0 && p.blur_k != 2 && p.blur_k != 3) return PA_ERR_INVALID_ARG;
        if (!in(p.hue_shift, -256.f, 256.f) || !in(p.sat_shift, -67.f, 67.f) || !in(p.val_shift, -5.f, 5.f)) return PA_ERR_INVALID_ARG;
        if (!in(p.noise_sigma, 0.f, 14.142136f)) return PA_ERR_INVALID_ARG;   // sqrt(var_limit = 200) as a float
        if (p.n_holes < 0 || p.n_holes > 8 || p.channel_mask < 0 || p.channel_mask > 6) return PA_ERR_INVALID_ARG;
        for (int h = 0; h < 2 * p.n_holes; ++h)
            if (p.holes[h] > 124) return PA_ERR_INVALID_ARG;
        for (int k = 0; k < 128; ++k)
            if (p.xmap[k] > 127 || p.ymap[k] > 127) return PA_ERR_INVALID_ARG;
    }
    return PA_OK;
}

}  // extern "C"

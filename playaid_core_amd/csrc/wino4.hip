// Winograd F(4x4, 3x3) TAKEN APART, for stride-1 3x3 layers on 4 x 4 maps (ResNet-18's layer 4). A 4 x 4 map is
// exactly one F(4x4, 3x3) tile and the zero-bordered 6 x 6 pixels the engine stores per crop are that tile's input patch, so the
// layer is
//   V[p][crop][cin]  = (B^T d B)[p]                    p = 6 i + j, one of 36 positions            wino4_input_kernel
//   M[p][crop][cout] = sum_cin V[p][crop][cin] U[p][cout][cin]   36 independent GEMMs, ONE launch   pigemm.hip, launch_pgemm_grouped
//   Y[crop]          = A^T M A, + bias (+ residual), ReLU                                           wino4_output_kernel
// with U = G g G^T (wino4_transform_weights, fp64, rounded once). 36 products per image and channel pair where F(2x2) spends 64
// and the direct form 144. The fused F(2x2) kernel (wino.hip) keeps its transforms beside the fp32 matrix instructions, where every
// vector instruction costs matrix time; here the products run as a plain GEMM fed from LDS and the two transforms are memory-bound
// element-wise kernels around it. No K split: a crop's bits do not depend on the batch it is in.
// Lavin & Gray's matrices (interpolation points 0, +-1, +-2, infinity):
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
#include "tile_common.h"

#include <cstdlib>

namespace pa {

namespace {

__device__ __forceinline__ f32x4 w4_fma(float a, f32x4 x, f32x4 y) {   // a * x + y, one rounding per component
    return f32x4{__builtin_fmaf(a, x.x, y.x), __builtin_fmaf(a, x.y, y.y), __builtin_fmaf(a, x.z, y.z), __builtin_fmaf(a, x.w, y.w)};
}

// t = B^T d for one line of six, in THIS order (every product by 2 or 4 is exact; fma = one rounding):
//   t0 = fma(4, d0, fma(-5, d2, d4))                 t5 = fma(4, d1, fma(-5, d3, d5))
//   a = fma(-4, d2, d4), b = fma(-4, d1, d3):        t1 = a + b, t2 = a - b
//   c = d4 - d2, e = d3 - d1:                        t3 = fma(2, e, c), t4 = fma(-2, e, c)
__device__ __forceinline__ void w4_bt(f32x4 (&d)[6]) {
    const f32x4 t0 = w4_fma(4.f, d[0], w4_fma(-5.f, d[2], d[4]));
    const f32x4 t5 = w4_fma(4.f, d[1], w4_fma(-5.f, d[3], d[5]));
    const f32x4 a = w4_fma(-4.f, d[2], d[4]), b = w4_fma(-4.f, d[1], d[3]);
    const f32x4 c = d[4] - d[2], e = d[3] - d[1];
    d[0] = t0; d[1] = a + b; d[2] = a - b; d[3] = w4_fma(2.f, e, c); d[4] = w4_fma(-2.f, e, c); d[5] = t5;
}

// y = A^T m for one line of six -> four, in THIS order:
//   s = m1 + m2, d = m1 - m2, u = m3 + m4, v = m3 - m4
//   y0 = (m0 + s) + u, y1 = fma(2, v, d), y2 = fma(4, u, s), y3 = fma(8, v, d) + m5
__device__ __forceinline__ void w4_at(const f32x4 (&m)[6], f32x4 (&y)[4]) {
    const f32x4 s = m[1] + m[2], d = m[1] - m[2], u = m[3] + m[4], v = m[3] - m[4];
    y[0] = (m[0] + s) + u;
    y[1] = w4_fma(2.f, v, d);
    y[2] = w4_fma(4.f, u, s);
    y[3] = w4_fma(8.f, v, d) + m[5];
}

// One thread per (row, four input channels), rows = the crops padded to the GEMM's row tile: the 36 pixels of the crop's padded
// 6 x 6 patch (the ring is the layer's zero padding) -> B^T d along the columns (i), then along the rows (j) -> V[6 i + j][row][c].
// Rows past the last crop are written as zeros. Consecutive lanes take consecutive channel quads: every load and store of a wave is
// one contiguous KiB.
__global__ __launch_bounds__(64) void wino4_input_kernel(const Wino4Params p) {
    const int cq_n = p.cin >> 2;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    const int row = idx / cq_n, c = (idx - row * cq_n) * 4;
    if (row >= p.rows) return;
    float* v = p.v + (size_t)row * p.cin + c;
    const size_t plane = (size_t)p.rows * p.cin;
    if (row >= p.n_img) {
#pragma unroll
        for (int q = 0; q < 36; ++q) *reinterpret_cast<f32x4*>(v + q * plane) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const float* x = p.act + (size_t)row * p.in_img_stride + c;
    f32x4 d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) d[i][j] = *reinterpret_cast<const f32x4*>(x + i * p.in_row_stride + j * p.in_px_stride);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        f32x4 l[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) l[i] = d[i][j];
        w4_bt(l);
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i][j] = l[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        w4_bt(d[i]);
#pragma unroll
        for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x4*>(v + (i * 6 + j) * plane) = d[i][j];
    }
}

// One thread per (crop, four output channels): M[6 i + j][crop][c] -> A^T m along the columns (i), then along the rows (j) -> the
// 4 x 4 outputs, epilogue4 (bias, residual before or after the activation, ReLU / SiLU) as the fused kernel, into the interior of
// the padded output.
__global__ __launch_bounds__(64) void wino4_output_kernel(const Wino4Params p) {
    const int cq_n = p.cout >> 2;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    const int row = idx / cq_n, c = (idx - row * cq_n) * 4;
    if (row >= p.n_img) return;
    const float* m = p.m + (size_t)row * p.cout + c;
    const size_t plane = (size_t)p.rows * p.cout;
    f32x4 t[4][6];   // A^T m along i, per column j
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        f32x4 l[6], y[4];
#pragma unroll
        for (int i = 0; i < 6; ++i) l[i] = *reinterpret_cast<const f32x4*>(m + (i * 6 + j) * plane);
        w4_at(l, y);
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i][j] = y[i];
    }
    const f32x4 bias4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    const size_t o00 = (size_t)row * p.out_img_stride + (size_t)p.out_pad * (p.out_row_stride + p.out_px_stride) + c;
    f32x4 res4[4][4];   // every residual value first (it may alias the output)
#pragma unroll
    for (int oy = 0; oy < 4; ++oy)
#pragma unroll
        for (int ox = 0; ox < 4; ++ox)
            res4[oy][ox] = p.residual ? *reinterpret_cast<const f32x4*>(p.residual + o00 + (size_t)oy * p.out_row_stride + ox * p.out_px_stride)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int oy = 0; oy < 4; ++oy) {
        f32x4 y[4];
        w4_at(t[oy], y);
#pragma unroll
        for (int ox = 0; ox < 4; ++ox)
            *reinterpret_cast<f32x4*>(p.out + o00 + (size_t)oy * p.out_row_stride + ox * p.out_px_stride) = epilogue4(y[ox], bias4, res4[oy][ox], p.relu, p.res_after);
    }
}

}  // namespace

size_t wino4_weight_floats(int cin, int cout) { return (size_t)36 * cin * cout; }

int wino4_rows(int n_img) { return (n_img + 63) / 64 * 64; }

// [cout][ky][kx][cin] (BatchNorm folded) -> U[36][cout][cin] = G g G^T in fp64, rounded once: U[p] is the [N][K] weight image of
// the GEMM of position p
void wino4_transform_weights(const float* w, int cin, int cout, float* u) {
    static const double Gm[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                    {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};
    const size_t plane = (size_t)cout * cin;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            double g[3][3], tmp[6][3];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) g[ky][kx] = (double)w[((size_t)co * 9 + ky * 3 + kx) * cin + ci];
            for (int i = 0; i < 6; ++i)
                for (int kx = 0; kx < 3; ++kx) tmp[i][kx] = Gm[i][0] * g[0][kx] + Gm[i][1] * g[1][kx] + Gm[i][2] * g[2][kx];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j)
                    u[(size_t)(i * 6 + j) * plane + (size_t)co * cin + ci] = (float)(tmp[i][0] * Gm[j][0] + tmp[i][1] * Gm[j][1] + tmp[i][2] * Gm[j][2]);
        }
}

// The three launches of one layer, ordered by the stream. p.tile: the GEMM's tile (launch_pgemm_grouped), 0 = the default.
hipError_t launch_wino4_conv3x3(const Wino4Params& p_in, hipStream_t s) {
    Wino4Params p = p_in;
    if (!p.act || !p.wgt || !p.out || !p.v || !p.m || p.n_img < 1 || p.cin < 64 || p.cin % 64 || p.cout < 64 || p.cout % 64 || p.in_px_stride < p.cin ||
        p.out_px_stride < p.cout || p.out_pad < 0)
        return hipErrorInvalidValue;
    auto mis = [](const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) != 0; };
    if (p.in_px_stride % 4 || p.out_px_stride % 4 || p.in_row_stride % 4 || p.in_img_stride % 4 || p.out_row_stride % 4 || p.out_img_stride % 4 || mis(p.act) ||
        mis(p.wgt) || mis(p.out) || mis(p.v) || mis(p.m) || (p.bias && mis(p.bias)) || (p.residual && mis(p.residual)))
        return hipErrorInvalidValue;
    p.rows = wino4_rows(p.n_img);
    const long long in_threads = (long long)p.rows * (p.cin / 4), out_threads = (long long)p.n_img * (p.cout / 4);
    if (in_threads >= (1ll << 31) || out_threads >= (1ll << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wino4_input_kernel, dim3((unsigned)((in_threads + 63) / 64)), dim3(64), 0, s, p);
    static const int tile_env = getenv("PA_WINO_F4_TILE") ? atoi(getenv("PA_WINO_F4_TILE")) : 0;   // A/B: 1 = 64 x 64, 2 = 128 x 64, 3 = 128 x 32
    const hipError_t e = launch_pgemm_grouped(p.v, p.wgt, p.m, 36, p.rows, p.cin, p.cout, p.tile ? p.tile : tile_env, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wino4_output_kernel, dim3((unsigned)((out_threads + 63) / 64)), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace pa

// ---- C ABI: the form as a single-layer operator (include/playaid_hip.h) ---------------------------------------------------
#include "../../include/playaid_hip.h"

extern "C" {

size_t pa_wino4_weight_floats(int32_t cin, int32_t cout) {
    if (cin < 64 || cin % 64 || cout < 64 || cout % 64) return 0;
    return pa::wino4_weight_floats(cin, cout);
}

int pa_wino4_transform_weights(const float* w_host, int32_t cin, int32_t cout, float* u_host) {
    if (!w_host || !u_host || cin < 64 || cin % 64 || cout < 64 || cout % 64) return PA_ERR_INVALID_ARG;
    pa::wino4_transform_weights(w_host, cin, cout, u_host);
    return PA_OK;
}

int pa_wino4_conv3x3(const float* x, const float* u, const float* bias, const float* residual, float* out, int32_t n, int32_t height, int32_t width,
                     int32_t cin, int32_t cout, int32_t in_px_stride, int32_t out_px_stride, int32_t out_pad, int32_t act, int32_t res_after,
                     float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !u || !out || !scratch || n < 1 || height != 4 || width != 4 || out_pad < 0 || act < 0 || act > 2 || cin < 64 || cin % 64 || cout < 64 ||
        cout % 64 || (reinterpret_cast<unsigned long long>(scratch) & 15ull))
        return PA_ERR_INVALID_ARG;
    const size_t rows = (size_t)pa::wino4_rows(n);
    if (scratch_floats < 36 * rows * ((size_t)cin + cout)) return PA_ERR_INVALID_ARG;
    pa::Wino4Params p{};
    p.act = x; p.wgt = u; p.bias = bias; p.residual = residual; p.out = out;
    p.v = scratch;
    p.m = scratch + 36 * rows * cin;
    p.n_img = n; p.cin = cin; p.cout = cout;
    p.in_px_stride = in_px_stride;
    p.in_row_stride = 6 * in_px_stride;
    p.in_img_stride = 6 * p.in_row_stride;
    p.out_px_stride = out_px_stride;
    p.out_row_stride = (4 + 2 * out_pad) * out_px_stride;
    p.out_img_stride = (4 + 2 * out_pad) * p.out_row_stride;
    p.out_pad = out_pad;
    p.relu = act;
    p.res_after = res_after;
    const hipError_t e = pa::launch_wino4_conv3x3(p, (hipStream_t)stream);
    return e == hipSuccess ? PA_OK : (e == hipErrorInvalidValue ? PA_ERR_INVALID_ARG : PA_ERR_HIP);
}

}  // extern "C"

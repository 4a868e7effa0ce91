// conv_rows.h: a table's convolution row -> launch parameters, and the per-form weight planes; behind them the single-layer
// convolution operator of the C ABI (pa_conv2d) on the persistent GEMM kernels. Host code only.
#include "conv_rows.h"
#include "../../include/playaid_hip.h"

namespace pa {

GemmParams conv_row_params(const ConvRow& r) {
    const int oh = r.in_h / r.stride, ow = r.in_w / r.stride;
    const int in_hb = r.in_h + 2 * r.in_pad, in_wb = r.in_w + 2 * r.in_pad;
    const int out_hb = oh + 2 * r.out_pad, out_wb = ow + 2 * r.out_pad;
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = r.images * oh * ow;
    p.N = r.cout;
    p.taps = r.ksize * r.ksize;
    p.kw_taps = r.ksize;
    p.chunk = r.cin;
    p.ktot = p.taps * p.chunk;
    p.howo = oh * ow;
    p.wo = ow;
    p.in_px_stride = r.in_px_stride;
    p.in_row_stride = in_wb * r.in_px_stride;
    p.in_img_stride = in_hb * in_wb * r.in_px_stride;
    p.stride = r.stride;
    p.off_y = p.off_x = r.in_pad - (r.ksize - 1) / 2;
    p.out_px_stride = r.out_px_stride;
    p.out_row_stride = out_wb * r.out_px_stride;
    p.out_img_stride = out_hb * out_wb * r.out_px_stride;
    p.out_pad = r.out_pad;
    p.relu = r.act;
    p.res_after = r.res_after;
    p.splitk = 1;
    return p;
}

WinoParams wino_params(const GemmParams& p, int n_img, int height, int width, int cin, const float* filters, int bn) {
    WinoParams q;
    memset(&q, 0, sizeof(q));
    q.act = p.act; q.wgt = filters; q.bias = p.bias; q.residual = p.residual; q.out = p.out;
    q.n_img = n_img; q.height = height; q.width = width; q.cin = cin; q.cout = p.N; q.bn = bn;
    q.in_px_stride = p.in_px_stride; q.in_row_stride = p.in_row_stride; q.in_img_stride = p.in_img_stride;
    q.out_px_stride = p.out_px_stride; q.out_row_stride = p.out_row_stride; q.out_img_stride = p.out_img_stride; q.out_pad = p.out_pad;
    q.relu = p.relu; q.res_after = p.res_after;
    return q;
}

FormWeights::~FormWeights() {
    (void)hipFree(wino);
    (void)hipFree(psgemm);
    (void)hipFree(bgemm);
}

namespace {

template <typename T>
hipError_t upload_plane(T** dst, const std::vector<T>& host, const char* alloc_what, const char* copy_what, const char** what) {
    if (host.empty()) return hipSuccess;
    *what = alloc_what;
    const hipError_t e = hipMalloc(dst, host.size() * sizeof(T));
    if (e != hipSuccess) return e;
    *what = copy_what;
    return hipMemcpy(*dst, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace

hipError_t FormWeights::prepare(const std::vector<FormRow>& rows, const float* blob, const char** what) {
    const size_t n = rows.size();
    wino_off.assign(n, -1);
    wino_bn.assign(n, 0);
    psgemm_off.assign(n, -1);
    bgemm_off.assign(n, -1);
    size_t n_wino = 0, n_ps = 0, n_bg = 0;
    for (size_t i = 0; i < n; ++i) {
        const FormRow& r = rows[i];
        const int ktot = r.ksize * r.ksize * r.cin;
        if (r.forms & FORM_WINO) {
            wino_off[i] = (long long)n_wino;
            wino_bn[i] = wino_pick_bn(r.cout, r.wino_tiles);
            n_wino += wino_weight_floats(r.cin, r.cout);
        }
        if (r.forms & FORM_PSGEMM) {
            psgemm_off[i] = (long long)n_ps;
            n_ps += psgemm_weight_elems(r.cout, ktot, r.residual);
        }
        if (r.forms & FORM_BGEMM) {
            bgemm_off[i] = (long long)n_bg;
            n_bg += r.packed ? r.packed_elems : bgemm_weight_elems(r.cout, ktot, r.residual);
            n_bg = (n_bg + 127) & ~(size_t)127;   // (every plane 256-byte aligned)
        }
    }
    std::vector<float> ug(n_wino);
    std::vector<unsigned short> ps(n_ps), bg(n_bg, 0);
    for (size_t i = 0; i < n; ++i) {
        const FormRow& r = rows[i];
        const float* w = blob + r.w_off;
        const int ktot = r.ksize * r.ksize * r.cin;
        if (wino_off[i] >= 0) wino_transform_weights(w, r.cin, r.cout, wino_bn[i], ug.data() + wino_off[i]);
        if (psgemm_off[i] >= 0) psgemm_pack_weights(w, r.cout, ktot, r.residual, ps.data() + psgemm_off[i]);
        if (bgemm_off[i] >= 0 && r.packed) memcpy(bg.data() + bgemm_off[i], r.packed, r.packed_elems * sizeof(unsigned short));
        else if (bgemm_off[i] >= 0) bgemm_pack_weights(w, r.cout, ktot, r.residual, bg.data() + bgemm_off[i]);
    }
    hipError_t e = upload_plane(&wino, ug, "hipMalloc Winograd filters", "upload Winograd filters", what);
    if (e == hipSuccess) e = upload_plane(&psgemm, ps, "hipMalloc split weights", "upload split weights", what);
    if (e == hipSuccess) e = upload_plane(&bgemm, bg, "hipMalloc bf16 weights", "upload bf16 weights", what);
    return e;
}

}  // namespace pa

extern "C" {

size_t pa_conv_weight_bytes(int32_t cin, int32_t cout, int32_t ksize, int32_t compute_dtype, int32_t has_residual) {
    if (cin <= 0 || cout <= 0 || (ksize != 1 && ksize != 3) || cin % 32 != 0 || cout % 32 != 0) return 0;
    if (compute_dtype == PA_DTYPE_F32) return (size_t)cout * ksize * ksize * cin * sizeof(float);
    if (compute_dtype == PA_DTYPE_EMULATED_F32) return pa::psgemm_weight_elems(cout, ksize * ksize * cin, has_residual) * sizeof(unsigned short);
    return 0;
}

int pa_conv_pack_weights(const float* w_host, int32_t cin, int32_t cout, int32_t ksize, int32_t compute_dtype, int32_t has_residual, void* out_host) {
    const size_t bytes = pa_conv_weight_bytes(cin, cout, ksize, compute_dtype, has_residual);
    if (!w_host || !out_host || bytes == 0) return PA_ERR_INVALID_ARG;
    if (compute_dtype == PA_DTYPE_F32) memcpy(out_host, w_host, bytes);
    else pa::psgemm_pack_weights(w_host, cout, ksize * ksize * cin, has_residual, static_cast<unsigned short*>(out_host));
    return PA_OK;
}

int pa_conv2d(const float* x, const void* w, const float* bias, const float* residual, float* out, int32_t n, int32_t height, int32_t width, int32_t cin,
              int32_t cout, int32_t ksize, int32_t stride, int32_t in_pad, int32_t in_px_stride, int32_t out_px_stride, int32_t out_pad, int32_t act,
              int32_t res_after, int32_t compute_dtype, void* stream) {
    if (!x || !w || !out || n <= 0 || height <= 0 || width <= 0 || (ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || height % stride || width % stride ||
        in_pad < (ksize - 1) / 2 || in_px_stride < cin || out_px_stride < cout || out_pad < 0 || act < 0 || act > 2 ||
        pa_conv_weight_bytes(cin, cout, ksize, compute_dtype, residual != nullptr) == 0)
        return PA_ERR_INVALID_ARG;
    // 16-byte units: the loaders' LDS-DMA reads and the epilogue's dwordx4 stores / residual loads move four floats at an address
    auto misaligned = [](const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) != 0; };
    if (in_px_stride % 4 || out_px_stride % 4 || misaligned(x) || misaligned(w) || misaligned(out) || misaligned(residual) ||
        (reinterpret_cast<unsigned long long>(bias) & 3ull))
        return PA_ERR_INVALID_ARG;
    const int oh = height / stride, ow = width / stride;
    const int in_wb = width + 2 * in_pad, in_hb = height + 2 * in_pad, out_wb = ow + 2 * out_pad, out_hb = oh + 2 * out_pad;
    if ((long long)n * in_hb * in_wb * in_px_stride >= (1ll << 29) || (long long)n * out_hb * out_wb * out_px_stride >= (1ll << 29)) return PA_ERR_CAPACITY;
    pa::GemmParams p = pa::conv_row_params({/*images*/ n, /*in h, w, pad, px stride*/ height, width, in_pad, in_px_stride, /*cin, cout, ksize, stride*/ cin, cout, ksize, stride,
                                            /*out pad, px stride*/ out_pad, out_px_stride, /*act, res_after*/ act, res_after});
    p.act = x;
    p.wgt = static_cast<const float*>(w);
    p.bias = bias;
    p.residual = residual;
    p.out = out;
    hipError_t e;
    if (compute_dtype == PA_DTYPE_EMULATED_F32) e = pa::launch_psgemm(p, static_cast<const unsigned short*>(w), (size_t)n * p.out_img_stride, 0, static_cast<hipStream_t>(stream));
    else if (residual) return PA_ERR_INVALID_ARG;   // (the exact persistent kernel has no residual epilogue: Winograd / the patch kernel take those layers)
    else e = pa::launch_pgemm(p, 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? PA_OK : (e == hipErrorInvalidValue ? PA_ERR_INVALID_ARG : PA_ERR_HIP);
}

int pa_conv2d_branch(const float* x, const void* w, const float* bias, const float* residual, float* out, const float* w2, float* out2, int32_t n,
                     int32_t height, int32_t width, int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t in_pad, int32_t in_px_stride,
                     int32_t out_px_stride, int32_t out_pad, int32_t act, int32_t res_after, int32_t compute_dtype, void* stream) {
    // the opener form alone: 3x3, stride 2, the tap the whole pixel, exact fp32, ReLU or nothing, no residual
    if (!x || !w || !out || !w2 || !out2 || residual || res_after || n <= 0 || height <= 0 || width <= 0 || ksize != 3 || stride != 2 || height % 2 || width % 2 ||
        in_pad < 1 || in_px_stride != cin || out_px_stride < cout || out_pad < 0 || act < 0 || act > 1 || compute_dtype != PA_DTYPE_F32 ||
        pa_conv_weight_bytes(cin, cout, 3, compute_dtype, 0) == 0)
        return PA_ERR_INVALID_ARG;
    auto misaligned = [](const void* q) { return (reinterpret_cast<unsigned long long>(q) & 15ull) != 0; };
    if (in_px_stride % 4 || out_px_stride % 4 || misaligned(x) || misaligned(w) || misaligned(out) || misaligned(w2) || misaligned(out2) ||
        (reinterpret_cast<unsigned long long>(bias) & 3ull))
        return PA_ERR_INVALID_ARG;
    const int oh = height / 2, ow = width / 2;
    const int in_wb = width + 2 * in_pad, in_hb = height + 2 * in_pad, out_wb = ow + 2 * out_pad, out_hb = oh + 2 * out_pad;
    if ((long long)n * in_hb * in_wb * in_px_stride >= (1ll << 29) || (long long)n * out_hb * out_wb * out_px_stride >= (1ll << 29)) return PA_ERR_CAPACITY;
    pa::GemmParams p = pa::conv_row_params({/*images*/ n, /*in h, w, pad, px stride*/ height, width, in_pad, in_px_stride, /*cin, cout, ksize, stride*/ cin, cout, 3, 2,
                                            /*out pad, px stride*/ out_pad, out_px_stride, /*act, res_after*/ act, 0});
    p.act = x;
    p.wgt = static_cast<const float*>(w);
    p.bias = bias;
    p.out = out;
    p.wgt2 = w2;
    p.out2 = out2;
    const hipError_t e = pa::launch_pgemm(p, 64, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? PA_OK : (e == hipErrorInvalidValue ? PA_ERR_INVALID_ARG : PA_ERR_HIP);
}

}  // extern "C"

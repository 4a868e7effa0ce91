// A conv-net described by a table, run on the engine's fp32 convolution kernels (the
// ResNet-50 backbone of the reference's ResnetTransformerDetector, playaid/models/resnet_transformer_detector.py:37,
// "reusing the same backbone kernels").
//
// The host hands over BatchNorm-folded weights laid out [cout][ky][kx][cin] (stem: [64][7][8 px][4 ch]) and one
// pa_conv_desc per layer; activations live in a small set of device buffers, zero-bordered NHWC, each used with
// ONE geometry so that borders written as zero at creation stay zero. Layers run in table order on one stream:
//   kind 0  convolution k x k (k = 1 | 3), stride 1 | 2, + bias (+ residual) (+ ReLU): conv3x3_patch_kernel for the
//           stride-1 3x3 layers it covers, the im2col engine (igemm.hip) for everything else (1x1 = a GEMM);
//   kind 1  the 7x7/2 stem + BatchNorm + ReLU + 3x3/2 max-pool of a 128 x 128 x 3 input (stem_pool.hip);
//   kind 2  global average pool of the interior;
//   kind 3  the kind-1 stem + max-pool of an in_hw x in_hw x 3 input, in_hw % 32 == 0, 64 .. 512 (stem_pool_any.hip; fp32 tables only).
// The table's stem row sets the size S of the input forward and trace take (128 without a kind-3 row); every other row runs on
// the launchers above at whatever map size the table gives it, a launcher that refuses a shape handing it to the next form.
// Under PA_DTYPE_BF16 (never the default) the stem and convolution rows store bf16: the stem on stem_pool.hip's bf16 form, every
// convolution on the one-slice bf16 GEMM (bgemm.hip), in its split-K form where the unsplit grid would leave most of the chip idle,
// the pool on a bf16 twin of the fp32 one (fp32 out). Rounding model: include/playaid_hip.h next to pa_convnet_create_dtype.
// Nothing here is specific to ResNet-50; the table in playaid_core_amd/resnet_transformer_detector.py is.
#include "conv_rows.h"
#include "../../include/playaid_hip.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace pa {
namespace {

// [n][(hw + 2 pad)^2][C] -> [n][C], mean over the interior
__global__ __launch_bounds__(256) void avgpool_any_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int hw, int pad, int C) {
    const int w = hw + 2 * pad;
    const size_t total = (size_t)n * C;
    const float inv = 1.f / (float)(hw * hw);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t img = i / C;
        const float* src = in + img * w * w * C + c;
        float sum = 0.f;
        for (int y = 0; y < hw; ++y)
            for (int x = 0; x < hw; ++x) sum += src[(size_t)((y + pad) * w + x + pad) * C];
        out[i] = sum * inv;
    }
}

// the same over a bf16 map (PA_DTYPE_BF16): the stored values summed in fp32 in the same fixed order (row by row), fp32 out
__global__ __launch_bounds__(256) void avgpool_bf16_any_kernel(const unsigned short* __restrict__ in, float* __restrict__ out, int n, int hw, int pad, int C) {
    const int w = hw + 2 * pad;
    const size_t total = (size_t)n * C;
    const float inv = 1.f / (float)(hw * hw);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t img = i / C;
        const unsigned short* src = in + img * w * w * C + c;
        float sum = 0.f;
        for (int y = 0; y < hw; ++y)
            for (int x = 0; x < hw; ++x) sum += __uint_as_float((unsigned)src[(size_t)((y + pad) * w + x + pad) * C] << 16);
        out[i] = sum * inv;
    }
}

}  // namespace
}  // namespace pa

struct pa_convnet {
    int device = 0, max_crops = 0;
    std::vector<pa_conv_desc> descs;
    std::vector<float*> bufs;
    std::vector<size_t> buf_floats;  // per crop (elements)
    float* weights = nullptr;
    size_t n_weights = 0;
    int compute_dtype = PA_DTYPE_F32;
    // per row: the stride-1 3x3 layers' Winograd filters; PA_DTYPE_EMULATED_F32: the psgemm.hip layers' three bf16 slices;
    // PA_DTYPE_BF16: the stem's [64][224] or bgemm_pack_weights' plane, RNE bf16
    pa::FormWeights fw;
    // PA_DTYPE_BF16: every stem and convolution row stores bf16 (the buffers it writes hold 2-byte elements), the pool fp32
    std::vector<char> buf_bf16;                // per buffer: 1 = bf16 elements
    float* bg_slab = nullptr;                  // bgemm split-K partials: BGEMM_SLAB_ITEMS workgroups x 128 x 128 fp32
    int32_t* bg_tickets = nullptr;             // BGEMM_TICKETS of them, zero between launches
    float* x0 = nullptr;  // [max_crops][in_hw + 6][in_hw + 6][4] model input of the stem (bf16 elements under PA_DTYPE_BF16)
    int in_hw = 128;      // side of the input crops: 128, or the in_hw of the table's kind-3 row
    bool sized = false;   // the table has a kind-3 row: the input goes through the sized conversion
    std::vector<int32_t> forms;  // per layer: the pa_cn_form the last forward or trace launched it as (pa_convnet_layer_forms)
    std::string last_error;
};

namespace {

int cn_fail(pa_convnet* h, int code, const std::string& msg) {
    if (h) h->last_error = msg;
    return code;
}

// interior size and channel count a layer leaves in its output buffer
void out_geom(const pa_conv_desc& d, int* hw, int* c) {
    if (d.kind == 1) { *hw = 32; *c = 64; }
    else if (d.kind == 3) { *hw = d.in_hw / 4; *c = 64; }
    else if (d.kind == 2) { *hw = 1; *c = d.cin; }
    else { *hw = d.in_hw / d.stride; *c = d.cout; }
}

// every call that can fail with a HIP error inside a function that returns a PA_* code for handle h
#define CN_HIP(call)                                                                                  \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess) return cn_fail(h, PA_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

bool is_bf16(const pa_convnet* h, int buf) { return h->compute_dtype == PA_DTYPE_BF16 && (buf < 0 || h->buf_bf16[buf]); }

// PA_CONVNET_BG_SPLIT (read once): unset = bgemm_pick_split's rule, 0 or 1 = no split-K, n = S forced to n on every row whose
// unsplit grid is below half the CUs (A/B runs)
int bg_split_knob() {
    static const int v = getenv("PA_CONVNET_BG_SPLIT") ? atoi(getenv("PA_CONVNET_BG_SPLIT")) : -1;
    return v;
}

// PA_CONVNET_WINO=0 (read once, at the first convolution row of the first create that is not bf16) keeps the stride-1 3x3 rows in their direct form (A/B)
int wino_knob() {
    static const int v = getenv("PA_CONVNET_WINO") ? atoi(getenv("PA_CONVNET_WINO")) : 1;
    return v;
}

// a convolution row at n crops: square maps, whole pixels (create validates its GemmParams before anything is allocated;
// convnet_run fills in the pointers)
pa::ConvRow conv_row(const pa_conv_desc& d, int n) {
    return {/*images*/ n, /*in h, w, pad, px stride*/ d.in_hw, d.in_hw, d.in_pad, d.cin, /*cin, cout, ksize, stride*/ d.cin, d.cout, d.ksize, d.stride,
            /*out pad, px stride*/ d.out_pad, d.cout, /*act, res_after*/ d.relu, 0};
}

}  // namespace

extern "C" {

const char* pa_convnet_last_error(const pa_convnet* h) { return h ? h->last_error.c_str() : "null handle"; }

int pa_convnet_create(int32_t device, const pa_conv_desc* descs, int32_t n_descs, const int64_t* buf_floats_per_crop, int32_t n_bufs,
                      const float* weights_host, size_t n_weights, int32_t max_crops, pa_convnet** out) {
    return pa_convnet_create_dtype(device, descs, n_descs, buf_floats_per_crop, n_bufs, weights_host, n_weights, max_crops, PA_DTYPE_F32, out);
}

int pa_convnet_create_dtype(int32_t device, const pa_conv_desc* descs, int32_t n_descs, const int64_t* buf_floats_per_crop, int32_t n_bufs,
                            const float* weights_host, size_t n_weights, int32_t max_crops, int32_t compute_dtype, pa_convnet** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (!descs || n_descs < 1 || !buf_floats_per_crop || n_bufs < 1 || !weights_host || n_weights < 1 || max_crops < 1 ||
        (compute_dtype != PA_DTYPE_F32 && compute_dtype != PA_DTYPE_EMULATED_F32 && compute_dtype != PA_DTYPE_BF16))
        return PA_ERR_INVALID_ARG;
    pa_convnet* h = new pa_convnet();
    *out = h;
    h->device = device;
    h->compute_dtype = compute_dtype;
    h->max_crops = max_crops;
    h->descs.assign(descs, descs + n_descs);
    h->forms.assign(n_descs, PA_CN_FORM_NOT_RUN);
    h->buf_floats.assign(buf_floats_per_crop, buf_floats_per_crop + n_bufs);
    h->buf_bf16.assign(n_bufs, compute_dtype == PA_DTYPE_BF16 ? 1 : 0);
    // validate the table: buffer indices, weight ranges, buffer sizes, one geometry per bordered buffer
    struct Geom { int hw = -1, pad = -1, c = -1; };
    std::vector<Geom> geom(n_bufs);
    auto use = [&](int b, int hw, int pad, int c, const char* what, int li) -> bool {
        if (b < 0 || b >= n_bufs) { h->last_error = "layer " + std::to_string(li) + ": bad " + what + " buffer"; return false; }
        const long long need = (long long)(hw + 2 * pad) * (hw + 2 * pad) * c;
        if (need > buf_floats_per_crop[b]) { h->last_error = "layer " + std::to_string(li) + ": " + what + " buffer too small"; return false; }
        Geom& g = geom[b];
        if (pad > 0 || g.pad > 0) {
            if (g.hw >= 0 && (g.hw != hw || g.pad != pad || g.c != c)) {
                h->last_error = "layer " + std::to_string(li) + ": zero-bordered buffer " + std::to_string(b) + " used with two geometries";
                return false;
            }
        }
        if (g.hw < 0 || pad > 0) { g.hw = hw; g.pad = pad; g.c = c; }
        return true;
    };
    for (int i = 0; i < n_descs; ++i) {
        const pa_conv_desc& d = h->descs[i];
        int ohw, oc;
        out_geom(d, &ohw, &oc);
        if (d.kind == 0) {
            if ((d.ksize != 1 && d.ksize != 3) || (d.stride != 1 && d.stride != 2) || d.cin % 32 != 0 || d.cout % 64 != 0 || d.in_hw < 1 ||
                d.in_hw % d.stride != 0 || d.in_pad < (d.ksize - 1) / 2 || d.out_pad < 0)
                return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": unsupported convolution");
            if (d.w_off < 0 || d.b_off < 0 || (size_t)d.w_off + (size_t)d.cout * d.ksize * d.ksize * d.cin > n_weights ||
                (size_t)d.b_off + d.cout > n_weights)
                return cn_fail(h, PA_ERR_BAD_WEIGHTS, "layer " + std::to_string(i) + ": weights outside the blob");
            if (!use(d.in_buf, d.in_hw, d.in_pad, d.cin, "input", i) || !use(d.out_buf, ohw, d.out_pad, oc, "output", i)) return PA_ERR_INVALID_ARG;
            if (d.res_buf >= 0 && !use(d.res_buf, ohw, d.out_pad, oc, "residual", i)) return PA_ERR_INVALID_ARG;
            // (the launchers address a buffer with 32-bit byte offsets)
            if ((long long)max_crops * (d.in_hw + 2 * d.in_pad) * (d.in_hw + 2 * d.in_pad) * d.cin * 4 >= (1ll << 31) ||
                (long long)max_crops * (ohw + 2 * d.out_pad) * (ohw + 2 * d.out_pad) * oc * 4 >= (1ll << 31))
                return cn_fail(h, PA_ERR_CAPACITY, "layer " + std::to_string(i) + ": max_crops maps of this size exceed 2 GiB");
        } else if (d.kind == 1) {
            if (d.out_pad != 1 || d.w_off < 0 || (size_t)d.w_off + 64 * 224 > n_weights || d.b_off < 0 || (size_t)d.b_off + 64 > n_weights)
                return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": bad stem");
            if (!use(d.out_buf, 32, 1, 64, "output", i)) return PA_ERR_INVALID_ARG;
        } else if (d.kind == 3) {
            const std::string row = "layer " + std::to_string(i) + " (stem of any size): ";
            if (compute_dtype == PA_DTYPE_BF16) return cn_fail(h, PA_ERR_INVALID_ARG, row + "a bf16 table takes the 128 x 128 stem (kind 1) only");
            if (d.in_hw % 32 != 0 || d.in_hw < 64 || d.in_hw > 512)
                return cn_fail(h, PA_ERR_INVALID_ARG, row + "in_hw must be a multiple of 32 in 64..512");
            if (d.in_pad != 3 || d.out_pad != 1 || d.cin != 3 || d.cout != 64) return cn_fail(h, PA_ERR_INVALID_ARG, row + "needs cin 3, cout 64, in_pad 3, out_pad 1");
            if (d.w_off < 0 || (size_t)d.w_off + 64 * 224 > n_weights || d.b_off < 0 || (size_t)d.b_off + 64 > n_weights)
                return cn_fail(h, PA_ERR_BAD_WEIGHTS, row + "weights outside the blob");
            if (h->sized) return cn_fail(h, PA_ERR_INVALID_ARG, row + "a table holds one stem row");
            if (!use(d.out_buf, d.in_hw / 4, 1, 64, "output", i)) return PA_ERR_INVALID_ARG;
            h->sized = true;
            h->in_hw = d.in_hw;
        } else if (d.kind == 2) {
            if (d.cin < 1 || d.in_hw < 1 || d.in_pad < 0) return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": bad pool");
            if (!use(d.in_buf, d.in_hw, d.in_pad, d.cin, "input", i) || !use(d.out_buf, 1, 0, d.cin, "output", i)) return PA_ERR_INVALID_ARG;
        } else {
            return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": unknown kind");
        }
    }
    if (h->sized)
        for (int i = 0; i < n_descs; ++i)
            if (h->descs[i].kind == 1) return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": a 128 x 128 stem beside a stem of another size");
    if (compute_dtype == PA_DTYPE_BF16) {
        // element type of each buffer from its writers: stem and convolutions bf16, the pool fp32; one type per buffer, every row
        // reads bf16, every convolution one bgemm takes, and the table ends in a pool (pa_convnet_forward's out is fp32)
        std::vector<int> wrote(n_bufs, -1);   // -1 unwritten, 1 bf16, 0 fp32
        for (int i = 0; i < n_descs; ++i) {
            const pa_conv_desc& d = h->descs[i];
            const int t = d.kind == 2 ? 0 : 1;
            if (wrote[d.out_buf] >= 0 && wrote[d.out_buf] != t)
                return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": buffer " + std::to_string(d.out_buf) + " written as both bf16 and fp32");
            wrote[d.out_buf] = t;
        }
        for (int b = 0; b < n_bufs; ++b) h->buf_bf16[b] = wrote[b] == 0 ? 0 : 1;
        for (int i = 0; i < n_descs; ++i) {
            const pa_conv_desc& d = h->descs[i];
            if (d.kind != 1 && (!h->buf_bf16[d.in_buf] || (d.kind == 0 && d.res_buf >= 0 && !h->buf_bf16[d.res_buf])))
                return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": reads an fp32 buffer (bf16 rows read bf16)");
            if (d.kind != 0) continue;
            const pa::GemmParams p = pa::conv_row_params(conv_row(d, max_crops));
            const unsigned long long in_bytes = (unsigned long long)max_crops * p.in_img_stride * 2ull;
            const unsigned long long out_bytes = (unsigned long long)max_crops * p.out_img_stride * 2ull;
            if (pa::psgemm_pick_bn(d.cout, d.res_buf >= 0) == 0 || p.M >= (1 << 24) || p.howo >= (1 << 16) || in_bytes >= (1ull << 31) ||
                out_bytes >= (1ull << 31) || d.relu < 0 || d.relu > 1)
                return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(i) + ": a convolution the bf16 GEMM (bgemm.hip) cannot take");
        }
        if (h->descs.back().kind != 2)
            return cn_fail(h, PA_ERR_INVALID_ARG, "layer " + std::to_string(n_descs - 1) + ": a bf16 table must end in a pool (the output is fp32)");
    }
    auto chk = [&](hipError_t e, const char* what) -> bool {
        if (e == hipSuccess) return true;
        h->last_error = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    if (!chk(hipSetDevice(device), "hipSetDevice")) return PA_ERR_NO_DEVICE;
    h->n_weights = n_weights;
    if (!chk(hipMalloc(&h->weights, n_weights * sizeof(float)), "hipMalloc weights")) return PA_ERR_HIP;
    if (!chk(hipMemcpy(h->weights, weights_host, n_weights * sizeof(float), hipMemcpyHostToDevice), "upload weights")) return PA_ERR_HIP;
    // which rows take which form; the planes themselves are FormWeights' business
    std::vector<pa::FormRow> rows(n_descs);
    std::vector<std::vector<unsigned short>> stems;
    for (int i = 0; i < n_descs; ++i) {
        const pa_conv_desc& d = h->descs[i];
        pa::FormRow& r = rows[i];
        if (d.kind == 1 && compute_dtype == PA_DTYPE_BF16) {
            // the stem's [64][224] weights rounded to nearest even once, as laid out: a slot of the bgemm plane packed here
            stems.emplace_back(64 * 224);
            for (int k = 0; k < 64 * 224; ++k) stems.back()[k] = pa::bf16_rne(weights_host[d.w_off + k]);
            r.forms = pa::FORM_BGEMM;
            r.packed = stems.back().data();
            r.packed_elems = stems.back().size();
        }
        if (d.kind != 0) continue;
        r = pa::FormRow{0, d.cin, d.cout, d.ksize, d.res_buf >= 0, d.w_off};
        if (compute_dtype == PA_DTYPE_BF16) {
            r.forms = pa::FORM_BGEMM;  // every convolution's weights rounded to nearest even once, in bgemm's plane layout
        } else if (wino_knob() && d.ksize == 3 && d.stride == 1 && d.in_pad == 1 && d.in_hw >= 8 && d.in_hw % 4 == 0 && d.cin % 8 == 0) {
            // stride-1 3x3 convolutions on maps of 8 x 8 and larger run as Winograd F(2x2, 3x3) (wino.hip, as in the engine's
            // ResNet-18: the 4 x 4 maps stay on the direct kernel)
            r.forms = pa::FORM_WINO;
            r.wino_tiles = (long long)max_crops * (d.in_hw / 4) * (d.in_hw / 4);
        } else if (compute_dtype == PA_DTYPE_EMULATED_F32 && d.cin % 32 == 0 && d.cout % 32 == 0) {
            // every convolution that is not in Winograd form and whose 128-pixel tiles can fill at least half the chip at max_crops runs on
            // the emulated-fp32 persistent GEMM (psgemm.hip; below that its one-workgroup-per-CU grid is mostly empty and the exact
            // engine's 64 x 64 tiles are faster: profiles/r06_pgemm_split_layers.txt, ResNet-18's 8 x 8 and 4 x 4 maps)
            const int ohw = d.in_hw / d.stride, bn = pa::psgemm_pick_bn(d.cout, d.res_buf >= 0);
            if (bn != 0 && (long long)(((long long)max_crops * ohw * ohw + 127) / 128) * (d.cout / bn) >= 128) r.forms = pa::FORM_PSGEMM;
        }
    }
    const char* what = "";
    if (!chk(h->fw.prepare(rows, weights_host, &what), what)) return PA_ERR_HIP;
    if (compute_dtype == PA_DTYPE_BF16) {
        const size_t slab_bytes = (size_t)pa::BGEMM_SLAB_ITEMS * 128 * 128 * sizeof(float);
        if (!chk(hipMalloc(&h->bg_slab, slab_bytes), "hipMalloc split-K slab")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&h->bg_tickets, pa::BGEMM_TICKETS * sizeof(int32_t)), "hipMalloc split-K tickets")) return PA_ERR_HIP;
        if (!chk(hipMemset(h->bg_tickets, 0, pa::BGEMM_TICKETS * sizeof(int32_t)), "hipMemset split-K tickets")) return PA_ERR_HIP;
    }
    h->bufs.assign(n_bufs, nullptr);
    for (int b = 0; b < n_bufs; ++b) {
        // (+ one 128-pixel tile of slack: a partial last tile of the patch kernel reads past the last crop)
        const size_t bytes = ((size_t)max_crops * h->buf_floats[b] + 128 * 2048) * (h->buf_bf16[b] ? 2 : sizeof(float));
        if (!chk(hipMalloc(&h->bufs[b], bytes), "hipMalloc activations")) return PA_ERR_HIP;
        if (!chk(hipMemset(h->bufs[b], 0, bytes), "hipMemset activations")) return PA_ERR_HIP;
    }
    const size_t x0_bytes = (size_t)max_crops * (h->in_hw + 6) * (h->in_hw + 6) * 4 * sizeof(float);
    if (!chk(hipMalloc(&h->x0, x0_bytes), "hipMalloc input")) return PA_ERR_HIP;
    if (!chk(hipMemset(h->x0, 0, x0_bytes), "hipMemset input")) return PA_ERR_HIP;
    return PA_OK;
}

void pa_convnet_destroy(pa_convnet* h) {
    if (!h) return;
    (void)hipFree(h->weights);
    (void)hipFree(h->bg_slab);
    (void)hipFree(h->bg_tickets);
    (void)hipFree(h->x0);
    for (float* b : h->bufs) (void)hipFree(b);
    delete h;
}

}  // extern "C"

namespace {

// What pa_convnet_forward enqueues for n crops, up to and including layer `last` (-1: the input conversion alone); records
// each layer's form. Arguments are checked by the callers.
int convnet_run(pa_convnet* h, const float* x, int32_t n, int last, hipStream_t s) {
    const bool bf = h->compute_dtype == PA_DTYPE_BF16;
    if (h->sized) CN_HIP(pa::launch_nchw_to_padded_sized(x, h->x0, n, h->in_hw, s));
    else CN_HIP(pa::launch_nchw_to_padded(x, h->x0, n, bf ? 1 : 0, s));
    for (int li = 0; li <= last; ++li) {
        const pa_conv_desc& d = h->descs[li];
        if (d.kind == 1) {
            pa::StemPoolParams sp;
            memset(&sp, 0, sizeof(sp));
            sp.x = h->x0;
            sp.wgt = bf ? (const void*)(h->fw.bgemm + h->fw.bgemm_off[li]) : (const void*)(h->weights + d.w_off);
            sp.bias = h->weights + d.b_off;
            sp.out = h->bufs[d.out_buf];
            sp.crops = n;
            sp.in_bf16 = sp.out_bf16 = bf ? 1 : 0;
            CN_HIP(pa::launch_stem_pool(sp, s));
            h->forms[li] = PA_CN_FORM_STEM_POOL;
            continue;
        }
        if (d.kind == 3) {
            pa::StemPoolAnyParams sp;
            memset(&sp, 0, sizeof(sp));
            sp.x = h->x0;
            sp.wgt = h->weights + d.w_off;
            sp.bias = h->weights + d.b_off;
            sp.out = h->bufs[d.out_buf];
            sp.crops = n;
            sp.in_hw = d.in_hw;
            CN_HIP(pa::launch_stem_pool_any(sp, s));
            h->forms[li] = PA_CN_FORM_STEM_POOL_ANY;
            continue;
        }
        if (d.kind == 2) {
            const size_t total = (size_t)n * d.cin;
            int grid = (int)((total + 255) / 256);
            grid = grid > 2048 ? 2048 : grid;
            if (bf) {
                hipLaunchKernelGGL(pa::avgpool_bf16_any_kernel, dim3(grid), dim3(256), 0, s, (const unsigned short*)h->bufs[d.in_buf], h->bufs[d.out_buf], n,
                                   d.in_hw, d.in_pad, d.cin);
                h->forms[li] = PA_CN_FORM_AVGPOOL_BF16;
            } else {
                hipLaunchKernelGGL(pa::avgpool_any_kernel, dim3(grid), dim3(256), 0, s, h->bufs[d.in_buf], h->bufs[d.out_buf], n, d.in_hw, d.in_pad, d.cin);
                h->forms[li] = PA_CN_FORM_AVGPOOL;
            }
            CN_HIP(hipGetLastError());
            continue;
        }
        pa::GemmParams p = pa::conv_row_params(conv_row(d, n));
        p.act = h->bufs[d.in_buf];
        p.wgt = h->weights + d.w_off;
        p.bias = h->weights + d.b_off;
        p.residual = d.res_buf >= 0 ? h->bufs[d.res_buf] : nullptr;
        p.out = h->bufs[d.out_buf];
        if (bf) {
            // every convolution on the one-slice bf16 GEMM; split-K where bgemm_pick_split says (PA_CONVNET_BG_SPLIT: A/B)
            const int S = pa::bgemm_pick_split(p, bg_split_knob());
            if (S > 1) {
                p.splitk = S;
                p.slab = h->bg_slab;
                p.tickets = h->bg_tickets;
            }
            const hipError_t pe = pa::launch_bgemm(p, h->fw.bgemm + h->fw.bgemm_off[li], (size_t)n * p.out_img_stride, 0, false, s);
            if (pe != hipSuccess)
                return cn_fail(h, PA_ERR_HIP, "layer " + std::to_string(li) + " (bf16): " +
                                                  (pe == hipErrorInvalidValue ? std::string("the bf16 GEMM refuses its shape") : hipGetErrorString(pe)));
            h->forms[li] = S > 1 ? PA_CN_FORM_BGEMM_SPLITK : PA_CN_FORM_BGEMM;
            continue;
        }
        const pa::GemmTile tile = pa::im2col_tile(p.M, p.N);
        hipError_t pe = hipErrorInvalidValue;
        int32_t form = PA_CN_FORM_PSGEMM;
        if (h->fw.psgemm_off[li] >= 0) pe = pa::launch_psgemm(p, h->fw.psgemm + h->fw.psgemm_off[li], (size_t)n * p.out_img_stride, 0, s);
        if (pe == hipErrorInvalidValue && h->fw.wino_off[li] >= 0) {
            form = PA_CN_FORM_WINO;
            pe = pa::launch_wino3x3(pa::wino_params(p, n, d.in_hw, d.in_hw, d.cin, h->fw.wino + h->fw.wino_off[li], h->fw.wino_bn[li]), s);
        }
        // (the patch-resident kernel's tiles and chunk swizzle are laid out for maps 32, 16, 8 and 4 pixels wide: no other width is tried)
        if (pe == hipErrorInvalidValue && d.ksize == 3 && d.stride == 1 && d.in_pad == 1 && (d.in_hw == 32 || d.in_hw == 16 || d.in_hw == 8 || d.in_hw == 4)) {
            form = PA_CN_FORM_PATCH;
            pe = pa::launch_conv3x3_patch(p, tile == pa::TILE_64x64 ? 64 : 128, s);
        }
        if (pe == hipErrorInvalidValue) {
            form = tile == pa::TILE_128x128 ? PA_CN_FORM_IGEMM_128x128 : (tile == pa::TILE_128x64 ? PA_CN_FORM_IGEMM_128x64 : PA_CN_FORM_IGEMM_64x64);
            pe = pa::launch_igemm(p, tile, s);
        }
        if (pe != hipSuccess) return cn_fail(h, PA_ERR_HIP, "layer " + std::to_string(li) + ": " + hipGetErrorString(pe));
        h->forms[li] = form;
    }
    return PA_OK;
}

}  // namespace

extern "C" {

int pa_convnet_forward(pa_convnet* h, const float* x, int32_t n, float* out, int32_t out_floats_per_crop, void* stream) {
    if (!h) return PA_ERR_INVALID_ARG;
    if (!x || !out || n < 1) return cn_fail(h, PA_ERR_INVALID_ARG, "pa_convnet_forward: bad argument");
    if (n > h->max_crops) return cn_fail(h, PA_ERR_CAPACITY, "pa_convnet_forward: more crops than max_crops");
    hipStream_t s = (hipStream_t)stream;
    const int rc = convnet_run(h, x, n, (int)h->descs.size() - 1, s);
    if (rc != PA_OK) return rc;
    // the last layer's output buffer as stored, zero border included when it has one (a pooled vector has none; under
    // PA_DTYPE_BF16 the last row is a pool, fp32)
    const pa_conv_desc& last = h->descs.back();
    int ohw, oc;
    out_geom(last, &ohw, &oc);
    const int opad = last.kind == 0 ? last.out_pad : (last.kind == 1 || last.kind == 3 ? 1 : 0);
    const int per_crop = (ohw + 2 * opad) * (ohw + 2 * opad) * oc;
    if (out_floats_per_crop != per_crop) return cn_fail(h, PA_ERR_INVALID_ARG, "pa_convnet_forward: out_floats_per_crop does not match the last layer");
    CN_HIP(hipMemcpyAsync(out, h->bufs[last.out_buf], (size_t)n * per_crop * sizeof(float), hipMemcpyDeviceToDevice, s));
    return PA_OK;
}

int pa_convnet_trace(pa_convnet* h, const float* x, int32_t n, int32_t last_row, int32_t buf, void* out, size_t out_bytes, void* stream) {
    if (!h) return PA_ERR_INVALID_ARG;
    auto fail = [&](const char* msg) { return cn_fail(h, PA_ERR_INVALID_ARG, std::string("pa_convnet_trace: ") + msg); };
    if (!x || !out) return fail("bad argument");
    if (n < 1 || n > h->max_crops) return fail("n outside 1..max_crops");
    if (last_row < -1 || last_row >= (int32_t)h->descs.size()) return fail("row out of range");
    if (buf < -1 || buf >= (int32_t)h->buf_floats.size()) return fail("buffer out of range");
    const size_t elems = (size_t)h->max_crops * (buf < 0 ? (size_t)(h->in_hw + 6) * (h->in_hw + 6) * 4 : (size_t)h->buf_floats[buf]);
    const size_t bytes = elems * (is_bf16(h, buf) ? 2 : sizeof(float));
    if (out_bytes < bytes) return fail("out is smaller than the buffer");
    if (buf >= (int32_t)h->bufs.size() || !h->x0) return fail("the handle holds no buffers (its creation failed)");
    hipStream_t s = (hipStream_t)stream;
    const int rc = convnet_run(h, x, n, last_row, s);
    if (rc != PA_OK) return rc;
    const hipError_t e = hipMemcpyAsync(out, buf < 0 ? h->x0 : h->bufs[buf], bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return cn_fail(h, PA_ERR_HIP, std::string("pa_convnet_trace: hipMemcpyAsync: ") + hipGetErrorString(e));
    return PA_OK;
}

int pa_convnet_layer_forms(const pa_convnet* h, int32_t* forms, int32_t cap) {
    if (!h || !forms || cap < (int32_t)h->forms.size()) return PA_ERR_INVALID_ARG;
    std::copy(h->forms.begin(), h->forms.end(), forms);
    return PA_OK;
}

}  // extern "C"

// C-ABI host side of the MI355X action-recognition path (include/playaid_hip.h).
// Owns device buffers, folds/re-lays-out the weights, sequences the kernels of
// one forward on the caller's stream. No torch types, no hidden synchronisation
// in the enqueue calls.
#include "../../include/playaid_hip.h"
#include "conv_rows.h"
#include "engine_table.h"   // the layer table, over engine_plan.h
#include "synth_math.h"     // SynthDesc, runner_in_plan
#include "scene_math.h"     // resize_read, scene_read, scene_bytes_padded
#include "train_common.h"   // adam_scalars, adam_config_ok, TrainerCore

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pa;

namespace {

static_assert(FEATURE_STRIDE == PA_FEATURE_STRIDE, "engine_table.h pads the fc to the cached feature rows' width");
constexpr int WINO_TICKETS = 4096;   // tiles of one Winograd launch that may use split K (more: no split)

// A row of the layer table (engine_table.h): what engine_plan.h plans from, plus its buffers and weights
struct ConvLayer : LayerDesc {
    std::string name;
    float* in = nullptr;
    float* out = nullptr;
    float* residual = nullptr;
    float* wgt = nullptr;   // device [cout][taps*chunk]; block-0 conv2 of layers 2-4, fp32: [W2 | Wd], the branch as extra K read from `ds.src`
    float* wino_wgt = nullptr;  // LayerDesc::wino: the filters in wino.hip's layout
    int wino_bn = 0;            // ... laid out for workgroups of this many output channels (wino_layer_shape at the full batch)
    WinoShape wino_shape = WINO_SHAPE_SPLIT;  // ... and how its launches are shaped: with the split-K scratch, or unsplit on one of three workgroups
    int wino_wg = 0;            // ... and how many output channels a workgroup of them takes: wino_bn, or 32 beside wino_bn == 64 (wino_layer_wg)
    float* wino4_wgt = nullptr; // LayerDesc::wino4: the filters as wino4.hip's 36 GEMM images
    float* bias = nullptr;  // device [cout]
    unsigned short* split_wgt = nullptr;  // LayerDesc::split: three bf16 slices per weight in psgemm.hip's stage-image order
    // conv2 of block 0 of layers 2-4: its 1x1/2 downsample branch (LayerDesc::branch says where it is computed)
    struct {
        float* src = nullptr;   // the zero-bordered block input
        float* wgt = nullptr;   // [cout][branch.c], bf16 on the bf16 path; nullptr: BRANCH_SECOND_K
        float* out = nullptr;   // the stored branch, laid out like `out` (no bias, no activation): conv2 adds it as its residual
        unsigned short* split_wgt = nullptr;  // LayerDesc::branch.split
    } ds;
    int carries_of = -1;  // the block's opener (LayerDesc::carries): index in pa_engine::convs of the conv2 whose branch it carries
};

struct ProfEntry {
    int name_id;
    hipEvent_t start, stop;
    double flops, bytes;
    double flops_executed;  // = flops unless the launch runs an algorithm that executes fewer (Winograd: 4 / 9)
};

}  // namespace

struct pa_engine {
    pa_config cfg;
    std::string last_error;
    int max_crops = 0;   // crops per backbone call
    EngineKnobs knobs;   // the environment's knobs as pa_create found them (engine_plan.h)
    ComputeDtype dtype = DT_F32;  // cfg.compute_dtype, as engine_plan.h counts it
    bool emu = false;   // cfg.compute_dtype == PA_DTYPE_EMULATED_F32: fp32 buffers and interfaces, the layers that have ConvLayer::split_wgt on psgemm.hip
    bool bf16 = false;   // cfg.compute_dtype == PA_DTYPE_BF16: the 3x3 conv stack stores bf16 (buffers keep their fp32 size)
    int cache_rows = 0;  // feature-cache rows
    // clip state
    int clip_frames = 0;
    int sub_frames = 0;  // > 0: the clip is a batch of independent clips of this many frames (pa_clip_begin_batch)
    int* gate_flag = nullptr;    // coherent pinned word the host opens pa_stream_gate's kernel with
    int jpeg_quality = 0;        // > 0: every crop goes through a baseline-JPEG write + read (pa_set_crop_jpeg_quality)
    int32_t* jpeg_qtab = nullptr; // [2][64] device
    uint8_t* crops_tmp = nullptr; // [max_crops][128][128][3]: the crops when the caller did not ask for them
    std::vector<char> ready;
    // device memory (all freed in pa_destroy)
    std::vector<void*> allocs;
    // every folded / re-laid-out weight tensor lives in ONE device arena at offsets that depend only on what the layer table and the
    // entries' sizes depend on: S, A, compute_dtype, the per-process knobs (EngineKnobs' first part) and whether max_crops reaches knobs.wino_f4_min (layer
    // 4's F(4x4) filters). A rank that received the arena over RCCL from an engine equal in all of these adopts it with one device
    // copy (pa_create_from_arena) instead of folding the blob again. (The size check of adopt mode sees the offsets only: the Winograd
    // filters' order inside their entry also follows ConvLayer::wino_bn, which wino_layer_shape takes from max_crops)
    uint8_t* arena = nullptr;
    size_t arena_cap = 0, arena_used = 0;
    std::vector<uint8_t> arena_stage;  // host mirror while pa_create folds (empty in adopt mode and afterwards)
    int32_t* dev_errors = nullptr;  // [4] device-side error counters ([0] = scatter ids outside the clip, [1] = crop images that did not fit)
    int32_t* savebox_rects = nullptr;  // [max_crops][4] scratch of pa_save_one_box_crops
    double* clean_g6 = nullptr;        // scratch of pa_clean_detections: the detection table through '%g' (grown on demand)
    size_t clean_g6_cap = 0;
    float* x0 = nullptr;      // slot 0 of the model-input double buffer [max_crops][134][134][4]
    float* x0_slot[2] = {nullptr, nullptr};
    // Integer stem (stem_pool.hip FORM 2): the producers that make the model input from u8 pixels (crop stage, runner
    // inputs, JPEG round trip) write the pixel INTEGERS as bf16 into these dedicated, once-zeroed buffers instead of k / 255 into
    // x0_slot; whatever comes as caller floats (pa_infer_windows, pa_backbone_windows, pa_backbone_trace) keeps x0 and the fp32 stem
    bool stem_int = false;                        // exact engines (f32, emulated_f32) unless PA_STEM_INT=0
    uint16_t* xi_slot[2] = {nullptr, nullptr};    // [max_crops][134][134][4] bf16, border and fourth channel zero for ever
    int slot_form[2] = {0, 0};                    // which buffer the slot's last producer wrote: 0 = x0_slot, 2 = xi_slot
    uint16_t* stem_wgt_int = nullptr;             // [3][64][224]: the three bf16 slices of the folded fp32 stem weights
    int32_t* pre_status[2] = {nullptr, nullptr};  // per-slot crop status written by the preprocess stage
    float* pooled = nullptr;  // [max_crops][512]
    float* feats_tmp = nullptr;  // [max_crops][1024] (b1 path)
    float* cache = nullptr;      // [cache_rows][1024]
    int32_t* cache_status = nullptr;  // [cache_rows]
    float* h1 = nullptr;              // [max_crops][512]
    int32_t* gather = nullptr;        // [max_crops][S]
    int gather_key[4] = {-1, -1, -1, -1}; // (f0, cnt, clip_frames, sub_frames) the table in `gather` was built for; -1 = none (other users of the buffer reset it)
    float* slab = nullptr;
    size_t slab_floats = 0;
    float* wino_tickets = nullptr;  // int32[2][WINO_TICKETS], zero between launches: split-K tickets of the Winograd kernel, one set per half batch
    float* wino4_scratch = nullptr;  // V and M of wino4.hip, one region of wino4_region floats per interleaved half batch
    size_t wino4_region = 0;
    std::vector<ConvLayer> convs;  // stem + the sixteen 3x3 convs (a block-0 downsample belongs to its conv2's entry)
    ConvLayer fc;
    float* stem_wgt_bf16 = nullptr;  // bf16 path: the folded stem weights [64][224] as bf16
    float* c1 = nullptr;  // stem output [max_crops][66][66][64] (only the unfused stem + pool fallback writes it)
    float* p1 = nullptr;  // maxpool output [max_crops][34][34][64]
    float* layer4_out = nullptr;
    // head weights
    float* w1d = nullptr;  // [512][S*1024]
    float* b1d = nullptr;
    float *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
    GemmTile head_tile = TILE_64x64;
    int head_splitk = 16;
    // preprocess scratch
    CropPlan* plans = nullptr;
    int32_t* coef = nullptr;
    int coef_dim = 0;
    int32_t* coef_cache = nullptr;  // Pillow tables of the passes (2 * (d / 2) + 2 * padding -> d), built for one padding at a time
    int coef_cache_pad = -1, coef_cache_dmax = 0;
    AreaTabPacked* area_tabs = nullptr;
    uint8_t* hop = nullptr;  // the horizontal matrix form's operands: [max crops][PA_HOP_BLOCKS_MAX][PA_HOP_BLOCK_BYTES]
    uint8_t *t1 = nullptr, *t2 = nullptr;
    size_t t_stride = 0;
    int32_t* status_tmp = nullptr;
    int32_t* fallback = nullptr;  // [1 + max_crops]: count, then crop indices
    AugmentTables* aug_tabs = nullptr;  // pa_augment_crops: the normal quantiles, OpenCV's two HSV division tables, k / 255 (augment.hip)
    // two-way interleave of the backbone (two half batches on two streams; knobs.interleave: measured +0.5 % only -- kernels of two
    // streams do not overlap usefully -- and kept as a knob)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_ds_fork = nullptr, ev_ds_join = nullptr;   // PA_DS_SIDE: a block's 1x1/2 branch GEMM on the side stream, under its opener
    // profiling
    bool profiling = false;
    std::vector<std::string> prof_names;
    std::vector<ProfEntry> prof_log;
    std::vector<hipEvent_t> event_pool;
};

namespace {

int fail(pa_engine* e, int code, const std::string& msg) {
    if (e) e->last_error = msg;
    return code;
}

// model input of `slot`: where its next producer writes (recording the form), and what its last producer wrote
float* slot_dst(pa_engine* e, int slot) {
    e->slot_form[slot] = e->stem_int ? 2 : 0;
    return e->stem_int ? reinterpret_cast<float*>(e->xi_slot[slot]) : e->x0_slot[slot];
}
const float* slot_src(const pa_engine* e, int slot) {
    return e->slot_form[slot] == 2 ? reinterpret_cast<const float*>(e->xi_slot[slot]) : e->x0_slot[slot];
}
// storage of a model-input buffer as PreprocParams::crops_f32_is_bf16 counts it: 2 = one of the integer buffers
int input_form(const pa_engine* e, const void* x) {
    if (x && e->stem_int && (x == e->xi_slot[0] || x == e->xi_slot[1])) return 2;
    return e->bf16 ? 1 : 0;
}

#define HIPCHK(e, call)                                                                              \
    do {                                                                                             \
        hipError_t err__ = (call);                                                                   \
        if (err__ != hipSuccess)                                                                     \
            return fail((e), PA_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(err__));      \
    } while (0)

template <typename T>
int dev_alloc(pa_engine* e, T** ptr, size_t count, bool zero) {
    void* p = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    HIPCHK(e, hipMalloc(&p, bytes));
    e->allocs.push_back(p);
    if (zero) HIPCHK(e, hipMemset(p, 0, bytes));
    *ptr = reinterpret_cast<T*>(p);
    return PA_OK;
}

// Place `n` elements of T in the weight arena (256-byte aligned bump): *dst gets their device address, in both modes of create.
// *stage: where pa_create writes them on the host for the single upload at its end (zeroed), nullptr when the arena is adopted
template <typename T, typename D>
int arena_place(pa_engine* e, D** dst, size_t n, T** stage) {
    const size_t off = (e->arena_used + 255) & ~(size_t)255, bytes = n * sizeof(T);
    if (off + bytes > e->arena_cap) return fail(e, PA_ERR_BAD_WEIGHTS, "weight arena overflow");
    e->arena_used = off + bytes;
    *dst = reinterpret_cast<D*>(e->arena + off);
    *stage = e->arena_stage.empty() ? nullptr : reinterpret_cast<T*>(e->arena_stage.data() + off);
    return PA_OK;
}

// ... n floats, the first n_host of them from `host` and the rest zero
int put(pa_engine* e, float** dst, size_t n, const float* host, size_t n_host) {
    float* s;
    const int rc = arena_place(e, dst, n, &s);
    if (!rc && s) memcpy(s, host, n_host * sizeof(float));
    return rc;
}
int put(pa_engine* e, float** dst, size_t n, const float* host) { return put(e, dst, n, host, n); }

// ... as bf16 (round to nearest even): weights of the bf16 conv path; the device pointer keeps the float* type of ConvLayer::wgt,
// the kernels reinterpret it.
int put_bf16(pa_engine* e, float** dst, size_t n, const float* host) {
    uint16_t* s;
    const int rc = arena_place(e, dst, n, &s);
    for (size_t i = 0; !rc && s && i < n; ++i) s[i] = bf16_rne(host[i]);
    return rc;
}

// ... fp32 [cout][ktot] as three bf16 slices per weight in psgemm.hip's stage-image order (PA_DTYPE_EMULATED_F32)
int put_split(pa_engine* e, unsigned short** dst, const float* host, int cout, int ktot) {
    const size_t n = psgemm_weight_elems(cout, ktot, false);
    if (n == 0) return PA_ERR_INVALID_ARG;
    unsigned short* s;
    const int rc = arena_place(e, dst, n, &s);
    if (!rc && s) psgemm_pack_weights(host, cout, ktot, false, s);
    return rc;
}

// --- weight blob walking (pa_create only) --------------------------------------
struct BlobReader {
    const float* base;
    size_t pos, limit;  // in floats
    const float* take(size_t n) {
        if (pos + n > limit) return nullptr;
        const float* r = base + pos;
        pos += n;
        return r;
    }
};

// Fold eval-mode BatchNorm (eps 1e-5) into conv weights in fp64 and re-lay-out
// OIHW -> [cout][tap][chunk] (tap = ky*kw_taps + kx, channels innermost, zero
// padded to `chunk`). The 7x7 stem uses tap = ky and chunk = 8 px * 4 ch.
bool fold_conv(BlobReader& br, const LayerDesc& L, std::vector<float>& w_out, std::vector<float>& b_out) {
    const size_t wn = (size_t)L.cout * L.cin * L.kh * L.kw;
    const float* w = br.take(wn);
    const float* gamma = br.take(L.cout);
    const float* beta = br.take(L.cout);
    const float* mean = br.take(L.cout);
    const float* var = br.take(L.cout);
    if (!w || !gamma || !beta || !mean || !var) return false;
    const int ktot = L.taps * L.chunk;
    w_out.assign((size_t)L.cout * ktot, 0.f);
    b_out.assign(L.cout, 0.f);
    const bool stem = (L.kh == 7);
    for (int co = 0; co < L.cout; ++co) {
        const double scale = (double)gamma[co] / std::sqrt((double)var[co] + 1e-5);
        b_out[co] = (float)((double)beta[co] - (double)mean[co] * scale);
        for (int ci = 0; ci < L.cin; ++ci)
            for (int ky = 0; ky < L.kh; ++ky)
                for (int kx = 0; kx < L.kw; ++kx) {
                    const double v = (double)w[(((size_t)co * L.cin + ci) * L.kh + ky) * L.kw + kx] * scale;
                    size_t k;
                    if (stem)
                        k = (size_t)ky * L.chunk + kx * 4 + ci;
                    else
                        k = (size_t)(ky * L.kw + kx) * L.chunk + ci;
                    w_out[(size_t)co * ktot + k] = (float)v;
                }
    }
    return true;
}

// --- profiling ------------------------------------------------------------------
int prof_name_id(pa_engine* e, const char* name) {
    for (size_t i = 0; i < e->prof_names.size(); ++i)
        if (e->prof_names[i] == name) return (int)i;
    e->prof_names.push_back(name);
    return (int)e->prof_names.size() - 1;
}

hipEvent_t get_event(pa_engine* e) {
    if (!e->event_pool.empty()) {
        hipEvent_t ev = e->event_pool.back();
        e->event_pool.pop_back();
        return ev;
    }
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}

struct ProfScope {
    pa_engine* e;
    hipStream_t s;
    ProfEntry ent;
    bool on;
    ProfScope(pa_engine* e_, hipStream_t s_, const char* name, double flops, double bytes, double executed = -1.0)
        : e(e_), s(s_), on(e_->profiling) {
        if (!on) return;
        ent.name_id = prof_name_id(e, name);
        ent.flops = flops;
        ent.flops_executed = executed >= 0.0 ? executed : flops;
        ent.bytes = bytes;
        ent.start = get_event(e);
        ent.stop = get_event(e);
        if (!ent.start || !ent.stop) {
            on = false;
            return;
        }
        (void)hipEventRecord(ent.start, s);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(ent.stop, s);
        e->prof_log.push_back(ent);
    }
};

// element `elems` of a layer buffer: 2-byte elements on the bf16 conv path (bf), else floats
float* buf_at(float* base, size_t elems, bool bf) { return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elems * (bf ? 2 : 4)); }

// PA_DS_SIDE=1 (A/B): the 1x1/2 branch GEMM of a block (layers 2-4: ~10 us each, a few dozen tiles) is
// launched on the side stream BEFORE the block's stride-2 opener instead of between the opener and conv2 -- both read the block
// input, so the small GEMM runs under the opener and conv2 only waits for an event. Whether the launches on `s` do so
bool branch_on_side(const pa_engine* e, hipStream_t s) { return e->knobs.ds_side && !e->profiling && !e->bf16 && e->side && s != e->side; }

// The 1x1/2 downsample branch of conv2 `L` as a GEMM of its own: the zero-bordered block input -> ds.out, laid out like L's output
// (add_conv builds the block so that L's output is branch.hw / branch.stride on a side with whole pixels of cout channels:
// the branch's M, howo, wo and output strides come out equal to the convolution's)
int run_branch_gemm(pa_engine* e, const ConvLayer& L, const BranchPlan& b, int crop0, int ncrops, size_t slab_off, hipStream_t s, const char* prof_name) {
    const int hw = L.branch.hw, c = L.branch.c, out_w = L.out_hw + 2 * L.out_pad;
    const size_t out_crop = (size_t)out_w * out_w * L.cout;
    GemmParams d = conv_row_params({/*images*/ ncrops, /*in h, w, pad, px stride*/ hw, hw, 1, c,
                                    /*cin, cout, ksize, stride*/ c, L.cout, 1, L.branch.stride,
                                    /*out pad, px stride*/ L.out_pad, L.cout, /*act, res_after*/ 0, 0});
    d.act = buf_at(L.ds.src, (size_t)crop0 * (hw + 2) * (hw + 2) * c, e->bf16);
    d.wgt = L.ds.wgt;
    d.out = buf_at(L.ds.out, crop0 * out_crop, e->bf16);
    d.slab = e->slab + slab_off;
    ProfScope ps(e, s, prof_name, b.acct.flops, b.acct.bytes);
    if (e->bf16) HIPCHK(e, launch_igemm_bf16(d, b.tile, s));
    else if (b.psgemm) HIPCHK(e, launch_psgemm(d, L.ds.split_wgt, (size_t)ncrops * out_crop, 0, s));
    else HIPCHK(e, launch_igemm(d, b.tile, s));
    return PA_OK;
}

// One layer: what plan_conv (engine_plan.h) decides, launched. crop0: first crop of this launch inside the layer's buffers (the two
// interleaved half batches address disjoint crop ranges of the same buffers); slab_off: its split-K slab region.
int run_conv(pa_engine* e, const ConvLayer& L, int crop0, int ncrops, size_t slab_off, hipStream_t s, const char* prof_name) {
    const size_t slab_avail = e->slab_floats > slab_off ? e->slab_floats - slab_off : 0;
    const ConvPlan P = plan_conv(e->knobs, e->dtype, L, ncrops, slab_avail, branch_on_side(e, s));
    const bool bf = e->bf16 && L.kh == 3;  // bf16 conv path: the 3x3 stack (buffers addressed in 2-byte elements)
    const int in_w = L.in_hw + 2 * L.in_pad;
    const int out_w = L.out_hw + 2 * L.out_pad;
    const size_t in_crop = (size_t)in_w * in_w * L.in_px_stride;
    const size_t out_crop = (size_t)out_w * out_w * L.cout;
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.act = buf_at(L.in, crop0 * in_crop, bf);
    p.wgt = L.wgt;
    p.bias = L.bias;
    p.residual = L.residual ? buf_at(L.residual, crop0 * out_crop, bf) : nullptr;
    p.out = buf_at(L.out, crop0 * out_crop, bf);
    p.slab = e->slab + slab_off;
    p.gather = nullptr;
    p.M = P.M;
    p.N = P.N;
    p.taps = L.taps;
    p.kw_taps = L.kw_taps;
    p.chunk = L.chunk;
    p.ktot = P.ktot;
    p.skip_w = L.kh == 7;  // stem: 3 channels in 4-float pixels
    p.howo = L.out_hw * L.out_hw;
    p.wo = L.out_hw;
    p.in_px_stride = L.in_px_stride;
    p.in_row_stride = in_w * L.in_px_stride;
    p.in_img_stride = (int)in_crop;
    p.stride = L.stride;
    p.off_y = L.off;
    p.off_x = L.off;
    p.out_px_stride = L.cout;
    p.out_row_stride = out_w * L.cout;
    p.out_img_stride = (int)out_crop;
    p.out_pad = L.out_pad;
    p.relu = L.relu;
    p.splitk = P.splitk;
    if (P.branch == BL_GEMM_BEFORE) {
        const int rc = run_branch_gemm(e, L, P.branch_gemm, crop0, ncrops, slab_off, s, prof_name);
        if (rc) return rc;
    }
    if (P.branch == BL_GEMM_BEFORE || P.branch == BL_STORED) {
        p.residual = buf_at(L.ds.out, crop0 * out_crop, bf);
    } else if (P.branch == BL_SECOND_K) {
        const int w2 = L.branch.hw + 2;  // zero-bordered block input
        p.act2 = buf_at(L.ds.src, (size_t)crop0 * w2 * w2 * L.branch.c, bf);
        p.k2_steps = L.branch.c / (bf ? 64 : 32);
        p.in2_px_stride = L.branch.c;
        p.in2_row_stride = w2 * L.branch.c;
        p.in2_img_stride = w2 * w2 * L.branch.c;
        p.stride2 = L.branch.stride;
        p.off2 = 1;
    }
    const ConvLayer* C2 = L.carries_of >= 0 ? &e->convs[L.carries_of] : nullptr;  // the conv2 whose branch this opener carries
    if (bf && P.branch == BL_ON_OPENER) {
        p.wgt2 = C2->ds.wgt;
        p.out2 = buf_at(C2->ds.out, crop0 * out_crop, bf);
    }
    bool branch_left = P.branch == BL_GEMM_BEHIND;   // the fp32 opener's branch is still to be computed
    {   // (the opener's profile scope ends before its branch's begins)
        ProfScope ps(e, s, prof_name, P.acct.flops, P.acct.bytes, P.acct.flops_executed);
        hipError_t pe = hipErrorInvalidValue;   // a launcher's refusal: the next form takes the launch
        if (P.form == CONV_PSGEMM) {
            pe = launch_psgemm(p, L.split_wgt, (size_t)ncrops * out_crop, 0, s);
        } else if (P.form == CONV_WINO && P.wino_f4) {   // F(4x4, 3x3) taken apart: three launches in this one profile row
            Wino4Params q{};
            q.act = p.act; q.wgt = L.wino4_wgt; q.bias = p.bias; q.residual = p.residual; q.out = p.out;
            q.v = e->wino4_scratch + (slab_off ? e->wino4_region : 0);
            q.m = q.v + (size_t)36 * wino4_rows(ncrops) * L.cin;
            q.n_img = ncrops; q.cin = L.cin; q.cout = L.cout;
            q.in_px_stride = p.in_px_stride; q.in_row_stride = p.in_row_stride; q.in_img_stride = p.in_img_stride;
            q.out_px_stride = p.out_px_stride; q.out_row_stride = p.out_row_stride; q.out_img_stride = p.out_img_stride; q.out_pad = p.out_pad;
            q.relu = p.relu; q.res_after = p.res_after;
            pe = launch_wino4_conv3x3(q, s);
        } else if (P.form == CONV_WINO) {
            WinoParams q = wino_params(p, ncrops, L.out_hw, L.out_hw, L.cin, L.wino_wgt, L.wino_bn);
            q.tg2 = L.wino_shape == WINO_SHAPE_TG2;
            // width 32 beside a 64-channel layout where this launch cannot split; a launch of few crops that can keeps its split
            const bool wg32 = L.wino_bn == 64 && wino_launch_wg(L.wino_wg, L.wino_bn, L.cin, L.cout, L.out_hw, ncrops, wino_ks_force()) == 32;
            if (wg32) q.wg = 32;
            if (!wg32 && L.wino_shape == WINO_SHAPE_SPLIT && e->wino_tickets && e->slab) {   // split-K scratch: this half batch's region
                q.slab = e->slab + slab_off;
                q.slab_floats = e->slab_floats > slab_off ? std::min(e->slab_floats - slab_off, e->slab_floats / 2) : 0;
                q.tickets = reinterpret_cast<int32_t*>(e->wino_tickets) + (slab_off ? WINO_TICKETS : 0);
                q.tickets_cap = WINO_TICKETS;
            }
            pe = launch_wino3x3(q, s);
        } else if (bf) {
            if (P.form == CONV_BF16_PATCH) pe = launch_conv3x3_bf16_patch(p, s);
            if (pe == hipErrorInvalidValue) pe = launch_igemm_bf16(p, P.tile_256 ? TILE_256x128 : P.tile, s);
        } else {
            if (P.form == CONV_PATCH) pe = launch_conv3x3_patch(p, P.patch_bm, s);
            if (P.form == CONV_PGEMM && P.branch == BL_ON_OPENER) {   // the block's 1x1/2 branch on the centre tap (pgemm_branch_kernel)
                p.wgt2 = C2->ds.wgt;
                p.out2 = buf_at(C2->ds.out, crop0 * out_crop, bf);
                pe = launch_pgemm(p, 64, s);
                branch_left = pe != hipSuccess;
                p.wgt2 = nullptr;
                p.out2 = nullptr;
            }
            if (P.form == CONV_PGEMM && pe == hipErrorInvalidValue) pe = launch_pgemm(p, P.pgemm_bm, s);
            if (pe == hipErrorInvalidValue) pe = launch_igemm(p, P.tile, s);  // geometry the patch kernel / the persistent GEMM does not cover
        }
        HIPCHK(e, pe);
    }
    // the opener ran unfused: the branch GEMM behind it, booked where conv2 books it (its layer's row, or the family's)
    if (branch_left) return run_branch_gemm(e, *C2, P.branch_gemm, crop0, ncrops, slab_off, s, e->knobs.profile_layers ? C2->name.c_str() : prof_name);
    return PA_OK;
}

// stop: the last trace stage to run (pa_backbone_trace: 1 = stem + pool, 2..17 = convs[1..16], 18 = avgpool); anything
// larger runs the whole backbone
int run_backbone_part(pa_engine* e, int crop0, int ncrops, const float* x_in, float* feats_out, size_t slab_off, hipStream_t s,
                      int stop = PA_TRACE_STAGES) {
    int rc;
    ConvLayer stem = e->convs[0];
    stem.in = const_cast<float*>(x_in);  // x_in / feats_out are the caller's bases: crop0 is applied by run_conv
    const EngineKnobs& K = e->knobs;
    auto stem_part = [&](int c0, int n, hipStream_t st) -> int {
        if (K.stem_igemm && !e->bf16) return run_conv(e, stem, c0, n, slab_off, st, "igemm_conv7x7_stem");
        StemParams sp;
        memset(&sp, 0, sizeof(sp));
        sp.x = x_in + (size_t)c0 * 134 * 134 * 4;
        sp.wgt = stem.wgt;
        sp.bias = stem.bias;
        sp.out = reinterpret_cast<float*>(reinterpret_cast<char*>(e->c1) + (size_t)c0 * 66 * 66 * 64 * (e->bf16 ? 2 : 4));
        sp.tiles = n * 32;
        sp.out_bf16 = e->bf16 ? 1 : 0;
        const double px = (double)n * 64 * 64;
        ProfScope ps(e, st, "stem_conv7x7", 2.0 * px * 64 * 147, 4.0 * ((double)n * 128 * 128 * 3 + px * 64 + 64.0 * 147));
        HIPCHK(e, launch_stem7x7(sp, st));
        return PA_OK;
    };
    auto pool_part = [&](int c0, int n, hipStream_t st) -> int {
        ProfScope ps(e, st, "maxpool3x3", 0.0, (e->bf16 ? 2.0 : 4.0) * n * (64.0 * 64 * 64 + 32.0 * 32 * 64));
        if (e->bf16)
            HIPCHK(e, launch_maxpool_bf16(reinterpret_cast<uint16_t*>(e->c1) + (size_t)c0 * 66 * 66 * 64,
                                          reinterpret_cast<uint16_t*>(e->p1) + (size_t)c0 * 34 * 34 * 64, n, st));
        else
            HIPCHK(e, launch_maxpool(e->c1 + (size_t)c0 * 66 * 66 * 64, e->p1 + (size_t)c0 * 34 * 34 * 64, n, st));
        return PA_OK;
    };
    // Default: stem + BatchNorm + ReLU + max-pool in one persistent kernel (stem_pool.hip), the 64 x 64 stem map never
    // reaches memory. PA_STEM_POOL=0 keeps the two-kernel form for A/B runs: there the max-pool (pure HBM/L2
    // streaming) of one half batch runs on the side stream underneath the stem (pure matrix work) of the other.
    const int x_form = input_form(e, x_in);
    if (engine_forms(K, e->dtype).stem_fused) {
        StemPoolParams sp;
        memset(&sp, 0, sizeof(sp));
        const size_t es_in = x_form ? 2 : 4, es_out = e->bf16 ? 2 : 4;   // (integer pixels: 2-byte input, fp32 output)
        sp.x = reinterpret_cast<const char*>(x_in) + (size_t)crop0 * 134 * 134 * 4 * es_in;
        sp.wgt = x_form == 2 ? (const void*)e->stem_wgt_int : e->bf16 ? (const void*)e->stem_wgt_bf16 : (const void*)stem.wgt;
        sp.bias = stem.bias;
        sp.out = reinterpret_cast<char*>(e->p1) + (size_t)crop0 * 34 * 34 * 64 * es_out;
        sp.crops = ncrops;
        sp.in_bf16 = x_form;
        sp.out_bf16 = e->bf16 ? 1 : 0;
        const double px = (double)ncrops * 64 * 64;
        ProfScope ps(e, s, "stem_conv7x7_pool", 2.0 * px * 64 * 147,
                     (double)es_in * ((double)ncrops * 128 * 128 * 4 + 64.0 * 147 * (x_form == 2 ? 3 : 1)) + (double)es_out * ncrops * 32 * 32 * 64);
        HIPCHK(e, launch_stem_pool(sp, s));
    } else if (x_form == 2) {
        return fail(e, PA_ERR_INVALID_ARG, "integer pixels reached an unfused stem (PA_STEM_POOL=0 / PA_STEM_IGEMM=1 switch the integer stem off)");
    } else if (e->bf16) {
        return fail(e, PA_ERR_INVALID_ARG, "the bf16 path has no unfused stem (PA_STEM_POOL=0 / PA_STEM_IGEMM=1 are fp32 A/B knobs)");
    } else if (K.pool_overlap && !e->profiling && !K.interleave && e->side && s != e->side && ncrops >= 64) {
        const int half = (ncrops / 2 + 7) & ~7;
        if ((rc = stem_part(crop0, half, s))) return rc;
        HIPCHK(e, hipEventRecord(e->ev_fork, s));
        HIPCHK(e, hipStreamWaitEvent(e->side, e->ev_fork, 0));
        if ((rc = pool_part(crop0, half, e->side))) return rc;
        HIPCHK(e, hipEventRecord(e->ev_join, e->side));
        if ((rc = stem_part(crop0 + half, ncrops - half, s))) return rc;
        if ((rc = pool_part(crop0 + half, ncrops - half, s))) return rc;
        HIPCHK(e, hipStreamWaitEvent(s, e->ev_join, 0));
    } else {
        if ((rc = stem_part(crop0, ncrops, s))) return rc;
        if ((rc = pool_part(crop0, ncrops, s))) return rc;
    }
    if (stop <= 1) return PA_OK;
    const bool on_side = branch_on_side(e, s);  // a branch GEMM of its own goes to the side stream, in front of its block's opener
    for (size_t i = 1; i < e->convs.size(); ++i) {
        const ConvLayer& L = e->convs[i];
        const char* pn = K.profile_layers ? L.name.c_str() : (L.kh == 3 ? "igemm_conv3x3" : "igemm_conv1x1_ds");
        const bool side_next = on_side && i + 1 < e->convs.size() && e->convs[i + 1].branch.place == BRANCH_OWN_GEMM;  // L is such an opener
        if (side_next) {
            const ConvLayer& Nx = e->convs[i + 1];
            HIPCHK(e, hipEventRecord(e->ev_ds_fork, s));
            HIPCHK(e, hipStreamWaitEvent(e->side, e->ev_ds_fork, 0));
            if ((rc = run_branch_gemm(e, Nx, plan_branch(e->dtype, Nx, ncrops), crop0, ncrops, slab_off, e->side, "igemm_conv1x1_ds"))) return rc;
            HIPCHK(e, hipEventRecord(e->ev_ds_join, e->side));
        }
        if (on_side && L.branch.place == BRANCH_OWN_GEMM) HIPCHK(e, hipStreamWaitEvent(s, e->ev_ds_join, 0));  // (plan_conv: the branch is stored)
        if ((rc = run_conv(e, L, crop0, ncrops, slab_off, s, pn))) return rc;
        if (stop <= (int)i + 1) {
            if (side_next) HIPCHK(e, hipStreamWaitEvent(s, e->ev_ds_join, 0));  // no side-stream work outlives the call
            return PA_OK;
        }
    }
    {
        ProfScope ps(e, s, "avgpool", 0.0, ncrops * ((e->bf16 ? 2.0 : 4.0) * 16.0 * 512 + 4.0 * 512));
        if (e->bf16)
            HIPCHK(e, launch_avgpool_bf16(reinterpret_cast<uint16_t*>(e->layer4_out) + (size_t)crop0 * 36 * 512,
                                          e->pooled + (size_t)crop0 * 512, ncrops, s));
        else
            HIPCHK(e, launch_avgpool(e->layer4_out + (size_t)crop0 * 36 * 512, e->pooled + (size_t)crop0 * 512, ncrops, s));
    }
    if (stop <= 18) return PA_OK;
    ConvLayer fc = e->fc;
    fc.out = feats_out;
    rc = run_conv(e, fc, crop0, ncrops, slab_off, s, "igemm_fc");
    return rc;
}

// The backbone of one batch. Large batches are cut into two halves that run on two streams
// (fork/join with events): every layer is then two kernels of half the grid that drift out of
// phase, so the launch gaps, prologues, epilogues and split-K reduces of one half are covered
// by the steady-state MFMA loop of the other (the layers' outside-the-loop time was ~14 %).
int run_backbone(pa_engine* e, int ncrops, const float* x_in, float* feats_out, hipStream_t s, int stop = PA_TRACE_STAGES) {
    if (!e->knobs.interleave || ncrops < 64 || !e->side) return run_backbone_part(e, 0, ncrops, x_in, feats_out, 0, s, stop);
    const int half = (ncrops / 2 + 7) & ~7;
    HIPCHK(e, hipEventRecord(e->ev_fork, s));
    HIPCHK(e, hipStreamWaitEvent(e->side, e->ev_fork, 0));
    int rc = run_backbone_part(e, 0, half, x_in, feats_out, 0, s, stop);
    if (rc) return rc;
    rc = run_backbone_part(e, half, ncrops - half, x_in, feats_out, e->slab_floats / 2, e->side, stop);
    if (rc) return rc;
    HIPCHK(e, hipEventRecord(e->ev_join, e->side));
    HIPCHK(e, hipStreamWaitEvent(s, e->ev_join, 0));
    return PA_OK;
}

int run_head(pa_engine* e, int nwin, const float* feats, const int32_t* gather, const int32_t* crop_status,
             pa_record* records, float* logp, hipStream_t s) {
    const int S = e->cfg.sequence_length;
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.act = feats;
    p.wgt = e->w1d;
    p.bias = e->b1d;
    p.out = e->h1;
    p.slab = e->slab;
    p.gather = gather;
    p.M = nwin;
    p.N = 512;
    p.taps = S;
    p.kw_taps = 1;
    p.chunk = PA_FEATURE_STRIDE;
    p.ktot = S * PA_FEATURE_STRIDE;
    p.howo = 1;
    p.wo = 1;
    p.in_px_stride = PA_FEATURE_STRIDE;
    p.out_px_stride = 512;
    p.out_row_stride = 512;
    p.out_img_stride = 512;
    p.relu = 1;
    p.splitk = e->head_splitk;
    if ((size_t)p.splitk * p.M * p.N > e->slab_floats) p.splitk = 1;
    int32_t splitk_used = 1;
    p.defer_reduce = 1;  // the MLP kernel sums the slabs itself
    p.splitk_used = &splitk_used;
    {
        ProfScope ps(e, s, "igemm_conv1d_head", 2.0 * nwin * 512.0 * 1000.0 * S,
                     4.0 * (512.0 * 1000 * S + (double)nwin * S * 1000 + nwin * 512.0));
        HIPCHK(e, launch_igemm(p, e->head_tile, s));
    }
    HeadParams h;
    memset(&h, 0, sizeof(h));
    h.h1 = splitk_used > 1 ? nullptr : e->h1;
    h.slab = e->slab;
    h.b1 = e->b1d;
    h.splitk = splitk_used;
    h.w2 = e->w2;
    h.b2 = e->b2;
    h.w3 = e->w3;
    h.b3 = e->b3;
    h.logp = logp;
    h.records = records;
    h.crop_status = crop_status;
    h.gather = gather;
    h.nwin = nwin;
    h.num_actions = e->cfg.num_actions;
    h.fighters = e->cfg.num_fighters;
    h.seq = S;
    for (int i = 0; i < 4; ++i) h.class_ids[i] = e->cfg.fighter_class_ids[i];
    {
        ProfScope ps(e, s, "head_mlp_logsoftmax", 2.0 * nwin * (512.0 * 128 + 128.0 * e->cfg.num_actions),
                     4.0 * (nwin * 512.0 + 512.0 * 128 + 128.0 * e->cfg.num_actions));
        HIPCHK(e, launch_head_mlp(h, s));
    }
    return PA_OK;
}

int run_preprocess(pa_engine* e, const uint8_t* frames, int n, int height, int width, const double* boxes, int padding,
                   int swap_rb, uint8_t* crops_u8, float* crops_f32, int32_t* status, hipStream_t s,
                   const int32_t* src_frame = nullptr, int n_src = 0, const pa_crop_window* windows = nullptr) {
    PreprocParams p;
    memset(&p, 0, sizeof(p));
    p.frames = frames;
    p.windows = reinterpret_cast<const CropWindow*>(windows);
    p.boxes = boxes;
    p.src_frame = src_frame;
    p.n_src = src_frame ? n_src : n;
    p.n_frames = n;
    p.height = height;
    p.width = width;
    p.fighters = e->cfg.num_fighters;
    p.padding = padding;
    p.swap_rb = swap_rb;
    p.plans = e->plans;
    p.coef = e->coef;
    p.coef_dim = e->coef_dim;
    // the cache holds the reference's padding (30); any other value computes its tables per crop, as every clipped crop does
    p.coef_cache = e->coef_cache_pad == padding ? e->coef_cache : nullptr;
    p.coef_cache_pad = padding;
    p.coef_cache_dmax = e->coef_cache_dmax;
    p.area_tabs = e->area_tabs;
    p.hop = e->hop;
    p.t1 = e->t1;
    p.t2 = e->t2;
    p.t_stride = e->t_stride;
    p.crops_u8 = crops_u8;
    p.crops_f32 = crops_f32;
    p.crops_f32_is_bf16 = input_form(e, crops_f32);
    p.status = status;
    p.fallback_count = e->fallback;
    p.fallback_list = e->fallback + 4;
    const double ncrops = (double)n * e->cfg.num_fighters;
    ProfScope ps(e, s, "preprocess_crops", 0.0, ncrops * (375.0 * 375 * 3 + 49152.0 * 5));
    if (e->jpeg_quality > 0 && !p.crops_u8) p.crops_u8 = e->crops_tmp;   // the round trip works on the u8 crops
    HIPCHK(e, launch_preprocess(p, s));
    if (e->jpeg_quality > 0) {
        JpegParams j;
        memset(&j, 0, sizeof(j));
        j.crops_u8 = p.crops_u8;
        j.qtab = e->jpeg_qtab;
        j.x0 = crops_f32;
        j.x0_bf16 = input_form(e, crops_f32);
        j.bgr = swap_rb ? 0 : 1;   // frames are B, G, R; swap_rb turns the crops into R, G, B
        ProfScope pj(e, s, "jpeg_roundtrip", 0.0, ncrops * 49152.0 * 2);
        HIPCHK(e, launch_jpeg_roundtrip(j, (int)ncrops, s));
    }
    return PA_OK;
}

}  // namespace

// ===============================================================================
// C ABI
// ===============================================================================

extern "C" {

int pa_abi_version(void) { return PA_ABI_VERSION; }

const char* pa_status_string(int status) {
    switch (status) {
        case PA_OK: return "ok";
        case PA_ERR_INVALID_ARG: return "invalid argument";
        case PA_ERR_HIP: return "HIP runtime error";
        case PA_ERR_BAD_WEIGHTS: return "weight blob does not match the expected layout";
        case PA_ERR_CAPACITY: return "request exceeds the capacity the engine was created with";
        case PA_ERR_NO_DEVICE: return "no usable HIP device";
        case PA_ERR_NOT_READY: return "features of a required frame are not in the cache";
        case PA_ERR_BAD_LABELS: return "labels outside [0, num_actions) were skipped";
        default: return "unknown status";
    }
}

const char* pa_last_error(const pa_engine* e) { return e ? e->last_error.c_str() : "null engine"; }

// (the blob is the same for every knob, dtype and batch: any table counts it)
size_t pa_weight_blob_bytes(int S, int A) { return 8 * sizeof(int32_t) + blob_floats(engine_table(EngineKnobs(), DT_F32, 1), S, A) * sizeof(float); }

}  // extern "C"

namespace {

// ---- the steps of create_impl, in its order ------------------------------------------------------------------------------------

#define ALLOC(ptr, count, zero)                                                     \
    do {                                                                            \
        if (int rc__ = dev_alloc(e, &(ptr), (size_t)(count), zero)) return rc__;    \
    } while (0)

int check_create_args(const pa_config* cfg, const void* blob, size_t src_bytes, const void* arena_dev, pa_engine** out) {
    if (!cfg || (!blob && !arena_dev) || !out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->abi_version != PA_ABI_VERSION) return PA_ERR_INVALID_ARG;
    const int S = cfg->sequence_length, A = cfg->num_actions, F = cfg->num_fighters;
    if (S < 1 || S % 2 == 0 || S > 15 || A < 1 || A > 64 || F < 1 || F > 4 || cfg->max_batch_frames < 1 ||
        cfg->max_clip_frames < 1 || cfg->max_frame_height < 1 || cfg->max_frame_width < 1 || cfg->crop_padding < 0 ||
        (cfg->compute_dtype != PA_DTYPE_F32 && cfg->compute_dtype != PA_DTYPE_BF16 && cfg->compute_dtype != PA_DTYPE_EMULATED_F32))
        return PA_ERR_INVALID_ARG;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(blob);
    if (blob && (src_bytes != pa_weight_blob_bytes(S, A) || hdr[0] != PA_WEIGHT_MAGIC || hdr[1] != 1 || hdr[2] != S || hdr[3] != A))
        return PA_ERR_BAD_WEIGHTS;
    return PA_OK;
}

int select_device(pa_engine* e) {
    int ndev = 0;
    const hipError_t derr = hipGetDeviceCount(&ndev);
    if (derr != hipSuccess || ndev <= 0 || e->cfg.device_id < 0 || e->cfg.device_id >= ndev)
        return fail(e, PA_ERR_NO_DEVICE,
                    std::string("hipGetDeviceCount: ") + hipGetErrorString(derr) + ", devices=" + std::to_string(ndev) +
                        ", requested device " + std::to_string(e->cfg.device_id));
    HIPCHK(e, hipSetDevice(e->cfg.device_id));
    HIPCHK(e, preprocess_init_device());
    return PA_OK;
}

// model input, stem and pool outputs, features, cache and the small per-crop tables (the layers' own buffers: wire_layers)
int alloc_activations(pa_engine* e) {
    const int NC = e->max_crops;
    ALLOC(e->x0_slot[0], (size_t)NC * 134 * 134 * 4, true);
    ALLOC(e->x0_slot[1], (size_t)NC * 134 * 134 * 4, true);
    e->x0 = e->x0_slot[0];
    // PA_STEM_INT=0: every producer writes k / 255 and the fp32 stem runs, as before the integer form (A/B runs). The unfused stems
    // of PA_STEM_POOL=0 / PA_STEM_IGEMM=1 have no integer form and switch it off too.
    e->stem_int = engine_forms(e->knobs, e->dtype).stem_int;
    if (e->stem_int) {
        ALLOC(e->xi_slot[0], (size_t)NC * 134 * 134 * 4, true);
        ALLOC(e->xi_slot[1], (size_t)NC * 134 * 134 * 4, true);
    }
    ALLOC(e->savebox_rects, (size_t)NC * 4, true);
    ALLOC(e->pre_status[0], (size_t)NC, true);
    ALLOC(e->pre_status[1], (size_t)NC, true);
    ALLOC(e->c1, (size_t)NC * 66 * 66 * 64, true);
    ALLOC(e->p1, (size_t)NC * 34 * 34 * 64, true);
    ALLOC(e->pooled, (size_t)NC * 512, true);
    ALLOC(e->feats_tmp, (size_t)NC * PA_FEATURE_STRIDE, true);
    ALLOC(e->jpeg_qtab, 128, true);
    ALLOC(e->crops_tmp, (size_t)NC * PA_CROP * PA_CROP * 3, true);
    ALLOC(e->cache, (size_t)e->cache_rows * PA_FEATURE_STRIDE, true);
    ALLOC(e->cache_status, (size_t)e->cache_rows, true);
    ALLOC(e->h1, (size_t)NC * 512, true);
    ALLOC(e->gather, (size_t)NC * e->cfg.sequence_length, true);
    ALLOC(e->status_tmp, (size_t)NC, true);
    ALLOC(e->dev_errors, 4, true);
    // scratch of pa_clean_detections, sized for the longest clip and the widest detection table (max_det <= 8): the enqueue-only
    // call never allocates for a table the engine was made for (a longer one still grows it, behind a device synchronisation)
    e->clean_g6_cap = (size_t)e->cfg.max_clip_frames * 8 * 6;
    ALLOC(e->clean_g6, e->clean_g6_cap, false);
    return PA_OK;
}

// The weight arena, and in fold mode its zeroed host mirror. Capacity: the folded tensors are the blob's plus zero padding (stem K
// 147 -> 224, fc and Conv1d 1000 -> 1024) and 256-byte alignment per tensor; 1.25x + 1 MiB covers every (S, A)
// (+ 16 / 9 of the 3x3 filters once more: the Winograd layout of the fp32 stride-1 3x3 layers, kept beside the direct one)
// (+ 36 / 9 of layer 4's three stride-1 filters where F(4x4, 3x3) taken apart can engage: engine_plan.h's wino4_layer)
int alloc_arena(pa_engine* e, bool fold) {
    const EngineKnobs& K = e->knobs;
    e->arena_cap = pa_weight_blob_bytes(e->cfg.sequence_length, e->cfg.num_actions) / 4 * 13 + (1u << 20);
    if (e->dtype != DT_BF16 && K.wino && K.wino_f4 && e->max_crops >= K.wino_f4_min) e->arena_cap += 3 * (wino4_weight_floats(512, 512) * sizeof(float) + 256);
    void* ar = nullptr;
    HIPCHK(e, hipMalloc(&ar, e->arena_cap));
    e->allocs.push_back(ar);
    e->arena = reinterpret_cast<uint8_t*>(ar);
    if (fold) e->arena_stage.assign(e->arena_cap, 0);
    return PA_OK;
}

// The table's rows (engine_table.h) as pa_engine::convs / fc, each with its buffers: per layer three zero-bordered activation
// buffers the four convs rotate through, and the stored 1x1/2 branch where block-0 conv2 adds one
int wire_layers(pa_engine* e, const std::vector<TableRow>& rows) {
    for (const TableRow& r : rows) {
        ConvLayer L;
        static_cast<LayerDesc&>(L) = r.d;
        L.name = r.name;
        L.carries_of = r.carries_of;
        if (r.kind == ROW_FC) e->fc = L;
        else e->convs.push_back(L);
    }
    e->convs[0].in = e->x0;
    e->convs[0].out = e->c1;
    float* cur = e->p1;
    for (int li = 0; li < 4; ++li) {
        ConvLayer* c = &e->convs[1 + 4 * li];  // conv1, conv2 of block 0; conv1, conv2 of block 1
        const size_t buf = (size_t)e->max_crops * (c[0].out_hw + 2) * (c[0].out_hw + 2) * c[0].cout;
        float *mid, *outA, *outB;
        ALLOC(mid, buf, true);
        ALLOC(outA, buf, true);
        ALLOC(outB, buf, true);
        c[0].in = cur; c[0].out = mid;
        c[1].in = mid; c[1].out = outA;
        if (rows[2 + 4 * li].kind == ROW_CONV2_DS) {
            c[1].ds.src = cur;
            if (c[1].branch.place != BRANCH_SECOND_K) ALLOC(c[1].ds.out, buf, true);
        } else {
            c[1].residual = cur;
        }
        c[2].in = outA; c[2].out = mid;
        c[3].in = mid; c[3].out = outB; c[3].residual = outA;
        cur = outB;
    }
    e->layer4_out = cur;
    e->fc.in = e->pooled;
    return PA_OK;
}

// The arena entries of one conv row, in the arena's order; br: fold mode, the blob at this row (nullptr: adopt mode, sizes only)
int place_conv(pa_engine* e, ConvLayer& L, RowKind kind, BlobReader* br) {
    const int cin = L.cin, co = L.cout, ktot = L.taps * L.chunk, cb = L.branch.c;
    const bool ds = kind == ROW_CONV2_DS, bf = e->bf16 && L.kh == 3;
    std::vector<float> w, b, wd, bd;  // fold mode: the conv, and the 1x1/2 downsample behind it, BatchNorm folded
    if (br && !fold_conv(*br, L, w, b)) return fail(e, PA_ERR_BAD_WEIGHTS, "weight blob too short at " + L.name);
    if (br && ds) {
        LayerDesc D;
        D.cin = cb; D.cout = co; D.kh = D.kw = 1; D.taps = 1; D.kw_taps = 1; D.chunk = cb;
        if (!fold_conv(*br, D, wd, bd)) return fail(e, PA_ERR_BAD_WEIGHTS, "weight blob too short at " + L.name.substr(0, L.name.rfind('.')) + ".downsample");
        for (int o = 0; o < co; ++o) b[o] = (float)((double)b[o] + (double)bd[o]);
    }
    int rc;
    float* s;
    if (bf) {   // bf16: the 3x3 alone, the branch always a matrix of its own
        if ((rc = put_bf16(e, &L.wgt, (size_t)co * ktot, w.data()))) return rc;
        if (ds && (rc = put_bf16(e, &L.ds.wgt, (size_t)co * cb, wd.data()))) return rc;
    } else if (ds) {   // [W2 | Wd]: the branch as extra K
        if ((rc = arena_place(e, &L.wgt, (size_t)co * (ktot + cb), &s))) return rc;
        for (int o = 0; s && o < co; ++o) {
            memcpy(s + (size_t)o * (ktot + cb), &w[(size_t)o * ktot], sizeof(float) * ktot);
            memcpy(s + (size_t)o * (ktot + cb) + ktot, &wd[(size_t)o * cb], sizeof(float) * cb);
        }
    } else if ((rc = put(e, &L.wgt, (size_t)co * ktot, w.data()))) {
        return rc;
    }
    if (L.wino) {
        const WinoLayerShape ws = wino_layer_shape(e->knobs, L, e->max_crops);
        L.wino_bn = ws.bn;
        L.wino_shape = ws.shape;
        L.wino_wg = wino_layer_wg(e->knobs, L, e->max_crops);
        if ((rc = arena_place(e, &L.wino_wgt, wino_weight_floats(cin, co), &s))) return rc;
        if (s) wino_transform_weights(w.data(), cin, co, L.wino_bn, s);
        // on a 4 x 4 map once more as the 36 GEMM images of F(4x4, 3x3) taken apart (wino4.hip), beside the F(2x2) image, which serves
        // the batches below the threshold and PA_WINO_F4=0 at run time
        if (L.wino4) {
            if ((rc = arena_place(e, &L.wino4_wgt, wino4_weight_floats(cin, co), &s))) return rc;
            if (s) wino4_transform_weights(w.data(), cin, co, s);
        }
        // block-0 conv2 in Winograd form: the 1x1/2 branch is a small GEMM of its own whose result the 3x3 adds as its residual
        if (ds && (rc = put(e, &L.ds.wgt, (size_t)co * cb, wd.data()))) return rc;
        if (ds && L.branch.split && (rc = put_split(e, &L.ds.split_wgt, wd.data(), co, cb))) return rc;
    }
    if (L.split && (rc = put_split(e, &L.split_wgt, w.data(), co, ktot))) return rc;
    if (e->bf16 && L.kh == 7 && (rc = put_bf16(e, &e->stem_wgt_bf16, (size_t)co * ktot, w.data()))) return rc;
    return put(e, &L.bias, co, b.data());
}

// Every arena entry, in the arena's order: the conv rows, the fc, the temporal head. Each entry's size follows from the table and
// (S, A) and is placed in both modes; only fold mode (br != nullptr) reads the blob and fills the host stage
int place_weights(pa_engine* e, const std::vector<TableRow>& rows, BlobReader* br) {
    const int S = e->cfg.sequence_length, A = e->cfg.num_actions;
    int rc;
    float* s;
    for (size_t i = 0; i < e->convs.size(); ++i)
        if ((rc = place_conv(e, e->convs[i], rows[i].kind, br))) return rc;
    {  // fc 512 -> 1000 (N padded to 1024 with zero rows so cached rows are 1024 wide)
        const float *w = nullptr, *b = nullptr;
        if (br && (!(w = br->take((size_t)1000 * 512)) || !(b = br->take(1000)))) return fail(e, PA_ERR_BAD_WEIGHTS, "weight blob too short at fc");
        if ((rc = put(e, &e->fc.wgt, (size_t)PA_FEATURE_STRIDE * 512, w, (size_t)1000 * 512))) return rc;
        if ((rc = put(e, &e->fc.bias, PA_FEATURE_STRIDE, b, 1000))) return rc;
    }
    {  // Conv1d(1000 -> 512, k=S): [512][1000][S] -> [512][S][1024]
        const float *w = nullptr, *b = nullptr;
        if (br && (!(w = br->take((size_t)512 * 1000 * S)) || !(b = br->take(512)))) return fail(e, PA_ERR_BAD_WEIGHTS, "weight blob too short at cnn1d");
        if ((rc = arena_place(e, &e->w1d, (size_t)512 * S * PA_FEATURE_STRIDE, &s))) return rc;
        for (int o = 0; s && o < 512; ++o)
            for (int c = 0; c < 1000; ++c)
                for (int t = 0; t < S; ++t) s[((size_t)o * S + t) * PA_FEATURE_STRIDE + c] = w[((size_t)o * 1000 + c) * S + t];
        if ((rc = put(e, &e->b1d, 512, b))) return rc;
    }
    {  // head_mlp_kernel reads both matrices k-major (lanes = outputs): w2 -> [512][128], w3 -> [128][64]
        const float *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
        if (br && (!(w2 = br->take(128 * 512)) || !(b2 = br->take(128)) || !(w3 = br->take((size_t)A * 128)) || !(b3 = br->take(A)) || br->pos != br->limit))
            return fail(e, PA_ERR_BAD_WEIGHTS, "weight blob size mismatch at classifier");
        if ((rc = arena_place(e, &e->w2, (size_t)512 * 128, &s))) return rc;
        for (int o = 0; s && o < 128; ++o)
            for (int k = 0; k < 512; ++k) s[(size_t)k * 128 + o] = w2[(size_t)o * 512 + k];
        if ((rc = put(e, &e->b2, 128, b2))) return rc;
        if ((rc = arena_place(e, &e->w3, (size_t)128 * 64, &s))) return rc;
        for (int a = 0; s && a < A; ++a)
            for (int k = 0; k < 128; ++k) s[(size_t)k * 64 + a] = w3[(size_t)a * 128 + k];
        if ((rc = put(e, &e->b3, A, b3))) return rc;
    }
    return PA_OK;
}

// The arena is laid out: one host-to-device copy of the stage (fold mode) or one device copy of the prepared arena (adopt mode)
int load_arena(pa_engine* e, const void* arena_dev, size_t src_bytes) {
    if (arena_dev) {
        if (src_bytes != e->arena_used) return fail(e, PA_ERR_BAD_WEIGHTS, "weight arena size does not match this configuration");
        HIPCHK(e, hipMemcpy(e->arena, arena_dev, e->arena_used, hipMemcpyDeviceToDevice));
    } else {
        HIPCHK(e, hipMemcpy(e->arena, e->arena_stage.data(), e->arena_used, hipMemcpyHostToDevice));
        std::vector<uint8_t>().swap(e->arena_stage);
    }
    return PA_OK;
}

// The integer stem's three bf16 slices, from the folded fp32 stem weights as they lie in the arena (so a folded and an adopted
// arena give the same slices and the arena keeps its size and layout): s0 = bf16(w), s1 = bf16(w - s0), s2 = bf16(w - s0 - s1),
// round to nearest even each, the splitting of pack_stage_weights
int make_stem_slices(pa_engine* e) {
    if (!e->stem_int) return PA_OK;
    const size_t nw = (size_t)64 * 224;
    std::vector<float> w(nw);
    HIPCHK(e, hipMemcpy(w.data(), e->convs[0].wgt, nw * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<uint16_t> sl(3 * nw);
    for (size_t i = 0; i < nw; ++i) {
        float x = w[i];
        for (int k = 0; k < 3; ++k) {
            const uint16_t hq = bf16_rne(x);
            sl[k * nw + i] = hq;
            const uint32_t u = (uint32_t)hq << 16;
            float f;
            memcpy(&f, &u, 4);
            x -= f;
        }
    }
    ALLOC(e->stem_wgt_int, 3 * nw, false);
    HIPCHK(e, hipMemcpy(e->stem_wgt_int, sl.data(), sl.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return PA_OK;
}

// The split-K slab (engine_table.h's slab_floats), the Winograd kernel's tickets -- one per tile -- and V and M of F(4x4, 3x3)
// taken apart (wino4.hip)
int alloc_slab(pa_engine* e, const std::vector<TableRow>& rows) {
    bool any_wino = false;
    for (const ConvLayer& L : e->convs) {
        any_wino = any_wino || L.wino;
        if (L.wino4) e->wino4_region = std::max(e->wino4_region, (size_t)36 * wino4_rows(e->max_crops) * (L.cin + L.cout));
    }
    if (any_wino) ALLOC(e->wino_tickets, (size_t)2 * WINO_TICKETS, true);
    if (e->wino4_region) ALLOC(e->wino4_scratch, e->wino4_region * (e->knobs.interleave ? 2 : 1), false);
    e->slab_floats = slab_floats(rows, e->knobs, e->max_crops, e->cfg.sequence_length);
    ALLOC(e->slab, e->slab_floats, false);
    return PA_OK;
}

int alloc_crop_scratch(pa_engine* e) {
    const pa_config* cfg = &e->cfg;
    const int NC = e->max_crops;
    e->coef_dim = std::max(cfg->max_frame_height, cfg->max_frame_width);
    // per-crop scratch of the resamplers: a whole frame slice, and at least the runner-input branch's worst
    // case (INTER_AREA result of 448 rows + the 128 rows behind the vertical pass, 128 px x 3 B each)
    e->t_stride = std::max((size_t)cfg->max_frame_height * cfg->max_frame_width * 3, (size_t)(448 + 128) * PA_CROP * 3);
    ALLOC(e->plans, (size_t)NC, true);
    ALLOC(e->fallback, (size_t)NC + 4, true);
    ALLOC(e->coef, (size_t)NC * 2 * e->coef_dim * (2 + PA_KSIZE_MAX), false);
    // a crop side cannot exceed the shorter frame side without being clipped (and then it is not a cached pair); 1024 caps the
    // cache at 36 MB
    e->coef_cache_dmax = std::min(std::min(cfg->max_frame_height, cfg->max_frame_width), 1024);
    ALLOC(e->coef_cache, coef_cache_ints(e->coef_cache_dmax), false);
    e->coef_cache_pad = 30;  // the one padding the reference's runner passes (ai_runner.py:418)
    HIPCHK(e, launch_build_coef_cache(e->coef_cache, e->coef_cache_pad, e->coef_cache_dmax, nullptr));
    ALLOC(e->area_tabs, (size_t)NC * 2 * PA_CROP, true);
    ALLOC(e->hop, (size_t)NC * PA_HOP_BLOCKS_MAX * PA_HOP_BLOCK_BYTES, true);  // 302 KB a crop
    ALLOC(e->t1, (size_t)NC * e->t_stride, false);
    ALLOC(e->t2, (size_t)NC * e->t_stride, false);
    AugmentTables at;
    augment_tables_host(&at);
    ALLOC(e->aug_tabs, (size_t)1, false);
    HIPCHK(e, hipMemcpy(e->aug_tabs, &at, sizeof(at), hipMemcpyHostToDevice));
    return PA_OK;
}
#undef ALLOC

int create_streams(pa_engine* e) {
    HIPCHK(e, hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
    HIPCHK(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    HIPCHK(e, hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    HIPCHK(e, hipEventCreateWithFlags(&e->ev_ds_fork, hipEventDisableTiming));
    HIPCHK(e, hipEventCreateWithFlags(&e->ev_ds_join, hipEventDisableTiming));
    HIPCHK(e, hipDeviceSynchronize());
    return PA_OK;
}

// pa_create (blob != nullptr: fold the Lightning tensors) and pa_create_from_arena (arena_dev != nullptr:
// adopt a prepared weight arena of `src_bytes` bytes) share everything but the source of the weights.
int create_impl(const pa_config* cfg, const void* blob, size_t src_bytes, const void* arena_dev, pa_engine** out) {
    int rc = check_create_args(cfg, blob, src_bytes, arena_dev, out);
    if (rc) return rc;
    pa_engine* e = new pa_engine();
    e->cfg = *cfg;
    e->bf16 = cfg->compute_dtype == PA_DTYPE_BF16;
    e->emu = cfg->compute_dtype == PA_DTYPE_EMULATED_F32;
    e->dtype = e->bf16 ? DT_BF16 : e->emu ? DT_EMULATED_F32 : DT_F32;
    e->knobs = engine_knobs();  // the per-create knobs as the environment has them now
    e->max_crops = cfg->max_batch_frames * cfg->num_fighters;
    e->cache_rows = cfg->max_clip_frames * cfg->num_fighters;
    *out = e;  // handed back even on failure so the caller can read pa_last_error, then pa_destroy
    const std::vector<TableRow> rows = engine_table(e->knobs, e->dtype, e->max_crops);
    if ((rc = select_device(e))) return rc;
    if ((rc = alloc_activations(e))) return rc;
    if ((rc = alloc_arena(e, blob != nullptr))) return rc;
    if ((rc = wire_layers(e, rows))) return rc;
    head_plan(e->knobs, e->max_crops, cfg->sequence_length, &e->head_tile, &e->head_splitk);
    if (blob) {   // fold: the tensors behind the blob's header, all of them
        BlobReader br{reinterpret_cast<const float*>(blob) + 8, 0, blob_floats(rows, cfg->sequence_length, cfg->num_actions)};
        rc = place_weights(e, rows, &br);
    } else {
        rc = place_weights(e, rows, nullptr);
    }
    if (rc) return rc;
    if ((rc = load_arena(e, arena_dev, src_bytes))) return rc;
    if ((rc = make_stem_slices(e))) return rc;
    if ((rc = alloc_slab(e, rows))) return rc;
    if ((rc = alloc_crop_scratch(e))) return rc;
    return create_streams(e);
}

}  // namespace

extern "C" {

int pa_create(const pa_config* cfg, const void* blob, size_t blob_bytes, pa_engine** out) {
    if (!blob) return PA_ERR_INVALID_ARG;
    return create_impl(cfg, blob, blob_bytes, nullptr, out);
}

int pa_create_from_arena(const pa_config* cfg, const void* arena_dev, size_t arena_bytes, pa_engine** out) {
    if (!arena_dev) return PA_ERR_INVALID_ARG;
    return create_impl(cfg, nullptr, arena_bytes, arena_dev, out);
}

size_t pa_weights_arena_bytes(const pa_engine* e) { return e ? e->arena_used : 0; }

int pa_weights_export(pa_engine* e, void* dst_dev, size_t bytes, void* stream) {
    if (!e || !dst_dev || bytes != e->arena_used) return fail(e, PA_ERR_INVALID_ARG, "pa_weights_export: size must be pa_weights_arena_bytes()");
    HIPCHK(e, hipMemcpyAsync(dst_dev, e->arena, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PA_OK;
}

void pa_destroy(pa_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->cfg.device_id);
    (void)hipDeviceSynchronize();
    for (ProfEntry& p : e->prof_log) {
        (void)hipEventDestroy(p.start);
        (void)hipEventDestroy(p.stop);
    }
    for (hipEvent_t ev : e->event_pool) (void)hipEventDestroy(ev);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->ev_ds_fork) (void)hipEventDestroy(e->ev_ds_fork);
    if (e->ev_ds_join) (void)hipEventDestroy(e->ev_ds_join);
    if (e->side) (void)hipStreamDestroy(e->side);
    if (e->gate_flag) (void)hipHostFree(e->gate_flag);
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
}

int pa_infer_windows(pa_engine* e, const float* x, int32_t batch, float* logp, void* stream) {
    if (!e || !x || !logp || batch < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_infer_windows: bad argument");
    const int S = e->cfg.sequence_length;
    hipStream_t s = (hipStream_t)stream;
    // the backbone scratch holds max_crops crops: run the windows in groups
    const int win_per_pass = e->max_crops / S;
    if (win_per_pass < 1) return fail(e, PA_ERR_CAPACITY, "pa_infer_windows: engine smaller than one window");
    for (int w0 = 0; w0 < batch; w0 += win_per_pass) {
        const int nw = std::min(win_per_pass, batch - w0);
        const int ncrops = nw * S;
        {
            ProfScope ps(e, s, "nchw_to_nhwc4", 0.0, ncrops * (49152.0 * 4 + 134.0 * 134 * 16));
            HIPCHK(e, launch_nchw_to_padded(x + (size_t)w0 * S * 3 * 128 * 128, e->x0, ncrops, e->bf16 ? 1 : 0, s));
        }
        int rc = run_backbone(e, ncrops, e->x0, e->feats_tmp, s);
        if (rc) return rc;
        HIPCHK(e, launch_identity_gather(e->gather, ncrops, s));
        e->gather_key[0] = -1;  // the clip head's cached window table is gone
        rc = run_head(e, nw, e->feats_tmp, e->gather, nullptr, nullptr, logp + (size_t)w0 * e->cfg.num_actions, s);
        if (rc) return rc;
    }
    return PA_OK;
}

int pa_backbone_windows(pa_engine* e, const float* x, int32_t n_crops, float* feats, void* stream) {
    if (!e || !x || !feats || n_crops < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_windows: bad argument");
    hipStream_t s = (hipStream_t)stream;
    for (int c0 = 0; c0 < n_crops; c0 += e->max_crops) {  // the backbone scratch holds max_crops crops
        const int n = std::min(e->max_crops, n_crops - c0);
        {
            ProfScope ps(e, s, "nchw_to_nhwc4", 0.0, n * (49152.0 * 4 + 134.0 * 134 * 16));
            HIPCHK(e, launch_nchw_to_padded(x + (size_t)c0 * 3 * 128 * 128, e->x0, n, e->bf16 ? 1 : 0, s));
        }
        const int rc = run_backbone(e, n, e->x0, feats + (size_t)c0 * PA_FEATURE_STRIDE, s);
        if (rc) return rc;
    }
    return PA_OK;
}

int pa_backbone_trace(pa_engine* e, const float* x, int32_t n_crops, int32_t stage, void* out, size_t out_bytes, void* aux,
                      size_t aux_bytes, void* stream) {
    if (!e || !x || !out) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: bad argument");
    if (stage < 0 || stage >= PA_TRACE_STAGES) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: stage out of range");
    if (n_crops < 1 || n_crops > e->max_crops) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: n_crops outside 1..max_crops");
    if (e->convs.size() != 17) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: unexpected layer table");
    const size_t n = (size_t)n_crops, es = e->bf16 ? 2 : 4;  // storage element of the stem and the 3x3 stack
    const void* src;
    const void* aux_src = nullptr;
    size_t bytes;
    bool has_branch = false;
    if (stage == 0) {
        src = e->x0;
        bytes = n * 134 * 134 * 4 * es;
    } else if (stage == 1) {
        src = e->p1;
        bytes = n * 34 * 34 * 64 * es;
    } else if (stage <= 17) {
        const ConvLayer& L = e->convs[stage - 1];
        const size_t w = (size_t)L.out_hw + 2 * L.out_pad;
        src = L.out;
        bytes = n * w * w * L.cout * es;
        has_branch = L.branch.place != BRANCH_NONE;
        aux_src = L.ds.out;
    } else if (stage == 18) {
        src = e->pooled;
        bytes = n * 512 * sizeof(float);
    } else {
        src = e->feats_tmp;
        bytes = n * PA_FEATURE_STRIDE * sizeof(float);
    }
    if (out_bytes < bytes) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: out is smaller than the stage");
    if (has_branch && aux) {
        if (!aux_src) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: this stage stores no downsample branch");
        if (aux_bytes < bytes) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_trace: aux is smaller than the stage");
    }
    hipStream_t s = (hipStream_t)stream;
    // what pa_backbone_windows enqueues for one chunk of n_crops, cut short after `stage`
    HIPCHK(e, launch_nchw_to_padded(x, e->x0, n_crops, e->bf16 ? 1 : 0, s));
    if (stage > 0) {
        const int rc = run_backbone(e, n_crops, e->x0, e->feats_tmp, s, stage);
        if (rc) return rc;
    }
    HIPCHK(e, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, s));
    if (has_branch && aux) HIPCHK(e, hipMemcpyAsync(aux, aux_src, bytes, hipMemcpyDeviceToDevice, s));
    return PA_OK;
}

int pa_crop_resize_width(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const int32_t* rects_host,
                         int32_t n_rects, int32_t out_w, uint8_t* out, int32_t out_h_cap, int32_t* out_h_host, void* stream) {
    if (!e || !frames || !rects_host || !out || !out_h_host || n < 1 || height < 1 || width < 1 || n_rects < 1 || n_rects > 4 || out_w < 1 ||
        out_h_cap < 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_crop_resize_width: bad argument");
    RectResizeParams q;
    memset(&q, 0, sizeof(q));
    q.frames = frames;
    q.height = height;
    q.width = width;
    q.n_rects = n_rects;
    q.out_w = out_w;
    q.out_h_cap = out_h_cap;
    q.out = out;
    for (int r = 0; r < n_rects; ++r) {
        const int x1 = rects_host[4 * r], y1 = rects_host[4 * r + 1], x2 = rects_host[4 * r + 2], y2 = rects_host[4 * r + 3];
        if (x1 < 0 || y1 < 0 || x2 > width || y2 > height || x2 <= x1 || y2 <= y1)
            return fail(e, PA_ERR_INVALID_ARG, "pa_crop_resize_width: empty rectangle or outside the frame (cv2.resize raises on an empty image)");
        // imutils.resize: r = width / float(w); dim = (width, int(h * r))
        const double ratio = (double)out_w / (double)(x2 - x1);
        const int oh = (int)((double)(y2 - y1) * ratio);
        if (oh < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_crop_resize_width: destination height 0");
        if (oh > out_h_cap) return fail(e, PA_ERR_CAPACITY, "pa_crop_resize_width: out_h_cap too small");
        q.x1[r] = x1; q.y1[r] = y1; q.x2[r] = x2; q.y2[r] = y2;
        q.out_h[r] = oh;
        out_h_host[r] = oh;
    }
    HIPCHK(e, launch_rect_resize(q, n, (hipStream_t)stream));
    return PA_OK;
}

int pa_square_crops(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const double* boxes,
                    int32_t padding, int32_t swap_rb, uint8_t* crops, int32_t* status, void* stream) {
    if (!e || !frames || !boxes || !crops || n < 1 || height < 1 || width < 1 || padding < 0)
        return fail(e, PA_ERR_INVALID_ARG, "pa_square_crops: bad argument");
    if (n > e->cfg.max_batch_frames || height > e->cfg.max_frame_height || width > e->cfg.max_frame_width)
        return fail(e, PA_ERR_CAPACITY, "pa_square_crops: frames exceed engine capacity");
    return run_preprocess(e, frames, n, height, width, boxes, padding, swap_rb, crops, nullptr, status, (hipStream_t)stream);
}

int pa_augment_crops(pa_engine* e, const uint8_t* src_dev, int32_t n_src, const pa_augment_params* params_dev, int32_t n,
                     int32_t out_format, void* out_dev, void* stream) {
    if (!e || !src_dev || !params_dev || !out_dev || n < 1 || n_src < 1 || (out_format != PA_AUGMENT_U8 && out_format != PA_AUGMENT_MODEL))
        return fail(e, PA_ERR_INVALID_ARG, "pa_augment_crops: bad argument");
    if (((uintptr_t)src_dev | (uintptr_t)out_dev) & 15 || (uintptr_t)params_dev & 7)
        return fail(e, PA_ERR_INVALID_ARG, "pa_augment_crops: src and out must be 16-byte aligned, params 8-byte aligned");
    if (!e->aug_tabs) return fail(e, PA_ERR_INVALID_ARG, "pa_augment_crops: the engine has no tables");
    ProfScope ps(e, (hipStream_t)stream, "augment", 0.0, (double)n * 49152.0 * (out_format == PA_AUGMENT_MODEL ? 5.0 : 2.0));
    HIPCHK(e, launch_augment(src_dev, n_src, params_dev, n, out_format, out_dev, e->aug_tabs, (hipStream_t)stream));
    return PA_OK;
}

int pa_square_crops_sized(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const double* boxes,
                          int32_t padding, int32_t swap_rb, int32_t output_size, uint8_t* crops, int32_t* status, void* stream) {
    if (!e || !frames || !boxes || !crops || n < 1 || height < 1 || width < 1 || padding < 0)
        return fail(e, PA_ERR_INVALID_ARG, "pa_square_crops_sized: bad argument");
    if (output_size < PA_CROP_SIZE_MIN || output_size > PA_CROP_SIZE_MAX)
        return fail(e, PA_ERR_INVALID_ARG, "pa_square_crops_sized: output_size outside " + std::to_string(PA_CROP_SIZE_MIN) + ".." + std::to_string(PA_CROP_SIZE_MAX));
    if (n > e->cfg.max_batch_frames || height > e->cfg.max_frame_height || width > e->cfg.max_frame_width)
        return fail(e, PA_ERR_CAPACITY, "pa_square_crops_sized: frames exceed engine capacity");
    // the engine's crop scratch (plans, Pillow tables, the two intermediates) is sized by its frame capacity and serves every
    // output size; the crop JPEG round trip (pa_set_crop_jpeg_quality) is a 128 x 128 stage and does not apply here
    PreprocParams p;
    memset(&p, 0, sizeof(p));
    p.frames = frames;
    p.boxes = boxes;
    p.n_src = n;
    p.n_frames = n;
    p.height = height;
    p.width = width;
    p.fighters = e->cfg.num_fighters;
    p.padding = padding;
    p.swap_rb = swap_rb;
    p.plans = e->plans;
    p.coef = e->coef;
    p.coef_dim = e->coef_dim;
    p.coef_cache = e->coef_cache_pad == padding ? e->coef_cache : nullptr;
    p.coef_cache_pad = padding;
    p.coef_cache_dmax = e->coef_cache_dmax;
    p.t1 = e->t1;
    p.t2 = e->t2;
    p.t_stride = e->t_stride;
    p.crops_u8 = crops;
    p.status = status;
    hipStream_t s = (hipStream_t)stream;
    const double ncrops = (double)n * e->cfg.num_fighters;
    ProfScope ps(e, s, "square_crops_sized", 0.0, ncrops * (375.0 * 375 * 3 * 3 + 3.0 * output_size * output_size));
    HIPCHK(e, launch_crop_sized(p, output_size, s));
    return PA_OK;
}

namespace {
int run_runner_inputs(pa_engine* e, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int n, int swap_rb,
                      uint8_t* inputs_u8, float* inputs_f32, int32_t* status, hipStream_t s) {
    RunnerInParams q;
    memset(&q, 0, sizeof(q));
    q.images = images;
    q.images_bytes = (long long)images_bytes;
    q.desc = reinterpret_cast<const CropImageDesc*>(desc);
    q.n = n;
    q.swap_rb = swap_rb;
    q.max_h = e->cfg.max_frame_height;
    q.max_w = e->cfg.max_frame_width;
    q.t1 = e->t1;
    q.t2 = e->t2;
    q.t_stride = e->t_stride;
    q.inputs_u8 = inputs_u8;
    q.inputs_f32 = inputs_f32;
    q.inputs_f32_is_bf16 = input_form(e, inputs_f32);
    q.status = status;
    ProfScope ps(e, s, "runner_inputs", 0.0, (double)images_bytes + (double)n * 49152.0 * 5);
    HIPCHK(e, launch_runner_inputs(q, s));
    return PA_OK;
}
}  // namespace

int pa_runner_inputs(pa_engine* e, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int32_t n_crops,
                     int32_t swap_rb, uint8_t* inputs_u8, int32_t* status, void* stream) {
    static_assert(sizeof(pa_crop_image) == sizeof(CropImageDesc), "descriptor layouts must agree");
    if (!e || !images || !desc || !inputs_u8 || n_crops < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_runner_inputs: bad argument");
    if (n_crops > e->max_crops) return fail(e, PA_ERR_CAPACITY, "pa_runner_inputs: more crops than max_batch_frames * num_fighters");
    return run_runner_inputs(e, images, images_bytes, desc, n_crops, swap_rb, inputs_u8, nullptr, status, (hipStream_t)stream);
}

int pa_backbone_crop_images(pa_engine* e, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int32_t n,
                            int32_t frame0, uint8_t* crops_rgb, int32_t* status, void* stream) {
    if (!e || !images || !desc || n < 1 || frame0 < 0) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_crop_images: bad argument");
    if (e->clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_crop_images: call pa_clip_begin first");
    if (n > e->cfg.max_batch_frames || frame0 + n > e->clip_frames)
        return fail(e, PA_ERR_CAPACITY, "pa_backbone_crop_images: frames exceed engine / clip capacity");
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    int rc = run_runner_inputs(e, images, images_bytes, desc, n * F, 1, crops_rgb, slot_dst(e, 0), e->pre_status[0], s);
    if (rc) return rc;
    if (status) HIPCHK(e, hipMemcpyAsync(status, e->pre_status[0], sizeof(int32_t) * n * F, hipMemcpyDeviceToDevice, s));
    return pa_backbone_slot(e, 0, n, frame0, stream);
}

namespace {
// The slice of YoloCrop.square_crop (fighter.py:305-343) on the host: the arithmetic of crop_plan_kernel up to the
// numpy slice, so that the window the host uploads is exactly the region the device plan will read.
void host_slice(const double* b, int W, int H, int pad, int* sy0, int* sx0, int* sh, int* sw) {
    *sy0 = *sx0 = *sh = *sw = 0;
    const double v[4] = {b[0] * W, b[1] * H, b[2] * W, b[3] * H};
    int iv[4];
    for (int k = 0; k < 4; ++k) {
        if (!(v[k] > -2.0e9 && v[k] < 2.0e9)) return;
        iv[k] = (int)v[k];
    }
    const int cx = iv[0], cy = iv[1], d = iv[2] > iv[3] ? iv[2] : iv[3];
    if (d <= 0 || d > 16384) return;
    const int half = d / 2;
    auto np_slice = [](int start, int stop, int size, int* s0, int* len) {
        if (start > size) start = size;
        if (stop < 0) {
            stop += size;
            if (stop < 0) stop = 0;
        }
        if (stop > size) stop = size;
        *s0 = start;
        *len = stop > start ? stop - start : 0;
    };
    np_slice(std::max(cy - half - pad, 0), std::min(cy + half + pad, H), H, sy0, sh);
    np_slice(std::max(cx - half - pad, 0), std::min(cx + half + pad, W), W, sx0, sw);
}
}  // namespace

int pa_upload_crop_windows(pa_engine* e, const uint8_t* frames_host, int32_t n, int32_t height, int32_t width,
                           const double* boxes_host, int32_t padding, uint8_t* windows_dev, size_t windows_capacity,
                           pa_crop_window* desc_host, pa_crop_window* desc_dev, size_t* bytes_used, void* stream) {
    static_assert(sizeof(pa_crop_window) == sizeof(CropWindow), "descriptor layouts must agree");
    if (!e || !frames_host || !boxes_host || !windows_dev || !desc_host || !desc_dev || n < 1 || height < 1 || width < 1 || padding < 0)
        return fail(e, PA_ERR_INVALID_ARG, "pa_upload_crop_windows: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    // the upload kernel dereferences frames_host on the device: it must be pinned (device-visible) host memory,
    // a pageable pointer would be a GPU page fault
    for (const void* hp : {(const void*)frames_host, (const void*)(frames_host + (size_t)n * height * width * 3 - 1), (const void*)desc_host}) {
        hipPointerAttribute_t attr;
        const hipError_t pe = hipPointerGetAttributes(&attr, hp);
        if (pe != hipSuccess || (attr.type != hipMemoryTypeHost && attr.type != hipMemoryTypeManaged && attr.type != hipMemoryTypeDevice)) {
            (void)hipGetLastError();
            return fail(e, PA_ERR_INVALID_ARG, "pa_upload_crop_windows: frames_host / desc_host must be pinned host memory (hipHostMalloc, torch pin_memory)");
        }
    }
    size_t off = 0;
    for (int i = 0; i < n * F; ++i) {
        int sy0, sx0, sh, sw;
        host_slice(boxes_host + (size_t)i * 4, width, height, padding, &sy0, &sx0, &sh, &sw);
        pa_crop_window& d = desc_host[i];
        d.offset = (int64_t)off;
        d.row_bytes = sw * 3;
        d.pitch = (sw * 3 + 15) & ~15;
        d.rows = sh;
        d.src_offset = (int64_t)((((size_t)(i / F) * height + sy0) * width + sx0) * 3);
        d.src_pitch = width * 3;
        const size_t bytes = (size_t)sh * d.pitch;
        if (sh == 0 || sw == 0) {  // empty / bad box: the device plan reports it and reads nothing
            d.rows = d.row_bytes = d.pitch = 0;
            continue;
        }
        if (off + bytes + 16 > windows_capacity) return fail(e, PA_ERR_CAPACITY, "pa_upload_crop_windows: window buffer too small");
        off += bytes;
    }
    // descriptors first (tiny, from the caller's pinned array), then ONE kernel that pulls every slice row out of
    // the pinned host frames over PCIe
    HIPCHK(e, hipMemcpyAsync(desc_dev, desc_host, sizeof(pa_crop_window) * n * F, hipMemcpyHostToDevice, s));
    HIPCHK(e, launch_slice_upload(frames_host, (long long)n * height * width * 3, reinterpret_cast<const CropWindow*>(desc_dev), windows_dev,
                                  n * F, s));
    if (bytes_used) *bytes_used = off;
    return PA_OK;
}

int pa_preprocess_windows(pa_engine* e, const uint8_t* windows_dev, const pa_crop_window* desc_dev, int32_t n, int32_t height,
                          int32_t width, const double* boxes, int32_t slot, uint8_t* crops_rgb, int32_t* status, void* stream) {
    if (!e || !windows_dev || !desc_dev || !boxes || n < 1 || height < 1 || width < 1 || slot < 0 || slot > 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_preprocess_windows: bad argument");
    if (n > e->cfg.max_batch_frames || height > e->cfg.max_frame_height || width > e->cfg.max_frame_width)
        return fail(e, PA_ERR_CAPACITY, "pa_preprocess_windows: frames exceed engine capacity");
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    int rc = run_preprocess(e, windows_dev, n, height, width, boxes, e->cfg.crop_padding, 1, crops_rgb, slot_dst(e, slot),
                            e->pre_status[slot], s, nullptr, 0, desc_dev);
    if (rc) return rc;
    if (status) HIPCHK(e, hipMemcpyAsync(status, e->pre_status[slot], sizeof(int32_t) * n * F, hipMemcpyDeviceToDevice, s));
    return PA_OK;
}

int pa_detect_postprocess(pa_engine* e, const float* pred, int32_t n_frames, int32_t rows, int32_t num_classes, float conf_thres,
                          float iou_thres, uint32_t class_mask, int32_t max_det, int32_t net_height, int32_t net_width,
                          int32_t img_height, int32_t img_width, float* dets, int32_t* counts, void* stream) {
    if (!e || !pred || !dets || !counts || n_frames < 1 || rows < 1 || num_classes < 1 || num_classes > 32 || max_det < 1 ||
        max_det > 8 || net_height < 1 || net_width < 1 || img_height < 1 || img_width < 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_detect_postprocess: bad argument");
    DetectParams q;
    memset(&q, 0, sizeof(q));
    q.pred = pred;
    q.n_frames = n_frames; q.rows = rows; q.nc = num_classes; q.max_det = max_det;
    q.conf_thres = conf_thres; q.iou_thres = iou_thres; q.class_mask = class_mask;
    // scale_boxes: gain and pad in double (Python floats), applied as float32 scalars to the float32 boxes
    const double gain = std::min((double)net_height / img_height, (double)net_width / img_width);
    q.gain = (float)gain;
    q.pad_x = (float)(((double)net_width - img_width * gain) / 2.0);
    q.pad_y = (float)(((double)net_height - img_height * gain) / 2.0);
    q.img_w = (float)img_width; q.img_h = (float)img_height;
    q.dets = dets; q.counts = counts;
    ProfScope ps(e, (hipStream_t)stream, "detect_nms", 0.0, (double)n_frames * rows * (5 + num_classes) * 4.0 * max_det);
    HIPCHK(e, launch_detect_nms(q, (hipStream_t)stream));
    return PA_OK;
}

int pa_detect_postprocess_classes(pa_engine* e, const float* pred, int32_t n_frames, int32_t rows, int32_t num_classes, float conf_thres,
                                  float iou_thres, const uint32_t* class_words, int32_t max_det, int32_t net_height, int32_t net_width,
                                  int32_t img_height, int32_t img_width, float* dets, int32_t* counts, void* stream) {
    if (!e || !pred || !dets || !counts || n_frames < 1 || rows < 1 || num_classes < 1 || num_classes > DETECT_MAX_CLASSES || max_det < 1 ||
        max_det > 8 || net_height < 1 || net_width < 1 || img_height < 1 || img_width < 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_detect_postprocess_classes: bad argument");
    DetectParams q;
    memset(&q, 0, sizeof(q));
    q.pred = pred;
    q.n_frames = n_frames; q.rows = rows; q.nc = num_classes; q.max_det = max_det;
    q.conf_thres = conf_thres; q.iou_thres = iou_thres;
    // class_words: ceil(num_classes / 32) words (the bits of classes >= num_classes are ignored); NULL = every class
    for (int w = 0; w < (num_classes + 31) / 32; ++w) q.class_words[w] = class_words ? class_words[w] : 0xffffffffu;
    const double gain = std::min((double)net_height / img_height, (double)net_width / img_width);
    q.gain = (float)gain;
    q.pad_x = (float)(((double)net_width - img_width * gain) / 2.0);
    q.pad_y = (float)(((double)net_height - img_height * gain) / 2.0);
    q.img_w = (float)img_width; q.img_h = (float)img_height;
    q.dets = dets; q.counts = counts;
    ProfScope ps(e, (hipStream_t)stream, "detect_nms_classes", 0.0, (double)n_frames * rows * (5 + num_classes) * 4.0);
    HIPCHK(e, launch_detect_nms_classes(q, (hipStream_t)stream));
    return PA_OK;
}

int pa_project_boxes(pa_engine* e, const double* log_rows, int32_t n_rows, double* boxes, void* stream) {
    if (!e || !log_rows || !boxes || n_rows < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_project_boxes: bad argument");
    HIPCHK(e, launch_project_boxes(log_rows, boxes, n_rows, (hipStream_t)stream));
    return PA_OK;
}

int pa_clip_begin(pa_engine* e, int32_t clip_frames) {
    if (!e || clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_clip_begin: bad argument");
    if (clip_frames > e->cfg.max_clip_frames) return fail(e, PA_ERR_CAPACITY, "pa_clip_begin: clip longer than max_clip_frames");
    e->clip_frames = clip_frames;
    e->sub_frames = 0;
    e->ready.assign(clip_frames, 0);
    return PA_OK;
}

int pa_clip_begin_batch(pa_engine* e, int32_t n_clips, int32_t clip_frames) {
    if (!e || n_clips < 1 || clip_frames < 2) return fail(e, PA_ERR_INVALID_ARG, "pa_clip_begin_batch: bad argument");
    if ((long long)n_clips * clip_frames > e->cfg.max_clip_frames)
        return fail(e, PA_ERR_CAPACITY, "pa_clip_begin_batch: n_clips * clip_frames exceeds max_clip_frames");
    const int rc = pa_clip_begin(e, n_clips * clip_frames);
    if (rc) return rc;
    e->sub_frames = clip_frames;
    return PA_OK;
}

int pa_preprocess_frames(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const double* boxes,
                         int32_t slot, uint8_t* crops_rgb, int32_t* status, void* stream) {
    if (!e || !frames || !boxes || n < 1 || height < 1 || width < 1 || slot < 0 || slot > 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_preprocess_frames: bad argument");
    if (n > e->cfg.max_batch_frames || height > e->cfg.max_frame_height || width > e->cfg.max_frame_width)
        return fail(e, PA_ERR_CAPACITY, "pa_preprocess_frames: frames exceed engine capacity");
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    int rc = run_preprocess(e, frames, n, height, width, boxes, e->cfg.crop_padding, 1, crops_rgb, slot_dst(e, slot),
                            e->pre_status[slot], s);
    if (rc) return rc;
    if (status) HIPCHK(e, hipMemcpyAsync(status, e->pre_status[slot], sizeof(int32_t) * n * F, hipMemcpyDeviceToDevice, s));
    return PA_OK;
}

int pa_backbone_slot(pa_engine* e, int32_t slot, int32_t n, int32_t frame0, void* stream) {
    if (!e || n < 1 || frame0 < 0 || slot < 0 || slot > 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_slot: bad argument");
    if (e->clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_slot: call pa_clip_begin first");
    if (n > e->cfg.max_batch_frames || frame0 + n > e->clip_frames)
        return fail(e, PA_ERR_CAPACITY, "pa_backbone_slot: frames exceed engine / clip capacity");
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    HIPCHK(e, hipMemcpyAsync(e->cache_status + (size_t)frame0 * F, e->pre_status[slot], sizeof(int32_t) * n * F,
                             hipMemcpyDeviceToDevice, s));
    int rc = run_backbone(e, n * F, slot_src(e, slot), e->cache + (size_t)frame0 * F * PA_FEATURE_STRIDE, s);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) e->ready[frame0 + i] = 1;
    return PA_OK;
}

int pa_backbone_frames(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const double* boxes,
                       int32_t frame0, uint8_t* crops_rgb, int32_t* status, void* stream) {
    if (!e || frame0 < 0) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_frames: bad argument");
    if (e->clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_frames: call pa_clip_begin first");
    if (frame0 + n > e->clip_frames) return fail(e, PA_ERR_CAPACITY, "pa_backbone_frames: frames exceed clip capacity");
    int rc = pa_preprocess_frames(e, frames, n, height, width, boxes, 0, crops_rgb, status, stream);
    if (rc) return rc;
    return pa_backbone_slot(e, 0, n, frame0, stream);
}

int pa_backbone_frames_indexed(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width,
                               const double* boxes, const int32_t* frame_ids, uint8_t* crops_rgb, int32_t* status, void* stream) {
    if (!e || !frame_ids) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_frames_indexed: bad argument");
    if (e->clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_frames_indexed: call pa_clip_begin first");
    int rc = pa_preprocess_frames(e, frames, n, height, width, boxes, 0, crops_rgb, status, stream);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    rc = run_backbone(e, n * F, slot_src(e, 0), e->feats_tmp, s);
    if (rc) return rc;
    ProfScope ps(e, s, "scatter_features", 0.0, 2.0 * n * F * PA_FEATURE_STRIDE * 4.0);
    HIPCHK(e, launch_scatter_rows(e->feats_tmp, e->pre_status[0], frame_ids, e->cache, e->cache_status, n, F, e->clip_frames,
                                  e->dev_errors, s));
    return PA_OK;
}

int pa_clean_detections(pa_engine* e, const float* dets, const int32_t* counts, int32_t n_labels, int32_t max_det, int32_t n_decoded_frames,
                        double* labels, int32_t* pixel_frame, double* pixel_box, int32_t* crop_kind, float* crop_row, int32_t* info4,
                        void* stream) {
    if (!e || !dets || !counts || !labels || !pixel_frame || !pixel_box || !crop_kind || !crop_row || !info4 || n_labels < 1 ||
        max_det < 1 || n_decoded_frames < 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_clean_detections: bad argument");
    pa::CleanParams p;
    p.dets = dets; p.counts = counts; p.n_labels = n_labels; p.max_det = max_det; p.n_decoded = n_decoded_frames;
    p.fighters = e->cfg.num_fighters;
    for (int i = 0; i < 4; ++i) p.class_ids[i] = e->cfg.fighter_class_ids[i];
    p.lab = labels; p.pixel_frame = pixel_frame; p.pixel_box = pixel_box; p.crop_kind = crop_kind; p.crop_row = crop_row; p.info = info4;
    const size_t need = (size_t)n_labels * max_det * 6;
    if (need > e->clean_g6_cap) {  // (a table longer than max_clip_frames x 8 detections: the old scratch may still be read by a call in flight)
        HIPCHK(e, hipDeviceSynchronize());
        double* grown = nullptr;
        HIPCHK(e, hipMalloc(&grown, need * sizeof(double)));
        e->allocs.push_back(grown);  // (the scratch it replaces stays in the engine's list and is freed with it)
        e->clean_g6 = grown;
        e->clean_g6_cap = need;
    }
    p.g6v = e->clean_g6;
    HIPCHK(e, pa::launch_clean_labels(p, (hipStream_t)stream));
    return PA_OK;
}

int pa_detector_plan(pa_engine* e, const int32_t* pixel_frame, const double* pixel_box, const int32_t* crop_kind, const int32_t* info4,
                     int32_t n_labels, int32_t* det_index, int32_t* src_own, int32_t* rep_entry, double* rep_boxes, int32_t* rep_src,
                     int32_t* words5, void* stream) {
    if (!e || !pixel_frame || !pixel_box || !crop_kind || !info4 || !det_index || !src_own || !rep_entry || !rep_boxes || !rep_src || !words5 ||
        n_labels < 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_detector_plan: bad argument");
    HIPCHK(e, pa::launch_detector_plan(pixel_frame, pixel_box, crop_kind, info4, n_labels, e->cfg.num_fighters, det_index, src_own, rep_entry,
                                       rep_boxes, rep_src, words5, (hipStream_t)stream));
    return PA_OK;
}

int pa_detector_plan_desc(pa_engine* e, pa_crop_image* desc, const int32_t* crop_kind, int32_t n_frames, int32_t step_frames,
                          long long region_bytes, const int32_t* rep_entry, int32_t n_rep, long long rep_base, void* stream) {
    if (!e || !desc || !crop_kind || n_frames < 1 || step_frames < 1 || region_bytes < 0 || n_rep < 0 || (n_rep && !rep_entry) || rep_base < 0)
        return fail(e, PA_ERR_INVALID_ARG, "pa_detector_plan_desc: bad argument");
    HIPCHK(e, pa::launch_detector_desc(reinterpret_cast<pa::CropImageDesc*>(desc), crop_kind, n_frames * e->cfg.num_fighters, e->cfg.num_fighters,
                                       step_frames, region_bytes, rep_entry, n_rep, rep_base, (hipStream_t)stream));
    return PA_OK;
}

int pa_square_crops_src(pa_engine* e, const uint8_t* frames, int32_t n_src, int32_t height, int32_t width, const double* boxes,
                        const int32_t* src_frame, int32_t n, int32_t padding, int32_t swap_rb, uint8_t* crops, int32_t* status, void* stream) {
    if (!e || !frames || !boxes || !src_frame || !crops || n < 1 || n_src < 1 || height < 1 || width < 1 || padding < 0)
        return fail(e, PA_ERR_INVALID_ARG, "pa_square_crops_src: bad argument");
    if (n > e->cfg.max_batch_frames || height > e->cfg.max_frame_height || width > e->cfg.max_frame_width)
        return fail(e, PA_ERR_CAPACITY, "pa_square_crops_src: crops exceed engine capacity");
    return run_preprocess(e, frames, n, height, width, boxes, padding, swap_rb, crops, nullptr, status, (hipStream_t)stream, src_frame, n_src);
}

int pa_save_one_box_crops(pa_engine* e, const uint8_t* frames, int32_t n_src, int32_t height, int32_t width, const float* dets,
                          const int32_t* counts, int32_t max_det, const int32_t* det_index, const int32_t* src_frame, int32_t n,
                          int32_t jpeg_quality, uint8_t* images, size_t images_capacity, pa_crop_image* desc, void* stream) {
    if (!e || !frames || !dets || !counts || !images || !desc || n < 1 || n_src < 1 || height < 1 || width < 1 || max_det < 1 ||
        jpeg_quality < 0 || jpeg_quality > 100 || (!src_frame && n_src != n))
        return fail(e, PA_ERR_INVALID_ARG, "pa_save_one_box_crops: bad argument");
    const int F = e->cfg.num_fighters;
    if (n * F > e->max_crops) return fail(e, PA_ERR_CAPACITY, "pa_save_one_box_crops: more frames than max_batch_frames");
    pa::SaveBoxParams p;
    memset(&p, 0, sizeof p);
    p.frames = frames; p.height = height; p.width = width; p.fighters = F; p.n_entries = n * F;
    p.dets = dets; p.counts = counts; p.max_det = max_det; p.det_index = det_index;
    p.src_frame = src_frame; p.n_src = n_src;
    for (int i = 0; i < 4; ++i) p.class_ids[i] = e->cfg.fighter_class_ids[i];
    p.gain = 1.02f; p.pad = 10.0f;  // save_one_box's defaults, which detect.py does not override
    p.images = images; p.capacity = images_capacity;
    p.desc = reinterpret_cast<pa::CropImageDesc*>(desc);
    p.rects = reinterpret_cast<pa::SaveBoxRect*>(e->savebox_rects);
    p.overflow = e->dev_errors + 1;
    p.quality = jpeg_quality;
    if (jpeg_quality > 0) {
        // jpeg_set_quality(quality, force_baseline = TRUE) on the standard tables (jcparam.c), natural order
        static const int lum[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
        static const int chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
        const int scale = jpeg_quality < 50 ? 5000 / jpeg_quality : 200 - jpeg_quality * 2;
        for (int i = 0; i < 64; ++i) {
            const int a = (lum[i] * scale + 50) / 100, b = (chr[i] * scale + 50) / 100;
            p.qtab[i] = a < 1 ? 1 : (a > 255 ? 255 : a);
            p.qtab[64 + i] = b < 1 ? 1 : (b > 255 ? 255 : b);
        }
    }
    ProfScope ps(e, (hipStream_t)stream, "save_one_box_crops", 0.0, 0.0);
    HIPCHK(e, pa::launch_save_one_box(p, (hipStream_t)stream));
    return PA_OK;
}

int pa_device_errors(pa_engine* e, int32_t* bad_frame_ids_host, void* stream) {
    if (!e || !bad_frame_ids_host) return fail(e, PA_ERR_INVALID_ARG, "pa_device_errors: bad argument");
    hipStream_t s = (hipStream_t)stream;
    int32_t h[4] = {0, 0, 0, 0};
    HIPCHK(e, hipMemcpyAsync(h, e->dev_errors, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemsetAsync(e->dev_errors, 0, sizeof(h), s));
    HIPCHK(e, hipStreamSynchronize(s));
    *bad_frame_ids_host = h[0];
    if (h[1] != 0)
        return fail(e, PA_ERR_CAPACITY, "pa_save_one_box_crops: " + std::to_string(h[1]) + " crop image(s) did not fit the image buffer");
    if (h[0] != 0)
        return fail(e, PA_ERR_CAPACITY, "pa_backbone_frames_indexed: " + std::to_string(h[0]) +
                                            " frame id(s) outside the clip were skipped on the device");
    return PA_OK;
}

int pa_backbone_frames_src(pa_engine* e, const uint8_t* frames, int32_t n_src, int32_t height, int32_t width,
                           const double* boxes, const int32_t* src_frame, int32_t n, int32_t frame0, uint8_t* crops_rgb,
                           int32_t* status, void* stream) {
    if (!e || !frames || !boxes || !src_frame || n < 1 || n_src < 1 || frame0 < 0 || height < 1 || width < 1)
        return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_frames_src: bad argument");
    if (e->clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_backbone_frames_src: call pa_clip_begin first");
    if (n > e->cfg.max_batch_frames || frame0 + n > e->clip_frames || height > e->cfg.max_frame_height ||
        width > e->cfg.max_frame_width)
        return fail(e, PA_ERR_CAPACITY, "pa_backbone_frames_src: frames exceed engine / clip capacity");
    hipStream_t s = (hipStream_t)stream;
    const int F = e->cfg.num_fighters;
    int rc = run_preprocess(e, frames, n, height, width, boxes, e->cfg.crop_padding, 1, crops_rgb, slot_dst(e, 0),
                            e->pre_status[0], s, src_frame, n_src);
    if (rc) return rc;
    if (status) HIPCHK(e, hipMemcpyAsync(status, e->pre_status[0], sizeof(int32_t) * n * F, hipMemcpyDeviceToDevice, s));
    return pa_backbone_slot(e, 0, n, frame0, stream);
}

int pa_clip_mark_ready(pa_engine* e, const int32_t* frame_ids_host, int32_t n) {
    if (!e || !frame_ids_host || n < 0) return fail(e, PA_ERR_INVALID_ARG, "pa_clip_mark_ready: bad argument");
    for (int i = 0; i < n; ++i) {
        if (frame_ids_host[i] < 0 || frame_ids_host[i] >= e->clip_frames)
            return fail(e, PA_ERR_CAPACITY, "pa_clip_mark_ready: frame id outside the clip");
        e->ready[frame_ids_host[i]] = 1;
    }
    return PA_OK;
}

int pa_head_frames(pa_engine* e, int32_t lo, int32_t hi, pa_record* records, float* logp, void* stream) {
    if (!e || lo < 1 || hi <= lo) return fail(e, PA_ERR_INVALID_ARG, "pa_head_frames: bad frame range");
    if (e->clip_frames < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_head_frames: call pa_clip_begin first");
    if (hi > e->clip_frames) return fail(e, PA_ERR_CAPACITY, "pa_head_frames: frame numbers run to max_frames - 1");
    const int S = e->cfg.sequence_length, F = e->cfg.num_fighters, D = e->cfg.frame_delta;
    const int mid = S / 2, reach = std::abs(D) * mid * mid;
    // every frame a window of [lo, hi) can touch must be cached
    {
        const int first = std::max(1, lo - reach), last = std::min(e->clip_frames - 1, hi - 1 + reach);
        for (int f = first; f <= last; ++f)
            if (!e->ready[f - 1]) return fail(e, PA_ERR_NOT_READY, "pa_head_frames: features of frame " + std::to_string(f) + " missing");
    }
    hipStream_t s = (hipStream_t)stream;
    const int frames_per_pass = e->max_crops / F;
    for (int f0 = lo; f0 < hi; f0 += frames_per_pass) {
        const int cnt = std::min(frames_per_pass, hi - f0);
        // the index table only depends on (first frame, count, clip length): a steady stream of
        // equal clips (bench.py, the frame-parallel runner) re-uses it instead of re-launching
        if (e->gather_key[0] != f0 || e->gather_key[1] != cnt || e->gather_key[2] != e->clip_frames || e->gather_key[3] != e->sub_frames) {
            HIPCHK(e, launch_window_gather(e->gather, f0, cnt, F, S, D, e->clip_frames, 1, e->sub_frames, s));
            e->gather_key[0] = f0; e->gather_key[1] = cnt; e->gather_key[2] = e->clip_frames; e->gather_key[3] = e->sub_frames;
        }
        const size_t o = (size_t)(f0 - lo) * F;
        int rc = run_head(e, cnt * F, e->cache, e->gather, e->cache_status, records ? records + o : nullptr,
                          logp ? logp + o * e->cfg.num_actions : nullptr, s);
        if (rc) return rc;
    }
    return PA_OK;
}

int pa_infer_clip(pa_engine* e, const uint8_t* frames, int32_t n, int32_t height, int32_t width, const double* boxes,
                  pa_record* records, float* logp, uint8_t* crops_rgb, int32_t* status, void* stream) {
    if (!e || n < 2) return fail(e, PA_ERR_INVALID_ARG, "pa_infer_clip: need at least 2 frames");
    int rc = pa_clip_begin(e, n);
    if (rc) return rc;
    const int F = e->cfg.num_fighters;
    const size_t frame_bytes = (size_t)height * width * 3;
    for (int f0 = 0; f0 < n; f0 += e->cfg.max_batch_frames) {
        const int cnt = std::min(e->cfg.max_batch_frames, n - f0);
        rc = pa_backbone_frames(e, frames + (size_t)f0 * frame_bytes, cnt, height, width, boxes + (size_t)f0 * F * 4, f0,
                                crops_rgb ? crops_rgb + (size_t)f0 * F * PA_CROP * PA_CROP * 3 : nullptr,
                                status ? status + (size_t)f0 * F : nullptr, stream);
        if (rc) return rc;
    }
    return pa_head_frames(e, 1, n, records, logp, stream);
}

int pa_features_export(pa_engine* e, int32_t frame0, int32_t n, float* feats, void* stream) {
    if (!e || !feats || frame0 < 0 || n < 1 || frame0 + n > e->clip_frames)
        return fail(e, PA_ERR_INVALID_ARG, "pa_features_export: bad range (call pa_clip_begin first)");
    for (int i = 0; i < n; ++i)
        if (!e->ready[frame0 + i])
            return fail(e, PA_ERR_NOT_READY, "pa_features_export: features of frame " + std::to_string(frame0 + i + 1) +
                                                 " are not cached in this clip");
    const size_t row = (size_t)e->cfg.num_fighters * PA_FEATURE_STRIDE;
    HIPCHK(e, hipMemcpyAsync(feats, e->cache + (size_t)frame0 * row, sizeof(float) * n * row, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    return PA_OK;
}

int pa_features_import(pa_engine* e, int32_t frame0, int32_t n, const float* feats, void* stream) {
    if (!e || !feats || frame0 < 0 || n < 1 || frame0 + n > e->clip_frames)
        return fail(e, PA_ERR_INVALID_ARG, "pa_features_import: bad range (call pa_clip_begin first)");
    const size_t row = (size_t)e->cfg.num_fighters * PA_FEATURE_STRIDE;
    HIPCHK(e, hipMemcpyAsync(e->cache + (size_t)frame0 * row, feats, sizeof(float) * n * row, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    // imported rows carry no crop of this engine: their status is PA_CROP_OK (== 0), not what an earlier clip left in the row
    static_assert(PA_CROP_OK == 0, "the memset below writes PA_CROP_OK");
    HIPCHK(e, hipMemsetAsync(e->cache_status + (size_t)frame0 * e->cfg.num_fighters, 0,
                             sizeof(int32_t) * (size_t)n * e->cfg.num_fighters, (hipStream_t)stream));
    for (int i = 0; i < n; ++i) e->ready[frame0 + i] = 1;
    return PA_OK;
}

int pa_profile_enable(pa_engine* e, int32_t on) {
    if (!e) return PA_ERR_INVALID_ARG;
    e->profiling = on != 0;
    return PA_OK;
}

int pa_profile_read(pa_engine* e, pa_kernel_stat* stats, int32_t max_stats, int32_t* n_stats) {
    if (!e || !stats || !n_stats || max_stats < 1) return fail(e, PA_ERR_INVALID_ARG, "pa_profile_read: bad argument");
    HIPCHK(e, hipDeviceSynchronize());
    std::vector<pa_kernel_stat> acc(e->prof_names.size());
    for (size_t i = 0; i < acc.size(); ++i) {
        memset(&acc[i], 0, sizeof(pa_kernel_stat));
        snprintf(acc[i].name, sizeof(acc[i].name), "%s", e->prof_names[i].c_str());
    }
    for (ProfEntry& p : e->prof_log) {
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, p.start, p.stop));
        acc[p.name_id].launches += 1;
        acc[p.name_id].total_ms += ms;
        acc[p.name_id].flops += p.flops;
        acc[p.name_id].bytes += p.bytes;
        acc[p.name_id].flops_executed += p.flops_executed;
        e->event_pool.push_back(p.start);
        e->event_pool.push_back(p.stop);
    }
    e->prof_log.clear();
    int n = 0;
    for (size_t i = 0; i < acc.size() && n < max_stats; ++i)
        if (acc[i].launches > 0) stats[n++] = acc[i];
    *n_stats = n;
    return PA_OK;
}

int pa_set_crop_jpeg_quality(pa_engine* e, int32_t quality) {
    if (!e || quality < 0 || quality > 100) return fail(e, PA_ERR_INVALID_ARG, "pa_set_crop_jpeg_quality: 0 (off) .. 100");
    if (quality > 0) {
        // jpeg_set_quality(quality, force_baseline = TRUE) on the standard tables (jcparam.c), natural order
        static const int lum[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
        static const int chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
        const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
        int32_t tab[128];
        for (int i = 0; i < 64; ++i) {
            const int a = (lum[i] * scale + 50) / 100, b = (chr[i] * scale + 50) / 100;
            tab[i] = a < 1 ? 1 : (a > 255 ? 255 : a);
            tab[64 + i] = b < 1 ? 1 : (b > 255 ? 255 : b);
        }
        HIPCHK(e, hipMemcpy(e->jpeg_qtab, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    e->jpeg_quality = quality;
    return PA_OK;
}

int pa_stream_spin(pa_engine* e, int32_t microseconds, void* stream) {
    if (!e || microseconds < 0 || microseconds > 100000) return fail(e, PA_ERR_INVALID_ARG, "pa_stream_spin: 0..100000 us");
    HIPCHK(e, launch_spin(microseconds, (hipStream_t)stream));
    return PA_OK;
}

int pa_stream_gate(pa_engine* e, int32_t max_microseconds, void* stream) {
    if (!e || max_microseconds < 1 || max_microseconds > 100000) return fail(e, PA_ERR_INVALID_ARG, "pa_stream_gate: 1..100000 us");
    if (!e->gate_flag) HIPCHK(e, hipHostMalloc((void**)&e->gate_flag, 64, hipHostMallocCoherent | hipHostMallocMapped));
    __atomic_store_n(e->gate_flag, 0, __ATOMIC_SEQ_CST);
    HIPCHK(e, launch_gate(e->gate_flag, max_microseconds, (hipStream_t)stream));
    return PA_OK;
}

int pa_stream_gate_open(pa_engine* e) {
    if (!e) return PA_ERR_INVALID_ARG;
    if (e->gate_flag) __atomic_store_n(e->gate_flag, 1, __ATOMIC_SEQ_CST);
    return PA_OK;
}

int pa_stream_sync(pa_engine* e, void* stream) {
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return PA_OK;
}

}  // extern "C"

// ===============================================================================
// Scoring (csrc/metrics.hip): a handle of its own, owned by no engine
// ===============================================================================

struct pa_eval {
    int actions = 0;
    // one allocation: counts {rows, correct, ignored, bad_labels} | sums {nll_sum, conf_sum} (= pa_eval_totals) | confusion [A][A] | slab
    unsigned char* state = nullptr;
    size_t state_bytes = 0;  // what pa_eval_reset zeroes: everything but the slab
    unsigned long long* counts() const { return reinterpret_cast<unsigned long long*>(state); }
    double* sums() const { return reinterpret_cast<double*>(state + 4 * sizeof(int64_t)); }
    unsigned long long* confusion() const { return reinterpret_cast<unsigned long long*>(state + sizeof(pa_eval_totals)); }
    double* slab() const { return reinterpret_cast<double*>(state + state_bytes); }
};

static_assert(sizeof(pa_eval_totals) == 48, "pa_eval_totals is four int64 and two doubles, read back in one copy");

extern "C" {

int pa_eval_create(int32_t device, int32_t num_actions, pa_eval** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (device < 0 || num_actions < 1 || num_actions > 4096) return PA_ERR_INVALID_ARG;
    pa_eval* h = new pa_eval();
    *out = h;
    h->actions = num_actions;
    h->state_bytes = sizeof(pa_eval_totals) + (size_t)num_actions * num_actions * sizeof(int64_t);
    if (hipSetDevice(device) != hipSuccess) return PA_ERR_NO_DEVICE;
    void* p = nullptr;
    if (hipMalloc(&p, h->state_bytes + 2 * EVAL_SLAB_PARTS * sizeof(double)) != hipSuccess) return PA_ERR_HIP;
    h->state = static_cast<unsigned char*>(p);
    if (hipMemset(h->state, 0, h->state_bytes) != hipSuccess) return PA_ERR_HIP;
    return PA_OK;
}

void pa_eval_destroy(pa_eval* h) {
    if (!h) return;
    (void)hipFree(h->state);
    delete h;
}

int pa_eval_reset(pa_eval* h, void* stream) {
    if (!h) return PA_ERR_INVALID_ARG;
    if (!h->state) return PA_ERR_NO_DEVICE;
    return hipMemsetAsync(h->state, 0, h->state_bytes, (hipStream_t)stream) == hipSuccess ? PA_OK : PA_ERR_HIP;
}

int pa_eval_update(pa_eval* h, const float* logp_dev, int32_t ld, int32_t n, const int32_t* labels_dev, int32_t label_stride,
                   void* stream) {
    if (!h || !logp_dev || !labels_dev || ld < h->actions || n < 0 || label_stride < 1) return PA_ERR_INVALID_ARG;
    if (!h->state) return PA_ERR_NO_DEVICE;
    return launch_eval_rows(logp_dev, ld, n, h->actions, labels_dev, label_stride, h->counts(), h->sums(), h->confusion(), h->slab(),
                            (hipStream_t)stream) == hipSuccess ? PA_OK : PA_ERR_HIP;
}

int pa_eval_read(pa_eval* h, pa_eval_totals* totals_host, int64_t* confusion_host, void* stream) {
    if (!h || !totals_host) return PA_ERR_INVALID_ARG;
    if (!h->state) return PA_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(totals_host, h->state, sizeof(pa_eval_totals), hipMemcpyDeviceToHost, s) != hipSuccess) return PA_ERR_HIP;
    if (confusion_host && hipMemcpyAsync(confusion_host, h->confusion(), (size_t)h->actions * h->actions * sizeof(int64_t),
                                         hipMemcpyDeviceToHost, s) != hipSuccess)
        return PA_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return PA_ERR_HIP;
    return totals_host->bad_labels != 0 ? PA_ERR_BAD_LABELS : PA_OK;
}

}  // extern "C"

// ===============================================================================
// Training of the temporal head (csrc/head_train.hip): a handle beside its engine
// ===============================================================================

struct pa_head_trainer : pa::TrainerCore {   // state: m | v (six tensors each, in the weights' layouts) | the step's scratch
    pa_engine* eng = nullptr;
    int max_batch = 0, S = 0, A = 0;
    float *m[6] = {}, *v[6] = {};
    float *h1 = nullptr, *h2 = nullptr, *dz3 = nullptr, *dz2 = nullptr, *dz1 = nullptr, *loss_b = nullptr, *gs = nullptr, *stats = nullptr;
    int32_t* hit_b = nullptr;
};

static_assert(sizeof(pa_train_stats) == 16 && sizeof(pa_adam_config) == 16, "pa_train_stats / pa_adam_config are four 32-bit words");

namespace {

// floats of tensor i (blob order) in the layout the inference kernels read
size_t head_layout_floats(int i, int S, int A) {
    const size_t n[6] = {(size_t)512 * S * PA_FEATURE_STRIDE, 512, 512 * 128, 128, 128 * 64, (size_t)A};
    return (n[i] + 63) & ~(size_t)63;   // every tensor starts 256-byte aligned
}

}  // namespace

extern "C" {

int pa_head_trainer_create(pa_engine* e, const pa_adam_config* cfg, int32_t max_batch, pa_head_trainer** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (!e || !cfg || max_batch < 1 || max_batch > 256) return PA_ERR_INVALID_ARG;
    if (!adam_config_ok(cfg->lr, cfg->beta1, cfg->beta2, cfg->eps)) return PA_ERR_INVALID_ARG;
    pa_head_trainer* t = new pa_head_trainer();
    *out = t;   // (handed back whatever follows: TrainerCore)
    t->eng = e;
    t->cfg = *cfg;
    t->max_batch = max_batch;
    t->S = e->cfg.sequence_length;
    t->A = e->cfg.num_actions;
    if (!e->w1d || !e->b1d || !e->w2 || !e->b2 || !e->w3 || !e->b3)
        return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_head_trainer_create: the engine has no weights on a device");
    if (hipSetDevice(e->cfg.device_id) != hipSuccess) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_head_trainer_create: hipSetDevice failed");
    size_t moments = 0;
    for (int i = 0; i < 6; ++i) moments += head_layout_floats(i, t->S, t->A);
    const size_t B = (size_t)max_batch;
    const size_t scratch = B * 512 * 2 + B * 128 * 2 + B * 64 + B * 2 + (512 * 128 + 128 * 64 + 512 + 128 + 64) + 64;
    if (const int rc = trainer_alloc_zeroed(t, 2 * moments + scratch, "pa_head_trainer_create")) return rc;
    float* q = t->state;
    for (int i = 0; i < 6; ++i) {
        t->m[i] = q;
        q += head_layout_floats(i, t->S, t->A);
    }
    for (int i = 0; i < 6; ++i) {
        t->v[i] = q;
        q += head_layout_floats(i, t->S, t->A);
    }
    t->h1 = q, q += B * 512;
    t->dz1 = q, q += B * 512;
    t->h2 = q, q += B * 128;
    t->dz2 = q, q += B * 128;
    t->dz3 = q, q += B * 64;
    t->loss_b = q, q += B;
    t->hit_b = reinterpret_cast<int32_t*>(q), q += B;
    t->gs = q, q += 512 * 128 + 128 * 64 + 512 + 128 + 64;
    t->stats = q;
    return PA_OK;
}

void pa_head_trainer_destroy(pa_head_trainer* t) { trainer_destroy(t); }

const char* pa_head_trainer_last_error(const pa_head_trainer* t) { return trainer_last_error(t); }

int64_t pa_head_trainer_steps(const pa_head_trainer* t) { return trainer_steps(t); }

int pa_head_train_step(pa_head_trainer* t, const float* feats, int32_t n_rows, const int32_t* gather, const int32_t* labels, int32_t batch,
                       int32_t apply, float* grads_out, pa_train_stats* stats_dev, void* stream) {
    if (!t) return PA_ERR_INVALID_ARG;
    if (!feats || !gather || !labels || n_rows < 1) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_head_train_step: null input or n_rows < 1");
    if (batch < 1 || batch > t->max_batch) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_head_train_step: batch outside 1..max_batch");
    if (const int rc = trainer_check_apply(t, apply, grads_out, "pa_head_train_step")) return rc;
    if ((reinterpret_cast<uintptr_t>(feats) & 15) != 0) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_head_train_step: feats must be 16-byte aligned");
    if (!t->state) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_head_train_step: the trainer has no device state");
    pa_engine* e = t->eng;
    HeadTrainParams p;
    memset(&p, 0, sizeof(p));
    p.feats = feats;
    p.gather = gather;
    p.labels = labels;
    p.n_rows = n_rows;
    p.B = batch;
    p.S = t->S;
    p.A = t->A;
    p.apply = apply;
    float* w[6] = {e->w1d, e->b1d, e->w2, e->b2, e->w3, e->b3};
    for (int i = 0; i < 6; ++i) {
        p.w[i] = w[i];
        p.m[i] = t->m[i];
        p.v[i] = t->v[i];
    }
    p.h1 = t->h1, p.h2 = t->h2, p.dz3 = t->dz3, p.dz2 = t->dz2, p.dz1 = t->dz1, p.loss_b = t->loss_b, p.gs = t->gs, p.stats = t->stats;
    p.hit_b = t->hit_b;
    p.stats_out = reinterpret_cast<float*>(stats_dev);
    p.grads_out = grads_out;
    const AdamScalars ak = adam_scalars(t->cfg.lr, t->cfg.beta1, t->cfg.beta2, t->cfg.eps, t->steps + 1, apply != 0);
    const hipError_t err = launch_head_train_step(p, ak, (hipStream_t)stream);
    if (err != hipSuccess) return trainer_fail(t, PA_ERR_HIP, std::string("pa_head_train_step: ") + hipGetErrorString(err));
    if (apply) t->steps += 1;
    return PA_OK;
}

int pa_head_trainer_read(pa_head_trainer* t, int32_t which, float* out_dev, size_t floats, void* stream) {
    if (!t) return PA_ERR_INVALID_ARG;
    const int set = which & ~PA_TRAIN_RAW;
    if (const int rc = trainer_check_which(t, set, out_dev, "pa_head_trainer_read")) return rc;
    const bool raw = (which & PA_TRAIN_RAW) != 0;
    const size_t raw_n[6] = {(size_t)512 * t->S * PA_FEATURE_STRIDE, 512, 512 * 128, 128, 128 * 64, (size_t)t->A};
    const size_t want = raw ? raw_n[0] + raw_n[1] + raw_n[2] + raw_n[3] + raw_n[4] + raw_n[5] : head_tensor_floats(t->S, t->A);
    if (floats != want) return trainer_fail(t, PA_ERR_INVALID_ARG, "pa_head_trainer_read: wrong output size");
    if (!t->state) return trainer_fail(t, PA_ERR_NO_DEVICE, "pa_head_trainer_read: the trainer has no device state");
    pa_engine* e = t->eng;
    HeadTensors src;
    const float* w[6] = {e->w1d, e->b1d, e->w2, e->b2, e->w3, e->b3};
    for (int i = 0; i < 6; ++i) src.p[i] = set == PA_TRAIN_WEIGHTS ? w[i] : set == PA_TRAIN_M ? t->m[i] : t->v[i];
    if (raw) {
        for (int i = 0; i < 6; ++i) {
            if (hipMemcpyAsync(out_dev, src.p[i], raw_n[i] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
                return trainer_fail(t, PA_ERR_HIP, "pa_head_trainer_read: hipMemcpyAsync failed");
            out_dev += raw_n[i];
        }
        return PA_OK;
    }
    const hipError_t err = launch_head_export(src, t->S, t->A, out_dev, (hipStream_t)stream);
    if (err != hipSuccess) return trainer_fail(t, PA_ERR_HIP, std::string("pa_head_trainer_read: ") + hipGetErrorString(err));
    return PA_OK;
}

}  // extern "C"

// ===============================================================================
// Annotation (csrc/annotate.hip): a handle of its own, owned by no engine
// ===============================================================================

// A call's draw lists are staged through one of PA_ANNOT_SLOTS (pinned host + device) buffers; a slot is taken again only
// after the event behind the launch that read it, so calls on several streams never share a list.
constexpr int PA_ANNOT_SLOTS = 4;

struct pa_annot {
    int cell_w = 0, cell_h = 0, first_char = 0, n_chars = 0, max_frames = 0, max_items = 0, max_text = 0;
    unsigned char* atlas = nullptr;
    size_t items_bytes = 0, counts_bytes = 0, slot_bytes = 0;  // slot: items | counts | text
    unsigned char* host[PA_ANNOT_SLOTS] = {};
    unsigned char* dev[PA_ANNOT_SLOTS] = {};
    hipEvent_t done[PA_ANNOT_SLOTS] = {};
    bool used[PA_ANNOT_SLOTS] = {};
    int next = 0;
};

static_assert(sizeof(pa_annot_item) == 40, "pa_annot_item is nine int32 and four bytes (playaid_core_amd/_lib.py mirrors it)");

extern "C" {

int pa_annot_create(int32_t device, const uint8_t* atlas_host, int32_t cell_w, int32_t cell_h, int32_t first_char, int32_t n_chars,
                    int32_t max_frames, int32_t max_items, int32_t max_text, pa_annot** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (device < 0 || !atlas_host || cell_w < 1 || cell_w > 64 || cell_h < 1 || cell_h > 64 || first_char < 0 || n_chars < 1 ||
        first_char + n_chars > 256 || max_frames < 1 || max_frames > 65535 || max_items < 1 || max_items > PA_ANNOT_MAX_ITEMS ||
        max_text < 1 || max_text > (1 << 20))
        return PA_ERR_INVALID_ARG;
    pa_annot* h = new pa_annot();
    *out = h;
    h->cell_w = cell_w, h->cell_h = cell_h, h->first_char = first_char, h->n_chars = n_chars;
    h->max_frames = max_frames, h->max_items = max_items, h->max_text = max_text;
    h->items_bytes = (size_t)max_frames * PA_ANNOT_MAX_ITEMS * sizeof(pa_annot_item);
    h->counts_bytes = (size_t)max_frames * sizeof(int32_t);
    h->slot_bytes = (h->items_bytes + h->counts_bytes + (size_t)max_text + 15) & ~(size_t)15;
    if (hipSetDevice(device) != hipSuccess) return PA_ERR_NO_DEVICE;
    const size_t atlas_bytes = (size_t)n_chars * (n_chars + 1) * cell_h * cell_w;
    void* p = nullptr;
    if (hipMalloc(&p, atlas_bytes) != hipSuccess) return PA_ERR_HIP;
    h->atlas = static_cast<unsigned char*>(p);
    if (hipMemcpy(h->atlas, atlas_host, atlas_bytes, hipMemcpyHostToDevice) != hipSuccess) return PA_ERR_HIP;
    for (int i = 0; i < PA_ANNOT_SLOTS; ++i) {
        if (hipHostMalloc(&p, h->slot_bytes, hipHostMallocDefault) != hipSuccess) return PA_ERR_HIP;
        h->host[i] = static_cast<unsigned char*>(p);
        if (hipMalloc(&p, h->slot_bytes) != hipSuccess) return PA_ERR_HIP;
        h->dev[i] = static_cast<unsigned char*>(p);
        if (hipEventCreateWithFlags(&h->done[i], hipEventDisableTiming) != hipSuccess) return PA_ERR_HIP;
    }
    return PA_OK;
}

void pa_annot_destroy(pa_annot* h) {
    if (!h) return;
    for (int i = 0; i < PA_ANNOT_SLOTS; ++i) {
        if (h->used[i]) (void)hipEventSynchronize(h->done[i]);
        if (h->done[i]) (void)hipEventDestroy(h->done[i]);
        if (h->dev[i]) (void)hipFree(h->dev[i]);
        if (h->host[i]) (void)hipHostFree(h->host[i]);
    }
    if (h->atlas) (void)hipFree(h->atlas);
    delete h;
}

int pa_annotate_frames(pa_annot* h, const uint8_t* frames_in, int32_t n, int32_t height, int32_t width, const pa_annot_item* items_host,
                       const int32_t* counts_host, const uint8_t* text_host, int32_t text_bytes, int32_t pad_left, int32_t pad_right,
                       int32_t pad_bottom, uint8_t* frames_out, void* stream) {
    if (!h || n < 0) return PA_ERR_INVALID_ARG;
    if (n == 0) return PA_OK;
    if (!frames_in || !frames_out || frames_in == frames_out || !counts_host || height < 1 || width < 1 || pad_left < 0 || pad_right < 0 ||
        pad_bottom < 0 || text_bytes < 0 || text_bytes > h->max_text || (text_bytes > 0 && !text_host))
        return PA_ERR_INVALID_ARG;
    if ((long long)height + pad_bottom > 32768 || (long long)pad_left + width + pad_right > 32768) return PA_ERR_INVALID_ARG;
    if (n > h->max_frames) return PA_ERR_CAPACITY;
    for (int f = 0; f < n; ++f) {
        if (counts_host[f] < 0 || counts_host[f] > h->max_items || (counts_host[f] > 0 && !items_host)) return PA_ERR_INVALID_ARG;
        for (int i = 0; i < counts_host[f]; ++i) {
            const pa_annot_item& it = items_host[(size_t)f * PA_ANNOT_MAX_ITEMS + i];
            if (it.line_width < 0 || it.line_width > 32767 || it.text_len < 0 || it.text_off < 0 ||
                (long long)it.text_off + it.text_len > text_bytes)
                return PA_ERR_INVALID_ARG;
        }
    }
    for (int i = 0; i < text_bytes; ++i)
        if (text_host[i] < h->first_char || text_host[i] >= h->first_char + h->n_chars) return PA_ERR_INVALID_ARG;
    if (!h->done[PA_ANNOT_SLOTS - 1]) return PA_ERR_NO_DEVICE;  // a create that stopped at the device

    const int slot = h->next;
    h->next = (h->next + 1) % PA_ANNOT_SLOTS;
    if (h->used[slot] && hipEventSynchronize(h->done[slot]) != hipSuccess) return PA_ERR_HIP;
    unsigned char* hs = h->host[slot];
    unsigned char* ds = h->dev[slot];
    const size_t used_items = (size_t)n * PA_ANNOT_MAX_ITEMS * sizeof(pa_annot_item);
    if (items_host)
        std::memcpy(hs, items_host, used_items);
    else
        std::memset(hs, 0, used_items);
    std::memcpy(hs + h->items_bytes, counts_host, (size_t)n * sizeof(int32_t));
    unsigned char* text = hs + h->items_bytes + h->counts_bytes;
    for (int i = 0; i < text_bytes; ++i) text[i] = (unsigned char)(text_host[i] - h->first_char);  // atlas rows
    hipStream_t s = (hipStream_t)stream;
    // (two copies: the used head of the items, then counts and text, which lie behind the items' full capacity)
    if (hipMemcpyAsync(ds, hs, used_items, hipMemcpyHostToDevice, s) != hipSuccess) return PA_ERR_HIP;
    if (hipMemcpyAsync(ds + h->items_bytes, hs + h->items_bytes, h->counts_bytes + (size_t)text_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return PA_ERR_HIP;
    pa::AnnotParams p;
    p.in = frames_in;
    p.out = frames_out;
    p.items = ds;
    p.counts = reinterpret_cast<const int*>(ds + h->items_bytes);
    p.text = ds + h->items_bytes + h->counts_bytes;
    p.atlas = h->atlas;
    p.n = n, p.H = height, p.W = width, p.pad_left = pad_left, p.pad_right = pad_right, p.pad_bottom = pad_bottom;
    p.cell_w = h->cell_w, p.cell_h = h->cell_h, p.n_chars = h->n_chars;
    if (pa::launch_annotate(p, s) != hipSuccess) return PA_ERR_HIP;
    h->used[slot] = true;
    if (hipEventRecord(h->done[slot], s) != hipSuccess) return PA_ERR_HIP;
    return PA_OK;
}

// ---- synthetic training frames (synth_composite.hip) ----------------------------------------------------------------------------

struct pa_synth_bank {
    int kind = 0;
    std::vector<SynthDesc> descs;   // the host's copy of the table: what the argument checks read
    int min_w = 0, min_h = 0;
    int dim_min = PA_SYNTH_DIM_MIN;   // sprites: the smallest dim at which every image resizes to at least 1 x 1
    unsigned char* dev = nullptr;   // [descriptor table, padded to 16 bytes][images]; nullptr: a bank made without an engine
    size_t table_bytes = 0;
    unsigned char* scratch = nullptr;   // pa_sprite_bank_create: the augmentation kernel's, [scratch_groups][SPRITE_SCRATCH_BYTES]
    int scratch_groups = 0;
    bool slots = false;                 // ... and its images are slots that pa_sprite_augment writes
    // pa_sprite_resize_bank_create: slots of up to slot_w x slot_h that pa_sprite_resize writes, descriptors included
    int slot_w = 0, slot_h = 0;
    size_t slot_bytes = 0;
    pa_sprite_resize_params* params_dev = nullptr;      // [slots], behind the pixels in `dev`
    pa_sprite_resize_params* params_pinned = nullptr;   // [slots]: where a call's records wait for their copy
    hipEvent_t staged = nullptr;                        // ... recorded behind that copy
    bool staged_pending = false;
};

int pa_synth_bank_create(pa_engine* e, int32_t kind, const uint8_t* const* images_host, const int32_t* widths, const int32_t* heights,
                         int32_t n, pa_synth_bank** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    pa_synth_bank* b = nullptr;
    try {   // (the table, the messages and the host copy of the whole bank allocate: no exception may cross the C ABI)
        if ((kind != PA_SYNTH_SPRITES && kind != PA_SYNTH_STAGES) || !images_host || !widths || !heights || n < 1)
            return fail(e, PA_ERR_INVALID_ARG, "pa_synth_bank_create: kind is PA_SYNTH_SPRITES or PA_SYNTH_STAGES, n at least 1, no null array");
        const int side_max = kind == PA_SYNTH_SPRITES ? PA_SYNTH_SPRITE_MAX : PA_SYNTH_STAGE_MAX;
        const size_t px_bytes = kind == PA_SYNTH_SPRITES ? 4 : 3;
        std::vector<SynthDesc> descs((size_t)n);
        size_t total = 0;
        int min_w = side_max, min_h = side_max, dim_min = PA_SYNTH_DIM_MIN;
        for (int32_t k = 0; k < n; ++k) {
            const int w = widths[k], h = heights[k];
            const std::string which = "pa_synth_bank_create: image " + std::to_string(k) + " (" + std::to_string(h) + " x " + std::to_string(w) + ")";
            if (!images_host[k]) return fail(e, PA_ERR_INVALID_ARG, which + " has no pixels");
            if (w < 1 || h < 1 || w > side_max || h > side_max)
                return fail(e, PA_ERR_INVALID_ARG, which + ": sides are 1.." + std::to_string(side_max));
            if (kind == PA_SYNTH_SPRITES) {
                const int d = synth_dim_min(w, h);
                if (d > PA_SYNTH_DIM_MAX) return fail(e, PA_ERR_INVALID_ARG, which + ": too thin, no dim resizes it to at least 1 x 1");
                dim_min = std::max(dim_min, d);
            }
            descs[k].offset = total;
            descs[k].w = w;
            descs[k].h = h;
            total += ((size_t)w * h * px_bytes + 15) & ~(size_t)15;
            min_w = std::min(min_w, w);
            min_h = std::min(min_h, h);
        }
        b = new pa_synth_bank();
        b->kind = kind;
        b->descs = descs;
        b->min_w = min_w;
        b->min_h = min_h;
        b->dim_min = dim_min;
        b->table_bytes = ((size_t)n * sizeof(SynthDesc) + 15) & ~(size_t)15;
        if (e) {   // (without an engine: the table alone, for pa_synth_params_check)
            std::vector<unsigned char> stage(b->table_bytes + total, 0);
            std::memcpy(stage.data(), descs.data(), (size_t)n * sizeof(SynthDesc));
            for (int32_t k = 0; k < n; ++k)
                std::memcpy(stage.data() + b->table_bytes + descs[k].offset, images_host[k], (size_t)descs[k].w * descs[k].h * px_bytes);
            void* p = nullptr;
            hipError_t err = hipMalloc(&p, stage.size());
            if (err == hipSuccess) {
                b->dev = static_cast<unsigned char*>(p);
                err = hipMemcpy(p, stage.data(), stage.size(), hipMemcpyHostToDevice);
            }
            if (err != hipSuccess) {
                pa_synth_bank_destroy(b);
                b = nullptr;
                return fail(e, PA_ERR_HIP, std::string("pa_synth_bank_create: ") + hipGetErrorString(err));
            }
        }
        *out = b;
        return PA_OK;
    } catch (const std::exception&) {
        pa_synth_bank_destroy(b);
        if (e) e->last_error.clear();   // (no allocation on this path)
        return PA_ERR_CAPACITY;         // out of host memory
    }
}

void pa_synth_bank_destroy(pa_synth_bank* b) {
    if (!b) return;
    if (b->dev) (void)hipFree(b->dev);
    if (b->scratch) (void)hipFree(b->scratch);
    if (b->staged) {
        if (b->staged_pending) (void)hipEventSynchronize(b->staged);
        (void)hipEventDestroy(b->staged);
    }
    if (b->params_pinned) (void)hipHostFree(b->params_pinned);
    delete b;
}

int pa_synth_params_check(const pa_synth_params* host, int32_t n, const pa_synth_bank* sprites, const pa_synth_bank* stages, int32_t dim) {
    if (!host || n < 1 || !sprites || !stages || sprites->kind != PA_SYNTH_SPRITES || stages->kind != PA_SYNTH_STAGES ||
        dim < PA_SYNTH_DIM_MIN || dim > PA_SYNTH_DIM_MAX || dim < sprites->dim_min)
        return PA_ERR_INVALID_ARG;
    for (int32_t i = 0; i < n; ++i) {
        const pa_synth_params& p = host[i];
        if (p.sprite < 0 || p.sprite >= (int32_t)sprites->descs.size() || p.stage < 0 || p.stage >= (int32_t)stages->descs.size())
            return PA_ERR_INVALID_ARG;
        const SynthDesc& g = stages->descs[(size_t)p.stage];
        if (g.w < dim || g.h < dim || p.stage_x < 0 || p.stage_x > g.w - dim || p.stage_y < 0 || p.stage_y > g.h - dim) return PA_ERR_INVALID_ARG;
        if (p.paste_dx < -PA_SYNTH_PASTE_MAX || p.paste_dx > PA_SYNTH_PASTE_MAX || p.paste_dy < -PA_SYNTH_PASTE_MAX || p.paste_dy > PA_SYNTH_PASTE_MAX)
            return PA_ERR_INVALID_ARG;
        if (p.reserved[0] != 0 || p.reserved[1] != 0) return PA_ERR_INVALID_ARG;
    }
    return PA_OK;
}

int pa_synth_composite(pa_engine* e, const pa_synth_bank* sprites, const pa_synth_bank* stages, const pa_synth_params* params_dev,
                       int32_t n, int32_t dim, int32_t out_format, void* out_dev, void* stream) {
    if (!e || !sprites || !stages || !params_dev || !out_dev || n < 1 || n > 65535 || sprites->kind != PA_SYNTH_SPRITES ||
        stages->kind != PA_SYNTH_STAGES || (out_format != PA_SYNTH_U8 && out_format != PA_SYNTH_MODEL))
        return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: bad argument");
    if (!sprites->dev || !stages->dev) return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: a bank that was made without an engine has no pixels");
    if (dim < PA_SYNTH_DIM_MIN || dim > PA_SYNTH_DIM_MAX || (out_format == PA_SYNTH_MODEL && dim != PA_CROP))
        return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: dim is " + std::to_string(PA_SYNTH_DIM_MIN) + ".." + std::to_string(PA_SYNTH_DIM_MAX) +
                                               ", and 128 for PA_SYNTH_MODEL");
    if ((uintptr_t)out_dev & 15 || (uintptr_t)params_dev & 7)
        return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: out must be 16-byte aligned, params 8-byte aligned");
    if (stages->min_w < dim || stages->min_h < dim) return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: a stage of the bank is smaller than dim");
    if (dim < sprites->dim_min)
        return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: a sprite of the bank is too thin for this dim (it resizes to an empty image below dim " +
                                               std::to_string(sprites->dim_min) + ")");
    if (!e->aug_tabs) return fail(e, PA_ERR_INVALID_ARG, "pa_synth_composite: the engine has no tables");
    SynthArgs a;
    a.sprite_px = sprites->dev + sprites->table_bytes;
    a.sprite_desc = reinterpret_cast<const SynthDesc*>(sprites->dev);
    a.n_sprites = (int)sprites->descs.size();
    a.stage_px = stages->dev + stages->table_bytes;
    a.stage_desc = reinterpret_cast<const SynthDesc*>(stages->dev);
    a.n_stages = (int)stages->descs.size();
    a.params = params_dev;
    a.n = n, a.dim = dim, a.out_format = out_format;
    a.out = out_dev;
    a.unit = e->aug_tabs->unit;
    const double px = (double)n * dim * dim;
    ProfScope ps(e, (hipStream_t)stream, "synth_composite", 0.0, px * (out_format == PA_SYNTH_MODEL ? 15.0 : 6.0));
    HIPCHK(e, launch_synth_composite(a, (hipStream_t)stream));
    return PA_OK;
}

// ---- augmentation of the renders before the paste (sprite_augment.hip) -----------------------------------------------------------

// The bank-level limits of pa_sprite_augment: PA_OK, PA_ERR_INVALID_ARG for a render whose resize to width 128 is empty (cv2.resize
// raises; so does Pillow for an empty contain size, which h1 <= PA_SPRITE_H1_MAX rules out), PA_ERR_CAPACITY for one taller than that.
static int sprite_bank_limits(const pa_synth_bank* sprites, int* which) {
    for (size_t k = 0; k < sprites->descs.size(); ++k) {
        const RunnerInPlan in = runner_in_plan(sprites->descs[k].w, sprites->descs[k].h, (size_t)1 << 30);
        *which = (int)k;
        if (in.status == PA_CROP_EMPTY || in.area.oh < 1) return PA_ERR_INVALID_ARG;
        if (in.status != PA_CROP_OK || in.area.oh > PA_SPRITE_H1_MAX) return PA_ERR_CAPACITY;
    }
    return PA_OK;
}

int pa_sprite_aug_params_check(const pa_sprite_aug_params* host, int32_t n, const pa_synth_bank* sprites) {
    if (!host || n < 1 || !sprites || sprites->kind != PA_SYNTH_SPRITES) return PA_ERR_INVALID_ARG;
    int which = 0;
    const int rc = sprite_bank_limits(sprites, &which);
    if (rc != PA_OK) return rc;
    auto in = [](float x, float lo, float hi) { return x >= lo && x <= hi; };   // false for NaN
    for (int32_t i = 0; i < n; ++i) {
        const pa_sprite_aug_params& p = host[i];
        if (p.src < 0 || p.src >= (int32_t)sprites->descs.size() || (p.flip != 0 && p.flip != 1)) return PA_ERR_INVALID_ARG;
        if (!in(p.alpha, 0.8f, 1.2f) || !in(p.beta, -0.2f, 0.6f)) return PA_ERR_INVALID_ARG;
        if (p.blur_k != 0 && p.blur_k != 2 && p.blur_k != 3) return PA_ERR_INVALID_ARG;
        if (!in(p.hue_shift, -256.f, 256.f) || !in(p.sat_shift, -67.f, 67.f) || !in(p.val_shift, -10.f, 10.f)) return PA_ERR_INVALID_ARG;
        if (p.noise_sigma != 0.f && !in(p.noise_sigma, 20.679216f, 22.360680f)) return PA_ERR_INVALID_ARG;   // sqrt(427.63), sqrt(500) as floats
        if (p.pixel_drop_thr != 0u && p.pixel_drop_thr != PA_SPRITE_DROP_THR) return PA_ERR_INVALID_ARG;
        if (p.new_scale != 0 && (p.new_scale < 96 || p.new_scale > 127)) return PA_ERR_INVALID_ARG;
        if ((p.sized_crop != 0 && p.sized_crop != 1) || p.reserved != 0) return PA_ERR_INVALID_ARG;
        const int C = p.new_scale ? 256 - p.new_scale : 128, O = p.sized_crop ? 128 : C;
        const int S = std::min(96, C / 3);
        if (p.n_holes < 0 || p.n_holes > 2 || p.channel_mask < 0 || p.channel_mask > 6) return PA_ERR_INVALID_ARG;
        for (int h = 0; h < 2 * p.n_holes; ++h)
            if (p.holes[h] > C - S) return PA_ERR_INVALID_ARG;
        for (int k = 0; k < O; ++k)
            if (p.xmap[k] >= C || p.ymap[k] >= C || p.axmap[k] >= C || p.aymap[k] >= C) return PA_ERR_INVALID_ARG;
    }
    return PA_OK;
}

int pa_sprite_bank_create(pa_engine* e, int32_t n, pa_synth_bank** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    pa_synth_bank* b = nullptr;
    try {
        if (n < 1 || n > 65535) return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_bank_create: n is 1..65535");
        b = new pa_synth_bank();
        b->kind = PA_SYNTH_SPRITES;
        b->slots = true;
        b->descs.resize((size_t)n);
        for (int32_t k = 0; k < n; ++k) {
            b->descs[(size_t)k].offset = (uint64_t)k * (PA_CROP * PA_CROP * 4);
            b->descs[(size_t)k].w = b->descs[(size_t)k].h = PA_CROP;
        }
        b->min_w = b->min_h = PA_CROP;
        b->table_bytes = ((size_t)n * sizeof(SynthDesc) + 15) & ~(size_t)15;
        if (e) {
            const size_t bytes = b->table_bytes + (size_t)n * (PA_CROP * PA_CROP * 4);
            b->scratch_groups = std::min((int)n, SPRITE_WORKGROUPS_MAX);
            void* p = nullptr;
            hipError_t err = hipMalloc(&p, bytes);
            if (err == hipSuccess) {
                b->dev = static_cast<unsigned char*>(p);
                err = hipMemset(p, 0, bytes);
            }
            if (err == hipSuccess) err = hipMemcpy(p, b->descs.data(), (size_t)n * sizeof(SynthDesc), hipMemcpyHostToDevice);
            if (err == hipSuccess) {
                err = hipMalloc(&p, (size_t)b->scratch_groups * SPRITE_SCRATCH_BYTES);
                if (err == hipSuccess) b->scratch = static_cast<unsigned char*>(p);
            }
            if (err != hipSuccess) {
                pa_synth_bank_destroy(b);
                b = nullptr;
                return fail(e, PA_ERR_HIP, std::string("pa_sprite_bank_create: ") + hipGetErrorString(err));
            }
        }
        *out = b;
        return PA_OK;
    } catch (const std::exception&) {
        pa_synth_bank_destroy(b);
        if (e) e->last_error.clear();
        return PA_ERR_CAPACITY;
    }
}

int pa_sprite_augment(pa_engine* e, const pa_synth_bank* sprites, const pa_sprite_aug_params* params_dev, int32_t n, pa_synth_bank* out_bank,
                      void* stream) {
    if (!e || !sprites || !params_dev || !out_bank || n < 1 || sprites->kind != PA_SYNTH_SPRITES || (uintptr_t)params_dev & 7)
        return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_augment: bad argument (params 8-byte aligned, n at least 1)");
    if (!out_bank->slots || !out_bank->dev || !out_bank->scratch || out_bank == sprites)
        return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_augment: out_bank is a bank of pa_sprite_bank_create, made with an engine, and not the source");
    if (!sprites->dev) return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_augment: a bank that was made without an engine has no pixels");
    if (n > (int32_t)out_bank->descs.size())
        return fail(e, PA_ERR_CAPACITY, "pa_sprite_augment: n is beyond out_bank's " + std::to_string(out_bank->descs.size()) + " slots");
    int which = 0;
    const int rc = sprite_bank_limits(sprites, &which);
    if (rc != PA_OK) {
        const SynthDesc& d = sprites->descs[(size_t)which];
        return fail(e, rc, "pa_sprite_augment: sprite " + std::to_string(which) + " (" + std::to_string(d.h) + " x " + std::to_string(d.w) +
                               (rc == PA_ERR_CAPACITY ? "): resized to width 128 it is taller than " + std::to_string(PA_SPRITE_H1_MAX) + " (h <= 3.5 w is always taken)"
                                                      : "): resized to width 128 it is empty"));
    }
    if (!e->aug_tabs) return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_augment: the engine has no tables");
    SpriteAugArgs a;
    a.sprite_px = sprites->dev + sprites->table_bytes;
    a.sprite_desc = reinterpret_cast<const SynthDesc*>(sprites->dev);
    a.n_sprites = (int)sprites->descs.size();
    a.params = params_dev;
    a.n = n;
    a.out_px = out_bank->dev + out_bank->table_bytes;
    a.scratch = out_bank->scratch;
    a.workgroups = std::min((int)n, out_bank->scratch_groups);
    a.tabs = e->aug_tabs;
    ProfScope ps(e, (hipStream_t)stream, "sprite_augment", 0.0, (double)n * 65536.0 * 8.0);
    HIPCHK(e, launch_sprite_augment(a, (hipStream_t)stream));
    return PA_OK;
}

int pa_sprite_bank_read(pa_engine* e, const pa_synth_bank* bank, int32_t first, int32_t n, uint8_t* out_host, void* stream) {
    if (!e || !bank || !out_host || !bank->slots || !bank->dev || first < 0 || n < 1 || (int64_t)first + n > (int64_t)bank->descs.size())
        return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_bank_read: a bank of pa_sprite_bank_create with pixels, and a range inside its slots");
    const size_t slot = (size_t)PA_CROP * PA_CROP * 4;
    HIPCHK(e, hipMemcpyAsync(out_host, bank->dev + bank->table_bytes + (size_t)first * slot, (size_t)n * slot, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return PA_OK;
}

// ---- the detector's synthetic training images (sprite_resize.hip, scene_composite.hip) ------------------------------------------

int pa_sprite_resize_params_check(const pa_sprite_resize_params* host, int32_t n, const pa_synth_bank* sprites, const pa_synth_bank* out_bank) {
    if (!host || n < 1 || !sprites || !out_bank || sprites->kind != PA_SYNTH_SPRITES || out_bank->slot_w < 1 || sprites == out_bank)
        return PA_ERR_INVALID_ARG;
    if (n > (int32_t)out_bank->descs.size()) return PA_ERR_CAPACITY;
    for (int32_t i = 0; i < n; ++i) {
        const pa_sprite_resize_params& p = host[i];
        if (p.src < 0 || p.src >= (int32_t)sprites->descs.size() || p.out_w < 1 || p.out_h < 1 || p.reserved != 0) return PA_ERR_INVALID_ARG;
        if (p.out_w > out_bank->slot_w || p.out_h > out_bank->slot_h) return PA_ERR_CAPACITY;
    }
    return PA_OK;
}

int pa_sprite_resize_bank_create(pa_engine* e, int32_t n, int32_t max_w, int32_t max_h, pa_synth_bank** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    pa_synth_bank* b = nullptr;
    try {
        if (n < 1 || n > 65535 || max_w < 1 || max_w > PA_SPRITE_RESIZE_W_MAX || max_h < 1 || max_h > PA_SPRITE_RESIZE_H_MAX)
            return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_resize_bank_create: n is 1..65535, max_w 1.." + std::to_string(PA_SPRITE_RESIZE_W_MAX) +
                                                   ", max_h 1.." + std::to_string(PA_SPRITE_RESIZE_H_MAX));
        b = new pa_synth_bank();
        b->kind = PA_SYNTH_SPRITES;
        b->slot_w = max_w;
        b->slot_h = max_h;
        b->slot_bytes = ((size_t)max_w * max_h * 4 + 15) & ~(size_t)15;
        b->descs.resize((size_t)n);
        for (int32_t k = 0; k < n; ++k) {
            b->descs[(size_t)k].offset = (uint64_t)k * b->slot_bytes;
            b->descs[(size_t)k].w = b->descs[(size_t)k].h = 1;   // a transparent pixel until a call fills the slot
        }
        b->min_w = b->min_h = 1;
        b->table_bytes = ((size_t)n * sizeof(SynthDesc) + 15) & ~(size_t)15;
        if (e) {
            const size_t px_bytes = (size_t)n * b->slot_bytes;
            const size_t bytes = b->table_bytes + px_bytes + (size_t)n * sizeof(pa_sprite_resize_params);
            b->scratch_groups = std::min((int)n, RESIZE_WORKGROUPS_MAX);
            void* p = nullptr;
            hipError_t err = hipMalloc(&p, bytes);
            if (err == hipSuccess) {
                b->dev = static_cast<unsigned char*>(p);
                b->params_dev = reinterpret_cast<pa_sprite_resize_params*>(b->dev + b->table_bytes + px_bytes);
                err = hipMemset(p, 0, bytes);
            }
            if (err == hipSuccess) err = hipMemcpy(p, b->descs.data(), (size_t)n * sizeof(SynthDesc), hipMemcpyHostToDevice);
            if (err == hipSuccess) {
                err = hipMalloc(&p, (size_t)b->scratch_groups * PA_SYNTH_SPRITE_MAX * (size_t)max_w * 4);
                if (err == hipSuccess) b->scratch = static_cast<unsigned char*>(p);
            }
            if (err == hipSuccess) {
                err = hipHostMalloc(&p, (size_t)n * sizeof(pa_sprite_resize_params), hipHostMallocDefault);
                if (err == hipSuccess) b->params_pinned = static_cast<pa_sprite_resize_params*>(p);
            }
            if (err == hipSuccess) err = hipEventCreateWithFlags(&b->staged, hipEventDisableTiming);
            if (err != hipSuccess) {
                pa_synth_bank_destroy(b);
                b = nullptr;
                return fail(e, PA_ERR_HIP, std::string("pa_sprite_resize_bank_create: ") + hipGetErrorString(err));
            }
        }
        *out = b;
        return PA_OK;
    } catch (const std::exception&) {
        pa_synth_bank_destroy(b);
        if (e) e->last_error.clear();
        return PA_ERR_CAPACITY;
    }
}

int pa_sprite_resize(pa_engine* e, const pa_synth_bank* sprites, const pa_sprite_resize_params* params_host, int32_t n, pa_synth_bank* out_bank,
                     void* stream) {
    if (!e || !sprites || !params_host || !out_bank || n < 1 || sprites->kind != PA_SYNTH_SPRITES)
        return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_resize: bad argument (params on the host, n at least 1)");
    if (out_bank->slot_w < 1 || !out_bank->dev || !out_bank->scratch || !out_bank->params_pinned || out_bank == sprites)
        return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_resize: out_bank is a bank of pa_sprite_resize_bank_create, made with an engine, and not the source");
    if (!sprites->dev) return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_resize: a bank that was made without an engine has no pixels");
    if (n > (int32_t)out_bank->descs.size())
        return fail(e, PA_ERR_CAPACITY, "pa_sprite_resize: n is beyond out_bank's " + std::to_string(out_bank->descs.size()) + " slots");
    hipStream_t s = (hipStream_t)stream;
    if (out_bank->staged_pending) {   // the previous call's copy out of the staging area (not its kernel)
        HIPCHK(e, hipEventSynchronize(out_bank->staged));
        out_bank->staged_pending = false;
    }
    std::memcpy(out_bank->params_pinned, params_host, (size_t)n * sizeof(pa_sprite_resize_params));
    HIPCHK(e, hipMemcpyAsync(out_bank->params_dev, out_bank->params_pinned, (size_t)n * sizeof(pa_sprite_resize_params), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipEventRecord(out_bank->staged, s));
    out_bank->staged_pending = true;
    for (int32_t i = 0; i < n; ++i) {   // the host's copy of what the kernel writes into the device's table
        const ResizeRead r = resize_read(params_host[i], (int)sprites->descs.size(), out_bank->slot_w, out_bank->slot_h);
        out_bank->descs[(size_t)i].w = r.ow;
        out_bank->descs[(size_t)i].h = r.oh;
    }
    SpriteResizeArgs a;
    a.sprite_px = sprites->dev + sprites->table_bytes;
    a.sprite_desc = reinterpret_cast<const SynthDesc*>(sprites->dev);
    a.n_sprites = (int)sprites->descs.size();
    a.params = out_bank->params_dev;
    a.n = n;
    a.out_desc = reinterpret_cast<SynthDesc*>(out_bank->dev);
    a.out_px = out_bank->dev + out_bank->table_bytes;
    a.slot_bytes = out_bank->slot_bytes;
    a.max_w = out_bank->slot_w;
    a.max_h = out_bank->slot_h;
    a.scratch = out_bank->scratch;
    a.workgroups = std::min((int)n, out_bank->scratch_groups);
    ProfScope ps(e, s, "sprite_resize", 0.0, 0.0);
    HIPCHK(e, launch_sprite_resize(a, s));
    return PA_OK;
}

int pa_sprite_resize_bank_read(pa_engine* e, const pa_synth_bank* bank, int32_t slot, uint8_t* out_host, size_t capacity, void* stream) {
    if (!e || !bank || !out_host || bank->slot_w < 1 || !bank->dev || slot < 0 || slot >= (int32_t)bank->descs.size())
        return fail(e, PA_ERR_INVALID_ARG, "pa_sprite_resize_bank_read: a bank of pa_sprite_resize_bank_create with pixels, and one of its slots");
    const SynthDesc& d = bank->descs[(size_t)slot];
    const size_t bytes = (size_t)d.w * d.h * 4;
    if (capacity < bytes) return fail(e, PA_ERR_CAPACITY, "pa_sprite_resize_bank_read: the slot holds " + std::to_string(bytes) + " bytes");
    HIPCHK(e, hipMemcpyAsync(out_host, bank->dev + bank->table_bytes + d.offset, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return PA_OK;
}

int pa_scene_params_check(const pa_scene_params* host, int32_t n, const pa_synth_bank* sprites, const pa_synth_bank* stages) {
    if (!host || n < 1 || !sprites || !stages || !sprites->slots || stages->kind != PA_SYNTH_STAGES) return PA_ERR_INVALID_ARG;
    for (int32_t i = 0; i < n; ++i) {
        const pa_scene_params& p = host[i];
        if (p.stage < 0 || p.stage >= (int32_t)stages->descs.size() || p.n_sprites < 0 || p.n_sprites > PA_SCENE_SPRITES_MAX) return PA_ERR_INVALID_ARG;
        if (p.reserved[0] != 0 || p.reserved[1] != 0) return PA_ERR_INVALID_ARG;
        for (int k = 0; k < PA_SCENE_SPRITES_MAX; ++k) {
            const pa_scene_sprite& q = p.sprites[k];
            if (k >= p.n_sprites) {
                if (q.slot != 0 || q.x != 0 || q.y != 0) return PA_ERR_INVALID_ARG;
                continue;
            }
            if (q.slot < 0 || q.slot >= (int32_t)sprites->descs.size()) return PA_ERR_INVALID_ARG;
            if (q.x < -PA_SYNTH_PASTE_MAX || q.x > PA_SYNTH_PASTE_MAX || q.y < -PA_SYNTH_PASTE_MAX || q.y > PA_SYNTH_PASTE_MAX) return PA_ERR_INVALID_ARG;
        }
    }
    return PA_OK;
}

int pa_scene_composite(pa_engine* e, const pa_synth_bank* sprites, const pa_synth_bank* stages, const pa_scene_params* params_dev, int32_t n,
                       uint8_t* images_dev, size_t images_capacity, pa_crop_image* desc_dev, void* stream) {
    if (!e || !sprites || !stages || !params_dev || !images_dev || !desc_dev || n < 1 || n > 65535 || stages->kind != PA_SYNTH_STAGES)
        return fail(e, PA_ERR_INVALID_ARG, "pa_scene_composite: bad argument (n is 1..65535, stages a PA_SYNTH_STAGES bank)");
    if (!sprites->slots) return fail(e, PA_ERR_INVALID_ARG, "pa_scene_composite: sprites is a bank of pa_sprite_bank_create (128 x 128 slots)");
    if (!sprites->dev || !stages->dev) return fail(e, PA_ERR_INVALID_ARG, "pa_scene_composite: a bank that was made without an engine has no pixels");
    if ((uintptr_t)images_dev & 15 || (uintptr_t)params_dev & 7 || (uintptr_t)desc_dev & 7)
        return fail(e, PA_ERR_INVALID_ARG, "pa_scene_composite: images must be 16-byte aligned, params and desc 8-byte aligned");
    uint64_t largest = 0;
    for (const SynthDesc& d : stages->descs) largest = std::max(largest, scene_bytes_padded(d.w, d.h));
    SceneArgs a;
    a.sprite_px = sprites->dev + sprites->table_bytes;
    a.n_slots = (int)sprites->descs.size();
    a.stage_px = stages->dev + stages->table_bytes;
    a.stage_desc = reinterpret_cast<const SynthDesc*>(stages->dev);
    a.n_stages = (int)stages->descs.size();
    a.params = params_dev;
    a.n = n;
    a.images = images_dev;
    a.images_capacity = images_capacity;
    a.desc = desc_dev;
    const uint64_t per_group = 16u * 256u * 4u;   // scene_composite.hip: SCENE_THREADS x SCENE_PIECES pieces of 16 bytes
    a.groups_x = (int)((largest + per_group - 1) / per_group);
    ProfScope ps(e, (hipStream_t)stream, "scene_composite", 0.0, 2.0 * (double)n * (double)largest);
    HIPCHK(e, launch_scene_composite(a, (hipStream_t)stream));
    return PA_OK;
}

}  // extern "C"

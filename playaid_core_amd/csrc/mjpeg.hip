// Motion-JPEG frame decode on the device: baseline JPEG files -> uint8 [n][H][W][3] BGR frames in HBM.
//
// Replaces the per-frame work of cv2.VideoCapture.read / cv2.imread in the reference (playaid/ai_runner.py:153,404-405,446;
// playaid/manuscript.py:154-155) for Motion-JPEG streams and JPEG image sequences. The arithmetic is libjpeg(-turbo)'s with
// its defaults, which is what OpenCV's JPEG reader runs: Huffman entropy decoding (T.81 F.2.2), de-quantisation + the
// slow-but-accurate integer IDCT (jidctint.c), "fancy" triangle-filter chroma up-sampling with libjpeg's edge
// replication (jdsample.c h2v2 / h2v1, jdmainct.c), YCbCr -> RGB (jdcolor.c). Bit-exact against oracle/jpeg.py::decode,
// which is pinned byte for byte against PIL.Image.open (live libjpeg-turbo).
//
// Pipeline per call (a call's frames go in GROUPS, each on a stream of the handle's own; see struct pa_mjpeg):
//   host : marker segments of every frame (SOF0/SOF1, DQT, DHT, DRI, SOS) -> frame descriptors + Huffman / quantisation
//          table sets (consecutive frames with identical tables share one set)
//   copy : the compressed bytes of each group (a copy stream that never waits); descriptors and table sets by
//          stage_copy_kernel out of the pinned staging buffers
//   unstuff_count_kernel / unstuff_write_kernel : the CLEAN stream of every frame (stuffed zeros and RSTm markers taken
//                  out, restart positions recorded)
//   sub_decode_kernel<0|1> + sub_verify_plan_kernel : one lane per subsequence of the clean stream finds the decoder
//                  state at its first bit (self-synchronisation, see below); nothing is stored but states and counts
//   sub_scan_kernel : block index at every subsequence's entry
//   sub_decode_kernel<2> : the final pass stores the non-zero quantised AC coefficients (int16) where the scan puts them
//                  -- block number in scan order, zig-zag index -- and every block's DC DIFFERENCE in an array apart
//   dc_scan_kernel : DC differences -> DC coefficients (running sums per component, from zero at every restart interval)
//   idct_kernel  : one thread per 8x8 block of the component rasters gathers its block from the scan-order buffer
//                  (de-zig-zag by constant indices), block in registers -> uint8 sample planes (padded to whole MCUs)
//   ycc420_kernel / ycc_kernel : up-sampling + colour conversion, 8 pixels x 4 (4:2:0) or FV rows per thread, 8-byte stores
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/playaid_hip.h"
#include "jpeg_entropy.h"

namespace pa {
namespace mj {

struct Geom {
    int32_t ncomp, mcus_x, mcus_y, blocks_per_mcu;
    int32_t hs[3], vs[3];
    int32_t bx[3], by[3];   // padded block raster of each component
    int32_t blk_off[3];     // first block of the component inside a frame's coefficient / sample buffer
    int32_t blocks_per_frame;
    int32_t height, width;
    int32_t fh, fv;         // chroma up-sampling factors (1 | 2)
    int32_t sub_shift;      // log2 of the subsequence size in bytes
    int32_t f0;             // first frame of the launch: a call's frames are decoded in groups, each on a stream of its own
    uint8_t b_comp[MAX_BLOCKS_MCU], b_dy[MAX_BLOCKS_MCU], b_dx[MAX_BLOCKS_MCU];
};

// diagnostics (pa_mjpeg_debug_counters): shader-clock cycles, 100 MHz wall ticks and symbols of one wave's symbol loop
__device__ unsigned long long g_dbg[16];

// Frame descriptors and table sets, pinned host staging -> HBM, read over the link by the device itself. (hipMemcpyAsync
// of a few KB on a stream that has just been told to wait for another stream's event blocked the calling thread for the
// length of a whole decode, every third call, on ROCm 7.2: measured with PA_MJPEG_TRACE.)
__global__ __launch_bounds__(256) void stage_copy_kernel(const uint32_t* __restrict__ a, uint32_t* __restrict__ da, int na,
                                                         const uint32_t* __restrict__ b, uint32_t* __restrict__ db, int nb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < na) da[i] = a[i];
    else if (i - na < nb) db[i - na] = b[i - na];
}

// ---- the passes, one frame of the launch per blockIdx.y / .x / .z (the device code itself: jpeg_entropy.h) -------------------

// chunk_cnt[f][c] = (markers, kept bytes) of chunk c of frame f
__global__ __launch_bounds__(256) void unstuff_count_kernel(const uint8_t* __restrict__ bits, const FrameDesc* __restrict__ fd,
                                                            int2* __restrict__ chunk_cnt, int max_chunks, int f0) {
    const int f = blockIdx.y + f0;
    const FrameDesc d = fd[f];
    unstuff_count_body(bits, d, chunk_cnt + (size_t)f * max_chunks, blockIdx.x);
}

__global__ __launch_bounds__(256) void unstuff_write_kernel(const uint8_t* __restrict__ bits, const FrameDesc* __restrict__ fd,
                                                            const int2* __restrict__ chunk_cnt, int max_chunks,
                                                            uint8_t* __restrict__ clean, uint32_t* __restrict__ seg_start,
                                                            uint32_t* __restrict__ clean_len, int32_t* __restrict__ status, int f0) {
    const int f = blockIdx.y + f0;
    const FrameDesc d = fd[f];
    unstuff_write_body(bits, d, chunk_cnt + (size_t)f * max_chunks, max_chunks, blockIdx.x, clean, seg_start, clean_len + f, status + f);
}

template <int MODE, int LANES = WG_SUBS>
__global__ __launch_bounds__(LANES) void sub_decode_kernel(const uint8_t* __restrict__ clean, const FrameDesc* __restrict__ fd,
                                                         const TableSet* __restrict__ ts, const uint32_t* __restrict__ seg_start,
                                                         const uint32_t* __restrict__ clean_len, const Geom g,
                                                         const uint32_t* __restrict__ g_in, uint32_t* __restrict__ g_out,
                                                         uint32_t* __restrict__ used, SubCnt* __restrict__ cnt,
                                                         const SubCnt* __restrict__ entry, int16_t* __restrict__ coef,
                                                         int32_t* __restrict__ status, int32_t* __restrict__ changed,
                                                         const int32_t* __restrict__ changed_last, const int32_t* __restrict__ todo,
                                                         const int32_t* __restrict__ todo_cnt, int16_t* __restrict__ dcdiff) {
    // verify pass: a frame whose previous verify pass changed nothing has settled (changed_last = that pass's flags)
    if (MODE == 1 && changed_last && changed_last[blockIdx.y + g.f0] == 0) return;
    const int f = blockIdx.y + g.f0;
    const FrameDesc d = fd[f];
    // Huffman table of every block position of an MCU (baseline: two DC, two AC tables), one bit each, wave-uniform:
    // bit b = the DC table of block b, bit 16 + b = its AC table
    uint32_t tabsel = 0;
    for (int bb = 0; bb < g.blocks_per_mcu; ++bb) {
        const int c = g.b_comp[bb];
        tabsel |= (uint32_t)(d.td[c] & 1) << bb;
        tabsel |= (uint32_t)(d.ta[c] & 1) << (16 + bb);
    }
    const int total_blocks = g.mcus_x * g.mcus_y * g.blocks_per_mcu;
    const bool stamp = __builtin_amdgcn_readfirstlane((int)(blockIdx.x == 0 && f == 0 && threadIdx.x < 64)) != 0;
    sub_decode_body<MODE, LANES>(clean, d, ts, seg_start, clean_len[f], g.sub_shift, g.blocks_per_mcu, tabsel, total_blocks, f, blockIdx.x,
                                 g_in, g_out, used, cnt, entry, MODE == 2 ? coef + (size_t)f * total_blocks * 64 : nullptr, status, changed,
                                 changed_last, todo, todo_cnt, MODE == 2 ? dcdiff + (size_t)f * total_blocks : nullptr, stamp, g_dbg);
}

__global__ __launch_bounds__(1024) void sub_verify_plan_kernel(const FrameDesc* __restrict__ fd, const uint32_t* __restrict__ clean_len,
                                                               int sub_shift, const uint32_t* __restrict__ g_in, uint32_t* __restrict__ g_out,
                                                               const uint32_t* __restrict__ used, int32_t* __restrict__ todo,
                                                               int32_t* __restrict__ todo_cnt, const int32_t* __restrict__ changed_last, int f0) {
    const int f = blockIdx.x + f0;
    if (changed_last && changed_last[f] == 0) {  // settled: nothing to do (both state buffers already agree)
        if (threadIdx.x == 0) todo_cnt[f] = 0;
        return;
    }
    const FrameDesc d = fd[f];
    verify_plan_body(d, clean_len[f], sub_shift, g_in, g_out, used, todo, todo_cnt + f);
}

__global__ __launch_bounds__(1024) void sub_scan_kernel(const FrameDesc* __restrict__ fd, const uint32_t* __restrict__ clean_len,
                                                        const SubCnt* __restrict__ cnt, SubCnt* __restrict__ entry, int sub_shift, int f0) {
    const int f = blockIdx.x + f0;
    const FrameDesc d = fd[f];
    sub_scan_body(d, clean_len[f], cnt, entry, sub_shift);
}

// One workgroup per (frame, component)
__global__ __launch_bounds__(1024) void dc_scan_kernel(int16_t* __restrict__ dc, const FrameDesc* __restrict__ fd, const Geom g) {
    const int f = blockIdx.x + g.f0, c = blockIdx.y;
    if (c >= g.ncomp) return;
    const int bpm = g.blocks_per_mcu;
    int b0 = 0, nbc = 0;  // the component's blocks inside an MCU: b0 .. b0 + nbc
    for (int b = 0; b < bpm; ++b) {
        if (g.b_comp[b] == c) {
            if (nbc == 0) b0 = b;
            ++nbc;
        }
    }
    const int mcus = g.mcus_x * g.mcus_y;
    dc_scan_body(dc + (size_t)f * mcus * bpm + b0, fd[f].ri, mcus, bpm, nbc);
}

// One thread per block of the component rasters. Its coefficients lie where the scan put them: block
// mcu * blocks_per_mcu + (position inside the MCU) of the frame, zig-zag order, the DC coefficient in dc[] (dc_scan_kernel).
__global__ __launch_bounds__(256) void idct_kernel(const int16_t* __restrict__ coef, const int16_t* __restrict__ dc,
                                                   const FrameDesc* __restrict__ fd, const TableSet* __restrict__ ts, const Geom g,
                                                   uint8_t* __restrict__ planes, int n_frames) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_frames * g.blocks_per_frame) return;
    const int fl = (int)(t / g.blocks_per_frame), r = (int)(t - (long long)fl * g.blocks_per_frame);
    const int f = fl + g.f0;
    const int c = (g.ncomp > 2 && r >= g.blk_off[2]) ? 2 : ((g.ncomp > 1 && r >= g.blk_off[1]) ? 1 : 0);
    const int off_c = c == 0 ? g.blk_off[0] : (c == 1 ? g.blk_off[1] : g.blk_off[2]);
    const int bx_c = c == 0 ? g.bx[0] : (c == 1 ? g.bx[1] : g.bx[2]);
    const int hs_c = c == 0 ? g.hs[0] : (c == 1 ? g.hs[1] : g.hs[2]);
    const int vs_c = c == 0 ? g.vs[0] : (c == 1 ? g.vs[1] : g.vs[2]);
    const int b0_c = c == 0 ? 0 : (c == 1 ? g.hs[0] * g.vs[0] : g.hs[0] * g.vs[0] + g.hs[1] * g.vs[1]);
    const int rb = r - off_c;
    const int by = rb / bx_c, bx = rb - by * bx_c;
    const int my = by / vs_c, mx = bx / hs_c;
    const size_t sblk = (size_t)f * g.blocks_per_frame + (size_t)(my * g.mcus_x + mx) * g.blocks_per_mcu + b0_c + (by - my * vs_c) * hs_c +
                        (bx - mx * hs_c);  // blocks_per_frame = mcus * blocks_per_mcu: the rasters are padded to whole MCUs
    const uint16_t* __restrict__ q = ts[fd[f].tabset].q[fd[f].tq[c]];
    const int pitch = bx_c * 8;
    uint8_t* dst = planes + ((size_t)f * g.blocks_per_frame + off_c) * 64 + (size_t)(by * 8) * pitch + bx * 8;
    idct_block(reinterpret_cast<const uint4*>(coef + sblk * 64), (int)dc[sblk], q, dst, pitch);
}

// One output row of 8 pixels of frame f
__device__ __forceinline__ void emit_row(const uint8_t* __restrict__ Y, int py, const Geom& g, int f, int y, int x0, bool colour,
                                         const int (&cb)[8], const int (&cr)[8], uint8_t* __restrict__ out, int rgb) {
    emit_row(Y, py, g.height, g.width, y, x0, colour, cb, cr, out + (((size_t)f * g.height + y) * g.width + x0) * 3, rgb);
}

// 8 pixels x FV rows per thread: up-sampling, jdcolor.c's YCbCr -> RGB, three 8-byte stores per row. The 64 lanes of a
// wave are 64 neighbouring groups of one row pair; lanes past the right or bottom edge stay in step (clamped addresses,
// nothing stored): their neighbours take samples from them.
template <int FH, int FV>
__global__ __launch_bounds__(256) void ycc_kernel(const uint8_t* __restrict__ planes, const Geom g, uint8_t* __restrict__ out, int rgb) {
    using namespace dct;
    const int f = blockIdx.z + g.f0, lane = threadIdx.x & 63;
    const int x0r = (blockIdx.x * 64 + lane) * 8, y0r = (blockIdx.y * 4 + (threadIdx.x >> 6)) * FV;
    const bool valid = x0r < g.width && y0r < g.height;
    if (y0r >= g.height) return;  // whole waves
    const int x0 = min(x0r, g.bx[0] * 8 - 8), y0 = y0r;
    const uint8_t* fp = planes + (size_t)f * g.blocks_per_frame * 64;
    const int py = g.bx[0] * 8;
    const uint8_t* Y = fp + (size_t)g.blk_off[0] * 64;
    int cb[FV][8], cr[FV][8];
    const bool colour = g.ncomp == 3;
    if (colour) {
        const int pc = g.bx[1] * 8;
        const int cw = (g.width + FH - 1) / FH, ch = (g.height + FV - 1) / FV;  // jdmaster.c: downsampled_width / _height
        chroma8<FH, FV>(fp + (size_t)g.blk_off[1] * 64, pc, cw, ch, x0, y0, lane, cb);
        chroma8<FH, FV>(fp + (size_t)g.blk_off[2] * 64, pc, cw, ch, x0, y0, lane, cr);
    }
    if (!valid) return;
#pragma unroll
    for (int v = 0; v < FV; ++v) emit_row(Y, py, g, f, y0 + v, x0, colour, cb[v], cr[v], out, rgb);
}

// 4:2:0, the path's own sampling: FOUR output rows (two chroma rows) per thread. The second pair's chroma rows are the
// first pair's shifted by one, so a thread fetches 4 + 4 chroma rows for 4 output rows instead of 6 + 6, and a wave lives
// twice as long behind one round of memory latency.
__global__ __launch_bounds__(256) void ycc420_kernel(const uint8_t* __restrict__ planes, const Geom g, uint8_t* __restrict__ out, int rgb) {
    const int f = blockIdx.z + g.f0, lane = threadIdx.x & 63;
    const int x0r = (blockIdx.x * 64 + lane) * 8, y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 4;
    if (y0 >= g.height) return;  // whole waves
    const bool valid = x0r < g.width;
    const int x0 = min(x0r, g.bx[0] * 8 - 8);
    const uint8_t* fp = planes + (size_t)f * g.blocks_per_frame * 64;
    const int py = g.bx[0] * 8, pc = g.bx[1] * 8;
    const uint8_t* Y = fp + (size_t)g.blk_off[0] * 64;
    const int cw = (g.width + 1) / 2, ch = (g.height + 1) / 2;
    const int cx0 = x0 >> 1, cy = y0 >> 1;
    const int r_m1 = max(cy - 1, 0), r_1 = min(cy + 1, ch - 1), r_2 = min(cy + 2, ch - 1);
    const bool second = y0 + 2 < g.height;  // (then cy + 1 <= ch - 1)
    int cb[4][8], cr[4][8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint8_t* C = fp + (size_t)(c ? g.blk_off[2] : g.blk_off[1]) * 64;
        int a[6], b[6], d[6], e[6];
        chroma_row6(C + (size_t)r_m1 * pc, cx0, cw, pc, lane, a);
        chroma_row6(C + (size_t)cy * pc, cx0, cw, pc, lane, b);
        chroma_row6(C + (size_t)r_1 * pc, cx0, cw, pc, lane, d);
        chroma_row6(C + (size_t)r_2 * pc, cx0, cw, pc, lane, e);
        if (c) {
            h2v2_rows(b, a, d, cx0, cw, cr[0], cr[1]);
            h2v2_rows(d, b, e, cx0, cw, cr[2], cr[3]);
        } else {
            h2v2_rows(b, a, d, cx0, cw, cb[0], cb[1]);
            h2v2_rows(d, b, e, cx0, cw, cb[2], cb[3]);
        }
    }
    if (!valid) return;
#pragma unroll
    for (int v = 0; v < 4; ++v)
        if (v < 2 || second) emit_row(Y, py, g, f, y0 + v, x0, true, cb[v], cr[v], out, rgb);
}

}  // namespace mj
}  // namespace pa

using namespace pa::mj;

namespace {
constexpr int MAX_ROUNDS = 16;  // verify passes enqueued without looking at the result (pa_mjpeg_set_sync_rounds)
constexpr int MAX_GROUPS = 4;   // frame groups of a call, each on its own stream (pa_mjpeg_set_groups)
}

struct pa_mjpeg {
    int device = 0, max_frames = 0, max_h = 0, max_w = 0;
    size_t max_bytes = 0;
    size_t max_blocks = 0;      // per frame
    size_t max_subs = 0, max_segs = 0;
    size_t clean_bytes = 0;     // size of a set's clean stream
    int max_chunks_cap = 0;
    int sync_rounds = 8;
    int sub_shift_override = 0;  // tuning: log2 of the subsequence size, 0 = chosen from the stream
    int wg_lanes = WG_SUBS;      // lanes per workgroup of the entropy passes: 256, or 128 (34.8 KB of LDS instead of 51.7: fits beside two
                                 // workgroups of the fp32 convolution kernel on a CU; PA_MJPEG_WG_LANES)
    // Device scratch, TWO sets used in turn (like the pinned staging below): a call never touches the memory of the call
    // before it, so its first groups start while that call's last groups are still decoding.
    struct Set {
        uint8_t* d_bits = nullptr;
        uint8_t* d_clean = nullptr;
        FrameDesc* d_fd = nullptr;
        TableSet* d_ts = nullptr;
        int2* d_chunk = nullptr;
        uint32_t* d_seg = nullptr;
        uint32_t* d_clean_len = nullptr;
        uint32_t* d_g[2] = {nullptr, nullptr};
        uint32_t* d_used = nullptr;
        SubCnt* d_cnt = nullptr;
        SubCnt* d_entry = nullptr;
        int32_t* d_changed = nullptr;  // [MAX_ROUNDS + 1][max_frames]
        int32_t* d_todo = nullptr;     // [max_subs] compact lane lists of a verify pass
        int32_t* d_todo_cnt = nullptr; // [max_frames]
        int16_t* d_coef = nullptr;
        int16_t* d_dc = nullptr;       // [max_frames][blocks of a frame in scan order] DC differences
        uint8_t* d_planes = nullptr;
        int32_t* d_status = nullptr;
        hipEvent_t done[MAX_GROUPS] = {};  // group g of the set's last call has finished
        bool used = false;
    } set[2];
    // pinned host staging, two sets used in turn
    FrameDesc* h_fd[2] = {nullptr, nullptr};
    TableSet* h_ts[2] = {nullptr, nullptr};
    int32_t* h_flag = nullptr;
    hipEvent_t staged[2] = {nullptr, nullptr};
    // A call's frames are decoded in GROUPS, each on a stream of the handle's own: the entropy passes of a group are bound
    // by instruction issue and by the latency of single waves (late verify passes keep a handful of waves busy), so groups
    // whose phases are out of step fill each other's idle time, and the upload of one group runs under the passes of the
    // group before it. The groups' uploads go one after the other (they share the link anyway), which is what puts their
    // phases out of step. Measured on 64 x 1080p quality-95 frames per call (scripts/mjpeg_rate.py): 16.4 k frames/s with
    // one group (everything on the caller's stream), 22.5 k with two, 20.9 k with three. A caller that keeps several
    // DECODERS busy on streams of its own (bench.py's decode_inclusive: three) gets the same effect at the size of whole
    // calls and should leave each at one group: 28.1 k with three decoders x one group, 22.3 k with three x two.
    hipStream_t gstream[MAX_GROUPS] = {};
    // The uploads have a stream to themselves that never waits for another stream: hipMemcpyAsync on a stream with a
    // pending cross-stream wait blocks the CALLING THREAD until the wait is over (ROCm 7.2, seen with PA_MJPEG_TRACE).
    // What they overwrite -- the set's bytes of two calls ago -- is known to be dead on the host: see `done`.
    hipStream_t copy_stream = nullptr;
    hipEvent_t fork = nullptr, prologue = nullptr, up[MAX_GROUPS] = {};
    int groups = 2;
    bool staged_used[2] = {false, false};
    int turn = 0;
    int last_rounds = 0;
    std::string last_error;
};


extern "C" {

const char* pa_mjpeg_last_error(const pa_mjpeg* h) { return h ? h->last_error.c_str() : "null handle"; }

void pa_mjpeg_destroy(pa_mjpeg* h) {
    if (!h) return;
    for (auto& S : h->set) {
        void* dev[] = {S.d_bits, S.d_clean, S.d_fd, S.d_ts, S.d_chunk, S.d_seg, S.d_clean_len, S.d_g[0], S.d_g[1], S.d_used,
                       S.d_cnt, S.d_entry, S.d_changed, S.d_todo, S.d_todo_cnt, S.d_coef, S.d_dc, S.d_planes, S.d_status};
        for (void* p : dev) (void)hipFree(p);
        for (hipEvent_t e : S.done)
            if (e) (void)hipEventDestroy(e);
    }
    for (int i = 0; i < 2; ++i) {
        if (h->h_fd[i]) (void)hipHostFree(h->h_fd[i]);
        if (h->h_ts[i]) (void)hipHostFree(h->h_ts[i]);
        if (h->staged[i]) (void)hipEventDestroy(h->staged[i]);
    }
    if (h->h_flag) (void)hipHostFree(h->h_flag);
    for (int g = 0; g < MAX_GROUPS; ++g) {
        if (h->gstream[g]) {
            (void)hipStreamSynchronize(h->gstream[g]);
            (void)hipStreamDestroy(h->gstream[g]);
        }
        if (h->up[g]) (void)hipEventDestroy(h->up[g]);
    }
    if (h->copy_stream) {
        (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamDestroy(h->copy_stream);
    }
    if (h->fork) (void)hipEventDestroy(h->fork);
    if (h->prologue) (void)hipEventDestroy(h->prologue);
    delete h;
}

int pa_mjpeg_create(int32_t device, int32_t max_frames, int32_t max_height, int32_t max_width, size_t max_bytes, pa_mjpeg** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_frames < 1 || max_height < 1 || max_width < 1 || max_height > 65535 || max_width > 65535 || max_bytes < 1024 ||
        max_bytes > 0xe0000000ull)
        return PA_ERR_INVALID_ARG;
    pa_mjpeg* h = new pa_mjpeg();
    *out = h;  // handed back on failure too (pa_mjpeg_last_error, then pa_mjpeg_destroy)
    h->device = device; h->max_frames = max_frames; h->max_h = max_height; h->max_w = max_width; h->max_bytes = max_bytes;
    if (const char* e = getenv("PA_MJPEG_SUB_SHIFT")) h->sub_shift_override = atoi(e);  // tuning knob (scripts/mjpeg_rate.py)
    auto chk = [&](hipError_t e, const char* what) -> bool {
        if (e == hipSuccess) return true;
        h->last_error = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    if (!chk(hipSetDevice(device), "hipSetDevice")) return PA_ERR_NO_DEVICE;
    // worst case: three full-resolution components, padded to 16-pixel MCUs
    const size_t bw = ((size_t)max_width + 15) / 16 * 2, bh = ((size_t)max_height + 15) / 16 * 2;
    const size_t n = (size_t)max_frames;
    h->max_blocks = 3 * bw * bh;
    h->max_chunks_cap = (int)(max_bytes / CHUNK) + 3;
    h->max_subs = max_bytes / SUB_MIN + 2 * n + 2;
    h->max_segs = n * bw * bh + n;
    const size_t clean_bytes = max_bytes + 32 * n + 4096;
    h->clean_bytes = clean_bytes;
    if (const char* e = getenv("PA_MJPEG_GROUPS")) h->groups = atoi(e);  // tuning knob (scripts/mjpeg_rate.py)
    if (const char* e = getenv("PA_MJPEG_WG_LANES")) h->wg_lanes = atoi(e) == 128 ? 128 : WG_SUBS;
    h->groups = h->groups < 1 ? 1 : (h->groups > MAX_GROUPS ? MAX_GROUPS : h->groups);
    for (auto& S : h->set) {
        if (!chk(hipMalloc(&S.d_bits, max_bytes + 64), "hipMalloc bitstream")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_clean, clean_bytes), "hipMalloc clean stream")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_fd, n * sizeof(FrameDesc)), "hipMalloc descriptors")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_ts, n * sizeof(TableSet)), "hipMalloc tables")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_chunk, (n * h->max_chunks_cap) * sizeof(int2)), "hipMalloc chunk counts")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_seg, h->max_segs * sizeof(uint32_t)), "hipMalloc restart positions")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_clean_len, n * sizeof(uint32_t)), "hipMalloc clean lengths")) return PA_ERR_HIP;
        for (int i = 0; i < 2; ++i)
            if (!chk(hipMalloc(&S.d_g[i], h->max_subs * sizeof(uint32_t)), "hipMalloc states")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_used, h->max_subs * sizeof(uint32_t)), "hipMalloc states")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_cnt, h->max_subs * sizeof(SubCnt)), "hipMalloc counts")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_entry, h->max_subs * sizeof(SubCnt)), "hipMalloc entries")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_changed, (MAX_ROUNDS + 1) * n * sizeof(int32_t)), "hipMalloc flags")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_todo, h->max_subs * sizeof(int32_t)), "hipMalloc lane lists")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_todo_cnt, n * sizeof(int32_t)), "hipMalloc lane counts")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_coef, n * h->max_blocks * 64 * sizeof(int16_t)), "hipMalloc coefficients")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_dc, n * h->max_blocks * sizeof(int16_t)), "hipMalloc DC differences")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_planes, n * h->max_blocks * 64), "hipMalloc sample planes")) return PA_ERR_HIP;
        if (!chk(hipMalloc(&S.d_status, n * sizeof(int32_t)), "hipMalloc status")) return PA_ERR_HIP;
        if (!chk(hipMemset(S.d_bits, 0, max_bytes + 64), "hipMemset")) return PA_ERR_HIP;
        if (!chk(hipMemset(S.d_clean, 0, clean_bytes), "hipMemset")) return PA_ERR_HIP;
        for (int g = 0; g < MAX_GROUPS; ++g)
            if (!chk(hipEventCreateWithFlags(&S.done[g], hipEventDisableTiming), "hipEventCreate")) return PA_ERR_HIP;
    }
    for (int i = 0; i < 2; ++i) {
        if (!chk(hipHostMalloc(&h->h_fd[i], n * sizeof(FrameDesc)), "hipHostMalloc")) return PA_ERR_HIP;
        if (!chk(hipHostMalloc(&h->h_ts[i], n * sizeof(TableSet)), "hipHostMalloc")) return PA_ERR_HIP;
        if (!chk(hipEventCreateWithFlags(&h->staged[i], hipEventDisableTiming), "hipEventCreate")) return PA_ERR_HIP;
    }
    // A/B knob PA_MJPEG_PRIO=1: the groups' streams at the device's greatest priority (the entropy passes are chains of
    // short, thinly occupied kernels; beside a detector that fills every CU they wait for a slot at each link of the chain)
    int prio = 0;
    if (const char* e = std::getenv("PA_MJPEG_PRIO")) {
        int least = 0, greatest = 0;
        if (std::atoi(e) > 0 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) prio = greatest;
    }
    for (int g = 0; g < MAX_GROUPS; ++g) {
        if (!chk(hipStreamCreateWithPriority(&h->gstream[g], hipStreamNonBlocking, prio), "hipStreamCreate")) return PA_ERR_HIP;
        if (!chk(hipEventCreateWithFlags(&h->up[g], hipEventDisableTiming), "hipEventCreate")) return PA_ERR_HIP;
    }
    if (!chk(hipStreamCreateWithPriority(&h->copy_stream, hipStreamNonBlocking, prio), "hipStreamCreate")) return PA_ERR_HIP;
    if (!chk(hipEventCreateWithFlags(&h->fork, hipEventDisableTiming), "hipEventCreate")) return PA_ERR_HIP;
    if (!chk(hipEventCreateWithFlags(&h->prologue, hipEventDisableTiming), "hipEventCreate")) return PA_ERR_HIP;
    if (!chk(hipHostMalloc(&h->h_flag, n * sizeof(int32_t)), "hipHostMalloc")) return PA_ERR_HIP;
    return PA_OK;
}

int pa_mjpeg_probe(const uint8_t* data_host, size_t nbytes, int32_t* info8, char* why, size_t why_bytes) {
    if (!data_host || !info8) return PA_ERR_INVALID_ARG;
    Parsed P;
    const char* msg = parse_header(data_host, nbytes, P);
    if (why && why_bytes) snprintf(why, why_bytes, "%s", msg ? msg : "");
    if (msg) return PA_ERR_INVALID_ARG;
    int hmax = 1, vmax = 1;
    for (int c = 0; c < P.ncomp; ++c) {
        hmax = P.h[c] > hmax ? P.h[c] : hmax;
        vmax = P.v[c] > vmax ? P.v[c] : vmax;
    }
    info8[0] = P.height; info8[1] = P.width; info8[2] = P.ncomp; info8[3] = hmax; info8[4] = vmax; info8[5] = P.ri;
    info8[6] = (int32_t)P.scan_off; info8[7] = 0;
    return PA_OK;
}

int pa_mjpeg_set_sync_rounds(pa_mjpeg* h, int32_t rounds) {
    if (!h || rounds < 0 || rounds > MAX_ROUNDS) return PA_ERR_INVALID_ARG;
    h->sync_rounds = rounds;
    return PA_OK;
}

int pa_mjpeg_last_sync_rounds(const pa_mjpeg* h) { return h ? h->last_rounds : 0; }

int pa_mjpeg_set_groups(pa_mjpeg* h, int32_t groups) {
    if (!h || groups < 1 || groups > MAX_GROUPS) return PA_ERR_INVALID_ARG;
    h->groups = groups;
    return PA_OK;
}

int pa_mjpeg_debug_counters(unsigned long long* out8_host) {
    if (!out8_host) return PA_ERR_INVALID_ARG;
    return hipMemcpyFromSymbol(out8_host, HIP_SYMBOL(g_dbg), 16 * sizeof(unsigned long long)) == hipSuccess ? PA_OK : PA_ERR_HIP;
}

int pa_mjpeg_decode(pa_mjpeg* h, const uint8_t* data_host, const int64_t* spans_host, int32_t n, int32_t height, int32_t width,
                    int32_t rgb, uint8_t* frames_dev, int32_t* status_dev, void* stream) {
    if (!h) return PA_ERR_INVALID_ARG;
    auto bad = [&](int code, const std::string& msg) { h->last_error = msg; return code; };
    if (!data_host || !spans_host || !frames_dev || n < 1 || height < 1 || width < 1)
        return bad(PA_ERR_INVALID_ARG, "pa_mjpeg_decode: bad argument");
    if (n > h->max_frames) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: more frames than max_frames");
    if (height > h->max_h || width > h->max_w) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: frame larger than max_height x max_width");
    // one copy moves the byte range that covers every frame of the call
    int64_t base = spans_host[0], top = spans_host[1];
    for (int f = 0; f < n; ++f) {
        const int64_t o = spans_host[2 * f], e = spans_host[2 * f + 1];
        if (o < 0 || e <= o) return bad(PA_ERR_INVALID_ARG, "pa_mjpeg_decode: frame " + std::to_string(f) + " has an empty or negative byte span");
        base = o < base ? o : base;
        top = e > top ? e : top;
    }
    const int64_t total = top - base;
    if ((size_t)total > h->max_bytes) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: compressed bytes exceed max_bytes");
    hipStream_t s = (hipStream_t)stream;
    auto chk = [&](hipError_t e, const char* what) -> bool {
        if (e == hipSuccess) return true;
        h->last_error = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    static const bool trace = getenv("PA_MJPEG_TRACE") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_in = now();
    double t_mark[8] = {0};
    if (!chk(hipSetDevice(h->device), "hipSetDevice")) return PA_ERR_HIP;
    const int k = h->turn;
    h->turn ^= 1;
    if (h->staged_used[k] && !chk(hipEventSynchronize(h->staged[k]), "hipEventSynchronize")) return PA_ERR_HIP;
    // the set's call before last has finished (at most two calls are in flight): nothing enqueued below has to wait for it
    if (h->set[k].used)
        for (int o = 0; o < MAX_GROUPS; ++o)
            if (!chk(hipEventSynchronize(h->set[k].done[o]), "hipEventSynchronize")) return PA_ERR_HIP;
    t_mark[0] = now();
    FrameDesc* fd = h->h_fd[k];
    TableSet* ts = h->h_ts[k];
    Geom g;
    memset(&g, 0, sizeof g);
    Parsed first, prev, cur;
    int n_sets = 0;
    size_t seg_total = 0, sub_total = 0, clean_total = 0;
    uint32_t max_scan = 0;
    int max_sub = 1;
    for (int f = 0; f < n; ++f) {
        const int64_t o = spans_host[2 * f], e = spans_host[2 * f + 1];
        const char* msg = parse_header(data_host + o, (size_t)(e - o), cur);
        if (msg) return bad(PA_ERR_INVALID_ARG, "pa_mjpeg_decode: frame " + std::to_string(f) + ": " + msg);
        if (cur.height != height || cur.width != width)
            return bad(PA_ERR_INVALID_ARG, "pa_mjpeg_decode: frame " + std::to_string(f) + " is " + std::to_string(cur.width) + "x" +
                                               std::to_string(cur.height) + ", the call said " + std::to_string(width) + "x" +
                                               std::to_string(height));
        if (f == 0) {
            first = cur;
            g.ncomp = cur.ncomp;
            int hmax = 1, vmax = 1;
            for (int c = 0; c < cur.ncomp; ++c) {
                hmax = cur.h[c] > hmax ? cur.h[c] : hmax;
                vmax = cur.v[c] > vmax ? cur.v[c] : vmax;
            }
            if (cur.ncomp == 3) {
                const bool ok = cur.h[0] == hmax && cur.v[0] == vmax && cur.h[1] == cur.h[2] && cur.v[1] == cur.v[2] && cur.h[1] == 1 &&
                                cur.v[1] == 1 && ((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2));
                if (!ok) return bad(PA_ERR_INVALID_ARG, "pa_mjpeg_decode: chroma sampling other than 4:4:4 / 4:2:2 / 4:2:0");
            }
            const bool single = cur.ncomp == 1;  // T.81 A.2.2: a one-component scan is not interleaved
            g.mcus_x = (width + 8 * (single ? 1 : hmax) - 1) / (8 * (single ? 1 : hmax));
            g.mcus_y = (height + 8 * (single ? 1 : vmax) - 1) / (8 * (single ? 1 : vmax));
            g.fh = hmax; g.fv = vmax;
            int nb = 0, off = 0;
            for (int c = 0; c < cur.ncomp; ++c) {
                g.hs[c] = single ? 1 : cur.h[c];
                g.vs[c] = single ? 1 : cur.v[c];
                g.bx[c] = g.mcus_x * g.hs[c];
                g.by[c] = g.mcus_y * g.vs[c];
                g.blk_off[c] = off;
                off += g.bx[c] * g.by[c];
                for (int v = 0; v < g.vs[c]; ++v)
                    for (int x = 0; x < g.hs[c]; ++x, ++nb) {
                        g.b_comp[nb] = (uint8_t)c; g.b_dy[nb] = (uint8_t)v; g.b_dx[nb] = (uint8_t)x;
                    }
            }
            g.blocks_per_mcu = nb;
            g.blocks_per_frame = off;
            g.height = height; g.width = width;
            if ((size_t)off > h->max_blocks) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: block raster exceeds the handle's capacity");
        } else {
            bool same = cur.ncomp == first.ncomp;
            for (int c = 0; same && c < cur.ncomp; ++c) same = cur.h[c] == first.h[c] && cur.v[c] == first.v[c];
            if (!same) return bad(PA_ERR_INVALID_ARG, "pa_mjpeg_decode: frame " + std::to_string(f) + " changes the sampling factors");
        }
        // tables: consecutive frames with identical DQT / DHT content share one device table set
        bool share = f > 0;
        if (share) share = memcmp(cur.q, prev.q, sizeof cur.q) == 0 && memcmp(cur.counts, prev.counts, sizeof cur.counts) == 0 &&
                           memcmp(cur.syms, prev.syms, sizeof cur.syms) == 0 && memcmp(cur.hdef, prev.hdef, sizeof cur.hdef) == 0;
        if (!share) {
            TableSet& T = ts[n_sets++];
            memset(&T.h, 0, sizeof T.h);
            for (int t = 0; t < 4; ++t)
                if (cur.hdef[t]) build_hufftab(T.h, t, cur.counts[t], cur.syms[t]);
            memcpy(T.q, cur.q, sizeof T.q);
        }
        prev = cur;
        FrameDesc& d = fd[f];
        memset(&d, 0, sizeof d);
        // the entropy-coded segment ends in front of the EOI marker (fill bytes / container padding may follow it)
        int64_t end = e;
        while (end - o > (int64_t)cur.scan_off + 2 && !(data_host[end - 2] == 0xff && data_host[end - 1] == 0xd9) && e - end < 16) --end;
        if (data_host[end - 2] == 0xff && data_host[end - 1] == 0xd9) end -= 2; else end = e;
        d.scan_off = (uint32_t)(o - base + (int64_t)cur.scan_off);
        d.scan_len = (uint32_t)((end - o) - (int64_t)cur.scan_off);
        d.ri = cur.ri;
        const int mcus = g.mcus_x * g.mcus_y;
        d.n_int = cur.ri ? (mcus + cur.ri - 1) / cur.ri : 1;
        d.seg_base = (int32_t)seg_total;
        seg_total += (size_t)d.n_int;
        d.sub_base = (int32_t)sub_total;

        d.clean_off = (uint32_t)clean_total;
        clean_total += ((size_t)d.scan_len + 31) & ~(size_t)15;
        d.tabset = n_sets - 1;
        for (int c = 0; c < cur.ncomp; ++c) {
            d.td[c] = (uint8_t)cur.td[c]; d.ta[c] = (uint8_t)cur.ta[c]; d.tq[c] = (uint8_t)cur.tq[c];
        }
        max_scan = d.scan_len > max_scan ? d.scan_len : max_scan;
    }
    // subsequence size: about four MCUs of the stream, a power of two. Measured at 1080p / quality 95 (1 MB per frame,
    // scripts/mjpeg_sync_probe.py, scripts/mjpeg_rate.py): the slowest lanes need about ten MCUs to fall into step, i.e.
    // two verify passes at 1024 bytes, three at 512, eleven at 128; a lane's symbol takes ~1000 cycles whether one or two
    // waves share its SIMD (~115 instructions, one LDS round trip), so 512-byte lanes (two waves per SIMD) finish a
    // pass in half the time of 1024-byte lanes and win although they need one more pass: 5.0 vs 5.8 ms per 64 frames.
    {
        size_t bytes = 0;
        for (int f = 0; f < n; ++f) bytes += fd[f].scan_len;
        const size_t per_mcu = bytes / ((size_t)n * g.mcus_x * g.mcus_y) + 1;
        int sh = 8;  // the power of two nearest to four MCUs, 256 bytes .. 8 KB
        while ((3u << sh) / 2 < 4 * per_mcu && sh < 13) ++sh;
        if (h->sub_shift_override >= 7 && h->sub_shift_override <= 13) sh = h->sub_shift_override;
        g.sub_shift = sh;
        for (int f = 0; f < n; ++f) {
            FrameDesc& d = fd[f];
            d.sub_base = (int32_t)sub_total;
            d.n_sub_cap = (int32_t)(((d.scan_len + (1u << sh) - 1) >> sh) + 1);
            sub_total += (size_t)d.n_sub_cap;
            max_sub = d.n_sub_cap > max_sub ? d.n_sub_cap : max_sub;
        }
    }
    t_mark[1] = now();
    const int max_chunks = (int)(max_scan / CHUNK) + 2;
    if (max_chunks > h->max_chunks_cap) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: scan longer than the handle's chunk table");
    if (seg_total > h->max_segs || sub_total > h->max_subs) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: more restart intervals / subsequences than the handle holds");
    // spans may overlap or repeat (the same frame several times): what bounds the clean stream is the SUM of the scans, not
    // the byte range the spans cover
    if (clean_total + 4096 > h->clean_bytes) return bad(PA_ERR_CAPACITY, "pa_mjpeg_decode: the frames' entropy-coded segments add up to more than max_bytes");
    pa_mjpeg::Set& S = h->set[k];
    // exact mode looks at flags on the host between passes: one group, on the caller's stream
    const int G = h->sync_rounds > 0 ? (h->groups < n ? h->groups : n) : 1;
    const bool forked = G > 1;
    // Nothing below depends on what the caller's stream holds except the WRITES of the decoded frames (the caller may
    // still be reading the output buffer): the groups wait for `fork` only in front of their last kernel, so a call's
    // entropy passes start while the call before it -- which the caller's stream has to wait for -- is still decoding.
    if (forked && !chk(hipEventRecord(h->fork, s), "hipEventRecord")) return PA_ERR_HIP;
    hipStream_t q0 = forked ? h->gstream[0] : s;
    // descriptors and tables -> HBM, flags cleared: on the first group's stream, which the other groups wait for
    {
        static_assert(sizeof(FrameDesc) % 4 == 0 && sizeof(TableSet) % 4 == 0, "copied as dwords");
        const int na = (int)((size_t)n * sizeof(FrameDesc) / 4), nb = (int)((size_t)n_sets * sizeof(TableSet) / 4);
        hipLaunchKernelGGL(stage_copy_kernel, dim3((na + nb + 255) / 256), dim3(256), 0, q0, reinterpret_cast<const uint32_t*>(fd),
                           reinterpret_cast<uint32_t*>(S.d_fd), na, reinterpret_cast<const uint32_t*>(ts),
                           reinterpret_cast<uint32_t*>(S.d_ts), nb);
    }
    if (!chk(hipEventRecord(h->staged[k], q0), "hipEventRecord")) return PA_ERR_HIP;
    h->staged_used[k] = true;
    t_mark[2] = now();
    if (!chk(hipMemsetAsync(S.d_status, 0, (size_t)n * sizeof(int32_t), q0), "clear status")) return PA_ERR_HIP;
    if (!chk(hipMemsetAsync(S.d_changed, 0, (size_t)(MAX_ROUNDS + 1) * h->max_frames * sizeof(int32_t), q0), "clear flags")) return PA_ERR_HIP;
    if (forked && !chk(hipEventRecord(h->prologue, q0), "hipEventRecord")) return PA_ERR_HIP;
    t_mark[3] = now();
    const int total_blocks = g.mcus_x * g.mcus_y * g.blocks_per_mcu;
    int rounds_run = 0;
    // the groups' compressed bytes (the byte range that covers a group's frames), one group after the other
    for (int gi = 0; gi < G; ++gi) {
        const int f0 = (int)((long long)n * gi / G), f1 = (int)((long long)n * (gi + 1) / G);
        hipStream_t cq = forked ? h->copy_stream : s;
        int64_t gb = spans_host[2 * f0], gt = spans_host[2 * f0 + 1];
        for (int f = f0; f < f1; ++f) {
            gb = spans_host[2 * f] < gb ? spans_host[2 * f] : gb;
            gt = spans_host[2 * f + 1] > gt ? spans_host[2 * f + 1] : gt;
        }
        if (!chk(hipMemcpyAsync(S.d_bits + (gb - base), data_host + gb, (size_t)(gt - gb), hipMemcpyHostToDevice, cq), "upload bitstream")) return PA_ERR_HIP;
        // readers run a few bytes past the end of a scan: zeros behind the last byte of the call
        if (gt == top && !chk(hipMemsetAsync(S.d_bits + total, 0, 64, cq), "pad bitstream")) return PA_ERR_HIP;
        if (forked && !chk(hipEventRecord(h->up[gi], cq), "hipEventRecord")) return PA_ERR_HIP;
    }
    for (int gi = 0; gi < G; ++gi) {
        const int f0 = (int)((long long)n * gi / G), f1 = (int)((long long)n * (gi + 1) / G), ng = f1 - f0;
        hipStream_t q = forked ? h->gstream[gi] : s;
        Geom gg = g;
        gg.f0 = f0;
        if (gi > 0 && !chk(hipStreamWaitEvent(q, h->prologue, 0), "hipStreamWaitEvent")) return PA_ERR_HIP;
        // the group's coefficient buffers, cleared while its bytes are still on their way
        if (!chk(hipMemsetAsync(S.d_coef + (size_t)f0 * total_blocks * 64, 0, (size_t)ng * total_blocks * 64 * sizeof(int16_t), q), "clear coefficients")) return PA_ERR_HIP;
        if (!chk(hipMemsetAsync(S.d_dc + (size_t)f0 * total_blocks, 0, (size_t)ng * total_blocks * sizeof(int16_t), q), "clear DC differences")) return PA_ERR_HIP;
        if (forked && !chk(hipStreamWaitEvent(q, h->up[gi], 0), "hipStreamWaitEvent")) return PA_ERR_HIP;
        hipLaunchKernelGGL(unstuff_count_kernel, dim3(max_chunks, ng), dim3(256), 0, q, S.d_bits, S.d_fd, S.d_chunk, max_chunks, f0);
        hipLaunchKernelGGL(unstuff_write_kernel, dim3(max_chunks, ng), dim3(256), 0, q, S.d_bits, S.d_fd, S.d_chunk, max_chunks, S.d_clean,
                           S.d_seg, S.d_clean_len, S.d_status, f0);
        const int wl = h->wg_lanes;
        const dim3 sgrid((max_sub + wl - 1) / wl, ng);
        int cur_g = 0;
#define MJ_LAUNCH(MODE_, ...)                                                                                         \
    do {                                                                                                              \
        if (wl == 128) hipLaunchKernelGGL((sub_decode_kernel<MODE_, 128>), sgrid, dim3(128), 0, q, __VA_ARGS__);      \
        else hipLaunchKernelGGL((sub_decode_kernel<MODE_, WG_SUBS>), sgrid, dim3(WG_SUBS), 0, q, __VA_ARGS__);        \
    } while (0)
        MJ_LAUNCH(0, S.d_clean, S.d_fd, S.d_ts, S.d_seg, S.d_clean_len, gg,
                  (const uint32_t*)nullptr, S.d_g[0], S.d_used, S.d_cnt, (const SubCnt*)nullptr, (int16_t*)nullptr, S.d_status,
                  (int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (int16_t*)nullptr);
        auto verify = [&](int slot, int prev_slot) {
            int32_t* flag = S.d_changed + (size_t)slot * h->max_frames;
            const int32_t* prev = prev_slot >= 0 ? S.d_changed + (size_t)prev_slot * h->max_frames : nullptr;
            hipLaunchKernelGGL(sub_verify_plan_kernel, dim3(ng), dim3(1024), 0, q, S.d_fd, S.d_clean_len, g.sub_shift, S.d_g[cur_g],
                               S.d_g[cur_g ^ 1], S.d_used, S.d_todo, S.d_todo_cnt, prev, f0);
            MJ_LAUNCH(1, S.d_clean, S.d_fd, S.d_ts, S.d_seg, S.d_clean_len, gg,
                      S.d_g[cur_g], S.d_g[cur_g ^ 1], S.d_used, S.d_cnt, (const SubCnt*)nullptr, (int16_t*)nullptr, S.d_status, flag,
                      prev, S.d_todo, S.d_todo_cnt, (int16_t*)nullptr);
            cur_g ^= 1;
        };
        int last_slot = MAX_ROUNDS;  // an all-zero row unless a verify pass wrote it
        if (h->sync_rounds > 0) {
            for (int r = 0; r < h->sync_rounds; ++r) verify(r, r - 1);
            last_slot = h->sync_rounds - 1;
            rounds_run = h->sync_rounds;
        } else {
            // exact mode: verify until a pass changes nothing, looking at the flags on the host (synchronises the stream)
            int rounds = 0;
            for (;;) {
                if (!chk(hipMemsetAsync(S.d_changed, 0, (size_t)h->max_frames * sizeof(int32_t), q), "clear flags")) return PA_ERR_HIP;
                verify(0, -1);
                ++rounds;
                if (!chk(hipMemcpyAsync(h->h_flag, S.d_changed, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, q), "read flags")) return PA_ERR_HIP;
                if (!chk(hipStreamSynchronize(q), "hipStreamSynchronize")) return PA_ERR_HIP;
                bool any = false;
                for (int f = 0; f < n; ++f) any = any || h->h_flag[f] != 0;
                if (!any) break;
                if (rounds > max_sub + 2) return bad(PA_ERR_HIP, "pa_mjpeg_decode: synchronisation did not settle");
            }
            last_slot = 0;
            rounds_run = rounds;
        }
        hipLaunchKernelGGL(sub_scan_kernel, dim3(ng), dim3(1024), 0, q, S.d_fd, S.d_clean_len, S.d_cnt, S.d_entry, g.sub_shift, f0);
        MJ_LAUNCH(2, S.d_clean, S.d_fd, S.d_ts, S.d_seg, S.d_clean_len, gg,
                  S.d_g[cur_g], (uint32_t*)nullptr, S.d_used, S.d_cnt, S.d_entry, S.d_coef, S.d_status, (int32_t*)nullptr,
                  S.d_changed + (size_t)last_slot * h->max_frames, (const int32_t*)nullptr, (const int32_t*)nullptr, S.d_dc);
#undef MJ_LAUNCH
        hipLaunchKernelGGL(dc_scan_kernel, dim3(ng, g.ncomp), dim3(1024), 0, q, S.d_dc, S.d_fd, gg);
        const long long nblk = (long long)ng * g.blocks_per_frame;
        hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, q, S.d_coef, S.d_dc, S.d_fd, S.d_ts, gg, S.d_planes, ng);
        const int fv = g.ncomp == 3 ? g.fv : 1, fhh = g.ncomp == 3 ? g.fh : 1;
        const dim3 grid((width + 511) / 512, (height + 4 * fv - 1) / (4 * fv), ng);
        if (forked && !chk(hipStreamWaitEvent(q, h->fork, 0), "hipStreamWaitEvent")) return PA_ERR_HIP;  // the output buffer is the caller's
        if (fhh == 2 && fv == 2)
            hipLaunchKernelGGL(ycc420_kernel, dim3((width + 511) / 512, (height + 15) / 16, ng), dim3(256), 0, q, S.d_planes, gg, frames_dev, rgb);
        else if (fhh == 2) hipLaunchKernelGGL((ycc_kernel<2, 1>), grid, dim3(256), 0, q, S.d_planes, gg, frames_dev, rgb);
        else hipLaunchKernelGGL((ycc_kernel<1, 1>), grid, dim3(256), 0, q, S.d_planes, gg, frames_dev, rgb);
        if (!chk(hipEventRecord(S.done[gi], q), "hipEventRecord")) return PA_ERR_HIP;
    }
    // groups the call did not use: their events must not hold a later call back with a stale record
    for (int gi = G; gi < MAX_GROUPS; ++gi)
        if (!chk(hipEventRecord(S.done[gi], s), "hipEventRecord")) return PA_ERR_HIP;
    S.used = true;
    h->last_rounds = rounds_run;
    if (forked)
        for (int gi = 0; gi < G; ++gi)
            if (!chk(hipStreamWaitEvent(s, S.done[gi], 0), "hipStreamWaitEvent")) return PA_ERR_HIP;
    if (status_dev && !chk(hipMemcpyAsync(status_dev, S.d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s), "copy status"))
        return PA_ERR_HIP;
    if (!chk(hipGetLastError(), "kernel launch")) return PA_ERR_HIP;
    if (trace)
        fprintf(stderr, "pa_mjpeg_decode host us: staging wait %.0f, headers %.0f, descriptors %.0f, clears %.0f, groups (copies + launches) %.0f\n",
                t_mark[0] - t_in, t_mark[1] - t_mark[0], t_mark[2] - t_mark[1], t_mark[3] - t_mark[2], now() - t_mark[3]);
    return PA_OK;
}

}  // extern "C"

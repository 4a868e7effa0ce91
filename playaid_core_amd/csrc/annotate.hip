// The annotator's drawing step on frames in HBM (pa_annotate_frames, include/playaid_hip.h): what the reference's
// Annotator.box_label does with Pillow per frame (playaid/annotator.py:103-145) -- ImageDraw.rectangle(outline=, width=),
// ImageDraw.rectangle(fill=), ImageDraw.text(bitmap font, white) -- and maybe_pad_image's np.pad, as ONE pass over n frames.
//
// The pass is a copy: a thread owns a run of 16 output pixels (48 bytes: three 16-byte loads and stores where the row pitches
// allow it, bytes otherwise). A workgroup works inside one frame; it derives the frame's draw list once into LDS -- per item
// the outline's strokes, the background rectangle, the text origin and ONE rectangle bounding everything the item can touch,
// clipped to the frame. A run that misses every bounding rectangle (nearly all of a frame) is stored as loaded; a run that
// hits one evaluates its 16 pixels against the items it hit, in list order (painter's order).
//
// Pillow's outlined rectangle (ImagingDrawRectangle, fill = 0), stated per pixel. With y0 <= y1 (the routine swaps them) and
// i = 0 .. width - 1 it draws hline(x0, y0 + i, x1), hline(x0, y1 - i, x1), line(x1 - i, y0 + width, x1 - i, y1 - width + 1)
// and line(x0 + i, ...same rows). hline orders its ends; a vertical `line` from row a to row b paints |b - a| pixels starting
// AT a and walking towards b -- it leaves out its end point. So the vertical strokes cover rows [a, b - 1] when b >= a
// (a roomy box: exactly the rows between the horizontal bands) and rows [b + 1, a] when b < a (a box thinner than twice the
// width: the stroke walks upwards from y0 + width, which can lie below y1, outside the box). tests/test_annotate_host.py
// pins annotator.outline_mask, which states the same rule, against live Pillow on every box of a 20 x 20 grid.
//
// Text: Pillow's bitmap font has only 0 / 255 in its masks, so a text pixel is the ink or untouched -- no blending. Cell k of
// a string is atlas[c_k][c_k+1] (the last column of a glyph's cell depends on the next character, a quirk of how Pillow pastes
// glyphs), the last cell atlas[c][n_chars].
#include "pa_kernels.h"
#include "../../include/playaid_hip.h"

namespace pa {
namespace {

constexpr int ANNOT_RUN = 16;        // output pixels per thread
constexpr int ANNOT_THREADS = 256;
constexpr int ANNOT_FAR = 1 << 29;   // box coordinates are clamped to +-ANNOT_FAR: far outside any frame either way, no overflow

struct AnnotDerived {
    int hx0, hy0, hx1, hy1;  // everything the item can touch, clipped to the frame (inclusive; hx0 > hx1: nothing)
    int x0, x1, y0, y1;      // the box, rows ordered; columns as given
    int xa, xb;              // columns of the horizontal strokes (ordered)
    int va, vb;              // rows of the vertical strokes (inclusive; va > vb: none)
    int lw;                  // 0: no outline
    int tx, ty, tw;          // text origin and width in pixels; tw == 0: no label
    int fill;                // background rectangle (tx, ty) .. (tx + tw + 1, ty + cell_h + 1) is painted
    int text_off, text_len;
    unsigned bgr;            // b | g << 8 | r << 16
};

__device__ inline int annot_clamp(int v) { return v < -ANNOT_FAR ? -ANNOT_FAR : (v > ANNOT_FAR ? ANNOT_FAR : v); }

__device__ inline void annot_derive(const pa_annot_item& it, int H, int W, int cell_w, int cell_h, AnnotDerived& d) {
    int x0 = annot_clamp(it.box[0]), y0 = annot_clamp(it.box[1]), x1 = annot_clamp(it.box[2]), y1 = annot_clamp(it.box[3]);
    // color=None: no background, and the outline in ImageDraw's default ink, white (rectangle(outline=None) falls back to it)
    d.bgr = it.has_color ? (unsigned)it.rgb[2] | ((unsigned)it.rgb[1] << 8) | ((unsigned)it.rgb[0] << 16) : 0xffffffu;
    // label geometry from the box as given (annotator.py:123-137)
    d.tw = it.text_len > 0 ? cell_w * it.text_len : 0;
    d.tx = x0;
    d.ty = (y0 - cell_h >= 0) ? y0 - cell_h : y0;
    d.fill = it.text_len > 0 && it.has_color;
    d.text_off = it.text_off;
    d.text_len = it.text_len;
    int bx0 = 1, bx1 = 0, by0 = 1, by1 = 0;
    if (d.tw > 0) {
        bx0 = d.tx;
        by0 = d.ty;
        bx1 = d.tx + d.tw + 1;
        by1 = d.ty + cell_h + 1;
    }
    // outline
    d.lw = it.draw_box ? it.line_width : 0;
    if (y0 > y1) {
        const int t = y0;
        y0 = y1;
        y1 = t;
    }
    d.x0 = x0;
    d.x1 = x1;
    d.y0 = y0;
    d.y1 = y1;
    d.xa = x0 < x1 ? x0 : x1;
    d.xb = x0 < x1 ? x1 : x0;
    const int a = y0 + d.lw, b = y1 - d.lw + 1;
    d.va = b >= a ? a : b + 1;
    d.vb = b >= a ? b - 1 : a;
    if (d.lw > 0) {
        int ox0 = min(d.xa, x1 - d.lw + 1), ox1 = max(d.xb, x0 + d.lw - 1);
        int oy0 = min(y0, y1 - d.lw + 1), oy1 = max(y1, y0 + d.lw - 1);
        if (d.va <= d.vb) {
            oy0 = min(oy0, d.va);
            oy1 = max(oy1, d.vb);
        }
        if (bx0 > bx1) {
            bx0 = ox0, bx1 = ox1, by0 = oy0, by1 = oy1;
        } else {
            bx0 = min(bx0, ox0), bx1 = max(bx1, ox1), by0 = min(by0, oy0), by1 = max(by1, oy1);
        }
    }
    d.hx0 = max(bx0, 0);
    d.hy0 = max(by0, 0);
    d.hx1 = min(bx1, W - 1);
    d.hy1 = min(by1, H - 1);
    if (d.hy0 > d.hy1) d.hx0 = 1, d.hx1 = 0;
}

// One pixel of the frame against one item: outline, then background, then text.
__device__ inline unsigned annot_pixel(const AnnotDerived& d, int x, int y, unsigned c, const unsigned char* __restrict__ text,
                                       const unsigned char* __restrict__ atlas, int cell_w, int cell_h, int n_chars) {
    if (d.lw > 0) {
        const bool band = (unsigned)(y - d.y0) < (unsigned)d.lw || (unsigned)(d.y1 - y) < (unsigned)d.lw;
        const bool side = (unsigned)(d.x1 - x) < (unsigned)d.lw || (unsigned)(x - d.x0) < (unsigned)d.lw;
        if ((band && x >= d.xa && x <= d.xb) || (side && y >= d.va && y <= d.vb)) c = d.bgr;
    }
    if (d.tw > 0) {
        const int dx = x - d.tx, dy = y - d.ty;
        if (d.fill && dx >= 0 && dx <= d.tw + 1 && dy >= 0 && dy <= cell_h + 1) c = d.bgr;
        if (dx >= 0 && dx < d.tw && dy >= 0 && dy < cell_h) {
            const int k = dx / cell_w;
            const int ch = text[d.text_off + k];
            const int nx = (k + 1 < d.text_len) ? text[d.text_off + k + 1] : n_chars;
            if (atlas[((size_t)(ch * (n_chars + 1) + nx) * cell_h + dy) * cell_w + (dx - k * cell_w)]) c = 0xffffffu;
        }
    }
    return c;
}

__device__ inline unsigned annot_byte(const unsigned (&w)[12], int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

// VEC: W, pad_left and pad_right are multiples of 16 and both buffers are 16-byte aligned, so every run is wholly padding or
// wholly picture and both of its ends are 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(ANNOT_THREADS) void annotate_kernel(AnnotParams p) {
    __shared__ AnnotDerived s_items[PA_ANNOT_MAX_ITEMS];
    const int f = blockIdx.y;
    int count = p.counts[f];
    count = count < 0 ? 0 : (count > PA_ANNOT_MAX_ITEMS ? PA_ANNOT_MAX_ITEMS : count);
    if ((int)threadIdx.x < count)
        annot_derive(static_cast<const pa_annot_item*>(p.items)[(size_t)f * PA_ANNOT_MAX_ITEMS + threadIdx.x], p.H, p.W, p.cell_w, p.cell_h,
                     s_items[threadIdx.x]);
    __syncthreads();

    const int Wo = p.pad_left + p.W + p.pad_right, Ho = p.H + p.pad_bottom;
    const int runs_per_row = (Wo + ANNOT_RUN - 1) / ANNOT_RUN;
    const int r = blockIdx.x * ANNOT_THREADS + threadIdx.x;
    if (r >= runs_per_row * Ho) return;
    const int y = r / runs_per_row;
    const int xo = (r - y * runs_per_row) * ANNOT_RUN;  // first output column of the run
    const int xi = xo - p.pad_left;                      // the same in the picture's columns
    unsigned char* dst = p.out + (((size_t)f * Ho + y) * Wo + xo) * 3;
    const size_t src_row = ((size_t)f * p.H + y) * p.W * 3;  // read only where y < H, at columns 0 <= x < W

    // items whose bounding rectangle the run meets
    unsigned hit = 0;
    if (y < p.H)
        for (int i = 0; i < count; ++i) {
            const AnnotDerived& d = s_items[i];
            if (y >= d.hy0 && y <= d.hy1 && xi <= d.hx1 && xi + ANNOT_RUN - 1 >= d.hx0) hit |= 1u << i;
        }

    if (VEC) {
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0, v2 = v0;
        if (y < p.H && xi >= 0 && xi < p.W) {
            const uint4* s4 = reinterpret_cast<const uint4*>(p.in + src_row + (size_t)xi * 3);
            v0 = s4[0];
            v1 = s4[1];
            v2 = s4[2];
            if (hit) {
                unsigned w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
                unsigned c[ANNOT_RUN];
#pragma unroll
                for (int k = 0; k < ANNOT_RUN; ++k) c[k] = annot_byte(w, 3 * k) | (annot_byte(w, 3 * k + 1) << 8) | (annot_byte(w, 3 * k + 2) << 16);
                for (int i = 0; i < count; ++i) {
                    if (!(hit >> i & 1)) continue;
                    const AnnotDerived& d = s_items[i];
#pragma unroll
                    for (int k = 0; k < ANNOT_RUN; ++k) c[k] = annot_pixel(d, xi + k, y, c[k], p.text, p.atlas, p.cell_w, p.cell_h, p.n_chars);
                }
#pragma unroll
                for (int j = 0; j < 12; ++j) w[j] = 0;
#pragma unroll
                for (int k = 0; k < ANNOT_RUN; ++k) {
#pragma unroll
                    for (int b = 0; b < 3; ++b) w[(3 * k + b) >> 2] |= ((c[k] >> (8 * b)) & 0xffu) << (((3 * k + b) & 3) * 8);
                }
                v0 = make_uint4(w[0], w[1], w[2], w[3]);
                v1 = make_uint4(w[4], w[5], w[6], w[7]);
                v2 = make_uint4(w[8], w[9], w[10], w[11]);
            }
        }
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        d4[0] = v0;
        d4[1] = v1;
        d4[2] = v2;
    } else {
        const int len = min(ANNOT_RUN, Wo - xo);
        for (int k = 0; k < len; ++k) {
            const int x = xi + k;
            unsigned c = 0;
            if (y < p.H && x >= 0 && x < p.W) {
                const unsigned char* src = p.in + src_row + (size_t)x * 3;
                c = (unsigned)src[0] | ((unsigned)src[1] << 8) | ((unsigned)src[2] << 16);
                for (int i = 0; i < count; ++i)
                    if (hit >> i & 1) c = annot_pixel(s_items[i], x, y, c, p.text, p.atlas, p.cell_w, p.cell_h, p.n_chars);
            }
            dst[3 * k] = (unsigned char)c;
            dst[3 * k + 1] = (unsigned char)(c >> 8);
            dst[3 * k + 2] = (unsigned char)(c >> 16);
        }
    }
}

}  // namespace

hipError_t launch_annotate(const AnnotParams& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const int Wo = p.pad_left + p.W + p.pad_right, Ho = p.H + p.pad_bottom;
    const int runs = ((Wo + ANNOT_RUN - 1) / ANNOT_RUN) * Ho;
    const dim3 grid((runs + ANNOT_THREADS - 1) / ANNOT_THREADS, p.n);
    const bool vec = p.W % 16 == 0 && p.pad_left % 16 == 0 && p.pad_right % 16 == 0 && (reinterpret_cast<uintptr_t>(p.in) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(p.out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(annotate_kernel<true>, grid, dim3(ANNOT_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(annotate_kernel<false>, grid, dim3(ANNOT_THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace pa

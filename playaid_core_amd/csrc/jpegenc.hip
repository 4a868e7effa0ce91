// Baseline JPEG ENCODE on the device: packed uint8 images in HBM -> complete JPEG files in HBM, byte for byte what
// libjpeg(-turbo) writes for the same pixels, quality and sampling (Pillow's Image.save(quality, subsampling) without
// `optimize`; cv2.imwrite up to the sampling default). This is the file half of YOLOv5's `--save-crop` hand-off
// (playaid/ai_runner.py:191-194, 291-295: crops/<Fighter>/<video>_<n>.jpg) and the writer of Motion-JPEG clips.
//
// The sample arithmetic is libjpeg's (jccolor.c, jcsample.c h2v2_downsample, jcprepct.c edge fill, jfdctint.c, the
// quantiser of jcdctmgr.c) as savebox.hip / jpeg_dct.h already restate it; the entropy coder is T.81 Annex F with the
// standard tables K.3-K.6, which is what libjpeg emits when it does not optimise its tables.
//
// One call = these launches on the caller's stream, none of which waits for another workgroup and none of which the host
// waits for (image sizes are only known on the device: grids are sized from max_height x max_width and n, threads beyond
// an image's blocks return):
//   plan_kernel     : per image block counts, exclusive scan -> where its blocks sit in the coefficient buffer
//   coef_kernel     : colour conversion, down-sampling, edge fill, FDCT, quantisation -> int16 coefficients, zig-zag
//                     order, blocks in MCU scan order (4:4:4: one thread per block position, three components;
//                     4:2:0: one thread per luma / chroma block)
//   length_kernel   : per block the DC difference against its predecessor in the component and the bits its codes take
//   scan_kernel     : exclusive scan of those lengths per image (wave64 shuffles + one LDS step) -> bit offsets
//   layout_kernel   : where each image's un-stuffed stream sits in the handle's scratch
//   pack_kernel     : every block writes its bits at its offset into the zeroed stream; words that two blocks share are
//                     merged with a vector integer OR atomic, which does not depend on the order
//   ff_count_kernel / ff_scan_kernel : FF bytes per 64-byte chunk of the stream, exclusive scan per image
//   file_layout_kernel : file sizes, 16-byte aligned offsets in input order, the records, the overflow count
//   write_kernel    : header (height / width patched in), stuffed bytes, FFD9
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/playaid_hip.h"
#include "jpeg_dct.h"

namespace pa {
namespace je {

constexpr int HEADER_BYTES = 623;
constexpr int SOF_HEIGHT_AT = 163;       // height (2 bytes), width (2 bytes), big-endian
constexpr int MAX_BLOCK_BITS = 27 + 63 * 26;
constexpr int CHUNK = 64;                // bytes of the un-stuffed stream per thread of the stuffing passes
constexpr int16_t DUMMY = 0x7fff;        // coefficient 0 of a 4:2:0 dummy block (a real DC is within +-2048)
constexpr int HUFF_STRIDE = 16 + 256;    // per table class: 16 DC entries, 256 AC entries; entry = length << 16 | code

constexpr int ZZ[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                        21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                        60, 61, 54, 47, 55, 62, 63};

struct ImgState {
    int64_t blk_base;     // first block of the image in the per-block arrays
    int64_t scr_off;      // first byte of its un-stuffed stream in the scratch (64-byte aligned)
    int64_t file_off;
    int32_t nblocks;      // coded blocks, all components, dummy blocks included
    int32_t state;        // 0 encode, 1 empty (height = width = 0), -1 does not fit / bad descriptor
    int32_t h, w;
    int32_t mx, my;       // 4:4:4: blocks per row / column; 4:2:0: MCUs per row / column
    uint32_t total_bits;
    uint32_t sbytes;      // un-stuffed stream bytes, the 1-bit fill included
    uint32_t ff;          // FF bytes in it
    int32_t pad;
};

struct QTab {
    uint16_t q[2][64];    // luma, chroma; natural order
};
struct Header {
    uint8_t b[HEADER_BYTES + 1];
};

struct Params {
    const uint8_t* images;
    size_t images_bytes;
    const pa_crop_image* desc;
    int32_t n, max_h, max_w, bgr, sub;
    ImgState* st;
    int16_t* coef;        // [max_blocks][64]
    int16_t* diff;        // [max_blocks] DC differences
    uint16_t* len;        // [max_blocks] bits of a block
    uint32_t* bitoff;     // [max_blocks] first bit of a block in its image's stream
    long long max_blocks;
    uint8_t* scratch;
    size_t scratch_bytes;
    uint32_t* chunk;      // [scratch_bytes / CHUNK + 1] FF counts, then their exclusive scan
    const uint32_t* huff; // [2][HUFF_STRIDE]
    uint8_t* files;
    size_t files_capacity;
    pa_jpeg_file* out;
    int32_t* overflow;
};

__device__ __forceinline__ unsigned long long wg_scan256(unsigned long long v, unsigned long long* lds) {
    // inclusive scan over a 256-thread workgroup: wave64 shuffles, then the four wave totals through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; ++k) v += lds[k];
    return v;
}

// one workgroup: validates the descriptors, counts blocks, exclusive scan over the images
__global__ __launch_bounds__(256) void plan_kernel(const Params p) {
    __shared__ unsigned long long tot[4];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < p.n; base += 256) {
        const int i = base + threadIdx.x;
        ImgState s = {};
        unsigned long long nb = 0;
        if (i < p.n) {
            const pa_crop_image d = p.desc[i];
            s.h = d.height; s.w = d.width;
            if (d.height == 0 && d.width == 0) {
                s.state = 1;
            } else if (d.height < 1 || d.width < 1 || d.height > p.max_h || d.width > p.max_w || d.offset < 0 ||
                       (unsigned long long)d.offset + (unsigned long long)d.height * d.width * 3 > p.images_bytes) {
                s.state = -1;
            } else {
                const int sh = p.sub ? 4 : 3;
                s.mx = (d.width + (1 << sh) - 1) >> sh;
                s.my = (d.height + (1 << sh) - 1) >> sh;
                nb = (unsigned long long)s.mx * s.my * (p.sub ? 6 : 3);
                if (nb * MAX_BLOCK_BITS > 0xffffffffull) { s.state = -1; nb = 0; }
            }
        }
        const unsigned long long incl = wg_scan256(nb, tot);
        const unsigned long long off = carry + incl - nb;
        if (i < p.n) {
            if (nb && off + nb > (unsigned long long)p.max_blocks) { s.state = -1; nb = 0; }
            s.blk_base = (int64_t)off;
            s.nblocks = (int32_t)nb;
            p.st[i] = s;
        }
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
}

// FDCT + quantisation of the block in d (sample - 128), stored as int16 in zig-zag order
__device__ __forceinline__ void fdct_quant_store(int* d, const int* __restrict__ q, int16_t* out) {
    using namespace dct;
#pragma unroll
    for (int y = 0; y < 8; ++y) fdct8<true>(d + y * 8, 1);
#pragma unroll
    for (int x = 0; x < 8; ++x) fdct8<false>(d + x, 8);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        // (|d| + dv / 2) / dv without an integer division: both operands are below 2^24, so the float quotient is off by
        // at most one and one correction step makes it exact (savebox.hip::block444)
        const int qv = q[i], dv = qv << 3;
        const int x = abs(d[i]) + (dv >> 1);
        int a = (int)((float)x * __builtin_amdgcn_rcpf((float)dv));
        const int r = x - a * dv;
        a += r >= dv ? 1 : (r < 0 ? -1 : 0);
        d[i] = d[i] < 0 ? -a : a;
    }
    uint4* o = reinterpret_cast<uint4*>(out);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = ((uint32_t)d[ZZ[g * 8 + 2 * k]] & 0xffffu) | ((uint32_t)d[ZZ[g * 8 + 2 * k + 1]] << 16);
        o[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// 4:4:4: one thread = one 8x8 block position, its three components one after the other
__global__ __launch_bounds__(64) void coef444_kernel(const Params p, const QTab qt_in) {
    __shared__ int qt[2][64];
    qt[0][threadIdx.x] = qt_in.q[0][threadIdx.x];
    qt[1][threadIdx.x] = qt_in.q[1][threadIdx.x];
    __syncthreads();
    const ImgState s = p.st[blockIdx.y];
    if (s.state != 0) return;
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= s.mx * s.my) return;
    const int h = s.h, w = s.w;
    const int by = m / s.mx, bx = m - by * s.mx;
    const uint8_t* img = p.images + p.desc[blockIdx.y].offset;
    const int ir = p.bgr ? 2 : 0, ib = 2 - ir;
    // the block's pixels, the last row / column repeated past the edge (jcprepct.c)
    uint32_t px[64];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const int yy = min(by * 8 + y, h - 1);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int xx = min(bx * 8 + x, w - 1);
            const uint8_t* sp = img + ((size_t)yy * w + xx) * 3;
            px[y * 8 + x] = sp[ib] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[ir] << 16);
        }
    }
    int16_t* out = p.coef + (s.blk_base + (int64_t)m * 3) * 64;
    int d[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int b = px[i] & 0xff, g = (px[i] >> 8) & 0xff, r = (px[i] >> 16) & 0xff;
        d[i] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
    }
    fdct_quant_store(d, qt[0], out);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int b = px[i] & 0xff, g = (px[i] >> 8) & 0xff, r = (px[i] >> 16) & 0xff;
        d[i] = ((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16) - 128;
    }
    fdct_quant_store(d, qt[1], out + 64);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int b = px[i] & 0xff, g = (px[i] >> 8) & 0xff, r = (px[i] >> 16) & 0xff;
        d[i] = ((32768 * r + (128 << 16) + 32767 - 27439 * g - 5329 * b) >> 16) - 128;
    }
    fdct_quant_store(d, qt[1], out + 128);
}

// 4:2:0: one thread = one block of the MCU scan (Y00 Y01 Y10 Y11 Cb Cr)
__global__ __launch_bounds__(64) void coef420_kernel(const Params p, const QTab qt_in) {
    __shared__ int qt[2][64];
    qt[0][threadIdx.x] = qt_in.q[0][threadIdx.x];
    qt[1][threadIdx.x] = qt_in.q[1][threadIdx.x];
    __syncthreads();
    const ImgState s = p.st[blockIdx.y];
    if (s.state != 0) return;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= s.nblocks) return;
    const int h = s.h, w = s.w;
    const int m = t / 6, k = t - m * 6;
    const int my = m / s.mx, mx = m - my * s.mx;
    const uint8_t* img = p.images + p.desc[blockIdx.y].offset;
    const int ir = p.bgr ? 2 : 0, ib = 2 - ir;
    int16_t* out = p.coef + (s.blk_base + t) * 64;
    int d[64];
    if (k < 4) {
        const int by = 2 * my + (k >> 1), bx = 2 * mx + (k & 1);
        if (by >= ((h + 7) >> 3) || bx >= ((w + 7) >> 3)) {
            // a dummy block of a half-empty MCU (jccoefct.c): AC 0, DC = that of the block coded before it
            uint4* o = reinterpret_cast<uint4*>(out);
            o[0] = make_uint4((uint32_t)(uint16_t)DUMMY, 0, 0, 0);
#pragma unroll
            for (int g = 1; g < 8; ++g) o[g] = make_uint4(0, 0, 0, 0);
            return;
        }
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int yy = min(by * 8 + y, h - 1);
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int xx = min(bx * 8 + x, w - 1);
                const uint8_t* sp = img + ((size_t)yy * w + xx) * 3;
                const int r = sp[ir], g = sp[1], b = sp[ib];
                d[y * 8 + x] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
            }
        }
    } else {
        // jcsample.c h2v2_downsample on the input padded to the right and to an even number of rows, the down-sampled
        // plane then filled up to whole blocks by repeating its last row (its width is a whole number of blocks already)
        const int kr = k == 4 ? -11059 : 32768, kg = k == 4 ? -21709 : -27439, kb = k == 4 ? 32768 : -5329;
        const int ch = (h + 1) >> 1;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int cy = min(my * 8 + y, ch - 1);
            const int r0 = 2 * cy, r1 = min(2 * cy + 1, h - 1);
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int cx = mx * 8 + x;
                const int c0 = min(2 * cx, w - 1), c1 = min(2 * cx + 1, w - 1);
                int sum = (x & 1) ? 2 : 1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint8_t* sp = img + ((size_t)((q >> 1) ? r1 : r0) * w + ((q & 1) ? c1 : c0)) * 3;
                    sum += (kr * (int)sp[ir] + kg * (int)sp[1] + kb * (int)sp[ib] + (128 << 16) + 32767) >> 16;
                }
                d[y * 8 + x] = (sum >> 2) - 128;
            }
        }
    }
    fdct_quant_store(d, qt[k >= 4], out);
}

__device__ __forceinline__ int nbits(int v) { return 32 - __clz(abs(v)); }  // abs(v) > 0 -> 1..; 0 -> 0

// block b's component class (0 luma tables, 1 chroma tables) and its predecessor in the component (-1: none)
__device__ __forceinline__ void block_role(int sub, int b, int& cls, long long& pred) {
    if (sub) {
        const int k = b % 6;
        cls = k >= 4;
        pred = k >= 4 ? b - 6 : (k ? b - 1 : (b ? b - 3 : -1));
    } else {
        cls = (b % 3) != 0;
        pred = b - 3;
    }
}

// the DC a block is coded with: a dummy block's is that of the block before it in its MCU (Y00 is never a dummy)
__device__ __forceinline__ int coded_dc(const int16_t* coef, long long b) {
    int v = coef[b * 64];
    while (v == DUMMY) {
        --b;
        v = coef[b * 64];
    }
    return v;
}

__global__ __launch_bounds__(256) void length_kernel(const Params p) {
    __shared__ uint8_t aclen[2][256];
    __shared__ uint8_t dclen[2][16];
    for (int i = threadIdx.x; i < 512; i += 256) aclen[i >> 8][i & 255] = (uint8_t)(p.huff[(i >> 8) * HUFF_STRIDE + 16 + (i & 255)] >> 16);
    if (threadIdx.x < 32) dclen[threadIdx.x >> 4][threadIdx.x & 15] = (uint8_t)(p.huff[(threadIdx.x >> 4) * HUFF_STRIDE + (threadIdx.x & 15)] >> 16);
    __syncthreads();
    const ImgState s = p.st[blockIdx.y];
    if (s.state != 0) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= s.nblocks) return;
    int cls;
    long long pred;
    block_role(p.sub, b, cls, pred);
    const int16_t* coef = p.coef + s.blk_base * 64;
    const uint4* c4 = reinterpret_cast<const uint4*>(coef + (long long)b * 64);
    int bits = 0, run = 0, dc = 0;
    for (int g = 0; g < 8; ++g) {
        const uint4 v = c4[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = (int)(int16_t)(w[k >> 1] >> ((k & 1) * 16));
            if (g == 0 && k == 0) { dc = c; continue; }
            if (c == 0) { ++run; continue; }
            const int nb = nbits(c);
            bits += (run >> 4) * aclen[cls][0xF0] + aclen[cls][((run & 15) << 4) | nb] + nb;
            run = 0;
        }
    }
    if (run) bits += aclen[cls][0];
    int df = 0;
    if (dc != DUMMY) df = dc - (pred >= 0 ? coded_dc(coef, pred) : 0);
    const int cat = nbits(df);
    bits += dclen[cls][cat] + cat;
    p.diff[s.blk_base + b] = (int16_t)df;
    p.len[s.blk_base + b] = (uint16_t)bits;
}

// one workgroup per image: exclusive scan of its blocks' lengths
__global__ __launch_bounds__(256) void scan_kernel(const Params p) {
    __shared__ unsigned long long tot[4];
    __shared__ unsigned long long carry;
    ImgState* sp = p.st + blockIdx.x;
    const ImgState s = *sp;
    if (s.state != 0) return;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < s.nblocks; base += 256) {
        const int b = base + threadIdx.x;
        const unsigned long long v = b < s.nblocks ? p.len[s.blk_base + b] : 0;
        const unsigned long long incl = wg_scan256(v, tot);
        if (b < s.nblocks) p.bitoff[s.blk_base + b] = (uint32_t)(carry + incl - v);
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sp->total_bits = (uint32_t)carry;
        sp->sbytes = (uint32_t)((carry + 7) >> 3);
    }
}

// one workgroup: the images' stream regions in the scratch
__global__ __launch_bounds__(256) void layout_kernel(const Params p) {
    __shared__ unsigned long long tot[4];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < p.n; base += 256) {
        const int i = base + threadIdx.x;
        unsigned long long region = 0;
        if (i < p.n && p.st[i].state == 0) region = ((unsigned long long)p.st[i].sbytes + CHUNK - 1) / CHUNK * CHUNK;
        const unsigned long long incl = wg_scan256(region, tot);
        const unsigned long long off = carry + incl - region;
        if (i < p.n && p.st[i].state == 0) {
            if (off + region > p.scratch_bytes) p.st[i].state = -1;
            p.st[i].scr_off = (int64_t)off;
        }
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
}

// MSB-first bit writer of one block into the zeroed stream: whole words it owns are stored, its first and last word are
// shared with the neighbours and merged by an OR atomic
struct BitWriter {
    uint32_t* words;
    unsigned long long acc;
    int nacc;
    long long word;
    bool first;
    __device__ __forceinline__ void put(uint32_t code, int len) {
        acc = (acc << len) | code;
        nacc += len;
        if (nacc >= 32) {
            const uint32_t w = (uint32_t)(acc >> (nacc - 32));
            nacc -= 32;
            acc &= (1ull << nacc) - 1;
            const uint32_t be = __builtin_bswap32(w);
            if (first) atomicOr(words + word, be); else words[word] = be;
            first = false;
            ++word;
        }
    }
    __device__ __forceinline__ void flush() {
        if (nacc > 0) atomicOr(words + word, __builtin_bswap32((uint32_t)(acc << (32 - nacc))));
    }
};

__global__ __launch_bounds__(256) void pack_kernel(const Params p) {
    __shared__ uint32_t huff[2 * HUFF_STRIDE];
    for (int i = threadIdx.x; i < 2 * HUFF_STRIDE; i += 256) huff[i] = p.huff[i];
    __syncthreads();
    const ImgState s = p.st[blockIdx.y];
    if (s.state != 0) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= s.nblocks) return;
    const int cls = p.sub ? (b % 6) >= 4 : (b % 3) != 0;
    const uint32_t* hd = huff + cls * HUFF_STRIDE;
    const uint32_t* ha = hd + 16;
    const uint32_t o = p.bitoff[s.blk_base + b];
    BitWriter bw;
    bw.words = reinterpret_cast<uint32_t*>(p.scratch + s.scr_off);
    bw.acc = 0;
    bw.nacc = (int)(o & 31);   // the bits in front belong to the blocks before: zeros here, OR-ed in by them
    bw.word = o >> 5;
    bw.first = true;
    {
        const int df = p.diff[s.blk_base + b];
        const int cat = nbits(df);
        const uint32_t e = hd[cat];
        const uint32_t extra = (uint32_t)(df < 0 ? df - 1 : df) & ((1u << cat) - 1);
        bw.put(((e & 0xffff) << cat) | extra, (int)(e >> 16) + cat);
    }
    const uint4* c4 = reinterpret_cast<const uint4*>(p.coef + (s.blk_base + b) * 64);
    int run = 0;
    for (int g = 0; g < 8; ++g) {
        const uint4 v = c4[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (g == 0 && k == 0) continue;
            const int c = (int)(int16_t)(w[k >> 1] >> ((k & 1) * 16));
            if (c == 0) { ++run; continue; }
            while (run >= 16) {
                bw.put(ha[0xF0] & 0xffff, (int)(ha[0xF0] >> 16));
                run -= 16;
            }
            const int nb = nbits(c);
            const uint32_t e = ha[(run << 4) | nb];
            const uint32_t extra = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << nb) - 1);
            bw.put(((e & 0xffff) << nb) | extra, (int)(e >> 16) + nb);
            run = 0;
        }
    }
    if (run) bw.put(ha[0] & 0xffff, (int)(ha[0] >> 16));
    if (b == s.nblocks - 1) {  // the last partial byte is filled with 1-bits
        const int fill = (8 - (int)(s.total_bits & 7)) & 7;
        if (fill) bw.put((1u << fill) - 1, fill);
    }
    bw.flush();
}

__global__ __launch_bounds__(256) void ff_count_kernel(const Params p) {
    const ImgState s = p.st[blockIdx.y];
    if (s.state != 0) return;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c * CHUNK >= s.sbytes) return;
    const uint8_t* src = p.scratch + s.scr_off + c * CHUNK;
    const int nb = (int)min((long long)CHUNK, (long long)s.sbytes - c * CHUNK);
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    int cnt = 0;
    for (int g = 0; g < CHUNK / 16; ++g) {
        const uint4 v = s4[g];   // (the region is whole chunks, the bytes behind the stream are zero)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            cnt += (g * 16 + k < nb) && ((w[k >> 2] >> ((k & 3) * 8)) & 0xff) == 0xff;
    }
    p.chunk[s.scr_off / CHUNK + c] = cnt;
}

// one workgroup per image: exclusive scan of its chunks' FF counts, in place
__global__ __launch_bounds__(256) void ff_scan_kernel(const Params p) {
    __shared__ unsigned long long tot[4];
    __shared__ unsigned long long carry;
    ImgState* sp = p.st + blockIdx.x;
    const ImgState s = *sp;
    if (s.state != 0) return;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const long long nch = ((long long)s.sbytes + CHUNK - 1) / CHUNK;
    uint32_t* cnt = p.chunk + s.scr_off / CHUNK;
    for (long long base = 0; base < nch; base += 256) {
        const long long c = base + threadIdx.x;
        const unsigned long long v = c < nch ? cnt[c] : 0;
        const unsigned long long incl = wg_scan256(v, tot);
        if (c < nch) cnt[c] = (uint32_t)(carry + incl - v);
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) sp->ff = (uint32_t)carry;
}

// one workgroup: file sizes -> 16-byte aligned offsets in input order, records, overflow count
__global__ __launch_bounds__(256) void file_layout_kernel(const Params p) {
    __shared__ unsigned long long tot[4];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < p.n; base += 256) {
        const int i = base + threadIdx.x;
        unsigned long long size = 0;
        int state = 1;
        if (i < p.n) {
            state = p.st[i].state;
            if (state == 0) size = (unsigned long long)HEADER_BYTES + p.st[i].sbytes + p.st[i].ff + 2;
        }
        const unsigned long long aligned = (size + 15) & ~15ull;
        const unsigned long long incl = wg_scan256(aligned, tot);
        const unsigned long long off = carry + incl - aligned;
        if (i < p.n) {
            if (state == 0 && off + size > p.files_capacity) state = p.st[i].state = -1;
            p.st[i].file_off = (int64_t)off;
            pa_jpeg_file r;
            r.offset = (int64_t)off;
            r.nbytes = state == 0 ? (int32_t)size : (state == 1 ? 0 : -1);
            r.reserved = 0;
            p.out[i] = r;
            if (state < 0) atomicAdd(p.overflow, 1);
        }
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void write_kernel(const Params p, const Header hdr) {
    const ImgState s = p.st[blockIdx.y];
    if (s.state != 0) return;
    uint8_t* file = p.files + s.file_off;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < HEADER_BYTES; i += 256) {
            uint8_t v = hdr.b[i];
            if (i == SOF_HEIGHT_AT) v = (uint8_t)(s.h >> 8);
            if (i == SOF_HEIGHT_AT + 1) v = (uint8_t)s.h;
            if (i == SOF_HEIGHT_AT + 2) v = (uint8_t)(s.w >> 8);
            if (i == SOF_HEIGHT_AT + 3) v = (uint8_t)s.w;
            file[i] = v;
        }
        if (threadIdx.x == 0) {
            uint8_t* e = file + HEADER_BYTES + s.sbytes + s.ff;
            e[0] = 0xff; e[1] = 0xd9;
        }
    }
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c * CHUNK >= s.sbytes) return;
    const int nb = (int)min((long long)CHUNK, (long long)s.sbytes - c * CHUNK);
    const uint4* s4 = reinterpret_cast<const uint4*>(p.scratch + s.scr_off + c * CHUNK);
    uint8_t* dst = file + HEADER_BYTES + c * CHUNK + p.chunk[s.scr_off / CHUNK + c];
    for (int g = 0; g < CHUNK / 16; ++g) {
        const uint4 v = s4[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (g * 16 + k < nb) {
                const uint8_t byte = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
                *dst++ = byte;
                if (byte == 0xff) *dst++ = 0;
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// T.81 Annex K.3 - K.6: what libjpeg writes when it does not optimise its tables (jcparam.c std_huff_tables)
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
const uint8_t STD_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jpeg_set_quality(quality, force_baseline = TRUE)
void quality_tables(int quality, QTab& qt) {
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int v = (STD_Q[t][i] * scale + 50) / 100;
            qt.q[t][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

// T.81 Annex C: code of every symbol, as length << 16 | code
void derive(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i) table[vals[k++]] = ((uint32_t)l << 16) | code++;
        code <<= 1;
    }
}

void huffman_tables(uint32_t* huff) {
    memset(huff, 0, 2 * HUFF_STRIDE * sizeof(uint32_t));
    for (int t = 0; t < 2; ++t) {
        derive(DC_BITS[t], DC_VALS, huff + t * HUFF_STRIDE);
        derive(AC_BITS[t], AC_VALS[t], huff + t * HUFF_STRIDE + 16);
    }
}

int write_header(int height, int width, const QTab& qt, int sub, uint8_t* out) {
    uint8_t* p = out;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    put({0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xdb, 0, 67, t});
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)qt.q[t][ZZ[k]];
    }
    put({0xff, 0xc0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, sub ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xc4, 0, 31, t});
        for (int i = 0; i < 16; ++i) *p++ = DC_BITS[t][i];
        for (int i = 0; i < 12; ++i) *p++ = DC_VALS[i];
        put({0xff, 0xc4, 0, 181, 0x10 | t});
        for (int i = 0; i < 16; ++i) *p++ = AC_BITS[t][i];
        for (int i = 0; i < 162; ++i) *p++ = AC_VALS[t][i];
    }
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return (int)(p - out);
}

long long coded_blocks(long long height, long long width, int sub) {
    return sub ? 6 * ((height + 15) / 16) * ((width + 15) / 16) : 3 * ((height + 7) / 8) * ((width + 7) / 8);
}

}  // namespace je
}  // namespace pa

using namespace pa::je;

struct pa_jpegenc {
    int device = 0, max_images = 0;
    long long max_blocks = 0;
    size_t scratch_bytes = 0;
    ImgState* d_st = nullptr;
    int16_t* d_coef = nullptr;
    int16_t* d_diff = nullptr;
    uint16_t* d_len = nullptr;
    uint32_t* d_bitoff = nullptr;
    uint8_t* d_scratch = nullptr;
    uint32_t* d_chunk = nullptr;
    uint32_t* d_huff = nullptr;
    int32_t* d_overflow = nullptr;
    bool ready = false;
    std::string last_error;
};

extern "C" {

const char* pa_jpegenc_last_error(const pa_jpegenc* h) { return h ? h->last_error.c_str() : "null handle"; }

void pa_jpegenc_destroy(pa_jpegenc* h) {
    if (!h) return;
    void* dev[] = {h->d_st, h->d_coef, h->d_diff, h->d_len, h->d_bitoff, h->d_scratch, h->d_chunk, h->d_huff, h->d_overflow};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    delete h;
}

int pa_jpegenc_create(int32_t device, int32_t max_images, int64_t max_blocks, size_t scratch_bytes, pa_jpegenc** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (device < 0 || max_images < 1 || max_images > 65535 || max_blocks < 3 || max_blocks > (1ll << 26) || scratch_bytes < 1024 ||
        scratch_bytes > 0xe0000000ull)
        return PA_ERR_INVALID_ARG;
    pa_jpegenc* h = new pa_jpegenc();
    *out = h;  // handed back on failure too (pa_jpegenc_last_error, then pa_jpegenc_destroy)
    h->device = device; h->max_images = max_images; h->max_blocks = max_blocks;
    h->scratch_bytes = (scratch_bytes + CHUNK - 1) / CHUNK * CHUNK;
    auto chk = [&](hipError_t e, const char* what) -> bool {
        if (e == hipSuccess) return true;
        h->last_error = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    if (!chk(hipSetDevice(device), "hipSetDevice")) return PA_ERR_NO_DEVICE;
    const size_t nb = (size_t)max_blocks;
    if (!chk(hipMalloc(&h->d_st, (size_t)max_images * sizeof(ImgState)), "hipMalloc image states")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_coef, nb * 64 * sizeof(int16_t)), "hipMalloc coefficients")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_diff, nb * sizeof(int16_t)), "hipMalloc DC differences")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_len, nb * sizeof(uint16_t)), "hipMalloc block lengths")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_bitoff, nb * sizeof(uint32_t)), "hipMalloc bit offsets")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_scratch, h->scratch_bytes + 4096), "hipMalloc stream scratch")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_chunk, (h->scratch_bytes / CHUNK + 1) * sizeof(uint32_t)), "hipMalloc chunk counts")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_huff, 2 * HUFF_STRIDE * sizeof(uint32_t)), "hipMalloc code tables")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_overflow, sizeof(int32_t)), "hipMalloc counter")) return PA_ERR_HIP;
    uint32_t huff[2 * HUFF_STRIDE];
    huffman_tables(huff);
    if (!chk(hipMemcpy(h->d_huff, huff, sizeof(huff), hipMemcpyHostToDevice), "hipMemcpy code tables")) return PA_ERR_HIP;
    if (!chk(hipMemset(h->d_overflow, 0, sizeof(int32_t)), "hipMemset")) return PA_ERR_HIP;
    h->ready = true;
    return PA_OK;
}

int pa_jpeg_header(int32_t height, int32_t width, int32_t quality, int32_t subsampling, uint8_t* out_host, size_t cap, int32_t* nbytes) {
    if (!out_host || height < 1 || width < 1 || height > 65535 || width > 65535 || quality < 1 || quality > 100 ||
        (subsampling != 0 && subsampling != 2) || cap < (size_t)HEADER_BYTES)
        return PA_ERR_INVALID_ARG;
    QTab qt;
    quality_tables(quality, qt);
    const int n = write_header(height, width, qt, subsampling, out_host);
    if (nbytes) *nbytes = n;
    return PA_OK;
}

size_t pa_jpeg_file_bytes_bound(int32_t height, int32_t width, int32_t subsampling) {
    if (height < 1 || width < 1 || height > 65535 || width > 65535 || (subsampling != 0 && subsampling != 2)) return 0;
    return (size_t)HEADER_BYTES + 2 * 209 * (size_t)coded_blocks(height, width, subsampling) + 2;
}

int pa_jpegenc_encode(pa_jpegenc* h, const uint8_t* images, size_t images_bytes, const pa_crop_image* desc, int32_t n, int32_t max_height,
                      int32_t max_width, int32_t bgr, int32_t quality, int32_t subsampling, uint8_t* files, size_t files_capacity,
                      pa_jpeg_file* out, void* stream) {
    if (!h) return PA_ERR_INVALID_ARG;
    auto bad = [&](int rc, const char* msg) { h->last_error = msg; return rc; };
    if (!images || !desc || !files || !out || n < 0 || max_height < 1 || max_width < 1 || max_height > 65535 || max_width > 65535 ||
        quality < 1 || quality > 100 || (subsampling != 0 && subsampling != 2) || (bgr != 0 && bgr != 1))
        return bad(PA_ERR_INVALID_ARG, "pa_jpegenc_encode: bad argument");
    if (n > h->max_images) return bad(PA_ERR_CAPACITY, "pa_jpegenc_encode: more images than max_images");
    if (!h->ready) return bad(PA_ERR_NOT_READY, "pa_jpegenc_encode: the handle has no device memory");
    if (n == 0) return PA_OK;
    hipStream_t s = (hipStream_t)stream;
    Params p = {};
    p.images = images; p.images_bytes = images_bytes; p.desc = desc;
    p.n = n; p.max_h = max_height; p.max_w = max_width; p.bgr = bgr; p.sub = subsampling;
    p.st = h->d_st; p.coef = h->d_coef; p.diff = h->d_diff; p.len = h->d_len; p.bitoff = h->d_bitoff;
    p.max_blocks = h->max_blocks;
    p.scratch = h->d_scratch; p.scratch_bytes = h->scratch_bytes; p.chunk = h->d_chunk; p.huff = h->d_huff;
    p.files = files; p.files_capacity = files_capacity; p.out = out; p.overflow = h->d_overflow;
    QTab qt;
    quality_tables(quality, qt);
    Header hdr;
    write_header(1, 1, qt, subsampling, hdr.b);
    // grids from the largest image the caller allows: blocks per image, and the chunks their bits can fill at most
    long long img_blocks = coded_blocks(max_height, max_width, subsampling);
    if (img_blocks > h->max_blocks) img_blocks = h->max_blocks;
    long long img_chunks = (img_blocks * 209 + CHUNK - 1) / CHUNK;
    if (img_chunks > (long long)(h->scratch_bytes / CHUNK)) img_chunks = (long long)(h->scratch_bytes / CHUNK);
    const unsigned gb = (unsigned)((img_blocks + 255) / 256), gc = (unsigned)((img_chunks + 255) / 256);
    if (hipMemsetAsync(h->d_scratch, 0, h->scratch_bytes, s) != hipSuccess) return bad(PA_ERR_HIP, "pa_jpegenc_encode: hipMemsetAsync failed");
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(256), 0, s, p);
    if (subsampling)
        hipLaunchKernelGGL(coef420_kernel, dim3((unsigned)((img_blocks + 63) / 64), n), dim3(64), 0, s, p, qt);
    else
        hipLaunchKernelGGL(coef444_kernel, dim3((unsigned)((img_blocks / 3 + 63) / 64), n), dim3(64), 0, s, p, qt);
    hipLaunchKernelGGL(length_kernel, dim3(gb, n), dim3(256), 0, s, p);
    hipLaunchKernelGGL(scan_kernel, dim3(n), dim3(256), 0, s, p);
    hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(256), 0, s, p);
    hipLaunchKernelGGL(pack_kernel, dim3(gb, n), dim3(256), 0, s, p);
    hipLaunchKernelGGL(ff_count_kernel, dim3(gc, n), dim3(256), 0, s, p);
    hipLaunchKernelGGL(ff_scan_kernel, dim3(n), dim3(256), 0, s, p);
    hipLaunchKernelGGL(file_layout_kernel, dim3(1), dim3(256), 0, s, p);
    hipLaunchKernelGGL(write_kernel, dim3(gc ? gc : 1, n), dim3(256), 0, s, p, hdr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        h->last_error = std::string("pa_jpegenc_encode: ") + hipGetErrorString(e);
        return PA_ERR_HIP;
    }
    return PA_OK;
}

int pa_jpegenc_overflows(pa_jpegenc* h, int32_t* count_host, void* stream) {
    if (!h || !count_host) return PA_ERR_INVALID_ARG;
    if (!h->ready) return PA_ERR_NOT_READY;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(count_host, h->d_overflow, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(h->d_overflow, 0, sizeof(int32_t), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        h->last_error = "pa_jpegenc_overflows: copy failed";
        return PA_ERR_HIP;
    }
    return PA_OK;
}

}  // extern "C"

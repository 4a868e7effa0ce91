// What the two JPEG decoders share (mjpeg.hip: frames of one size per call; jpegdec.hip: files of any size per call):
// the marker-segment parser and Huffman table builder of the host, and the device code of every pass as functions that
// take ONE image's descriptor -- un-stuffing, the self-synchronising entropy decoder, the scans, IDCT, up-sampling and
// colour conversion. The kernels around them decide which image a workgroup works on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "jpeg_dct.h"

namespace pa {
namespace mj {

constexpr int LB = 10;           // bits of the direct Huffman lookup
constexpr int CHUNK = 4096;      // bytes per workgroup of the marker scan (256 threads x 16 bytes)
constexpr int MAX_BLOCKS_MCU = 10;
constexpr int SUB_MIN = 128;     // bytes per subsequence (one lane) of the entropy decoder: a power of two >= this, per call
constexpr int RING_DW = 32;      // dwords of a lane's LDS ring (128 bytes of its stream)
constexpr int TOPUP = 16;        // symbols between two ring top-ups
constexpr int WG_SUBS = 256;     // subsequences per workgroup

enum { ERR_HUFF = 1, ERR_RST = 2, ERR_COEF = 4, ERR_SYNC = 8 };

// How far a symbol moves the zig-zag index (T.81 F.2.2.2): the DC symbol to 1; a coefficient RRRRSSSS past its run of
// zeros and itself; ZRL 16; EOB (libjpeg: any other symbol of size 0) beyond the end of the block from wherever it stands.
__host__ __device__ inline int symbol_advance(bool dc, int sym) {
    if (dc) return 1;
    const int s = sym & 15, r = sym >> 4;
    return s ? r + 1 : (r == 15 ? 16 : 64);
}

// Huffman tables as the decoder's lanes read them (LDS image = global layout). A 16-bit entry holds everything a symbol
// needs: code length (bits 0-4), number of extra bits s (5-8), advance of the zig-zag index (9-15); 0 = no entry.
// Codes of up to LB bits are found in lut1 under their first LB bits. Longer codes sit at the top of a canonical code
// space: whenever they all start with six 1-bits (every table whose long codes fill less than 1/64 of the code space --
// the standard tables, and what libjpeg's optimiser produces) they are found in lutB under bits 6..15, so both tables
// are read at once and neither look-up waits for the other. A code in neither table leaves both entries 0 and the lane
// walks the canonical MAXCODE list instead.
struct HuffTables {
    uint16_t lut1[4][1 << LB];  // DC0, DC1, AC0, AC1
    uint16_t lutB[4][1 << LB];
    int32_t maxcode[4][18];     // largest code of length l (-1: none); [17] = sentinel
    int32_t valoff[4][17];      // valptr[l] - mincode[l]
    uint8_t vals[4][256];
};
struct TableSet {
    HuffTables h;
    uint16_t q[4][64];  // quantisation tables, natural order
};
static_assert(sizeof(HuffTables) % 4 == 0, "copied to LDS as dwords");

struct FrameDesc {
    uint32_t scan_off, scan_len;  // entropy-coded segment inside the device byte buffer (EOI excluded)
    uint32_t clean_off;           // where the frame's un-stuffed stream starts in the clean buffer (16-byte aligned)
    int32_t ri, n_int, seg_base, tabset;
    int32_t sub_base, n_sub_cap;  // the frame's slice of the per-subsequence arrays
    uint8_t td[4], ta[4], tq[4];
};

// ---- byte un-stuffing + restart markers --------------------------------------------------------------------------------------
//
// The entropy-coded segment of every frame is rewritten once into a CLEAN stream: stuffed zeros (FF 00 -> FF) and the
// RSTm markers are removed, and the clean offset at which every restart interval starts is recorded (seg_start). Bit
// positions in the clean stream are plain arithmetic, which is what lets the decoder below start anywhere.

// per 16 raw bytes [a, a + 16) of the scan [lo, hi): bit j of `keep` = byte a + j survives, of `mark` = byte a + j is the
// 0xFF of an RSTm marker
__device__ __forceinline__ void classify16(const uint8_t* bits, uint32_t a, uint32_t lo, uint32_t hi, uint32_t& keep, uint32_t& mark,
                                           uint32_t (&w)[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(bits + a);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    const uint32_t prev = a > lo ? bits[a - 1] : 0, next = bits[a + 16];
    keep = 0;
    mark = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
        const uint32_t bp = j ? (w[(j - 1) >> 2] >> (8 * ((j - 1) & 3))) & 0xff : prev;
        const uint32_t bn = j < 15 ? (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xff : next;
        const uint32_t p = a + j;
        const bool in = p >= lo && p < hi;
        const bool is_mark = b == 0xff && (bn & 0xf8) == 0xd0 && p + 1 < hi;
        const bool drop = (bp == 0xff && p > lo && (b == 0 || (b & 0xf8) == 0xd0)) || is_mark;
        if (in && !drop) keep |= 1u << j;
        if (in && is_mark) mark |= 1u << j;
    }
}

// cnt_row[c] = (markers, kept bytes) of chunk c of the image (a workgroup of 256 threads per chunk)
__device__ __forceinline__ void unstuff_count_body(const uint8_t* __restrict__ bits, const FrameDesc& d, int2* __restrict__ cnt_row, int c) {
    __shared__ int red[8];
    const int tid = threadIdx.x;
    const uint32_t lo = d.scan_off, hi = d.scan_off + d.scan_len;
    const uint32_t a = (lo & ~15u) + (uint32_t)c * CHUNK + tid * 16;
    int nm = 0, nk = 0;
    if (a < hi) {
        uint32_t keep, mark, w[4];
        classify16(bits, a, lo, hi, keep, mark, w);
        nm = __popc(mark);
        nk = __popc(keep);
    }
    for (int o = 32; o; o >>= 1) {
        nm += __shfl_down(nm, o, 64);
        nk += __shfl_down(nk, o, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = nm;
        red[4 + (tid >> 6)] = nk;
    }
    __syncthreads();
    if (tid == 0) cnt_row[c] = make_int2(red[0] + red[1] + red[2] + red[3], red[4] + red[5] + red[6] + red[7]);
}

// chunk c of the image -> its place in the clean stream (cnt_row: the image's max_chunks counts; clean_len_f, status_f: the
// image's entries)
__device__ __forceinline__ void unstuff_write_body(const uint8_t* __restrict__ bits, const FrameDesc& d, const int2* __restrict__ cnt_row,
                                                   int max_chunks, int c, uint8_t* __restrict__ clean, uint32_t* __restrict__ seg_start,
                                                   uint32_t* __restrict__ clean_len_f, int32_t* __restrict__ status_f) {
    __shared__ int red[16];
    __shared__ int2 scan[256];
    const int tid = threadIdx.x;
    const uint32_t lo = d.scan_off, hi = d.scan_off + d.scan_len;
    if ((lo & ~15u) + (uint32_t)c * CHUNK >= hi && c != 0) return;
    // markers / kept bytes in the chunks before this one, and in the whole frame
    int bm = 0, bk = 0, tm = 0, tk = 0;
    for (int i = tid; i < max_chunks; i += 256) {
        const int2 v = cnt_row[i];
        tm += v.x;
        tk += v.y;
        if (i < c) {
            bm += v.x;
            bk += v.y;
        }
    }
    for (int o = 32; o; o >>= 1) {
        bm += __shfl_down(bm, o, 64);
        bk += __shfl_down(bk, o, 64);
        tm += __shfl_down(tm, o, 64);
        tk += __shfl_down(tk, o, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = bm;
        red[4 + (tid >> 6)] = bk;
        red[8 + (tid >> 6)] = tm;
        red[12 + (tid >> 6)] = tk;
    }
    __syncthreads();
    bm = red[0] + red[1] + red[2] + red[3];
    bk = red[4] + red[5] + red[6] + red[7];
    tm = red[8] + red[9] + red[10] + red[11];
    tk = red[12] + red[13] + red[14] + red[15];
    if (c == 0 && tid == 0) {
        *clean_len_f = (uint32_t)tk;
        seg_start[d.seg_base] = 0;
        if (tm != d.n_int - 1) atomicOr(status_f, ERR_RST);
    }
    const uint32_t a = (lo & ~15u) + (uint32_t)c * CHUNK + tid * 16;
    uint32_t keep = 0, mark = 0, w[4] = {0, 0, 0, 0};
    if (a < hi) classify16(bits, a, lo, hi, keep, mark, w);
    scan[tid] = make_int2(__popc(mark), __popc(keep));
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the per-thread counts
        int2 v = make_int2(0, 0);
        if (tid >= o) v = scan[tid - o];
        __syncthreads();
        scan[tid].x += v.x;
        scan[tid].y += v.y;
        __syncthreads();
    }
    int km = bm + scan[tid].x - __popc(mark);    // markers before this thread's bytes
    uint32_t kk = (uint32_t)(bk + scan[tid].y - __popc(keep));  // clean offset of this thread's first kept byte
    // The chunk's kept bytes are gathered in LDS, laid out like the 16-byte lines of the clean stream they go to, and
    // written with one 16-byte store per thread (byte stores only for the two lines shared with the neighbouring
    // chunks): 16 byte-wide stores per thread cost 113 us per 64 frames, this 4x less.
    __shared__ __attribute__((aligned(16))) uint8_t stage[CHUNK + 32];
    const uint32_t g0 = d.clean_off + (uint32_t)bk;  // clean-buffer offset of the chunk's first kept byte
    const uint32_t mis = g0 & 15u;
    uint32_t sl = mis + (kk - (uint32_t)bk);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (mark & (1u << j)) {
            // the interval after this marker starts at the clean offset reached so far
            ++km;
            if (km < d.n_int) seg_start[d.seg_base + km] = kk;
        }
        if (keep & (1u << j)) {
            stage[sl++] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xff);
            ++kk;
        }
    }
    __syncthreads();
    const uint32_t total = (uint32_t)scan[255].y;
    const uint32_t nlines = (mis + total + 15) >> 4;
    uint8_t* const line0 = clean + (g0 - mis);
    for (uint32_t q = tid; q < nlines; q += 256) {
        const uint32_t b0 = q == 0 ? mis : 0u;
        const uint32_t b1 = min(16u, mis + total - q * 16);
        if (b0 == 0 && b1 == 16) {
            *reinterpret_cast<uint4*>(line0 + q * 16) = *reinterpret_cast<const uint4*>(stage + q * 16);
        } else {
            for (uint32_t bb = b0; bb < b1; ++bb) line0[q * 16 + bb] = stage[q * 16 + bb];
        }
    }
}

// ---- entropy decoding --------------------------------------------------------------------------------------------------------
//
// One lane per subsequence (128 bytes or more, see below) of a frame's clean stream, wherever it falls (Weissenberger & Schmidt's
// self-synchronising scheme, restated for this layout). A lane's decoding state at a bit position is (block of the MCU,
// zig-zag index); given the right state at its entry a lane decodes exactly the codewords that START inside its
// subsequence and hands (overshoot bits, block, index) to the next lane.
//   pass A (MODE 0): every lane assumes the state of a block start at its first bit. Huffman streams re-synchronise by
//                    themselves, so most exit states are already right;
//   verify (MODE 1): every lane whose entry (= the predecessor's exit) differs from what it last decoded with decodes
//                    again; repeated until no exit state changes = the exact sequential states. Lanes that follow a
//                    restart marker are exact from the start: at a marker the state is known.
//   scan           : per frame, exclusive scan of the blocks completed, with resets at restart markers -> every lane's
//                    absolute block index at entry;
//   final (MODE 2) : decode once more and store the non-zero AC coefficients and the DC differences (int16) by block
//                    number in scan order (buffers cleared beforehand). Only this pass extracts values; the passes
//                    before it need code lengths, run lengths and sizes alone.
// The subsequence size is chosen per call (a power of two, about four MCUs of the stream: states settle within a
// couple of MCUs, so most lanes are right after pass A and one verify pass). Every lane keeps the next 128 bytes of its
// stream in an LDS ring (33-dword pitch: the 64 lanes' window reads fall on distinct banks) that all lanes top up
// together every 16 symbols with 16-byte loads; the 64-bit window is re-read from the ring at every symbol, so there is
// no refill branch inside the symbol loop.

struct SubCnt {     // what a subsequence contributes to the scan
    int32_t blk;    // blocks completed; bit 31: a restart marker lies inside, blk then counts from the frame start
};


// One workgroup of LANES lanes = subsequences wg * LANES .. of image f (descriptor d, clean length clen, subsequence size
// 1 << sh bytes, bpm blocks per MCU, tabsel: bit b = the DC table of block b of an MCU, bit 16 + b = its AC table;
// total_blocks in the scan). status / changed / changed_last / todo_cnt are indexed by f; frame_coef / frame_dc are the image's own
// (MODE 2).
template <int MODE, int LANES>
__device__ __forceinline__ void sub_decode_body(const uint8_t* __restrict__ clean, const FrameDesc& d, const TableSet* __restrict__ ts,
                                                const uint32_t* __restrict__ seg_start, const uint32_t clen, const int sh, const int bpm,
                                                const uint32_t tabsel, const int total_blocks, const int f, const int wg,
                                                const uint32_t* __restrict__ g_in, uint32_t* __restrict__ g_out,
                                                uint32_t* __restrict__ used, SubCnt* __restrict__ cnt, const SubCnt* __restrict__ entry,
                                                int16_t* __restrict__ frame_coef, int32_t* __restrict__ status, int32_t* __restrict__ changed,
                                                const int32_t* __restrict__ changed_last, const int32_t* __restrict__ todo,
                                                const int32_t* __restrict__ todo_cnt, int16_t* __restrict__ frame_dc, const bool stamp,
                                                unsigned long long* __restrict__ dbg) {
    // verify pass: a frame whose previous verify pass changed nothing has settled (changed_last = that pass's flags)
    if (MODE == 1 && changed_last && changed_last[f] == 0) return;
    __shared__ HuffTables T;
    __shared__ uint32_t ring[LANES * (RING_DW + 1)];
    const int tid = threadIdx.x;
    const int nsub = (int)((clen + (1u << sh) - 1) >> sh);
    const int j0 = wg * LANES;
    int j = j0 + tid;
    bool active;
    if (MODE == 1) {
        // a verify pass walks the COMPACT list of the frame's lanes whose entry changed (sub_verify_plan_kernel): the few
        // lanes that still move in a late pass fill whole waves instead of keeping one lane busy in every wave
        const int cnt = todo_cnt[f];
        if (j0 >= cnt) return;
        active = j < cnt;
        j = active ? todo[(size_t)d.sub_base + j] : 0;
    } else {
        if (j0 >= nsub) return;
        active = j < nsub && j < d.n_sub_cap;
    }
    if (MODE == 2 && wg == 0 && tid == 0 && changed_last[f]) atomicOr(&status[f], ERR_SYNC);
    const size_t sj = (size_t)d.sub_base + j;
    const uint32_t entry_st = (MODE == 0 || j == 0 || !active) ? 0u : g_in[sj - 1];
    const bool mine = active;  // this lane decodes in this pass and records what it found
    {   // tables, block layout of an MCU
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&ts[d.tabset].h);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
        for (int i = tid; i < (int)(sizeof(HuffTables) / 4); i += LANES) dst[i] = src[i];
    }
    __syncthreads();
    // positions are bits from the start of the frame's clean stream
    const uint32_t s_byte = (uint32_t)j << sh;
    const uint32_t end_bits = min((uint32_t)(j + 1) << sh, clen) * 8;
    uint32_t bitpos = s_byte * 8 + (entry_st & 31);
    int b = (entry_st >> 5) & 15, z = (entry_st >> 9) & 63;
    if (b >= bpm) b = 0;
    // this lane's ring: bytes [fill - 128, fill) of the stream, most significant bit first; dword X at ring[X & 31], and
    // ring[32] repeats ring[0] so that a window's two dwords are always neighbours
    uint32_t* const my_ring = ring + tid * (RING_DW + 1);
    const uint8_t* const stream = clean + d.clean_off;
    uint32_t fill = s_byte;  // multiple of 16
    auto top_up = [&]() {
        // keep the dwords (bitpos >> 5) and the one after it, fill the rest of the ring
        while (fill + 16 <= ((bitpos >> 5) << 2) + 4 * RING_DW) {
            const uint4 v = *reinterpret_cast<const uint4*>(stream + fill);
            uint32_t* q = my_ring + ((fill >> 2) & (RING_DW - 1));
            q[0] = __builtin_bswap32(v.x); q[1] = __builtin_bswap32(v.y);
            q[2] = __builtin_bswap32(v.z); q[3] = __builtin_bswap32(v.w);
            if (q == my_ring) my_ring[RING_DW] = q[0];
            fill += 16;
        }
    };
    // first restart boundary at or after this subsequence's first byte
    int nbk = d.n_int;  // index of the next boundary's interval; n_int = none
    uint32_t nb_bits = 0xffffffffu;
    if (active && d.n_int > 1) {
        int lo = 1, hi = d.n_int;  // lower_bound over seg_start[1 .. n_int)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (seg_start[d.seg_base + mid] < s_byte) lo = mid + 1; else hi = mid;
        }
        nbk = lo;
        if (nbk < d.n_int) nb_bits = seg_start[d.seg_base + nbk] * 8;
    }
    int nblk = 0, reset = 0, err = 0;
    int absblk = 0;  // MODE 2: index of the current block in scan order; else: first block of the last restart interval entered
    if (MODE == 2 && active) {
        const SubCnt e = entry[sj];
        absblk = e.blk & 0x7fffffff;
    }
    // final pass: coefficients in SCAN order (block absblk of the frame, zig-zag index inside the block), DC differences apart
    // row of T.lut1 / T.lutB for the symbol in hand: DC tables 0-1, AC tables 2-3
    auto table_row = [&](bool dc, int blk) -> uint32_t { return ((tabsel >> (blk + (dc ? 0 : 16))) & 1u) | (dc ? 0u : 2u); };
    if (MODE == 2 && active && absblk % bpm != b) {  // the scan and the synchronised state disagree: corrupt stream
        err |= ERR_SYNC;
        active = false;
    }
    uint32_t lim = min(nb_bits, end_bits);
    // the next 32 bits of the stream, straight from the ring
    auto window = [&]() -> uint32_t {
        const uint32_t* q = my_ring + ((bitpos >> 5) & (RING_DW - 1));
        return (uint32_t)(((((uint64_t)q[0]) << 32) | q[1]) << (bitpos & 31) >> 32);
    };
    const uint16_t* const lut1 = &T.lut1[0][0];
    const uint16_t* const lutB = &T.lutB[0][0];
    // what the lane hands on, captured when it reaches the end of its subsequence (it free-runs after that)
    uint32_t x_state = 0;
    int x_blk = 0;
    bool gen = false;
    // diagnostics (stamp): only the first wave of the first frame reads the clocks (s_memtime + a wait in every wave's
    // slow step was 2 % of a pass)
    unsigned long long c0 = 0, w0t = 0;
    if (stamp) {
        c0 = clock64();
        w0t = wall_clock64();
    }
    int it = 0;
    unsigned long long slow_cyc = 0;
    int outer = 0;
    while (__ballot(active)) {
        unsigned long long cs = 0;
        if (stamp) cs = clock64();
        ++outer;
        // ---- the slow step: ring top-up, restart markers, end of the subsequence, symbols the fast loop does not take
        if (MODE == 2 && absblk >= total_blocks) active = false;  // what follows the last block is padding
        if (active) {
            top_up();
            if (bitpos >= lim) {
                gen = false;
                if (bitpos >= nb_bits) {
                    // restart marker: byte aligned, block 0 of MCU nbk * ri, predictions zero (T.81 F.2.2.4 / E.2.4)
                    bitpos = nb_bits;
                    b = 0; z = 0;
                    reset = 1;
                    nblk = 0;
                    absblk = nbk * d.ri * bpm;
                    ++nbk;
                    nb_bits = nbk < d.n_int ? seg_start[d.seg_base + nbk] * 8 : 0xffffffffu;
                    lim = min(nb_bits, end_bits);
                }
                if (bitpos >= end_bits) {
                    active = false;
                    x_state = ((bitpos - end_bits) & 31) | ((uint32_t)b << 5) | ((uint32_t)z << 9);
                    // blocks since the last restart marker inside the subsequence (absblk = that marker's block), if any
                    x_blk = reset ? (int32_t)(((uint32_t)(absblk + nblk) & 0x7fffffffu) | 0x80000000u) : nblk;
                }
            } else if (gen) {
                // one symbol the general way: codes outside the look-up tables, padding in front of a marker, errors
                gen = false;
                const uint32_t win = window();
                const bool dc = z == 0;
                const uint32_t t = table_row(dc, b);
                uint32_t e = T.lut1[t][win >> (32 - LB)];
                if (e == 0 && !dc && (win >> 26) == 63) e = T.lutB[t][(win >> (26 - LB)) & ((1 << LB) - 1)];
                int len = e & 31, s = (e >> 5) & 15, adv = e >> 9;
                bool invalid = false;
                if (e == 0) {  // canonical search (T.81 F.2.2.3)
                    const uint32_t pk = win >> 16;
                    len = 17;
                    int sym = 0;
                    for (int l = LB + 1; l <= 16; ++l) {
                        const int code = (int)(pk >> (16 - l));
                        if (code <= T.maxcode[t][l]) {
                            sym = T.vals[t][(T.valoff[t][l] + code) & 255];
                            len = l;
                            break;
                        }
                    }
                    if (len == 17) {
                        // no such code: the 1-bits that pad the byte in front of a restart marker (caught below), a lane
                        // that is out of step (A / verify: move on by one bit), or a corrupt stream (final)
                        invalid = true;
                        len = 1;
                        sym = 0;
                    }
                    s = sym & 15;
                    adv = symbol_advance(dc, sym);
                }
                const int use = len + s;
                const uint32_t np = bitpos + use;
                if (np > nb_bits || (invalid && nb_bits - bitpos < 8)) {
                    bitpos = nb_bits;  // the padding bits in front of a restart marker, not a symbol
                } else if (invalid && MODE == 2) {
                    err |= ERR_HUFF;
                    active = false;
                } else {
                    bitpos = np;
                    int zn = z + adv;
                    const bool over = !dc && s && zn > 64;  // a coefficient beyond index 63
                    if (MODE == 2) {
                        const uint32_t raw = s ? (uint32_t)(win << len) >> (32 - s) : 0u;
                        const int v = (int)raw - ((int)raw < ((1 << s) >> 1) ? (1 << s) - 1 : 0);
                        if (over) {
                            err |= ERR_COEF;
                            active = false;
                        } else if (absblk < total_blocks) {
                            if (dc) {
                                frame_dc[absblk] = (int16_t)v;  // the difference; dc_scan_kernel adds the predictions up
                            } else if (s) {
                                frame_coef[(size_t)absblk * 64 + zn - 1] = (int16_t)v;
                            }
                        }
                    }
                    if (over) zn = 64;
                    if (zn >= 64) {
                        zn = 0;
                        ++nblk;
                        if (MODE == 2) ++absblk;
                        if (++b >= bpm) b = 0;
                    }
                    z = zn;
                }
            }
        }
        // ---- the fast loop: straight-line code, every lane; left as soon as one active lane meets anything else.
        // A step is two LDS round trips -- the window's two dwords from the ring, then the table look-ups side by side
        // -- and some seventy vector instructions; the passes are bound by instruction issue, not by those latencies.
        if (stamp) slow_cyc += clock64() - cs;
#pragma unroll
        for (int k = 0; k < TOPUP; ++k, ++it) {  // (`it` counts steps: a pair is one)
            const uint32_t win = window();
            const bool dc = z == 0;
            const uint32_t tb = table_row(dc, b) << LB;
            uint32_t eA = lut1[tb + (win >> (32 - LB))];
            uint32_t eB = lutB[tb + ((win >> (26 - LB)) & ((1 << LB) - 1))];
            // passes A / verify: the AC table's pair entry for these ten bits (lutB row = AC table number)
            uint32_t eP = MODE != 2 ? lutB[(tb & (1u << LB)) + (win >> (32 - LB))] : 0u;
            asm volatile("" : "+v"(eA), "+v"(eB), "+v"(eP));  // the look-ups in flight together, none behind a branch
            const uint32_t e = eA ? eA : (!dc && (win >> 26) == 63 ? eB : 0u);
            const int len = e & 31, s = (e >> 5) & 15;
            int adv = e >> 9, use = len + s;
            // two symbols in one step where the pair neither ends the block nor reaches the end of the subsequence / a
            // restart boundary (the exit state is taken at the FIRST symbol boundary behind the end)
            // (bitwise, not short-circuit: hipcc turns && chains over lane values into exec-mask branches)
            const int p_use = (int)(eP & 15), p_adv = (int)((eP >> 4) & 63), p_eob = (int)((eP >> 4) & 64);
            const bool pair = (MODE != 2) & !dc & ((eP >> 15) != 0) & (z + p_adv < 64) & (bitpos + (uint32_t)p_use < lim);
            if (MODE != 2) {
                use = pair ? p_use : use;
                adv = pair ? p_adv + p_eob : adv;  // (an EOB behind the coefficients ends the block: index beyond 64)
            }
            const uint32_t np = bitpos + use;
            const int zn = z + adv;  // DC: 1 | coefficient: past its zero run and itself | ZRL: + 16 | EOB: beyond 64
            const bool rare = !pair & ((bitpos >= lim) | (e == 0) | (np > nb_bits) | ((zn > 64) & (adv < 64)));
            if (__builtin_amdgcn_ballot_w64(active && rare) != 0) {
                gen = rare && bitpos < lim;
                break;
            }
            // commit
            bitpos = np;
            if (MODE == 2) {
                // the value (extra bits, T.81 F.2.2.1 EXTEND): nothing before the final pass needs it
                const uint32_t raw = s ? (uint32_t)(win << len) >> ((32 - s) & 31) : 0u;
                const int v = (int)raw - ((int)raw < ((1 << s) >> 1) ? (1 << s) - 1 : 0);
                // one store: the DC difference (dc_scan_kernel adds the predictions up) or a non-zero AC coefficient
                int16_t* const base = dc ? frame_dc : frame_coef;
                const uint32_t off = dc ? (uint32_t)absblk : (uint32_t)absblk * 64u + (uint32_t)(zn - 1);
                if (active && absblk < total_blocks && s) base[off] = (int16_t)v;
            }
            const bool bend = zn >= 64;
            z = bend ? 0 : zn;
            nblk += bend ? 1 : 0;
            if (MODE == 2) absblk += bend ? 1 : 0;
            const int bn = b + 1 == bpm ? 0 : b + 1;
            b = bend ? bn : b;
        }
    }
    if (stamp && tid == 0) {
        dbg[MODE * 2] = clock64() - c0;
        dbg[MODE * 2 + 1] = ((wall_clock64() - w0t) << 32) | (unsigned)it;
        dbg[8 + MODE * 2] = slow_cyc;
        dbg[8 + MODE * 2 + 1] = (unsigned)outer;
    }
    if (err) atomicOr(&status[f], err);
    if (MODE != 2 && mine) {
        if (MODE == 1 && x_state != g_in[sj]) atomicOr(&changed[f], 1);
        g_out[sj] = x_state;
        used[sj] = entry_st;
        SubCnt c;
        c.blk = x_blk;
        cnt[sj] = c;
    }
}

// Which lanes of a frame decode again in the next verify pass: those whose entry state (the predecessor's exit) is not the
// one they last decoded with. Their indices are compacted into todo[] (frame order), the others keep their exit state.
// (1024 threads; a frame that has settled is the caller's business: todo_cnt 0, nothing else)
__device__ __forceinline__ void verify_plan_body(const FrameDesc& d, const uint32_t clen, int sub_shift, const uint32_t* __restrict__ g_in,
                                                 uint32_t* __restrict__ g_out, const uint32_t* __restrict__ used, int32_t* __restrict__ todo,
                                                 int32_t* __restrict__ todo_cnt_f) {
    __shared__ int sh[1024];
    const int tid = threadIdx.x;
    int nsub = (int)((clen + (1u << sub_shift) - 1) >> sub_shift);
    nsub = nsub < d.n_sub_cap ? nsub : d.n_sub_cap;
    const int per = (nsub + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, nsub);
    int cnt = 0;
    for (int j = lo; j < hi; ++j) {
        const size_t sj = (size_t)d.sub_base + j;
        const uint32_t entry_st = j == 0 ? 0u : g_in[sj - 1];
        cnt += entry_st != used[sj] ? 1 : 0;
    }
    sh[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    int k = sh[tid] - cnt;
    for (int j = lo; j < hi; ++j) {
        const size_t sj = (size_t)d.sub_base + j;
        const uint32_t entry_st = j == 0 ? 0u : g_in[sj - 1];
        if (entry_st != used[sj]) todo[(size_t)d.sub_base + k++] = j;
        else g_out[sj] = g_in[sj];
    }
    if (tid == 1023) *todo_cnt_f = sh[1023];
}

// entry[j] = what lanes 0 .. j-1 of the frame accumulated: the absolute block index at lane j's entry
__device__ __forceinline__ void sub_scan_body(const FrameDesc& d, const uint32_t clen, const SubCnt* __restrict__ cnt,
                                              SubCnt* __restrict__ entry, int sub_shift) {
    __shared__ SubCnt sh[1024];
    const int tid = threadIdx.x;
    int nsub = (int)((clen + (1u << sub_shift) - 1) >> sub_shift);
    nsub = nsub < d.n_sub_cap ? nsub : d.n_sub_cap;
    const int per = (nsub + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, nsub);
    auto combine = [](const SubCnt& a, const SubCnt& b) {  // a then b
        if (b.blk < 0) return b;
        SubCnt r;
        r.blk = a.blk + b.blk;  // keeps a's marker bit: b.blk < 2^30
        return r;
    };
    SubCnt acc = {0};
    for (int i = lo; i < hi; ++i) acc = combine(acc, cnt[(size_t)d.sub_base + i]);
    sh[tid] = acc;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        SubCnt v = {0};
        const bool has = tid >= o;
        if (has) v = sh[tid - o];
        __syncthreads();
        if (has) sh[tid] = combine(v, sh[tid]);
        __syncthreads();
    }
    SubCnt run = {0};
    if (tid > 0) run = sh[tid - 1];
    for (int i = lo; i < hi; ++i) {
        entry[(size_t)d.sub_base + i] = run;
        run = combine(run, cnt[(size_t)d.sub_base + i]);
    }
}

// DC differences (scan order, as the final pass left them) -> DC coefficients, in place: per component a running sum over
// the component's blocks in scan order, starting again from zero at every restart interval (T.81 F.2.1.3.1 / F.2.2.4).
// One workgroup per (frame, component); every thread owns a run of consecutive blocks of the component.
// (p: the image's DC array at the component's first block of an MCU, nbc: the component's blocks per MCU, ri: restart interval)
__device__ __forceinline__ void dc_scan_body(int16_t* __restrict__ p, const int ri, const int mcus, const int bpm, const int nbc) {
    __shared__ int w_sum[16];
    __shared__ int w_flag[16];
    const int tid = threadIdx.x;
    const int n = mcus * nbc;
    const int per = (n + 1023) / 1024;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    // a thread's run, sixteen blocks at a time: the sixteen loads are in flight together (one after the other they cost a
    // memory latency each, 2 x 32 of them for the luma of a 1080p frame)
    constexpr int DCB = 16;  // loads in flight per thread
    auto walk = [&](int& run, int& flag, bool store) {
        int mcu = lo / nbc, t = lo - mcu * nbc;
        int in_ri = ri > 0 ? mcu % ri : 1;  // MCU's place in its restart interval, kept by counting (a modulo per block was
                                            // most of this kernel's instructions); without restart markers never 0
        for (int k0 = lo; k0 < hi; k0 += DCB) {
            int idx[DCB], val[DCB];
            bool rst[DCB];
#pragma unroll
            for (int i = 0; i < DCB; ++i) {
                idx[i] = mcu * bpm + t;
                rst[i] = t == 0 && in_ri == 0;
                if (++t == nbc) {
                    t = 0;
                    ++mcu;
                    if (ri > 0 && ++in_ri == ri) in_ri = 0;
                }
            }
#pragma unroll
            for (int i = 0; i < DCB; ++i) val[i] = k0 + i < hi ? (int)p[idx[i]] : 0;
#pragma unroll
            for (int i = 0; i < DCB; ++i) {
                if (k0 + i < hi) {
                    if (rst[i]) {
                        run = 0;
                        flag = 1;
                    }
                    run += val[i];
                    if (store) p[idx[i]] = (int16_t)run;
                }
            }
        }
    };
    int run = 0, flag = 0;
    walk(run, flag, false);
    // segmented inclusive scan of the threads' (sum, restart seen): a run with a restart inside forgets what precedes
    // it. Inside a wave by lane shuffles, across the sixteen waves through LDS: one barrier (twenty of them, ten scan steps
    // over 1024 threads, were most of this kernel's 54 us).
    const int lane = tid & 63, wave = tid >> 6;
    int ssum = run, sflag = flag;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int vs = __shfl_up(ssum, o), vf = __shfl_up(sflag, o);
        if (lane >= o && !sflag) {
            ssum += vs;
            sflag = vf;
        }
    }
    if (lane == 63) {
        w_sum[wave] = ssum;
        w_flag[wave] = sflag;
    }
    __syncthreads();
    int psum = 0;  // what the waves before this one leave
    for (int w = 0; w < wave; ++w) psum = w_flag[w] ? w_sum[w] : psum + w_sum[w];
    int esum = __shfl_up(ssum, 1), eflag = __shfl_up(sflag, 1);  // exclusive: the lanes before this one
    if (lane == 0) {
        esum = 0;
        eflag = 0;
    }
    run = eflag ? esum : psum + esum;
    walk(run, flag, true);
}

// ---- de-quantisation + inverse DCT -------------------------------------------------------------------------------------------

// One thread per block of the component rasters. Its coefficients lie where the scan put them: block
// mcu * blocks_per_mcu + (position inside the MCU) of the frame, zig-zag order, the DC coefficient in dc[] (dc_scan_kernel).
// (src: the block's 64 coefficients in zig-zag order, dc0: its DC coefficient, q: quantisation table in natural order)
__device__ __forceinline__ void idct_block(const uint4* __restrict__ src, const int dc0, const uint16_t* __restrict__ q,
                                           uint8_t* __restrict__ dst, const int pitch) {
    using namespace dct;
    constexpr int ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    int d[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = src[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[ZZ[i * 8 + 2 * j]] = (int)(int16_t)(w[j] & 0xffff) * (int)q[ZZ[i * 8 + 2 * j]];
            d[ZZ[i * 8 + 2 * j + 1]] = (int)(int16_t)(w[j] >> 16) * (int)q[ZZ[i * 8 + 2 * j + 1]];
        }
    }
    d[0] = dc0 * (int)q[0];
#pragma unroll
    for (int x = 0; x < 8; ++x) idct8<true>(d + x, 8);
#pragma unroll
    for (int y = 0; y < 8; ++y) idct8<false>(d + y * 8, 1);
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            lo |= (uint32_t)clamp255(d[y * 8 + x] + 128) << (8 * x);
            hi |= (uint32_t)clamp255(d[y * 8 + 4 + x] + 128) << (8 * x);
        }
        *reinterpret_cast<uint2*>(dst + (size_t)y * pitch) = make_uint2(lo, hi);
    }
}

// ---- up-sampling + colour conversion -----------------------------------------------------------------------------------------

// Chroma samples of 8 pixels x FV rows (pixel x0 .., rows y0 ..) by jdsample.c's fancy triangle filters. cw x ch = the
// component's real (down-sampled) size: libjpeg replicates ITS last row / column, not the padding of the block raster.
// With 2:1 horizontal sampling a thread needs six samples of a chroma row: four are one aligned dword, the outer two
// are the neighbouring lanes' (the lanes of a wave walk along the row), fetched from memory only at the ends of the
// wave and where the row's last column must be replicated.
__device__ __forceinline__ void chroma_row6(const uint8_t* __restrict__ row, int cx0, int cw, int pc, int lane, int (&s)[6]) {
    const uint32_t d = *reinterpret_cast<const uint32_t*>(row + min(cx0, pc - 4));
    const uint32_t l = (uint32_t)__shfl_up((int)d, 1), r = (uint32_t)__shfl_down((int)d, 1);
    if (cx0 + 5 > cw) {  // the row ends here: clamp every index
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = row[min(max(cx0 - 1 + i, 0), cw - 1)];
        return;
    }
    s[1] = d & 0xff; s[2] = (d >> 8) & 0xff; s[3] = (d >> 16) & 0xff; s[4] = d >> 24;
    s[0] = lane == 0 ? (int)row[max(cx0 - 1, 0)] : (int)(l >> 24);
    s[5] = lane == 63 ? (int)row[cx0 + 4] : (int)(r & 0xff);
}

// jdsample.c h2v2_fancy_upsample for the two output rows of chroma row s0 (sa = the row above, sb = the row below, both
// already clamped to the component): 8 output samples each
__device__ __forceinline__ void h2v2_rows(const int (&s0)[6], const int (&sa)[6], const int (&sb)[6], int cx0, int cw, int (&o0)[8],
                                          int (&o1)[8]) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        int col[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = 3 * s0[i] + (v ? sb[i] : sa[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cx = cx0 + i;
            const int e = cx == 0 ? (col[i + 1] * 4 + 8) >> 4 : (col[i + 1] * 3 + col[i] + 8) >> 4;
            const int od = cx >= cw - 1 ? (col[i + 1] * 4 + 7) >> 4 : (col[i + 1] * 3 + col[i + 2] + 7) >> 4;
            if (v) {
                o1[2 * i] = e;
                o1[2 * i + 1] = od;
            } else {
                o0[2 * i] = e;
                o0[2 * i + 1] = od;
            }
        }
    }
}

template <int FH, int FV>
__device__ __forceinline__ void chroma8(const uint8_t* __restrict__ C, int pc, int cw, int ch, int x0, int y0, int lane, int (&o)[FV][8]) {
    if (FH == 1 && FV == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[0][i] = C[(size_t)y0 * pc + min(x0 + i, cw - 1)];
    } else if (FH == 2 && FV == 1) {
        const int cx0 = x0 >> 1;
        int s[6];
        chroma_row6(C + (size_t)y0 * pc, cx0, cw, pc, lane, s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cx = cx0 + i;
            o[0][2 * i] = cx == 0 ? s[i + 1] : (3 * s[i + 1] + s[i] + 1) >> 2;
            o[0][2 * i + 1] = cx >= cw - 1 ? s[i + 1] : (3 * s[i + 1] + s[i + 2] + 2) >> 2;
        }
    } else {
        const int cx0 = x0 >> 1, cy = y0 >> 1;
        const int ya = max(cy - 1, 0), yb = min(cy + 1, ch - 1);
        int s0[6], sa[6], sb[6];
        chroma_row6(C + (size_t)cy * pc, cx0, cw, pc, lane, s0);
        chroma_row6(C + (size_t)ya * pc, cx0, cw, pc, lane, sa);
        chroma_row6(C + (size_t)yb * pc, cx0, cw, pc, lane, sb);
        h2v2_rows(s0, sa, sb, cx0, cw, o[0], o[FV - 1]);
    }
}

// One output row of 8 pixels: jdcolor.c's YCbCr -> RGB on the up-sampled chroma, three 8-byte stores.
// (o: where pixel x0 of row y goes, 8-byte aligned when the width is a multiple of 8; height x width: the image)
__device__ __forceinline__ void emit_row(const uint8_t* __restrict__ Y, int py, int height, int width, int y, int x0, bool colour,
                                         const int (&cb)[8], const int (&cr)[8], uint8_t* __restrict__ o, int rgb) {
    using namespace dct;
    if (y >= height) return;
    const uint2 yv = *reinterpret_cast<const uint2*>(Y + (size_t)y * py + x0);
    uint32_t px[24];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int yy = (int)(((i < 4 ? yv.x : yv.y) >> (8 * (i & 3))) & 0xff);
        int r = yy, gg = yy, bb = yy;
        if (colour) {
            const int xb = cb[i] - 128, xr = cr[i] - 128;
            // (24-bit multiplies: |x| <= 128 and the constants are below 2^17; the 32-bit multiply runs at a quarter of the rate)
            r = clamp255(yy + ((__mul24(91881, xr) + 32768) >> 16));
            gg = clamp255(yy + ((__mul24(-22554, xb) + 32768 + __mul24(-46802, xr)) >> 16));
            bb = clamp255(yy + ((__mul24(116130, xb) + 32768) >> 16));
        }
        px[3 * i] = (uint32_t)(rgb ? r : bb);
        px[3 * i + 1] = (uint32_t)gg;
        px[3 * i + 2] = (uint32_t)(rgb ? bb : r);
    }
    if ((width & 7) == 0) {  // whole groups of 8 pixels; row starts and x0 * 3 are multiples of 8 bytes
        uint32_t w[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | (px[4 * k + 3] << 24);
        uint2* o2 = reinterpret_cast<uint2*>(o);
        o2[0] = make_uint2(w[0], w[1]);
        o2[1] = make_uint2(w[2], w[3]);
        o2[2] = make_uint2(w[4], w[5]);
    } else {
#pragma unroll
        for (int k = 0; k < 24; ++k)
            if (x0 + k / 3 < width) o[k] = (uint8_t)px[k];
    }
}

// ---- host: marker segments ---------------------------------------------------------------------------------------------------

struct Parsed {
    int height = 0, width = 0, ncomp = 0;
    int cid[3] = {0, 0, 0}, h[3] = {1, 1, 1}, v[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    uint16_t q[4][64];
    uint8_t counts[4][16];  // DC0 DC1 AC0 AC1
    uint8_t syms[4][256];
    bool qdef[4] = {false, false, false, false}, hdef[4] = {false, false, false, false};
    int ri = 0;
    size_t scan_off = 0;
};

static const uint8_t h_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex B. Returns nullptr or what is wrong with the file.
inline const char* parse_header(const uint8_t* d, size_t n, Parsed& P) {
    if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return "no SOI marker";
    size_t pos = 2;
    bool sof = false;
    P = Parsed();  // nothing carries over from the previous file (tables, restart interval)
    memset(P.q, 0, sizeof P.q);
    memset(P.counts, 0, sizeof P.counts);
    memset(P.syms, 0, sizeof P.syms);
    for (;;) {
        if (pos + 4 > n) return "truncated before SOS";
        if (d[pos] != 0xff) return "marker expected";
        const int m = d[pos + 1];
        if (m == 0xff) {
            ++pos;
            continue;
        }
        const size_t seg = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (seg < 2 || pos + 2 + seg > n) return "truncated segment";
        const uint8_t* b = d + pos + 4;
        const size_t len = seg - 2;
        if (m == 0xdb) {
            size_t i = 0;
            while (i < len) {
                const int pq = b[i] >> 4, tq = b[i] & 15;
                if (pq != 0) return "16-bit quantisation table (not baseline)";
                if (tq > 3 || i + 65 > len) return "bad DQT";
                for (int k = 0; k < 64; ++k) P.q[tq][h_zigzag[k]] = b[i + 1 + k];
                P.qdef[tq] = true;
                i += 65;
            }
        } else if (m == 0xc0 || m == 0xc1) {
            if (len < 6 || b[0] != 8) return "only 8-bit samples";
            P.height = (b[1] << 8) | b[2];
            P.width = (b[3] << 8) | b[4];
            P.ncomp = b[5];
            if (P.ncomp != 1 && P.ncomp != 3) return "1 or 3 components expected";
            if (len < (size_t)(6 + 3 * P.ncomp)) return "bad SOF";
            for (int c = 0; c < P.ncomp; ++c) {
                P.cid[c] = b[6 + 3 * c];
                P.h[c] = b[7 + 3 * c] >> 4;
                P.v[c] = b[7 + 3 * c] & 15;
                P.tq[c] = b[8 + 3 * c];
                if (P.tq[c] > 3) return "bad quantisation table selector";
            }
            sof = true;
        } else if (m >= 0xc2 && m <= 0xcf && m != 0xc4 && m != 0xc8 && m != 0xcc) {
            return "progressive / lossless / arithmetic-coded JPEG (only baseline Huffman is decoded)";
        } else if (m == 0xc4) {
            size_t i = 0;
            while (i < len) {
                if (i + 17 > len) return "bad DHT";
                const int tc = b[i] >> 4, th = b[i] & 15;
                if (tc > 1 || th > 1) return "Huffman table id beyond the baseline's 0 / 1";
                int ns = 0;
                for (int k = 0; k < 16; ++k) ns += b[i + 1 + k];
                if (ns > 256 || i + 17 + ns > len) return "bad DHT";
                const int t = tc * 2 + th;
                memcpy(P.counts[t], b + i + 1, 16);
                memset(P.syms[t], 0, 256);
                memcpy(P.syms[t], b + i + 17, ns);
                P.hdef[t] = true;
                i += 17 + ns;
            }
        } else if (m == 0xdd) {
            if (len < 2) return "bad DRI";
            P.ri = (b[0] << 8) | b[1];
        } else if (m == 0xda) {
            if (!sof) return "SOS before SOF";
            if (len < 1 || b[0] != P.ncomp || len < (size_t)(4 + 2 * P.ncomp)) return "multi-scan file (one interleaved scan expected)";
            for (int c = 0; c < P.ncomp; ++c) {
                if (b[1 + 2 * c] != P.cid[c]) return "scan component order differs from the frame header";
                P.td[c] = b[2 + 2 * c] >> 4;
                P.ta[c] = b[2 + 2 * c] & 15;
                if (P.td[c] > 1 || P.ta[c] > 1) return "Huffman table selector beyond the baseline's 0 / 1";
                if (!P.hdef[P.td[c]] || !P.hdef[2 + P.ta[c]]) return "scan uses a Huffman table the file does not define";
                if (!P.qdef[P.tq[c]]) return "frame uses a quantisation table the file does not define";
            }
            if (b[1 + 2 * P.ncomp] != 0 || b[2 + 2 * P.ncomp] != 63) return "spectral selection in a baseline scan";
            P.scan_off = pos + 2 + seg;
            return nullptr;
        } else if (m == 0xd9) {
            return "EOI before SOS";
        }
        pos += 2 + seg;
    }
}

// Table t (0 DC0, 1 DC1, 2 AC0, 3 AC1) of a set from a DHT segment's counts / symbols.
inline void build_hufftab(HuffTables& T, int t, const uint8_t* counts, const uint8_t* syms) {
    const bool dc = t < 2;
    auto entry = [&](int len, int sym) -> uint16_t {
        return (uint16_t)(len | ((sym & 15) << 5) | (symbol_advance(dc, sym) << 9));
    };
    memset(T.lut1[t], 0, sizeof T.lut1[t]);
    memset(T.lutB[t], 0, sizeof T.lutB[t]);
    memcpy(T.vals[t], syms, 256);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        T.valoff[t][l] = k - code;
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) continue;  // over-subscribed table: left to the canonical search (and its error)
            if (l <= LB) {
                const int lo = code << (LB - l), hi = (code + 1) << (LB - l);
                for (int e = lo; e < hi; ++e) T.lut1[t][e] = entry(l, syms[k]);
            } else if (!dc && (code >> (l - 6)) == 63) {
                // six leading 1-bits: found under bits 6 .. 6 + LB - 1 of the window (AC tables only: rows 0 / 1 of
                // lutB hold the AC tables' PAIR entries, see below; a DC code of more than LB bits -- a difference
                // of 1024 or more -- takes the canonical search)
                const int rest = l - 6;  // <= 10 bits after them
                const int lo = (code & ((1 << rest) - 1)) << (LB - rest), hi = lo + (1 << (LB - rest));
                for (int e = lo; e < hi; ++e) T.lutB[t][e] = entry(l, syms[k]);
            }
        }
        T.maxcode[t][l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    T.maxcode[t][17] = 0x7fffffff;
    T.maxcode[t][0] = -1;
    T.valoff[t][0] = 0;
    if (!dc) {
        // PAIR entries of AC table t - 2 (lutB row t - 2): where the first LB bits of the window hold TWO whole symbols
        // (code + extra bits each) -- a coefficient or ZRL, then a coefficient, ZRL or EOB -- the entry gives what they
        // consume and how far they move the zig-zag index together: bit 15 set, bits 0-3 total bits (2 .. 10), bits 4-9
        // the advance of the coefficients / ZRLs (1 .. 32), bit 10: the second symbol is EOB. The passes that only look
        // for the decoder state (A, verify) take such a pair in one step.
        uint16_t* pair = T.lutB[t - 2];
        for (int w = 0; w < (1 << LB); ++w) {
            pair[w] = 0;
            const uint16_t e1 = T.lut1[t][w];
            if (!e1) continue;
            const int use1 = (e1 & 31) + ((e1 >> 5) & 15), adv1 = e1 >> 9;
            if (use1 >= LB || adv1 >= 64) continue;
            const uint16_t e2 = T.lut1[t][(w << use1) & ((1 << LB) - 1)];
            if (!e2) continue;
            const int use2 = (e2 & 31) + ((e2 >> 5) & 15), adv2 = e2 >> 9;
            if (use1 + use2 > LB) continue;
            pair[w] = adv2 >= 64 ? (uint16_t)(0x8000 | 0x400 | (use1 + use2) | (adv1 << 4))
                                 : (uint16_t)(0x8000 | (use1 + use2) | ((adv1 + adv2) << 4));
        }
    }
}

}  // namespace mj
}  // namespace pa

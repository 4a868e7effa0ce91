// Batched decode of baseline JPEG FILES OF DIFFERENT SIZES AND SAMPLINGS on the device: the detector's crop cache
// (crops/<Fighter>/<video>_<n>.jpg) -> the packed crop-image layout pa_backbone_crop_images / pa_runner_inputs consume.
//
// Replaces the cv2.imread of every cached crop in the reference's resume path (playaid/ai_runner.py:191-194, 445-446). A cache
// directory mixes YOLOv5's save_one_box crops (any size, 4:4:4) with the 128 x 128 4:2:0 files the label repair writes (:420),
// which is what pa_mjpeg_decode (one size and sampling per call, one Geom by value) refuses. The arithmetic is the frame
// decoder's -- the passes are the same device functions (jpeg_entropy.h) -- with one difference: where the chroma plane is at
// most 2 samples wide libjpeg-turbo replicates 2:1 sub-sampled chroma instead of filtering it (jdsample.c: do_fancy &&
// downsampled_width > 2), and a crop clipped by the frame border can be that narrow.
//
// What differs from mjpeg.hip is who works on what. Geometry is a device table, one ImgGeom per image, and every grid is a
// FLATTENED WORK LIST: the host lays the images' un-stuffing chunks, workgroups of subsequences, 8x8 blocks and pixel tiles
// end to end and uploads the prefix sums; a workgroup (a thread of the IDCT) finds its image by bisection. Images of one
// call differ in area by 100x and more, so "largest image x n" grids would be mostly idle. A workgroup never spans two
// images, so the sampling branch is uniform per wave. The launches per call do not depend on n, nothing waits on the host
// (exact mode apart), and the passes of an image are ordered by the stream alone: no atomics between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/playaid_hip.h"
#include "jpeg_entropy.h"

namespace pa {
namespace jd {

using namespace pa::mj;

constexpr int LANES = 64;      // subsequences per workgroup of the entropy passes: one wave, so a small crop wastes few lanes
constexpr int TILE_W = 64;     // pixel tile of the colour pass: 8 threads x 8 pixels wide ...
constexpr int TILE_ROWS = 32;  // ... 32 threads high, FV output rows each
constexpr int MAX_ROUNDS = 16;

struct ImgGeom {
    int32_t ncomp, mcus_x, mcus_y, bpm;
    int32_t hs[3], vs[3];
    int32_t bx[3];        // padded block raster of each component, blocks per row
    int32_t blk_off[3];   // first block of the component inside the image's sample planes
    int32_t b0[3], nbc[3];  // the component's blocks inside an MCU: b0 .. b0 + nbc
    int32_t blocks;       // mcus * bpm = all components' padded blocks
    int32_t height, width;
    int32_t fh, fv;       // chroma up-sampling factors (1 | 2)
    int32_t fancy;        // 2:1 chroma by the triangle filter (0: replication, chroma plane at most 2 samples wide)
    int32_t sub_shift;    // log2 of the image's subsequence size in bytes
    uint32_t tabsel;      // bit b = DC table of block b of an MCU, bit 16 + b = its AC table
    int32_t tiles_x;      // pixel tiles per tile row
    int32_t reserved;
    int64_t blk_base;     // first block of the image in the call's coefficient / DC / sample buffers
    int64_t out_off;      // byte offset of the image in the packed output
};
static_assert(sizeof(ImgGeom) % 8 == 0 && sizeof(FrameDesc) % 8 == 0, "laid out back to back in the staging block");

// the image whose work items [start[i], start[i + 1]) hold x (start[0] = 0 <= x < start[n]; empty images have none)
__device__ __forceinline__ int find_image(const int32_t* __restrict__ start, int n, int x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void stage_kernel(const uint32_t* __restrict__ a, uint32_t* __restrict__ d, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = a[i];
}

__global__ __launch_bounds__(256) void unstuff_count_kernel(const uint8_t* __restrict__ bits, const FrameDesc* __restrict__ fd,
                                                            const int32_t* __restrict__ start, int n, int2* __restrict__ chunk_cnt) {
    const int i = find_image(start, n, blockIdx.x), s0 = start[i];
    const FrameDesc d = fd[i];
    unstuff_count_body(bits, d, chunk_cnt + s0, (int)blockIdx.x - s0);
}

__global__ __launch_bounds__(256) void unstuff_write_kernel(const uint8_t* __restrict__ bits, const FrameDesc* __restrict__ fd,
                                                            const int32_t* __restrict__ start, int n, const int2* __restrict__ chunk_cnt,
                                                            uint8_t* __restrict__ clean, uint32_t* __restrict__ seg_start,
                                                            uint32_t* __restrict__ clean_len, int32_t* __restrict__ status) {
    const int i = find_image(start, n, blockIdx.x), s0 = start[i];
    const FrameDesc d = fd[i];
    unstuff_write_body(bits, d, chunk_cnt + s0, start[i + 1] - s0, (int)blockIdx.x - s0, clean, seg_start, clean_len + i, status + i);
}

template <int MODE>
__global__ __launch_bounds__(LANES) void sub_decode_kernel(const uint8_t* __restrict__ clean, const FrameDesc* __restrict__ fd,
                                                           const ImgGeom* __restrict__ ig, const int32_t* __restrict__ start, int n,
                                                           const TableSet* __restrict__ ts, const uint32_t* __restrict__ seg_start,
                                                           const uint32_t* __restrict__ clean_len, const uint32_t* __restrict__ g_in,
                                                           uint32_t* __restrict__ g_out, uint32_t* __restrict__ used, SubCnt* __restrict__ cnt,
                                                           const SubCnt* __restrict__ entry, int16_t* __restrict__ coef,
                                                           int32_t* __restrict__ status, int32_t* __restrict__ changed,
                                                           const int32_t* __restrict__ changed_last, const int32_t* __restrict__ todo,
                                                           const int32_t* __restrict__ todo_cnt, int16_t* __restrict__ dcdiff) {
    const int i = find_image(start, n, blockIdx.x);
    if (MODE == 1 && changed_last && changed_last[i] == 0) return;
    const FrameDesc d = fd[i];
    const ImgGeom* __restrict__ g = ig + i;
    const int64_t bb = g->blk_base;
    sub_decode_body<MODE, LANES>(clean, d, ts, seg_start, clean_len[i], g->sub_shift, g->bpm, g->tabsel, g->blocks, i,
                                 (int)blockIdx.x - start[i], g_in, g_out, used, cnt, entry, MODE == 2 ? coef + bb * 64 : nullptr, status,
                                 changed, changed_last, todo, todo_cnt, MODE == 2 ? dcdiff + bb : nullptr, false, nullptr);
}

__global__ __launch_bounds__(1024) void sub_verify_plan_kernel(const FrameDesc* __restrict__ fd, const ImgGeom* __restrict__ ig,
                                                               const uint32_t* __restrict__ clean_len, const uint32_t* __restrict__ g_in,
                                                               uint32_t* __restrict__ g_out, const uint32_t* __restrict__ used,
                                                               int32_t* __restrict__ todo, int32_t* __restrict__ todo_cnt,
                                                               const int32_t* __restrict__ changed_last) {
    const int i = blockIdx.x;
    if (changed_last && changed_last[i] == 0) {  // settled
        if (threadIdx.x == 0) todo_cnt[i] = 0;
        return;
    }
    const FrameDesc d = fd[i];
    verify_plan_body(d, clean_len[i], ig[i].sub_shift, g_in, g_out, used, todo, todo_cnt + i);
}

__global__ __launch_bounds__(1024) void sub_scan_kernel(const FrameDesc* __restrict__ fd, const ImgGeom* __restrict__ ig,
                                                        const uint32_t* __restrict__ clean_len, const SubCnt* __restrict__ cnt,
                                                        SubCnt* __restrict__ entry) {
    const int i = blockIdx.x;
    const FrameDesc d = fd[i];
    sub_scan_body(d, clean_len[i], cnt, entry, ig[i].sub_shift);
}

__global__ __launch_bounds__(1024) void dc_scan_kernel(int16_t* __restrict__ dc, const FrameDesc* __restrict__ fd,
                                                       const ImgGeom* __restrict__ ig) {
    const int i = blockIdx.x, c = blockIdx.y;
    const ImgGeom* __restrict__ g = ig + i;
    if (c >= g->ncomp) return;  // (an empty entry has no components)
    dc_scan_body(dc + g->blk_base + g->b0[c], fd[i].ri, g->mcus_x * g->mcus_y, g->bpm, g->nbc[c]);
}

// One thread per block of all images' component rasters.
__global__ __launch_bounds__(256) void idct_kernel(const int16_t* __restrict__ coef, const int16_t* __restrict__ dc,
                                                   const FrameDesc* __restrict__ fd, const ImgGeom* __restrict__ ig,
                                                   const int32_t* __restrict__ start, int n, const TableSet* __restrict__ ts,
                                                   uint8_t* __restrict__ planes) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= start[n]) return;
    const int i = find_image(start, n, t);
    const ImgGeom* __restrict__ g = ig + i;
    const int r = t - start[i];
    const int c = (g->ncomp > 2 && r >= g->blk_off[2]) ? 2 : ((g->ncomp > 1 && r >= g->blk_off[1]) ? 1 : 0);
    const int off_c = g->blk_off[c], bx_c = g->bx[c], hs_c = g->hs[c], vs_c = g->vs[c];
    const int rb = r - off_c;
    const int by = rb / bx_c, bx = rb - by * bx_c;
    const int my = by / vs_c, mx = bx / hs_c;
    const size_t sblk = (size_t)g->blk_base + (size_t)(my * g->mcus_x + mx) * g->bpm + g->b0[c] + (by - my * vs_c) * hs_c + (bx - mx * hs_c);
    const uint16_t* __restrict__ q = ts[fd[i].tabset].q[fd[i].tq[c]];
    const int pitch = bx_c * 8;
    uint8_t* dst = planes + ((size_t)g->blk_base + off_c) * 64 + (size_t)(by * 8) * pitch + bx * 8;
    idct_block(reinterpret_cast<const uint4*>(coef + sblk * 64), (int)dc[sblk], q, dst, pitch);
}

// six samples cx0 - 1 .. cx0 + 4 of a chroma row, libjpeg's edge replication (every index clamped to the component)
__device__ __forceinline__ void chroma_row6_clamped(const uint8_t* __restrict__ row, int cx0, int cw, int (&s)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = row[min(max(cx0 - 1 + i, 0), cw - 1)];
}

// Chroma of 8 pixels x fv rows. fh, fv, fancy are uniform over the workgroup.
__device__ __forceinline__ void chroma_px8(const uint8_t* __restrict__ C, int pc, int cw, int ch, int x0, int y0, int fh, int fv, int fancy,
                                           int (&o0)[8], int (&o1)[8]) {
    if (fh == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o0[i] = o1[i] = C[(size_t)y0 * pc + min(x0 + i, cw - 1)];
    } else if (!fancy) {  // jdsample.c h2v1_upsample / h2v2_upsample: plain replication
        const int cy = fv == 2 ? y0 >> 1 : y0;
#pragma unroll
        for (int i = 0; i < 8; ++i) o0[i] = o1[i] = C[(size_t)cy * pc + min((x0 + i) >> 1, cw - 1)];
    } else if (fv == 1) {  // h2v1_fancy_upsample
        const int cx0 = x0 >> 1;
        int s[6];
        chroma_row6_clamped(C + (size_t)y0 * pc, cx0, cw, s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cx = cx0 + i;
            o0[2 * i] = cx == 0 ? s[i + 1] : (3 * s[i + 1] + s[i] + 1) >> 2;
            o0[2 * i + 1] = cx >= cw - 1 ? s[i + 1] : (3 * s[i + 1] + s[i + 2] + 2) >> 2;
            o1[2 * i] = o0[2 * i];
            o1[2 * i + 1] = o0[2 * i + 1];
        }
    } else {  // h2v2_fancy_upsample
        const int cx0 = x0 >> 1, cy = y0 >> 1;
        const int ya = max(cy - 1, 0), yb = min(cy + 1, ch - 1);
        int s0[6], sa[6], sb[6];
        chroma_row6_clamped(C + (size_t)cy * pc, cx0, cw, s0);
        chroma_row6_clamped(C + (size_t)ya * pc, cx0, cw, sa);
        chroma_row6_clamped(C + (size_t)yb * pc, cx0, cw, sb);
        h2v2_rows(s0, sa, sb, cx0, cw, o0, o1);
    }
}

// One workgroup per pixel tile of one image: 8 pixels x FV rows per thread, written straight into the packed output.
__global__ __launch_bounds__(256) void ycc_kernel(const uint8_t* __restrict__ planes, const ImgGeom* __restrict__ ig,
                                                  const int32_t* __restrict__ start, int n, uint8_t* __restrict__ out, int rgb) {
    const int i = find_image(start, n, blockIdx.x);
    const ImgGeom* __restrict__ g = ig + i;
    const int tile = (int)blockIdx.x - start[i];
    const int tyy = tile / g->tiles_x, txx = tile - tyy * g->tiles_x;
    const bool colour = g->ncomp == 3;
    const int fh = colour ? g->fh : 1, fv = colour ? g->fv : 1;
    const int height = g->height, width = g->width;
    const int x0 = (txx * (TILE_W / 8) + (int)(threadIdx.x & 7)) * 8, y0 = (tyy * TILE_ROWS + (int)(threadIdx.x >> 3)) * fv;
    if (x0 >= width || y0 >= height) return;
    const uint8_t* fp = planes + (size_t)g->blk_base * 64;
    const int py = g->bx[0] * 8;
    const uint8_t* Y = fp + (size_t)g->blk_off[0] * 64;
    int cb[2][8], cr[2][8];
    if (colour) {
        const int pc = g->bx[1] * 8;
        const int cw = (width + fh - 1) / fh, ch = (height + fv - 1) / fv;  // jdmaster.c: downsampled_width / _height
        chroma_px8(fp + (size_t)g->blk_off[1] * 64, pc, cw, ch, x0, y0, fh, fv, g->fancy, cb[0], cb[1]);
        chroma_px8(fp + (size_t)g->blk_off[2] * 64, pc, cw, ch, x0, y0, fh, fv, g->fancy, cr[0], cr[1]);
    }
    uint8_t* o = out + g->out_off;
#pragma unroll
    for (int v = 0; v < 2; ++v)
        if (v < fv) emit_row(Y, py, height, width, y0 + v, x0, colour, cb[v], cr[v], o + ((size_t)(y0 + v) * width + x0) * 3, rgb);
}

// ---- host --------------------------------------------------------------------------------------------------------------------

struct Totals {
    size_t images_bytes = 0;
    int64_t blocks = 0, chunks = 0, subs = 0, sub_wgs = 0, segs = 0, tiles = 0;
    size_t clean = 0;
    int64_t base = 0, top = 0;  // byte range of data_host that covers every non-empty span
    int max_sub = 1;
};

struct Plan {
    std::vector<FrameDesc> fd;
    std::vector<ImgGeom> ig;
    std::vector<pa_crop_image> desc;
    std::vector<int32_t> start[4];  // chunks, workgroups of subsequences, blocks, pixel tiles
    std::vector<TableSet> sets;
    Totals t;
};

uint64_t table_hash(const Parsed& P) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t nb) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (size_t i = 0; i < nb; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    mix(P.q, sizeof P.q); mix(P.counts, sizeof P.counts); mix(P.syms, sizeof P.syms); mix(P.hdef, sizeof P.hdef);
    return h;
}

// The marker segments of n files -> descriptors, geometry, work lists (and, with_tables, the Huffman / quantisation table
// sets: files with identical DQT / DHT content share one). Returns the index of the first file that is not taken, -1 if all are.
int plan_images(const uint8_t* data, const int64_t* spans, int n, bool with_tables, Plan& pl, std::string& why) {
    pl.fd.assign(n, FrameDesc());
    pl.ig.assign(n, ImgGeom());
    pl.desc.assign(n, pa_crop_image());
    for (auto& s : pl.start) s.assign(n + 1, 0);
    pl.sets.clear();
    Totals& T = pl.t;
    T = Totals();
    std::unordered_map<uint64_t, std::vector<std::pair<int, Parsed>>> seen;
    Parsed cur;
    bool any = false;
    for (int f = 0; f < n; ++f) {
        const int64_t o = spans[2 * f], e = spans[2 * f + 1];
        FrameDesc& d = pl.fd[f];
        ImgGeom& g = pl.ig[f];
        memset(&d, 0, sizeof d);
        memset(&g, 0, sizeof g);
        pl.desc[f].offset = (int64_t)T.images_bytes;
        pl.desc[f].height = pl.desc[f].width = 0;
        for (int k = 0; k < 4; ++k) pl.start[k][f] = (int32_t)(k == 0 ? T.chunks : k == 1 ? T.sub_wgs : k == 2 ? T.blocks : T.tiles);
        g.blk_base = T.blocks;
        g.out_off = (int64_t)T.images_bytes;
        g.tiles_x = 1;
        d.sub_base = (int32_t)T.subs;
        d.seg_base = (int32_t)T.segs;
        d.clean_off = (uint32_t)T.clean;
        if (o < 0 || e < o) {
            why = "negative byte span";
            return f;
        }
        if (e == o) continue;  // no file for this entry: 0 x 0, no work
        if (const char* msg = parse_header(data + o, (size_t)(e - o), cur)) {
            why = msg;
            return f;
        }
        if (cur.height < 1 || cur.width < 1) {
            why = "zero height or width in the frame header";
            return f;
        }
        int hmax = 1, vmax = 1;
        for (int c = 0; c < cur.ncomp; ++c) {
            hmax = cur.h[c] > hmax ? cur.h[c] : hmax;
            vmax = cur.v[c] > vmax ? cur.v[c] : vmax;
        }
        if (cur.ncomp == 3) {
            const bool ok = cur.h[0] == hmax && cur.v[0] == vmax && cur.h[1] == cur.h[2] && cur.v[1] == cur.v[2] && cur.h[1] == 1 &&
                            cur.v[1] == 1 && ((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2));
            if (!ok) {
                why = "chroma sampling other than 4:4:4 / 4:2:2 / 4:2:0";
                return f;
            }
        }
        const bool single = cur.ncomp == 1;  // T.81 A.2.2: a one-component scan is not interleaved
        const int height = cur.height, width = cur.width;
        g.ncomp = cur.ncomp;
        g.mcus_x = (width + 8 * (single ? 1 : hmax) - 1) / (8 * (single ? 1 : hmax));
        g.mcus_y = (height + 8 * (single ? 1 : vmax) - 1) / (8 * (single ? 1 : vmax));
        g.fh = single ? 1 : hmax;
        g.fv = single ? 1 : vmax;
        g.fancy = (width + g.fh - 1) / g.fh > 2 ? 1 : 0;
        int nb = 0;
        int64_t off = 0;
        uint32_t tabsel = 0;
        for (int c = 0; c < cur.ncomp; ++c) {
            g.hs[c] = single ? 1 : cur.h[c];
            g.vs[c] = single ? 1 : cur.v[c];
            g.bx[c] = g.mcus_x * g.hs[c];
            g.blk_off[c] = (int32_t)off;
            off += (int64_t)g.bx[c] * g.mcus_y * g.vs[c];
            g.b0[c] = nb;
            g.nbc[c] = g.hs[c] * g.vs[c];
            for (int k = 0; k < g.nbc[c]; ++k, ++nb) {
                tabsel |= (uint32_t)(cur.td[c] & 1) << nb;
                tabsel |= (uint32_t)(cur.ta[c] & 1) << (16 + nb);
            }
            d.td[c] = (uint8_t)cur.td[c]; d.ta[c] = (uint8_t)cur.ta[c]; d.tq[c] = (uint8_t)cur.tq[c];
        }
        g.bpm = nb;
        g.tabsel = tabsel;
        const int64_t mcus = (int64_t)g.mcus_x * g.mcus_y;
        if (mcus * nb > 0x3fffffff) {
            why = "image too large";
            return f;
        }
        g.blocks = (int32_t)(mcus * nb);  // = off: the rasters are padded to whole MCUs
        g.height = height; g.width = width;
        const int fv = g.fv;
        g.tiles_x = (width + TILE_W - 1) / TILE_W;
        const int tiles_y = (height + TILE_ROWS * fv - 1) / (TILE_ROWS * fv);
        // the entropy-coded segment ends in front of the EOI marker (fill bytes may follow it)
        int64_t end = e;
        while (end - o > (int64_t)cur.scan_off + 2 && !(data[end - 2] == 0xff && data[end - 1] == 0xd9) && e - end < 16) --end;
        if (end - o >= (int64_t)cur.scan_off + 2 && data[end - 2] == 0xff && data[end - 1] == 0xd9) end -= 2; else end = e;
        if (!any) {
            T.base = o; T.top = e;
            any = true;
        }
        T.base = o < T.base ? o : T.base;
        T.top = e > T.top ? e : T.top;
        d.scan_off = (uint32_t)cur.scan_off;  // relative to the span for now (T.base is not final yet)
        d.scan_len = (uint32_t)((end - o) - (int64_t)cur.scan_off);
        d.ri = cur.ri;
        d.n_int = cur.ri ? (int32_t)((mcus + cur.ri - 1) / cur.ri) : 1;
        // Subsequence size: about 24 BLOCKS of THIS image's stream, a power of two from 256 bytes. pa_mjpeg_decode's measured
        // choice is four MCUs of a 4:2:0 stream, which is 24 blocks; how far a lane decodes before it falls into step is a
        // matter of blocks (it needs an end of block to find the zig-zag index), and four MCUs of a grey file are 4 blocks.
        const size_t per_block = d.scan_len / (size_t)(mcus * nb) + 1;
        int sh = 8;
        while ((3u << sh) / 2 < 24 * per_block && sh < 13) ++sh;
        g.sub_shift = sh;
        d.n_sub_cap = (int32_t)(((d.scan_len + (1u << sh) - 1) >> sh) + 1);
        T.max_sub = d.n_sub_cap > T.max_sub ? d.n_sub_cap : T.max_sub;
        if (with_tables) {
            const uint64_t hk = table_hash(cur);
            auto& bucket = seen[hk];
            int found = -1;
            for (auto& kv : bucket) {
                const Parsed& p = kv.second;
                if (memcmp(cur.q, p.q, sizeof cur.q) == 0 && memcmp(cur.counts, p.counts, sizeof cur.counts) == 0 &&
                    memcmp(cur.syms, p.syms, sizeof cur.syms) == 0 && memcmp(cur.hdef, p.hdef, sizeof cur.hdef) == 0) {
                    found = kv.first;
                    break;
                }
            }
            if (found < 0) {
                found = (int)pl.sets.size();
                pl.sets.emplace_back();
                TableSet& S = pl.sets.back();
                memset(&S.h, 0, sizeof S.h);
                for (int t = 0; t < 4; ++t)
                    if (cur.hdef[t]) build_hufftab(S.h, t, cur.counts[t], cur.syms[t]);
                memcpy(S.q, cur.q, sizeof S.q);
                bucket.emplace_back(found, cur);
            }
            d.tabset = found;
        }
        pl.desc[f].height = height;
        pl.desc[f].width = width;
        T.images_bytes += ((size_t)height * width * 3 + 15) & ~(size_t)15;
        T.blocks += g.blocks;
        T.chunks += (int64_t)(d.scan_len / CHUNK) + 2;
        T.subs += d.n_sub_cap;
        T.sub_wgs += (d.n_sub_cap + LANES - 1) / LANES;
        T.segs += d.n_int;
        T.tiles += (int64_t)g.tiles_x * tiles_y;
        T.clean += ((size_t)d.scan_len + 31) & ~(size_t)15;
        if (T.blocks > 0x7fffffff || T.chunks > 0x7fffffff || T.subs > 0x7fffffff || T.tiles > 0x7fffffff || T.clean > 0xe0000000ull) {
            why = "the call's work lists exceed 2^31 entries";
            return f;
        }
    }
    for (int k = 0; k < 4; ++k) pl.start[k][n] = (int32_t)(k == 0 ? T.chunks : k == 1 ? T.sub_wgs : k == 2 ? T.blocks : T.tiles);
    for (int f = 0; f < n; ++f)  // scan offsets inside the uploaded byte range
        if (spans[2 * f + 1] > spans[2 * f]) pl.fd[f].scan_off += (uint32_t)(spans[2 * f] - T.base);
    return -1;
}

}  // namespace jd
}  // namespace pa

using namespace pa::mj;
using namespace pa::jd;

struct pa_jpegdec {
    int device = 0, max_images = 0;
    int64_t max_blocks = 0;
    size_t max_bytes = 0, clean_bytes = 0;
    int64_t max_subs = 0, max_segs = 0, max_chunks = 0;
    // verify passes enqueued per call. A pass over an image that has settled returns at once, so the passes beyond the third or
    // so cost their launches only; one call holds images of every kind (a noise-like crop at quality 95 has few ends of block
    // and settles slowly), so the default is the most the flag rows hold rather than pa_mjpeg's 8.
    int sync_rounds = MAX_ROUNDS;
    // device scratch of one call (calls on a handle are stream-ordered with each other)
    uint8_t* d_bits = nullptr;
    uint8_t* d_clean = nullptr;
    uint8_t* d_stage = nullptr;  // ImgGeom[n] FrameDesc[n] pa_crop_image[n] start[4][n + 1] TableSet[sets]
    int2* d_chunk = nullptr;
    uint32_t* d_seg = nullptr;
    uint32_t* d_clean_len = nullptr;
    uint32_t* d_g[2] = {nullptr, nullptr};
    uint32_t* d_used = nullptr;
    SubCnt* d_cnt = nullptr;
    SubCnt* d_entry = nullptr;
    int32_t* d_changed = nullptr;  // [MAX_ROUNDS + 1][max_images]
    int32_t* d_todo = nullptr;
    int32_t* d_todo_cnt = nullptr;
    int16_t* d_coef = nullptr;
    int16_t* d_dc = nullptr;
    uint8_t* d_planes = nullptr;
    int32_t* d_status = nullptr;
    // pinned staging; the device reads it itself (stage_kernel), `staged` says when it has
    uint8_t* h_stage = nullptr;
    size_t stage_bytes = 0;
    int32_t* h_flag = nullptr;
    hipEvent_t staged = nullptr;
    bool staged_used = false;
    pa::jd::Plan plan;
    std::string last_error;
};

namespace {
size_t stage_size(size_t n, size_t sets) {
    return n * (sizeof(ImgGeom) + sizeof(FrameDesc) + sizeof(pa_crop_image)) + 4 * (n + 1) * sizeof(int32_t) + 8 + sets * sizeof(TableSet);
}
}  // namespace

extern "C" {

const char* pa_jpegdec_last_error(const pa_jpegdec* h) { return h ? h->last_error.c_str() : "null handle"; }

void pa_jpegdec_destroy(pa_jpegdec* h) {
    if (!h) return;
    void* dev[] = {h->d_bits, h->d_clean, h->d_stage, h->d_chunk, h->d_seg, h->d_clean_len, h->d_g[0], h->d_g[1], h->d_used, h->d_cnt,
                   h->d_entry, h->d_changed, h->d_todo, h->d_todo_cnt, h->d_coef, h->d_dc, h->d_planes, h->d_status};
    if (h->d_bits) (void)hipDeviceSynchronize();
    for (void* p : dev) (void)hipFree(p);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_flag) (void)hipHostFree(h->h_flag);
    if (h->staged) (void)hipEventDestroy(h->staged);
    delete h;
}

int pa_jpegdec_create(int32_t device, int32_t max_images, int64_t max_blocks, size_t max_bytes, pa_jpegdec** out) {
    if (!out) return PA_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_images < 1 || max_images > (1 << 20) || max_blocks < 1 || max_blocks > 0x3fffffff || max_bytes < 1024 || max_bytes > 0xe0000000ull)
        return PA_ERR_INVALID_ARG;
    pa_jpegdec* h = new pa_jpegdec();
    *out = h;  // handed back on failure too (pa_jpegdec_last_error, then pa_jpegdec_destroy)
    h->device = device; h->max_images = max_images; h->max_blocks = max_blocks; h->max_bytes = max_bytes;
    auto chk = [&](hipError_t e, const char* what) -> bool {
        if (e == hipSuccess) return true;
        h->last_error = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    if (!chk(hipSetDevice(device), "hipSetDevice")) return PA_ERR_NO_DEVICE;
    const size_t n = (size_t)max_images;
    h->max_chunks = (int64_t)(max_bytes / CHUNK) + 2 * (int64_t)n + 2;
    h->max_subs = (int64_t)(max_bytes / SUB_MIN) + 2 * (int64_t)n + 2;
    h->max_segs = max_blocks + (int64_t)n + 1;  // a restart interval holds at least one MCU
    h->clean_bytes = max_bytes + 32 * n + 4096;
    h->stage_bytes = stage_size(n, n);
    const size_t nb = (size_t)max_blocks;
    if (!chk(hipMalloc(&h->d_bits, max_bytes + 64), "hipMalloc bitstream")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_clean, h->clean_bytes), "hipMalloc clean stream")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_stage, h->stage_bytes), "hipMalloc descriptors")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_chunk, (size_t)h->max_chunks * sizeof(int2)), "hipMalloc chunk counts")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_seg, (size_t)h->max_segs * sizeof(uint32_t)), "hipMalloc restart positions")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_clean_len, n * sizeof(uint32_t)), "hipMalloc clean lengths")) return PA_ERR_HIP;
    for (int i = 0; i < 2; ++i)
        if (!chk(hipMalloc(&h->d_g[i], (size_t)h->max_subs * sizeof(uint32_t)), "hipMalloc states")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_used, (size_t)h->max_subs * sizeof(uint32_t)), "hipMalloc states")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_cnt, (size_t)h->max_subs * sizeof(SubCnt)), "hipMalloc counts")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_entry, (size_t)h->max_subs * sizeof(SubCnt)), "hipMalloc entries")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_changed, (MAX_ROUNDS + 1) * n * sizeof(int32_t)), "hipMalloc flags")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_todo, (size_t)h->max_subs * sizeof(int32_t)), "hipMalloc lane lists")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_todo_cnt, n * sizeof(int32_t)), "hipMalloc lane counts")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_coef, nb * 64 * sizeof(int16_t)), "hipMalloc coefficients")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_dc, nb * sizeof(int16_t)), "hipMalloc DC differences")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_planes, nb * 64), "hipMalloc sample planes")) return PA_ERR_HIP;
    if (!chk(hipMalloc(&h->d_status, n * sizeof(int32_t)), "hipMalloc status")) return PA_ERR_HIP;
    if (!chk(hipMemset(h->d_bits, 0, max_bytes + 64), "hipMemset")) return PA_ERR_HIP;
    if (!chk(hipMemset(h->d_clean, 0, h->clean_bytes), "hipMemset")) return PA_ERR_HIP;
    if (!chk(hipHostMalloc(&h->h_stage, h->stage_bytes), "hipHostMalloc")) return PA_ERR_HIP;
    if (!chk(hipHostMalloc(&h->h_flag, n * sizeof(int32_t)), "hipHostMalloc")) return PA_ERR_HIP;
    if (!chk(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming), "hipEventCreate")) return PA_ERR_HIP;
    return PA_OK;
}

int pa_jpegdec_set_sync_rounds(pa_jpegdec* h, int32_t rounds) {
    if (!h || rounds < 0 || rounds > MAX_ROUNDS) return PA_ERR_INVALID_ARG;
    h->sync_rounds = rounds;
    return PA_OK;
}

int pa_jpegdec_plan(const uint8_t* data_host, const int64_t* spans_host, int32_t n, pa_crop_image* desc_host, size_t* images_bytes,
                    int64_t* blocks, char* why, size_t why_bytes) {
    if (why && why_bytes) why[0] = 0;
    if (!data_host || !spans_host || n < 1) return PA_ERR_INVALID_ARG;
    pa::jd::Plan pl;
    std::string msg;
    const int bad = plan_images(data_host, spans_host, n, false, pl, msg);
    if (bad >= 0) {
        if (why && why_bytes) snprintf(why, why_bytes, "image %d: %s", bad, msg.c_str());
        return PA_ERR_INVALID_ARG;
    }
    if (desc_host) memcpy(desc_host, pl.desc.data(), (size_t)n * sizeof(pa_crop_image));
    if (images_bytes) *images_bytes = pl.t.images_bytes;
    if (blocks) *blocks = pl.t.blocks;
    return PA_OK;
}

int pa_jpegdec_decode(pa_jpegdec* h, const uint8_t* data_host, const int64_t* spans_host, int32_t n, int32_t bgr, uint8_t* images_dev,
                      size_t images_capacity, pa_crop_image* desc_dev, int32_t* status_dev, void* stream) {
    if (!h) return PA_ERR_INVALID_ARG;
    auto bad = [&](int code, const std::string& msg) { h->last_error = msg; return code; };
    if (!data_host || !spans_host || !images_dev || !desc_dev || n < 1 || ((uintptr_t)images_dev & 15))
        return bad(PA_ERR_INVALID_ARG, "pa_jpegdec_decode: bad argument (images_dev is 16-byte aligned)");
    if (n > h->max_images) return bad(PA_ERR_CAPACITY, "pa_jpegdec_decode: more images than max_images");
    pa::jd::Plan& pl = h->plan;
    std::string msg;
    const int badf = plan_images(data_host, spans_host, n, true, pl, msg);
    if (badf >= 0) return bad(PA_ERR_INVALID_ARG, "pa_jpegdec_decode: image " + std::to_string(badf) + ": " + msg);
    const Totals& T = pl.t;
    const int64_t total = T.top - T.base;
    if (T.blocks > h->max_blocks) return bad(PA_ERR_CAPACITY, "pa_jpegdec_decode: the images' 8x8 blocks exceed max_blocks");
    if ((size_t)total > h->max_bytes) return bad(PA_ERR_CAPACITY, "pa_jpegdec_decode: compressed bytes exceed max_bytes");
    if (T.images_bytes > images_capacity) return bad(PA_ERR_CAPACITY, "pa_jpegdec_decode: the decoded images exceed images_capacity");
    if (T.chunks > h->max_chunks || T.subs > h->max_subs || T.segs > h->max_segs || T.clean + 4096 > h->clean_bytes)
        return bad(PA_ERR_CAPACITY, "pa_jpegdec_decode: the files' entropy-coded segments add up to more than max_bytes holds");
    hipStream_t s = (hipStream_t)stream;
    auto chk = [&](hipError_t e, const char* what) -> bool {
        if (e == hipSuccess) return true;
        h->last_error = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    };
    if (!chk(hipSetDevice(h->device), "hipSetDevice")) return PA_ERR_HIP;
    // the staging block of the call before this one has been read
    if (h->staged_used && !chk(hipEventSynchronize(h->staged), "hipEventSynchronize")) return PA_ERR_HIP;
    const size_t N = (size_t)n, n_sets = pl.sets.size();
    const size_t o_ig = 0, o_fd = o_ig + N * sizeof(ImgGeom), o_desc = o_fd + N * sizeof(FrameDesc),
                 o_start = o_desc + N * sizeof(pa_crop_image), o_ts = (o_start + 4 * (N + 1) * sizeof(int32_t) + 7) & ~(size_t)7,
                 used_bytes = o_ts + n_sets * sizeof(TableSet);
    memcpy(h->h_stage + o_ig, pl.ig.data(), N * sizeof(ImgGeom));
    memcpy(h->h_stage + o_fd, pl.fd.data(), N * sizeof(FrameDesc));
    memcpy(h->h_stage + o_desc, pl.desc.data(), N * sizeof(pa_crop_image));
    for (int k = 0; k < 4; ++k) memcpy(h->h_stage + o_start + (size_t)k * (N + 1) * sizeof(int32_t), pl.start[k].data(), (N + 1) * sizeof(int32_t));
    if (n_sets) memcpy(h->h_stage + o_ts, pl.sets.data(), n_sets * sizeof(TableSet));
    const ImgGeom* d_ig = reinterpret_cast<const ImgGeom*>(h->d_stage + o_ig);
    const FrameDesc* d_fd = reinterpret_cast<const FrameDesc*>(h->d_stage + o_fd);
    const int32_t* d_start = reinterpret_cast<const int32_t*>(h->d_stage + o_start);
    const int32_t *st_chunk = d_start, *st_wg = d_start + (N + 1), *st_blk = d_start + 2 * (N + 1), *st_tile = d_start + 3 * (N + 1);
    const TableSet* d_ts = reinterpret_cast<const TableSet*>(h->d_stage + o_ts);
    {
        const int ndw = (int)(used_bytes / 4);
        hipLaunchKernelGGL(stage_kernel, dim3((ndw + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(h->h_stage),
                           reinterpret_cast<uint32_t*>(h->d_stage), ndw);
    }
    if (!chk(hipEventRecord(h->staged, s), "hipEventRecord")) return PA_ERR_HIP;
    h->staged_used = true;
    if (!chk(hipMemcpyAsync(desc_dev, h->d_stage + o_desc, N * sizeof(pa_crop_image), hipMemcpyDeviceToDevice, s), "write descriptors")) return PA_ERR_HIP;
    if (!chk(hipMemsetAsync(h->d_status, 0, N * sizeof(int32_t), s), "clear status")) return PA_ERR_HIP;
    if (!chk(hipMemsetAsync(h->d_clean_len, 0, N * sizeof(uint32_t), s), "clear lengths")) return PA_ERR_HIP;
    if (!chk(hipMemsetAsync(h->d_changed, 0, (size_t)(MAX_ROUNDS + 1) * h->max_images * sizeof(int32_t), s), "clear flags")) return PA_ERR_HIP;
    if (T.blocks > 0) {
        if (total > 0 && !chk(hipMemcpyAsync(h->d_bits, data_host + T.base, (size_t)total, hipMemcpyHostToDevice, s), "upload bitstream")) return PA_ERR_HIP;
        // readers run a few bytes past the end of a scan: zeros behind the last byte of the call
        if (!chk(hipMemsetAsync(h->d_bits + total, 0, 64, s), "pad bitstream")) return PA_ERR_HIP;
        if (!chk(hipMemsetAsync(h->d_coef, 0, (size_t)T.blocks * 64 * sizeof(int16_t), s), "clear coefficients")) return PA_ERR_HIP;
        if (!chk(hipMemsetAsync(h->d_dc, 0, (size_t)T.blocks * sizeof(int16_t), s), "clear DC differences")) return PA_ERR_HIP;
        hipLaunchKernelGGL(pa::jd::unstuff_count_kernel, dim3((unsigned)T.chunks), dim3(256), 0, s, h->d_bits, d_fd, st_chunk, n, h->d_chunk);
        hipLaunchKernelGGL(pa::jd::unstuff_write_kernel, dim3((unsigned)T.chunks), dim3(256), 0, s, h->d_bits, d_fd, st_chunk, n, h->d_chunk,
                           h->d_clean, h->d_seg, h->d_clean_len, h->d_status);
        const dim3 sgrid((unsigned)T.sub_wgs);
        int cur_g = 0;
        hipLaunchKernelGGL((pa::jd::sub_decode_kernel<0>), sgrid, dim3(LANES), 0, s, h->d_clean, d_fd, d_ig, st_wg, n, d_ts, h->d_seg,
                           h->d_clean_len, (const uint32_t*)nullptr, h->d_g[0], h->d_used, h->d_cnt, (const SubCnt*)nullptr, (int16_t*)nullptr,
                           h->d_status, (int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr,
                           (int16_t*)nullptr);
        auto verify = [&](int slot, int prev_slot) {
            int32_t* flag = h->d_changed + (size_t)slot * h->max_images;
            const int32_t* prev = prev_slot >= 0 ? h->d_changed + (size_t)prev_slot * h->max_images : nullptr;
            hipLaunchKernelGGL(pa::jd::sub_verify_plan_kernel, dim3(n), dim3(1024), 0, s, d_fd, d_ig, h->d_clean_len, h->d_g[cur_g],
                               h->d_g[cur_g ^ 1], h->d_used, h->d_todo, h->d_todo_cnt, prev);
            hipLaunchKernelGGL((pa::jd::sub_decode_kernel<1>), sgrid, dim3(LANES), 0, s, h->d_clean, d_fd, d_ig, st_wg, n, d_ts, h->d_seg,
                               h->d_clean_len, h->d_g[cur_g], h->d_g[cur_g ^ 1], h->d_used, h->d_cnt, (const SubCnt*)nullptr,
                               (int16_t*)nullptr, h->d_status, flag, prev, h->d_todo, h->d_todo_cnt, (int16_t*)nullptr);
            cur_g ^= 1;
        };
        int last_slot = MAX_ROUNDS;  // an all-zero row unless a verify pass wrote it
        if (h->sync_rounds > 0) {
            for (int r = 0; r < h->sync_rounds; ++r) verify(r, r - 1);
            last_slot = h->sync_rounds - 1;
        } else {
            // exact mode: verify until a pass changes nothing, looking at the flags on the host (synchronises the stream)
            int rounds = 0;
            for (;;) {
                if (!chk(hipMemsetAsync(h->d_changed, 0, (size_t)h->max_images * sizeof(int32_t), s), "clear flags")) return PA_ERR_HIP;
                verify(0, -1);
                ++rounds;
                if (!chk(hipMemcpyAsync(h->h_flag, h->d_changed, N * sizeof(int32_t), hipMemcpyDeviceToHost, s), "read flags")) return PA_ERR_HIP;
                if (!chk(hipStreamSynchronize(s), "hipStreamSynchronize")) return PA_ERR_HIP;
                bool any = false;
                for (int f = 0; f < n; ++f) any = any || h->h_flag[f] != 0;
                if (!any) break;
                if (rounds > T.max_sub + 2) return bad(PA_ERR_HIP, "pa_jpegdec_decode: synchronisation did not settle");
            }
            last_slot = 0;
        }
        hipLaunchKernelGGL(pa::jd::sub_scan_kernel, dim3(n), dim3(1024), 0, s, d_fd, d_ig, h->d_clean_len, h->d_cnt, h->d_entry);
        hipLaunchKernelGGL((pa::jd::sub_decode_kernel<2>), sgrid, dim3(LANES), 0, s, h->d_clean, d_fd, d_ig, st_wg, n, d_ts, h->d_seg,
                           h->d_clean_len, h->d_g[cur_g], (uint32_t*)nullptr, h->d_used, h->d_cnt, h->d_entry, h->d_coef, h->d_status,
                           (int32_t*)nullptr, h->d_changed + (size_t)last_slot * h->max_images, (const int32_t*)nullptr,
                           (const int32_t*)nullptr, h->d_dc);
        hipLaunchKernelGGL(pa::jd::dc_scan_kernel, dim3(n, 3), dim3(1024), 0, s, h->d_dc, d_fd, d_ig);
        hipLaunchKernelGGL(pa::jd::idct_kernel, dim3((unsigned)((T.blocks + 255) / 256)), dim3(256), 0, s, h->d_coef, h->d_dc, d_fd, d_ig,
                           st_blk, n, d_ts, h->d_planes);
        hipLaunchKernelGGL(pa::jd::ycc_kernel, dim3((unsigned)T.tiles), dim3(256), 0, s, h->d_planes, d_ig, st_tile, n, images_dev, bgr ? 0 : 1);
    }
    if (status_dev && !chk(hipMemcpyAsync(status_dev, h->d_status, N * sizeof(int32_t), hipMemcpyDeviceToDevice, s), "copy status"))
        return PA_ERR_HIP;
    if (!chk(hipGetLastError(), "kernel launch")) return PA_ERR_HIP;
    return PA_OK;
}

}  // extern "C"

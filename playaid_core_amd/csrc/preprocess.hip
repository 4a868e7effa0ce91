// Crop preprocessing on gfx950: frame + normalised box -> 128x128 model input.
//
// Device-side equivalent of YoloCrop.square_crop(frame, 128, padding=30)
// (playaid/fighter.py:323-381) followed by the BGR2RGB + /255 of
// playaid/ai_runner.py:448,463. The reference composes three third-party
// resamplers; each is reproduced bit-for-bit in integer / IEEE arithmetic:
//
//   1. numpy slice of the padded square      (fighter.py:335-343)
//   2. Pillow ImageOps.pad(slice, (d,d))     (fighter.py:346-357)
//        = ImageOps.contain (aspect-preserving BICUBIC resize, 22-bit fixed
//          point, horizontal pass then vertical pass, u8 between the passes)
//          pasted centred on a black d x d canvas
//   3. imutils.resize(width=128) = cv2.resize(INTER_AREA) to (128, int(d*(128/d)))
//        (fighter.py:364) -- copy / 2x2 / integer-scale / fractional paths
//   4. ImageOps.pad to 128x128 when step 3 produced 127 rows (fighter.py:369-373)
//
// This file is compiled with -ffp-contract=off: the coefficient tables are
// computed in double precision exactly as Pillow's precompute_coeffs does, and
// the INTER_AREA fractional path accumulates in fp32 with separate multiply
// and add like OpenCV's generic C++ -- a fused multiply-add would change bits.
//
// The stage is HBM/L2 streaming work: one thread per output
// element, consecutive lanes on consecutive bytes (the matrix shapes in it are the fused
// kernel's two bicubic passes, on the int8 matrix instruction). Five small kernels keep every
// size general (any box, any frame): a fused LDS kernel for crops whose bands fit 48 KB,
// a multi-pass fallback over global scratch for the rest.
//
// Where the pieces live: the reference arithmetic itself -- the plan's geometry, the INTER_AREA branch and pixel, Pillow's
// tables and output values, the matrix forms' digits -- is crop_math.h's, once each and host-compilable; what needs
// PreprocParams (slice / intermediates / tables of a crop, the two global-memory passes, the plan kernels' head and tail)
// is crop_common.h's, shared with crop_sized.hip. This file holds the 128 path's kernels -- plan (its sub-band and
// matrix-form search), operand builder, fallback, the fused kernel as stage functions (cf_*) under its band loop (the
// vector form of its horizontal pass alone stays inline: see there) -- and the
// runner-input, rectangle, box-projection and window-upload kernels.
#include "crop_common.h"
#ifdef PA_STAMP_BUILD
#include <cstdio>
#include <vector>
#endif
#include "../../include/playaid_hip.h"
#include <cstdlib>

namespace pa {


// Rows each stage must hold in LDS to produce output rows [r0, r1) of the
// 128-row crop: canvas rows [dy0,dy1) -> resized rows [ry0,ry1) -> slice rows
// [ty0,ty1) (the vertical pass's taps).
struct BandRows {
    int dy0, dy1, ry0, ry1, ty0, ty1;
};

__device__ __forceinline__ BandRows band_rows(const CropPlan& pl, int r0, int r1) {
    BandRows b;
    b.dy0 = b.dy1 = b.ry0 = b.ry1 = b.ty0 = b.ty1 = 0;
    if (r1 > pl.out_h) r1 = pl.out_h;
    if (r0 >= r1) return b;
    if (pl.area_mode == 0) {
        b.dy0 = r0;
        b.dy1 = r1;
    } else if (pl.area_mode == 1) {
        b.dy0 = 2 * r0;
        b.dy1 = 2 * r1;
    } else if (pl.area_mode == 2) {
        b.dy0 = r0 * pl.iscale_y;
        b.dy1 = r1 * pl.iscale_y;
    } else {
        const AreaTab t0 = area_tab(r0, pl.scale_y, pl.d);
        const AreaTab t1 = area_tab(r1 - 1, pl.scale_y, pl.d);
        b.dy0 = t0.s_first;
        b.dy1 = t1.s_first + t1.n;
    }
    int ry0 = b.dy0 - pl.py, ry1 = b.dy1 - pl.py;
    ry0 = ry0 < 0 ? 0 : (ry0 > pl.rh ? pl.rh : ry0);
    ry1 = ry1 < 0 ? 0 : (ry1 > pl.rh ? pl.rh : ry1);
    b.ry0 = ry0;
    b.ry1 = ry1;
    if (ry1 <= ry0) return b;
    if (pl.need_v) {
        int ymin, cnt;
        bicubic_bounds(pl.sh, pl.rh, ry0, &ymin, &cnt);
        b.ty0 = ymin;
        bicubic_bounds(pl.sh, pl.rh, ry1 - 1, &ymin, &cnt);
        b.ty1 = ymin + cnt;
    } else {
        b.ty0 = ry0;
        b.ty1 = ry1;
    }
    return b;
}

__device__ __forceinline__ int align_up(int v, int a) { return (v + a - 1) / a * a; }

// LDS layout of one sub-band: B0 source rows | B1 after the horizontal pass; B2 (after the
// vertical pass) reuses B0's space when both passes run (B0 is dead once H is done).
// With CropPlan::mfma_v the vertical pass runs on v_mfma_i32_32x32x32_i8 and B1 is kept TRANSPOSED, [byte column][source
// row]: byte (col, row) at off1 + col * pt + (col >> 3) * skew + row -- a lane of the pass reads the 16 consecutive rows of
// its byte column as one operand. pt is the row count rounded up to 4 (the horizontal pass stores four rows as one dword);
// where pt / 4 is even, one dword of skew per 8 columns spreads those stores (3 * pt / 4 dwords apart from lane to lane) and
// the operand reads (pt / 4 apart) over the 64 banks. Columns are padded to whole 32-column blocks, 32 B of slack behind the
// last (a lane reads rows up to 31 of its column whatever pt is: they meet zero coefficients). Behind the stage buffers,
// at offc, the pass's coefficient operand: three base-256 digit planes [digit][resized row 0..31][source row 0..31], int8.
struct BandLds {
    int p0, p1;          // row pitches in bytes (multiples of 4)
    int off1, off2, total;
    int pt, skew;        // transposed B1 (mfma_v): column pitch, bytes of skew per 8 columns; pt == 0: B1 is row-major
    int offc;            // coefficient operand (mfma_v)
};

// Sub-bands the matrix form covers: one instruction tile, N = 32 resized rows from K = 32 source rows. (A second K block
// would never run: with both passes at <= 7 taps, more than 32 source rows of B0 and B1 do not fit the kernel's LDS budget.)
constexpr int CF_MFMA_N = 32, CF_MFMA_K = 32;

__device__ __forceinline__ BandLds band_lds(const CropPlan& pl, const BandRows& b) {
    BandLds l;
    l.p0 = align_up(pl.sw * 3, 4) + 4;
    // matrix-form horizontal pass: a row holds the slice's bytes behind their misalignment (aligned staging), and the
    // pitch is an odd number of dwords -- the pass's 32 lanes of a half read the same dwords of 32 rows, on 32 banks
    if (pl.mfma_h) l.p0 = align_up(pl.h_mis + pl.sw * 3, 4) | 4;
    l.p1 = align_up(pl.rw * 3, 4) + 4;
    l.pt = l.skew = l.offc = 0;
    const int n0 = b.ty1 - b.ty0, n2 = b.ry1 - b.ry0;
    int s1 = align_up(n0 * l.p1, 16);
    if (pl.mfma_v) {
        // B2's rows hold whole 32-column blocks (the pass stores every column of its last block) and lie 2 x odd dwords
        // apart: the pass's 64 lanes store one dword each to 32 rows x 2 neighbouring dwords, on 64 different banks
        const int pt4 = (n0 + 3) >> 2, nblk = (pl.rw * 3 + 31) >> 5;
        if (l.p1 < nblk * 32) l.p1 = nblk * 32;
        while (((l.p1 >> 2) & 3) != 2) l.p1 += 4;
        l.pt = pt4 * 4;
        l.skew = (pt4 & 1) ? 0 : 4;
        s1 = align_up(nblk * 32 * l.pt + nblk * 4 * l.skew + 32, 16);
    }
    const int s0 = align_up(n0 * l.p0, 16), s2 = align_up(n2 * l.p1, 16);
    l.off1 = s0;
    if (pl.need_h && pl.need_v) {
        // B2 reuses B0's space only when it fits there: the vertical pass reads B1 while it writes B2, so a B2
        // larger than B0 (an enlarging slice: more / wider resized rows than source rows) must not reach B1
        if (s2 <= s0) {
            l.off2 = 0;
            l.total = s0 + s1;
        } else {
            l.off2 = s0 + s1;
            l.total = s0 + s1 + s2;
        }
    } else if (pl.need_h) {
        l.off2 = 0;  // unused
        l.total = s0 + s1;
    } else if (pl.need_v) {
        l.off2 = s0;
        l.total = s0 + s2;
    } else {
        l.off2 = 0;
        l.total = s0;
    }
    if (pl.mfma_v) {
        l.offc = l.total;
        l.total += 3 * CF_MFMA_N * CF_MFMA_K;
    }
    return l;
}

// One wave per crop: every lane derives the geometry (cheap, identical), then the lanes
// share the search for the largest LDS sub-band (128 candidate sub-bands in parallel).
// Workgroup = one crop: wave 0 plans, then all four waves fill the crop's two Pillow coefficient tables.
__global__ __launch_bounds__(256) void crop_plan_kernel(const PreprocParams p) {
    __shared__ CropPlan plan_sh;
    const int crop = blockIdx.x;
    if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    CropPlan pl = crop_plan_geometry(p, crop, PA_CROP);  // (every lane: cheap, identical)
    if (p.ablate & 16) pl.fused_rb = 2;
    if (pl.status == PA_CROP_OK && pl.area_mode != 4 && !(p.ablate & 16)) {
        // largest sub-band height whose LDS stages fit the fused kernel's budget. At each height the matrix form of the
        // vertical pass is tried first (both passes, <= 7 taps, every sub-band within one 32 x 32 operand tile); where its
        // transposed B1 and operand space do not fit, the vector form at the same height comes before a lower height.
        // (not under the timing ablations of either pass: a skipped pass leaves the other with the wrong layout of B1)
        const int mfma_ok = p.crop_mfma && pl.need_h && pl.need_v && pl.ksize_v <= 7 && !(p.ablate & 6);
        // The horizontal pass takes the matrix form too (tried first, m == 2) where its filter has <= 7 taps, the slice's rows
        // share one byte misalignment (row pitch a multiple of 4), the crop's blocks of PA_HOP_PIXELS output pixels fit the
        // operand scratch, and the taps of every block -- THIS pass's own bounds, clipped slices included -- lie within the
        // PA_HOP_WINDOW bytes behind the aligned dword that holds the block's first tap (lane = block).
        int h_mode = 0, h_mis = 0;
        if (mfma_ok && p.crop_mfma_h && p.hop && pl.ksize_h <= 7) {
            size_t pitch;
            const uint8_t* sp = slice_ptr(p, crop, pl, &pitch);
            const int nb = (pl.rw + PA_HOP_PIXELS - 1) / PA_HOP_PIXELS;
            if ((pitch & 3) == 0 && nb <= PA_HOP_BLOCKS_MAX) {
                h_mode = p.crop_mfma_h == 2 ? 2 : 1;
                h_mis = h_mode == 2 ? 0 : (int)((uintptr_t)sp & 3);
                int fit = 1;
                if (lane < nb) {
                    const int x0 = lane * PA_HOP_PIXELS, x1 = x0 + PA_HOP_PIXELS - 1 < pl.rw - 1 ? x0 + PA_HOP_PIXELS - 1 : pl.rw - 1;
                    int lo, cnt, lo1, cnt1;
                    bicubic_bounds(pl.sw, pl.rw, x0, &lo, &cnt);
                    bicubic_bounds(pl.sw, pl.rw, x1, &lo1, &cnt1);  // (first tap and end are monotone in the output coordinate)
                    fit = ((h_mis + 3 * lo) & 3) + 3 * (lo1 + cnt1 - lo) <= PA_HOP_WINDOW;
                }
                if (__ballot(!fit) != 0ull) h_mode = 0;
            }
        }
#pragma unroll 1
        for (int rb = 8; rb >= 1 && pl.fused_rb == 0; rb >>= 1) {
#pragma unroll 1
            for (int m = mfma_ok ? (h_mode ? 2 : 1) : 0; m >= 0 && pl.fused_rb == 0; --m) {
                pl.mfma_v = m >= 1;
                pl.mfma_h = m == 2 ? h_mode : 0;
                pl.h_mis = m == 2 ? h_mis : 0;
                int worst = 0;
#pragma unroll 1
                for (int r0 = lane * rb; r0 < PA_CROP; r0 += 64 * rb) {
                    const BandRows b = band_rows(pl, r0, r0 + rb);
                    int need = band_lds(pl, b).total;
                    if (m && (b.ty1 - b.ty0 > CF_MFMA_K || b.ry1 - b.ry0 > CF_MFMA_N)) need = 1 << 30;
                    worst = need > worst ? need : worst;
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const int o = __shfl_xor(worst, d, 64);
                    worst = o > worst ? o : worst;
                }
                if (worst <= p.fused_lds) pl.fused_rb = rb;
            }
        }
        if (pl.fused_rb == 0) pl.mfma_v = pl.mfma_h = pl.h_mis = 0;
    }
    if (lane == 0) {
        if (pl.status == PA_CROP_OK && pl.fused_rb == 0) {
            const int slot = atomicAdd(p.fallback_count, 1);
            p.fallback_list[slot] = crop;
        }
        crop_plan_publish(p, crop, pl);
        plan_sh = pl;
    }
    }
    __syncthreads();
    const CropPlan pl = plan_sh;
    if (pl.status != PA_CROP_OK) return;
    // cv::computeResizeAreaTab for the 128 destination columns and rows (fp64 with divisions): once per crop, not once
    // per workgroup of the fused kernel
    if (pl.area_mode == 3 && p.area_tabs && !(p.ablate & 32)) {
        const int t = threadIdx.x;
        AreaTabPacked q = {0u, 0.f, 0.f, 0.f};
        if (t < PA_CROP) q = area_pack(area_tab(t, pl.scale_x, pl.d));
        else if (t - PA_CROP < pl.out_h) q = area_pack(area_tab(t - PA_CROP, pl.scale_y, pl.d));
        p.area_tabs[(size_t)crop * 2 * PA_CROP + t] = q;
    }
    crop_plan_fill_tables(p, crop, pl);
}

// The engine's coefficient cache: table d = the pass (2 * (d / 2) + 2 * padding -> d), at row d * (d - 1) / 2.
__global__ __launch_bounds__(256) void coef_cache_kernel(int32_t* __restrict__ cache, int padding, int dmax) {
    const int d = blockIdx.y + 1, xx = blockIdx.x * 256 + threadIdx.x;
    if (d > dmax || xx >= d) return;
    bicubic_coef_row(2 * (d / 2) + 2 * padding, d, xx, cache + ((size_t)d * (d - 1) / 2 + xx) * COEF_ROW);
}

// The horizontal matrix form's operand, once per crop (CropPlan::mfma_h) and call, block by block of PA_HOP_PIXELS
// output pixels. The pass computes B1[source row][output byte column] from the block's PA_HOP_WINDOW-byte window of the
// staged row as int8 products with this [window byte][column] matrix of coefficient digits -- non-zero only at the
// <= 7 taps x 3 channels of a column, at window byte s + 3 * (tap pixel - first pixel of the block) + channel, where s is
// the first tap's byte offset inside its aligned dword (slice misalignment included). Zero-fill, then scatter the digits
// in fragment order (pa_kernels.h: PA_HOP_BLOCK_BYTES), so that a wave of the pass loads a fragment as one 1 KB read.
// A workgroup builds PA_HOP_WG_BLOCKS neighbouring blocks, so that the loads of their taps are in flight together and the
// crops of a clip take one round of workgroups.
constexpr int PA_HOP_WG_BLOCKS = 4;
__global__ __launch_bounds__(256) void crop_hop_kernel(const PreprocParams p) {
    const int crop = blockIdx.y, blk0 = blockIdx.x * PA_HOP_WG_BLOCKS, tid = threadIdx.x;
    const CropPlan* plp = p.plans + crop;
    if (plp->status != PA_CROP_OK || !plp->mfma_h) return;
    const int rw = plp->rw, h_mis = plp->h_mis;
    int nblk = (rw + PA_HOP_PIXELS - 1) / PA_HOP_PIXELS;
    nblk = nblk < PA_HOP_BLOCKS_MAX ? nblk : PA_HOP_BLOCKS_MAX;  // (the plan's own condition: never write outside the crop's operand)
    const int here = nblk - blk0 < PA_HOP_WG_BLOCKS ? nblk - blk0 : PA_HOP_WG_BLOCKS;
    if (here <= 0) return;
    const int32_t* coef = plp->coef_h;
    uint8_t* ob0 = p.hop + ((size_t)crop * PA_HOP_BLOCKS_MAX + blk0) * PA_HOP_BLOCK_BYTES;
    for (int i = tid; i < here * (6 * 1024 / 16); i += 256) {
        const int u = i / (6 * 1024 / 16), j = i - u * (6 * 1024 / 16);
        reinterpret_cast<uint4*>(ob0 + (size_t)u * PA_HOP_BLOCK_BYTES)[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (tid < here * 33) {  // the blocks' tails: 32 constants and the window base each
        const int u = tid / 33, e = tid - u * 33, x0 = (blk0 + u) * PA_HOP_PIXELS;
        int v = 0;
        if (e == 32) {
            v = (h_mis + 3 * coef[(size_t)x0 * COEF_ROW]) & ~3;
        } else if (e < 3 * PA_HOP_PIXELS && x0 + e / 3 < rw) {
            v = coef_row_constant(coef + (size_t)(x0 + e / 3) * COEF_ROW);
        }
        reinterpret_cast<int32_t*>(ob0 + (size_t)u * PA_HOP_BLOCK_BYTES + 6 * 1024)[e] = v;
    }
    // thread = (output byte column, tap) of every block of the workgroup: all loads first
    const int n = tid >> 3, t = tid & 7;
    const int px = n / 3, c = n - 3 * px;
    int xmin0[PA_HOP_WG_BLOCKS], xmin[PA_HOP_WG_BLOCKS], cnt[PA_HOP_WG_BLOCKS], k[PA_HOP_WG_BLOCKS];
#pragma unroll
    for (int u = 0; u < PA_HOP_WG_BLOCKS; ++u) {
        const int x0 = (blk0 + u) * PA_HOP_PIXELS, xx = x0 + px;
        const bool on = u < here && n < 3 * PA_HOP_PIXELS && xx < rw && t < 7;
        const int32_t* row = coef + (size_t)(on ? xx : 0) * COEF_ROW;
        xmin0[u] = coef[(size_t)(on ? x0 : 0) * COEF_ROW];
        xmin[u] = row[0];
        cnt[u] = on ? row[1] : 0;
        k[u] = row[2 + (t < 7 ? t : 0)];
    }
    __syncthreads();  // the zeros are in place before the digits
#pragma unroll
    for (int u = 0; u < PA_HOP_WG_BLOCKS; ++u) {
        const int first = h_mis + 3 * xmin0[u];
        const int kidx = (first & 3) + 3 * (xmin[u] + t - xmin0[u]) + c;
        if (t < cnt[u] && kidx >= 0 && kidx < PA_HOP_WINDOW) {  // (the plan checked the window; never write outside the block)
            int d0, d1, d2;
            coef_digits(k[u], &d0, &d1, &d2);
            // fragment (digit, half window): lane = (window byte's 16-byte quarter & 1) * 32 + column, its byte kidx & 15
            uint8_t* o = ob0 + (size_t)u * PA_HOP_BLOCK_BYTES + (kidx >> 5) * 1024 + (((kidx >> 4) & 1) * 32 + n) * 16 + (kidx & 15);
            o[0 * 2048] = (uint8_t)d2;
            o[1 * 2048] = (uint8_t)d1;
            o[2 * 2048] = (uint8_t)d0;
        }
    }
}

// Four clip8 as one dword, bytes in argument order: v_ashr_pk_u8_i32 shifts two int32 right, saturates each to 0..255 and
// packs them into bytes 0 and 1 -- what hipcc itself selects for this pattern. Bits 16..31 of its result are not zero on
// gfx950 (hipcc 7.2 combines its own uses as if they were: the note at the vector form of the vertical pass), so the two
// results are joined by byte selection (v_perm_b32), which never looks at them. Used by the matrix form of the pass only.
__device__ __forceinline__ uint32_t clip8_pk4(int a, int b, int c, int d) {
    // (the builtin, not inline assembly: the compiler then keeps the wait states between a matrix instruction and this read)
    const uint32_t lo = __builtin_amdgcn_ashr_pk_u8_i32(a, b, PRECISION_BITS), hi = __builtin_amdgcn_ashr_pk_u8_i32(c, d, PRECISION_BITS);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// ---------------------------------------------------------------------------
// Multi-pass fallback for crops whose bands exceed the fused kernel's LDS budget (very
// large boxes): same arithmetic, intermediates in global scratch (t1, t2). One workgroup
// walks the compact list the plan kernel built and runs the three passes of a crop back to
// back (workgroup barrier + fence between them), so the common case -- empty list -- costs
// one tiny launch.
// The two bicubic passes are crop_common.h's (crop_pass_h / crop_pass_v), shared with crop_sized.hip.
// channel swap + u8 crop + zero-bordered NHWC4 model input for pixel i of `crop`: k / 255 as fp32 or bf16, or the integers k as bf16
__device__ __forceinline__ void write_crop_pixel(const PreprocParams& p, int crop, int i, int o0, int o1, int o2) {
    if (p.swap_rb) {
        const int t = o0;
        o0 = o2;
        o2 = t;
    }
    if (p.crops_u8) {
        uint8_t* o = p.crops_u8 + ((size_t)crop * PA_CROP * PA_CROP + i) * 3;
        o[0] = (uint8_t)o0;
        o[1] = (uint8_t)o1;
        o[2] = (uint8_t)o2;
    }
    if (p.crops_f32) {
        const int dy = i >> 7, dx = i & 127;
        const size_t o = ((size_t)crop * 134 + (dy + 3)) * 134 + (dx + 3);
        if (p.crops_f32_is_bf16 == 2) {  // integer stem: the pixel integers themselves, each exactly one bf16 (the stem divides its sums)
            reinterpret_cast<uint2*>(p.crops_f32)[o] = make_uint2(u8_bf16x2(o0, o1), u8_bf16x2(o2, 0));
            return;
        }
        float4 v;
        v.x = (float)o0 / 255.0f;
        v.y = (float)o1 / 255.0f;
        v.z = (float)o2 / 255.0f;
        v.w = 0.f;
        if (p.crops_f32_is_bf16) {  // bf16 conv path: the /255 quotient rounded to bf16 (nearest even)
            reinterpret_cast<uint2*>(p.crops_f32)[o] = make_uint2(pack_bf16x2(v.x, v.y), f32_to_bf16(v.z));
        } else {
            reinterpret_cast<float4*>(p.crops_f32)[o] = v;
        }
    }
}

// INTER_AREA from the global-memory intermediates, final black pad to 128 rows.
__device__ void fallback_area(const PreprocParams& p, int crop, const CropPlan& pl) {
    const Canvas cv = crop_canvas(p, crop, pl);
    const AreaGeom g = area_geom(pl, PA_CROP);
    for (int i = threadIdx.x; i < PA_CROP * PA_CROP; i += blockDim.x) {
        const int dy = i >> 7, dx = i & 127;
        int o0 = 0, o1 = 0, o2 = 0;
        if (dy < pl.out_h) area_pixel(g, cv, dy, dx, o0, o1, o2);
        write_crop_pixel(p, crop, i, o0, o1, o2);
    }
}

// Runs as the LAST row of crop_fused_kernel's grid (blockIdx.y == number of crops): no launch of its own.
__device__ void crop_fallback_body(const PreprocParams& p, int band) {
    const int count = *p.fallback_count;
    for (int fb = band; fb < count; fb += gridDim.x) {
        const int crop = p.fallback_list[fb];
        const CropPlan pl = p.plans[crop];
        crop_pass_h(p, crop, pl, threadIdx.x, blockDim.x);
        __threadfence();
        __syncthreads();
        crop_pass_v(p, crop, pl, threadIdx.x, blockDim.x);
        __threadfence();
        __syncthreads();
        fallback_area(p, crop, pl);
    }
    // re-arm the list for the next call (every block has read `count`; the last one to leave resets it)
    __syncthreads();
    if (threadIdx.x == 0) {
        const int done = atomicAdd(p.fallback_count + 1, 1) + 1;
        if (done == (int)gridDim.x) {
            p.fallback_count[1] = 0;
            __threadfence();
            p.fallback_count[0] = 0;
        }
    }
}

// ---------------------------------------------------------------------------
// Fused path: one workgroup = 8 output rows of one crop, every intermediate in
// LDS. Per sub-band of fused_rb rows:
//   stage 0  slice rows [ty0,ty1) -> B0, dword loads, re-aligned with
//            v_alignbyte so every LDS row starts on a 4-byte boundary
//   stage H  Pillow horizontal pass B0 -> B1 (thread = output column, its
//            <= 15 fixed-point coefficients live in registers across the rows)
//   stage V  Pillow vertical pass B1 -> B2 (thread = 4 output bytes: one
//            ds_read_b32 per tap row feeds four accumulators)
//   stage A  INTER_AREA from B2 (black outside the paste) -> u8 crop + fp32 input
// With CropPlan::mfma_v / mfma_h stages V / H run on the int8 matrix instruction instead; with mfma_h
// stage 0 copies the frame's aligned dwords as they are.
// The frame is read from HBM exactly once (about 0.42 MB per crop at 1080p).
extern __shared__ __attribute__((aligned(16))) uint8_t pa_smem[];

struct LdsCanvas {
    int base, pitch;  // byte offset of resized row ry0 in pa_smem, row pitch
    int px, py, rw, ry0, ry1;
    __device__ __forceinline__ void load(int y, int x, int& c0, int& c1, int& c2) const {
        y -= py;
        x -= px;
        if (y >= ry0 && y < ry1 && (unsigned)x < (unsigned)rw) {
            const int o = base + (y - ry0) * pitch + x * 3;
            c0 = pa_smem[o];
            c1 = pa_smem[o + 1];
            c2 = pa_smem[o + 2];
        } else {
            c0 = c1 = c2 = 0;
        }
    }
};

__device__ __forceinline__ const int32_t* uniform_ptr(const int32_t* q) {
    const uintptr_t v = (uintptr_t)q;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const int32_t*>(((uintptr_t)hi << 32) | lo);
}

constexpr int CF_NT = 512;         // threads of a crop_fused_kernel workgroup
constexpr int CF_NW = CF_NT / 64;   // its waves
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// One 32 x 32 tile of exact bicubic sums on the int8 matrix instruction, for both passes: the pixels (offset to p - 128) as
// NA A fragments of 32 K values each, the coefficients' base-256 digits (crop_math.h: coef_digits) as B fragments b[3][NA],
// digit 2 first, cst the lane's column constant (coef_row_constant). Horner over the digits in one accumulator tile:
// ((D_2 << 8) + D_1 << 8) + D_0 + constant, the constant added with the middle digit (wrapping int32 arithmetic; the total
// itself fits).
template <int NA>
__device__ __forceinline__ i32x16 mfma_digits_tile(const i32x4* a, const i32x4* b, int cst) {
    i32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // digit 2, 1, 0
#pragma unroll
        for (int h = 0; h < NA; ++h) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[h], b[NA * j + h], acc, 0, 0, 0);
        if (j < 2) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = (int)(((uint32_t)acc[e] << 8) + (j == 1 ? (uint32_t)cst : 0u));
        }
    }
    return acc;
}

// ---- stage 0: slice rows [ty0, ty0 + n0) -> B0 (aligned dwords) ------------------------------------------------------
// wave w takes rows w, w+8, ...; its lanes take consecutive dwords of the row, four
// independent 256-byte segments in flight per iteration (the loop is latency-bound).
// Aligned copy, for the matrix-form horizontal pass: the frame's own aligned dwords, one load each -- the rows share the
// misalignment h_mis (row pitch a multiple of 4) and the pass's operand places its taps behind it. The first
// and last dword of a row are whole dwords that hold a byte of the slice, so they lie inside the frame buffer.
__device__ __forceinline__ void cf_stage_aligned(const uint8_t* slice, size_t frame_pitch, int row_dwords, int ty0, int n0, int p0, int wave,
                                                 int lane) {
    for (int y = wave; y < n0; y += CF_NW) {
        const uintptr_t ga = (uintptr_t)(slice + (size_t)(ty0 + y) * frame_pitch);
        const uint32_t* g4 = reinterpret_cast<const uint32_t*>(ga & ~(uintptr_t)3);
        uint32_t* dst = reinterpret_cast<uint32_t*>(pa_smem + y * p0);
        for (int j0 = 0; j0 < row_dwords; j0 += 256) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + lane + 64 * u;
                v[u] = j < row_dwords ? g4[j] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + lane + 64 * u;
                if (j < row_dwords) dst[j] = v[u];
            }
        }
    }
}

// Re-aligning copy (v_alignbyte): every LDS row starts on the slice row's first byte
__device__ __forceinline__ void cf_stage_realign(const uint8_t* slice, size_t frame_pitch, int sw, int ty0, int n0, int p0, int wave, int lane) {
    const int row_dwords = (sw * 3 + 3) >> 2;
    const int row_bytes = sw * 3;
    for (int y = wave; y < n0; y += CF_NW) {
        const uintptr_t ga = (uintptr_t)(slice + (size_t)(ty0 + y) * frame_pitch);
        const uint32_t* g4 = reinterpret_cast<const uint32_t*>(ga & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(ga & 3);  // wave-uniform misalignment of this row
        uint32_t* dst = reinterpret_cast<uint32_t*>(pa_smem + y * p0);
        for (int j0 = 0; j0 < row_dwords; j0 += 256) {
            uint32_t lo[4], hi[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + lane + 64 * u;
                lo[u] = j < row_dwords ? g4[j] : 0u;
                // the next dword is only dereferenced when the row really straddles it
                hi[u] = (sh && j < row_dwords && 4 * (j + 1) < (int)sh + row_bytes) ? g4[j + 1] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + lane + 64 * u;
                if (j < row_dwords) dst[j] = __builtin_amdgcn_alignbyte(hi[u], lo[u], sh);
            }
        }
    }
}

// ---- the matrix-form vertical pass's coefficient operand ----------------------------------------------------------------
// once per workgroup and sub-band, over zeros (the band outside the taps): thread = (resized row, tap).
// k = d0 + 256 d1 + 65536 d2 with d0, d1 in [-128, 127]; digit plane j holds d_j at [row][first tap + t]
__device__ __forceinline__ void cf_v_operand(const int32_t* coef_v, const BandRows b, const BandLds L, int tid) {
    const int n = tid >> 3, t = tid & 7;
    if (tid < CF_MFMA_N * 8 && n < b.ry1 - b.ry0) {
        const int32_t* row = coef_v + (uint32_t)(b.ry0 + n) * (uint32_t)COEF_ROW;  // (scalar base + 32-bit lane offset)
        const int rel = row[0] - b.ty0 + t;
        if (t < row[1] && t < 7 && rel >= 0 && rel < CF_MFMA_K) {
            int d0, d1, d2;
            coef_digits(row[2 + t], &d0, &d1, &d2);
            uint8_t* c = pa_smem + L.offc + n * CF_MFMA_K + rel;
            c[0] = (uint8_t)d0;
            c[CF_MFMA_N * CF_MFMA_K] = (uint8_t)d1;
            c[2 * CF_MFMA_N * CF_MFMA_K] = (uint8_t)d2;
        }
    }
}

// ---- stage H: B0 -> B1 -------------------------------------------------------------------------------------------------
// Matrix form: B1[source row m][output byte column] of a block of PA_HOP_PIXELS output pixels = the block's
// 64-byte window of row m x the crop's operand (crop_hop_kernel), digit by digit as in the vertical pass
// below. A = 32 source rows x 64 window bytes: a lane (row lane & 31, half lane >> 5) reads bytes
// 16 half .. + 15 of each 32-byte step of its row from B0, - 128 = one XOR per dword; rows past the band's
// end repeat its last row, window bytes past the row's end meet zero digits. B = the operand's fragments,
// straight from global memory (L2: the crop's 16 workgroups share them), column lane & 31, the same bytes.
// Result register 4g + e of a lane is source row 8g + 4 (lane >> 5) + e of column lane & 31: a register
// group is one dword of the transposed B1 the vertical pass reads. A wave takes every eighth block.
__device__ __forceinline__ void cf_h_mfma(const uint8_t* hop, int rw, const BandLds L, int n0, int wave, int lane) {
    const int n = lane & 31, half = lane >> 5;
    const int nb = (rw + PA_HOP_PIXELS - 1) / PA_HOP_PIXELS, rw3 = rw * 3;
    const int arow = (n < n0 ? n : n0 - 1) * L.p0 + half * 16;
    // The window bases of all of this wave's blocks come in one load before the loop (lane i: its i-th block), and
    // a block's six fragments and constants are requested together ahead of the reads of B0 -- a tile would
    // otherwise wait for L2 four times in a row (base -> B0 address, then fragment pair by fragment pair).
    int wb_all = 0;
    if (wave + CF_NW * lane < nb)
        wb_all = reinterpret_cast<const int32_t*>(hop + (size_t)(wave + CF_NW * lane) * PA_HOP_BLOCK_BYTES + 6 * 1024)[32];
    int it = 0;
    for (int blk = wave; blk < nb; blk += CF_NW, ++it) {
        const uint8_t* ob = hop + (size_t)blk * PA_HOP_BLOCK_BYTES;
        i32x4 bf[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) bf[f] = (reinterpret_cast<const i32x4*>(ob) + lane)[f * 64];
        const int cst = reinterpret_cast<const int32_t*>(ob + 6 * 1024)[n];
        int wbase = __builtin_amdgcn_readlane(wb_all, it);
        // (the builder wrote a dword offset inside the row; clamped all the same, so that a read never leaves LDS)
        wbase = wbase < 0 ? 0 : (wbase > L.p0 ? L.p0 : wbase) & ~3;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(pa_smem + arow + wbase);
        i32x4 a[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[0][q] = (int)(src[q] ^ 0x80808080u);
            a[1][q] = (int)(src[8 + q] ^ 0x80808080u);
        }
        const i32x16 acc = mfma_digits_tile<2>(a, bf, cst);
        const int col = blk * (3 * PA_HOP_PIXELS) + n;
        if (n < 3 * PA_HOP_PIXELS && col < rw3) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(pa_smem + L.off1 + col * L.pt + (col >> 3) * L.skew + half * 4);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (8 * g + 4 * half < L.pt) dst[2 * g] = clip8_pk4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        }
    }
}

// ---- stage V: (B1 | B0) -> B2 ------------------------------------------------------------------------------------------
// Matrix form: B2[resized row n][byte column] = clip8((2^21 + sum_k B1[k][column] * coef[n][k]) >> 22) as three
// int8 products D_j = (B1 - 128) x digit_j, one v_mfma_i32_32x32x32_i8 each: A = 32 byte
// columns x 32 source rows (a lane: its column's 16 consecutive rows from the transposed B1, -128 = one XOR per
// dword), B = the digit plane, 32 source rows x 32 resized rows (a lane: resized row lane & 31, the same 16 source
// rows as its A fragment, so the order of k inside the instruction does not matter). With the resized row's
// constant 2^21 + 128 * sum(coef), the exact int32 sum Pillow accumulates is D_0 + (D_1 << 8) + (D_2 << 16) + constant.
// A wave takes every eighth 32-column block; the B fragments stay in registers over its blocks.
__device__ __forceinline__ void cf_v_mfma(const int32_t* coef_v, int rw, const BandRows b, const BandLds L, int wave, int lane) {
    const int n = lane & 31, hk = (lane >> 5) * 16, n2 = b.ry1 - b.ry0;
    const int nblk = (rw * 3 + 31) >> 5;
    const uint8_t* cop = pa_smem + L.offc + n * CF_MFMA_K + hk;  // + j * CF_MFMA_N * CF_MFMA_K: digit plane j
    i32x4 bop[3];  // digit 2, 1, 0
#pragma unroll
    for (int j = 0; j < 3; ++j) bop[j] = *reinterpret_cast<const i32x4*>(cop + (2 - j) * CF_MFMA_N * CF_MFMA_K);
    int cst = 0;
    if (n < n2) cst = coef_row_constant(coef_v + (uint32_t)(b.ry0 + n) * (uint32_t)COEF_ROW);
    uint32_t* dst = reinterpret_cast<uint32_t*>(pa_smem + L.off2 + n * L.p1 + (lane >> 5) * 4);
    for (int blk = wave; blk < nblk; blk += CF_NW) {
        const int col = blk * 32 + n;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(pa_smem + L.off1 + col * L.pt + (col >> 3) * L.skew + hk);
        i32x4 a;
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = (int)(src[q] ^ 0x80808080u);
        const i32x16 acc = mfma_digits_tile<1>(&a, bop, cst);
        // result register 4g + e of a lane: byte column 32 blk + 8g + 4 (lane >> 5) + e of resized row lane & 31,
        // so a register group is one dword of B2's row (whose pitch holds the whole last block)
        if (n < n2) {
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[blk * 8 + 2 * g] = clip8_pk4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        }
    }
}

// hipcc 7.2 fuses "two (x >> 22) clamped to u8, packed" into v_ashr_pk_u8_i32
// and then ORs its result as if bits 16..31 were zero; on gfx950 they are not,
// which corrupted bytes 2 and 3 of every dword. The empty asm keeps the four
// clamped values opaque so the pack is plain shifts and ORs.
__device__ __forceinline__ uint32_t clip8_x4(int a0, int a1, int a2, int a3) {
    uint32_t c0 = clip8(a0), c1 = clip8(a1), c2 = clip8(a2), c3 = clip8(a3);
    asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// Vector form: wave w takes output rows w, w+8, ...: the row's coefficients are wave-uniform (loaded
// once), each lane produces 4 bytes from one ds_read_b32 per tap row.
__device__ __forceinline__ void cf_v_vector(const int32_t* coef_v, int rw, int ksize_v, const BandRows b, const BandLds L, int in_base, int in_pitch,
                                            int wave, int lane) {
    const int n2 = b.ry1 - b.ry0;
    const int row_dwords = (rw * 3 + 3) >> 2;
    const uint32_t* lds32 = reinterpret_cast<const uint32_t*>(pa_smem);
    const int pitch_dw = in_pitch >> 2;
    for (int yy = wave; yy < n2; yy += CF_NW) {
        const int32_t* row = coef_v + (size_t)(b.ry0 + yy) * COEF_ROW;
        const int ymin = row[0], cnt = row[1];
        const int s0 = (in_base >> 2) + (ymin - b.ty0) * pitch_dw;
        uint32_t* dst = reinterpret_cast<uint32_t*>(pa_smem + L.off2 + yy * L.p1);
        if (ksize_v <= 7) {
            // common case: 7 taps fully unrolled (a 15-way unroll spilled the coefficient
            // array to scratch); taps beyond cnt have zero coefficients and re-read the
            // last valid row
            int k[7];
#pragma unroll
            for (int t = 0; t < 7; ++t) k[t] = t < cnt ? row[2 + t] : 0;
            for (int j0 = 0; j0 < row_dwords; j0 += 256) {
                // four independent dwords per lane: 28 LDS reads in flight
                int acc[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[u][c] = 1 << (PRECISION_BITS - 1);
#pragma unroll
                for (int t = 0; t < 7; ++t) {
                    const int tr = t < cnt ? t : cnt - 1;
                    uint32_t v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + lane + 64 * u;
                        v[u] = lds32[s0 + tr * pitch_dw + (j < row_dwords ? j : row_dwords - 1)];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[u][0] += __mul24((int)(v[u] & 0xff), k[t]);
                        acc[u][1] += __mul24((int)((v[u] >> 8) & 0xff), k[t]);
                        acc[u][2] += __mul24((int)((v[u] >> 16) & 0xff), k[t]);
                        acc[u][3] += __mul24((int)(v[u] >> 24), k[t]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + lane + 64 * u;
                    const uint32_t packed = clip8_x4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
                    if (j < row_dwords) dst[j] = packed;
                }
            }
        } else {
            for (int j = lane; j < row_dwords; j += 64) {
                int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t v = lds32[s0 + t * pitch_dw + j];
                    const int kt = row[2 + t];
                    a0 += __mul24((int)(v & 0xff), kt);
                    a1 += __mul24((int)((v >> 8) & 0xff), kt);
                    a2 += __mul24((int)((v >> 16) & 0xff), kt);
                    a3 += __mul24((int)(v >> 24), kt);
                }
                dst[j] = clip8_x4(a0, a1, a2, a3);
            }
        }
    }
}

// ---- stage A: INTER_AREA + pad + outputs -------------------------------------------------------------------------------
// Fractional INTER_AREA, the common case, from the plan kernel's tables in LDS. Same fp32 operation order as
// area_pixel(); taps that fall on the black canvas add +0.0f in the
// reference order, so clipping the tap ranges to the pasted region is
// exact. One (unaligned) 32-bit LDS read fetches the three channels.
// Table entries as plain scalars (passing the structs by reference made
// hipcc keep them in scratch memory); cv.ry0 .. is the sub-band's window of resized rows.
__device__ __forceinline__ void cf_area_frac(const AreaTabPacked qx, const AreaTabPacked qy, const LdsCanvas cv, int rh, int& o0, int& o1, int& o2) {
    const int x_first = (int)(qx.bits & 0xffff), x_mid = (int)((qx.bits >> 16) & 0xff);
    const int x_hf = (int)((qx.bits >> 24) & 1), x_n = x_hf + x_mid + (int)((qx.bits >> 25) & 1);
    const int y_first = (int)(qy.bits & 0xffff), y_mid = (int)((qy.bits >> 16) & 0xff);
    const int y_hf = (int)((qy.bits >> 24) & 1), y_n = y_hf + y_mid + (int)((qy.bits >> 25) & 1);
#define PA_ALPHA_X(K) ((K) < x_hf ? qx.a_first : ((K) < x_hf + x_mid ? qx.a_mid : qx.a_last))
#define PA_ALPHA_Y(J) ((J) < y_hf ? qy.a_first : ((J) < y_hf + y_mid ? qy.a_mid : qy.a_last))
    int k_lo = cv.px - x_first, k_hi = cv.px + cv.rw - x_first;
    k_lo = k_lo > 0 ? k_lo : 0;
    k_hi = k_hi < x_n ? k_hi : x_n;
    int j_lo = cv.py - y_first, j_hi = cv.py + rh - y_first;
    j_lo = j_lo > 0 ? j_lo : 0;
    j_hi = j_hi < y_n ? j_hi : y_n;
    float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f;
    const int col0 = (x_first + k_lo - cv.px) * 3;
    const int nk = k_hi - k_lo;
    if (nk <= 6) {
        // <= 6 taps x 3 channels = <= 18 bytes per row: six aligned dwords cover them
        // at any alignment; funnel-shifted, every byte sits at a static position
        float al[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) al[k] = k < nk ? PA_ALPHA_X(k_lo + k) : 0.f;
        for (int j = j_lo; j < j_hi; ++j) {
            const float beta = PA_ALPHA_Y(j);
            const int o = cv.base + (y_first + j - cv.py - cv.ry0) * cv.pitch + col0;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(pa_smem + (o & ~3));
            const uint32_t shb = (uint32_t)(o & 3);
            uint32_t w[6], r[5];
#pragma unroll
            for (int q = 0; q < 6; ++q) w[q] = src[q];
#pragma unroll
            for (int q = 0; q < 5; ++q) r[q] = __builtin_amdgcn_alignbyte(w[q + 1], w[q], shb);
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if (k < nk) {
                    const int q0 = 3 * k, q1 = 3 * k + 1, q2 = 3 * k + 2;
                    b0 = b0 + (float)((r[q0 >> 2] >> (8 * (q0 & 3))) & 0xff) * al[k];
                    b1 = b1 + (float)((r[q1 >> 2] >> (8 * (q1 & 3))) & 0xff) * al[k];
                    b2 = b2 + (float)((r[q2 >> 2] >> (8 * (q2 & 3))) & 0xff) * al[k];
                }
            }
            sum0 = sum0 + beta * b0;
            sum1 = sum1 + beta * b1;
            sum2 = sum2 + beta * b2;
        }
    } else {
        for (int j = j_lo; j < j_hi; ++j) {
            const float beta = PA_ALPHA_Y(j);
            int o = cv.base + (y_first + j - cv.py - cv.ry0) * cv.pitch + col0;
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            for (int k = k_lo; k < k_hi; ++k) {
                const float alpha = PA_ALPHA_X(k);
                b0 = b0 + (float)pa_smem[o] * alpha;
                b1 = b1 + (float)pa_smem[o + 1] * alpha;
                b2 = b2 + (float)pa_smem[o + 2] * alpha;
                o += 3;
            }
            sum0 = sum0 + beta * b0;
            sum1 = sum1 + beta * b1;
            sum2 = sum2 + beta * b2;
        }
    }
#undef PA_ALPHA_X
#undef PA_ALPHA_Y
    o0 = cv_saturate_u8(sum0);
    o1 = cv_saturate_u8(sum1);
    o2 = cv_saturate_u8(sum2);
}

// The sub-band's rb output rows from r0 on: INTER_AREA from the canvas in LDS, the black pad below out_h, the outputs
__device__ __forceinline__ void cf_area(const PreprocParams& p, int crop, const CropPlan& pl, const LdsCanvas cv, const AreaTabPacked* tabs, int band0,
                                        int r0, int rb, int tid) {
    const AreaGeom g = area_geom(pl, PA_CROP);
    for (int i = tid; i < rb * PA_CROP; i += CF_NT) {
        const int dy = r0 + (i >> 7), dx = i & 127;
        int o0 = 0, o1 = 0, o2 = 0;
        if (dy < pl.out_h) {
            if (pl.area_mode == 3) cf_area_frac(tabs[dx], tabs[PA_CROP + dy - band0], cv, pl.rh, o0, o1, o2);
            else area_pixel(g, cv, dy, dx, o0, o1, o2);
        }
        write_crop_pixel(p, crop, dy * PA_CROP + dx, o0, o1, o2);
    }
}

// The kernel: the band loop, the barriers and the choice of forms.
__global__ __launch_bounds__(CF_NT, 4) void crop_fused_kernel(const PreprocParams p) {
#ifdef PA_STAMP_BUILD
    const unsigned long long st0 = __builtin_amdgcn_s_memrealtime();
#endif
    // Workgroups are handed to the 8 XCDs round robin in launch order. PreprocParams::crop_xcd: of every 128 consecutive
    // workgroups (8 rows of the grid), the 16 that one XCD gets are the 16 bands of ONE row, so a crop's operand of the
    // horizontal matrix form is fetched into one XCD's L2, not into all eight. The rows behind the last whole group of 8
    // (the fallback row among them) keep the grid's own order.
    int crop = blockIdx.y, band = blockIdx.x;
    if (p.crop_xcd && (int)blockIdx.y < (int)(gridDim.y & ~7u)) {
        const int l = (blockIdx.y & 7) * 16 + blockIdx.x;  // gridDim.x == 16
        crop = (blockIdx.y & ~7) + (l & 7);
        band = l >> 3;
    }
    if (crop == p.n_frames * p.fighters) {  // the grid's extra row: crops whose bands do not fit the LDS budget
        crop_fallback_body(p, band);
        return;
    }
    const int band0 = band * 8;  // first of this workgroup's 8 output rows
    const int tid = threadIdx.x;
    const CropPlan pl = p.plans[crop];
    if (pl.status != PA_CROP_OK) {
        // failed crop: all-zero rows (the fallback kernels skip it as well)
        for (int i = tid; i < 8 * PA_CROP; i += CF_NT) write_crop_pixel(p, crop, band0 * PA_CROP + i, 0, 0, 0);
        return;
    }
    if (!pl.fused_rb) return;
    size_t frame_pitch;
    const uint8_t* slice = slice_ptr(p, crop, pl, &frame_pitch);
    // (the plan arrives through vector loads; the two table addresses are the same in every lane and are used in every
    // stage, so they are moved to scalar registers -- as a lane's pair of vector registers one of them went to scratch)
    const int32_t* coef_h = uniform_ptr(pl.coef_h);
    const int32_t* coef_v = uniform_ptr(pl.coef_v);
    const int rb = pl.fused_rb;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // computeResizeAreaTab entries for the 128 destination columns and this workgroup's 8
    // destination rows, computed once (fp64 with divisions) and kept behind the stage buffers
    AreaTabPacked* tabs = reinterpret_cast<AreaTabPacked*>(pa_smem + p.fused_lds);
    if (pl.area_mode == 3) {
        const AreaTabPacked* at = p.area_tabs + (size_t)crop * 2 * PA_CROP;  // the plan kernel's
        if (tid < PA_CROP) tabs[tid] = at[tid];
        else if (tid < PA_CROP + 8 && band0 + (tid - PA_CROP) < pl.out_h) tabs[tid] = at[PA_CROP + band0 + (tid - PA_CROP)];
    }
    __syncthreads();
    for (int r0 = band0; r0 < band0 + 8; r0 += rb) {
        const BandRows b = band_rows(pl, r0, r0 + rb);
        const BandLds L = band_lds(pl, b);
        const int n0 = b.ty1 - b.ty0;
        const bool mfma_v = L.pt != 0;  // matrix-form vertical pass
        if (pl.mfma_h == 1 && !(p.ablate & 1)) cf_stage_aligned(slice, frame_pitch, (pl.h_mis + pl.sw * 3 + 3) >> 2, b.ty0, n0, L.p0, wave, lane);
        else if (!(p.ablate & 1)) cf_stage_realign(slice, frame_pitch, pl.sw, b.ty0, n0, L.p0, wave, lane);
        if (mfma_v) {  // its coefficient operand starts as zeros
            uint32_t* cz = reinterpret_cast<uint32_t*>(pa_smem + L.offc);
            for (int i = tid; i < 3 * CF_MFMA_N * CF_MFMA_K / 4; i += CF_NT) cz[i] = 0u;
        }
        __syncthreads();
        int in_base = 0, in_pitch = L.p0;
        if (pl.need_h && !(p.ablate & 2)) {
            if (mfma_v) cf_v_operand(coef_v, b, L, tid);
            if (pl.mfma_h && n0 > 0) cf_h_mfma(p.hop + (size_t)crop * PA_HOP_BLOCKS_MAX * PA_HOP_BLOCK_BYTES, pl.rw, L, n0, wave, lane);
            // Vector form of stage H, the one stage left inline, its wide-filter branch with its own copy of the sum:
            // as a stage function (or as per-item functions under this loop, or with bicubic_acc in the wide branch)
            // the object kept 128 VGPRs and no scratch, but the allocation moved everywhere and the crop stage of
            // crops that take the MATRIX forms -- which never run this code -- went from 0.0977 to 0.1038 ms per 64
            // 1080p frames (profiles/crop_shared_parent_ab.md).
            // Work item = (output column, chunk of 4 rows): the column's <= 15 coefficients are
            // fetched once per item and reused for its rows; ~6 items per thread keeps all 512
            // threads busy (one item per column would leave the second pass 3/4 empty).
            const int chunks = (n0 + 3) >> 2;
            const int items = pl.mfma_h ? 0 : chunks * pl.rw;
            for (int it = tid; it < items; it += CF_NT) {
                const int ck = it / pl.rw, xx = it - ck * pl.rw;
                const int32_t* row = coef_h + (size_t)xx * COEF_ROW;
                const int xmin = row[0], cnt = row[1];
                const int y_end = (ck * 4 + 4) < n0 ? (ck * 4 + 4) : n0;
                if (pl.ksize_h <= 7) {
                    // common case (scale <= 1.5): 7 taps fully unrolled; coefficients beyond cnt are
                    // zero, so the extra byte reads (still inside the LDS allocation) add nothing
                    int k[7];
#pragma unroll
                    for (int t = 0; t < 7; ++t) k[t] = t < cnt ? row[2 + t] : 0;
                    // the 7 taps x 3 channels are 21 consecutive bytes starting at byte 3*xmin of the
                    // (4-byte aligned) LDS row: fetch the 6 aligned dwords that cover them (3x
                    // ds_read2_b32 instead of 21 ds_read_u8 -- this stage is LDS-instruction bound),
                    // funnel-shift them into place, then every byte sits at a compile-time position.
                    const int sb = xmin * 3;
                    const uint32_t shb = (uint32_t)(sb & 3);
                    const int a_dw = sb >> 2;
                    // the chunk's 4 rows are independent: all 24 LDS reads are issued before the first
                    // use (the stage is latency-bound at 3 waves per SIMD otherwise). Rows past the end
                    // of the band are clamped for the reads and skipped for the store.
                    uint32_t w[4][6];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int y = ck * 4 + u < n0 ? ck * 4 + u : n0 - 1;
                        const uint32_t* src = reinterpret_cast<const uint32_t*>(pa_smem + y * L.p0) + a_dw;
#pragma unroll
                        for (int q = 0; q < 6; ++q) w[u][q] = src[q];
                    }
                    int tr[3][4];  // transposed B1: the chunk's four rows of each channel become one dword
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        uint32_t r[6];
#pragma unroll
                        for (int q = 0; q < 5; ++q) r[q] = __builtin_amdgcn_alignbyte(w[u][q + 1], w[u][q], shb);
                        r[5] = __builtin_amdgcn_alignbyte(0u, w[u][5], shb);
                        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
#pragma unroll
                        for (int t = 0; t < 7; ++t) {
                            const int j0 = 3 * t, j1 = 3 * t + 1, j2 = 3 * t + 2;
                            a0 += __mul24((int)((r[j0 >> 2] >> (8 * (j0 & 3))) & 0xff), k[t]);
                            a1 += __mul24((int)((r[j1 >> 2] >> (8 * (j1 & 3))) & 0xff), k[t]);
                            a2 += __mul24((int)((r[j2 >> 2] >> (8 * (j2 & 3))) & 0xff), k[t]);
                        }
                        const int y = ck * 4 + u;
                        if (mfma_v) {
                            tr[0][u] = a0, tr[1][u] = a1, tr[2][u] = a2;
                        } else if (y < n0) {
                            const int d = L.off1 + y * L.p1 + xx * 3;
                            pa_smem[d + 0] = (uint8_t)clip8(a0);
                            pa_smem[d + 1] = (uint8_t)clip8(a1);
                            pa_smem[d + 2] = (uint8_t)clip8(a2);
                        }
                    }
                    if (mfma_v) {
                        // rows past the band's end (the clamped repeats) land in the column's padding: pt >= 4 * chunks
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int col = xx * 3 + c;
                            *reinterpret_cast<uint32_t*>(pa_smem + L.off1 + col * L.pt + (col >> 3) * L.skew + ck * 4) = clip8_pk4(tr[c][0], tr[c][1], tr[c][2], tr[c][3]);
                        }
                    }
                } else {
                    for (int y = ck * 4; y < y_end; ++y) {
                        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
                        const int s = y * L.p0 + xmin * 3;
                        for (int t = 0; t < cnt; ++t) {
                            const int kt = row[2 + t];
                            a0 += __mul24((int)pa_smem[s + 3 * t + 0], kt);
                            a1 += __mul24((int)pa_smem[s + 3 * t + 1], kt);
                            a2 += __mul24((int)pa_smem[s + 3 * t + 2], kt);
                        }
                        if (mfma_v) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const int col = xx * 3 + c;
                                pa_smem[L.off1 + col * L.pt + (col >> 3) * L.skew + y] = (uint8_t)clip8(c == 0 ? a0 : (c == 1 ? a1 : a2));
                            }
                        } else {
                            const int d = L.off1 + y * L.p1 + xx * 3;
                            pa_smem[d + 0] = (uint8_t)clip8(a0);
                            pa_smem[d + 1] = (uint8_t)clip8(a1);
                            pa_smem[d + 2] = (uint8_t)clip8(a2);
                        }
                    }
                }
            }
            in_base = L.off1;
            in_pitch = L.p1;
            __syncthreads();
        }
        if (mfma_v || (pl.need_v && !(p.ablate & 4))) {
            if (mfma_v) cf_v_mfma(coef_v, pl.rw, b, L, wave, lane);
            else cf_v_vector(coef_v, pl.rw, pl.ksize_v, b, L, in_base, in_pitch, wave, lane);
            in_base = L.off2;
            in_pitch = L.p1;
            __syncthreads();
        }
#ifdef PA_DEBUG_DUMP
        if (p.dbg && crop == p.dbg_crop && r0 == p.dbg_row) {
            int* meta = reinterpret_cast<int*>(p.dbg);
            if (tid == 0) {
                meta[0] = b.dy0; meta[1] = b.dy1; meta[2] = b.ry0; meta[3] = b.ry1; meta[4] = b.ty0; meta[5] = b.ty1;
                meta[6] = L.p0; meta[7] = L.p1; meta[8] = L.off1; meta[9] = L.off2; meta[10] = L.total; meta[11] = rb;
                meta[12] = pl.sw; meta[13] = pl.sh; meta[14] = pl.rw; meta[15] = pl.rh; meta[16] = pl.px; meta[17] = pl.py;
                meta[18] = pl.need_h; meta[19] = pl.need_v; meta[20] = pl.d; meta[21] = pl.area_mode; meta[22] = pl.sx0; meta[23] = pl.sy0;
            }
            for (int i = tid; i < L.total; i += CF_NT) p.dbg[256 + i] = pa_smem[i];
        }
#endif
        if (!(p.ablate & 8)) {
            LdsCanvas cv;
            cv.base = in_base;
            cv.pitch = in_pitch;
            cv.px = pl.px; cv.py = pl.py; cv.rw = pl.rw;
            cv.ry0 = b.ry0; cv.ry1 = b.ry1;
            cf_area(p, crop, pl, cv, tabs, band0, r0, rb, tid);
        }
        __syncthreads();  // the next sub-band reuses the LDS stages
#ifdef PA_STAMP_BUILD
        if (p.dbg && threadIdx.x == 0 && r0 + rb >= band0 + 8) {
            unsigned long long* o = reinterpret_cast<unsigned long long*>(p.dbg) + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4;
            o[0] = st0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = (unsigned long long)pl.d; o[3] = rb;
        }
#endif
    }
}

// ---------------------------------------------------------------------------
// Log-projection boxes: the reference's current source of
// fighter boxes. Fighter.set_from_json (playaid/fighter.py:494-539) projects four corners
// around the logged world position through a look-at camera (calculate_lookat_matrix :87-121,
// calculate_intrinsic_matrix :66-84, project_point_to_pixel :124-155, all for a hard-coded
// 1280x720 image) and YoloCrop.from_pixel_coordinates (:170-190) turns the rounded pixels
// into a normalised box. One thread per (frame, fighter), fp64 like numpy.
// log row: pos_x, pos_y, cam_x, cam_y, cam_z, tgt_x, tgt_y, tgt_z, fov_degrees.
__global__ void project_boxes_kernel(const double* __restrict__ log, double* __restrict__ boxes, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = log + (size_t)i * 9;
    const double W = 1280.0, H = 720.0;
    // look-at basis
    double fx = r[2] - r[5], fy = r[3] - r[6], fz = r[4] - r[7];
    const double fn = sqrt(fx * fx + fy * fy + fz * fz);
    fx /= fn; fy /= fn; fz /= fn;
    double rx = 1.0 * fz - 0.0 * fy, ry = 0.0 * fx - 0.0 * fz, rz = 0.0 * fy - 1.0 * fx;  // cross(up, forward)
    const double rn = sqrt(rx * rx + ry * ry + rz * rz);
    rx /= rn; ry /= rn; rz /= rn;
    const double ux = fy * rz - fz * ry, uy = fz * rx - fx * rz, uz = fx * ry - fy * rx;  // cross(forward, right)
    const double fov_rad = r[8] * (3.141592653589793 / 180.0);
    const double focal = W / (2.0 * tan(fov_rad / 2.0));
    const double dxs[4] = {-10.0, 10.0, -10.0, 10.0};
    const double dys[4] = {20.0, 20.0, -3.0, -3.0};
    double px[4], py[4];
    for (int c = 0; c < 4; ++c) {
        // inverse of [R | t] with orthonormal rows R = (right, up, -forward): R^T (p - t)
        const double dx = r[0] + dxs[c] - r[2], dy = r[1] + dys[c] - r[3], dz = 0.0 - r[4];
        const double cxm = rx * dx + ux * dy - fx * dz;
        const double cym = ry * dx + uy * dy - fy * dz;
        const double czm = rz * dx + uz * dy - fz * dz;
        const double nx = cxm / czm, ny = cym / czm;
        const double ix = focal * nx + W / 2.0;
        const double iy = H - (focal * ny + H / 2.0);
        px[c] = rint(ix);  // np.round: half to even
        py[c] = rint(iy);
    }
    const double cx = (px[0] + px[1] + px[2] + px[3]) / 4.0, cy = (py[0] + py[1] + py[2] + py[3]) / 4.0;
    const double bw = fmax(fmax(px[0], px[1]), fmax(px[2], px[3])) - fmin(fmin(px[0], px[1]), fmin(px[2], px[3]));
    const double bh = fmax(fmax(py[0], py[1]), fmax(py[2], py[3])) - fmin(fmin(py[0], py[1]), fmin(py[2], py[3]));
    double* o = boxes + (size_t)i * 4;
    o[0] = cx / W;
    o[1] = cy / H;
    o[2] = bw / W;
    o[3] = bh / H;
}

hipError_t launch_project_boxes(const double* log, double* boxes, int32_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(project_boxes_kernel, dim3((n + 127) / 128), dim3(128), 0, s, log, boxes, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The runner's own input branch (playaid/ai_runner.py:446-459): a crop IMAGE of any size -- what
// YOLOv5 --save-crop writes and cv2.imread returns, uint8 [h][w][3] BGR -- becomes the 128 x 128 model
// input by  BGR2RGB -> imutils.resize(width=128) = cv2.resize(INTER_AREA) to (128, int(h * (128 / w)))
// -> ImageOps.pad((128, 128), black) when that is not 128 rows (Pillow: aspect-preserving BICUBIC
// "contain", pasted centred). The order of the two resamplers is the reverse of square_crop's, and the
// INTER_AREA source is not square, so this is its own kernel: one workgroup per image, the three
// passes over L2-resident scratch (t1: INTER_AREA result, t2: after the horizontal bicubic pass, then
// t1's second half: after the vertical pass), coefficient tables in LDS. Same integer / IEEE arithmetic
// as the fused path (shared helpers above), bit-exact against oracle/yolo_crop.runner_input_from_crop.
// The plan (RunnerInPlan, runner_in_plan) and the pixel of the last step (runner_in_pixel) are crop_math.h's.

// What get_action_recognition_input_for_frame does to one crop image (ai_runner.py:446-459), decided once per image: the
// descriptor's bounds here, then the INTER_AREA destination, the branch of cv::resize it takes, ImageOps.pad's contain
// size / paste offset / bicubic passes.
__device__ RunnerInPlan runner_plan(const RunnerInParams& q, int crop, long long& off) {
    off = q.desc[crop].offset;
    const int sh = q.desc[crop].height, sw = q.desc[crop].width;
    if (sh < 1 || sw < 1 || sh > q.max_h || sw > q.max_w || off < 0 || off + (long long)sh * sw * 3 > q.images_bytes) {
        RunnerInPlan bad = {};
        bad.status = PA_CROP_BAD_BOX;
        return bad;
    }
    return runner_in_plan(sw, sh, q.t_stride);
}

// The three steps of a runner input as three launches over (image, part) grids -- INTER_AREA | Pillow's horizontal pass | its
// vertical pass fused with the paste -- instead of one workgroup per image walking all of them between barriers (round 3:
// 128 workgroups on a 256-CU part, 0.39 ms per 128 crop images; the kernel boundaries are the barriers now, and every
// launch has 4 x as many workgroups). Every workgroup works the image's plan out again (a few dozen scalar operations).
// Same arithmetic, same order per output value: bit-identical results.
constexpr int RI_PARTS = 4;
template <int STAGE>
__global__ __launch_bounds__(256) void runner_input_stage_kernel(const RunnerInParams q) {
    __shared__ int32_t coef[PA_CROP][COEF_ROW];  // the pad step's table of this stage's axis: <= 128 output coordinates
    const int crop = blockIdx.x, part = blockIdx.y;
    const int tid = threadIdx.x;
    const int i0 = part * 256 + tid, istep = RI_PARTS * 256;
    PreprocParams out;  // write_crop_pixel() only reads these fields
    out.swap_rb = q.swap_rb;
    out.crops_u8 = q.inputs_u8;
    out.crops_f32 = q.inputs_f32;
    out.crops_f32_is_bf16 = q.inputs_f32_is_bf16;
    long long off;
    const RunnerInPlan pl = runner_plan(q, crop, off);
    const int oh = pl.area.oh;
    if (STAGE == 0 && part == 0 && tid == 0 && q.status) q.status[crop] = pl.status;
    if (pl.status != PA_CROP_OK) {
        if (STAGE == 2)
            for (int i = i0; i < PA_CROP * PA_CROP; i += istep) write_crop_pixel(out, crop, i, 0, 0, 0);
        return;
    }
    uint8_t* A = q.t1 + (size_t)crop * q.t_stride;   // [oh][128][3] behind INTER_AREA
    uint8_t* B = q.t2 + (size_t)crop * q.t_stride;   // [oh][rw][3] behind the horizontal pass
    if (STAGE == 0) {
        WhCanvas cv;
        cv.src = q.images + off;
        cv.pitch = pl.area.sw * 3;
        for (int i = i0; i < oh * PA_CROP; i += istep) {
            const int dy = i >> 7, dx = i & 127;
            int o0, o1, o2;
            area_pixel(pl.area, cv, dy, dx, o0, o1, o2);
            uint8_t* o = A + (size_t)i * 3;
            o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
        }
        return;
    }
    if (STAGE == 1) {  // ImagingResampleHorizontal_8bpc: [oh][128] -> B as [oh][rw]
        if (!pl.need_h) return;
        if (tid < pl.rw) bicubic_coef_row(PA_CROP, pl.rw, tid, coef[tid]);  // (fp64, one output coordinate per thread)
        __syncthreads();
        bicubic_pass_h(coef[0], A, (size_t)PA_CROP * 3, oh, pl.rw, B, i0, istep);
        return;
    }
    // STAGE 2: ImagingResampleVertical_8bpc for the canvas pixels that need it, paste on the black 128 x 128 canvas, channel
    // swap, u8 + model input
    if (pl.need_v) {
        if (tid < pl.rh) bicubic_coef_row(oh, pl.rh, tid, coef[tid]);
        __syncthreads();
    }
    for (int i = i0; i < PA_CROP * PA_CROP; i += istep) {
        int o0, o1, o2;
        runner_in_pixel(pl, pl.need_h ? B : A, coef[0], i, o0, o1, o2);
        write_crop_pixel(out, crop, i, o0, o1, o2);
    }
}

hipError_t launch_runner_inputs(const RunnerInParams& q, hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    const dim3 grid(q.n, RI_PARTS);
    hipLaunchKernelGGL(runner_input_stage_kernel<0>, grid, dim3(256), 0, s, q);
    hipLaunchKernelGGL(runner_input_stage_kernel<1>, grid, dim3(256), 0, s, q);
    hipLaunchKernelGGL(runner_input_stage_kernel<2>, grid, dim3(256), 0, s, q);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Window ingest: the frames stay in (pinned, device-visible) HOST memory and only every crop's source slice
// crosses PCIe. One wave copies one slice row at a time straight out of host memory -- coalesced dword reads
// from the 4-byte-aligned address below the row start, re-aligned with v_alignbyte like stage 0 of the fused
// kernel -- into the packed window buffer (row pitch padded to 16 bytes). A 2-D hipMemcpy per crop was measured
// at ~2 ms each on this stack; this kernel is one launch for all crops and is bound by the link.
__global__ __launch_bounds__(256) void slice_upload_kernel(const uint8_t* __restrict__ frames_host, const CropWindow* __restrict__ desc,
                                                           uint8_t* __restrict__ windows, long long frames_bytes) {
    const int crop = blockIdx.y;
    const CropWindow w = desc[crop];
    const int rows = w.rows;
    const int row_bytes = w.row_bytes;
    if (rows <= 0 || row_bytes <= 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int row_dwords = (row_bytes + 3) >> 2;
    for (int y = wave; y < rows; y += nwaves) {
        const long long so = w.src_offset + (long long)y * w.src_pitch;
        const uintptr_t ga = (uintptr_t)(frames_host + so);
        const uint32_t* g4 = reinterpret_cast<const uint32_t*>(ga & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(ga & 3);
        // bytes of the frame buffer left from the aligned address on: never read past its end. A buffer whose size is not a
        // multiple of 4 ends inside a dword; that dword is gathered byte by byte (it holds the last pixels of the last frame's
        // rows that reach the last column), the bytes behind the end read as 0
        const long long left = frames_bytes - (so - (long long)sh);
        auto ld = [&](int j) -> uint32_t {
            if (4ll * (j + 1) <= left) return g4[j];
            const uint8_t* b = reinterpret_cast<const uint8_t*>(g4 + j);
            uint32_t v = 0;
            for (int k = 0; k < 4 && 4ll * j + k < left; ++k) v |= (uint32_t)b[k] << (8 * k);
            return v;
        };
        uint32_t* dst = reinterpret_cast<uint32_t*>(windows + w.offset + (size_t)y * w.pitch);
        // the link's latency is microseconds: every lane requests up to six dwords (a 1.5 KB row per pass) before the
        // first one is used
        for (int j0 = 0; j0 < row_dwords; j0 += 384) {
            uint32_t lo[6], hi[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int j = j0 + lane + 64 * u;
                lo[u] = j < row_dwords ? ld(j) : 0u;
                hi[u] = (sh && j < row_dwords && 4ll * (j + 1) < (long long)sh + row_bytes) ? ld(j + 1) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int j = j0 + lane + 64 * u;
                if (j < row_dwords) dst[j] = __builtin_amdgcn_alignbyte(hi[u], lo[u], sh);
            }
        }
    }
}

hipError_t launch_slice_upload(const uint8_t* frames_host, long long frames_bytes, const CropWindow* desc, uint8_t* windows, int ncrops,
                               hipStream_t s) {
    if (ncrops <= 0) return hipSuccess;
    hipLaunchKernelGGL(slice_upload_kernel, dim3(32, ncrops), dim3(256), 0, s, frames_host, desc, windows, frames_bytes);
    return hipGetLastError();
}

// YoloCrop.crop_img (fighter.py:316-321) + imutils.resize(width = out_w) (= cv2.resize INTER_AREA to
// (out_w, int(h * (out_w / float(w)))), imutils 0.5.4) for up to four fixed pixel rectangles per frame: the damage
// HUD crops of AIRunner.run_damage_detection (ai_runner.py:556-571, damage_crop_to_percent :114). One workgroup per
// (rectangle, frame), one thread per destination pixel, every INTER_AREA branch of area_pixel (the HUD boxes are
// ENLARGED at 720p / 1080p: OpenCV's bilinear emulation). Channel order is kept (BGR in, BGR out).
__global__ __launch_bounds__(256) void rect_resize_kernel(const RectResizeParams q) {
    const int r = blockIdx.x, f = blockIdx.y;
    const AreaGeom g = area_branch(q.x2[r] - q.x1[r], q.y2[r] - q.y1[r], q.out_w, q.out_h[r]);
    WhCanvas cv;
    cv.pitch = q.width * 3;
    cv.src = q.frames + ((size_t)f * q.height + q.y1[r]) * q.width * 3 + (size_t)q.x1[r] * 3;
    uint8_t* dst = q.out + ((size_t)f * q.n_rects + r) * q.out_h_cap * q.out_w * 3;
    for (int i = threadIdx.x; i < g.oh * g.ow; i += 256) {
        const int dy = i / g.ow, dx = i - dy * g.ow;
        int o0, o1, o2;
        area_pixel(g, cv, dy, dx, o0, o1, o2);
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
    }
}

hipError_t launch_rect_resize(const RectResizeParams& q, int n_frames, hipStream_t s) {
    if (n_frames <= 0 || q.n_rects <= 0) return hipSuccess;
    hipLaunchKernelGGL(rect_resize_kernel, dim3(q.n_rects, n_frames), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t preprocess_init_device() {
    // dynamic LDS beyond the 64 KiB default; the attribute is per device, so pa_create sets it for its own
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&crop_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

hipError_t launch_preprocess(const PreprocParams& p_in, hipStream_t s) {
    PreprocParams p = p_in;
    static const int budget = getenv("PA_FUSED_LDS") ? atoi(getenv("PA_FUSED_LDS")) : PA_FUSED_LDS_BYTES;
    p.fused_lds = budget & ~15;
    static const int ablate = getenv("PA_PRE_ABLATE") ? atoi(getenv("PA_PRE_ABLATE")) : 0;  // timing experiments only
    p.ablate = ablate;
    static const int crop_mfma = getenv("PA_CROP_MFMA") ? atoi(getenv("PA_CROP_MFMA")) : 1;  // 0: the A/B switch of the matrix-core vertical pass
    p.crop_mfma = crop_mfma;
    // 0: the vector horizontal pass and re-aligning staging; 1: the matrix form; 2: the matrix form behind re-aligning staging
    static const int crop_mfma_h = getenv("PA_CROP_MFMA_H") ? atoi(getenv("PA_CROP_MFMA_H")) : PA_CROP_MFMA_H_DEFAULT;
    p.crop_mfma_h = crop_mfma && p.hop ? crop_mfma_h : 0;
    static const int crop_xcd = getenv("PA_CROP_XCD") ? atoi(getenv("PA_CROP_XCD")) : 1;  // 0: a crop's workgroups in launch order
    p.crop_xcd = crop_xcd;
    const int ncrops = p.n_frames * p.fighters;
    if (ncrops <= 0) return hipSuccess;
    hipLaunchKernelGGL(crop_plan_kernel, dim3(ncrops), dim3(256), 0, s, p);
    if (p.crop_mfma_h) hipLaunchKernelGGL(crop_hop_kernel, dim3(PA_HOP_BLOCKS_MAX / PA_HOP_WG_BLOCKS, ncrops), dim3(256), 0, s, p);
#ifdef PA_STAMP_BUILD
    static int calls = 0;
    static unsigned long long* sd = nullptr;
    const char* sf = getenv("PA_CROP_STAMP_FILE");
    const bool now = sf && calls++ == 5;
    if (now) {
        if (!sd) (void)hipMalloc(&sd, (size_t)16 * ncrops * 32);
        (void)hipMemsetAsync(sd, 0, (size_t)16 * ncrops * 32, s);
        p.dbg = reinterpret_cast<uint8_t*>(sd);
    }
#endif
    hipLaunchKernelGGL(crop_fused_kernel, dim3(PA_CROP / 8, ncrops + 1), dim3(CF_NT), p.fused_lds + (PA_CROP + 8) * sizeof(AreaTabPacked), s, p);
    { hipError_t e1 = hipGetLastError(); if (e1 != hipSuccess) return e1; }
#ifdef PA_STAMP_BUILD
    if (now) {
        (void)hipStreamSynchronize(s);
        std::vector<unsigned long long> h((size_t)16 * ncrops * 4);
        (void)hipMemcpy(h.data(), sd, h.size() * 8, hipMemcpyDeviceToHost);
        FILE* f = fopen(sf, "wb");
        if (f) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
        p.dbg = nullptr;
    }
#endif
    return hipGetLastError();
}

size_t coef_cache_ints(int dmax) { return (size_t)dmax * (dmax + 1) / 2 * COEF_ROW; }

hipError_t launch_build_coef_cache(int32_t* cache, int padding, int dmax, hipStream_t s) {
    if (dmax <= 0) return hipSuccess;
    hipLaunchKernelGGL(coef_cache_kernel, dim3((dmax + 255) / 256, dmax), dim3(256), 0, s, cache, padding, dmax);
    return hipGetLastError();
}

}  // namespace pa

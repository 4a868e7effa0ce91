// The detector's synthetic training images, composite_chars_onto_stage (gen_synth_char_detection.py:190-262) from the paste on:
// up to four augmented 128 x 128 sprites over a WHOLE stage picture, pa_scene_composite of include/playaid_hip.h, which states
// the arithmetic; DESIGN.md 5.17. detect_composite.compose_scenes_reference is the numpy twin and the contract: this file and
// the twin give the same bytes.
//
// Two launches:
//   scene_layout_kernel   one workgroup: the records' stage sizes, each rounded up to 16 bytes, summed in order (a block scan
//                         per 256 records) -> desc[i] = {offset, H, W}, or {offset, 0, 0} for a scene that does not fit
//   scene_composite_kernel   (groups_x, n) workgroups of 256 threads. A scene is a COPY with at most four small blends in it,
//                         so it is laid out as one: a stage image starts on a 16-byte boundary in its bank and so does a scene
//                         in the output, both are packed rows, so the 3 W H bytes move as 16-byte pieces -- one aligned
//                         dwordx4 load and one aligned dwordx4 store per thread and piece, consecutive lanes on consecutive
//                         pieces, SCENE_PIECES per thread in flight -- whatever W is. A piece holds 5 1/3 pixels. Whether any
//                         sprite can touch it is decided on its byte range first (two comparisons per sprite against the
//                         sprite's first and last byte in the scene); only a piece inside such a band works out its pixel
//                         coordinates (a multiplication by the row's reciprocal, exact for every byte of a scene), tests the
//                         sprites' columns, and only where a sprite covers one of its pixels walks its six pixels through
//                         pillow_blend, sprite after sprite (scene_blend_piece).
// The last piece of a scene may reach into the padding behind it (on both sides: zeros in the bank); its bytes past the
// picture belong to no image and no blend touches them (their row is H).
//
// Memory safety for ANY parameter bytes: scene_read of scene_math.h clamps the stage and the slots into their banks, n_sprites
// to 0..4 and the offsets to +-PA_SYNTH_PASTE_MAX; a sprite's pixel is addressed only where both of its coordinates are 0..127;
// the pieces of a scene are counted from the (library's own) descriptor and the layout launch keeps every scene inside
// images_capacity. Compiled with -ffp-contract=off.
#include "pa_kernels.h"
#include "scene_math.h"

namespace pa {
namespace {

constexpr int SCENE_THREADS = 256;
constexpr int SCENE_PIECES = 4;   // 16-byte pieces per thread: a workgroup moves 16 KB

struct SceneSprite {
    uint32_t px;         // the slot's first pixel, in dwords from the bank's (an offset, not a pointer: the loads stay global)
    int x, y;            // top-left corner in the picture
    uint32_t lo, hi;     // the first byte of the scene the (clipped) sprite covers, and the one behind its last; lo >= hi: none
};

struct alignas(16) SceneLds {
    uint64_t src, dst;   // the stage's and the scene's first byte, from the bank's and the buffer's
    int W, H, n;
    uint32_t pieces;
    uint64_t inv_row;    // ceil(2^40 / (3 W)): byte / (3 W) == (byte * inv_row) >> 40 for every byte of a scene (< 2^26, 3 W <= 12288)
    SceneSprite sp[PA_SCENE_SPRITES_MAX];
};

__global__ __launch_bounds__(SCENE_THREADS) void scene_layout_kernel(const SceneArgs a) {
    __shared__ unsigned long long scan[SCENE_THREADS];
    __shared__ unsigned long long base;
    const int tid = threadIdx.x;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < a.n; i0 += SCENE_THREADS) {
        const int i = i0 + tid;
        int w = 0, h = 0;
        unsigned long long bytes = 0;
        if (i < a.n) {
            const SynthDesc gd = a.stage_desc[scene_clampi(a.params[i].stage, 0, a.n_stages - 1)];
            w = gd.w;
            h = gd.h;
            bytes = scene_bytes_padded(w, h);
        }
        scan[tid] = bytes;
        __syncthreads();
        for (int d = 1; d < SCENE_THREADS; d <<= 1) {   // inclusive scan
            const unsigned long long v = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const unsigned long long end = base + scan[tid];
        if (i < a.n) {
            const bool fits = end <= (unsigned long long)a.images_capacity;
            pa_crop_image d;
            d.offset = (int64_t)(end - bytes);
            d.height = fits ? h : 0;
            d.width = fits ? w : 0;
            a.desc[i] = d;
        }
        __syncthreads();
        if (tid == SCENE_THREADS - 1) base = end;
        __syncthreads();
    }
}

// The blends of one piece whose first byte is channel `ch` of pixel (x, y). The sixteen bytes are moved up by `ch` bytes inside
// five words, so that pixel k of the piece (six of them, the first and the last possibly in part) has its three bytes at the
// fixed positions 3 k .. 3 k + 2; every pixel is then tested against the sprites once and a covering sprite's dword is loaded
// once for its three channels. Bytes of the five words outside the piece are zero, take part in nothing that is kept, and fall
// off when the words are moved back.
__device__ __forceinline__ void scene_blend_piece(uint4& v, int ch, int x, int y, const SceneLds& L, const uint32_t* __restrict__ slots) {
    const uint32_t in[6] = {0u, v.x, v.y, v.z, v.w, 0u};
    const int up = 8 * ch;
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = (uint32_t)((((uint64_t)in[i + 1] << 32) | (uint64_t)in[i]) >> (32 - up));
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (y < L.H) {
            int c[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = (int)((w[(3 * k + j) >> 2] >> (8 * ((3 * k + j) & 3))) & 0xff);
            bool hit = false;
            for (int s = 0; s < L.n; ++s) {
                const int lx = x - L.sp[s].x, ly = y - L.sp[s].y;
                if ((unsigned)lx < (unsigned)SCENE_SPRITE && (unsigned)ly < (unsigned)SCENE_SPRITE) {
                    const uint32_t q = slots[L.sp[s].px + (uint32_t)(ly * SCENE_SPRITE + lx)];
                    const int al = (int)(q >> 24);
                    c[0] = pillow_blend((int)(q & 0xff), c[0], al);
                    c[1] = pillow_blend((int)((q >> 8) & 0xff), c[1], al);
                    c[2] = pillow_blend((int)((q >> 16) & 0xff), c[2], al);
                    hit = true;
                }
            }
            if (hit) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int sh = 8 * ((3 * k + j) & 3);
                    w[(3 * k + j) >> 2] = (w[(3 * k + j) >> 2] & ~(0xffu << sh)) | ((uint32_t)c[j] << sh);
                }
            }
        }
        if (++x == L.W) {
            x = 0;
            ++y;
        }
    }
    v.x = (uint32_t)((((uint64_t)w[1] << 32) | (uint64_t)w[0]) >> up);
    v.y = (uint32_t)((((uint64_t)w[2] << 32) | (uint64_t)w[1]) >> up);
    v.z = (uint32_t)((((uint64_t)w[3] << 32) | (uint64_t)w[2]) >> up);
    v.w = (uint32_t)((((uint64_t)w[4] << 32) | (uint64_t)w[3]) >> up);
}

__global__ __launch_bounds__(SCENE_THREADS) void scene_composite_kernel(const SceneArgs a) {
    __shared__ SceneLds L;
    const int tid = threadIdx.x;
    const int scene = blockIdx.y;
    if (tid == 0) {
        const pa_crop_image d = a.desc[scene];
        const SceneRead r = scene_read(a.params[scene], a.n_slots, a.n_stages);
        const SynthDesc gd = a.stage_desc[r.stage];
        L.src = gd.offset;
        L.dst = (uint64_t)d.offset;
        L.W = gd.w;
        L.H = gd.h;
        L.n = r.n;
        L.inv_row = (((uint64_t)1 << 40) + (uint64_t)(3 * gd.w) - 1) / (uint64_t)(3 * gd.w);
        // (a scene that did not fit has an empty descriptor: nothing of it is written)
        L.pieces = (d.height == gd.h && d.width == gd.w) ? (uint32_t)(scene_bytes_padded(gd.w, gd.h) >> 4) : 0u;
        for (int k = 0; k < PA_SCENE_SPRITES_MAX; ++k) {
            SceneSprite s;
            s.px = (uint32_t)r.slot[k] * (uint32_t)(SCENE_SPRITE * SCENE_SPRITE);   // (at most 65535 slots of 2^14 dwords)
            s.x = r.x[k];
            s.y = r.y[k];
            const int xa = max(s.x, 0), xb = min(s.x + SCENE_SPRITE, gd.w), ya = max(s.y, 0), yb = min(s.y + SCENE_SPRITE, gd.h);
            if (k < r.n && xa < xb && ya < yb) {
                s.lo = ((uint32_t)ya * (uint32_t)gd.w + (uint32_t)xa) * 3u;
                s.hi = ((uint32_t)(yb - 1) * (uint32_t)gd.w + (uint32_t)xb) * 3u;
            } else {
                s.lo = 1u;
                s.hi = 0u;
            }
            L.sp[k] = s;
        }
    }
    __syncthreads();
    const uint32_t pieces = L.pieces;
    const int W = L.W, n = L.n;
    const uint64_t inv_row = L.inv_row;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.stage_px + L.src);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.images + L.dst);
    const uint32_t* __restrict__ slots = reinterpret_cast<const uint32_t*>(a.sprite_px);
    const uint32_t c0 = (uint32_t)blockIdx.x * (SCENE_THREADS * SCENE_PIECES) + (uint32_t)tid;
    uint4 v[SCENE_PIECES];
#pragma unroll
    for (int u = 0; u < SCENE_PIECES; ++u) {
        const uint32_t c = c0 + (uint32_t)u * SCENE_THREADS;
        if (c < pieces) v[u] = src[c];
    }
#pragma unroll
    for (int u = 0; u < SCENE_PIECES; ++u) {
        const uint32_t c = c0 + (uint32_t)u * SCENE_THREADS;
        if (c >= pieces) continue;
        const uint32_t b0 = c * 16u, b1 = b0 + 16u;
        bool band = false;
        for (int s = 0; s < n; ++s) band = band || (b1 > L.sp[s].lo && b0 < L.sp[s].hi);
        if (band) {
            int y = (int)(((uint64_t)b0 * inv_row) >> 40);
            const uint32_t in_row = b0 - (uint32_t)y * (3u * (uint32_t)W);
            int x = (int)(in_row / 3u);
            const int ch = (int)(in_row - 3u * (uint32_t)x);
            // the piece's pixels: columns x .. x + 5 of row y, unless it runs into the next row
            const bool one_row = x + 5 < W;
            bool covered = false;
            for (int s = 0; s < n; ++s) {
                const int sx = L.sp[s].x, sy = L.sp[s].y;
                covered = covered || !one_row || (y >= sy && y < sy + SCENE_SPRITE && x + 5 >= sx && x < sx + SCENE_SPRITE);
            }
            if (covered) scene_blend_piece(v[u], ch, x, y, L, slots);
        }
        dst[c] = v[u];
    }
}

}  // namespace

hipError_t launch_scene_composite(const SceneArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(scene_layout_kernel, dim3(1), dim3(SCENE_THREADS), 0, s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(scene_composite_kernel, dim3((unsigned)a.groups_x, (unsigned)a.n), dim3(SCENE_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace pa

// The reference's synthetic training frames, load_and_augment_frame_to_stage_crop at synth_difficulty 0
// (ult_action_dataset.py:97-136), composed on the device: pa_synth_composite of include/playaid_hip.h, which states the
// arithmetic; DESIGN.md 5.15. synth_dataset.composite_reference is the numpy twin and the contract: this file and the twin give
// the same bytes.
//
// One launch for n output frames, SYN_BANDS workgroups of 256 threads per frame, no intermediate image in memory:
//   1. thread 0 reads the frame's 32-byte record, clamps it and decides the geometry (sprite size, INTER_AREA branch, paste
//      offset) into LDS; the k / 255 table goes to LDS beside it;
//   2. for the general and the enlarging branch the workgroup builds the two per-axis tables once, in area_pack's 16-byte form
//      (their fp64 is paid ow + oh times, not once per pixel);
//   3. every thread takes four consecutive output pixels: the stage crop's twelve bytes (aligned dword loads), and where the pasted sprite covers the pixel
//      its resampled RGBA value -- gathered from the sprite with one dword load per source pixel, all four channels through
//      the same fp32 sums -- blended in as Pillow does; then three 16-byte stores (one per plane, model layout) or three 4-byte
//      stores (12 packed bytes, uint8 layout). Consecutive lanes write consecutive addresses and read neighbouring sprite
//      columns, so a wave's gather walks whole cache lines of the sprite's rows.
//
// Memory safety for ANY parameter bytes: the sprite and stage numbers are clamped into their banks, the stage origin into
// [0, W - D] x [0, H - D], the paste offsets to +-4096; every sprite and stage coordinate is clamped into its image again where
// the address is formed. The descriptors are the library's own (pa_synth_bank_create). Compiled with -ffp-contract=off.
#include "pa_kernels.h"
#include "synth_math.h"

namespace pa {
namespace {

constexpr int SYN_THREADS = 256;
constexpr int SYN_BANDS = 4;

struct SynFrame {
    const uint32_t* sprite;
    const uint8_t* stage;   // the stage image's first byte
    int stage_w, stage_h;
    int x0, y0;             // stage crop origin
    int ow, oh, px, py;     // resized sprite and where it is pasted
    AreaGeom g;
};

struct alignas(16) SynLds {
    SynFrame f;
    float unit[256];
    AreaTabPacked xt[PA_SYNTH_DIM_MAX], yt[PA_SYNTH_DIM_MAX];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(SYN_THREADS) void synth_composite_kernel(const SynthArgs a) {
    __shared__ SynLds L;
    const int tid = threadIdx.x;
    const int frame = blockIdx.y;
    const int D = a.dim;
    if (tid == 0) {
        const pa_synth_params prm = a.params[frame];
        const SynthDesc sd = a.sprite_desc[clampi(prm.sprite, 0, a.n_sprites - 1)];
        const SynthDesc gd = a.stage_desc[clampi(prm.stage, 0, a.n_stages - 1)];
        SynFrame f;
        f.sprite = reinterpret_cast<const uint32_t*>(a.sprite_px + sd.offset);
        f.stage = a.stage_px + gd.offset;
        f.stage_w = gd.w;
        f.stage_h = gd.h;
        f.x0 = clampi(prm.stage_x, 0, max(gd.w - D, 0));
        f.y0 = clampi(prm.stage_y, 0, max(gd.h - D, 0));
        synth_sprite_size(sd.w, sd.h, D, &f.ow, &f.oh);
        f.px = (D - f.ow) / 2 + clampi(prm.paste_dx, -PA_SYNTH_PASTE_MAX, PA_SYNTH_PASTE_MAX);
        f.py = (D - f.oh) / 2 + clampi(prm.paste_dy, -PA_SYNTH_PASTE_MAX, PA_SYNTH_PASTE_MAX);
        f.g = area_branch(sd.w, sd.h, f.ow, f.oh);
        L.f = f;
    }
    L.unit[tid] = a.unit[tid];
    __syncthreads();
    const SynFrame f = L.f;
    const AreaGeom g = f.g;
    if (g.mode == 3) {
        for (int i = tid; i < g.ow + g.oh; i += SYN_THREADS) {
            if (i < g.ow)
                L.xt[i] = area_pack(area_tab(i, g.scale_x, g.sw));
            else
                L.yt[i - g.ow] = area_pack(area_tab(i - g.ow, g.scale_y, g.sh));
        }
    } else if (g.mode == 4) {
        for (int i = tid; i < g.ow + g.oh; i += SYN_THREADS) {
            if (i < g.ow)
                L.xt[i] = lin_pack(area_lin_x(i, g));
            else
                L.yt[i - g.ow] = lin_pack(area_lin_y(i - g.ow, g));
        }
    }
    __syncthreads();

    const RgbaImage img = {f.sprite, g.sw, g.sh};
    const int P = D * D;
    const int quads = (P + 3) >> 2;
    const int per_band = (quads + SYN_BANDS - 1) / SYN_BANDS;
    const int q_end = min(quads, ((int)blockIdx.x + 1) * per_band);
    for (int quad = (int)blockIdx.x * per_band + tid; quad < q_end; quad += SYN_THREADS) {
        uint8_t px[4][3];
        // the quad's twelve stage bytes, packed
        uint32_t sb[3];
        if ((D & 3) == 0) {
            // the quad lies in one row of the crop: twelve consecutive bytes, at any alignment, out of the (at most four) aligned
            // dwords that hold them. Every one of those dwords holds a byte of the image, and an image starts on a 16-byte
            // boundary and is padded to one, so none leaves the bank. (x0 + 3 < W for a stage at least D wide; clamped anyway.)
            const int p0 = quad * 4;
            const int y = p0 / D, x0 = p0 - y * D;
            const int gy = min(f.y0 + y, f.stage_h - 1), gx = max(min(f.x0 + x0, f.stage_w - 4), 0);
            const int o = (gy * f.stage_w + gx) * 3;
            const uint32_t* w = reinterpret_cast<const uint32_t*>(f.stage + (o & ~3));
            const uint32_t sh = (uint32_t)(o & 3);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = sh ? w[3] : 0u;
            sb[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
            sb[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
            sb[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
        } else {
            uint8_t d[12];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = min(quad * 4 + j, P - 1);
                const int y = p / D, x = p - y * D;
                const int gy = min(f.y0 + y, f.stage_h - 1), gx = min(f.x0 + x, f.stage_w - 1);
                const uint8_t* s = f.stage + ((size_t)gy * f.stage_w + gx) * 3;
                d[3 * j] = s[0]; d[3 * j + 1] = s[1]; d[3 * j + 2] = s[2];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
                sb[k] = (uint32_t)d[4 * k] | ((uint32_t)d[4 * k + 1] << 8) | ((uint32_t)d[4 * k + 2] << 16) | ((uint32_t)d[4 * k + 3] << 24);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = min(quad * 4 + j, P - 1);   // (a last quad past the frame repeats its last pixel and stores none of it)
            const int y = p / D, x = p - y * D;
            int c0 = (int)((sb[(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 0xff);
            int c1 = (int)((sb[(3 * j + 1) >> 2] >> (8 * ((3 * j + 1) & 3))) & 0xff);
            int c2 = (int)((sb[(3 * j + 2) >> 2] >> (8 * ((3 * j + 2) & 3))) & 0xff);
            const int lx = x - f.px, ly = y - f.py;
            if ((unsigned)lx < (unsigned)f.ow && (unsigned)ly < (unsigned)f.oh) {
                uint32_t s;
                if (g.mode == 0)
                    s = img.load(ly, lx);
                else if (g.mode == 1 || g.mode == 2)
                    s = area4_box(img, ly, lx, g.iscale_x, g.iscale_y);
                else if (g.mode == 3)
                    s = area4_general(area_unpack(L.xt[lx]), area_unpack(L.yt[ly]), img);
                else
                    s = area4_linear(lin_unpack(L.xt[lx]), lin_unpack(L.yt[ly]), img);
                const int al = (int)(s >> 24);
                c0 = pillow_blend((int)(s & 0xff), c0, al);
                c1 = pillow_blend((int)((s >> 8) & 0xff), c1, al);
                c2 = pillow_blend((int)((s >> 16) & 0xff), c2, al);
            }
            px[j][0] = (uint8_t)c0; px[j][1] = (uint8_t)c1; px[j][2] = (uint8_t)c2;
        }
        if (a.out_format == PA_SYNTH_MODEL) {   // D == 128 (the host refuses any other): a quad lies in one row, 16-byte aligned
            float* o = reinterpret_cast<float*>(a.out) + (size_t)frame * 3 * P + (size_t)quad * 4;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                *reinterpret_cast<float4*>(o + (size_t)k * P) = make_float4(L.unit[px[0][k]], L.unit[px[1][k]], L.unit[px[2][k]], L.unit[px[3][k]]);
        } else {
            uint8_t* ob = reinterpret_cast<uint8_t*>(a.out) + (size_t)frame * P * 3 + (size_t)quad * 12;
            const uint8_t* b = &px[0][0];
            if ((D & 3) == 0) {   // every frame starts on a 16-byte boundary and holds whole quads
                uint32_t* o = reinterpret_cast<uint32_t*>(ob);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    o[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
            } else {
                const int nb = min(4, P - quad * 4) * 3;
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k < nb) ob[k] = b[k];
            }
        }
    }
}

}  // namespace

hipError_t launch_synth_composite(const SynthArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(synth_composite_kernel, dim3(SYN_BANDS, (unsigned)a.n), dim3(SYN_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace pa

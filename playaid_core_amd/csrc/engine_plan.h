// The ResNet-18 engine's decisions as plain host code: its environment knobs in one table, what follows from them, and which
// kernel form, tile, K split and branch placement one convolution launch takes (pa_api.hip's run_conv launches what plan_conv
// returns). The rows it plans from: engine_table.h. No HIP, no pointers: tests/helpers/engine_plan_table.cpp compiles both headers with
// the host compiler alone.
#pragma once
#include "gemm_tile.h"
#include "wino_shape.h"

#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace pa {

// Crops per launch from which F(4x4, 3x3) taken apart (wino4.hip) replaces the fused F(2x2) kernel on 4 x 4 maps: measured per layer
// in profiles/wino_f4_parent_ab.md. Clips of 40 and of 64 frames (80 and 128 crops) are on the same side of it.
constexpr int WINO_F4_MIN_CROPS = 64;

// One field per knob pa_api.hip obeys, with its default. (The launchers' own knobs stay private to their kernels.)
struct EngineKnobs {
    // -- read once per process: every engine of a process sees the same values --
    int patch = 1;          // PA_PATCH=0: the fp32 stride-1 3x3 layers PA_WINO leaves alone on the im2col engine, not patchconv.hip
    int bf16_patch = 1;     // PA_BF16_PATCH=0: the bf16 stride-1 3x3 layers on igemm_bf16.hip
    int bf16_t256 = 1;      // PA_BF16_T256=0: no 256x128 tile on igemm_bf16.hip
    int s2_pgemm = 2;       // PA_S2_PGEMM: stride-2 3x3 convs without split K on pigemm.hip; 2: 64-row tiles, 1: its own height, 0: igemm.hip
    int stem_igemm = 0;     // PA_STEM_IGEMM (non-zero = on): the fp32 stem on the generic engine
    int stem_pool = 1;      // PA_STEM_POOL=0: stem and max-pool as two kernels
    int pool_overlap = 1;   // PA_POOL_OVERLAP=0: ... without the pool of one half batch under the stem of the other
    int ds_side = 0;        // PA_DS_SIDE=1: a block's 1x1/2 branch GEMM on the side stream, under its opener
    int stem_int = 1;       // PA_STEM_INT=0: no integer stem
    int wino = 1;           // PA_WINO=0: no Winograd form
    int wino_min_hw = 4;    // PA_WINO_MIN_HW: ... for maps at least this wide
    int wino_ds = 1;        // PA_WINO_DS=0: block-0 conv2 of layers 2-4 stays one implicit GEMM with the branch as its second K source
    int wino_f4 = 1;        // PA_WINO_F4=0: the Winograd layers on 4 x 4 maps stay on the fused F(2x2) kernel at every batch
    int wino_f4_min = WINO_F4_MIN_CROPS;  // PA_WINO_F4_MIN: ... below this many crops per launch
    int wino_l3_shape = -1; // PA_WINO_L3_SHAPE=0..3: the launches of the Winograd layers on 8 x 8 maps (layer 3) as this WinoShape (wino_shape.h) at
                            // every batch -- 0 split K, 1 unsplit eight waves, 2 unsplit four waves of 32 channels, 3 unsplit 2 x 2 waves; unset: the rule's own
    int wino_wg = 0;        // PA_WINO_WG=32|64: the launch width (output channels per workgroup) of the Winograd layers that run unsplit on a 64-channel
                            // filter layout (layers 1 and 2; wino_shape.h); unset: the rule's own
    int wino_wg_hw = 0;     // PA_WINO_WG_HW: ... forced only on maps of this width (32: layer 1, 16: layer 2); 0: on every open layer
    int bf16_ds_fuse = 1;   // PA_BF16_DS_FUSE: the bf16 openers carry their block's branch; 0: its own GEMM, 2: own GEMM, the opener's tile as if fused
    int f32_ds_fuse = 1;    // PA_F32_DS_FUSE=0: the exact openers do not carry their block's branch
    // -- read at every pa_create / pa_create_from_arena --
    bool profile_layers = false;  // PA_PROFILE_LAYERS=1: one profile row per conv layer instead of per kernel family
    int force_tile = -1;          // PA_FORCE_TILE=0..4 (scripts/tune_tiles.py); -1: unset
    int force_splitk = 0;         // PA_FORCE_SPLITK, PA_FC_SPLITK, PA_HEAD_SPLITK: at least 1 when set; 0: unset
    int fc_splitk = 0;
    int head_splitk = 0;
    int interleave = 0;           // PA_INTERLEAVE=1: two half batches on two streams
};

inline int env_int(const char* name, int unset) {
    const char* v = getenv(name);
    return v ? atoi(v) : unset;
}
inline int env_min1(const char* name) {
    const char* v = getenv(name);
    return v ? std::max(1, atoi(v)) : 0;
}

// The table as the environment gives it now; its per-process part as the process's first call found it.
inline EngineKnobs engine_knobs() {
    static const EngineKnobs once = [] {
        EngineKnobs k;
        k.patch = env_int("PA_PATCH", k.patch);
        k.bf16_patch = env_int("PA_BF16_PATCH", k.bf16_patch);
        k.bf16_t256 = env_int("PA_BF16_T256", k.bf16_t256);
        k.s2_pgemm = env_int("PA_S2_PGEMM", k.s2_pgemm);
        k.stem_igemm = env_int("PA_STEM_IGEMM", k.stem_igemm);
        k.stem_pool = env_int("PA_STEM_POOL", k.stem_pool);
        k.pool_overlap = env_int("PA_POOL_OVERLAP", k.pool_overlap);
        k.ds_side = env_int("PA_DS_SIDE", k.ds_side);
        k.stem_int = env_int("PA_STEM_INT", k.stem_int);
        k.wino = env_int("PA_WINO", k.wino);
        k.wino_min_hw = env_int("PA_WINO_MIN_HW", k.wino_min_hw);
        k.wino_ds = env_int("PA_WINO_DS", k.wino_ds);
        k.wino_f4 = env_int("PA_WINO_F4", k.wino_f4);
        k.wino_f4_min = env_int("PA_WINO_F4_MIN", k.wino_f4_min);
        k.wino_l3_shape = env_int("PA_WINO_L3_SHAPE", k.wino_l3_shape);
        k.wino_wg = env_int("PA_WINO_WG", k.wino_wg);
        k.wino_wg_hw = env_int("PA_WINO_WG_HW", k.wino_wg_hw);
        k.bf16_ds_fuse = env_int("PA_BF16_DS_FUSE", k.bf16_ds_fuse);
        k.f32_ds_fuse = env_int("PA_F32_DS_FUSE", k.f32_ds_fuse);
        return k;
    }();
    EngineKnobs k = once;
    const char* pl = getenv("PA_PROFILE_LAYERS");
    k.profile_layers = pl && pl[0] == '1';
    k.force_tile = env_int("PA_FORCE_TILE", -1);
    k.force_splitk = env_min1("PA_FORCE_SPLITK");
    k.fc_splitk = env_min1("PA_FC_SPLITK");
    k.head_splitk = env_min1("PA_HEAD_SPLITK");
    k.interleave = env_int("PA_INTERLEAVE", 0);
    return k;
}

enum ComputeDtype { DT_F32, DT_EMULATED_F32, DT_BF16 };   // pa_config::compute_dtype

// What the knobs imply together, for create and run alike
struct EngineForms {
    bool stem_fused;     // stem + max-pool in one kernel (stem_pool.hip); else the two-kernel fp32 forms
    bool stem_int;       // ... on integer pixels: the exact engines, and only the fused kernel has that form
    bool opener_branch;  // the stride-2 openers may carry their block's 1x1/2 branch. fp32: the fused kernel is pigemm.hip's, and a
                         // branch on the side stream is a GEMM of its own (emulated_f32 has no such kernel)
};
inline EngineForms engine_forms(const EngineKnobs& k, ComputeDtype dt) {
    EngineForms f;
    f.stem_fused = k.stem_pool && !k.stem_igemm;
    f.stem_int = dt != DT_BF16 && k.stem_int && f.stem_fused;
    f.opener_branch = dt == DT_BF16 ? k.bf16_ds_fuse != 0 : dt == DT_F32 && k.f32_ds_fuse && !k.ds_side && k.s2_pgemm;
    return f;
}

// Where a block's 1x1/2 downsample branch is computed, decided at create and stated on the conv2 that adds it
// (LayerDesc::branch.place) and on the block's opener (LayerDesc::carries: BRANCH_NONE or one of the two BRANCH_OPENER*)
enum BranchPlace {
    BRANCH_NONE,
    BRANCH_SECOND_K,      // conv2 and the branch are one implicit GEMM, K = 9 cout + cin
    BRANCH_OWN_GEMM,      // a GEMM into the stored branch, which conv2 adds as its residual
    BRANCH_OPENER,        // the opener computes the stored branch on its centre tap
    BRANCH_OPENER_PROBE,  // PA_BF16_DS_FUSE=2: the opener takes the fused launch's tile and K split, the branch stays a GEMM of its own
};
// ... and at one launch
enum BranchLaunch {
    BL_NONE,
    BL_SECOND_K,     // conv2: second K source
    BL_GEMM_BEFORE,  // conv2: the branch GEMM in front of it
    BL_STORED,       // conv2: already stored (by the opener, the GEMM behind it, or the side stream)
    BL_ON_OPENER,    // opener: on its centre tap; fp32: a launch the fused kernel refuses leaves the branch to the GEMM behind it
    BL_GEMM_BEHIND,  // fp32 opener that runs split K (small batches): the branch GEMM behind it
};

struct LayerDesc {
    int cin = 0, cout = 0, kh = 0, kw = 0, stride = 1;  // logical conv
    int in_hw = 0, out_hw = 0;      // spatial size (square) of input / output interior
    int in_pad = 0, out_pad = 0;    // zero-border widths of the buffers
    int off = 0;                    // tap origin inside the padded input
    int taps = 0, kw_taps = 0, chunk = 0;  // igemm K geometry
    int in_px_stride = 0;           // floats per input pixel
    int relu = 1;
    double k_alg = 0;               // algorithmic K (unpadded) for FLOP accounting; with a branch: + its cin
    GemmTile tile = TILE_128x64;    // at the full batch ...
    int splitk = 1;
    bool forced = false;            // ... pinned by PA_FORCE_* / the fc's own choice, else chosen per launch
    bool adds_residual = false;     // adds a residual tensor of its own (not the stored branch)
    bool wino = false;              // has its filters in wino.hip's layout: fp32 stride-1 3x3 layers run as Winograd F(2x2, 3x3)
    bool wino4 = false;             // ... and in wino4.hip's too: a 4 x 4 map runs as F(4x4, 3x3) taken apart from wino_f4_min crops on
    bool split = false;             // emulated_f32: has its weights as three bf16 slices and runs on psgemm.hip
    struct {
        BranchPlace place = BRANCH_NONE;
        int c = 0, hw = 0, stride = 1;  // the block input the branch reads: channels, size, step
        bool split = false;             // emulated_f32: the branch GEMM on psgemm.hip
    } branch;                           // conv2 of block 0 of layers 2-4
    BranchPlace carries = BRANCH_NONE;  // the block's opener
};

inline void choose_tile(int M, int N, int nk, GemmTile* tile, int* splitk) {
    // Aim for >= 2 workgroups per CU (512) so that the un-pipelined K loop of
    // one workgroup hides behind another's; fall back to split-K when even the
    // smallest tile cannot fill the chip.
    *tile = im2col_tile(M, N);
    const int tm = (M + 127) / 128;
    const int tiles = *tile == TILE_128x128 ? tm * (N / 128) : *tile == TILE_128x64 ? tm * (N / 64) : ((M + 63) / 64) * (N / 64);
    int sk = 1;
    while (tiles * sk < 512 && nk / (sk * 2) >= 8) sk *= 2;
    *splitk = sk;
}

// A k x k convolution (k = 7: the stem) of the layer table: geometry, its tile and K split at `max_crops`, PA_FORCE_*
inline LayerDesc conv_desc(const EngineKnobs& k, ComputeDtype dt, int max_crops, int cin, int cout, int ksize, int stride, int in_hw, bool residual) {
    LayerDesc L;
    L.cin = cin; L.cout = cout; L.kh = L.kw = ksize; L.stride = stride;
    L.in_hw = in_hw; L.out_hw = in_hw / stride;
    L.adds_residual = residual;
    if (ksize == 7) {
        L.in_pad = 3; L.out_pad = 1; L.off = 0;
        L.taps = 7; L.kw_taps = 1; L.chunk = 32; L.in_px_stride = 4;
    } else if (ksize == 3) {
        L.in_pad = 1; L.out_pad = 1; L.off = 0;
        L.taps = 9; L.kw_taps = 3; L.chunk = cin; L.in_px_stride = cin;
    } else {
        L.in_pad = 1; L.out_pad = 1; L.off = 1;
        L.taps = 1; L.kw_taps = 1; L.chunk = cin; L.in_px_stride = cin;
    }
    L.k_alg = (double)cin * ksize * ksize;
    choose_tile(max_crops * L.out_hw * L.out_hw, cout, L.taps * L.chunk / ((dt == DT_BF16 && ksize == 3) ? 64 : 32), &L.tile, &L.splitk);
    // tuning knobs (scripts/tune_tiles.py): PA_FORCE_TILE=0|1|2, PA_FORCE_SPLITK=n
    if (k.force_tile >= 0 && k.force_tile <= 4 && !(k.force_tile == 0 && cout % 128 != 0)) { L.tile = (GemmTile)k.force_tile; L.forced = true; }
    if (k.force_splitk) { L.splitk = k.force_splitk; L.forced = true; }
    return L;
}

// fc 512 -> 1000 as a 1x1 row, N padded to n_pad with zero rows (the cached feature rows' width). 32 tiles of 64x64 only: split
// the 16 k-steps four ways (measured 16.9 / 14.5 / 12.3 us for 1 / 2 / 4) unless PA_FC_SPLITK says otherwise
inline LayerDesc fc_desc(const EngineKnobs& k, int n_pad) {
    LayerDesc L;
    L.cin = 512; L.cout = n_pad; L.kh = L.kw = 1;
    L.in_hw = L.out_hw = 1;
    L.taps = 1; L.kw_taps = 1; L.chunk = 512; L.in_px_stride = 512;
    L.relu = 0;
    L.k_alg = 512.0 * 1000.0 / n_pad;
    L.tile = TILE_64x64;
    L.splitk = k.fc_splitk ? k.fc_splitk : 4;
    L.forced = true;
    return L;
}

// Winograd F(2x2, 3x3) for the fp32 stride-1 3x3 layers (wino.hip; measured per layer at 128 crops,
// profiles/r05_resnet_layer_times_wino_options.txt). Layer 4's 4 x 4 maps -- 64 tiles at 128 crops -- were slower there
// than on the direct kernel (117-160 against 84 us) until the kernel learnt to split K. PA_WINO=0: none (A/B);
// PA_WINO_MIN_HW=8: layers 1-3 only (A/B)
inline bool wino_layer(const EngineKnobs& k, ComputeDtype dt, const LayerDesc& L) {
    return dt != DT_BF16 && L.kh == 3 && L.stride == 1 && k.wino && L.out_hw >= k.wino_min_hw && L.out_hw % 4 == 0;
}

// ... of which the 4 x 4 maps (layer 4) also get their filters as 36 GEMM images: F(4x4, 3x3) taken apart (wino4.hip, DESIGN.md
// 5.1d), if the engine's full batch reaches the threshold at all. PA_WINO_F4=0: never (A/B)
inline bool wino4_layer(const EngineKnobs& k, ComputeDtype dt, const LayerDesc& L, int max_crops) {
    return wino_layer(k, dt, L) && k.wino_f4 && L.out_hw == 4 && L.in_hw == 4 && L.cin % 64 == 0 && L.cout % 64 == 0 && max_crops >= k.wino_f4_min;
}

// How the launches of Winograd layer L are shaped in an engine of `max_crops` crops (wino_shape.h): decided at create, from the
// layer's geometry, max_crops and the per-process knobs alone, so that every engine of one shape in a process decides alike
inline WinoLayerShape wino_layer_shape(const EngineKnobs& k, const LayerDesc& L, int max_crops) {
    return wino_layer_shape(k.wino_l3_shape, L.cin, L.cout, L.out_hw, max_crops, wino_bn_force());
}

// ... and their width: the output channels per workgroup of its launches at the full batch (ws.bn unless the layer is open for the
// choice); a launch of fewer crops checks wino_wg_launch_open for itself
inline int wino_layer_wg(const EngineKnobs& k, const LayerDesc& L, int max_crops) {
    return wino_layer_wg(k.wino_wg, k.wino_wg_hw, wino_layer_shape(k, L, max_crops), L.cin, L.cout, L.out_hw, max_crops, wino_ks_force());
}

// Can `opener` compute the branch that `conv2` adds? Same input, same output shape, padding and chunk, tile not pinned;
// `extras`: what the dtype's fused kernel asks beyond that
inline bool opener_can_carry(const LayerDesc& opener, const LayerDesc& conv2, bool same_input, bool extras) {
    return same_input && opener.stride == 2 && opener.cout == conv2.cout && opener.out_hw == conv2.out_hw && opener.out_pad == conv2.out_pad &&
           opener.chunk == conv2.branch.c && !opener.forced && extras;
}

// Placement of the branch of block 0 of layer `li` + 1 (li = 1..3); conv2.wino and conv2.branch.c / hw / stride are set.
// bf16: the branch is always stored (patchconv_bf16.hip has no second source), igemm_bf16.hip's opener form wants whole 64-value
// k-steps. fp32: stored beside the Winograd form of conv2; pigemm.hip's pgemm_branch_kernel takes blocks 2 and 3 only (block 4's
// opener runs split K on igemm.hip, which has no such form), 3x3 with a one-pixel border
inline BranchPlace place_branch(const EngineKnobs& k, ComputeDtype dt, const LayerDesc& opener, const LayerDesc& conv2, bool same_input, int li) {
    if (dt != DT_BF16 && !conv2.wino) return BRANCH_SECOND_K;
    const bool extras = dt == DT_BF16 ? opener.chunk % 64 == 0
                                      : li < 3 && opener.kh == 3 && opener.cin == conv2.branch.c && opener.in_hw == conv2.branch.hw && opener.in_pad == 1;
    if (!engine_forms(k, dt).opener_branch || !opener_can_carry(opener, conv2, same_input, extras)) return BRANCH_OWN_GEMM;
    return dt == DT_BF16 && k.bf16_ds_fuse == 2 ? BRANCH_OPENER_PROBE : BRANCH_OPENER;
}

// The kernel form a launch tries first. The launchers' own refusals stay its fallbacks: bf16 patch -> bf16 im2col, fp32 patch ->
// im2col, persistent GEMM with the branch -> plain persistent GEMM -> im2col
enum ConvForm { CONV_PSGEMM, CONV_BF16_PATCH, CONV_BF16_IM2COL, CONV_WINO, CONV_PATCH, CONV_PGEMM, CONV_IM2COL };

struct LaunchAccount {
    double flops = 0, bytes = 0;
    double flops_executed = 0;  // = flops unless the launch runs an algorithm that executes fewer (Winograd: 4 / 9)
};

// A branch GEMM of its own: block input (hw x hw x c, every stride-th pixel) -> M x N
struct BranchPlan {
    GemmTile tile = TILE_128x64;  // bf16: always (128x128 / 256x128 tiles measured 2-7 us slower here); fp32: choose_tile's, without its K split
    bool psgemm = false;          // emulated_f32 with split weights: psgemm.hip
    LaunchAccount acct;
};
inline BranchPlan plan_branch(bool bf, bool psgemm, int ncrops, int M, int N, int hw, int c, int stride) {
    BranchPlan b;
    b.psgemm = psgemm;
    int sk;
    if (!bf) choose_tile(M, N, c / 32, &b.tile, &sk);
    b.acct.flops = b.acct.flops_executed = 2.0 * M * N * c;
    b.acct.bytes = (bf ? 2.0 : 4.0) * ((double)ncrops * hw * hw * c / (stride * stride) + (double)M * N + (double)N * c);
    return b;
}

// ... the one conv2 adds, from conv2's own row
inline BranchPlan plan_branch(ComputeDtype dt, const LayerDesc& conv2, int ncrops) {
    return plan_branch(dt == DT_BF16, dt == DT_EMULATED_F32 && conv2.branch.split, ncrops, ncrops * conv2.out_hw * conv2.out_hw, conv2.cout,
                       conv2.branch.hw, conv2.branch.c, conv2.branch.stride);
}

struct ConvPlan {
    ConvForm form = CONV_IM2COL;
    int M = 0, N = 0, ktot = 0;   // ktot: with the second K source
    GemmTile tile = TILE_64x64;   // after choose_tile and the bf16 opener override
    int splitk = 1;               // ... and the slab cap
    bool tile_256 = false;        // bf16 im2col (also behind a refusing patch kernel): promote `tile` to 256x128
    int patch_bm = 0;             // CONV_PATCH: rows per tile
    int pgemm_bm = 0;             // CONV_PGEMM: 64, or 0 = the launcher's own choice of tile height
    bool wino_f4 = false;         // CONV_WINO: as F(4x4, 3x3) taken apart -- three launches (wino4.hip) instead of the fused F(2x2) kernel
    BranchLaunch branch = BL_NONE;
    LaunchAccount acct;           // of the main launch, a branch it carries included
    BranchPlan branch_gemm;       // BL_GEMM_BEFORE, BL_GEMM_BEHIND, and fp32 BL_ON_OPENER's fallback
};

// Everything one launch of layer L on `ncrops` crops decides before it calls a launcher. slab_floats: split-K slab left to this
// launch; branch_on_side: the launch context sends an own-GEMM fp32 branch to the side stream (PA_DS_SIDE), so conv2 finds it stored
inline ConvPlan plan_conv(const EngineKnobs& k, ComputeDtype dt, const LayerDesc& L, int ncrops, size_t slab_floats, bool branch_on_side) {
    ConvPlan P;
    const bool bf = dt == DT_BF16 && L.kh == 3;  // bf16 conv path: the 3x3 stack
    const bool emu = dt == DT_EMULATED_F32;
    const BranchPlace place = L.branch.place;
    const bool stored = place == BRANCH_OWN_GEMM || place == BRANCH_OPENER || place == BRANCH_OPENER_PROBE;
    P.M = ncrops * L.out_hw * L.out_hw;
    P.N = L.cout;
    P.ktot = L.taps * L.chunk;
    if (place == BRANCH_OPENER || (stored && !bf && branch_on_side)) {
        P.branch = BL_STORED;
    } else if (stored) {
        P.branch = BL_GEMM_BEFORE;
        P.branch_gemm = plan_branch(dt, L, ncrops);
    } else if (place == BRANCH_SECOND_K) {
        P.branch = BL_SECOND_K;
        P.ktot += L.branch.c;
    }
    const bool second_k = P.branch == BL_SECOND_K, has_residual = L.adds_residual || stored;
    P.tile = L.tile;
    P.splitk = L.splitk;
    if (!L.forced) choose_tile(P.M, P.N, P.ktot / (bf ? 64 : 32), &P.tile, &P.splitk);  // per launch: M depends on the batch
    if ((size_t)P.splitk * P.M * P.N > slab_floats) P.splitk = 1;
    const bool f32_opener = !bf && !emu && L.carries == BRANCH_OPENER;  // the exact path's opener: the fused kernel if it takes the launch
    const bool f32_here = f32_opener && P.splitk <= 1;
    const bool bf_opener = bf && L.carries == BRANCH_OPENER;
    const bool branch_here = bf_opener || f32_here;  // this launch also computes the next conv's 1x1/2 branch
    if (bf && L.carries != BRANCH_NONE) {
        P.tile = (P.N % 128 == 0 && ((P.M + 127) / 128) * (P.N / 128) >= 256) ? TILE_128x128 : TILE_128x64;
        P.splitk = 1;
    }
    // (the branch's FLOPs and bytes are booked where it runs: its own launch, or the opener's)
    const double es = bf ? 2 : 4;
    const double k_main = (stored ? L.k_alg - L.branch.c : L.k_alg) + (branch_here ? L.cin : 0);
    P.acct.flops = P.acct.flops_executed = 2.0 * P.M * P.N * k_main;
    P.acct.bytes = es * ((double)ncrops * L.in_hw * L.in_hw * L.cin + (double)P.M * P.N * ((has_residual || branch_here) ? 2 : 1) + (double)P.N * k_main +
                         (second_k ? (double)ncrops * L.branch.hw * L.branch.hw * L.branch.c : 0.0));
    if (emu && L.split && !second_k && !has_residual) {
        P.form = CONV_PSGEMM;
    } else if (bf) {
        P.form = (k.bf16_patch && L.stride == 1 && !second_k) ? CONV_BF16_PATCH : CONV_BF16_IM2COL;  // im2col: stride-2 convs, second K source
        // a 256-pixel tile halves the weight fill per pixel (this kernel is bound by its L2 -> LDS copies) where it
        // still leaves every CU a workgroup; PA_BF16_T256=0 for A/B runs
        P.tile_256 = k.bf16_t256 && !bf_opener && P.tile == TILE_128x128 && P.splitk == 1 && ((P.M + 255) / 256) * (P.N / 128) >= 256;
    } else if (L.wino && !second_k) {
        P.form = CONV_WINO;
        P.acct.flops_executed = P.acct.flops * 4.0 / 9.0;
        if (L.wino4 && k.wino_f4 && ncrops >= k.wino_f4_min) {   // 36 products per 4 x 4 map where the direct form has 144
            P.wino_f4 = true;
            P.acct.flops_executed = P.acct.flops / 4.0;
        }
    } else if (k.patch && L.kh == 3 && L.stride == 1) {
        // stride-1 3x3 layers without the Winograd form: input patch resident in LDS across the nine taps (patchconv.hip);
        // PA_PATCH=0 keeps the generic im2col engine for A/B runs
        P.form = CONV_PATCH;
        P.patch_bm = P.tile == TILE_64x64 || P.tile == TILE_64x64_K64 ? 64 : 128;
        const int howo = L.out_hw * L.out_hw, in_w2 = L.out_hw + 2;
        const int px128 = howo >= 128 ? (128 / L.out_hw + 2) * in_w2 : (128 / howo) * in_w2 * in_w2;
        if (P.patch_bm == 128 && px128 > 224) P.patch_bm = 64;  // keep two workgroups per CU (2 patch buffers + weight ring <= 80 KB)
    } else if (k.s2_pgemm && L.kh == 3 && L.stride == 2 && !second_k && !has_residual && P.splitk <= 1) {
        // Stride-2 3x3 convolutions that need no split-K run on the persistent form of the engine (pigemm.hip) with 64-row tiles:
        // two tiles per workgroup slot, so the second tile's first operands arrive under the first one's matrix instructions
        // (one 128-row tile per slot, round 4's A/B, gained nothing: 48.39 k against 48.53 k frames/s). At 128 crops: 50.3 / 50.2 /
        // 54.0 -> 48.8 / 46.6 / 52.7 us for the three openers. Same k order as igemm.hip; the bias is the value pgemm's accumulators start
        // from and igemm's last addition: results agree to that rounding. PA_S2_PGEMM=0: igemm.hip (A/B), 1: pgemm's own choice of tile height
        P.form = CONV_PGEMM;
        P.pgemm_bm = k.s2_pgemm == 2 ? 64 : 0;
    }
    if (bf_opener || (f32_here && P.form == CONV_PGEMM)) P.branch = BL_ON_OPENER;
    else if (f32_opener) P.branch = BL_GEMM_BEHIND;   // split K (small batches): where the branch runs without PA_F32_DS_FUSE
    if (f32_opener) P.branch_gemm = plan_branch(false, false, ncrops, P.M, P.N, L.in_hw, L.cin, L.stride);
    return P;
}

}  // namespace pa

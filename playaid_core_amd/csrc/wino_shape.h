// How a launch of the Winograd F(2x2, 3x3) kernel (wino.hip) is shaped, as plain host code: the output channels per workgroup of a
// layer's filter layout, and -- for the engine's few-tile layers -- whether the launch splits K or runs unsplit, and on which
// workgroup. No HIP, no pointers: tests/helpers/wino_shape_table.cpp compiles this header (through engine_plan.h) with the host
// compiler alone.
#pragma once
#include <cstdlib>

namespace pa {

// PA_WINO_BN=32|64 forces the channels per workgroup (A/B); 0: unset. Read once per process.
inline int wino_bn_force() {
    static const int force = getenv("PA_WINO_BN") ? atoi(getenv("PA_WINO_BN")) : 0;
    return force;
}

// The K split the launcher reaches on `wg64` 64-channel workgroups when the caller hands it split-K scratch (cin = the layer's input
// channels; 0: no scratch): the largest power of two that leaves eight chunks per split and the grid within 256 workgroups
inline int wino_split64(long long wg64, int cin) {
    int k = 1;
    if (cin > 0)
        for (int k2 = 2; k2 <= 8 && (cin / 8) % k2 == 0 && (cin / 8) / k2 >= 8 && wg64 * k2 <= 256; k2 *= 2) k = k2;
    return k;
}

// Output channels per workgroup (= per stage image of the filter layout) for a layer of `cout` channels and `n_sb` 4x4-pixel
// sub-blocks per launch: 64 (eight waves: 4 tile groups x 2 channel groups) where that fills the chip; 32 -- four waves, two
// workgroups per CU -- where 64-channel workgroups would leave CUs idle (ResNet-18's layer 3 at 128 crops: 128 workgroups of 64
// channels take 81 us, 256 of 32 channels 65; the detector's 12 x 20 map at 64 frames has 240 and keeps 64: 83 against 121 us)
// and for layers of 32 channels.
inline int wino_pick_bn_rule(int cout, long long n_sb, int cin_split, int force) {
    if (cout % 64) return 32;
    if (force == 32 || force == 64) return force;
    long long wg64 = ((n_sb + 15) / 16) * (cout / 64);
    // a caller with split-K scratch: 64-channel workgroups x 4 beat 32-channel ones x 4 on ResNet-18's layers 3 / 4 (52-54 against
    // 55 us, 56 against 61 us at 128 crops)
    wg64 *= wino_split64(wg64, cin_split);
    return wg64 < 192 ? 32 : 64;
}

// The shape of one engine layer's launches, decided at create and obeyed at every launch (a split sum and an unsplit sum are
// different fp32 sums: every engine of one geometry and max_crops must decide alike, whichever lane or stream it serves).
enum WinoShape {
    WINO_SHAPE_SPLIT = 0,       // the launcher gets the split-K scratch and splits where the tiles leave CUs empty; channels per
                                // workgroup by wino_pick_bn_rule. A layer with tiles enough runs unsplit under this value too.
    WINO_SHAPE_UNSPLIT8 = 1,    // no scratch: eight waves, 16 sub-blocks x 64 channels
    WINO_SHAPE_UNSPLIT4 = 2,    // no scratch: four waves, 16 sub-blocks x 32 channels, two workgroups per CU
    WINO_SHAPE_TG2 = 3,         // no scratch: four waves as 2 tile groups x 2 channel groups, 8 sub-blocks x 64 channels
    WINO_SHAPE_COUNT
};
struct WinoLayerShape {
    WinoShape shape;
    int bn;   // channels per workgroup the layer's filters are laid out for
};

// Which layers the choice is open for: 8 x 8 maps of whole 64-channel groups -- ResNet-18's layer 3, the one family of this
// engine that the fused kernel still runs with a K split at the headline batch (layers 1 and 2 have tiles enough; layer 4's 4 x 4
// maps have F(4x4, 3x3) taken apart from 64 crops on and keep the split below).
inline bool wino_shape_open(int cout, int out_hw) { return out_hw == 8 && cout % 64 == 0; }

// Workgroups one launch over n_sb sub-blocks has on a shape's own tile (before any K split)
inline long long wino_shape_workgroups(WinoShape s, long long n_sb, int cout) {
    switch (s) {
        case WINO_SHAPE_UNSPLIT4: return ((n_sb + 15) / 16) * (cout / 32);
        case WINO_SHAPE_TG2: return ((n_sb + 7) / 8) * (cout / 64);
        default: return ((n_sb + 15) / 16) * (cout / 64);
    }
}

// Unset knob: the form measured best for the headline's two lanes (profiles/wino_l3_shapes_parent_ab.md) -- four-wave workgroups
// of 32 channels over the full K, two to a CU: 256 of them hold 128 CUs for 60 us where the two-way split holds all 256 for 53, and
// the other lane's kernels run on what is left (+3.6 % on two lanes, -2.1 % on one). Taken exactly where that was measured: where
// the split would fill the whole chip (WINO_SHAPE_MIN_WG workgroups) and this shape has as many workgroups of its own -- layer 3 at
// 125-128 crops. Engines of fewer crops keep the split (at 64, 80 and 96 crops, where this shape has 128-192 workgroups, the split
// measured 1.5 / 2.5 / 0.6 % faster on two lanes); engines of more have too many tiles for a split and keep what wino_pick_bn_rule gives them.
constexpr WinoShape WINO_SHAPE_DEFAULT = WINO_SHAPE_UNSPLIT4;
constexpr long long WINO_SHAPE_MIN_WG = 256;
inline bool wino_shape_default_applies(int cin, int cout, long long n_sb) {
    const long long wg64 = wino_shape_workgroups(WINO_SHAPE_UNSPLIT8, n_sb, cout);
    const int k = wino_split64(wg64, cin);
    return k > 1 && wg64 * k >= WINO_SHAPE_MIN_WG && wino_shape_workgroups(WINO_SHAPE_DEFAULT, n_sb, cout) >= WINO_SHAPE_MIN_WG;
}

// knob: PA_WINO_L3_SHAPE (0..3 = a WinoShape for every open layer at every max_crops; anything else = unset)
inline WinoLayerShape wino_layer_shape(int knob, int cin, int cout, int out_hw, int max_crops, int bn_force) {
    const long long n_sb = (long long)max_crops * (out_hw / 4) * (out_hw / 4);
    WinoShape s = WINO_SHAPE_SPLIT;
    if (wino_shape_open(cout, out_hw)) {
        if (knob >= 0 && knob < WINO_SHAPE_COUNT) s = (WinoShape)knob;
        else if (wino_shape_default_applies(cin, cout, n_sb)) s = WINO_SHAPE_DEFAULT;
    }
    switch (s) {
        case WINO_SHAPE_UNSPLIT8: return {s, 64};
        case WINO_SHAPE_UNSPLIT4: return {s, 32};
        case WINO_SHAPE_TG2: return {s, 64};
        default: return {WINO_SHAPE_SPLIT, wino_pick_bn_rule(cout, n_sb, cin, bn_force)};
    }
}

// ---- the launch width of the many-tile layers -----------------------------------------------------------------------------------
// A layer on the 64-channel filter layout that runs unsplit (tiles enough) has two workgroups to choose from: eight waves over 16
// sub-blocks x 64 channels (104 KB of LDS: one to a CU, nothing of another stream beside it), or four waves over 16 sub-blocks x 32
// channels, two to a CU at 72 KB each, reading the same layout (wino.hip's WIDE kernel). Per lane both execute the same instructions
// on the same values: the choice never changes a bit of the result, only who else fits on the CU meanwhile.

// PA_WINO_KS as the launcher reads it (0: unset; 1: it never splits K). Read once per process.
inline int wino_ks_force() {
    static const int force = getenv("PA_WINO_KS") ? atoi(getenv("PA_WINO_KS")) : 0;
    return force;
}

// Can a launch over n_sb sub-blocks run on width 32 beside a 64-channel layout? Only where the launcher, handed the split-K scratch,
// would not split (the width takes no scratch, and a split sum is another fp32 sum): the layer's 64-channel tiles times every
// split its K allows exceed the chip, or PA_WINO_KS=1.
inline bool wino_wg_launch_open(int cin, int cout, long long n_sb, int ks_force) {
    if (cout % 64) return false;
    return ks_force == 1 || wino_split64(wino_shape_workgroups(WINO_SHAPE_UNSPLIT8, n_sb, cout), cin) == 1;
}

// Which layers the width is open for: stride-1 3x3 layers under WINO_SHAPE_SPLIT (the launcher's own rule) on a 64-channel layout
// that run unsplit at the engine's full batch, on maps of at least 16 x 16 -- ResNet-18's layers 1 and 2. The 8 x 8 maps have
// PA_WINO_L3_SHAPE; the 4 x 4 maps split, or run as F(4x4) taken apart.
inline bool wino_wg_open(WinoLayerShape ws, int cin, int cout, int out_hw, long long n_sb, int ks_force) {
    return ws.shape == WINO_SHAPE_SPLIT && ws.bn == 64 && out_hw >= 16 && wino_wg_launch_open(cin, cout, n_sb, ks_force);
}

// Unset knob: width 32 exactly where it was measured to win on two lanes by the project's bar (profiles/wino_wg_width_parent_ab.md),
// 64 elsewhere:
//   * engines of 96 to 128 crops, where layers 1 and 2 are both open: measured at both ends, +1.9 % at 96 crops and +1.4 % at 128
//     (layer 2 alone +1.3 % at 128; layer 1 alone stayed under the bar at both, +0.7 % and +1.1 %, and is taken with layer 2, the
//     pair being the best median of the three);
//   * a layer whose eight-wave workgroups are exactly one per CU (WINO_WG_ONE_PER_CU of them): layer 1 at 64 crops, +2.6 %.
// Layer 1 at 80 crops measured +0.7 %, under the bar, and keeps 64; engines above 128 crops were not measured and keep 64.
constexpr long long WINO_WG_ONE_PER_CU = 256;
constexpr int WINO_WG_CROPS_LO = 96, WINO_WG_CROPS_HI = 128;
inline int wino_wg_default(int cout, int out_hw, long long n_sb) {
    const long long crops = n_sb / ((out_hw / 4) * (out_hw / 4));
    if (wino_shape_workgroups(WINO_SHAPE_UNSPLIT8, n_sb, cout) == WINO_WG_ONE_PER_CU) return 32;
    return crops >= WINO_WG_CROPS_LO && crops <= WINO_WG_CROPS_HI ? 32 : 64;
}

// knobs: PA_WINO_WG (32 | 64 = that width for every open layer at every max_crops; anything else = unset) and PA_WINO_WG_HW (a map
// width: the knob forces only the open layers on maps of that width -- 32 = layer 1, 16 = layer 2 -- the others keep the rule; 0 = all)
inline int wino_layer_wg(int knob, int knob_hw, WinoLayerShape ws, int cin, int cout, int out_hw, int max_crops, int ks_force) {
    const long long n_sb = (long long)max_crops * (out_hw / 4) * (out_hw / 4);
    if (!wino_wg_open(ws, cin, cout, out_hw, n_sb, ks_force)) return ws.bn;
    if ((knob == 32 || knob == 64) && (knob_hw == 0 || knob_hw == out_hw)) return knob;
    return wino_wg_default(cout, out_hw, n_sb);
}

// The width of ONE launch of `ncrops` crops of a layer whose width at the full batch is layer_wg on a layout of bn channels: a launch
// of few crops that the launcher could split keeps the eight-wave workgroups and its split, as before the width existed
inline int wino_launch_wg(int layer_wg, int bn, int cin, int cout, int out_hw, int ncrops, int ks_force) {
    const long long n_sb = (long long)ncrops * (out_hw / 4) * (out_hw / 4);
    return layer_wg == 32 && bn == 64 && wino_wg_launch_open(cin, cout, n_sb, ks_force) ? 32 : bn;
}

}  // namespace pa

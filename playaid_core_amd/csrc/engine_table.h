// The ResNet-18 engine's layer table, once: the seventeen conv rows + fc that plan_conv (engine_plan.h) plans from, with every
// decision pa_create makes about a row, and what follows from the rows alone -- the weight blob's float count and the split-K slab.
// pa_api.hip wires buffers and weights onto these rows; tests/helpers/engine_plan_table.cpp prints them. Same rule as
// engine_plan.h: no HIP, no pointers, the host compiler alone.
#pragma once
#include "engine_plan.h"

#include <string>
#include <vector>

namespace pa {

constexpr int FEATURE_STRIDE = 1024;  // the fc's 1000 outputs padded to the cached feature rows' width (PA_FEATURE_STRIDE)

// What follows a row's own conv + BatchNorm in the weight blob
enum RowKind {
    ROW_CONV,     // nothing
    ROW_CONV2_DS, // block-0 conv2 of layers 2-4: the block's 1x1/2 downsample conv + BatchNorm (LayerDesc::branch)
    ROW_FC,       // the fc row: weight [1000][512] and bias, no BatchNorm
};

struct TableRow {
    std::string name;
    LayerDesc d;
    int carries_of = -1;  // the block's opener (LayerDesc::carries): index of the conv2 whose branch it carries
    RowKind kind = ROW_CONV;
    int layer = 0, block = 0, conv = 0;  // layer<layer>.<block>.conv<conv>; 0, 0, 0: the stem and the fc
};

// Rows 0..16: stem, then conv1, conv2 of the two blocks of layers 1-4; row 17: fc
inline std::vector<TableRow> engine_table(const EngineKnobs& K, ComputeDtype dt, int max_crops) {
    std::vector<TableRow> rows;
    auto add = [&](int layer, int block, int conv, int cin, int cout, int k, int stride, int in_hw, bool residual) -> LayerDesc& {
        TableRow r;
        r.name = layer ? "layer" + std::to_string(layer) + "." + std::to_string(block) + ".conv" + std::to_string(conv) : "conv1";
        r.layer = layer; r.block = block; r.conv = conv;
        r.d = conv_desc(K, dt, max_crops, cin, cout, k, stride, in_hw, residual);
        rows.push_back(r);
        return rows.back().d;
    };
    // the forms of a row that is one plain conv: Winograd filters (F(2x2), and F(4x4) beside them), or, on emulated_f32, the
    // stride-2 3x3 openers of layers 2-4 on psgemm.hip (the stride-1 3x3 layers keep their exact Winograd kernel: per layer the
    // two measure the same, profiles/r06_pgemm_split_layers.txt)
    auto plain = [&](LayerDesc& L) {
        L.wino = wino_layer(K, dt, L);
        L.wino4 = wino4_layer(K, dt, L, max_crops);
        L.split = dt == DT_EMULATED_F32 && L.kh == 3 && L.stride == 2 && L.cin % 32 == 0;
    };
    plain(add(0, 0, 0, 3, 64, 7, 2, 128, false));
    const int widths[4] = {64, 128, 256, 512}, hw_in[4] = {32, 32, 16, 8};
    int cin = 64;
    for (int li = 0; li < 4; ++li) {
        const int co = widths[li], stride = li == 0 ? 1 : 2, hw_out = hw_in[li] / stride;
        plain(add(li + 1, 0, 1, cin, co, 3, stride, hw_in[li], false));
        if (li == 0) {
            plain(add(1, 0, 2, co, co, 3, 1, hw_out, /*residual=*/true));  // adds the block input
        } else {
            // conv2 and the 1x1/2 downsample of the block input are ONE implicit GEMM:
            //   out = relu( [W2' | Wd'] . [im2col3x3(mid) ; x(2y,2x)] + (b2' + bd') )
            // (K = 9*co + cin): no separate downsample launch, no residual tensor. fp32 with PA_WINO_DS: the 3x3 alone on wino.hip,
            // the branch stored by a GEMM of its own or by the block's opener, and added as the residual
            LayerDesc& L = add(li + 1, 0, 2, co, co, 3, 1, hw_out, false);
            rows.back().kind = ROW_CONV2_DS;
            L.branch.c = cin;
            L.branch.hw = hw_in[li];
            L.branch.stride = stride;
            if (K.wino_ds && wino_layer(K, dt, L)) {
                L.wino = true;
                L.wino4 = wino4_layer(K, dt, L, max_crops);
                L.branch.split = dt == DT_EMULATED_F32;
            }
            // Where the branch is computed. same_input: the opener (the row before) and the branch both read the previous block's
            // output -- that is how this loop wires a block 0, so it is true by construction. bf16, PA_BF16_DS_FUSE=0: its own GEMM,
            // for A/B runs. The exact path: the block's stride-2 opener computes it on its centre tap (pigemm.hip's
            // pgemm_branch_kernel) and this row adds the stored branch without a launch (headline +1.7 %,
            // profiles/opener_branch_parent_ab.md; results are bit-identical either way). PA_F32_DS_FUSE=0: the branch as its own
            // GEMM (A/B); PA_DS_SIDE=1 and PA_S2_PGEMM=0 keep the separate GEMM too
            const int at = (int)rows.size() - 1;
            TableRow& opener = rows[at - 1];
            L.branch.place = place_branch(K, dt, opener.d, L, /*same_input=*/true, li);
            if (L.branch.place == BRANCH_OPENER || L.branch.place == BRANCH_OPENER_PROBE) {
                opener.d.carries = L.branch.place;
                opener.carries_of = at;
            }
            L.k_alg += cin;
        }
        plain(add(li + 1, 1, 1, co, co, 3, 1, hw_out, false));
        plain(add(li + 1, 1, 2, co, co, 3, 1, hw_out, /*residual=*/true));  // adds block 0's output
        cin = co;
    }
    TableRow fc;
    fc.name = "fc";
    fc.kind = ROW_FC;
    fc.d = fc_desc(K, FEATURE_STRIDE);
    rows.push_back(fc);
    return rows;
}

// Floats of the weight blob behind its header: per conv row OIHW weights + BatchNorm's gamma, beta, mean, var; the fc; the temporal
// head's Conv1d(1000 -> 512, k = S) and its two classifier layers (512 -> 128 -> A). The same for every knob, dtype and batch.
inline size_t blob_floats(const std::vector<TableRow>& rows, int S, int A) {
    size_t n = 0;
    for (const TableRow& r : rows) {
        if (r.kind == ROW_FC) { n += (size_t)1000 * 512 + 1000; continue; }
        n += (size_t)r.d.cout * r.d.cin * r.d.kh * r.d.kw + 4 * (size_t)r.d.cout;
        if (r.kind == ROW_CONV2_DS) n += (size_t)r.d.cout * r.d.branch.c + 4 * (size_t)r.d.cout;
    }
    n += (size_t)512 * 1000 * S + 512;
    n += 128 * 512 + 128;
    n += (size_t)A * 128 + A;
    return n;
}

// The temporal head's GEMM ([crops][S * 1024] x [S * 1024][512]) at the full batch: 16 tiles x 224 k-steps at S = 7, where 16 splits
// of 14 steps beat 32 of 7 (26.2 vs 28.6 us incl. the reduce)
inline void head_plan(const EngineKnobs& K, int max_crops, int S, GemmTile* tile, int* splitk) {
    choose_tile(max_crops, 512, S * 32, tile, splitk);
    if (*splitk > 16) *splitk = 16;
    if (K.head_splitk) *splitk = K.head_splitk;
}

// Floats of the split-K slab: the largest splitk * M * N over the rows at the full batch (the fc row: M = max_crops, N = its padded
// width), the temporal head's, and the Winograd kernel's split-K scratch (wino.hip): at most one launch's worth of partial output
// tiles -- a grid of 256 eight-wave (512 four-wave) workgroups x 32 floats per thread. One region per interleaved half batch.
inline size_t slab_floats(const std::vector<TableRow>& rows, const EngineKnobs& K, int max_crops, int S) {
    size_t need = 0;
    bool any_wino = false;
    for (const TableRow& r : rows) {
        if (r.d.splitk > 1) need = std::max(need, (size_t)r.d.splitk * max_crops * r.d.out_hw * r.d.out_hw * r.d.cout);
        any_wino = any_wino || r.d.wino;
    }
    GemmTile head_tile;
    int head_splitk;
    head_plan(K, max_crops, S, &head_tile, &head_splitk);
    if (head_splitk > 1) need = std::max(need, (size_t)head_splitk * max_crops * 512);
    if (any_wino) need = std::max(need, (size_t)256 * 512 * 32);
    return need * 2;
}

}  // namespace pa

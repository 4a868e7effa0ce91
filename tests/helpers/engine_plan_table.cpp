// Stand-alone table program of tests/test_engine_plan.py: what the ResNet-18 engine plans for every layer (csrc/engine_plan.h),
// without a GPU. Arguments: NAME=value sets a knob in this process's environment (read by the library's own engine_knobs());
// dtype:max_crops:crops (dtype = f32 | emulated_f32 | bf16) prints one "forms" line and one "plan" line per layer of the
// seventeen-conv table + fc, built the way pa_api.hip's create_impl builds it.
#include "../../playaid_core_amd/csrc/engine_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace pa;

namespace {

struct Row {
    std::string name;
    LayerDesc d;
};

std::vector<Row> layer_table(const EngineKnobs& K, ComputeDtype dt, int NC) {
    std::vector<Row> rows;
    // add_conv: a block-0 conv2 of layers 2-4 (keep) gets its forms from the block code below
    auto add = [&](const std::string& name, int cin, int cout, int k, int stride, int in_hw, bool residual, bool keep = false) {
        LayerDesc L = conv_desc(K, dt, NC, cin, cout, k, stride, in_hw, residual);
        if (!keep) {
            L.wino = wino_layer(K, dt, L);
            L.split = dt == DT_EMULATED_F32 && k == 3 && stride == 2 && cin % 32 == 0;
        }
        rows.push_back({name, L});
    };
    add("conv1", 3, 64, 7, 2, 128, false);
    const int widths[4] = {64, 128, 256, 512}, hw_in[4] = {32, 32, 16, 8};
    int cin = 64;
    for (int li = 0; li < 4; ++li) {
        const int co = widths[li], stride = li == 0 ? 1 : 2, hw_out = hw_in[li] / stride;
        const std::string pre = "layer" + std::to_string(li + 1);
        add(pre + ".0.conv1", cin, co, 3, stride, hw_in[li], false);
        if (li == 0) {
            add(pre + ".0.conv2", co, co, 3, 1, hw_out, true);
        } else {
            add(pre + ".0.conv2", co, co, 3, 1, hw_out, false, /*keep=*/true);
            LayerDesc& L = rows.back().d;
            LayerDesc& C1 = rows[rows.size() - 2].d;
            L.branch.c = cin;
            L.branch.hw = hw_in[li];
            L.branch.stride = stride;
            if (dt != DT_BF16 && K.wino_ds && wino_layer(K, dt, L)) {
                L.wino = true;
                L.branch.split = dt == DT_EMULATED_F32;
            }
            L.branch.place = place_branch(K, dt, C1, L, /*same_input=*/true, li);
            if (L.branch.place == BRANCH_OPENER || L.branch.place == BRANCH_OPENER_PROBE) C1.carries = L.branch.place;
            L.k_alg += cin;
        }
        add(pre + ".1.conv1", co, co, 3, 1, hw_out, false);
        add(pre + ".1.conv2", co, co, 3, 1, hw_out, true);
        cin = co;
    }
    rows.push_back({"fc", fc_desc(K, 1024)});
    return rows;
}

// create_impl's split-K slab: the largest splitk * M * N of the table at the full batch, the Winograd kernel's scratch, one region
// per interleaved half batch (the temporal head's own need can only raise it)
size_t slab_floats(const std::vector<Row>& rows, int NC) {
    size_t need = 0;
    bool any_wino = false;
    for (const Row& r : rows) {
        if (r.d.splitk > 1) need = std::max(need, (size_t)r.d.splitk * NC * r.d.out_hw * r.d.out_hw * r.d.cout);
        any_wino = any_wino || r.d.wino;
    }
    if (any_wino) need = std::max(need, (size_t)256 * 512 * 32);
    return need * 2;
}

const char* const FORM[] = {"psgemm", "bf16_patch", "bf16_im2col", "wino", "patch", "pgemm", "im2col"};
const char* const TILE[] = {"128x128", "128x64", "64x64", "128x64_k64", "64x64_k64", "256x128"};
const char* const PLACE[] = {"none", "second_k", "own_gemm", "opener", "opener_probe"};
const char* const LAUNCH[] = {"none", "second_k", "gemm_before", "stored", "on_opener", "gemm_behind"};

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (strchr(argv[i], '=')) putenv(argv[i]);
    const EngineKnobs K = engine_knobs();
    for (int i = 1; i < argc; ++i) {
        if (strchr(argv[i], '=')) continue;
        char name[32];
        int NC = 0, n = 0;
        if (sscanf(argv[i], "%31[^:]:%d:%d", name, &NC, &n) != 3 || NC < 1 || n < 1 || n > NC) return 2;
        const ComputeDtype dt = !strcmp(name, "bf16") ? DT_BF16 : !strcmp(name, "emulated_f32") ? DT_EMULATED_F32 : DT_F32;
        if (dt == DT_F32 && strcmp(name, "f32")) return 2;
        const EngineForms F = engine_forms(K, dt);
        printf("forms dtype=%s stem_fused=%d stem_int=%d opener_branch=%d\n", name, F.stem_fused, F.stem_int, F.opener_branch);
        const std::vector<Row> rows = layer_table(K, dt, NC);
        const size_t slab = slab_floats(rows, NC);
        for (const Row& r : rows) {
            const ConvPlan P = plan_conv(K, dt, r.d, n, slab, /*branch_on_side=*/false);
            printf("plan dtype=%s max_crops=%d crops=%d layer=%s form=%s tile=%s splitk=%d tile_256=%d patch_bm=%d pgemm_bm=%d ktot=%d "
                   "place=%s carries=%s branch=%s flops=%.17g bytes=%.17g flops_executed=%.17g "
                   "branch_tile=%s branch_psgemm=%d branch_flops=%.17g branch_bytes=%.17g\n",
                   name, NC, n, r.name.c_str(), FORM[P.form], TILE[P.tile], P.splitk, P.tile_256, P.patch_bm, P.pgemm_bm, P.ktot,
                   PLACE[r.d.branch.place], PLACE[r.d.carries], LAUNCH[P.branch], P.acct.flops, P.acct.bytes, P.acct.flops_executed,
                   TILE[P.branch_gemm.tile], P.branch_gemm.psgemm, P.branch_gemm.acct.flops, P.branch_gemm.acct.bytes);
        }
    }
    return 0;
}

// Stand-alone table program of tests/test_engine_plan.py and tests/test_wino4.py: the ResNet-18 engine's own layer table
// (csrc/engine_table.h, the one pa_create builds) and what plan_conv (csrc/engine_plan.h) plans from it, without a GPU. Arguments:
// NAME=value sets a knob in this process's environment (read by the library's own engine_knobs()); dtype:max_crops:crops[:S] (dtype =
// f32 | emulated_f32 | bf16; S: the model's sequence length, 7 unless given -- the split-K slab counts the temporal head) prints one
// "forms" line and one "plan" line per row of the seventeen-conv table + fc; blob:S:A prints the weight blob's float count. The first
// line is the knobs that decide F(4x4, 3x3).
#include "../../playaid_core_amd/csrc/engine_table.h"

#include <cstdio>
#include <cstring>

using namespace pa;

namespace {

const char* const FORM[] = {"psgemm", "bf16_patch", "bf16_im2col", "wino", "patch", "pgemm", "im2col"};
const char* const TILE[] = {"128x128", "128x64", "64x64", "128x64_k64", "64x64_k64", "256x128"};
const char* const PLACE[] = {"none", "second_k", "own_gemm", "opener", "opener_probe"};
const char* const LAUNCH[] = {"none", "second_k", "gemm_before", "stored", "on_opener", "gemm_behind"};

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (strchr(argv[i], '=')) putenv(argv[i]);
    const EngineKnobs K = engine_knobs();
    printf("knobs wino_f4=%d wino_f4_min=%d default_min=%d\n", K.wino_f4, K.wino_f4_min, WINO_F4_MIN_CROPS);
    for (int i = 1; i < argc; ++i) {
        if (strchr(argv[i], '=')) continue;
        char name[32];
        int NC = 0, n = 0, S = 7;
        const int fields = sscanf(argv[i], "%31[^:]:%d:%d:%d", name, &NC, &n, &S);
        if (fields < 3 || NC < 1 || n < 1 || S < 1) return 2;
        if (!strcmp(name, "blob")) {   // blob:S:A
            printf("blob S=%d A=%d floats=%zu\n", NC, n, blob_floats(engine_table(K, DT_F32, 1), NC, n));
            continue;
        }
        if (n > NC) return 2;
        const ComputeDtype dt = !strcmp(name, "bf16") ? DT_BF16 : !strcmp(name, "emulated_f32") ? DT_EMULATED_F32 : DT_F32;
        if (dt == DT_F32 && strcmp(name, "f32")) return 2;
        const EngineForms F = engine_forms(K, dt);
        printf("forms dtype=%s stem_fused=%d stem_int=%d opener_branch=%d\n", name, F.stem_fused, F.stem_int, F.opener_branch);
        const std::vector<TableRow> rows = engine_table(K, dt, NC);
        const size_t slab = slab_floats(rows, K, NC, S);
        for (const TableRow& r : rows) {
            const ConvPlan P = plan_conv(K, dt, r.d, n, slab, /*branch_on_side=*/false);
            printf("plan dtype=%s max_crops=%d crops=%d layer=%s form=%s tile=%s splitk=%d tile_256=%d patch_bm=%d pgemm_bm=%d ktot=%d "
                   "wino4=%d wino_f4=%d place=%s carries=%s branch=%s flops=%.17g bytes=%.17g flops_executed=%.17g "
                   "branch_tile=%s branch_psgemm=%d branch_flops=%.17g branch_bytes=%.17g\n",
                   name, NC, n, r.name.c_str(), FORM[P.form], TILE[P.tile], P.splitk, P.tile_256, P.patch_bm, P.pgemm_bm, P.ktot,
                   r.d.wino4, P.wino_f4, PLACE[r.d.branch.place], PLACE[r.d.carries], LAUNCH[P.branch], P.acct.flops, P.acct.bytes, P.acct.flops_executed,
                   TILE[P.branch_gemm.tile], P.branch_gemm.psgemm, P.branch_gemm.acct.flops, P.branch_gemm.acct.bytes);
        }
    }
    return 0;
}

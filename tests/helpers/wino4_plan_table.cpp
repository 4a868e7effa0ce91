// Stand-alone table program of tests/test_wino4.py: which stride-1 3x3 rows of the ResNet-18 engine plan_conv (csrc/engine_plan.h)
// sends to Winograd F(4x4, 3x3) taken apart, without a GPU. Arguments: NAME=value sets a knob in this process's environment (read by
// the library's own engine_knobs()); dtype:max_crops:crops (dtype = f32 | emulated_f32 | bf16) prints one line per row of the four
// layers' second blocks (layerN.1.conv1: cin = cout = 64 .. 512 on maps of 32 .. 4), with the row's flags set the way pa_api.hip's
// create_impl sets them.
#include "../../playaid_core_amd/csrc/engine_plan.h"

#include <cstdio>
#include <cstring>

using namespace pa;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (strchr(argv[i], '=')) putenv(argv[i]);
    const EngineKnobs K = engine_knobs();
    printf("knobs wino_f4=%d wino_f4_min=%d default_min=%d\n", K.wino_f4, K.wino_f4_min, WINO_F4_MIN_CROPS);
    static const char* const FORM[] = {"psgemm", "bf16_patch", "bf16_im2col", "wino", "patch", "pgemm", "im2col"};
    for (int i = 1; i < argc; ++i) {
        if (strchr(argv[i], '=')) continue;
        char name[32];
        int NC = 0, n = 0;
        if (sscanf(argv[i], "%31[^:]:%d:%d", name, &NC, &n) != 3 || NC < 1 || n < 1 || n > NC) return 2;
        const ComputeDtype dt = !strcmp(name, "bf16") ? DT_BF16 : !strcmp(name, "emulated_f32") ? DT_EMULATED_F32 : DT_F32;
        if (dt == DT_F32 && strcmp(name, "f32")) return 2;
        const int widths[4] = {64, 128, 256, 512}, hw[4] = {32, 16, 8, 4};
        for (int li = 0; li < 4; ++li) {
            LayerDesc L = conv_desc(K, dt, NC, widths[li], widths[li], 3, 1, hw[li], false);
            L.wino = wino_layer(K, dt, L);
            L.wino4 = wino4_layer(K, dt, L, NC);
            const ConvPlan P = plan_conv(K, dt, L, n, (size_t)1 << 24, false);
            printf("plan dtype=%s max_crops=%d crops=%d layer=layer%d.1.conv1 form=%s has_f4_filters=%d wino_f4=%d flops=%.17g flops_executed=%.17g\n", name, NC, n,
                   li + 1, FORM[P.form], L.wino4 ? 1 : 0, P.wino_f4 ? 1 : 0, P.acct.flops, P.acct.flops_executed);
        }
    }
    return 0;
}

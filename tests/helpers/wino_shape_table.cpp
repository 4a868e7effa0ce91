// Stand-alone table program of tests/test_wino_shape_rule.py: how the ResNet-18 engine shapes the launches of each of its sixteen
// 3x3 layers on the Winograd F(2x2, 3x3) kernel (csrc/wino_shape.h through csrc/engine_plan.h's wino_layer_shape, over the engine's own
// layer table, csrc/engine_table.h), without a GPU. Arguments: NAME=value sets a knob in this process's environment (read by the
// library's own engine_knobs()); dtype:max_crops (dtype = f32 | emulated_f32) prints one "shape" line per 3x3 row.
#include "../../playaid_core_amd/csrc/engine_table.h"

#include <cstdio>
#include <cstring>

using namespace pa;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (strchr(argv[i], '=')) putenv(argv[i]);
    const EngineKnobs K = engine_knobs();
    static const char* const SHAPE[] = {"split", "unsplit8", "unsplit4", "tg2"};
    printf("knobs wino_l3_shape=%d default=%s min_wg=%lld\n", K.wino_l3_shape, SHAPE[WINO_SHAPE_DEFAULT], WINO_SHAPE_MIN_WG);
    for (int i = 1; i < argc; ++i) {
        if (strchr(argv[i], '=')) continue;
        char name[32];
        int NC = 0;
        if (sscanf(argv[i], "%31[^:]:%d", name, &NC) != 2 || NC < 1) return 2;
        const ComputeDtype dt = !strcmp(name, "emulated_f32") ? DT_EMULATED_F32 : DT_F32;
        if (dt == DT_F32 && strcmp(name, "f32")) return 2;
        for (const TableRow& r : engine_table(K, dt, NC)) {
            if (r.d.kh != 3) continue;
            if (!r.d.wino) {
                printf("shape dtype=%s max_crops=%d layer=%s wino=0 shape=none bn=0\n", name, NC, r.name.c_str());
                continue;
            }
            const WinoLayerShape ws = wino_layer_shape(K, r.d, NC);
            printf("shape dtype=%s max_crops=%d layer=%s wino=1 shape=%s bn=%d\n", name, NC, r.name.c_str(), SHAPE[ws.shape], ws.bn);
        }
    }
    return 0;
}

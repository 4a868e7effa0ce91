// Stand-alone table program of tests/test_wino_wg_rule.py: the launch width (output channels per workgroup) the ResNet-18 engine
// gives each of its sixteen 3x3 layers on the Winograd F(2x2, 3x3) kernel, beside the shape and the filter layout they have
// (csrc/wino_shape.h through csrc/engine_plan.h's wino_layer_wg, over the engine's own layer table, csrc/engine_table.h), without a
// GPU. Arguments: NAME=value sets a knob in this process's environment (read by the library's own engine_knobs()); dtype:max_crops
// (dtype = f32 | emulated_f32) prints one "width" line per 3x3 row; dtype:max_crops:crops prints instead whether a launch of `crops`
// crops of that engine takes width 32 (what pa_api.hip's run_conv decides per launch).
#include "../../playaid_core_amd/csrc/engine_table.h"

#include <cstdio>
#include <cstring>

using namespace pa;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (strchr(argv[i], '=')) putenv(argv[i]);
    const EngineKnobs K = engine_knobs();
    static const char* const SHAPE[] = {"split", "unsplit8", "unsplit4", "tg2"};
    printf("knobs wino_wg=%d wino_wg_hw=%d ks_force=%d bn_force=%d\n", K.wino_wg, K.wino_wg_hw, wino_ks_force(), wino_bn_force());
    for (int i = 1; i < argc; ++i) {
        if (strchr(argv[i], '=')) continue;
        char name[32];
        int NC = 0, n = 0;
        const int fields = sscanf(argv[i], "%31[^:]:%d:%d", name, &NC, &n);
        if (fields < 2 || NC < 1 || (fields == 3 && (n < 1 || n > NC))) return 2;
        const ComputeDtype dt = !strcmp(name, "emulated_f32") ? DT_EMULATED_F32 : DT_F32;
        if (dt == DT_F32 && strcmp(name, "f32")) return 2;
        for (const TableRow& r : engine_table(K, dt, NC)) {
            if (r.d.kh != 3) continue;
            if (!r.d.wino) {
                printf("width dtype=%s max_crops=%d crops=%d layer=%s wino=0 shape=none bn=0 wg=0 launch_wg=0\n", name, NC, fields == 3 ? n : NC, r.name.c_str());
                continue;
            }
            const WinoLayerShape ws = wino_layer_shape(K, r.d, NC);
            const int wg = wino_layer_wg(K, r.d, NC), crops = fields == 3 ? n : NC;
            printf("width dtype=%s max_crops=%d crops=%d layer=%s wino=1 shape=%s bn=%d wg=%d launch_wg=%d\n", name, NC, crops, r.name.c_str(),
                   SHAPE[ws.shape], ws.bn, wg, wino_launch_wg(wg, ws.bn, r.d.cin, r.d.cout, r.d.out_hw, crops, wino_ks_force()));
        }
    }
    return 0;
}

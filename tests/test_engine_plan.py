"""What the ResNet-18 engine plans for each layer (csrc/engine_plan.h: the knob table, plan_conv), without a GPU.

tests/helpers/engine_plan_table.cpp prints the seventeen-conv table + fc that ``pa_create`` itself builds (csrc/engine_table.h: the
rows, the split-K slab and the weight blob's float count are the engine's own, not a copy), one line per (dtype, max crops, crops,
layer); knob settings are arguments, so nothing here touches this process's environment. It is compiled with the host C++ compiler
alone ($CXX, else g++): no hipcc, no GPU.

The expected values are written out by hand from the rules themselves -- ``choose_tile`` / ``im2col_tile`` (transcribed here as
``choose_tile``), the order of forms, ``wino4_layer``'s rule and the table's placement of the 1x1/2 branches -- never
taken from ``plan_conv``'s output. They are also what tests/helpers/opener_branch_worker.py and tests/test_backbone_layers.py say their batch
sizes reach.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "engine_plan_table.cpp")

OPENERS = ["layer2.0.conv1", "layer3.0.conv1", "layer4.0.conv1"]
BLOCK0_CONV2 = ["layer2.0.conv2", "layer3.0.conv2", "layer4.0.conv2"]
STRIDE1 = [f"layer{l}.{b}.conv{c}" for l in (1, 2, 3, 4) for b in (0, 1) for c in (1, 2) if not (l > 1 and b == 0 and c == 1)]
WIDTH = {1: 64, 2: 128, 3: 256, 4: 512}   # output channels of layer l
OUT_HW = {1: 32, 2: 16, 3: 8, 4: 4}


def choose_tile(M, N, nk):
    """The engine's rule for tile and K split (engine_plan.h's choose_tile over gemm_tile.h's im2col_tile), written out again."""
    t128 = (M + 127) // 128 * (N // 64)
    tile = "128x128" if (N % 128 == 0 and t128 // 2 >= 512) else ("128x64" if t128 >= 512 else "64x64")
    tm = (M + 127) // 128
    tiles = tm * (N // 128) if tile == "128x128" else tm * (N // 64) if tile == "128x64" else ((M + 63) // 64) * (N // 64)
    sk = 1
    while tiles * sk < 512 and nk // (sk * 2) >= 8:
        sk *= 2
    return tile, sk


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = os.environ.get("CXX") or "g++"
    if not shutil.which(cxx.split()[0]):
        pytest.skip(f"no host C++ compiler ({cxx})")
    exe = str(tmp_path_factory.mktemp("engine_plan") / "engine_plan_table")
    subprocess.run(cxx.split() + ["-std=c++17", "-O1", "-o", exe, SRC], check=True)
    cache = {}

    def run(cases, *knobs):
        """{(dtype, max_crops, crops, layer): fields}, {dtype: forms} of the cases "dtype:max:crops" under the knobs "NAME=value"."""
        key = (tuple(cases), knobs)
        if key not in cache:
            env = {k: v for k, v in os.environ.items() if not k.startswith("PA_")}
            out = subprocess.run([exe, *knobs, *cases], check=True, capture_output=True, text=True, env=env).stdout
            plans, forms = {}, {}
            for line in out.splitlines():
                kind, *fields = line.split()
                f = dict(x.split("=", 1) for x in fields)
                if kind == "forms":
                    forms[f["dtype"]] = f
                elif kind == "plan":
                    plans[(f["dtype"], int(f["max_crops"]), int(f["crops"]), f["layer"])] = f
            cache[key] = (plans, forms)
        return cache[key]

    run.exe = exe
    return run


def rows(plans, dtype, max_crops, crops):
    return {k[3]: v for k, v in plans.items() if k[:3] == (dtype, max_crops, crops)}


F32_CASES = [f"f32:128:{n}" for n in (1, 5, 35, 64, 128)]
LAYER4_STRIDE1 = ["layer4.0.conv2", "layer4.1.conv1", "layer4.1.conv2"]   # the 4 x 4 maps: F(4x4, 3x3) from 64 crops per launch


def test_f32_openers_at_default_knobs(table):
    plans, forms = table(F32_CASES)
    assert forms["f32"]["stem_int"] == "1" and forms["f32"]["stem_fused"] == "1"
    # (tile, split K, form, where the branch goes) of layer2/3/4.0.conv1
    behind, fused, none = "gemm_behind", "on_opener", "none"
    want = {
        1: [("64x64", 2, "im2col", behind), ("64x64", 4, "im2col", behind), ("64x64", 8, "im2col", none)],
        5: [("64x64", 2, "im2col", behind), ("64x64", 4, "im2col", behind), ("64x64", 8, "im2col", none)],
        64: [("64x64", 1, "pgemm", fused), ("64x64", 2, "im2col", behind), ("64x64", 4, "im2col", none)],
        128: [("128x64", 1, "pgemm", fused), ("64x64", 1, "pgemm", fused), ("64x64", 2, "im2col", none)],
    }
    for n, exp in want.items():
        r = rows(plans, "f32", 128, n)
        for l, name, (tile, sk, form, branch) in zip((2, 3, 4), OPENERS, exp):
            assert choose_tile(n * OUT_HW[l] ** 2, WIDTH[l], 9 * WIDTH[l - 1] // 32) == (tile, sk), (n, name)  # the table above is choose_tile's
            got = r[name]
            assert (got["tile"], int(got["splitk"]), got["form"], got["branch"]) == (tile, sk, form, branch), (n, name, got)
            if form == "pgemm":
                assert got["pgemm_bm"] == "64"
            assert got["carries"] == ("opener" if l < 4 else "none")
        # blocks 2-3: conv2 finds the branch stored (by the opener or the GEMM behind it); block 4: its own GEMM in front of conv2
        assert [r[c]["branch"] for c in BLOCK0_CONV2] == ["stored", "stored", "gemm_before"], n
        assert [r[c]["place"] for c in BLOCK0_CONV2] == ["opener", "opener", "own_gemm"], n
        # an opener that carries the branch books its cin more K and a second output; the GEMM behind books the branch itself
        for l, name in zip((2, 3), OPENERS):
            M, N, cin = n * OUT_HW[l] ** 2, WIDTH[l], WIDTH[l - 1]
            here = r[name]["branch"] == fused
            assert float(r[name]["flops"]) == 2.0 * M * N * (9 * cin + (cin if here else 0))
            assert float(r[name]["branch_flops"]) == 2.0 * M * N * cin


def test_f32_default_any_batch(table):
    plans, _ = table(F32_CASES)
    for n in (1, 5, 35, 64, 128):
        r = rows(plans, "f32", 128, n)
        assert len(r) == 18
        for name in STRIDE1:
            assert r[name]["form"] == "wino", (n, name)
            f4 = name in LAYER4_STRIDE1 and n >= 64
            assert r[name]["wino_f4"] == str(int(f4)), (n, name)
            assert float(r[name]["flops_executed"]) == float(r[name]["flops"]) * (1.0 / 4.0 if f4 else 4.0 / 9.0), (n, name)
        for l, name in zip((2, 3, 4), BLOCK0_CONV2):
            assert r[name]["branch"] in ("stored", "gemm_before") and r[name]["place"] != "second_k"
            assert int(r[name]["ktot"]) == 9 * WIDTH[l]   # no second K source
            assert float(r[name]["flops"]) == 2.0 * n * OUT_HW[l] ** 2 * WIDTH[l] * 9 * WIDTH[l]
        assert (r["fc"]["form"], r["fc"]["tile"], r["fc"]["splitk"]) == ("im2col", "64x64", "4")
        assert r["conv1"]["form"] == "im2col"   # (the generic stem: only PA_STEM_IGEMM=1 launches it)


def test_f4_filters_per_case(table):
    """LayerDesc::wino4 by wino4_layer's rule: an exact dtype, a Winograd layer on a 4 x 4 map, PA_WINO_F4, and an engine whose full
    batch reaches the threshold of 64 crops."""
    def have(case, *knobs):
        return sorted(k[3] for k, v in table([case], *knobs)[0].items() if v["wino4"] == "1")

    assert have("f32:128:128") == LAYER4_STRIDE1
    assert have("f32:128:1") == LAYER4_STRIDE1       # the filters belong to the engine, not to the launch
    assert have("emulated_f32:128:128") == LAYER4_STRIDE1
    assert have("f32:32:32") == []
    assert have("f32:128:128", "PA_WINO_F4=0") == []
    assert have("bf16:128:128") == []
    assert all(v["wino_f4"] == "0" for case in ("f32:32:32", "bf16:128:128", "f32:128:1") for v in table([case])[0].values())
    assert all(v["wino_f4"] == "0" for v in table(["f32:128:128"], "PA_WINO_F4=0")[0].values())


@pytest.mark.parametrize("S,A", [(1, 1), (5, 7), (15, 64)])
def test_blob_float_count(table, S, A):
    """The table's count of the weight blob against Python's own statement of it and against ResNet-18 counted by hand: 11 689 512
    parameters (the 1000-way fc included) + running mean and variance of 4 800 BatchNorm channels = 11 699 112."""
    import math

    from playaid_core_amd.weights import blob_key_order

    out = subprocess.run([table.exe, f"blob:{S}:{A}"], check=True, capture_output=True, text=True).stdout.splitlines()
    got = [dict(x.split("=", 1) for x in line.split()[1:]) for line in out if line.startswith("blob ")]
    assert len(got) == 1 and (got[0]["S"], got[0]["A"]) == (str(S), str(A))
    assert int(got[0]["floats"]) == sum(math.prod(shape) for _, shape in blob_key_order(S, A))
    assert int(got[0]["floats"]) == 11_699_112 + 512 * 1000 * S + 512 + 128 * 512 + 128 + 128 * A + A


def test_knob_precedence_f32(table):
    base, base_forms = table(F32_CASES)
    # PA_PATCH acts only on the layers PA_WINO leaves alone
    assert table(F32_CASES, "PA_PATCH=0")[0] == base
    for n in (1, 35, 128):
        case = [f"f32:128:{n}"]
        patch = rows(table(case, "PA_WINO=0")[0], "f32", 128, n)
        im2col = rows(table(case, "PA_WINO=0", "PA_PATCH=0")[0], "f32", 128, n)
        for name in STRIDE1:
            assert patch[name]["form"] == "patch" and patch[name]["patch_bm"] in ("64", "128"), (n, name)
            assert im2col[name]["form"] == "im2col", (n, name)
        for r in (patch, im2col):
            for l, name in zip((2, 3, 4), BLOCK0_CONV2):
                assert r[name]["branch"] == "second_k" and r[name]["place"] == "second_k"
                assert int(r[name]["ktot"]) == 9 * WIDTH[l] + WIDTH[l - 1]
            assert all(r[o]["carries"] == "none" and r[o]["branch"] == "none" for o in OPENERS)
        hw8 = rows(table(case, "PA_WINO_MIN_HW=8")[0], "f32", 128, n)
        for name in STRIDE1:
            assert hw8[name]["form"] == ("patch" if name.startswith("layer4") else "wino"), (n, name)
        assert hw8["layer4.0.conv2"]["branch"] == "second_k" and hw8["layer3.0.conv2"]["branch"] == "stored"
    for knob in ("PA_DS_SIDE=1", "PA_S2_PGEMM=0", "PA_F32_DS_FUSE=0"):
        plans, forms = table(F32_CASES, knob)
        assert forms["f32"]["opener_branch"] == "0"
        assert all(v["branch"] not in ("on_opener", "gemm_behind") and v["carries"] == "none" for v in plans.values()), knob
        for n in (1, 128):
            assert [rows(plans, "f32", 128, n)[c]["branch"] for c in BLOCK0_CONV2] == ["gemm_before"] * 3, knob
    assert all(v["form"] != "pgemm" for v in table(F32_CASES, "PA_S2_PGEMM=0")[0].values())
    own = rows(table(F32_CASES, "PA_S2_PGEMM=1")[0], "f32", 128, 128)
    assert own["layer2.0.conv1"]["branch"] == "on_opener" and own["layer4.0.conv1"]["form"] == "im2col"
    assert base_forms["f32"]["stem_int"] == "1"
    for knob in ("PA_STEM_POOL=0", "PA_STEM_IGEMM=1", "PA_STEM_IGEMM=-1", "PA_STEM_INT=0"):
        assert table(F32_CASES, knob)[1]["f32"]["stem_int"] == "0", knob
    for knob in ("PA_STEM_POOL=0", "PA_STEM_IGEMM=1"):
        assert table(F32_CASES, knob)[1]["f32"]["stem_fused"] == "0", knob


def test_bf16_openers(table):
    cases = ["bf16:136:136", "bf16:136:35"]
    plans, forms = table(cases)
    assert forms["bf16"]["stem_int"] == "0"
    full, part = rows(plans, "bf16", 136, 136), rows(plans, "bf16", 136, 35)
    assert (136 * 256 + 127) // 128 * (128 // 128) == 272   # >= 256: the 128x128 tile
    for r, tile in ((full, "128x128"), (part, "128x64")):
        o = r["layer2.0.conv1"]
        assert (o["form"], o["tile"], o["splitk"], o["branch"], o["tile_256"]) == ("bf16_im2col", tile, "1", "on_opener", "0")
        assert [r[c]["branch"] for c in BLOCK0_CONV2] == ["stored"] * 3
        assert all(r[name]["form"] == "bf16_patch" for name in STRIDE1)
    probe = table(cases, "PA_BF16_DS_FUSE=2")[0]
    for n, tile in ((136, "128x128"), (35, "128x64")):
        r = rows(probe, "bf16", 136, n)
        o = r["layer2.0.conv1"]
        assert (o["form"], o["tile"], o["splitk"], o["branch"], o["carries"]) == ("bf16_im2col", tile, "1", "none", "opener_probe")
        assert [r[c]["branch"] for c in BLOCK0_CONV2] == ["gemm_before"] * 3
        assert r["layer2.0.conv2"]["branch_tile"] == "128x64"
    own = table(cases, "PA_BF16_DS_FUSE=0")[0]
    for n in (136, 35):
        r = rows(own, "bf16", 136, n)
        for l, name in zip((2, 3, 4), OPENERS):
            tile, sk = choose_tile(n * OUT_HW[l] ** 2, WIDTH[l], 9 * WIDTH[l - 1] // 64)
            assert (r[name]["tile"], int(r[name]["splitk"]), r[name]["branch"], r[name]["carries"]) == (tile, sk, "none", "none")
        assert [r[c]["branch"] for c in BLOCK0_CONV2] == ["gemm_before"] * 3
    assert (rows(own, "bf16", 136, 136)["layer2.0.conv1"]["tile"], rows(own, "bf16", 136, 35)["layer2.0.conv1"]["tile"]) == ("128x64", "64x64")
    assert all(v["form"] == "bf16_im2col" for k, v in table(cases, "PA_BF16_PATCH=0")[0].items() if k[3] in STRIDE1)


def test_emulated_f32(table):
    plans, forms = table(["emulated_f32:128:1", "emulated_f32:128:128"])
    assert forms["emulated_f32"]["stem_int"] == "1" and forms["emulated_f32"]["opener_branch"] == "0"
    for n in (1, 128):
        r = rows(plans, "emulated_f32", 128, n)
        for name in OPENERS:
            assert (r[name]["form"], r[name]["carries"], r[name]["branch"]) == ("psgemm", "none", "none")
        for name in BLOCK0_CONV2:
            assert (r[name]["form"], r[name]["place"], r[name]["branch"], r[name]["branch_psgemm"]) == ("wino", "own_gemm", "gemm_before", "1")
        assert all(r[name]["form"] == "wino" for name in STRIDE1)

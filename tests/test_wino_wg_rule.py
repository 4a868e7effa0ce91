"""The launch width of the ResNet-18 engine's Winograd layers (csrc/wino_shape.h's wino_layer_wg through csrc/engine_plan.h), without a
GPU: tests/helpers/wino_wg_table.cpp prints, over the table ``pa_create`` itself builds, the width (output channels per workgroup) each
of the sixteen 3x3 layers gets beside its shape and filter layout. Compiled with the host C++ compiler alone ($CXX, else g++).

The expected values are written out by hand from the rule. The width is open for a layer on maps of at least 16 x 16 (layers 1 and 2)
whose filters are laid out for 64 channels and whose launch at the full batch the launcher could not split. Sub-blocks = crops x (map /
4)^2, 64-channel workgroups = ceil(sub-blocks / 16) x cout / 64, the layout is 64 from 192 of them (times the K split) on:

  layer 1 (32 x 32, 64 -> 64, 8 chunks: never split): 4 workgroups per crop -> 64-channel layout from 48 crops: open at 64 .. 256
  layer 2 (16 x 16, 128 -> 128, 16 chunks: two splits while they fit 256): 2 per crop -> at 64 crops 128 x 2 splits: layout 64 but
    split, closed; at 80 crops 160 (no split fits, under 192): layout 32, closed; at 96, 125, 128, 256 crops 192 .. 512: open
  1, 5 and 16 crops: 32-channel layouts everywhere, closed

A closed layer's width is its layout's. ``PA_WINO_WG=32|64`` forces the open layers, ``PA_WINO_WG_HW=32|16`` only those on maps of that
width; unset, the rule takes 32 where profiles/wino_wg_width_parent_ab.md measured it to win (DEFAULT_32 below). A launch of fewer crops
than the engine's takes width 32 only if it, too, cannot split."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "helpers")

CROPS = (1, 5, 16, 64, 80, 96, 125, 128, 256)
OPENERS = ["layer2.0.conv1", "layer3.0.conv1", "layer4.0.conv1"]
LAYER1 = [f"layer1.{b}.conv{c}" for b in (0, 1) for c in (1, 2)]
LAYER2 = ["layer2.0.conv2", "layer2.1.conv1", "layer2.1.conv2"]
ALL3X3 = [f"layer{l}.{b}.conv{c}" for l in (1, 2, 3, 4) for b in (0, 1) for c in (1, 2)]
OPEN = {1: (64, 80, 96, 125, 128, 256), 2: (96, 125, 128, 256)}    # layer -> max_crops at which its width is open
# knob unset: (layer, max_crops) that take width 32 -- where it was measured to win by the project's bar
DEFAULT_32 = {(1, 64), (1, 96), (1, 125), (1, 128), (2, 96), (2, 125), (2, 128)}
DTYPES = ("f32", "emulated_f32")


def _build(tmp, name):
    cxx = os.environ.get("CXX") or "g++"
    if not shutil.which(cxx.split()[0]):
        pytest.skip(f"no host C++ compiler ({cxx})")
    exe = str(tmp / name)
    subprocess.run(cxx.split() + ["-std=c++17", "-O1", "-o", exe, os.path.join(HELPERS, name + ".cpp")], check=True)
    return exe


def _rows(exe, cases, knobs, keys):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PA_")}
    out = subprocess.run([exe, *knobs, *cases], check=True, capture_output=True, text=True, env=env).stdout
    rows, head = {}, None
    for line in out.splitlines():
        kind, *fields = line.split()
        f = dict(x.split("=", 1) for x in fields)
        if kind == "knobs":
            head = f
        else:
            rows[(f["dtype"], int(f["max_crops"]), int(f.get("crops", f["max_crops"])), f["layer"])] = tuple(
                f[k] if k == "shape" else int(f[k]) for k in keys)
    return head, rows


@pytest.fixture(scope="module")
def width_table(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("wino_wg"), "wino_wg_table")
    return lambda cases, *knobs: _rows(exe, cases, knobs, ("shape", "bn", "wg", "launch_wg"))


@pytest.fixture(scope="module")
def shape_table(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("wino_shape2"), "wino_shape_table")
    return lambda cases, *knobs: _rows(exe, cases, knobs, ("shape", "bn"))


CASES = [f"{dt}:{nc}" for dt in DTYPES for nc in CROPS]
KNOBS = [(), ("PA_WINO_WG=32",), ("PA_WINO_WG=64",), ("PA_WINO_WG=32", "PA_WINO_WG_HW=32"), ("PA_WINO_WG=32", "PA_WINO_WG_HW=16"),
         ("PA_WINO_WG=64", "PA_WINO_WG_HW=32")]


def _layer_of(name):
    return 1 if name in LAYER1 else 2 if name in LAYER2 else 0


def _expected_wg(layer, nc, bn, knobs):
    li = _layer_of(layer)
    if not li or nc not in OPEN[li]:
        return bn
    k = dict(x.split("=") for x in knobs)
    hw = int(k.get("PA_WINO_WG_HW", 0))
    if "PA_WINO_WG" in k and hw in (0, {1: 32, 2: 16}[li]):
        return int(k["PA_WINO_WG"])
    return 32 if (li, nc) in DEFAULT_32 else 64


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "+".join(k) or "unset")
def test_width_per_layer(width_table, knobs):
    head, rows = width_table(CASES, *knobs)
    k = dict(x.split("=") for x in knobs)
    assert head["wino_wg"] == k.get("PA_WINO_WG", "0") and head["wino_wg_hw"] == k.get("PA_WINO_WG_HW", "0")
    assert len(rows) == len(CASES) * 16
    for (dt, nc, n, layer), (shape, bn, wg, launch_wg) in rows.items():
        if layer in OPENERS:
            assert (shape, bn, wg, launch_wg) == ("none", 0, 0, 0)
            continue
        assert wg == _expected_wg(layer, nc, bn, knobs), (dt, nc, layer)
        assert launch_wg == wg and n == nc   # at the full batch the launch is the layer's
        if wg != bn:
            assert (wg, bn, shape) == (32, 64, "split") and _layer_of(layer), (dt, nc, layer)
    # the open layers are on 64-channel layouts, and the forced width reaches exactly them
    if k.get("PA_WINO_WG") == "32" and "PA_WINO_WG_HW" not in k:
        narrow = {(nc, layer) for (dt, nc, n, layer), v in rows.items() if dt == "f32" and v[2] == 32 and v[1] == 64}
        assert narrow == {(nc, layer) for li, names in ((1, LAYER1), (2, LAYER2)) for layer in names for nc in OPEN[li]}


@pytest.mark.parametrize("knobs", KNOBS + [("PA_WINO_WG=32", "PA_WINO_L3_SHAPE=1"), ("PA_WINO_WG=32", "PA_WINO_BN=64", "PA_WINO_KS=1")],
                         ids=lambda k: "+".join(k) or "unset")
def test_shapes_and_layouts_did_not_move(width_table, shape_table, knobs):
    """(shape, bn) as tests/helpers/wino_shape_table.cpp prints them: the same with and without the width knobs, and the same in both
    programs."""
    other = tuple(x for x in knobs if not x.startswith("PA_WINO_WG"))
    _, before = shape_table(CASES, *other)
    _, after = shape_table(CASES, *knobs)
    assert before == after and len(after) == len(CASES) * 16
    _, widths = width_table(CASES, *knobs)
    assert {key: v[:2] for key, v in widths.items()} == after


def test_known_layouts_at_the_headline(shape_table):
    """... and what they are at 128 crops, by hand (tests/test_wino_shape_rule.py): layers 1, 2 and 4 split / 64, layer 3 unsplit4 / 32."""
    _, rows = shape_table(["f32:128"], "PA_WINO_WG=32")
    for layer in ALL3X3:
        want = ("none", 0) if layer in OPENERS else ("unsplit4", 32) if layer.startswith("layer3") else ("split", 64)
        assert rows[("f32", 128, 128, layer)] == want, layer


def test_small_engines_on_forced_64_channel_layouts_are_open(width_table):
    """PA_WINO_BN=64 PA_WINO_KS=1 (what tests/test_wino_wg_engine.py runs its engines of 16 crops under): every layer of layers 1 and 2
    on a 64-channel layout, never split, so the knob reaches them at every size, at the full batch and at 5 crops."""
    for nc, n in ((16, 16), (16, 5), (5, 5), (1, 1)):
        for v, want in (("32", 32), ("64", 64)):
            _, rows = width_table([f"f32:{nc}:{n}"], f"PA_WINO_WG={v}", "PA_WINO_BN=64", "PA_WINO_KS=1")
            for layer in LAYER1 + LAYER2:
                assert rows[("f32", nc, n, layer)] == ("split", 64, want, want), (nc, n, layer)
            for layer in ("layer3.1.conv1", "layer4.1.conv2"):
                assert rows[("f32", nc, n, layer)][1:] == (64, 64, 64), (nc, n, layer)


def test_a_launch_of_few_crops_keeps_its_split(width_table):
    """An engine of 128 crops with width 32 on layers 1 and 2, launched over 5 and over 64 crops: layer 2 (16 chunks) has 10 and 128
    64-channel workgroups there, which the launcher splits two ways -- it keeps the eight-wave workgroups and the split it had; layer 1
    (8 chunks) can never split and takes width 32 at every size."""
    for n in (5, 64):
        _, rows = width_table([f"f32:128:{n}"], "PA_WINO_WG=32")
        for layer in LAYER1:
            assert rows[("f32", 128, n, layer)] == ("split", 64, 32, 32), (n, layer)
        for layer in LAYER2:
            assert rows[("f32", 128, n, layer)] == ("split", 64, 32, 64), (n, layer)
    _, rows = width_table(["f32:128:65"], "PA_WINO_WG=32")   # 130 workgroups x 2 > 256: no split
    assert rows[("f32", 128, 65, "layer2.1.conv1")] == ("split", 64, 32, 32)


def test_unknown_knob_values_leave_the_rule_alone(width_table):
    _, unset = width_table(CASES)
    for v in ("0", "16", "48", "128", "-32"):
        _, rows = width_table(CASES, f"PA_WINO_WG={v}")
        assert rows == unset, v


def test_table_program_is_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program, built with -fsanitize=address,undefined (the runtimes linked statically: the program then stands
    alone whatever else the process loads) and run on the CPU, ends clean."""
    cxx = os.environ.get("CXX") or "g++"
    if not shutil.which(cxx.split()[0]):
        pytest.skip(f"no host C++ compiler ({cxx})")
    exe = str(tmp_path / "wino_wg_table_san")
    subprocess.run(cxx.split() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                                  os.path.join(HELPERS, "wino_wg_table.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PA_")}
    for knobs in KNOBS:
        r = subprocess.run([exe, *knobs, *CASES, "f32:128:5"], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]

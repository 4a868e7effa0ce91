"""Loading an ultralytics YOLOv5 ``.pt`` without the YOLOv5 checkout (``playaid_core_amd.yolov5_checkpoint``).

The checkpoints are written here: stand-in classes registered as ``models.yolo`` / ``models.common`` while ``torch.save``
pickles a module tree of the checkpoint's layout (fp16, as ultralytics saves it), then removed from ``sys.modules`` before
loading, as on a machine without the checkout.
"""
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from playaid_core_amd import synth

NAMES80 = [f"class{i}" for i in range(80)]


def _classes():
    yolo, common = types.ModuleType("models.yolo"), types.ModuleType("models.common")
    out = {}
    for mod, names in ((yolo, ("DetectionModel", "Model", "Detect", "Segment", "ClassificationModel")),
                       (common, ("Conv", "C3", "Bottleneck", "SPPF", "Concat", "Focus", "SPP", "Proto"))):
        for n in names:
            cls = type(n, (torch.nn.Module,), {"__module__": mod.__name__, "__qualname__": n})
            setattr(mod, n, cls)
            out[n] = cls
    return {"models": types.ModuleType("models"), "models.yolo": yolo, "models.common": common}, out


def _tree(sd, C, model_cls="DetectionModel", sppf="SPPF", head="Detect", act=torch.nn.SiLU):
    """A module tree whose state_dict() is sd (fp16), of the checkout's classes."""
    def node(path, keys):
        kids = sorted({k[len(path) + 1:].split(".")[0] for k in keys if k.startswith(path + ".")}, key=lambda s: (not s.isdigit(), int(s) if s.isdigit() else 0, s))
        if path.endswith(".conv") or (path.startswith("model.24.m.")):
            w = torch.from_numpy(np.asarray(sd[path + ".weight"])).half()
            m = torch.nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], bias=path + ".bias" in sd)
            m.weight = torch.nn.Parameter(w, requires_grad=False)
            if m.bias is not None:
                m.bias = torch.nn.Parameter(torch.from_numpy(np.asarray(sd[path + ".bias"])).half(), requires_grad=False)
            return m
        if path.endswith(".bn"):
            m = torch.nn.BatchNorm2d(int(np.asarray(sd[path + ".weight"]).shape[0]), eps=1e-3)
            for n in ("weight", "bias"):
                setattr(m, n, torch.nn.Parameter(torch.from_numpy(np.asarray(sd[f"{path}.{n}"])).half(), requires_grad=False))
            for n in ("running_mean", "running_var"):
                setattr(m, n, torch.from_numpy(np.asarray(sd[f"{path}.{n}"])).half())
            return m
        if kids == ["conv", "bn"] or kids == ["bn", "conv"] or set(kids) == {"conv", "bn"}:
            m = C["Conv"]()
            m.conv, m.bn, m.act = node(path + ".conv", keys), node(path + ".bn", keys), act()
            return m
        if path == "model.24":
            m = C[head]()
            m.m = torch.nn.ModuleList([node(f"model.24.m.{i}", keys) for i in range(3)])
            m.register_buffer("anchors", torch.from_numpy(np.asarray(sd["model.24.anchors"])).half())
            m.nc, m.no, m.nl, m.na = 0, 0, 3, 3
            return m
        if path.count(".") == 2 and path.endswith(".m"):
            return torch.nn.Sequential(*[node(f"{path}.{j}", keys) for j in kids])
        cls = {True: C["C3"], False: C[sppf]}["cv3" in kids] if path.count(".") == 1 else C["Bottleneck"]
        m = cls()
        for k in kids:
            setattr(m, k, node(f"{path}.{k}", keys))
        return m

    keys = list(sd)
    n_layers = 1 + max(int(k.split(".")[1]) for k in keys)
    seq = []
    for i in range(n_layers):
        if any(k.startswith(f"model.{i}.") for k in keys):
            seq.append(node(f"model.{i}", keys))
        else:   # Upsample / Concat: no parameters
            seq.append(torch.nn.Upsample(scale_factor=2.0, mode="nearest") if i in (11, 15) else C["Concat"]())
    top = C[model_cls]()
    top.model = torch.nn.Sequential(*seq)
    return top


def _save(path, obj, mods):
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        torch.save(obj, path)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert "models.yolo" not in sys.modules and "models.common" not in sys.modules


def _yaml(gd, gw, nc, **kw):
    y = {"nc": nc, "depth_multiple": gd, "width_multiple": gw,
         "anchors": [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]],
         "backbone": [[-1, 1, "Conv", [64, 6, 2, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C3", [128]], [-1, 1, "SPPF", [1024, 5]]],
         "head": [[[17, 20, 23], 1, "Detect", ["nc", "anchors"]]]}
    y.update(kw)
    return y


def _fp16_rounded(sd):
    return {k: np.asarray(v, np.float32).astype(np.float16).astype(np.float32) for k, v in sd.items()}


def _checkpoint(tmp_path, size="m", nc=6, where="ema", yaml_kw=None, tree_kw=None, name="ckpt.pt", names=None):
    from playaid_core_amd.yolov5 import P5_SIZES

    sd = synth.make_yolov5_state_dict(size, nc=nc)
    mods, C = _classes()
    m = _tree(sd, C, **(tree_kw or {}))
    m.yaml = _yaml(*P5_SIZES[size], nc, **(yaml_kw or {}))
    m.names = names if names is not None else NAMES80[:nc]
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    ckpt = {"epoch": -1, "best_fitness": None, "model": None, "ema": None, "updates": None, "optimizer": None,
            "opt": {"weights": "yolov5m.pt", "save_dir": "runs/train/exp"}, "git": None, "date": "2023-07-31T00:00:00"}
    ckpt[where] = m
    if where == "ema":
        ckpt["model"] = m
    p = os.path.join(tmp_path, name)
    _save(p, ckpt, mods)
    return p, sd


@pytest.mark.parametrize("where", ["model", "ema"])
def test_checkpoint_round_trip(tmp_path, where):
    from playaid_core_amd.yolov5_checkpoint import load_yolov5_checkpoint

    p, sd = _checkpoint(tmp_path, "m", 6, where)
    got, meta = load_yolov5_checkpoint(p)
    want = _fp16_rounded(sd)
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], v), k
    assert meta["nc"] == 6 and meta["names"] == NAMES80[:6]
    assert (meta["depth_multiple"], meta["width_multiple"]) == (0.67, 0.75)
    assert meta["anchors"][2] == [116, 90, 156, 198, 373, 326]
    assert meta["graph"]["widths"] == (48, 96, 192, 384, 768) and meta["graph"]["repeats"][6] == 6


def test_ema_is_preferred_over_model(tmp_path):
    from playaid_core_amd.yolov5_checkpoint import load_yolov5_checkpoint

    p, sd = _checkpoint(tmp_path, "n", 80, "ema")
    ck = torch.load(p, weights_only=False, pickle_module=_StubPickle)
    assert ck["ema"] is ck["model"]
    ck2 = dict(ck)
    other = synth.make_yolov5_state_dict("n", seed=99, nc=80)
    mods, C = _classes()
    ck2["model"] = _tree(other, C)
    ck2["ema"] = _tree(sd, C)
    ck2["ema"].yaml, ck2["ema"].names = _yaml(0.33, 0.25, 80), {i: n for i, n in enumerate(NAMES80)}
    q = os.path.join(tmp_path, "two.pt")
    _save(q, ck2, mods)
    got, meta = load_yolov5_checkpoint(q)
    assert np.array_equal(got["model.1.conv.weight"], _fp16_rounded(sd)["model.1.conv.weight"])
    assert meta["nc"] == 80 and meta["names"] == NAMES80


class _StubPickle:
    """An unpickler for the test's own look inside a checkpoint: every checkout class becomes a plain nn.Module."""

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            if module.startswith("models"):
                return type(name, (torch.nn.Module,), {})
            return super().find_class(module, name)

    __name__ = "stub"

    @staticmethod
    def load(f, **kw):
        return _StubPickle.Unpickler(f, **kw).load()


def test_bare_state_dict(tmp_path):
    from playaid_core_amd.yolov5_checkpoint import load_yolov5_checkpoint

    sd = synth.make_yolov5_state_dict("n", nc=3)
    p = os.path.join(tmp_path, "sd.pt")
    torch.save({k: torch.from_numpy(np.asarray(v)).half() for k, v in sd.items()}, p)
    got, meta = load_yolov5_checkpoint(p)
    assert all(np.array_equal(got[k], v) for k, v in _fp16_rounded(sd).items())
    assert meta["nc"] == 3 and meta["names"] is None and meta["depth_multiple"] is None
    assert meta["graph"]["widths"] == (16, 32, 64, 128, 256)


@pytest.mark.parametrize("case,match", [
    ("focus", "v5.0-or-older"),
    ("spp", "v5.0-or-older"),
    ("p6", "P6"),
    ("segment", "Segment"),
    ("classify", "classification"),
    ("nc81", "at most 80"),
    ("leaky", "SiLU"),
    ("leaky_module", "SiLU"),
    ("yaml_disagrees", "disagrees|give"),
])
def test_refusals_name_their_reason(tmp_path, case, match):
    from playaid_core_amd.yolov5_checkpoint import CheckpointError, load_yolov5_checkpoint

    kw = {}
    if case == "focus":
        kw = dict(yaml_kw={"backbone": [[-1, 1, "Focus", [64, 3]]]})
    elif case == "spp":
        kw = dict(tree_kw={"sppf": "SPP"})
    elif case == "p6":
        kw = dict(yaml_kw={"anchors": [[19, 27, 44, 40, 38, 94]] * 4})
    elif case == "segment":
        kw = dict(tree_kw={"head": "Segment"})
    elif case == "classify":
        kw = dict(tree_kw={"model_cls": "ClassificationModel"})
    elif case == "leaky":
        kw = dict(yaml_kw={"activation": "nn.LeakyReLU(0.1)"})
    elif case == "leaky_module":
        kw = dict(tree_kw={"act": torch.nn.LeakyReLU})
    elif case == "yaml_disagrees":
        kw = dict(yaml_kw={"width_multiple": 0.5})
    if case == "nc81":
        p, _ = _checkpoint(tmp_path, "n", 81, names=[str(i) for i in range(81)])
    else:
        p, _ = _checkpoint(tmp_path, "n", 6, **kw)
    with pytest.raises(CheckpointError, match=match):
        load_yolov5_checkpoint(p)


def test_anchor_free_ultralytics_model_is_refused(tmp_path):
    from playaid_core_amd.yolov5_checkpoint import CheckpointError, load_yolov5_checkpoint

    mod = types.ModuleType("ultralytics.nn.tasks")
    cls = type("DetectionModel", (torch.nn.Module,), {"__module__": "ultralytics.nn.tasks", "__qualname__": "DetectionModel"})
    mod.DetectionModel = cls
    p = os.path.join(tmp_path, "u.pt")
    _save(p, {"model": cls()}, {"ultralytics": types.ModuleType("ultralytics"), "ultralytics.nn": types.ModuleType("ultralytics.nn"),
                                "ultralytics.nn.tasks": mod})
    with pytest.raises(CheckpointError, match="anchor-free"):
        load_yolov5_checkpoint(p)


class _Boom:
    def __reduce__(self):
        return (os.system, ("echo pwned > " + _Boom.target,))


def test_a_pickle_naming_os_system_is_refused_and_runs_nothing(tmp_path):
    from playaid_core_amd.yolov5_checkpoint import CheckpointError, load_yolov5_checkpoint

    _Boom.target = os.path.join(tmp_path, "ran")
    p = os.path.join(tmp_path, "evil.pt")
    torch.save({"model": {"model.0.conv.weight": torch.zeros(1)}, "x": _Boom()}, p)
    with pytest.raises(CheckpointError, match="refused global .*system"):
        load_yolov5_checkpoint(p)
    assert not os.path.exists(_Boom.target)


@pytest.mark.gpu
def test_detector_from_a_checkpoint_is_the_detector_from_its_state_dict(tmp_path):
    """load_from_checkpoint on a synthetic fp16 m checkpoint: the same pred, bit for bit, as the fp16-rounded state dict."""
    from playaid_core_amd.yolov5 import YoloV5Detector

    p, sd = _checkpoint(tmp_path, "m", 6, "ema")
    frames = synth.make_frames(2, 720, 1280, seed=13)
    for dtype in ("f32", "bf16"):
        a = YoloV5Detector.load_from_checkpoint(p, net_hw=(128, 224), max_images=2, compute_dtype=dtype)
        b = YoloV5Detector(_fp16_rounded(sd), 6, (128, 224), max_images=2, compute_dtype=dtype)
        try:
            pa, pb = a(frames), b(frames)
            torch.cuda.synchronize()
            assert a.names == NAMES80[:6] and a.meta["graph"]["repeats"][2] == 2
            assert torch.equal(pa, pb), dtype
        finally:
            a.close()
            b.close()

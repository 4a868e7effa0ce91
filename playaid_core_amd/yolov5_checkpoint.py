"""Load an ultralytics YOLOv5 ``.pt`` checkpoint without the YOLOv5 checkout (``YoloV5Detector.load_from_checkpoint``).

A YOLOv5 training checkpoint is a dict whose ``ema`` (preferred) or ``model`` entry is the whole pickled
``models.yolo.DetectionModel`` (v7.0; ``models.yolo.Model`` in v6.x), usually fp16; unpickling it normally needs the
checkout's ``models`` and ``utils`` packages. Here ``torch.load`` runs with a restricted unpickler instead: every
``models.*`` / ``utils.*`` class becomes an inert ``nn.Module`` stand-in that only holds what was pickled (parameters,
buffers, sub-modules, attributes such as ``yaml`` and ``names``), and besides those only what such a file needs is allowed --
torch's tensor and storage rebuilds, dtypes and sizes, ``torch.nn`` modules, ``collections.OrderedDict``, ``set``, numpy
scalars and dtypes, ``pathlib`` paths. Any other global is refused before anything runs. A bare state dict saved with
``torch.save`` loads too. fp16 weights become fp32 exactly.
"""
from __future__ import annotations

import pickle
import types
from typing import Dict, Mapping, Tuple

import numpy as np
import torch

from .yolov5 import graph_of, p5_graph


class CheckpointError(ValueError):
    """A checkpoint this loader refuses (the message names the reason)."""


class _StandIn(torch.nn.Module):
    """An inert stand-in for a class of the YOLOv5 checkout: holds its pickled state, runs nothing."""

    _checkout_name = ""

    def forward(self, *args, **kwargs):
        raise RuntimeError(f"{self._checkout_name} is a stand-in of the YOLOv5 checkout's class; it does not run")


_OK_GLOBALS = {
    ("collections", "OrderedDict"),
    ("builtins", "set"),
    ("builtins", "frozenset"),
    ("__builtin__", "set"),         # (protocol 2 names them as Python 2 did)
    ("__builtin__", "frozenset"),
    ("torch", "Size"),
    ("torch", "device"),
    ("torch._utils", "_rebuild_tensor"),
    ("torch._utils", "_rebuild_tensor_v2"),
    ("torch._utils", "_rebuild_parameter"),
    ("torch._utils", "_rebuild_parameter_with_state"),
    ("numpy", "dtype"),
    ("numpy.core.multiarray", "scalar"),
    ("numpy._core.multiarray", "scalar"),
    ("pathlib", "Path"),
    ("pathlib", "PosixPath"),
    ("pathlib", "WindowsPath"),
    ("pathlib", "PurePosixPath"),
    ("pathlib", "PureWindowsPath"),
}


def _make_unpickler_module(seen: set):
    standins: Dict[Tuple[str, str], type] = {}

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            top = module.split(".")[0]
            if top == "ultralytics":
                raise CheckpointError(f"{module}.{name}: an ultralytics-package (anchor-free YOLOv5u / YOLOv8-style) model, not a "
                                      "YOLOv5 v6.0 / v7.0 checkpoint")
            if top in ("models", "utils"):
                seen.add(name)
                key = (module, name)
                if key not in standins:
                    standins[key] = type(name, (_StandIn,), {"_checkout_name": f"{module}.{name}", "__module__": __name__})
                return standins[key]
            if (module, name) in _OK_GLOBALS:
                return super().find_class(module, name)
            if module == "torch" and isinstance(getattr(torch, name, None), torch.dtype):
                return getattr(torch, name)
            if module == "numpy.dtypes" and name.endswith("DType"):
                return super().find_class(module, name)
            if module.startswith("torch.nn.modules."):
                cls = super().find_class(module, name)
                if isinstance(cls, type) and issubclass(cls, torch.nn.Module):
                    return cls
            raise CheckpointError(f"refused global {module}.{name}: not something a YOLOv5 checkpoint holds")

    def load(f, **kw):
        return Unpickler(f, **kw).load()

    mod = types.ModuleType("yolov5_checkpoint_unpickler")
    mod.Unpickler = Unpickler
    mod.load = load
    return mod


def _yaml_meta(model, yaml) -> Dict[str, object]:
    meta = {"nc": None, "names": None, "depth_multiple": None, "width_multiple": None, "anchors": None}
    if isinstance(yaml, dict):
        meta.update(nc=yaml.get("nc"), depth_multiple=yaml.get("depth_multiple"), width_multiple=yaml.get("width_multiple"),
                    anchors=yaml.get("anchors"))
    names = getattr(model, "names", None) if model is not None else None
    if isinstance(names, dict):
        names = [names[k] for k in sorted(names)]
    meta["names"] = list(names) if names is not None else None
    return meta


def _refuse_graph(seen: set, yaml) -> None:
    if seen & {"Focus", "SPP"}:
        raise CheckpointError(f"a v5.0-or-older model ({', '.join(sorted(seen & {'Focus', 'SPP'}))}): only the v6.0 / v7.0 P5 graph "
                              "(6x6 stem, SPPF) is supported")
    if seen & {"Segment", "Proto"}:
        raise CheckpointError("a Segment head (instance segmentation model): only Detect is supported")
    if seen & {"ClassificationModel", "Classify"}:
        raise CheckpointError("a classification model: only Detect is supported")
    if not isinstance(yaml, dict):
        return
    layers = list(yaml.get("backbone", []) or []) + list(yaml.get("head", []) or [])
    mods = {str(l[2]) for l in layers if isinstance(l, (list, tuple)) and len(l) > 2}
    if mods & {"Focus", "SPP"}:
        raise CheckpointError("a v5.0-or-older model (Focus / SPP in its yaml): only the v6.0 / v7.0 P5 graph is supported")
    if "Segment" in mods:
        raise CheckpointError("a Segment head (instance segmentation model): only Detect is supported")
    anchors = yaml.get("anchors")
    if isinstance(anchors, (list, tuple)) and len(anchors) != 3:
        raise CheckpointError(f"{len(anchors)} Detect scales (a P6 model has four): only P5 models with three are supported")
    if isinstance(anchors, int):
        raise CheckpointError("auto-generated anchors (anchors: int): only explicit P5 anchors are supported")
    act = yaml.get("activation")
    if act is not None and str(act).replace(" ", "") not in ("nn.SiLU()", "SiLU()", "nn.SiLU"):
        raise CheckpointError(f"activation {act!r}: the device network computes SiLU only")


def _refuse_activations(model) -> None:
    for name, m in model.named_modules():
        act = getattr(m, "act", None)
        if isinstance(m, _StandIn) and isinstance(act, torch.nn.Module) and not isinstance(act, (torch.nn.SiLU, torch.nn.Identity)):
            raise CheckpointError(f"{name}.act is {type(act).__name__}: the device network computes SiLU only")


def load_yolov5_checkpoint(path) -> Tuple[Dict[str, np.ndarray], Dict[str, object]]:
    """An ultralytics YOLOv5 v6.x / v7.0 ``.pt`` (or a bare state dict saved with ``torch.save``) -> (state dict of float32
    numpy arrays in the checkpoint's key layout, meta). meta: ``nc``, ``names`` (None for a bare state dict),
    ``depth_multiple``, ``width_multiple`` and ``anchors`` as the model's yaml states them (None where it has none), and
    ``graph``: the widths and bottlenecks per C3 block read from the shapes (``yolov5.graph_of``). Raises CheckpointError,
    naming the reason, for v5.0-and-older (Focus / SPP) models, P6 models, Segment and classification heads, anchor-free
    ultralytics-package models, nc > 80, a non-SiLU activation, a yaml that disagrees with the shapes, and any pickled global
    outside what such a file needs."""
    seen: set = set()
    try:
        ckpt = torch.load(path, map_location="cpu", pickle_module=_make_unpickler_module(seen), weights_only=False)
    except CheckpointError:
        raise
    except pickle.UnpicklingError as e:
        raise CheckpointError(f"{path}: {e}") from e
    model = None
    if isinstance(ckpt, torch.nn.Module):
        model = ckpt
    elif isinstance(ckpt, Mapping):
        for key in ("ema", "model"):
            if isinstance(ckpt.get(key), torch.nn.Module):
                model = ckpt[key]
                break
        if model is None and isinstance(ckpt.get("model"), Mapping):
            ckpt = ckpt["model"]
    yaml = getattr(model, "yaml", None) if model is not None else None
    _refuse_graph(seen, yaml)
    if model is not None:
        _refuse_activations(model)
        raw = model.state_dict()
    elif isinstance(ckpt, Mapping) and all(isinstance(v, torch.Tensor) for v in ckpt.values()):
        raw = ckpt
    else:
        raise CheckpointError(f"{path}: neither a YOLOv5 checkpoint (ema / model) nor a state dict")
    # (fp16 -> fp32 is exact; integer entries such as BatchNorm's num_batches_tracked are no weights and are left out)
    sd = {k: v.detach().to(torch.float32).numpy() for k, v in raw.items() if v.is_floating_point()}
    try:
        g = graph_of(sd)
    except (KeyError, ValueError) as e:
        raise CheckpointError(f"not a YOLOv5 v6.0 / v7.0 P5 detection model: {e}") from e
    meta = _yaml_meta(model, yaml)
    if meta["nc"] is not None and int(meta["nc"]) != g["nc"]:
        raise CheckpointError(f"the yaml's nc = {meta['nc']} disagrees with the Detect head's {g['nc']} classes")
    meta["nc"] = g["nc"]
    if g["nc"] > 80:
        raise CheckpointError(f"nc = {g['nc']}: the device NMS takes at most 80 classes")
    if meta["depth_multiple"] is not None and meta["width_multiple"] is not None:
        want = p5_graph(float(meta["depth_multiple"]), float(meta["width_multiple"]))
        if want["widths"] != g["widths"] or want["repeats"] != g["repeats"]:
            raise CheckpointError(f"the yaml's multiples ({meta['depth_multiple']}, {meta['width_multiple']}) give {want}, the "
                                  f"shapes say {g['widths']} / {g['repeats']}")
    if meta["names"] is not None and len(meta["names"]) != g["nc"]:
        raise CheckpointError(f"{len(meta['names'])} class names for {g['nc']} classes")
    meta["graph"] = {"widths": g["widths"], "repeats": g["repeats"]}
    return sd, meta

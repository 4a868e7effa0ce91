"""``ResnetTransformerDetector`` -- the reference's second alternative model.

Mirror of ``playaid/models/resnet_transformer_detector.py:26-141`` for inference: a timm ``resnet50`` without
classifier (2048 pooled features per frame, ``:37``), ``Linear(2048, 247)`` (``:41``), the 9-value time encoding of the
frame's position in the window appended (``:18-23,43-49,77-80``) -> 256, three post-norm
``nn.TransformerEncoderLayer(d_model=256, nhead=8)`` (``:53-60``), ``Linear(256, A)`` (``:65``), ``log_softmax`` over
the actions (``:141``); ``model(x)`` with ``x: float32[B,S,3,C,C]`` -> ``float32[B,S,A]``, C = ``crop_size`` (128 by default; the
reference's own driver for this model cuts 256 x 256 crops). As with the LSTM model the
encoder is built without ``batch_first``, so attention runs ACROSS THE WINDOWS of a call (dimension 0) for each
frame slot; that is reproduced as is.

The ResNet-50 runs on the engine's fp32 convolution kernels through a layer table (``pa_convnet_*``,
``csrc/convnet.hip``): BatchNorm folded in fp64 here, 1x1 convolutions as GEMMs on the im2col engine, the stride-1
3x3 ones on the patch-resident kernel, the stem on ``stem_pool_kernel``. The encoder and the classifier run in
``csrc/transformer.hip`` (``pa_encoder_*``). No PyTorch fallback.

Scoring is mirrored (``validation_step`` / ``test_step``, ``:179-205``): this model's reference flattens its ``[B, S, A]`` output
and ``action_label`` to ``B * S`` rows and scores every one of them (not the centre label the CNN model scores) -- NLL loss and
multiclass top-1 accuracy, accumulated on the device (``metrics.EvalState``) with nothing read back per step;
``metrics(split)`` is the one read (``val_action_loss``, ``val_action_acc``, ... plus confusion matrix and mean confidence),
``reset_metrics(split)`` clears a split.

Training is mirrored for the encoder head with the ResNet-50 frozen (``freeze_encoder=True``; ``encoder_trainer.EncoderTrainer``,
csrc/encoder_train.hip): ``train()``, ``configure_optimizers()`` (the reference's ``torch.optim.Adam(lr=self.learning_rate)``,
``:207-209``), ``training_step`` (``:143-164``: NLL over every row against ``action_label`` flattened to ``B * S``, with the encoder
layers' dropout), ``state_dict()`` and ``save_checkpoint()``. ``model.resnet.*`` stays as loaded and runs on the inference kernels
with eval-mode BatchNorm; ``model.freq_encoding`` is a buffer and ``model.resnet_classifier.*`` (never used by the reference's
forward) passes through. The reference ignores ``freeze_encoder`` for this model and trains the ResNet-50 too: here it is the
explicit opt-in and the only form that trains. ``model(x)`` stays the inference path, without dropout, also while
``model.training`` is set. Not mirrored: training the ResNet-50 and its BatchNorm statistics, and the data hooks
(``:166-177, 211-260``).

``compute_dtype="bf16"`` (never the default) runs the ResNet-50 with bf16 storage and bf16 products: the stem on
``stem_pool_kernel``'s bf16 form, every convolution on the one-slice bf16 GEMM (``csrc/bgemm.hip``, split-K on the small maps),
the average pool summing bf16 in fp32; the pooled features and the encoder stay fp32. Rounding model: ``include/playaid_hip.h``
next to ``pa_convnet_create_dtype``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import EngineError, _ptr
from .metrics import SplitMetrics

HIDDEN_DIM, NUM_FREQ, NUM_HEADS, NUM_LAYERS, FF_DIM = 247, 4, 8, 3, 2048
D_MODEL = HIDDEN_DIM + 1 + 2 * NUM_FREQ
RESNET50_BLOCKS = (3, 4, 6, 3)
BN_EPS = 1e-5


def _np(v) -> np.ndarray:
    return v if isinstance(v, np.ndarray) else v.detach().cpu().numpy()


def resnet50_param_shapes() -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of a timm / torchvision ``resnet50`` without its classifier (bottleneck blocks [3, 4, 6, 3],
    stride on the 3x3 convolution), in module order."""
    out: List[Tuple[str, Tuple[int, ...]]] = []

    def bn(prefix, c):
        out.extend([(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,))])

    out.append(("conv1.weight", (64, 3, 7, 7)))
    bn("bn1", 64)
    cin = 64
    for li, (width, blocks) in enumerate(zip((64, 128, 256, 512), RESNET50_BLOCKS), start=1):
        for b in range(blocks):
            p = f"layer{li}.{b}"
            out.append((p + ".conv1.weight", (width, cin, 1, 1)))
            bn(p + ".bn1", width)
            out.append((p + ".conv2.weight", (width, width, 3, 3)))
            bn(p + ".bn2", width)
            out.append((p + ".conv3.weight", (4 * width, width, 1, 1)))
            bn(p + ".bn3", 4 * width)
            if b == 0:
                out.append((p + ".downsample.0.weight", (4 * width, cin, 1, 1)))
                bn(p + ".downsample.1", 4 * width)
            cin = 4 * width
    return out


def time_encoding(sequence_length: int) -> np.ndarray:
    """``time_encoding(torch.linspace(0, 1, S).reshape(-1, 1), 4)`` (``:18-23,43-49``) -> float32[S, 9]:
    x, then cos(pi x 2^i), sin(pi x 2^i) for i = 0..3, computed by torch in fp32 exactly as the reference does."""
    x = torch.linspace(0, 1, sequence_length).reshape(-1, 1)
    out = [x]
    for i in range(NUM_FREQ):
        out.extend((torch.cos(np.pi * x * (2 ** i)), torch.sin(np.pi * x * (2 ** i))))
    return torch.cat(out, dim=1).numpy().astype(np.float32)


class _Table:
    """Builds the ``pa_conv_desc`` table, the buffer plan and the folded weight blob of a ResNet-50."""

    def __init__(self):
        self.descs: List[dict] = []
        self.buf_floats: List[int] = []
        self.weights: List[np.ndarray] = []
        self.n_weights = 0

    def buffer(self, floats_per_crop: int) -> int:
        self.buf_floats.append(int(floats_per_crop))
        return len(self.buf_floats) - 1

    def put(self, a: np.ndarray) -> int:
        off = self.n_weights
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        pad = (-a.size) % 64  # keep every tensor 256-byte aligned
        self.weights.append(a)
        if pad:
            self.weights.append(np.zeros(pad, np.float32))
        self.n_weights += a.size + pad
        return off

    def fold(self, sd: Mapping, conv_key: str, bn_key: str):
        w = _np(sd[conv_key + ".weight"]).astype(np.float64)
        g, b = _np(sd[bn_key + ".weight"]).astype(np.float64), _np(sd[bn_key + ".bias"]).astype(np.float64)
        m, v = _np(sd[bn_key + ".running_mean"]).astype(np.float64), _np(sd[bn_key + ".running_var"]).astype(np.float64)
        scale = g / np.sqrt(v + BN_EPS)
        return w * scale[:, None, None, None], b - m * scale

    def conv(self, sd, conv_key, bn_key, cin, cout, k, stride, in_hw, in_buf, in_pad, out_buf, out_pad, res_buf, relu):
        w, bias = self.fold(sd, conv_key, bn_key)
        assert w.shape == (cout, cin, k, k), (conv_key, w.shape)
        self.descs.append(dict(kind=0, cin=cin, cout=cout, ksize=k, stride=stride, in_hw=in_hw, in_buf=in_buf, in_pad=in_pad,
                               out_buf=out_buf, out_pad=out_pad, res_buf=res_buf, relu=int(relu),
                               w_off=self.put(w.transpose(0, 2, 3, 1)), b_off=self.put(bias)))


def check_crop_size(crop_size) -> int:
    """The network input sizes the table's stem takes: multiples of 32 in 64..512 (the map is halved five times, and the
    sized stem kernel's limits, ``include/playaid_hip.h`` at ``pa_conv_desc``)."""
    c = int(crop_size)
    if c != crop_size or c % 32 != 0 or not 64 <= c <= 512:
        raise ValueError(f"crop_size must be a multiple of 32 in 64..512, got {crop_size!r}")
    return c


def build_resnet50_table(state_dict: Mapping, prefix: str = "model.resnet.", crop_size: int = 128):
    """-> (descs, buf_floats_per_crop, weights float32, feature_dim). Buffers: 0 stem output (bordered), 1 / 2 block
    outputs (ping-pong), 3 the 3x3 convolution's output, 4 the downsample branch, then one bordered buffer per
    (map size, width) a 3x3 convolution reads, last the pooled 2048-vector.

    ``crop_size``: the side of the square input. 128 gives the table this function always gave (stem row kind 1,
    ``stem_pool_kernel``); any other multiple of 32 in 64..512 a kind-3 stem row (``stem_pool_any.hip``) and maps of
    ``crop_size / 4, / 8, / 16, / 32`` pixels behind it."""
    crop_size = check_crop_size(crop_size)
    q = crop_size // 4   # the pooled stem map
    sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    for key, shape in resnet50_param_shapes():
        if key not in sd:
            raise KeyError(f"state_dict is missing {prefix}{key}")
        if tuple(_np(sd[key]).shape) != tuple(shape):
            raise ValueError(f"{prefix}{key}: expected shape {tuple(shape)}, got {tuple(_np(sd[key]).shape)}")
    t = _Table()
    stem_out = t.buffer((q + 2) * (q + 2) * 64)
    ping, pong = t.buffer(q * q * 256), t.buffer(q * q * 256)
    t2, ds = t.buffer(q * q * 64), t.buffer(q * q * 256)
    bordered: Dict[Tuple[int, int], int] = {}
    # stem: [64][7 ky][8 px][4 ch]
    w, bias = t.fold(sd, "conv1", "bn1")
    stem = np.zeros((64, 7, 8, 4), np.float64)
    stem[:, :, :7, :3] = w.transpose(0, 2, 3, 1)
    t.descs.append(dict(kind=1 if crop_size == 128 else 3, cin=3, cout=64, ksize=7, stride=2, in_hw=crop_size, in_buf=0, in_pad=3,
                        out_buf=stem_out, out_pad=1, res_buf=-1, relu=1, w_off=t.put(stem), b_off=t.put(bias)))
    cur, cur_pad, cin, hw = stem_out, 1, 64, q
    for li, (width, blocks) in enumerate(zip((64, 128, 256, 512), RESNET50_BLOCKS), start=1):
        for b in range(blocks):
            p = f"layer{li}.{b}"
            stride = 2 if (b == 0 and li > 1) else 1
            out_hw = hw // stride
            key = (hw, width)
            if key not in bordered:
                bordered[key] = t.buffer((hw + 2) * (hw + 2) * width)
            t1 = bordered[key]
            nxt = ping if cur != ping else pong
            t.conv(sd, p + ".conv1", p + ".bn1", cin, width, 1, 1, hw, cur, cur_pad, t1, 1, -1, True)
            t.conv(sd, p + ".conv2", p + ".bn2", width, width, 3, stride, hw, t1, 1, t2, 0, -1, True)
            if b == 0:
                t.conv(sd, p + ".downsample.0", p + ".downsample.1", cin, 4 * width, 1, stride, hw, cur, cur_pad, ds, 0, -1, False)
                res = ds
            else:
                res = cur
            t.conv(sd, p + ".conv3", p + ".bn3", width, 4 * width, 1, 1, out_hw, t2, 0, nxt, 0, res, True)
            cur, cur_pad, cin, hw = nxt, 0, 4 * width, out_hw
    pooled = t.buffer(cin)
    t.descs.append(dict(kind=2, cin=cin, cout=cin, ksize=1, stride=1, in_hw=hw, in_buf=cur, in_pad=0, out_buf=pooled, out_pad=0,
                        res_buf=-1, relu=0, w_off=0, b_off=0))
    return t.descs, t.buf_floats, np.concatenate(t.weights), cin


class ConvNet:
    """A layer table on the device (``pa_convnet_create`` / ``pa_convnet_forward``)."""

    def __init__(self, descs, buf_floats, weights: np.ndarray, out_floats: int, device: str = "cuda:0", max_crops: int = 64,
                 compute_dtype: str = "f32"):
        self._lib = _lib.load()
        if compute_dtype not in ("f32", "emulated_f32", "bf16"):
            raise ValueError("compute_dtype must be 'f32', 'emulated_f32' or 'bf16'")
        self.compute_dtype = compute_dtype
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no HIP device visible to PyTorch-ROCm; this path has no CPU fallback")
        self.device = torch.device(device)
        self.max_crops = max_crops
        self.out_floats = out_floats
        self.buf_floats = [int(b) for b in buf_floats]
        self.n_rows = len(descs)
        # side of the input crops: the table's stem row (kind 1: 128; kind 3: its in_hw)
        self.in_hw = next((int(d["in_hw"]) for d in descs if int(d["kind"]) == 3), 128)
        # element type of each buffer as stored (-1: the stem's input): under bf16 what a stem or convolution row writes is bf16,
        # what a pool writes fp32 (include/playaid_hip.h, PA_DTYPE_BF16)
        self.buf_dtype = {b: torch.float32 for b in range(-1, len(self.buf_floats))}
        if compute_dtype == "bf16":
            pooled = {int(d["out_buf"]) for d in descs if int(d["kind"]) == 2}
            self.buf_dtype = {b: torch.float32 if b in pooled else torch.bfloat16 for b in self.buf_dtype}
        arr = (_lib.pa_conv_desc * len(descs))()
        for i, d in enumerate(descs):
            for k, v in d.items():
                setattr(arr[i], k, int(v))
        bufs = (C.c_int64 * len(buf_floats))(*buf_floats)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        h = C.c_void_p()
        rc = self._lib.pa_convnet_create_dtype(self.device.index or 0, arr, len(descs), bufs, len(buf_floats),
                                               weights.ctypes.data_as(C.c_void_p), weights.size, max_crops, _lib.DTYPES[compute_dtype], C.byref(h))
        self._h = h
        if rc != 0:
            msg = self._lib.pa_convnet_last_error(h).decode() if h else "bad argument"
            self.close()
            raise EngineError(rc, msg)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pa_convnet_destroy(self._h)
            self._h = None

    def trace(self, x: torch.Tensor, last_row: int, buf: int) -> torch.Tensor:
        """Test aid (``pa_convnet_trace``): run what ``forward`` runs for x float32[n,3,S,S] (S = ``in_hw``; n <= max_crops, one group)
        through table row ``last_row`` (-1: the input conversion alone) and return the whole of buffer ``buf`` as stored:
        [max_crops * buf_floats[buf]] elements of ``buf_dtype[buf]`` (float32, or bfloat16 for what a bf16 table's stem and
        convolutions write) on the device (buf = -1: the stem input, [max_crops][S + 6][S + 6][4])."""
        xd = self._input(x)
        floats = self.max_crops * ((self.in_hw + 6) * (self.in_hw + 6) * 4 if buf < 0 else self.buf_floats[buf])
        out = torch.empty(floats, dtype=self.buf_dtype.get(buf, torch.float32), device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._lib.pa_convnet_trace(self._h, _ptr(xd), int(xd.shape[0]), last_row, buf, _ptr(out), out.numel() * out.element_size(), stream)
        if rc != 0:
            raise EngineError(rc, self._lib.pa_convnet_last_error(self._h).decode())
        return out

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.in_hw, self.in_hw):
            raise ValueError(f"expected [n,3,{self.in_hw},{self.in_hw}], got {tuple(x.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def layer_forms(self) -> List[str]:
        """The kernel form (``_lib.CN_FORM_NAMES``) each table row ran as in the last forward or trace."""
        forms = (C.c_int32 * self.n_rows)()
        rc = self._lib.pa_convnet_layer_forms(self._h, forms, self.n_rows)
        if rc != 0:
            raise EngineError(rc, "pa_convnet_layer_forms")
        return [_lib.CN_FORM_NAMES[f] for f in forms]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x float32[n,3,S,S] (S = ``in_hw``, the table's input size) -> float32[n, out_floats] on the device (groups of max_crops)."""
        xd = self._input(x)
        n = int(xd.shape[0])
        out = torch.empty((n, self.out_floats), dtype=torch.float32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        for c0 in range(0, n, self.max_crops):
            m = min(self.max_crops, n - c0)
            rc = self._lib.pa_convnet_forward(self._h, _ptr(xd[c0:]), m, _ptr(out[c0:]), self.out_floats, stream)
            if rc != 0:
                raise EngineError(rc, self._lib.pa_convnet_last_error(self._h).decode())
        return out


def pack_encoder_blob(state_dict: Mapping, num_actions: int, sequence_length: int) -> np.ndarray:
    """-> uint8 blob of ``pa_encoder_create`` (layout: include/playaid_hip.h)."""
    enc_dim = 1 + 2 * NUM_FREQ
    hdr = np.zeros(16, np.int32)
    hdr[:10] = [_lib.PA_ENCODER_MAGIC, 1, 2048, HIDDEN_DIM, sequence_length, enc_dim, NUM_HEADS, NUM_LAYERS, FF_DIM, num_actions]
    parts = [hdr.view(np.uint8)]

    def take(key, shape):
        if key not in state_dict:
            raise KeyError(f"state_dict is missing {key}")
        a = np.ascontiguousarray(_np(state_dict[key]), dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        parts.append(a.reshape(-1).view(np.uint8))

    take("model.resnet_ffn.weight", (HIDDEN_DIM, 2048))
    take("model.resnet_ffn.bias", (HIDDEN_DIM,))
    take("model.freq_encoding", (sequence_length, enc_dim))
    for layer in range(NUM_LAYERS):
        p = f"model.transformer.layers.{layer}."
        take(p + "self_attn.in_proj_weight", (3 * D_MODEL, D_MODEL))
        take(p + "self_attn.in_proj_bias", (3 * D_MODEL,))
        take(p + "self_attn.out_proj.weight", (D_MODEL, D_MODEL))
        take(p + "self_attn.out_proj.bias", (D_MODEL,))
        take(p + "linear1.weight", (FF_DIM, D_MODEL))
        take(p + "linear1.bias", (FF_DIM,))
        take(p + "linear2.weight", (D_MODEL, FF_DIM))
        take(p + "linear2.bias", (D_MODEL,))
        for nm in ("norm1", "norm2"):
            take(p + nm + ".weight", (D_MODEL,))
            take(p + nm + ".bias", (D_MODEL,))
    take("model.classifier.weight", (num_actions, D_MODEL))
    take("model.classifier.bias", (num_actions,))
    return np.concatenate(parts)


class ResnetTransformerDetector:
    def __init__(
        self,
        actions: List[str],
        batch_size: int = 64,
        sequence_length: int = 4,
        learning_rate: float = 2e-4,
        num_samples: int = 1024,
        freeze_encoder=False,
        state_dict: Optional[Mapping] = None,
        device: str = "cuda:0",
        max_rows: int = 448,
        crop_size: int = 128,
        **kwargs,
    ):
        if state_dict is None:
            raise ValueError("ResnetTransformerDetector needs weights: use load_from_checkpoint() or pass state_dict= "
                             "(timm's pretrained download is not available offline)")
        a = int(_np(state_dict["model.classifier.weight"]).shape[0])
        if a != len(actions):
            raise ValueError(f"checkpoint has {a} action logits but {len(actions)} actions were given")
        s = int(_np(state_dict["model.freq_encoding"]).shape[0])
        if s != sequence_length:
            raise ValueError(f"checkpoint encodes {s} frame slots but sequence_length={sequence_length}")
        self.actions = list(actions)
        self.num_actions = a
        self.sequence_length = s
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.num_samples = num_samples
        self.dataset_kwargs = kwargs
        self.freeze_encoder = bool(freeze_encoder)
        self.training = False
        self._trainer = None
        self._state_dict = {k: v for k, v in state_dict.items()}   # (model.resnet.* as loaded: state_dict() hands it back)
        self.max_rows = max_rows
        # (crop_size: the reference's dataset argument -- its driver feeds this model 256 x 256 crops; a multiple of 32 in 64..512)
        self.crop_size = check_crop_size(crop_size)
        if kwargs.get("compute_dtype", "f32") == "bf16" and self.crop_size != 128:
            raise ValueError("compute_dtype='bf16' runs 128 x 128 crops only (the stem of any size is fp32)")
        self._lib = _lib.load()
        descs, bufs, weights, feat_dim = build_resnet50_table(state_dict, crop_size=self.crop_size)
        # (compute_dtype: beyond the reference's arguments -- "emulated_f32" = pa_convnet_create_dtype(PA_DTYPE_EMULATED_F32), "bf16" =
        # PA_DTYPE_BF16: the ResNet-50 in bf16 on bgemm.hip, the encoder head fp32 as always; neither is the default, and bf16 is not
        # within the fp32 path's 1e-4 bar)
        self._net = ConvNet(descs, bufs, weights, feat_dim, device=device, max_crops=min(max_rows, 64),
                            compute_dtype=kwargs.get("compute_dtype", "f32"))
        self.device = self._net.device
        blob = pack_encoder_blob(state_dict, a, s)
        enc_dim = 1 + 2 * NUM_FREQ
        assert blob.nbytes == self._lib.pa_encoder_blob_bytes(2048, HIDDEN_DIM, s, enc_dim, NUM_LAYERS, FF_DIM, a)
        h = C.c_void_p()
        rc = self._lib.pa_encoder_create(self.device.index or 0, 2048, HIDDEN_DIM, s, enc_dim, NUM_HEADS, NUM_LAYERS, FF_DIM, a, max_rows,
                                         blob.ctypes.data_as(C.c_void_p), blob.nbytes, C.byref(h))
        self._h = h
        if rc != 0:
            msg = self._lib.pa_encoder_last_error(h).decode() if h else "bad argument"
            self.close()
            raise EngineError(rc, msg)

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, map_location=None, **kwargs):
        """Lightning ``.ckpt`` (``state_dict`` + ``hyper_parameters``; keyword arguments override the saved ones,
        ``action_detector.py:55``)."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        if "state_dict" not in ckpt:
            raise KeyError(f"{checkpoint_path} has no 'state_dict' (not a Lightning checkpoint)")
        hparams = dict(ckpt.get("hyper_parameters", {}) or {})
        hparams.update(kwargs)
        return cls(state_dict=ckpt["state_dict"], **hparams)

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode and not self.freeze_encoder:
            raise NotImplementedError("only the encoder head trains: build the model with freeze_encoder=True")
        self.training = bool(mode)
        return self

    # -- training (resnet_transformer_detector.py:143-164, 207-209; the ResNet-50 frozen) -------------
    def configure_optimizers(self):
        """The reference's ``torch.optim.Adam(self.parameters(), lr=self.learning_rate)`` for what trains here: the one
        ``EncoderTrainer`` on this model's handle (made once; it owns the Adam moments and the running epoch statistics).
        ``dropout=`` and ``seed=`` among the model's keyword arguments are the trainer's (0.1 and 0 by default)."""
        if not self.freeze_encoder:
            raise NotImplementedError("only the encoder head trains: build the model with freeze_encoder=True")
        if self._trainer is None:
            from .encoder_trainer import EncoderTrainer

            self._trainer = EncoderTrainer(self, lr=self.learning_rate, dropout=self.dataset_kwargs.get("dropout", 0.1),
                                           seed=self.dataset_kwargs.get("seed", 0))
        return self._trainer

    def training_step(self, batch, batch_idx):
        """``batch = (input [B,S,3,C,C], char_label, action_label [B,S], ...)``: the ResNet-50 features of every frame, then one
        ``pa_encoder_train_step`` with ``seq_len = B`` windows of ``batch = S`` slots and ``action_label.view(B * S)`` (``-100`` =
        no ground truth). -> the loss before the update, a 0-dim float32 device tensor; nothing waits."""
        if not self.training:
            raise RuntimeError("training_step in eval mode: call train() first")
        input, action_label = batch[0], batch[2]
        c = self.crop_size
        if input.dim() != 5 or tuple(input.shape[2:]) != (3, c, c) or input.shape[1] != self.sequence_length:
            raise ValueError(f"expected [B,{self.sequence_length},3,{c},{c}], got {tuple(input.shape)}")
        b, s = int(input.shape[0]), int(input.shape[1])
        if b * s > self.max_rows:
            raise ValueError(f"{b} x {s} rows exceed max_rows={self.max_rows}")
        trainer = self.configure_optimizers()
        feats = self._net.forward(input.reshape(b * s, 3, c, c))
        labels = action_label.reshape(b * s) if isinstance(action_label, torch.Tensor) else np.asarray(action_label).reshape(b * s)
        stats = trainer.step(feats, b, s, labels)
        return trainer.loss_of(stats)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The key set the model was built from: ``model.resnet.*``, ``model.freq_encoding`` (and anything else it carried, such
        as ``model.resnet_classifier.*``) as loaded, the trained tensors as they are on the device now (CPU tensors; waits for
        the read when a trainer exists)."""
        out = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v))) for k, v in self._state_dict.items()}
        if self._trainer is not None:
            for k, v in self._trainer.read("weights").items():
                out[k] = v.cpu()
        return out

    def save_checkpoint(self, path: str):
        """A Lightning-shaped ``.ckpt`` (``state_dict`` + ``hyper_parameters``) that ``load_from_checkpoint`` reads back."""
        hparams = dict(actions=list(self.actions), batch_size=self.batch_size, sequence_length=self.sequence_length,
                       learning_rate=self.learning_rate, num_samples=self.num_samples, freeze_encoder=self.freeze_encoder,
                       crop_size=self.crop_size)
        hparams.update(self.dataset_kwargs)
        torch.save({"state_dict": self.state_dict(), "hyper_parameters": hparams}, path)

    def close(self):
        if getattr(self, "_trainer", None) is not None:
            self._trainer.close()   # (before the handle whose weights it borrows)
            self._trainer = None
        if getattr(self, "_h", None):
            self._lib.pa_encoder_destroy(self._h)
            self._h = None
        if getattr(self, "_metrics", None) is not None:
            self._metrics.close()
            self._metrics = None
        if getattr(self, "_net", None) is not None:
            self._net.close()
            self._net = None

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        """frames [batch_size, frames_per_sequence, channel, height, width] -> log-probabilities [batch, frames, A]."""
        c = self.crop_size
        if frames.dim() != 5 or tuple(frames.shape[2:]) != (3, c, c) or frames.shape[1] != self.sequence_length:
            raise ValueError(f"expected [B,{self.sequence_length},3,{c},{c}], got {tuple(frames.shape)}")
        b, s = int(frames.shape[0]), int(frames.shape[1])
        if b * s > self.max_rows:
            raise ValueError(f"{b} x {s} rows exceed max_rows={self.max_rows}")
        feats = self._net.forward(frames.reshape(b * s, 3, c, c))
        out = torch.empty((b, s, self.num_actions), dtype=torch.float32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._lib.pa_encoder_forward(self._h, _ptr(feats), feats.shape[1], b, s, _ptr(out), stream)
        if rc != 0:
            raise EngineError(rc, self._lib.pa_encoder_last_error(self._h).decode())
        return out if frames.is_cuda else out.cpu()

    __call__ = forward

    # -- scoring (resnet_transformer_detector.py:179-205) -----------------------------
    def _split_metrics(self) -> SplitMetrics:
        if getattr(self, "_metrics", None) is None:
            self._metrics = SplitMetrics(self.num_actions, self.device)
        return self._metrics

    def _score(self, split: str, batch):
        input, char_label, action_label, _ = batch
        logp = self.forward(input.to(self.device))  # a device input: the rows stay on the device, nothing waits
        self._split_metrics().step(split, logp.reshape(-1, self.num_actions), action_label.reshape(-1))  # "b s f -> (b s) f"

    def validation_step(self, batch, batch_idx):
        self._score("val", batch)

    def test_step(self, batch, batch_idx):
        self._score("test", batch)

    def metrics(self, split: str = "val"):
        """The epoch's figures so far (``metrics.finish``) plus ``<split>_action_loss`` / ``<split>_action_acc``; waits."""
        return self._split_metrics().metrics(split)

    def reset_metrics(self, split: str = None):
        self._split_metrics().reset(split)

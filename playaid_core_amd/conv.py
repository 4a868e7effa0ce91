"""One convolution + bias + activation (+ residual) on the persistent implicit-GEMM kernels (``pa_conv2d``).

``compute_dtype="f32"`` runs ``csrc/pigemm.hip`` (the exact fp32 matrix instruction), ``"emulated_f32"`` runs
``csrc/psgemm.hip``: fp32 in, fp32 out, fp32-accurate sums, the products as six bf16 matrix instructions per fp32 product
(three bf16 slices per operand). These are the kernels the detection network's 1x1 / stride-2 layers
(``playaid/ai_runner.py:191-224``: YOLOv5s) and, under ``emulated_f32``, every 3x3 convolution of the ResNet-18
(``playaid/models/cnn_action_detector.py:16,32``) run on inside the library; this module exposes them as a single-layer
operator for parity tests and measurements. No CPU fallback: it needs the HIP library and a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def pack_weights(w_oihw: np.ndarray, compute_dtype: str = "emulated_f32", has_residual: bool = False) -> np.ndarray:
    """[cout, cin, k, k] fp32 (BatchNorm folded) -> the bytes the kernel of ``compute_dtype`` reads (uint8, host)."""
    lib = _lib.load()
    w = np.ascontiguousarray(np.asarray(w_oihw, dtype=np.float32).transpose(0, 2, 3, 1))   # [cout][ky][kx][cin]
    cout, k, _, cin = w.shape
    dt = _lib.DTYPES[compute_dtype]
    nbytes = lib.pa_conv_weight_bytes(cin, cout, k, dt, int(has_residual))
    if nbytes == 0:
        raise ValueError("cin and cout must be multiples of 32, the kernel 1x1 or 3x3, the dtype 'f32' or 'emulated_f32'")
    out = np.empty(nbytes, dtype=np.uint8)
    rc = lib.pa_conv_pack_weights(w.ctypes.data_as(C.c_void_p), cin, cout, k, dt, int(has_residual), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(f"pa_conv_pack_weights: status {rc}")
    return out


def conv2d(x_pad: torch.Tensor, w_packed: torch.Tensor, cin: int, cout: int, ksize: int, stride: int = 1, in_pad: int = None, bias=None,
           residual=None, out=None, out_pad: int = 0, act: int = 0, res_after: bool = False, out_px_stride: int = None,
           compute_dtype: str = "emulated_f32") -> torch.Tensor:
    """x_pad float32[n, H + 2 in_pad, W + 2 in_pad, C >= cin] (device, zero border) -> out float32[n, H / stride + 2 out_pad,
    W / stride + 2 out_pad, C' >= cout] (interior written). ``w_packed``: ``pack_weights`` of the same dtype (and the same
    ``has_residual``), on the device. Enqueues on the current stream."""
    lib = _lib.load()
    if x_pad.dtype != torch.float32 or not x_pad.is_cuda or not x_pad.is_contiguous() or x_pad.dim() != 4:
        raise ValueError("x_pad: contiguous float32[n, H + 2 pad, W + 2 pad, C] on the device")
    in_pad = (ksize - 1) // 2 if in_pad is None else in_pad
    n, hp, wp, cs = x_pad.shape
    h, w = hp - 2 * in_pad, wp - 2 * in_pad
    oh, ow = h // stride, w // stride
    ops = out_px_stride or cout
    if out is None:
        out = torch.zeros((n, oh + 2 * out_pad, ow + 2 * out_pad, ops), dtype=torch.float32, device=x_pad.device)
    ptr = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else C.c_void_p(0)
    stream = C.c_void_p(torch.cuda.current_stream(x_pad.device).cuda_stream)
    rc = lib.pa_conv2d(ptr(x_pad), ptr(w_packed), ptr(bias), ptr(residual), ptr(out), n, h, w, cin, cout, ksize, stride, in_pad, cs, out.shape[3],
                       out_pad, int(act), int(bool(res_after)), _lib.DTYPES[compute_dtype], stream)
    if rc:
        raise ValueError(f"pa_conv2d: status {rc}")
    return out


def conv2d_branch(x_pad: torch.Tensor, w: torch.Tensor, w2: torch.Tensor, cin: int, cout: int, bias=None, out=None, out2=None, out_pad: int = 0,
                  act: int = 0, in_pad: int = 1, ksize: int = 3, stride: int = 2, compute_dtype: str = "f32"):
    """A ResNet block's 3x3 stride-2 opener and its 1x1 stride-2 downsample branch in one launch (``pa_conv2d_branch``,
    ``csrc/pigemm.hip``): x_pad float32[n, H + 2 in_pad, W + 2 in_pad, cin] -> (out, out2), both float32[n, H / 2 + 2 out_pad,
    W / 2 + 2 out_pad, C' >= cout]; ``out`` = act(conv3x3(x) + bias), ``out2`` = conv1x1(x) with ``w2`` float32[cout, cin] on the
    device, no bias, no activation. ``w``: ``pack_weights(..., "f32")`` on the device. The library refuses anything but ksize 3,
    stride 2, whole pixels (C == cin) and the exact dtype; ``ksize`` and ``stride`` are passed through as given (the C call has
    ``pa_conv2d``'s argument list) so that a caller sees that refusal rather than a silently corrected call."""
    lib = _lib.load()
    if x_pad.dtype != torch.float32 or not x_pad.is_cuda or not x_pad.is_contiguous() or x_pad.dim() != 4:
        raise ValueError("x_pad: contiguous float32[n, H + 2 pad, W + 2 pad, C] on the device")
    n, hp, wp, cs = x_pad.shape
    h, wd = hp - 2 * in_pad, wp - 2 * in_pad
    oh, ow = h // stride, wd // stride
    mk = lambda: torch.zeros((n, oh + 2 * out_pad, ow + 2 * out_pad, cout), dtype=torch.float32, device=x_pad.device)
    out = mk() if out is None else out
    out2 = mk() if out2 is None else out2
    if out2.shape != out.shape:
        raise ValueError("out2 is addressed like out: same shape")
    ptr = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else C.c_void_p(0)
    stream = C.c_void_p(torch.cuda.current_stream(x_pad.device).cuda_stream)
    rc = lib.pa_conv2d_branch(ptr(x_pad), ptr(w), ptr(bias), C.c_void_p(0), ptr(out), ptr(w2), ptr(out2), n, h, wd, cin, cout, ksize, stride, in_pad, cs,
                              out.shape[3], out_pad, int(act), 0, _lib.DTYPES[compute_dtype], stream)
    if rc:
        raise ValueError(f"pa_conv2d_branch: status {rc}")
    return out, out2


def stem_int_pack_weights(w_oihw: np.ndarray) -> np.ndarray:
    """BatchNorm-folded stem weights [64, 3, 7, 7] fp32 -> the three bf16 slices uint16[3, 64, 224] (host) ``stem_int`` reads:
    ``w = s0 + s1 + s2`` exactly (``pa_stem_int_pack_weights``)."""
    lib = _lib.load()
    w = np.ascontiguousarray(np.asarray(w_oihw, dtype=np.float32).transpose(0, 2, 3, 1))   # [cout][ky][kx][cin]
    if w.shape != (64, 7, 7, 3):
        raise ValueError("w_oihw: [64, 3, 7, 7]")
    out = np.empty((3, 64, 224), dtype=np.uint16)
    rc = lib.pa_stem_int_pack_weights(w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError(f"pa_stem_int_pack_weights: status {rc}")
    return out


def stem_int(crops_u8: torch.Tensor, w_slices: torch.Tensor, bias: torch.Tensor, packed: torch.Tensor = None, out: torch.Tensor = None):
    """The ResNet-18 stem + ReLU + max-pool on integer pixels (``pa_stem_int``, ``csrc/stem_pool.hip``): crops_u8 uint8[n, 128, 128, 3]
    (device) -> (out float32[n, 34, 34, 64] with a zero border of one pixel, packed bf16[n, 134, 134, 4]: the pixel integers the
    stem multiplied, zero border of three pixels, zero fourth channel). ``w_slices``: ``stem_int_pack_weights`` on the device;
    ``packed`` / ``out``: buffers of an earlier call (their borders are never written). Enqueues on the current stream."""
    lib = _lib.load()
    if crops_u8.dtype != torch.uint8 or not crops_u8.is_cuda or not crops_u8.is_contiguous() or crops_u8.shape[1:] != (128, 128, 3):
        raise ValueError("crops_u8: contiguous uint8[n, 128, 128, 3] on the device")
    n = crops_u8.shape[0]
    if packed is None:
        packed = torch.zeros((n, 134, 134, 4), dtype=torch.bfloat16, device=crops_u8.device)
    if out is None:
        out = torch.zeros((n, 34, 34, 64), dtype=torch.float32, device=crops_u8.device)
    ptr = lambda t_: C.c_void_p(t_.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(crops_u8.device).cuda_stream)
    rc = lib.pa_stem_int(ptr(crops_u8), ptr(w_slices), ptr(bias), ptr(packed), ptr(out), n, stream)
    if rc:
        raise ValueError(f"pa_stem_int: status {rc}")
    return out, packed

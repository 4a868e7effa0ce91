"""Baseline JPEG files of mixed sizes -> packed crop images in HBM (the read side of rows a2 / a3 of SURVEY.md section 8).

The reference returns from ``run_yolo`` at once when ``crops/`` exists and reads every cached crop back with ``cv2.imread``
(``playaid/ai_runner.py:191-194, 445-446``). ``JpegDecoder`` does that read on the device (``pa_jpegdec_decode``,
``csrc/jpegdec.hip``): the files of a cache directory -- ``save_one_box`` crops of any size (4:4:4) and the repaired gaps'
128 x 128 4:2:0 files side by side -- go in one call straight into the packed layout ``pa_backbone_crop_images`` /
``pa_runner_inputs`` consume, pixel for pixel what libjpeg-turbo behind ``PIL.Image.open`` / ``cv2.imread`` decodes.

There is no CPU fallback: decoding needs the HIP library and a GPU (``HipLibraryError`` otherwise). ``plan`` is host
arithmetic on the files' marker segments and needs no device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

ERR_SYNC = 8   # status bit: the decoder states had not settled in the enqueued verify passes (decode again, exactly)


class JpegDecodeError(ValueError):
    """A file that does not decode; ``index`` is its place in the list handed in."""

    def __init__(self, index: int, msg: str):
        super().__init__(msg)
        self.index = int(index)


def blocks_bound(height: int, width: int) -> int:
    """An upper bound of an image's 8x8 blocks for any sampling the decoder takes (three full components, 16-pixel MCUs)."""
    return 3 * (2 * (-(-height // 16))) * (2 * (-(-width // 16)))


def _concat(blobs: Sequence[Optional[bytes]]):
    """-> (uint8 array of all files back to back, int64[n, 2] spans; None / b"" = an empty span)."""
    spans = np.zeros((len(blobs), 2), np.int64)
    off = 0
    for i, b in enumerate(blobs):
        nb = len(b) if b else 0
        spans[i] = (off, off + nb)
        off += nb
    data = np.frombuffer(b"".join(b for b in blobs if b), dtype=np.uint8) if off else np.zeros(1, np.uint8)
    return data, spans


def plan(blobs: Sequence[Optional[bytes]]):
    """``pa_jpegdec_plan``: -> (desc int64[n, 2] = byte offset, ``width << 32 | height``; images_bytes; blocks). Raises
    ``ValueError`` naming the index of a file the decoder does not take."""
    from . import _lib

    lib = _lib.load()
    n = len(blobs)
    if n == 0:
        return np.zeros((0, 2), np.int64), 0, 0
    data, spans = _concat(blobs)
    desc = np.zeros((n, 2), np.int64)
    total, blocks = C.c_size_t(0), C.c_int64(0)
    why = C.create_string_buffer(256)
    rc = lib.pa_jpegdec_plan(data.ctypes.data_as(C.c_void_p), spans.ctypes.data_as(C.c_void_p), n, desc.ctypes.data_as(C.c_void_p),
                             C.byref(total), C.byref(blocks), why, 256)
    if rc != _lib.PA_OK:
        msg = why.value.decode() or lib.pa_status_string(rc).decode()
        idx = int(msg.split()[1].rstrip(":")) if msg.startswith("image ") else 0
        raise JpegDecodeError(idx, f"jpeg_decode.plan: {msg}")
    return desc, int(total.value), int(blocks.value)


class JpegDecoder:
    """``pa_jpegdec_create`` / ``pa_jpegdec_decode``: a handle owns the scratch of one call -- up to ``max_images`` files with
    ``max_blocks`` 8x8 blocks (all components, padded to whole MCUs) and ``max_bytes`` compressed bytes."""

    SYNC_ROUNDS = 16   # the handle's default number of verify passes per call

    def __init__(self, max_images: int, max_blocks: int, max_bytes: int, device: str = "cuda:0"):
        import torch

        from . import _lib

        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no HIP device visible to PyTorch-ROCm; JPEG decode has no CPU fallback")
        self.device = torch.device(device)
        self.max_images, self.max_blocks, self.max_bytes = int(max_images), int(max_blocks), max(int(max_bytes), 1024)
        self._h = C.c_void_p(0)
        self.sync_rounds = self.SYNC_ROUNDS
        torch.cuda.set_device(self.device)
        rc = self._lib.pa_jpegdec_create(self.device.index or 0, self.max_images, self.max_blocks, self.max_bytes, C.byref(self._h))
        if rc != _lib.PA_OK:
            msg = self._lib.pa_jpegdec_last_error(self._h).decode() if self._h else self._lib.pa_status_string(rc).decode()
            self.close()
            from .engine import EngineError

            raise EngineError(rc, msg)

    @classmethod
    def for_crops(cls, n: int, max_height: int, max_width: int, device: str = "cuda:0") -> "JpegDecoder":
        """A handle that takes ``n`` files of up to ``max_height`` x ``max_width`` per call (a file is taken to be no longer
        than its pixels: quality-95 4:4:4 noise stays below that)."""
        return cls(n, n * blocks_bound(max_height, max_width), n * (max_height * max_width * 3 + 1024), device=device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pa_jpegdec_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def plan(self, blobs):
        return plan(blobs)

    def set_sync_rounds(self, rounds: int):
        from . import _lib
        from .engine import EngineError

        rc = self._lib.pa_jpegdec_set_sync_rounds(self._h, int(rounds))
        if rc != _lib.PA_OK:
            raise EngineError(rc, "set_sync_rounds: 0 (exact) .. 16")
        self.sync_rounds = int(rounds)

    def decode_call(self, data: np.ndarray, spans: np.ndarray, images, desc, status, bgr: bool = True):
        """One ``pa_jpegdec_decode``: ``data`` uint8 host array, ``spans`` int64[n, 2]; ``images`` (uint8, its size is the
        capacity), ``desc`` int64[n, 2] and ``status`` int32[n] are device tensors. Only enqueues on the current stream;
        ``data`` must stay alive until the stream has passed the call."""
        import torch

        from . import _lib
        from .engine import EngineError

        n = spans.shape[0]
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._lib.pa_jpegdec_decode(self._h, data.ctypes.data_as(C.c_void_p), spans.ctypes.data_as(C.c_void_p), n, int(bool(bgr)),
                                         C.c_void_p(images.data_ptr()), images.numel(), C.c_void_p(desc.data_ptr()),
                                         C.c_void_p(status.data_ptr()), stream)
        if rc != _lib.PA_OK:
            raise EngineError(rc, self._lib.pa_jpegdec_last_error(self._h).decode())

    def decode_files(self, blobs: Sequence[Optional[bytes]], bgr: bool = True):
        """``blobs``: the files' bytes, None (or ``b""``) where there is none -> (``images`` packed uint8 device tensor,
        ``desc`` int64[n, 2] device tensor = byte offset, ``width << 32 | height`` (0 x 0 for an empty entry), ``status``
        int32[n] device tensor, all zero). A list that exceeds the handle goes in consecutive calls on one output buffer. An
        image whose decoder states had not settled (status bit 8) is decoded again in exact mode; ``ValueError`` names the
        index of an image with any status left, or of a file the decoder does not take."""
        import torch

        n = len(blobs)
        hdesc, total, _ = plan(blobs)
        images = torch.empty(total + 64, dtype=torch.uint8, device=self.device)
        desc = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return images, desc, status
        hh, ww = hdesc[:, 1] & 0xFFFFFFFF, hdesc[:, 1] >> 32
        nblk = 12 * (-(-hh // 16)) * (-(-ww // 16))
        nbytes = np.array([len(b) if b else 0 for b in blobs], np.int64)
        keep = []   # host buffers of the calls in flight
        i0 = 0
        while i0 < n:
            i1, blk, byt = i0, 0, 0
            while i1 < n and i1 - i0 < self.max_images and blk + nblk[i1] <= self.max_blocks and byt + nbytes[i1] <= self.max_bytes:
                blk += int(nblk[i1])
                byt += int(nbytes[i1])
                i1 += 1
            if i1 == i0:
                raise JpegDecodeError(i0, f"decode_files: image {i0} ({int(hh[i0])} x {int(ww[i0])}, {int(nbytes[i0])} bytes) exceeds the "
                                 f"decoder's max_blocks / max_bytes")
            data, spans = _concat(blobs[i0:i1])
            keep.append(data)
            off0 = int(hdesc[i0, 0])
            self.decode_call(data, spans, images[off0:total] if total > off0 else images[total:], desc[i0:i1], status[i0:i1], bgr)
            if off0:
                desc[i0:i1, 0] += off0
            i0 = i1
        torch.cuda.synchronize(self.device)
        keep.clear()
        st = status.cpu().numpy()
        again = np.nonzero(st & ERR_SYNC)[0]
        if len(again):
            before = self.sync_rounds
            self.set_sync_rounds(0)
            try:
                for i in again.tolist():
                    data, spans = _concat([blobs[i]])
                    off, nb = int(hdesc[i, 0]), (int(hh[i]) * int(ww[i]) * 3 + 15) & ~15
                    tmp = torch.empty(nb, dtype=torch.uint8, device=self.device)
                    d1 = torch.empty((1, 2), dtype=torch.int64, device=self.device)
                    self.decode_call(data, spans, tmp, d1, status[i:i + 1], bgr)
                    images[off:off + nb].copy_(tmp)
                    torch.cuda.synchronize(self.device)
            finally:
                self.set_sync_rounds(before)
            st = status.cpu().numpy()
        bad = np.nonzero(st)[0]
        if len(bad):
            raise JpegDecodeError(int(bad[0]), f"decode_files: image {int(bad[0])} does not decode (status {int(st[bad[0]])})")
        return images, desc, status

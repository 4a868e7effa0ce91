"""Baseline JPEG encode on the MI355X (rows a2 / a3 of SURVEY.md section 8): images in HBM -> complete JPEG files.

The reference keeps its detector's output as files -- ``crops/<Fighter>/<video>_<n>.jpg`` written by YOLOv5's
``--save-crop`` (``playaid/ai_runner.py:191-194, 208, 291-295``) -- and every crop its CNN sees has been written as a
JPEG and read back. ``JpegEncoder`` produces those files on the device (``pa_jpegenc_encode``, ``csrc/jpegenc.hip``), byte
for byte what libjpeg-turbo behind ``PIL.Image.save(format="JPEG", quality=q, subsampling=s)`` writes for the same
pixels; ``ai_cache.py`` lays them out as the reference's cache directory, ``video.write_frames_mjpeg`` as a clip.

There is no CPU fallback: encoding needs the HIP library and a GPU (``HipLibraryError`` otherwise). ``jpeg_header`` and
``file_bytes_bound`` are host arithmetic and need neither.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

HEADER_BYTES = 623
SUBSAMPLING_444, SUBSAMPLING_420 = 0, 2


def jpeg_header(height: int, width: int, quality: int = 95, subsampling: int = 0) -> bytes:
    """The 623 bytes in front of the entropy-coded data (SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS)."""
    from . import _lib
    from .engine import EngineError

    lib = _lib.load()
    buf = (C.c_uint8 * HEADER_BYTES)()
    n = C.c_int32(0)
    rc = lib.pa_jpeg_header(int(height), int(width), int(quality), int(subsampling), buf, HEADER_BYTES, C.byref(n))
    if rc != _lib.PA_OK:
        raise EngineError(rc, "jpeg_header: height / width 1..65535, quality 1..100, subsampling 0 (4:4:4) or 2 (4:2:0)")
    return bytes(buf[: n.value])


def file_bytes_bound(height: int, width: int, subsampling: int = 0) -> int:
    """An upper bound of the file length of an image of that size (``pa_jpeg_file_bytes_bound``)."""
    from . import _lib

    return int(_lib.load().pa_jpeg_file_bytes_bound(int(height), int(width), int(subsampling)))


def coded_blocks(height: int, width: int, subsampling: int = 0) -> int:
    """8x8 blocks in the scan of an image, all components, dummy blocks of half-empty 4:2:0 MCUs included."""
    if subsampling:
        return 6 * (-(-height // 16)) * (-(-width // 16))
    return 3 * (-(-height // 8)) * (-(-width // 8))


class JpegEncoder:
    """``pa_jpegenc_create`` / ``pa_jpegenc_encode``: a handle owns the scratch of one call -- ``max_blocks`` 8x8 blocks over
    all images of a call (``coded_blocks``) and ``scratch_bytes`` for their un-stuffed entropy-coded streams."""

    def __init__(self, max_images: int, max_blocks: int, scratch_bytes: int = 0, device: str = "cuda:0"):
        import torch

        from . import _lib

        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no HIP device visible to PyTorch-ROCm; JPEG encode has no CPU fallback")
        self.device = torch.device(device)
        self.max_images, self.max_blocks = int(max_images), int(max_blocks)
        # default: every block half as long as the entropy coder allows, which quality 100 noise does not reach
        self.scratch_bytes = int(scratch_bytes) or max(self.max_blocks * 104 + 64 * self.max_images, 4096)
        self._h = C.c_void_p(0)
        torch.cuda.set_device(self.device)
        rc = self._lib.pa_jpegenc_create(self.device.index or 0, self.max_images, self.max_blocks, self.scratch_bytes, C.byref(self._h))
        if rc != _lib.PA_OK:
            msg = self._lib.pa_jpegenc_last_error(self._h).decode() if self._h else self._lib.pa_status_string(rc).decode()
            self.close()
            from .engine import EngineError

            raise EngineError(rc, msg)

    @classmethod
    def for_frames(cls, n: int, height: int, width: int, subsampling: int = 2, device: str = "cuda:0") -> "JpegEncoder":
        """A handle that takes ``n`` images of up to ``height`` x ``width`` per call."""
        return cls(n, n * coded_blocks(height, width, subsampling), device=device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pa_jpegenc_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_images(self, images, desc, max_height: int, max_width: int, quality: int = 95, subsampling: int = 0,
                      bgr: bool = True, files=None, records=None):
        """Device in, device out. ``images``: packed uint8 device tensor, ``desc`` int64[n, 2] device tensor (byte offset,
        ``width << 32 | height``: ``pa_crop_image``, what ``Engine.save_one_box_crops`` returns); every image is at most
        ``max_height`` x ``max_width``. Enqueues on the current stream and returns (``files`` uint8 device tensor, ``records``
        int64[n, 2] device tensor: byte offset of a file in ``files``, its length in the low 32 bits -- 0 for an empty
        entry, -1 for an image that did not fit the handle's scratch or ``files``)."""
        import torch

        from . import _lib
        from .engine import EngineError

        if images.dtype != torch.uint8 or not images.is_cuda or not images.is_contiguous():
            raise ValueError("encode_images: images is a contiguous uint8 device tensor")
        if desc.dtype != torch.int64 or not desc.is_cuda or not desc.is_contiguous() or desc.ndim != 2 or desc.shape[1] != 2:
            raise ValueError("encode_images: desc is a contiguous int64[n, 2] device tensor")
        n = desc.shape[0]
        if files is None:
            files = torch.empty(n * (file_bytes_bound(max_height, max_width, subsampling) // 2 + 16), dtype=torch.uint8, device=self.device)
        elif files.dtype != torch.uint8 or not files.is_cuda or not files.is_contiguous():
            raise ValueError("encode_images: files is a contiguous uint8 device tensor (its size is the capacity)")
        if records is None:
            records = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        elif records.dtype != torch.int64 or not records.is_cuda or not records.is_contiguous() or records.numel() < 2 * n:
            raise ValueError(f"encode_images: records is a contiguous int64[{n}, 2] device tensor")
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._lib.pa_jpegenc_encode(self._h, C.c_void_p(images.data_ptr()), images.numel(), C.c_void_p(desc.data_ptr()), n,
                                         int(max_height), int(max_width), int(bool(bgr)), int(quality), int(subsampling),
                                         C.c_void_p(files.data_ptr()), files.numel(), C.c_void_p(records.data_ptr()), stream)
        if rc != _lib.PA_OK:
            raise EngineError(rc, self._lib.pa_jpegenc_last_error(self._h).decode())
        return files, records

    def overflows(self) -> int:
        """Images that did not fit since the last query (synchronises the current stream)."""
        import torch

        from . import _lib
        from .engine import EngineError

        n = C.c_int32(0)
        rc = self._lib.pa_jpegenc_overflows(self._h, C.byref(n), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != _lib.PA_OK:
            raise EngineError(rc, self._lib.pa_jpegenc_last_error(self._h).decode())
        return int(n.value)

    @staticmethod
    def unpack_files(files, records) -> List[bytes]:
        """(files, records) of ``encode_images`` -> one ``bytes`` per image (``b""`` for an empty entry, None for one that
        did not fit), with ONE device -> host copy of the used range."""
        rec = records.cpu().numpy()
        nbytes = rec[:, 1].astype(np.int32)
        ends = rec[:, 0] + np.maximum(nbytes, 0)
        used = int(ends.max()) if len(ends) else 0
        buf = files[:used].cpu().numpy()
        return [None if nb < 0 else buf[off: off + nb].tobytes() for off, nb in zip(rec[:, 0].tolist(), nbytes.tolist())]

    def encode_frames(self, frames, quality: int = 95, subsampling: int = 2, bgr: bool = True) -> List[bytes]:
        """Uniform frames uint8[n, H, W, 3] (device tensor or numpy array) -> the n JPEG files."""
        import torch

        fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        fd = fd.to(self.device).contiguous()
        if fd.ndim != 4 or fd.shape[3] != 3 or fd.dtype != torch.uint8:
            raise ValueError("encode_frames: frames are uint8[n, H, W, 3]")
        n, h, w, _ = fd.shape
        if n == 0:
            return []
        desc = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        desc[:, 0] = torch.arange(n, device=self.device, dtype=torch.int64) * (h * w * 3)
        desc[:, 1] = (w << 32) | h
        files, rec = self.encode_images(fd.reshape(-1), desc, h, w, quality=quality, subsampling=subsampling, bgr=bgr)
        out = self.unpack_files(files, rec)
        if any(f is None for f in out):
            self.overflows()
            raise ValueError("encode_frames: the frames do not fit the encoder's scratch (max_blocks / scratch_bytes)")
        return out

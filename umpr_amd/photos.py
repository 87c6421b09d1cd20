"""Item photos resized on the GPU (umpr_photo_resize_u8, csrc/photos.hip).

The host form of the loader (data.get_image) decodes, resizes and divides by 255 on the host and uploads a float32
[B, V, P, 3, dh, dw] tensor.  Here the host only decodes: ``decode_for_gpu`` keeps the source rows and columns the resize
taps read (at most 2*dh x 2*dw x 3 bytes, never more than the 3*dh*dw*4 bytes of the float photo) and the tap tables
data.resize_bilinear_u8 would use; ``RawPhotos`` packs a batch of them into one uint8 buffer (descriptors, tables, pixels), so
a batch is one H2D copy, and ``RawPhotos.to(device)`` runs the integer resize on the device.  The result is bit-identical to
the host form.
"""
from __future__ import annotations

import numpy as np
import torch

from .data import _column_taps, _row_taps

# one per photo, at the head of the packed buffer; layout of umpr_photo_desc (include/umpr_hip.h)
DESC = np.dtype([("pixels", "<i8"), ("taps", "<i8"), ("rows", "<i4"), ("cols", "<i4")])
assert DESC.itemsize == 24


def decode_for_gpu(path, size=(224, 224)):
    """(pixels uint8 [rows][cols][3], taps int32 [4*dw + 4*dh]) of one photo, or None for a missing one (unreadable file,
    'unknown' path: get_image's except branch).  `size` = (dw, dh) as for get_image.  The taps index the compacted pixels."""
    dw, dh = size
    try:
        from PIL import Image
        with Image.open(path) as im:
            rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
        h, w, _ = rgb.shape
        x0, x1, a0, a1 = _column_taps(dw, w)
        y0, y1, b0, b1 = _row_taps(dh, h)
    except Exception:
        return None
    rows = np.unique(np.concatenate([y0, y1]))
    cols = np.unique(np.concatenate([x0, x1]))
    if len(rows) < h:
        rgb = np.take(rgb, rows, axis=0)
    if len(cols) < w:
        rgb = np.take(rgb, cols, axis=1)
    taps = np.concatenate([np.searchsorted(cols, x0), np.searchsorted(cols, x1), a0, a1,
                           np.searchsorted(rows, y0), np.searchsorted(rows, y1), b0, b1]).astype(np.int32)
    return np.ascontiguousarray(rgb), taps


class RawPhotos:
    """A batch of decoded photos in one packed uint8 buffer: [n descriptors][tap tables][pixels], n = B*V*P.

    Stands in for the float32 photo tensor of a collated batch: ``.shape`` is the logical (B, V, P, 3, dh, dw),
    ``.pin_memory()`` (DataLoader(pin_memory=True)) and pickling (DataLoader workers) keep the buffer, and
    ``.to(device)`` uploads it on the current stream and returns the float32 photos resized there."""

    def __init__(self, data, geometry, size):
        self.data = data                          # torch.uint8, 1-D, host
        self.geometry = tuple(int(g) for g in geometry)
        self.size = (int(size[0]), int(size[1]))  # (dw, dh)

    @classmethod
    def pack(cls, decoded, geometry, size):
        """Packs decode_for_gpu results (photo order: sample, view, photo) for a batch of `geometry` = (B, V, P)."""
        n = int(np.prod(geometry))
        assert len(decoded) == n, (len(decoded), geometry)
        dw, dh = size
        tap_bytes = 16 * (dw + dh)
        desc = np.zeros(n, dtype=DESC)
        head = -(-desc.nbytes // 16) * 16          # tables and pixels start 16-byte aligned
        off = head
        present = [i for i, d in enumerate(decoded) if d is not None]
        for i in present:
            desc["taps"][i] = off
            off += tap_bytes
        for i in present:
            pix = decoded[i][0]
            desc["pixels"][i] = off
            desc["rows"][i], desc["cols"][i] = pix.shape[:2]
            off += pix.nbytes
        buf = np.empty(off, dtype=np.uint8)
        buf[:desc.nbytes] = desc.view(np.uint8)
        buf[desc.nbytes:head] = 0
        for i in present:
            pix, taps = decoded[i]
            t, p = int(desc["taps"][i]), int(desc["pixels"][i])
            buf[t:t + tap_bytes] = taps.view(np.uint8)
            buf[p:p + pix.nbytes] = pix.reshape(-1)
        return cls(torch.from_numpy(buf), geometry, size)

    @property
    def shape(self):
        dw, dh = self.size
        return torch.Size(self.geometry + (3, dh, dw))

    def descriptors(self):
        """The n umpr_photo_desc records as a numpy structured array (a view of the buffer)."""
        n = int(np.prod(self.geometry))
        return self.data.numpy()[:n * DESC.itemsize].view(DESC)

    def pin_memory(self, device=None):
        return RawPhotos(self.data.pin_memory(), self.geometry, self.size)

    def is_pinned(self):
        return self.data.is_pinned()

    def to(self, device, non_blocking=False):
        """Uploads the buffer (one copy) and resizes on `device`'s current stream: float32 [B, V, P, 3, dh, dw]."""
        from ._lib import UmprHipError, lib
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("RawPhotos resize on an MI355X only (no CPU path): use batch_loader(resize_on_gpu=False)")
        dw, dh = self.size
        n = int(np.prod(self.geometry))
        out = torch.empty(self.shape, dtype=torch.float32, device=device)
        if n == 0:
            return out
        if self.data.dtype != torch.uint8 or self.data.dim() != 1 or self.data.numel() < n * DESC.itemsize:
            raise UmprHipError(f"RawPhotos: buffer of {self.data.numel()} bytes cannot hold the {n} photo descriptors")
        with torch.cuda.device(device):
            packed = self.data.to(device, non_blocking=non_blocking)
            # the descriptors are read (and checked against the buffer size) on the host, from the head of the host buffer
            lib().call("umpr_photo_resize_u8", packed, packed.numel(), self.data, n, dh, dw, out,
                       torch.cuda.current_stream(device).cuda_stream)
        return out

    def __repr__(self):
        return f"RawPhotos(shape={tuple(self.shape)}, bytes={self.data.numel()})"

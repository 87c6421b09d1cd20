"""What an augmented photo is (umpr_photo_fetch_augment_u8, photos.PhotoAugment), on top of the host resize and nothing else:
the window of the resized uint8 image, resized back to the full size, mirrored or not, through the loader's 256-entry table."""
import numpy as np

from umpr_amd.data import resize_bilinear_u8

LUT = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def augment_u8(U, record):
    """uint8 [dh][dw][3] from U uint8 [dh][dw][3] and record = (x0, y0, cw, ch, flip)."""
    x0, y0, cw, ch, flip = (int(v) for v in record)
    dh, dw, _ = U.shape
    assert 1 <= cw and 0 <= x0 and x0 + cw <= dw and 1 <= ch and 0 <= y0 and y0 + ch <= dh and flip in (0, 1), record
    A = resize_bilinear_u8(np.ascontiguousarray(U[y0:y0 + ch, x0:x0 + cw]), (dw, dh))
    return A[:, ::-1] if flip else A


def augment_photo(U, record):
    """float32 [3][dh][dw]: the photo the model sees."""
    return np.ascontiguousarray(LUT[augment_u8(U, record)].transpose(2, 0, 1))


def augment_batch(images, records, size):
    """float32 [n][3][dh][dw]; images[i] is U or None for a missing photo (all zeros whatever its record says)."""
    dw, dh = size
    out = np.zeros((len(images), 3, dh, dw), dtype=np.float32)
    for i, (U, r) in enumerate(zip(images, records)):
        if U is not None:
            out[i] = augment_photo(U, r)
    return out

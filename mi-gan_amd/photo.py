"""Photo loading on the device (``migan_photo_resize_batch``, include/migan_photo_hip.h): what every caller of the reference does to
a photo and its mask before the network sees them, byte for byte as Pillow computes it for uint8 images.

  ``resize_bicubic`` / ``resize_nearest``   ``Image.resize((w, h), Image.BICUBIC)`` of RGB photos, ``Image.resize((w, h), Image.NEAREST)``
                                            of one-channel masks
  ``load_eval``                             scripts/evaluate_fid_lpips.py:142-149 (``InferenceDataset.__getitem__``)
  ``load_demo``                             scripts/demo.py:125-130 with ``resize`` :48-53, ``read_mask`` :26-45 and ``preprocess`` :56-60

Every function takes lists of device uint8 tensors of any sizes, photos [H_i, W_i, 3] and masks [h_i, w_i], and launches on the current
stream.  Both ``load_*`` results go straight into ``Generator.forward_uint8`` / ``forward_samples_uint8`` of either model: 255 means
known there as well, every other value is a hole, which is the scripts' ``// 255``.  Not here: file decoding, the channel selection of
RGBA / LA masks (``read_mask`` :30-41; pass one channel), and the back half of demo.py (``cv2.resize(..., INTER_CUBIC)`` :138).
Like the generators there is no CPU path."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from .hipbind import PHOTO_BICUBIC, PHOTO_INVERT, PHOTO_NEAREST, PHOTO_THRESHOLD, load_library

_SCRATCH = {}
_NO_CPU = "mi-gan_amd.photo needs tensors on an MI355X (HIP) device; there is no CPU path"
SRC_MAX, DST_MAX, ASPECT_MAX = 16384, 4096, 32          # the domain of include/migan_photo_hip.h
READ_MASK_MAX = 512                                      # demo.py:28


def _scratch(need: int, device: torch.device) -> torch.Tensor:
    """one buffer per (device, stream), as metrics keeps its own"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(device).cuda_stream))
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        if len(_SCRATCH) >= 8:                             # (stream handles come and go: keep the cache bounded)
            _SCRATCH.clear()
        buf = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf


def check_sizes(src_hw: Tuple[int, int], dst_wh: Tuple[int, int], what: str = "image") -> None:
    """the domain of migan_photo_resize_batch, refused here with the same words before anything is allocated"""
    sh, sw = src_hw
    dw, dh = dst_wh
    if not (1 <= sh <= SRC_MAX and 1 <= sw <= SRC_MAX):
        raise ValueError(f"{what}: source sides must be in 1 .. {SRC_MAX}, got {sh} x {sw}")
    if not (1 <= dh <= DST_MAX and 1 <= dw <= DST_MAX):
        raise ValueError(f"{what}: destination sides must be in 1 .. {DST_MAX}, got {dh} x {dw}")
    if max(sh, sw) > ASPECT_MAX * min(sh, sw):
        raise ValueError(f"{what}: source aspect ratio above {ASPECT_MAX} : 1 ({sh} x {sw}); Pillow resamples such an image in another order")


def _sizes(size, n: int) -> List[Tuple[int, int]]:
    """(w, h) for all, or one (w, h) per image -> a list of n pairs of ints"""
    if len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in size):
        return [(int(size[0]), int(size[1]))] * n
    if len(size) != n or not all(len(s) == 2 for s in size):
        raise ValueError(f"size must be one (w, h) or one (w, h) per image ({n}), got {size!r}")
    return [(int(w), int(h)) for w, h in size]


def _check_inputs(tensors: Sequence[torch.Tensor], channels: int, what: str) -> torch.device:
    if not isinstance(tensors, (list, tuple)) or len(tensors) == 0 or not all(torch.is_tensor(t) for t in tensors):
        raise RuntimeError(f"{what} must be a non-empty list of tensors")
    device = tensors[0].device
    for i, t in enumerate(tensors):
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)
        if t.dtype != torch.uint8:
            raise RuntimeError(f"{what}[{i}] must be uint8, got {t.dtype}")
        if t.device != device:
            raise RuntimeError(f"{what} must be on one device")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}[{i}] must be contiguous")
        if (channels == 3 and not (t.dim() == 3 and t.shape[2] == 3)) or (channels == 1 and t.dim() != 2):
            raise RuntimeError(f"expected {what}[{i}] {'(H, W, 3)' if channels == 3 else '(H, W)'}, got {list(t.shape)}")
    return device


@torch.no_grad()
def _resize(tensors: Sequence[torch.Tensor], sizes: Sequence[Tuple[int, int]], channels: int, filt: int, flags: int, what: str,
            out: torch.Tensor = None):
    """one migan_photo_resize_batch over the list; `out`: a stacked destination [N, h, w(, 3)] whose rows take the results"""
    device = tensors[0].device
    for i, (t, s) in enumerate(zip(tensors, sizes)):
        check_sizes((int(t.shape[0]), int(t.shape[1])), s, f"{what}[{i}]")
    tail = (3,) if channels == 3 else ()
    outs = [out[i] for i in range(len(tensors))] if out is not None else [torch.empty((h, w) + tail, dtype=torch.uint8, device=device) for w, h in sizes]
    items = [(t.data_ptr(), o.data_ptr(), int(t.shape[0]), int(t.shape[1]), h, w) for t, o, (w, h) in zip(tensors, outs, sizes)]
    lib = load_library()
    with torch.cuda.device(device):                              # the handle-free entry points launch on the CURRENT device
        scratch = _scratch(lib.photo_scratch_bytes(items, channels, filt), device)
        lib.photo_resize_batch(items, channels, filt, flags, scratch.data_ptr(), int(torch.cuda.current_stream(device).cuda_stream))
    return outs


def _result(outs, sizes):
    return torch.stack(outs) if len(set(sizes)) == 1 else outs


def resize_bicubic(images: Sequence[torch.Tensor], size):
    """``img.resize((w, h), Image.BICUBIC)`` of every [H_i, W_i, 3] uint8 photo.  ``size``: one ``(w, h)`` for all (the result is one
    stacked tensor [N, h, w, 3]) or one ``(w, h)`` per image (a list, stacked when all sizes agree)."""
    _check_inputs(images, 3, "images")
    sizes = _sizes(size, len(images))
    return _result(_resize(images, sizes, 3, PHOTO_BICUBIC, 0, "images"), sizes)


def resize_nearest(masks: Sequence[torch.Tensor], size, invert: bool = False, threshold: bool = False):
    """``mask.resize((w, h), Image.NEAREST)`` of every [h_i, w_i] uint8 mask; then ``invert``: 255 - v, then ``threshold``: v < 255 -> 0
    (demo.py:42-44).  ``size`` as in ``resize_bicubic``."""
    _check_inputs(masks, 1, "masks")
    sizes = _sizes(size, len(masks))
    flags = (PHOTO_INVERT if invert else 0) | (PHOTO_THRESHOLD if threshold else 0)
    return _result(_resize(masks, sizes, 1, PHOTO_NEAREST, flags, "masks"), sizes)


def _check_pairs(images, masks, resolution) -> None:
    _check_inputs(images, 3, "images")
    _check_inputs(masks, 1, "masks")
    if len(images) != len(masks):
        raise RuntimeError("images and masks must be lists of one length")
    if masks[0].device != images[0].device:
        raise RuntimeError("images and masks must be on one device")
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not 1 <= resolution <= DST_MAX:
        raise ValueError(f"resolution must be an int in 1 .. {DST_MAX}, got {resolution!r}")


def load_eval(images: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], resolution: int):
    """scripts/evaluate_fid_lpips.py:142-149 -> (img_u8 [N, R, R, 3], mask_u8 [N, R, R]): the photo BICUBIC to (R, R) if a side differs
    from R, the mask NEAREST to (R, R) always."""
    _check_pairs(images, masks, resolution)
    n, r, device = len(images), resolution, images[0].device
    img = torch.empty((n, r, r, 3), dtype=torch.uint8, device=device)
    mask = torch.empty((n, r, r), dtype=torch.uint8, device=device)
    _resize(images, [(r, r)] * n, 3, PHOTO_BICUBIC, 0, "images", out=img)        # (sizes that agree are a copy, as the script's `if` leaves them)
    _resize(masks, [(r, r)] * n, 1, PHOTO_NEAREST, 0, "masks", out=mask)
    return img, mask


def fit_size(w: int, h: int, max_size: int) -> Tuple[int, int]:
    """the size demo.py's ``resize`` (:48-53) gives a (w, h) image, in the script's own expressions (``int(w * (R / w))`` can be R - 1)"""
    if w > max_size or h > max_size:
        resize_ratio = max_size / w if w > h else max_size / h
        w, h = int(w * resize_ratio), int(h * resize_ratio)
        if w < 1 or h < 1:
            raise ValueError(f"demo.py's resize to fit {max_size} leaves a side of 0 ({w} x {h})")
    return w, h


def demo_plan(image_wh: Tuple[int, int], mask_wh: Tuple[int, int], resolution: int):
    """the sizes (w, h) demo.py:125-130 takes a photo and its mask through: (photo fitted to R, mask fitted to 512, that fitted to R)"""
    photo = fit_size(image_wh[0], image_wh[1], resolution)
    first = fit_size(mask_wh[0], mask_wh[1], READ_MASK_MAX)
    return photo, first, fit_size(first[0], first[1], resolution)


def load_demo(images: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], resolution: int, invert_mask: bool = False):
    """scripts/demo.py:125-130 -> (img_u8 [N, R, R, 3], mask_u8 [N, R, R]).  Photo: ``resize(img, R)`` (BICUBIC to fit R, keeping the
    aspect), then (R, R) BICUBIC.  Mask: NEAREST to fit 512, inversion if asked and the threshold ``v < 255 -> 0``, NEAREST to fit R,
    NEAREST to (R, R).  The back half of the script (OpenCV's cubic resize of the result) is not served."""
    _check_pairs(images, masks, resolution)
    n, r, device = len(images), resolution, images[0].device
    plans = [demo_plan((int(i.shape[1]), int(i.shape[0])), (int(m.shape[1]), int(m.shape[0])), r) for i, m in zip(images, masks)]
    img = torch.empty((n, r, r, 3), dtype=torch.uint8, device=device)
    mask = torch.empty((n, r, r), dtype=torch.uint8, device=device)
    fitted = _resize(images, [p[0] for p in plans], 3, PHOTO_BICUBIC, 0, "images")
    _resize(fitted, [(r, r)] * n, 3, PHOTO_BICUBIC, 0, "images", out=img)
    flags = (PHOTO_INVERT if invert_mask else 0) | PHOTO_THRESHOLD
    m1 = _resize(masks, [p[1] for p in plans], 1, PHOTO_NEAREST, flags, "masks")
    m2 = _resize(m1, [p[2] for p in plans], 1, PHOTO_NEAREST, 0, "masks")
    _resize(m2, [(r, r)] * n, 1, PHOTO_NEAREST, 0, "masks", out=mask)
    return img, mask

"""PSNR / SSIM of completions against the ground-truth photo, on the device (``migan_metrics_batch``, include/migan_metrics_hip.h):
the reference's ``lib/evaluator/eva_psnr.py`` (``for_dataset=None`` and ``'div2k'``) and ``lib/evaluator/eva_ssim.py``
(``compute_ssim(..., size_average=False)``) for S completions per photo in one call, plus the hole-only variant inpainting reports.
Like the generators there is no CPU path."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .hipbind import METRICS_CHW, METRICS_F32, METRICS_HWC, METRICS_U8, load_library

_SCRATCH = {}
_NO_CPU = "mi-gan_amd.metrics needs tensors on an MI355X (HIP) device; there is no CPU path"


def _scratch(need: int, device: torch.device) -> torch.Tensor:
    """one buffer per (device, stream), as MIGAN_Pipeline keeps its own: two streams measuring at once never share the partial sums"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(device).cuda_stream))
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        if len(_SCRATCH) >= 8:                             # (stream handles come and go: keep the cache bounded)
            _SCRATCH.clear()
        buf = torch.empty(need, dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf


def _hw(shape, layout: str, lead: int) -> Optional[Tuple[int, int]]:
    """(H, W) of a shape with `lead` leading axes in front of the image axes, or None when it is no 3-channel image in `layout`"""
    if len(shape) != lead + 3:
        return None
    if layout == "chw":
        return (int(shape[-2]), int(shape[-1])) if shape[-3] == 3 else None
    return (int(shape[-3]), int(shape[-2])) if shape[-1] == 3 else None


def _check_pair(pred: torch.Tensor, gt: torch.Tensor, device, dtype) -> None:
    if not (pred.is_cuda and gt.is_cuda):
        raise RuntimeError(_NO_CPU)
    if gt.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"gt must be uint8 or float32, got {gt.dtype}")
    if pred.dtype != gt.dtype or gt.dtype != dtype:
        raise RuntimeError(f"pred and gt must have one dtype, got {pred.dtype} and {gt.dtype}")
    if pred.device != device or gt.device != device:
        raise RuntimeError("pred, gt and mask must be on the same device")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise RuntimeError("pred and gt must be contiguous")


def _check_mask(mask: torch.Tensor, h: int, w: int, device, what: str) -> None:
    if not mask.is_cuda:
        raise RuntimeError(_NO_CPU)
    if mask.dtype != torch.uint8:
        raise RuntimeError("mask must be uint8, 255 = known pixel (the convention of compose and of the pipeline)")
    if mask.device != device:
        raise RuntimeError("pred, gt and mask must be on the same device")
    if not mask.is_contiguous():
        raise RuntimeError("mask must be contiguous")
    if tuple(mask.shape[-2:]) != (h, w):
        raise RuntimeError(f"expected {what} of size {[h, w]}, got {list(mask.shape)}")


@torch.no_grad()
def psnr_ssim(pred, gt, mask=None, *, shave: int = 0, value_range: Tuple[float, float] = (0.0, 1.0), layout: Optional[str] = None):
    """(psnr, ssim) of completions against photos, float64 tensors on the inputs' device.

    Tensor form: ``gt`` [N,3,H,W] (``layout="chw"``) or [N,H,W,3] (``"hwc"``), float32 or uint8; the default layout is ``chw`` for
    float32 and ``hwc`` for uint8, the layouts the generators produce.  ``pred`` has gt's shape -> results [N], or an S axis after N
    ([N,S,3,H,W] / [N,S,H,W,3], what ``forward_samples`` / ``forward_samples_uint8`` return) -> results [N,S].  ``mask``: [N,H,W] or
    [N,1,H,W] uint8.
    List form (photos of different sizes): ``gt`` a list of [1,3,H_i,W_i] or [3,H_i,W_i], ``pred`` a list of [S,3,H_i,W_i] (what
    ``MIGAN_Pipeline.forward_samples`` returns), ``mask`` a list of [1,1,H_i,W_i] or [H_i,W_i]; the default layout is ``chw``, the
    pipeline's; results [N,S].

    uint8 data is v / 255, float32 data (v - lo) / (hi - lo) with ``value_range=(lo, hi)``, not clamped: (0, 1) is the reference's
    ``rgb_range=1``, (-1, 1) serves the generators' float32 images.  ``shave``: the MSE leaves out that many rows and columns at
    every side (8 is the reference's default evaluator, ``scale + 6``); the SSIM mean is never shaved.  With a mask (255 = known
    pixel) both means run over the hole alone, the windows still see the whole image; a photo without a hole pixel gives NaN.
    ``psnr = -10 log10(mse)``: an identical pair gives +inf, as numpy does in the reference.  Runs on the current stream of the
    inputs' device."""
    listed = isinstance(gt, (list, tuple))
    if listed != isinstance(pred, (list, tuple)) or (mask is not None and listed != isinstance(mask, (list, tuple))):
        raise RuntimeError("pred, gt and mask must all be tensors or all be lists")
    if isinstance(shave, bool) or not isinstance(shave, int) or shave < 0:
        raise RuntimeError(f"shave must be a non-negative int, got {shave!r}")
    if not listed and not (torch.is_tensor(gt) and torch.is_tensor(pred) and (mask is None or torch.is_tensor(mask))):
        raise RuntimeError("pred, gt and mask must all be tensors or all be lists")
    first = gt[0] if listed and len(gt) else gt
    if listed and (len(gt) == 0 or len(pred) != len(gt) or (mask is not None and len(mask) != len(gt))):
        raise RuntimeError("pred, gt and mask must be lists of one length, at least 1")
    if not torch.is_tensor(first):
        raise RuntimeError("pred, gt and mask must all be tensors or all be lists")
    if layout is None:
        layout = "chw" if listed or first.dtype != torch.uint8 else "hwc"
    if layout not in ("chw", "hwc"):
        raise RuntimeError(f"layout must be 'chw' or 'hwc', got {layout!r}")
    device, dtype = first.device, first.dtype
    items, squeeze = [], False
    if listed:
        samples = None
        for i, (g, p) in enumerate(zip(gt, pred)):
            _check_pair(p, g, device, dtype)
            hw = _hw(g.shape, layout, 1 if g.dim() == 4 else 0)
            if hw is None or (g.dim() == 4 and g.shape[0] != 1):
                raise RuntimeError(f"expected gt[{i}] (1, 3, H, W) or (3, H, W) in layout {layout}, got {list(g.shape)}")
            if _hw(p.shape, layout, 1) != hw or (samples is not None and p.shape[0] != samples):
                raise RuntimeError(f"expected pred[{i}] (S, ...) of gt[{i}]'s image shape with one S for all, got {list(p.shape)} for {list(g.shape)}")
            samples = int(p.shape[0])
            m = None
            if mask is not None:
                m = mask[i]
                if not (m.dim() == 2 or (m.dim() == 4 and m.shape[0] == 1 and m.shape[1] == 1)):
                    raise RuntimeError(f"expected mask[{i}] (1, 1, H, W) or (H, W), got {list(m.shape)}")
                _check_mask(m, hw[0], hw[1], device, f"mask[{i}]")
            items.append((g.data_ptr(), p.data_ptr(), None if m is None else m.data_ptr(), hw[0], hw[1]))
    else:
        _check_pair(pred, gt, device, dtype)
        hw = _hw(gt.shape, layout, 1)
        if hw is None:
            raise RuntimeError(f"expected gt (N, 3, H, W) for layout chw or (N, H, W, 3) for hwc, got {list(gt.shape)} with layout {layout}")
        n = int(gt.shape[0])
        if tuple(pred.shape) == tuple(gt.shape):
            samples, squeeze = 1, True
        elif pred.dim() == 5 and pred.shape[0] == n and tuple(pred.shape[2:]) == tuple(gt.shape[1:]):
            samples = int(pred.shape[1])
        else:
            raise RuntimeError(f"expected pred of gt's shape {list(gt.shape)}, or with an S axis after N, got {list(pred.shape)}")
        if mask is not None:
            if not ((mask.dim() == 3 or (mask.dim() == 4 and mask.shape[1] == 1)) and mask.shape[0] == n):
                raise RuntimeError(f"expected mask (N, H, W) or (N, 1, H, W), got {list(mask.shape)}")
            _check_mask(mask, hw[0], hw[1], device, "mask")
        per_gt, per_mask = 3 * hw[0] * hw[1] * gt.element_size(), hw[0] * hw[1]
        items = [(gt.data_ptr() + i * per_gt, pred.data_ptr() + i * samples * per_gt, None if mask is None else mask.data_ptr() + i * per_mask,
                  hw[0], hw[1]) for i in range(n)]
    if not items or samples < 1:
        raise RuntimeError("nothing to measure: at least one photo and one completion per photo")
    for _, _, _, h, w in items:
        if h - 2 * shave < 1 or w - 2 * shave < 1:
            raise RuntimeError(f"shave {shave} leaves nothing of a {h} x {w} image")
    lib = load_library()
    mse = torch.empty((len(items), samples), dtype=torch.float64, device=device)
    ssim_out = torch.empty_like(mse)
    with torch.cuda.device(device):                              # the handle-free entry points launch on the CURRENT device
        scratch = _scratch(lib.metrics_scratch_bytes(items, samples), device)
        lib.metrics_batch(items, samples, METRICS_U8 if dtype == torch.uint8 else METRICS_F32, METRICS_CHW if layout == "chw" else METRICS_HWC,
                          shave, float(value_range[0]), float(value_range[1]), scratch.data_ptr(), mse.data_ptr(), ssim_out.data_ptr(),
                          int(torch.cuda.current_stream(device).cuda_stream))
    psnr_out = -10.0 * torch.log10(mse)                          # eva_psnr.py:56
    return (psnr_out[:, 0], ssim_out[:, 0]) if squeeze else (psnr_out, ssim_out)


def psnr(pred, gt, mask=None, **kw):
    return psnr_ssim(pred, gt, mask, **kw)[0]


def ssim(pred, gt, mask=None, **kw):
    return psnr_ssim(pred, gt, mask, **kw)[1]

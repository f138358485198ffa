"""Random hole masks on the device (``migan_masks_draw`` / ``migan_masks_raster``, include/migan_masks_hip.h): the reference's
``RandomMask`` (scripts/generate_masks.py:16-93; the same text in scripts/evaluate_fid_lpips.py and lib/data_factory/ds_ffhq.py),
byte for byte for the same state of numpy's legacy generator.

  ``random_masks(n, resolution, hole_range=(0, 1), rng=None)``   ``np.stack([RandomMask(R, list(hole_range)) for _ in range(n)])`` as a
                                                                 device uint8 tensor, 255 known / 0 hole: the ``mask_u8`` of
                                                                 ``forward_uint8``, ``metrics.psnr_ssim`` and ``MIGAN_Pipeline``

The draws (numpy's MT19937 stream, the vertices, the corners of Pillow's wide-line quadrilaterals) are made by host code inside the
library; one launch per chunk of candidates rasterises them as Pillow does and counts their hole pixels; the counts come back once per
chunk and decide which candidates the reference would have returned.  After the call ``rng`` is in exactly the state the reference's
loop leaves it in, so a caller can interleave its own draws.  The training formatters' float form is ``(m / 255).float()[None]``.
Like the generators there is no CPU path."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from .hipbind import MASKS_BAND, MASKS_PLAN_WORDS_MAX, MasksRng, load_library

R_MIN, R_MAX = 16, 1024                                  # the domain of include/migan_masks_hip.h
CHUNK_MAX = 4096                                         # candidates of one launch, and
CHUNK_BYTES = 256 << 20                                  # the bytes their masks may take
_NO_CPU = "mi-gan_amd.masks needs an MI355X (HIP) device; there is no CPU path"


def default_max_candidates(n: int) -> int:
    return max(10000, 1000 * n)


def check_arguments(n, resolution, hole_range):
    """what is refused before any draw -> coef, the reference's ``min(hole_range[0] + hole_range[1], 1.0)`` (None draws like [0, 1])"""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"n must be an int >= 1, got {n!r}")
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not R_MIN <= resolution <= R_MAX:
        raise ValueError(f"resolution must be an int in {R_MIN} .. {R_MAX}, got {resolution!r}")
    if hole_range is None:
        return 1.0
    if len(hole_range) != 2:
        raise ValueError(f"hole_range must be (low, high) or None, got {hole_range!r}")
    coef = min(hole_range[0] + hole_range[1], 1.0)
    if not math.isfinite(coef) or int(5 * coef) < 1:
        raise ValueError(f"hole_range {tuple(hole_range)!r}: hole_range[0] + hole_range[1] must be at least 0.2 "
                         "(below, the reference's np.random.randint(int(5 * coef)) raises)")
    return coef


def _get_state(rng):
    if rng is None:
        return np.random.get_state()
    if isinstance(rng, np.random.RandomState):
        return rng.get_state()
    raise TypeError(f"rng must be a numpy.random.RandomState or None (numpy's global legacy generator), got {type(rng).__name__}; "
                    "numpy.random.Generator draws another stream")


def _set_state(rng, state):
    (np.random if rng is None else rng).set_state(state)


class TorchBackend:
    """where the candidates of a chunk are rasterised: device tensors and the current stream"""

    def __init__(self, lib, device: torch.device):
        self.lib, self.device = lib, device

    def empty(self, k: int, r: int):
        return torch.empty((k, r, r), dtype=torch.uint8, device=self.device)

    def raster(self, words: np.ndarray, count: int, r: int, buf):
        """launches the chunk on the current stream -> a handle for `holes`"""
        plans = torch.from_numpy(words).to(self.device, non_blocking=True)
        holes = torch.empty((count, (r + MASKS_BAND - 1) // MASKS_BAND), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):                     # the handle-free entry points launch on the CURRENT device
            self.lib.masks_raster(plans.data_ptr(), words.size, count, r, buf.data_ptr(), holes.data_ptr(),
                                  int(torch.cuda.current_stream(self.device).cuda_stream))
        return holes, plans

    def holes(self, handle) -> np.ndarray:
        """the one read-back of a chunk: hole pixels per candidate"""
        return handle[0].cpu().numpy().astype(np.int64).sum(axis=1)

    def take(self, buf, idx: Sequence[int], out, pos: int) -> None:
        if len(idx) == 0:
            return
        index = torch.tensor(list(idx), dtype=torch.int64).to(self.device, non_blocking=True)
        torch.index_select(buf, 0, index, out=out[pos:pos + len(idx)])


def generate(backend, lib, n: int, resolution: int, hole_range, rng, out, max_candidates: Optional[int] = None, chunk: Optional[int] = None):
    """The acceptance loop over chunks of candidates -> float64 [n] hole ratios; fills out[0 .. n).  `backend`: TorchBackend, or the
    CPU tests' stand-in over host memory."""
    coef = check_arguments(n, resolution, hole_range)
    if max_candidates is None:
        max_candidates = default_max_candidates(n)
    if isinstance(max_candidates, bool) or not isinstance(max_candidates, int) or max_candidates < 1:
        raise ValueError(f"max_candidates must be an int >= 1, got {max_candidates!r}")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"chunk must be an int >= 1, got {chunk!r}")
    r, pixels = resolution, resolution * resolution
    start = _get_state(rng)
    state = MasksRng.from_state(start)
    limit = max(1, min(CHUNK_MAX, CHUNK_BYTES // pixels))
    ratios = np.empty(n, np.float64)
    have = drawn = 0
    rate = 1.0                                                   # accepted / drawn so far
    ahead = None                                                 # a chunk drawn while the previous one was on the device
    scratch = None
    try:
        while have < n:
            if drawn >= max_candidates:
                raise RuntimeError(f"{max_candidates} candidates gave {have} of {n} masks with a hole ratio inside {hole_range!r} "
                                   f"at resolution {r}; the generator is back in the state of the call's start")
            if ahead is not None:
                k, words, states = ahead
                ahead = None
            else:
                if hole_range is None:
                    k = min(limit, n - have) if chunk is None else min(chunk, n - have)
                else:
                    k = chunk if chunk is not None else min(limit, int((n - have) / max(rate, 1e-3) * 1.25) + 8)
                k = max(1, min(k, max_candidates - drawn))
                k, words, states = _draw(lib, state, r, coef, k)
            direct = hole_range is None                          # nothing is rejected: straight into the result
            if direct:
                buf = out[have:have + k]
            else:
                if scratch is None or scratch.shape[0] < k:
                    scratch = backend.empty(k, r)
                buf = scratch
            handle = backend.raster(words, k, r, buf)
            # the next chunk's draws overlap the launch where the acceptance so far says this chunk will not be the last
            expect = have + rate * k
            if chunk is None and drawn > 0 and expect < 0.8 * n and drawn + k < max_candidates:
                k2 = max(1, min(limit, int((n - expect) / max(rate, 1e-3) * 1.25) + 8, max_candidates - drawn - k))
                ahead = _draw(lib, state, r, coef, min(k2, n - have - k) if hole_range is None else k2)
            holes = backend.holes(handle)
            if (holes < 0).any():
                raise RuntimeError("migan_masks_raster refused a plan migan_masks_draw made")
            ratio = 1.0 - (pixels - holes) / float(pixels)       # 1 - np.mean(mask): the sums are exact
            if hole_range is None:
                keep = np.arange(k)
            else:
                keep = np.nonzero(~((ratio <= hole_range[0]) | (ratio >= hole_range[1])))[0]
            keep = keep[:n - have]
            if not direct:
                backend.take(buf, keep.tolist(), out, have)
            ratios[have:have + len(keep)] = ratio[keep]
            have += len(keep)
            if have >= n:
                # the generator as the reference leaves it: behind the last candidate it returned
                state = states[int(keep[-1])]
                ahead = None
            drawn += k
            rate = max(have, 0.5) / drawn
    except BaseException:
        _set_state(rng, start)
        raise
    _set_state(rng, state.to_state())
    return ratios


def _draw(lib, state: MasksRng, r: int, coef: float, k: int):
    """draws k candidates, advancing `state` -> (k, the plan words, the generator behind every candidate)"""
    words = np.empty(k + 1 + k * MASKS_PLAN_WORDS_MAX, np.int32)
    states = (MasksRng * k)()
    used = lib.masks_draw(state, r, coef, k, words.ctypes.data, words.size, states)
    return k, words[:used], states


@torch.no_grad()
def random_masks(n: int, resolution: int, hole_range=(0, 1), *, rng=None, device=None, out: Optional[torch.Tensor] = None,
                 return_hole_ratio: bool = False, max_candidates: Optional[int] = None, chunk: Optional[int] = None):
    """``np.stack([RandomMask(resolution, list(hole_range)) for _ in range(n)])`` -> uint8 [n, R, R] on the device, 255 known, 0 hole.

    ``rng``: a ``numpy.random.RandomState``, or None for numpy's global legacy generator, as in the reference; afterwards it is in
    exactly the state the reference's loop leaves it in.  ``hole_range=None``: no candidate is rejected (the draws are those of
    ``[0, 1]``).  ``out``: a contiguous uint8 device tensor [n, R, R] to fill.  ``return_hole_ratio``: also the float64 [n] hole ratios
    (a host tensor).  ``max_candidates`` (default ``max(10000, 1000 n)``): more rejected candidates than that raise RuntimeError -- a
    range such as (0.999, 1) would never return -- with the generator restored to the call's start.  ``chunk``: candidates per launch
    (default: from ``n`` and the acceptance so far).  Raises ValueError before any draw for ``n < 1``, a resolution outside 16 .. 1024
    and ``hole_range[0] + hole_range[1] < 0.2``, where the reference's ``randint`` raises."""
    check_arguments(n, resolution, hole_range)
    _get_state(rng)                                              # (the type of rng, before a device is asked for)
    if out is not None:
        if not torch.is_tensor(out) or not out.is_cuda:
            raise RuntimeError(_NO_CPU)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, resolution, resolution) or not out.is_contiguous():
            raise RuntimeError(f"out must be a contiguous uint8 tensor of shape {(n, resolution, resolution)}, got {out.dtype} {list(out.shape)}")
        if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, out.device.index):
            raise RuntimeError("out is on another device")
        dev = out.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(_NO_CPU)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((n, resolution, resolution), dtype=torch.uint8, device=dev)
    lib = load_library()
    ratios = generate(TorchBackend(lib, dev), lib, n, resolution, hole_range, rng, out, max_candidates, chunk)
    return (out, torch.from_numpy(ratios)) if return_hole_ratio else out

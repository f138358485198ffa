"""ctypes binding of the C ABI in include/*.h (libmigan_hip.so): the table ``ABI`` declares every entry point once.

This is the binding a maintainer of the reference would add next to
``lib/model_zoo/migan_inference.py``.  It deals in raw
addresses and sizes only; torch appears nowhere in this file.  There is no
fallback: if the shared library is missing or fails to load, ``load_library``
raises ``MiganError`` naming the build command.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libmigan_hip.so"

MIGAN_OK, MIGAN_EINVAL, MIGAN_ESTATE, MIGAN_ERUNTIME, MIGAN_EUNSUPPORTED = 0, 1, 2, 3, 4
# activation storage formats (MIGAN_DTYPE_*) and GEMM variants (MIGAN_GEMM_*) of include/migan_hip.h
DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "f16": 2, "fp16": 2, "float16": 2}
DTYPE_NAMES = {0: "f32", 1: "bf16", 2: "f16"}
GEMMS = {"default": -1, "f32": 0, "bf16x3": 1, "f16x2": 2, "f16": 3}
GEMM_NAMES = {0: "f32", 1: "bf16x3", 2: "f16x2", 3: "f16"}


def dtype_code(dtype) -> int:
    """'f32' | 'bf16' | 'f16' | a MIGAN_DTYPE_* int | anything whose str() ends in one of those names (torch.bfloat16)"""
    if isinstance(dtype, int):
        if dtype not in DTYPE_NAMES:
            raise ValueError(f"unknown activation dtype code {dtype}")
        return dtype
    key = str(dtype).split(".")[-1].lower()
    if key not in DTYPES:
        raise ValueError(f"activation dtype must be one of f32 / bf16 / f16, got {dtype!r}")
    return DTYPES[key]


class MiganError(RuntimeError):
    def __init__(self, msg: str, code: int = MIGAN_ERUNTIME):
        super().__init__(msg)
        self.code = code


def library_path() -> str:
    """the in-tree libmigan_hip.so; MIGAN_HIP_LIBRARY may name ANOTHER BUILD OF THE SAME LIBRARY (measurement builds for same-box
    A/B runs: scripts/phase_profile.py) -- whatever is loaded must report the gfx950 backend, see MiganLib"""
    return os.environ.get("MIGAN_HIP_LIBRARY", os.path.join(_HERE, "csrc", _LIBNAME))


PRODUCT_BACKEND = "hip:gfx950"


class SepConvDesc(C.Structure):
    """struct migan_sepconv_desc"""
    _fields_ = [(n, C.c_void_p) for n in (
        "x", "y", "skip", "conv1_weight", "conv1_bias", "conv2_weight", "noise_const", "noise_strength",
        "fromrgb_weight", "fromrgb_bias", "torgb_weight", "torgb_bias", "img_prev", "img_out")] + [
        (n, C.c_int) for n in ("batch", "cin", "cout", "res_in", "down", "up")] + [
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("wsplit", C.c_void_p), ("wsplit_bytes", C.c_size_t)] + [
        (n, C.c_int) for n in ("gemm", "dtype", "width_in")]


COMODGAN_DTYPE_F32, COMODGAN_DTYPE_F16 = 0, 2    # include/comodgan_fp16_storage_hip.h
METRICS_U8, METRICS_F32 = 0, 1                    # include/migan_metrics_hip.h
METRICS_CHW, METRICS_HWC = 0, 1
PHOTO_NEAREST, PHOTO_BICUBIC = 0, 1               # include/migan_photo_hip.h
PHOTO_INVERT, PHOTO_THRESHOLD = 1, 2
MASKS_PLAN_WORDS_MAX, MASKS_BAND = 4958, 32       # include/migan_masks_hip.h
NOISE_MODES = {"none": 0, "const": 1, "random": 2}  # COMODGAN_NOISE_* of include/comodgan_hip.h


def _table(struct, rows, null_ok=True):
    """rows of values in the order of `struct`'s fields -> a (struct * max(1, len))() array: pointers `or None`, ints int(), an int[4] box
    by slice.  null_ok: None passes a null table through"""
    if rows is None and null_ok:
        return None
    arr = (struct * max(1, len(rows)))()
    for a, row in zip(arr, rows):
        for (field, ctype), v in zip(struct._fields_, row, strict=True):
            if ctype is C.c_void_p:
                setattr(a, field, v or None)
            elif ctype is C.c_int:
                setattr(a, field, int(v))
            else:
                getattr(a, field)[:] = [int(t) for t in v]
    return arr


class MetricsItem(C.Structure):
    """struct migan_metrics_item"""
    _fields_ = [("gt", C.c_void_p), ("pred", C.c_void_p), ("mask", C.c_void_p), ("H", C.c_int), ("W", C.c_int)]


def metrics_items(items):
    """[(gt_ptr, pred_ptr, mask_ptr or None, H, W), ...] -> a migan_metrics_item array (None passes a null table through)"""
    return _table(MetricsItem, items)


class PhotoItem(C.Structure):
    """struct migan_photo_item"""
    _fields_ = [("src_u8", C.c_void_p), ("dst_u8", C.c_void_p)] + [(n, C.c_int) for n in ("src_height", "src_width", "dst_height", "dst_width")]


def photo_items(items):
    """[(src_ptr, dst_ptr, src_height, src_width, dst_height, dst_width), ...] -> a migan_photo_item array (None passes a null table through)"""
    return _table(PhotoItem, items)


class MasksRng(C.Structure):
    """struct migan_masks_rng: RandomState.get_state() without its name"""
    _fields_ = [("key", C.c_uint32 * 624), ("pos", C.c_int32), ("has_gauss", C.c_int32), ("gauss", C.c_double)]

    @classmethod
    def from_state(cls, state):
        """('MT19937', key, pos, has_gauss, cached_gaussian) -> struct"""
        import numpy as np
        if state[0] != "MT19937":
            raise TypeError(f"the generator must be numpy's legacy MT19937 RandomState, got {state[0]!r}")
        s = cls()
        C.memmove(s.key, np.ascontiguousarray(state[1], dtype=np.uint32).ctypes.data, 624 * 4)
        s.pos, s.has_gauss, s.gauss = int(state[2]), int(state[3]), float(state[4])
        return s

    def to_state(self):
        import numpy as np
        return ("MT19937", np.frombuffer(bytes(self.key), dtype=np.uint32).copy(), int(self.pos), int(self.has_gauss), float(self.gauss))


class PipelineItem(C.Structure):
    """struct migan_pipeline_item"""
    _fields_ = [("image_chw_u8", C.c_void_p), ("mask_u8", C.c_void_p)] + [
        (n, C.c_int) for n in ("height", "width", "mask_height", "mask_width")]


def pipeline_items(items):
    """[(image_ptr, mask_ptr, height, width, mask_height, mask_width), ...] -> a migan_pipeline_item array"""
    return _table(PipelineItem, items, null_ok=False)


class PipelineRegionRow(C.Structure):
    """struct migan_pipeline_region_row"""
    _fields_ = [("image_chw_u8", C.c_void_p), ("mask_u8", C.c_void_p), ("labels_u8", C.c_void_p), ("height", C.c_int), ("width", C.c_int),
                ("label", C.c_int), ("box", C.c_int * 4)]


def pipeline_region_rows(rows):
    """[(image_ptr, mask_ptr, labels_ptr or None, height, width, label, (x_min, x_max, y_min, y_max)), ...] -> a migan_pipeline_region_row
    array (None passes a null table through)"""
    return _table(PipelineRegionRow, rows)


class PipelineRegionPasteRow(C.Structure):
    """struct migan_pipeline_region_paste_row"""
    _fields_ = [("image_chw_u8", C.c_void_p), ("labels_u8", C.c_void_p), ("patch_chw_u8", C.c_void_p), ("height", C.c_int), ("width", C.c_int),
                ("label", C.c_int), ("box", C.c_int * 4)]


def pipeline_region_paste_rows(rows):
    """[(image_ptr, labels_ptr or None, patch_ptr, height, width, label, (x_min, x_max, y_min, y_max)), ...] -> a
    migan_pipeline_region_paste_row array (None passes a null table through)"""
    return _table(PipelineRegionPasteRow, rows)


class CoModGANConfig(C.Structure):
    """struct comodgan_config"""
    _fields_ = [(n, C.c_int) for n in ("resolution", "ch_base", "ch_max", "z_dim", "w_dim", "w0_dim", "map_layers", "num_ws")]


# THE DECLARATION OF THE C ABI: header (in the order the headers were added) -> entry point -> (result type, argument types), in the
# header's own order.  A new entry point is declared in its header and here, nowhere else; tests/test_abi_headers.py holds every row
# against the prototype.  vp for a pointer is a DEVICE (or opaque) address passed as an integer, P(...) a host array or out-parameter.
P = C.POINTER
vp, ci, sz, fl, db, cs, i64 = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_double, C.c_char_p, C.c_int64
ABI = {
    "migan_hip.h": {
        "migan_create": (ci, (ci, ci, ci, P(vp))),
        "migan_destroy": (ci, (vp,)),
        "migan_set_gemm": (ci, (vp, ci)),
        "migan_get_gemm": (ci, (vp, P(ci))),
        "migan_assume_static_weights": (ci, (vp, ci)),
        "migan_set_streams": (ci, (vp, ci)),
        "migan_num_weights": (ci, (vp, P(ci))),
        "migan_weight_info": (ci, (vp, ci, P(cs), P(i64), P(ci), P(ci))),
        "migan_set_weight": (ci, (vp, cs, vp, P(i64), ci)),
        "migan_commit": (ci, (vp, vp)),
        "migan_workspace_bytes": (ci, (vp, ci, P(sz))),
        "migan_forward": (ci, (vp, vp, vp, ci, vp, sz, vp)),
        "migan_workspace_bytes_hw": (ci, (vp, ci, ci, ci, P(sz))),
        "migan_forward_hw": (ci, (vp, vp, vp, ci, ci, ci, vp, sz, vp)),
        "migan_forward_u8": (ci, (vp, vp, vp, vp, ci, vp, sz, vp)),
        "migan_pipeline_mask_resize": (ci, (vp, ci, ci, vp, ci, ci, vp)),
        "migan_pipeline_scratch_bytes": (ci, (ci, ci, P(sz))),
        "migan_pipeline_bbox": (ci, (vp, ci, ci, ci, ci, vp, P(ci), vp)),
        "migan_pipeline_pre": (ci, (vp, vp, ci, ci, P(ci), ci, vp, vp)),
        "migan_pipeline_post": (ci, (vp, vp, ci, ci, P(ci), ci, vp, P(fl), vp, vp)),
        "migan_pipeline_batch_scratch_bytes": (ci, (P(PipelineItem), ci, P(sz))),
        "migan_pipeline_batch_pre": (ci, (P(PipelineItem), ci, ci, ci, vp, vp, vp, vp)),
        "migan_pipeline_batch_post": (ci, (P(PipelineItem), ci, ci, vp, vp, P(fl), vp, vp)),
        "migan_num_launches": (ci, (vp, P(ci))),
        "migan_launch_info": (ci, (vp, ci, P(cs), P(cs), P(db), P(db), P(db), P(ci))),
        "migan_forward_split": (ci, (vp, ci, P(ci), P(ci))),
        "migan_forward_parts": (ci, (vp, vp, P(vp), ci, vp, sz, vp, P(vp), ci, P(ci), P(ci))),
        "migan_forward_timed": (ci, (vp, vp, vp, ci, vp, sz, vp, P(fl), ci)),
        "migan_set_debug": (ci, (vp, ci)),
        "migan_debug_tensor": (ci, (vp, ci, cs, P(sz), P(i64))),
        "migan_debug_tensor_hw": (ci, (vp, ci, ci, ci, cs, P(sz), P(i64))),
        "migan_sepconv_forward": (ci, (P(SepConvDesc), vp)),
        "migan_pack_input": (ci, (vp, vp, vp, ci, ci, vp)),
        "migan_compose_output": (ci, (vp, vp, vp, vp, ci, ci, vp)),
        "migan_set_tuning": (ci, (cs, ci)),
        "migan_get_tuning": (ci, (cs, P(ci))),
        "migan_tuning_key": (cs, (ci,)),
        "migan_last_error": (cs, ()),
        "migan_last_kernel": (cs, ()),
        "migan_nan_policy": (cs, ()),
        "migan_backend": (cs, ()),
        "migan_gemm_variant": (cs, ()),
        "migan_version": (ci, ()),
    },
    "comodgan_hip.h": {
        "comodgan_create": (ci, (P(CoModGANConfig), ci, P(vp))),
        "comodgan_destroy": (ci, (vp,)),
        "comodgan_num_weights": (ci, (vp, P(ci))),
        "comodgan_weight_info": (ci, (vp, ci, P(cs), P(i64), P(ci), P(ci))),
        "comodgan_set_weight": (ci, (vp, cs, vp, P(i64), ci)),
        "comodgan_commit": (ci, (vp, vp)),
        "comodgan_workspace_bytes": (ci, (vp, ci, P(sz))),
        "comodgan_assume_static_weights": (ci, (vp, ci)),
        "comodgan_noise_floats": (ci, (vp, P(sz))),
        "comodgan_forward": (ci, (vp, vp, vp, vp, ci, fl, ci, vp, vp, sz, vp)),
        "comodgan_num_launches": (ci, (vp, P(ci))),
        "comodgan_launch_info": (ci, (vp, ci, P(cs), P(cs), P(db), P(db), P(db))),
        "comodgan_forward_timed": (ci, (vp, vp, vp, vp, ci, fl, ci, vp, vp, sz, vp, P(fl), ci)),
        "comodgan_set_truncation_cutoff": (ci, (vp, ci)),
        "comodgan_set_debug": (ci, (vp, ci)),
        "comodgan_debug_tensor": (ci, (vp, ci, cs, P(sz), P(i64), P(ci))),
    },
    "comodgan_samples_hip.h": {
        "comodgan_workspace_bytes_samples": (ci, (vp, ci, ci, P(sz))),
        "comodgan_forward_samples": (ci, (vp, vp, vp, vp, ci, ci, fl, ci, vp, vp, sz, vp)),
        "comodgan_forward_samples_timed": (ci, (vp, vp, vp, vp, ci, ci, fl, ci, vp, vp, sz, vp, P(fl), ci)),
        "comodgan_debug_tensor_samples": (ci, (vp, ci, ci, cs, P(sz), P(i64), P(ci))),
    },
    "migan_pipeline_samples_hip.h": {
        "migan_pipeline_batch_post_samples": (ci, (P(PipelineItem), ci, ci, ci, vp, vp, P(fl), vp, P(vp), vp)),
    },
    "comodgan_fp16_hip.h": {
        "comodgan_set_fp16_blocks": (ci, (vp, ci, ci)),
        "comodgan_get_fp16_blocks": (ci, (vp, P(ci), P(ci))),
    },
    "comodgan_fp16_storage_hip.h": {
        "comodgan_set_fp16_storage": (ci, (vp, ci)),
        "comodgan_get_fp16_storage": (ci, (vp, P(ci))),
        "comodgan_debug_tensor_dtype": (ci, (vp, ci, ci, cs, P(ci))),
    },
    "comodgan_stages_hip.h": {
        "comodgan_stages_workspace_bytes": (ci, (vp, ci, ci, P(sz))),
        "comodgan_mapping": (ci, (vp, vp, vp, ci, fl, ci, vp, sz, vp)),
        "comodgan_encode": (ci, (vp, vp, vp, P(vp), ci, vp, sz, vp)),
        "comodgan_synthesize": (ci, (vp, vp, P(vp), vp, vp, ci, ci, ci, vp, P(vp), P(vp), vp, sz, vp)),
        "comodgan_weight_preparations": (ci, (vp, P(C.c_ulonglong))),
    },
    "migan_pipeline_patches_hip.h": {
        "migan_pipeline_batch_post_patches": (ci, (P(PipelineItem), ci, ci, ci, vp, vp, P(fl), vp, P(vp), P(sz), vp)),
    },
    "comodgan_u8_hip.h": {
        "comodgan_forward_u8": (ci, (vp, vp, vp, vp, vp, ci, ci, fl, ci, vp, vp, sz, vp)),
        "comodgan_forward_u8_timed": (ci, (vp, vp, vp, vp, vp, ci, ci, fl, ci, vp, vp, sz, vp, P(fl), ci)),
    },
    "migan_metrics_hip.h": {
        "migan_metrics_scratch_bytes": (sz, (P(MetricsItem), ci, ci)),
        "migan_metrics_batch": (ci, (P(MetricsItem), ci, ci, ci, ci, ci, fl, fl, vp, vp, vp, vp)),
    },
    "migan_photo_hip.h": {
        "migan_photo_scratch_bytes": (ci, (P(PhotoItem), ci, ci, ci, P(sz))),
        "migan_photo_resize_batch": (ci, (P(PhotoItem), ci, ci, ci, ci, vp, vp)),
    },
    "migan_pipeline_regions_hip.h": {
        "migan_pipeline_regions_scratch_bytes": (ci, (P(PipelineItem), ci, ci, ci, P(sz))),
        "migan_pipeline_regions_find": (ci, (P(PipelineItem), ci, ci, ci, ci, ci, P(vp), vp, vp, vp, vp)),
        "migan_pipeline_regions_pre": (ci, (P(PipelineRegionRow), ci, ci, vp, vp)),
        "migan_pipeline_regions_post": (ci, (P(PipelineRegionRow), ci, ci, vp, P(fl), vp)),
    },
    "migan_masks_hip.h": {
        "migan_masks_draw": (ci, (P(MasksRng), ci, db, ci, vp, sz, P(sz), P(MasksRng))),
        "migan_masks_raster": (ci, (vp, sz, ci, ci, vp, vp, vp)),
    },
    "migan_pipeline_region_patches_hip.h": {
        "migan_pipeline_regions_post_patches": (ci, (P(PipelineRegionRow), ci, ci, ci, vp, P(fl), P(vp), P(sz), vp)),
        "migan_pipeline_regions_paste": (ci, (P(PipelineRegionPasteRow), ci, vp)),
    },
    "migan_noise_samples_hip.h": {
        "migan_noise_floats_hw": (ci, (vp, ci, ci, P(sz))),
        "migan_workspace_bytes_samples_hw": (ci, (vp, ci, ci, ci, ci, P(sz))),
        "migan_forward_samples_hw": (ci, (vp, vp, vp, vp, ci, ci, ci, ci, vp, sz, vp)),
        "migan_sepconv_forward_samples": (ci, (P(SepConvDesc), ci, vp)),
    },
    "migan_pipeline_native_hip.h": {
        "migan_pipeline_native_pre": (ci, (P(PipelineRegionRow), ci, ci, ci, vp, vp)),
        "migan_pipeline_native_post": (ci, (P(PipelineRegionRow), ci, ci, ci, vp, P(fl), vp)),
    },
}


def exports(header: Optional[str] = None) -> tuple:
    """the entry points one header of include/ declares ("migan_photo_hip.h"), or all of them"""
    return tuple(ABI[header]) if header is not None else tuple(name for decls in ABI.values() for name in decls)


def _gauss(gauss25):
    """the 5x5 blur weights as float[25]; None: the library's own (kernel_size=5, sigma=1)"""
    return None if gauss25 is None else (C.c_float * 25)(*[float(v) for v in gauss25])


def _per_item(ctype, values, n: int, what: str, unit: str = "item"):
    """one pointer (c_void_p) or size (c_size_t) per item as an array (None passes a null table through)"""
    if values is None:
        return None
    if len(values) != n:
        raise ValueError(f"expected one {what} per {unit}, got {len(values)} for {n} {unit}s")
    return (ctype * max(1, n))(*[(v or None) if ctype is C.c_void_p else int(v) for v in values])


class MiganLib:
    """Typed view of one loaded libmigan_hip.so."""

    def __init__(self, path: Optional[str] = None, allow_test_backend: bool = False):
        """allow_test_backend: only the CPU test-suite passes True, with an explicit path, to drive the same host code + kernel
        source through the fiber emulator (tests/emu); the package itself never does, so no environment variable can make the
        product run on anything but the HIP library."""
        self.path = path or library_path()
        self.stamp_missing = False
        if not os.path.exists(self.path):
            raise MiganError(
                f"{self.path} not found: the MI355X HIP extension is not built. "
                f"Run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                f"There is no CPU/PyTorch fallback for this path.")
        # the in-tree product library must be the product build: build.py stamps it with a digest of its compile flags, and a measurement
        # build (-DMIGAN_PHASE_PROF) left under this name would otherwise be picked up silently
        if os.path.abspath(self.path) == os.path.abspath(os.path.join(_HERE, "csrc", _LIBNAME)):
            stamp = self.path + ".flags"
            if not os.path.exists(stamp):
                # build.py deletes the stamp exactly when the ISA lint has not passed (the packed-fp32 hazard): a library without
                # one is refused, not warned about -- hand builds opt out explicitly or go under another name
                if os.environ.get("MIGAN_ALLOW_UNSTAMPED") != "1":
                    raise MiganError(f"{self.path} has no build stamp ({stamp}): it was not produced by mi-gan_amd/build.py, or its ISA lint never "
                                     f"passed; rebuild with `python -c 'import __graft_entry__ as g; g.build()'` (MIGAN_ALLOW_UNSTAMPED=1 loads "
                                     f"a hand build anyway; measurement builds belong under another name via MIGAN_HIP_LIBRARY)")
                self.stamp_missing = True
            else:
                from . import build as _build
                if open(stamp).read().strip() != _build.flags_digest(()):
                    raise MiganError(f"{self.path} was not built with the product flags (stamp {stamp} differs): rebuild with "
                                     f"`python -c 'import __graft_entry__ as g; g.build()'`; measurement builds go under another name")
        try:
            self.lib = C.CDLL(self.path)
        except OSError as e:  # pragma: no cover - depends on the machine
            raise MiganError(f"cannot load {self.path}: {e}") from e
        for decls in ABI.values():
            for name, (restype, argtypes) in decls.items():
                if not hasattr(self.lib, name):
                    raise MiganError(f"{self.path} does not export {name}")
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
        if not allow_test_backend and self.backend() != PRODUCT_BACKEND:
            raise MiganError(f"{self.path} reports backend {self.backend()!r}, not {PRODUCT_BACKEND!r}: only the gfx950 HIP "
                             f"library is a product backend (the CPU emulator build is test infrastructure)")

    # -- error mapping: EINVAL -> ValueError-like, like the reference's constructor / load_state_dict
    def check(self, rc: int) -> None:
        if rc == MIGAN_OK:
            return
        msg = (self.lib.migan_last_error() or b"").decode()
        if rc == MIGAN_EINVAL:
            err: Exception = ValueError(msg)
        elif rc == MIGAN_EUNSUPPORTED:
            err = NotImplementedError(msg)
        else:
            err = MiganError(msg, rc)
        raise err

    def out(self, fn, *args, ctype=C.c_size_t):
        """fn(*args, &v) for an entry point whose last parameter is its result -> v"""
        v = ctype()
        self.check(fn(*args, C.byref(v)))
        return v.value

    def backend(self) -> str:
        return self.lib.migan_backend().decode()

    def gemm_variant(self) -> str:
        return self.lib.migan_gemm_variant().decode()

    def nan_policy(self) -> str:
        """"propagate" (default build: Tensor.clamp's behaviour, reference :21-23) or "clamp" (libmigan_hip_nanclamp.so): what lrelu_agc's clamp does with a NaN"""
        return self.lib.migan_nan_policy().decode()

    def last_kernel(self) -> str:
        """symbol of the fused-SeparableConv2d kernel this thread launched last"""
        return (self.lib.migan_last_kernel() or b"").decode()

    def set_tuning(self, key: str, value: int) -> None:
        self.check(self.lib.migan_set_tuning(key.encode(), int(value)))

    def get_tuning(self, key: str) -> int:
        """the stored value of a knob (what set_tuning normalised the request to)"""
        return self.out(self.lib.migan_get_tuning, key.encode(), ctype=C.c_int)

    def tuning_keys(self) -> list:
        """every key set_tuning / get_tuning accept"""
        keys = []
        while (k := self.lib.migan_tuning_key(len(keys))) is not None:
            keys.append(k.decode())
        return keys

    def pack_input(self, img_ptr: int, mask_ptr: int, x_ptr: int, batch: int, resolution: int, stream: int = 0) -> None:
        self.check(self.lib.migan_pack_input(C.c_void_p(img_ptr), C.c_void_p(mask_ptr), C.c_void_p(x_ptr), int(batch),
                                             int(resolution), C.c_void_p(stream)))

    def compose_output(self, y_ptr: int, img_ptr: int, mask_ptr: int, out_ptr: int, batch: int, resolution: int,
                       stream: int = 0) -> None:
        self.check(self.lib.migan_compose_output(C.c_void_p(y_ptr), C.c_void_p(img_ptr), C.c_void_p(mask_ptr),
                                                 C.c_void_p(out_ptr), int(batch), int(resolution), C.c_void_p(stream)))

    # the deployed pipeline (include/migan_hip.h, reference scripts/create_onnx_pipeline.py:118-264)
    def pipeline_mask_resize(self, mask_ptr: int, mask_height: int, mask_width: int, out_ptr: int, height: int, width: int, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_mask_resize(C.c_void_p(mask_ptr), int(mask_height), int(mask_width), C.c_void_p(out_ptr),
                                                       int(height), int(width), C.c_void_p(stream)))

    def pipeline_scratch_bytes(self, height: int, width: int) -> int:
        return self.out(self.lib.migan_pipeline_scratch_bytes, int(height), int(width))

    def pipeline_bbox(self, mask_ptr: int, height: int, width: int, resolution: int, padding: int, scratch_ptr: int, stream: int = 0):
        box = (C.c_int * 4)()
        self.check(self.lib.migan_pipeline_bbox(C.c_void_p(mask_ptr), int(height), int(width), int(resolution), int(padding),
                                                C.c_void_p(scratch_ptr), box, C.c_void_p(stream)))
        return tuple(int(v) for v in box)

    def pipeline_pre(self, image_ptr: int, mask_ptr: int, height: int, width: int, bbox, resolution: int, x_ptr: int, stream: int = 0) -> None:
        box = (C.c_int * 4)(*[int(v) for v in bbox])
        self.check(self.lib.migan_pipeline_pre(C.c_void_p(image_ptr), C.c_void_p(mask_ptr), int(height), int(width), box, int(resolution),
                                               C.c_void_p(x_ptr), C.c_void_p(stream)))

    def pipeline_post(self, image_ptr: int, mask_ptr: int, height: int, width: int, bbox, resolution: int, y_ptr: int, scratch_ptr: int,
                      gauss25=None, stream: int = 0) -> None:
        box = (C.c_int * 4)(*[int(v) for v in bbox])
        self.check(self.lib.migan_pipeline_post(C.c_void_p(image_ptr), C.c_void_p(mask_ptr), int(height), int(width), box, int(resolution),
                                                C.c_void_p(y_ptr), _gauss(gauss25), C.c_void_p(scratch_ptr), C.c_void_p(stream)))

    # the batch form: `items` = [(image_ptr, mask_ptr, height, width, mask_height, mask_width), ...]; the boxes stay on the device
    def pipeline_batch_scratch_bytes(self, items) -> int:
        return self.out(self.lib.migan_pipeline_batch_scratch_bytes, pipeline_items(items), len(items))

    def pipeline_batch_pre(self, items, resolution: int, padding: int, x_ptr: int, bbox_ptr: int, scratch_ptr: int, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_batch_pre(pipeline_items(items), len(items), int(resolution), int(padding), C.c_void_p(x_ptr),
                                                     C.c_void_p(bbox_ptr), C.c_void_p(scratch_ptr), C.c_void_p(stream)))

    def pipeline_batch_post(self, items, resolution: int, y_ptr: int, bbox_ptr: int, scratch_ptr: int, gauss25=None, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_batch_post(pipeline_items(items), len(items), int(resolution), C.c_void_p(y_ptr),
                                                      C.c_void_p(bbox_ptr), _gauss(gauss25), C.c_void_p(scratch_ptr), C.c_void_p(stream)))

    def pipeline_batch_post_samples(self, items, samples: int, resolution: int, y_ptr: int, bbox_ptr: int, scratch_ptr: int, out_ptrs,
                                    gauss25=None, stream: int = 0) -> None:
        """include/migan_pipeline_samples_hip.h: y [len(items) * samples, 3, R, R] -> out_ptrs[i] = [samples, 3, H_i, W_i] uint8, out of
        place (the images are only read); out_ptrs has one entry per item (None passes a null table through)"""
        outs = _per_item(C.c_void_p, out_ptrs, len(items), "destination")
        self.check(self.lib.migan_pipeline_batch_post_samples(pipeline_items(items), len(items), int(samples), int(resolution),
                                                              C.c_void_p(y_ptr), C.c_void_p(bbox_ptr), _gauss(gauss25), C.c_void_p(scratch_ptr),
                                                              outs, C.c_void_p(stream)))

    def pipeline_batch_post_patches(self, items, samples: int, resolution: int, y_ptr: int, bbox_ptr: int, scratch_ptr: int, out_ptrs,
                                    out_bytes, gauss25=None, stream: int = 0) -> None:
        """include/migan_pipeline_patches_hip.h: y [len(items) * samples, 3, R, R] -> out_ptrs[i] = [samples, 3, ch_i, cw_i] uint8, the
        crop of item i alone; out_bytes[i] = the capacity of out_ptrs[i] in bytes (an item that needs more is skipped).  One entry of
        each per item (None passes a null table through)"""
        outs = _per_item(C.c_void_p, out_ptrs, len(items), "destination")
        caps = _per_item(C.c_size_t, out_bytes, len(items), "capacity")
        self.check(self.lib.migan_pipeline_batch_post_patches(pipeline_items(items), len(items), int(samples), int(resolution),
                                                              C.c_void_p(y_ptr), C.c_void_p(bbox_ptr), _gauss(gauss25), C.c_void_p(scratch_ptr),
                                                              outs, caps, C.c_void_p(stream)))

    # one crop per hole region (include/migan_pipeline_regions_hip.h): `items` as for the batch form; `rows` =
    # [(image_ptr, mask_ptr, labels_ptr or None, height, width, label, box), ...], the mask at the image's size
    def pipeline_regions_scratch_bytes(self, items, gap: int, max_regions: int) -> int:
        return self.out(self.lib.migan_pipeline_regions_scratch_bytes, pipeline_items(items), len(items), int(gap), int(max_regions))

    def pipeline_regions_find(self, items, resolution: int, padding: int, gap: int, max_regions: int, label_ptrs, count_ptr: int,
                              boxes_ptr: int, scratch_ptr: int, stream: int = 0) -> None:
        """label_ptrs[i] -> uint8 [H_i, W_i]; count int32 [n]; boxes int32 [n, max_regions + 1, 4], slot 0 = the single box"""
        labels = _per_item(C.c_void_p, label_ptrs, len(items), "label map")
        self.check(self.lib.migan_pipeline_regions_find(pipeline_items(items), len(items), int(resolution), int(padding), int(gap),
                                                        int(max_regions), labels, C.c_void_p(count_ptr), C.c_void_p(boxes_ptr),
                                                        C.c_void_p(scratch_ptr), C.c_void_p(stream)))

    def pipeline_regions_pre(self, rows, resolution: int, x_ptr: int, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_regions_pre(pipeline_region_rows(rows), 0 if rows is None else len(rows), int(resolution),
                                                       C.c_void_p(x_ptr), C.c_void_p(stream)))

    def pipeline_regions_post(self, rows, resolution: int, y_ptr: int, gauss25=None, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_regions_post(pipeline_region_rows(rows), 0 if rows is None else len(rows), int(resolution),
                                                        C.c_void_p(y_ptr), _gauss(gauss25), C.c_void_p(stream)))

    # S completions per hole region as patches, and the paste back (include/migan_pipeline_region_patches_hip.h)
    def pipeline_regions_post_patches(self, rows, samples: int, resolution: int, y_ptr: int, out_ptrs, out_bytes, gauss25=None,
                                      stream: int = 0) -> None:
        """rows as for pipeline_regions_post (the images are only read); y [len(rows) * samples, 3, R, R], row r * samples + s = sample s
        of rows[r] -> out_ptrs[r] = [samples, 3, ch_r, cw_r] uint8, the box of row r: the blended bytes where labels == label, the
        image's elsewhere; out_bytes[r] = the capacity of out_ptrs[r] in bytes (too small: ValueError, nothing launched).  One entry
        of each per row (None passes a null table through)"""
        n = 0 if rows is None else len(rows)
        outs = _per_item(C.c_void_p, out_ptrs, n, "destination", "row")
        caps = _per_item(C.c_size_t, out_bytes, n, "capacity", "row")
        self.check(self.lib.migan_pipeline_regions_post_patches(pipeline_region_rows(rows), n, int(samples), int(resolution),
                                                                C.c_void_p(y_ptr), _gauss(gauss25), outs, caps, C.c_void_p(stream)))

    def pipeline_regions_paste(self, rows, stream: int = 0) -> None:
        """rows = [(image_ptr, labels_ptr or None, patch_ptr, height, width, label, box), ...]: patch_ptr -> ONE sample [3, ch, cw] of the
        row's patches; it is copied into the image where labels == label (label 0: the whole box)"""
        self.check(self.lib.migan_pipeline_regions_paste(pipeline_region_paste_rows(rows), 0 if rows is None else len(rows),
                                                         C.c_void_p(stream)))

    # crops at native size (include/migan_pipeline_native_hip.h): rows as for pipeline_regions_pre, the box = the part of the
    # [height, width] network window inside the photo; x [len(rows), 4, height, width], y [len(rows), 3, height, width]
    def pipeline_native_pre(self, rows, height: int, width: int, x_ptr: int, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_native_pre(pipeline_region_rows(rows), 0 if rows is None else len(rows), int(height), int(width),
                                                      C.c_void_p(x_ptr), C.c_void_p(stream)))

    def pipeline_native_post(self, rows, height: int, width: int, y_ptr: int, gauss25=None, stream: int = 0) -> None:
        self.check(self.lib.migan_pipeline_native_post(pipeline_region_rows(rows), 0 if rows is None else len(rows), int(height), int(width),
                                                       C.c_void_p(y_ptr), _gauss(gauss25), C.c_void_p(stream)))

    # PSNR / SSIM of completions against the photo (include/migan_metrics_hip.h): `items` = [(gt_ptr, pred_ptr, mask_ptr or None, H, W), ...]
    def metrics_scratch_bytes(self, items, samples: int) -> int:
        n = self.lib.migan_metrics_scratch_bytes(metrics_items(items), 0 if items is None else len(items), int(samples))
        if n == 0:
            raise ValueError((self.lib.migan_last_error() or b"").decode())
        return int(n)

    def metrics_batch(self, items, samples: int, dtype: int, layout: int, shave: int, lo: float, hi: float, scratch_ptr: int,
                      out_mse_ptr: int, out_ssim_ptr: int, stream: int = 0) -> None:
        """out_mse / out_ssim: device float64 [len(items) * samples], row i * samples + s = sample s of item i"""
        self.check(self.lib.migan_metrics_batch(metrics_items(items), 0 if items is None else len(items), int(samples), int(dtype), int(layout),
                                                int(shave), C.c_float(lo), C.c_float(hi), C.c_void_p(scratch_ptr), C.c_void_p(out_mse_ptr),
                                                C.c_void_p(out_ssim_ptr), C.c_void_p(stream)))

    # Pillow-exact resize of uint8 images (include/migan_photo_hip.h): `items` = [(src_ptr, dst_ptr, src_h, src_w, dst_h, dst_w), ...]
    def photo_scratch_bytes(self, items, channels: int, filter: int) -> int:
        return self.out(self.lib.migan_photo_scratch_bytes, photo_items(items), 0 if items is None else len(items), int(channels), int(filter))

    def photo_resize_batch(self, items, channels: int, filter: int, flags: int, scratch_ptr: int, stream: int = 0) -> None:
        self.check(self.lib.migan_photo_resize_batch(photo_items(items), 0 if items is None else len(items), int(channels), int(filter), int(flags),
                                                     C.c_void_p(scratch_ptr), C.c_void_p(stream)))

    # the reference's RandomMask (include/migan_masks_hip.h).  masks_draw is host code: it needs no device
    def masks_draw(self, rng: MasksRng, resolution: int, coef: float, count: int, plans_ptr: int = 0, capacity_words: int = 0, states=None) -> int:
        """draws `count` candidates, advancing `rng` in place; -> the words written to the plan buffer (0 for a null buffer).
        `states`: a (MasksRng * count)() array that receives the generator behind every candidate"""
        used = C.c_size_t(0)
        self.check(self.lib.migan_masks_draw(C.byref(rng) if rng is not None else None, int(resolution), C.c_double(coef), int(count),
                                             C.c_void_p(plans_ptr or None), int(capacity_words), C.byref(used), states))
        return int(used.value)

    def masks_raster(self, plans_ptr: int, words: int, count: int, resolution: int, out_ptr: int, holes_ptr: int, stream: int = 0) -> None:
        self.check(self.lib.migan_masks_raster(C.c_void_p(plans_ptr or None), int(words), int(count), int(resolution), C.c_void_p(out_ptr or None),
                                               C.c_void_p(holes_ptr or None), C.c_void_p(stream)))

    def sepconv_forward(self, stream: int = 0, samples: Optional[int] = None, **kw) -> None:
        """samples: migan_sepconv_forward_samples -- noise_const is [batch][res_out][width_out] (one plane per row), skip [batch / samples]..."""
        d = SepConvDesc()
        for f, _ in SepConvDesc._fields_:
            setattr(d, f, kw.pop(f, None if f not in ("batch", "cin", "cout", "res_in", "down", "up", "scratch_bytes", "wsplit_bytes",
                                                      "gemm", "dtype", "width_in") else (-1 if f == "gemm" else 0)))
        if kw:
            raise TypeError(f"unknown sepconv fields: {sorted(kw)}")
        d.down = d.down or 1
        d.up = d.up or 1
        if samples is not None:
            self.check(self.lib.migan_sepconv_forward_samples(C.byref(d), int(samples), C.c_void_p(stream)))
            return
        self.check(self.lib.migan_sepconv_forward(C.byref(d), C.c_void_p(stream)))


class _Handle:
    """What ``migan_handle*`` and ``comodgan_handle*`` have in common: the same entry points up to their prefix."""
    _prefix = ""
    _launch_ints: Tuple[str, ...] = ()      # int results of <prefix>launch_info behind the three doubles

    def _fn(self, name: str):
        return getattr(self.lib.lib, self._prefix + name)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def weights(self) -> List[Tuple[str, Tuple[int, ...], bool]]:
        out = []
        for i in range(self.lib.out(self._fn("num_weights"), self._h, ctype=C.c_int)):
            name = C.c_char_p()
            shape = (C.c_int64 * 4)()
            nd, isb = C.c_int(), C.c_int()
            self.lib.check(self._fn("weight_info")(self._h, i, C.byref(name), shape, C.byref(nd), C.byref(isb)))
            out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value)), bool(isb.value)))
        return out

    def set_weight(self, name: str, ptr: int, shape: Sequence[int]) -> None:
        arr = (C.c_int64 * max(1, len(shape)))(*[int(s) for s in shape])
        self.lib.check(self._fn("set_weight")(self._h, name.encode(), C.c_void_p(ptr), arr, len(shape)))

    def commit(self, stream: int = 0) -> None:
        self.lib.check(self._fn("commit")(self._h, C.c_void_p(stream)))

    def workspace_bytes(self, batch: int) -> int:
        return self.lib.out(self._fn("workspace_bytes"), self._h, int(batch))

    def assume_static_weights(self, on: bool) -> None:
        self.lib.check(self._fn("assume_static_weights")(self._h, 1 if on else 0))

    def set_debug(self, keep: bool) -> None:
        self.lib.check(self._fn("set_debug")(self._h, 1 if keep else 0))

    def launches(self) -> List[Dict]:
        out = []
        for i in range(self.lib.out(self._fn("num_launches"), self._h, ctype=C.c_int)):
            layer, kern = C.c_char_p(), C.c_char_p()
            fl, mf, by = C.c_double(), C.c_double(), C.c_double()
            ints = [C.c_int() for _ in self._launch_ints]
            self.lib.check(self._fn("launch_info")(self._h, i, *[C.byref(v) for v in (layer, kern, fl, mf, by, *ints)]))
            out.append(dict(layer=layer.value.decode(), kernel=kern.value.decode(), flops=fl.value, mfma_flops=mf.value, bytes=by.value,
                            **{k: v.value for k, v in zip(self._launch_ints, ints)}))
        return out

    def _timed(self, fn, args) -> List[float]:
        """fn(*args, launch_ms, n): the milliseconds of every launch of the plan launches() describes"""
        n = len(self.launches())
        ms = (C.c_float * n)()
        self.lib.check(fn(*args, ms, n))
        return [float(v) for v in ms]


class MiganHandle(_Handle):
    """RAII wrapper of ``migan_handle*`` (one Generator(resolution) instance)."""
    _prefix = "migan_"
    _launch_ints = ("workgroups_batch1",)

    def __init__(self, lib: MiganLib, resolution: int, device: int = 0, dtype=0):
        self.lib = lib
        self._h = C.c_void_p()
        self.dtype = dtype_code(dtype)
        lib.check(lib.lib.migan_create(int(resolution), self.dtype, int(device), C.byref(self._h)))
        self.resolution = int(resolution)

    # -- per-handle options
    def set_gemm(self, variant) -> None:
        code = GEMMS[variant] if isinstance(variant, str) else int(variant)
        if code < 0:
            # MIGAN_GEMM_DEFAULT: what migan_create picks for this storage format (f16x2 for fp32 storage unless MIGAN_GEMM says
            # otherwise, f16 for 16-bit storage)
            code = GEMMS[self.lib.lib.migan_gemm_variant().decode()] if self.dtype == 0 else GEMMS["f16"]
        self.lib.check(self.lib.lib.migan_set_gemm(self._h, code))

    def gemm(self) -> str:
        return GEMM_NAMES[self.lib.out(self.lib.lib.migan_get_gemm, self._h, ctype=C.c_int)]

    def set_streams(self, n: int) -> None:
        self.lib.check(self.lib.lib.migan_set_streams(self._h, int(n)))

    def forward(self, x_ptr: int, y_ptr: int, batch: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
        self.lib.check(self.lib.lib.migan_forward(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), int(batch),
                                                  C.c_void_p(ws_ptr), C.c_size_t(ws_bytes), C.c_void_p(stream)))

    def forward_split(self, batch: int) -> List[int]:
        """images per sub-batch of a forward of `batch` images (migan_forward_split)"""
        n, parts = (C.c_int * 4)(), C.c_int()
        self.lib.check(self.lib.lib.migan_forward_split(self._h, int(batch), n, C.byref(parts)))
        return [int(n[k]) for k in range(parts.value)]

    def forward_parts(self, x_ptr: int, y_ptrs: List[int], batch: int, ws_ptr: int, ws_bytes: int, stream: int, part_streams: List[int]) -> List[int]:
        """migan_forward_parts: sub-batch k -> y_ptrs[k]; sub-batch k >= 1 on the caller's stream part_streams[k - 1]; streams are not joined"""
        ys = (C.c_void_p * 4)(*([C.c_void_p(p) for p in y_ptrs] + [C.c_void_p(0)] * (4 - len(y_ptrs))))
        st = (C.c_void_p * 4)(*([C.c_void_p(p) for p in part_streams] + [C.c_void_p(0)] * (4 - len(part_streams))))
        n, parts = (C.c_int * 4)(), C.c_int()
        self.lib.check(self.lib.lib.migan_forward_parts(self._h, C.c_void_p(x_ptr), ys, int(batch), C.c_void_p(ws_ptr), C.c_size_t(ws_bytes),
                                                        C.c_void_p(stream), st, len(part_streams), n, C.byref(parts)))
        return [int(n[k]) for k in range(parts.value)]

    def workspace_bytes_hw(self, batch: int, height: int, width: int) -> int:
        return self.lib.out(self.lib.lib.migan_workspace_bytes_hw, self._h, int(batch), int(height), int(width))

    def forward_hw(self, x_ptr: int, y_ptr: int, batch: int, height: int, width: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
        self.lib.check(self.lib.lib.migan_forward_hw(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), int(batch), int(height), int(width),
                                                     C.c_void_p(ws_ptr), C.c_size_t(ws_bytes), C.c_void_p(stream)))

    def noise_floats_hw(self, height: int, width: int) -> int:
        return self.lib.out(self.lib.lib.migan_noise_floats_hw, self._h, int(height), int(width))

    def workspace_bytes_samples_hw(self, n_images: int, samples: int, height: int, width: int) -> int:
        return self.lib.out(self.lib.lib.migan_workspace_bytes_samples_hw, self._h, int(n_images), int(samples), int(height), int(width))

    def forward_samples_hw(self, x_ptr: int, noise_ptr: int, y_ptr: int, n_images: int, samples: int, height: int, width: int, ws_ptr: int,
                           ws_bytes: int, stream: int = 0) -> None:
        self.lib.check(self.lib.lib.migan_forward_samples_hw(self._h, C.c_void_p(x_ptr), C.c_void_p(noise_ptr), C.c_void_p(y_ptr), int(n_images),
                                                             int(samples), int(height), int(width), C.c_void_p(ws_ptr), int(ws_bytes),
                                                             C.c_void_p(stream)))

    def forward_u8(self, img_ptr: int, mask_ptr: int, out_ptr: int, batch: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
        self.lib.check(self.lib.lib.migan_forward_u8(self._h, C.c_void_p(img_ptr), C.c_void_p(mask_ptr), C.c_void_p(out_ptr), int(batch),
                                                     C.c_void_p(ws_ptr), C.c_size_t(ws_bytes), C.c_void_p(stream)))

    def forward_timed(self, x_ptr: int, y_ptr: int, batch: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> List[float]:
        return self._timed(self.lib.lib.migan_forward_timed, [self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), int(batch), C.c_void_p(ws_ptr),
                                                              C.c_size_t(ws_bytes), C.c_void_p(stream)])

    def debug_tensor(self, batch: int, layer: str) -> Tuple[int, Tuple[int, ...]]:
        off = C.c_size_t()
        shape = (C.c_int64 * 4)()
        self.lib.check(self.lib.lib.migan_debug_tensor(self._h, int(batch), layer.encode(), C.byref(off), shape))
        return int(off.value), tuple(int(s) for s in shape)

    def debug_tensor_hw(self, batch: int, height: int, width: int, layer: str) -> Tuple[int, Tuple[int, ...]]:
        """debug_tensor for the plan of forward_hw at height x width"""
        off = C.c_size_t()
        shape = (C.c_int64 * 4)()
        self.lib.check(self.lib.lib.migan_debug_tensor_hw(self._h, int(batch), int(height), int(width), layer.encode(), C.byref(off), shape))
        return int(off.value), tuple(int(s) for s in shape)


class CoModGANHandle(_Handle):
    """RAII wrapper of ``comodgan_handle*`` (one CoModGANGenerator(mapping, encoder, synthesis) instance)."""
    _prefix = "comodgan_"

    def __init__(self, lib: MiganLib, resolution: int, num_ws: int, ch_base: int = 32768, ch_max: int = 512, z_dim: int = 512,
                 w_dim: int = 512, w0_dim: int = 1024, map_layers: int = 8, device: int = 0):
        self.lib = lib
        self._h = C.c_void_p()
        self.cfg = CoModGANConfig(int(resolution), int(ch_base), int(ch_max), int(z_dim), int(w_dim), int(w0_dim), int(map_layers),
                                  int(num_ws))
        lib.check(lib.lib.comodgan_create(C.byref(self.cfg), int(device), C.byref(self._h)))

    def workspace_bytes_samples(self, batch: int, samples: int) -> int:
        return self.lib.out(self.lib.lib.comodgan_workspace_bytes_samples, self._h, int(batch), int(samples))

    def noise_floats(self) -> int:
        return self.lib.out(self.lib.lib.comodgan_noise_floats, self._h)

    def _forward(self, fn, fn_timed, tensors, counts, plan, ws_ptr, ws_bytes, truncation_psi, noise_mode, noise_ptr, stream, timed):
        """the three forwards: fn(h, *tensors, *counts, psi, noise mode, noise, workspace, bytes, stream); timed: fn_timed with the
        milliseconds of every launch behind them.  plan: None, or the (batch, samples) whose plan launches() is to describe"""
        if noise_mode not in NOISE_MODES:
            raise AssertionError(noise_mode)             # stylegan.py:280
        args = [self._h, *[C.c_void_p(p) for p in tensors], *[int(c) for c in counts], C.c_float(truncation_psi), NOISE_MODES[noise_mode],
                C.c_void_p(noise_ptr), C.c_void_p(ws_ptr), C.c_size_t(ws_bytes), C.c_void_p(stream)]
        if not timed:
            self.lib.check(fn(*args))
            return None
        if plan is not None:
            self.workspace_bytes_samples(*plan)          # launches() describes the plan made last: make it this one
        return self._timed(fn_timed, args)

    def forward(self, x_ptr: int, z_ptr: int, y_ptr: int, batch: int, ws_ptr: int, ws_bytes: int, truncation_psi: float = 1.0,
                noise_mode: str = "const", noise_ptr: Optional[int] = None, stream: int = 0, timed: bool = False):
        return self._forward(self.lib.lib.comodgan_forward, self.lib.lib.comodgan_forward_timed, (x_ptr, z_ptr, y_ptr), (batch,), None,
                             ws_ptr, ws_bytes, truncation_psi, noise_mode, noise_ptr, stream, timed)

    def forward_samples(self, x_ptr: int, z_ptr: int, y_ptr: int, batch: int, samples: int, ws_ptr: int, ws_bytes: int,
                        truncation_psi: float = 1.0, noise_mode: str = "const", noise_ptr: Optional[int] = None, stream: int = 0,
                        timed: bool = False):
        """x [batch,4,R,R], z [batch*samples,z_dim] -> y [batch*samples,3,R,R] (image-major): the encoder once per image"""
        return self._forward(self.lib.lib.comodgan_forward_samples, self.lib.lib.comodgan_forward_samples_timed, (x_ptr, z_ptr, y_ptr),
                             (batch, samples), (batch, samples), ws_ptr, ws_bytes, truncation_psi, noise_mode, noise_ptr, stream, timed)

    def forward_u8(self, img_ptr: int, mask_ptr: int, z_ptr: int, out_ptr: int, batch: int, samples: int, ws_ptr: int, ws_bytes: int,
                   truncation_psi: float = 1.0, noise_mode: str = "const", noise_ptr: Optional[int] = None, stream: int = 0,
                   timed: bool = False):
        """include/comodgan_u8_hip.h: uint8 img [batch,R,R,3] and mask [batch,R,R] (255 = known), z [batch*samples,z_dim] -> uint8
        out [batch*samples,R,R,3], row i * samples + s composed over photo i; a workspace of workspace_bytes_samples(batch, samples).
        (The uint8 plan has the launches of the fp32-I/O plan, two of them under other names.)"""
        return self._forward(self.lib.lib.comodgan_forward_u8, self.lib.lib.comodgan_forward_u8_timed, (img_ptr, mask_ptr, z_ptr, out_ptr),
                             (batch, samples), (batch, samples), ws_ptr, ws_bytes, truncation_psi, noise_mode, noise_ptr, stream, timed)

    # -- include/comodgan_stages_hip.h: the three stages as calls of their own, stage tensors in caller memory
    def levels(self) -> int:
        """feature resolutions 4 ... R"""
        return int(self.cfg.resolution).bit_length() - 2

    def _level_ptrs(self, ptrs, what: str):
        if ptrs is None:
            return None
        if len(ptrs) != self.levels():
            raise ValueError(f"{what}: expected {self.levels()} pointers (res 4 ... {self.cfg.resolution}), got {len(ptrs)}")
        return (C.c_void_p * len(ptrs))(*[C.c_void_p(p) if p else None for p in ptrs])

    def stages_workspace_bytes(self, batch: int, samples: int = 1) -> int:
        return self.lib.out(self.lib.lib.comodgan_stages_workspace_bytes, self._h, int(batch), int(samples))

    def mapping(self, z_ptr: int, ws_rows_ptr: int, rows: int, ws_ptr: int, ws_bytes: int, truncation_psi: float = 1.0,
                truncation_cutoff: Optional[int] = None, stream: int = 0) -> None:
        self.lib.check(self.lib.lib.comodgan_mapping(self._h, C.c_void_p(z_ptr), C.c_void_p(ws_rows_ptr), int(rows), float(truncation_psi),
                                                     -1 if truncation_cutoff is None else int(truncation_cutoff), C.c_void_p(ws_ptr), ws_bytes,
                                                     C.c_void_p(stream)))

    def encode(self, x_ptr: int, w0_ptr: int, feat_ptrs: Sequence[int], batch: int, ws_ptr: int, ws_bytes: int, stream: int = 0) -> None:
        """feat_ptrs: NHWC tensors for res 4, 8, ..., R"""
        self.lib.check(self.lib.lib.comodgan_encode(self._h, C.c_void_p(x_ptr), C.c_void_p(w0_ptr), self._level_ptrs(feat_ptrs, "feats"), int(batch),
                                                    C.c_void_p(ws_ptr), ws_bytes, C.c_void_p(stream)))

    def synthesize(self, w0_ptr: int, feat_ptrs: Sequence[int], ws_rows_ptr: int, y_ptr: int, batch: int, samples: int, ws_ptr: int, ws_bytes: int,
                   noise_mode: str = "const", noise_ptr: Optional[int] = None, to_rgb_ptrs: Optional[Sequence[int]] = None,
                   res_img_ptrs: Optional[Sequence[int]] = None, stream: int = 0) -> None:
        """to_rgb_ptrs / res_img_ptrs: None, or one pointer (or 0) per res 4, 8, ..., R"""
        self.lib.check(self.lib.lib.comodgan_synthesize(
            self._h, C.c_void_p(w0_ptr), self._level_ptrs(feat_ptrs, "feats"), C.c_void_p(ws_rows_ptr), C.c_void_p(y_ptr), int(batch), int(samples),
            NOISE_MODES[noise_mode], C.c_void_p(noise_ptr) if noise_ptr else None, self._level_ptrs(to_rgb_ptrs, "to_rgb"),
            self._level_ptrs(res_img_ptrs, "res_img"), C.c_void_p(ws_ptr), ws_bytes, C.c_void_p(stream)))

    def weight_preparations(self) -> int:
        return self.lib.out(self.lib.lib.comodgan_weight_preparations, self._h, ctype=C.c_ulonglong)

    def set_truncation_cutoff(self, cutoff: Optional[int]) -> None:
        """None: truncation_psi applies to every row of ws; n: to rows [0, n) only (stylegan.py:432-437)"""
        self.lib.check(self.lib.lib.comodgan_set_truncation_cutoff(self._h, -1 if cutoff is None else int(cutoff)))

    def set_fp16_blocks(self, encoder_before_res: Optional[int], synthesis_after_res: Optional[int]) -> None:
        """the reference's use_fp16_before_res / use_fp16_after_res (comodgan.py:148,384); None marks no block.  Before sizing the workspace."""
        self.lib.check(self.lib.lib.comodgan_set_fp16_blocks(self._h, -1 if encoder_before_res is None else int(encoder_before_res),
                                                             -1 if synthesis_after_res is None else int(synthesis_after_res)))

    def fp16_blocks(self) -> Tuple[Optional[int], Optional[int]]:
        e, s = C.c_int(), C.c_int()
        self.lib.check(self.lib.lib.comodgan_get_fp16_blocks(self._h, C.byref(e), C.byref(s)))
        return (None if e.value < 0 else e.value, None if s.value < 0 else s.value)

    def set_fp16_storage(self, on: bool = True) -> None:
        """the blocks marked through set_fp16_blocks store their activations in fp16 (include/comodgan_fp16_storage_hip.h).  Before
        sizing the workspace."""
        self.lib.check(self.lib.lib.comodgan_set_fp16_storage(self._h, 1 if on else 0))

    def get_fp16_storage(self) -> bool:
        return bool(self.lib.out(self.lib.lib.comodgan_get_fp16_storage, self._h, ctype=C.c_int))

    def debug_tensor(self, batch: int, layer: str) -> Tuple[int, Tuple[int, ...]]:
        off = C.c_size_t()
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        self.lib.check(self.lib.lib.comodgan_debug_tensor(self._h, int(batch), layer.encode(), C.byref(off), shape, C.byref(nd)))
        return int(off.value), tuple(int(shape[k]) for k in range(nd.value))

    def debug_tensor_samples(self, batch: int, samples: int, layer: str) -> Tuple[int, Tuple[int, ...]]:
        off = C.c_size_t()
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        self.lib.check(self.lib.lib.comodgan_debug_tensor_samples(self._h, int(batch), int(samples), layer.encode(), C.byref(off), shape,
                                                                  C.byref(nd)))
        return int(off.value), tuple(int(shape[k]) for k in range(nd.value))

    def debug_tensor_dtype(self, batch: int, layer: str, samples: int = 1) -> int:
        """COMODGAN_DTYPE_F32 or COMODGAN_DTYPE_F16: how the debug tensor is stored in the workspace"""
        return self.lib.out(self.lib.lib.comodgan_debug_tensor_dtype, self._h, int(batch), int(samples), layer.encode(), ctype=C.c_int)

    def read_debug_tensor(self, ws_bytes, batch: int, layer: str, samples: int = 1):
        """A debug tensor as a float32 numpy array, whatever its stored type.  ws_bytes: the workspace after a forward of this plan
        as a flat uint8 numpy array in host memory (the caller copies it back from the device)."""
        import numpy as np
        off, shape = self.debug_tensor_samples(batch, samples, layer)
        half = self.debug_tensor_dtype(batch, layer, samples) == COMODGAN_DTYPE_F16
        n = 1
        for d in shape:
            n *= d
        raw = np.ascontiguousarray(ws_bytes).view(np.uint8).reshape(-1)[off:off + n * (2 if half else 4)]
        return raw.view(np.float16 if half else np.float32).reshape(shape).astype(np.float32)


_LIB: Optional[MiganLib] = None


_CLAMP_LIB: Optional["MiganLib"] = None


def load_library(path: Optional[str] = None, nan_policy: str = "propagate") -> MiganLib:
    """Process-wide libmigan_hip.so (raises MiganError when it is not built).  nan_policy="propagate" (default): a NaN activation stays a NaN
    through lrelu_agc's clamp, like Tensor.clamp in the reference module; "clamp": the build of the same library without that repair
    (libmigan_hip_nanclamp.so, -DMIGAN_NAN_CLAMP: v_med3_f32 turns a NaN into -256, ~2 % faster)."""
    global _LIB, _CLAMP_LIB
    if nan_policy not in ("clamp", "propagate"):
        raise ValueError(f"nan_policy must be 'clamp' or 'propagate', got {nan_policy!r}")
    if path is not None:
        return MiganLib(path)
    if nan_policy == "clamp":
        if _CLAMP_LIB is None:
            _CLAMP_LIB = MiganLib(os.path.join(_HERE, "csrc", "libmigan_hip_nanclamp.so"))
            if _CLAMP_LIB.nan_policy() != "clamp":
                raise MiganError("libmigan_hip_nanclamp.so was not built with -DMIGAN_NAN_CLAMP")
        return _CLAMP_LIB
    if _LIB is None:
        _LIB = MiganLib()
    return _LIB

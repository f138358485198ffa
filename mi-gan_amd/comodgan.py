"""Drop-in for ``lib.model_zoo.comodgan`` of Picsart-AI-Research/MI-GAN.

``Generator(Mapping(num_ws), Encoder(resolution), Synthesis(resolution))`` -- the way the reference's
scripts/demo.py:95-106 assembles ``comodgan-256|512`` -- keeps the reference's constructors, sub-module tree /
``state_dict`` schema (``load_state_dict(torch.load(path))``, demo.py:110) and ``forward`` contract
(comodgan.py:435-455), but ``Generator.forward`` is one call into the MI355X HIP library through the C ABI
(include/comodgan_hip.h).  The three sub-modules of a ``Generator`` are callable with the reference's signatures as well
(include/comodgan_stages_hip.h): ``G.mapping(z)`` -> ws, ``G.encoder(img)`` -> (x, feats), ``G.synthesis(x, feats, ws)`` -> img, with the
stage tensors in torch memory -- encode once and complete later, edit ws, read the per-resolution ToRGB outputs
(``return_intermediate_outs=True``).  PyTorch is used for device memory, streams and drawing ``z`` / the per-pixel noise of
``noise_mode='random'`` only.  There is no CPU or pure-PyTorch path: a CPU tensor, a missing libmigan_hip.so or
a missing GPU raises.  ``Encoder(use_fp16_before_res=)`` / ``Synthesis(use_fp16_after_res=)`` mark half-precision blocks as
in the reference: their 3x3 convolutions take fp16 operands (fp32 accumulation and storage; ``Generator.set_fp16_storage()``
makes those blocks store their activations in fp16 as well, as the reference does).  Not supported: autograd,
``c`` (class conditioning: c_dim = 0 in every reference config), ``return_intermediate_outs`` on ``Generator.forward`` (the fused call
keeps no per-resolution image; ``G.synthesis(..., return_intermediate_outs=True)`` is where the reference defines them).
"""
from __future__ import annotations

import operator
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import comodgan_schema as cs
from .hipbind import CoModGANHandle, MiganLib, load_library


version = '3'          # reference comodgan.py:10-11 (lib/model_zoo/__init__.py imports `version` from this module)
symbol = 'comodgan'


class _Node(nn.Module):
    def __init__(self, kind: str = "Module"):
        super().__init__()
        self._kind = kind

    def _get_name(self):
        return self._kind

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{self._kind}: on the MI355X HIP path only comodgan.Generator and the Mapping / Encoder / Synthesis of a "
                                  "Generator compute; other sub-modules hold the reference-named parameters")

    def _generator(self) -> "Generator":
        """The Generator this stage belongs to: it owns the handle, the workspace and the weight binding.  Kept in a tuple in the instance
        dict, so that it is no registered sub-module (no cycle in modules() / state_dict()) and copies follow it."""
        owner = self.__dict__.get("_owner")
        if owner is None:
            raise NotImplementedError(f"{self._kind}: a stage computes as part of a comodgan.Generator (which owns the HIP handle and the "
                                      "weight binding); stand-alone it holds the reference-named parameters")
        return owner[0]


def _init_tensor(e: cs.Entry) -> torch.Tensor:
    """Constructor-time values of the reference layers (stylegan.py:79-80,213-215,273,275-276,393)."""
    if e.role in ("conv_w", "rgb_w", "affine_w"):
        return torch.randn(e.shape)
    if e.role == "dense_w":
        return torch.randn(e.shape) / (0.01 if e.name.startswith("mapping.") else 1.0)
    if e.role in ("conv_b", "rgb_b", "dense_b", "w_avg"):
        return torch.zeros(e.shape)
    if e.role == "affine_b":
        return torch.ones(e.shape)
    if e.role == "noise_strength":
        return torch.zeros(())
    if e.role == "noise_const":
        return torch.randn(e.shape)
    if e.role == "fir":
        return torch.tensor(cs.fir_kernel_2d())
    raise AssertionError(e.role)


def _populate(root: nn.Module, prefix: str, cfg: cs.Config) -> None:
    for e in cs.entries(cfg):
        if not e.name.startswith(prefix + "."):
            continue
        node: nn.Module = root
        parts = e.name[len(prefix) + 1:].split(".")
        for p in parts[:-1]:
            if not hasattr(node, p):
                node.add_module(p, _Node(p))
            node = getattr(node, p)
        t = _init_tensor(e)
        if e.kind == "param":
            node.register_parameter(parts[-1], nn.Parameter(t))
        else:
            node.register_buffer(parts[-1], t)


def _fp16_res(name: str, value) -> Optional[int]:
    """use_fp16_before_res / use_fp16_after_res: None (no half-precision block) or a non-negative integer resolution"""
    if value is None:
        return None
    try:
        res = None if isinstance(value, bool) else operator.index(value)
    except TypeError:
        res = None
    if res is None or res < 0:
        raise ValueError(f"{name} must be None or a non-negative integer, got {value!r}")
    return res


class Mapping(_Node):
    """stylegan.py:356-439 (c_dim = 0).  Callable as the ``mapping`` of a Generator."""

    def __init__(self, z_dim: int = 512, c_dim: int = 0, w_dim: int = 512, num_ws: int = 14, num_layers: int = 8, **unused):
        super().__init__("Mapping")
        if c_dim:
            raise NotImplementedError("class-conditional mapping (c_dim > 0) is not part of the inference path")
        self.z_dim, self.c_dim, self.w_dim, self.num_ws, self.num_layers = z_dim, c_dim, w_dim, num_ws, num_layers
        _populate(self, "mapping", cs.Config(resolution=8, z_dim=z_dim, w_dim=w_dim, map_layers=num_layers, num_ws=num_ws))

    def forward(self, z, c=None, truncation_psi=1, truncation_cutoff=None, skip_w_avg_update=False):
        """z [N, z_dim] -> ws [N, num_ws, w_dim] (stylegan.py:402-439): rows below the cutoff truncated, the others raw."""
        return self._generator()._stage_mapping(z, c, truncation_psi, truncation_cutoff)


class Encoder(_Node):
    """comodgan.py:114-204."""

    def __init__(self, resolution: int = 256, ic_n: int = 4, oc_n: int = 1024, ch_base: int = 32768, ch_max: int = 512,
                 use_fp16_before_res: Optional[int] = None, **unused):
        super().__init__("Encoder")
        self.use_fp16_before_res = _fp16_res("use_fp16_before_res", use_fp16_before_res)    # blocks b<res>, res > it (comodgan.py:148)
        if ic_n != 4:
            raise NotImplementedError("the inference path takes 4 input channels (mask, rgb)")
        cfg = cs.Config(resolution=resolution, ch_base=ch_base, ch_max=ch_max, w0_dim=oc_n)
        cs.check_config(cfg)                                     # ValueError like comodgan.py:134-135
        self.resolution, self.ic_n, self.oc_n, self.ch_base, self.ch_max = resolution, ic_n, oc_n, ch_base, ch_max
        _populate(self, "encoder", cfg)

    def forward(self, img, c=None):
        """img [N, 4, R, R] -> (x [N, oc_n], feats {res: [N, C_res, res, res]}) (comodgan.py:190-204).  The feature tensors are
        channels_last (the kernels' NHWC layout under an NCHW shape); float16 for the blocks that store fp16 (set_fp16_storage)."""
        return self._generator()._stage_encoder(img, c)


class Synthesis(_Node):
    """comodgan.py:346-420."""

    def __init__(self, w_dim: int = 512, w0_dim: int = 1024, resolution: int = 256, rgb_n: int = 3, ch_base: int = 32768,
                 ch_max: int = 512, use_fp16_after_res: Optional[int] = None, **unused):
        super().__init__("Synthesis")
        self.use_fp16_after_res = _fp16_res("use_fp16_after_res", use_fp16_after_res)       # blocks b<res>, res > it (comodgan.py:384)
        if rgb_n != 3:
            raise NotImplementedError("rgb_n must be 3")
        cfg = cs.Config(resolution=resolution, ch_base=ch_base, ch_max=ch_max, w_dim=w_dim, w0_dim=w0_dim)
        cs.check_config(cfg)                                     # ValueError like comodgan.py:358-359
        self.w_dim, self.w0_dim, self.resolution, self.rgb_n, self.ch_base, self.ch_max = w_dim, w0_dim, resolution, rgb_n, ch_base, ch_max
        self.num_ws = cs.default_num_ws(resolution)              # comodgan.py:367-370 (14 at 256, 16 at 512)
        _populate(self, "synthesis", cfg)

    def forward(self, x, feats, ws, noise_mode="random", return_intermediate_outs=False):
        """comodgan.py:395-421: img [B, 3, R, R], or (img, {"res_to_rgb": {res: ...}, "res_img": {res: ...}}).  Beyond the reference:
        ws may hold B = N * S rows for N encoded images, image-major as in forward_samples -- row i * S + s is completed from image i."""
        return self._generator()._stage_synthesis(x, feats, ws, noise_mode, return_intermediate_outs)


class Generator(nn.Module):
    """Co-Mod-GAN generator (reference comodgan.py:423-455) on MI355X."""

    def __init__(self, mapping: Mapping, encoder: Encoder, synthesis: Synthesis):
        super().__init__()
        if synthesis.num_ws != mapping.num_ws:
            raise ValueError                                     # stylegan.py:606-607
        if (encoder.resolution, encoder.ch_base, encoder.ch_max, encoder.oc_n) != (
                synthesis.resolution, synthesis.ch_base, synthesis.ch_max, synthesis.w0_dim) or mapping.w_dim != synthesis.w_dim:
            raise ValueError("encoder and synthesis geometries differ")
        self.mapping, self.synthesis, self.encoder = mapping, synthesis, encoder
        for stage in (mapping, encoder, synthesis):
            stage.__dict__["_owner"] = (self,)                   # (_Node._generator)
        self.num_ws, self.z_dim, self.c_dim, self.w_dim = mapping.num_ws, mapping.z_dim, mapping.c_dim, mapping.w_dim
        self.img_resolution, self.img_channels, self.ic_n = synthesis.resolution, synthesis.rgb_n, encoder.ic_n
        self._cfg = cs.Config(resolution=synthesis.resolution, ch_base=synthesis.ch_base, ch_max=synthesis.ch_max, z_dim=mapping.z_dim,
                              w_dim=mapping.w_dim, w0_dim=synthesis.w0_dim, map_layers=mapping.num_layers, num_ws=mapping.num_ws)
        self._names: List[str] = [e.name for e in cs.entries(self._cfg)]
        self._lib: Optional[MiganLib] = None
        self._handle: Optional[CoModGANHandle] = None
        self._handle_device: Optional[int] = None
        self._bound: Optional[Tuple[int, ...]] = None
        self._dirty = True
        self._ws: Optional[torch.Tensor] = None
        self._frozen = False         # freeze_weights(): the caller's promise that parameters no longer change in place
        self._refreeze = True        # the handle has not been told yet
        self._cutoff: Optional[int] = None   # truncation_cutoff the handle was last told
        self._fp16: Tuple[Optional[int], Optional[int]] = (None, None)   # half-precision blocks the handle was last told
        self._fp16_storage = False       # set_fp16_storage(): the marked blocks keep their activations in fp16
        self._fp16_storage_told = False  # what the handle was last told
        self._stage_need: Dict[tuple, int] = {}   # workspace bytes of the stage calls, per (handle, batch, samples, plan settings)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())

    # ------------------------------------------------------------------ plumbing
    def freeze_weights(self, frozen: bool = True) -> "Generator":
        """Opt-in for repeated inference: promise that no parameter is modified in place from now on, so the per-forward
        weight preparation (0.45 ms of a 19 ms batch-16 forward) runs once.  load_state_dict / .to() / re-assignment of a
        parameter are picked up automatically; after an in-place write (``p.data.mul_()``, an optimizer step, a raw-pointer
        write) call ``freeze_weights()`` again, or ``freeze_weights(False)`` to go back to re-preparing every forward."""
        self._frozen = bool(frozen)
        self._refreeze = True
        return self

    def set_fp16_storage(self, on: bool = True) -> "Generator":
        """Opt-in beside ``use_fp16_before_res`` / ``use_fp16_after_res``: the blocks they mark store their activations in fp16, as
        the reference's half-precision path does (half the workspace and the activation traffic of those blocks; arithmetic stays
        fp32 on converted values).  No effect while no block is marked.  Honoured by forward, forward_samples and forward_timed."""
        self._fp16_storage = bool(on)
        return self

    def _invalidate(self) -> None:
        self._dirty = True

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate()
        return out

    def _tensors(self) -> List[torch.Tensor]:
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        return [sd[n] for n in self._names]

    def _stream(self, x: torch.Tensor) -> int:
        return int(torch.cuda.current_stream(x.device).cuda_stream)

    def _engine(self, x: torch.Tensor) -> CoModGANHandle:
        if not x.is_cuda:
            raise RuntimeError("mi-gan_amd comodgan.Generator.forward needs a tensor on an MI355X (HIP) device; there is no CPU path. "
                               "Move the model and input with .to('cuda').")
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        if self._lib is None:
            self._lib = load_library()                           # raises MiganError when not built
        if self._handle is None or self._handle_device != dev:
            if self._handle is not None:
                self._handle.close()
            c = self._cfg
            self._handle = CoModGANHandle(self._lib, c.resolution, c.num_ws, c.ch_base, c.ch_max, c.z_dim, c.w_dim, c.w0_dim, c.map_layers, dev)
            self._handle_device = dev
            self._bound = None
            self._refreeze = True
            self._cutoff = None
            self._fp16 = (None, None)
            self._fp16_storage_told = False
        # half-precision blocks (the reference's constructor arguments, kept as attributes of the two sub-modules): their 3x3
        # convolutions run with single fp16 operands.  Part of the plan, so the handle is told before the workspace is sized.
        fp16 = (_fp16_res("use_fp16_before_res", self.encoder.use_fp16_before_res),
                _fp16_res("use_fp16_after_res", self.synthesis.use_fp16_after_res))
        if fp16 != self._fp16:
            self._handle.set_fp16_blocks(*fp16)
            self._fp16 = fp16
        if self._fp16_storage != self._fp16_storage_told:        # (part of the plan as well)
            self._handle.set_fp16_storage(self._fp16_storage)
            self._fp16_storage_told = self._fp16_storage
        tensors = self._tensors()
        ptrs = tuple(t.data_ptr() for t in tensors)
        if self._dirty or ptrs != self._bound:
            for name, t in zip(self._names, tensors):
                if t.device != x.device:
                    raise RuntimeError(f"Expected all tensors to be on the same device, but {name} is on {t.device} and the input on {x.device}")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError(f"{name}: parameters must be contiguous float32 (got {t.dtype})")
                self._handle.set_weight(name, t.data_ptr(), tuple(t.shape))
            self._handle.commit(self._stream(x))
            self._bound = ptrs
            self._dirty = False
        return self._handle

    def _workspace(self, h: CoModGANHandle, batch: int, device: torch.device, samples: int = 1) -> torch.Tensor:
        need = h.workspace_bytes(batch) if samples == 1 else h.workspace_bytes_samples(batch, samples)
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = None
            self._refreeze = True            # a new allocation holds no prepared weight planes (even at a recycled address)
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    # ------------------------------------------------------------------ API
    def forward(self, x: torch.Tensor, z: Optional[torch.Tensor] = None, c=None, truncation_psi: float = 1, truncation_cutoff=None,
                noise_mode: str = "random", return_intermediate_outs: bool = False, _timed: bool = False):
        """Args: x: 4 channel rgb+mask [N,4,R,R] (comodgan.py:437-441); z: [N,z_dim] (drawn with torch.randn when None, :438-439)."""
        assert noise_mode in ["random", "const", "none"]         # stylegan.py:280
        if c is not None or return_intermediate_outs:
            raise NotImplementedError("c (class conditioning: c_dim = 0 in every published config) is not part of the MI355X inference path, and "
                                      "the fused Generator.forward keeps no per-resolution image: for return_intermediate_outs call the stages, "
                                      "G.synthesis(*G.encoder(x), G.mapping(z), return_intermediate_outs=True)")
        if truncation_cutoff is not None and (int(truncation_cutoff) != truncation_cutoff or truncation_cutoff < 0):
            raise ValueError(f"truncation_cutoff must be a non-negative integer or None, got {truncation_cutoff!r}")
        r = self.img_resolution
        if x.dim() != 4 or x.shape[1] != 4 or x.shape[2] != r or x.shape[3] != r:
            raise RuntimeError(f"expected input of shape [N, 4, {r}, {r}] (mask-0.5, img*mask), got {list(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"Input type ({x.dtype}) and weight type (torch.float32) should be the same")
        n = x.shape[0]
        if n == 0:
            raise RuntimeError("empty batch")
        h = self._engine(x)
        x = x.contiguous()
        if z is None:
            z = torch.randn([n, self.z_dim]).to(x.device)        # comodgan.py:439
        if z.shape != (n, self.z_dim):
            raise RuntimeError(f"expected z of shape [{n}, {self.z_dim}], got {list(z.shape)}")
        z = z.to(device=x.device, dtype=torch.float32).contiguous()
        noise = None
        if noise_mode == "random":
            noise = torch.randn(n * h.noise_floats(), dtype=torch.float32, device=x.device)    # stylegan.py:284-285, all layers at once
        cutoff = None if truncation_cutoff is None else int(truncation_cutoff)
        if cutoff != self._cutoff:                               # (part of the workspace layout: set before sizing it)
            h.set_truncation_cutoff(cutoff)
            self._cutoff = cutoff
        ws = self._workspace(h, n, x.device)
        # freeze_weights(): the fp16 operand planes / demodulation statistics of the 3x3 weights at the head of the workspace
        # are prepared once and reused (the library re-prepares them by itself after a re-binding, on another workspace or
        # another stream).  Without it they are rebuilt every forward, so in-place parameter updates are always seen.
        if self._refreeze:
            h.assume_static_weights(self._frozen)          # (re-)asserting drops the planes prepared so far
            self._refreeze = False
        y = torch.empty((n, 3, r, r), dtype=torch.float32, device=x.device)
        ms = h.forward(x.data_ptr(), z.data_ptr(), y.data_ptr(), n, ws.data_ptr(), ws.numel(), float(truncation_psi), noise_mode,
                       None if noise is None else noise.data_ptr(), self._stream(x), timed=_timed)
        return (y, ms) if _timed else y

    def forward_samples(self, x: torch.Tensor, z: Optional[torch.Tensor] = None, samples: Optional[int] = None, truncation_psi: float = 1,
                        truncation_cutoff=None, noise_mode: str = "random", _timed: bool = False):
        """Several completions per image from one encoder pass (no reference equivalent).  x: [N,4,R,R]; z: [N,S,z_dim], or None with
        ``samples=S`` (drawn with torch.randn) -> [N,S,3,R,R].  ``forward_samples(x, z)[i, s]`` is what
        ``forward(x.repeat_interleave(S, 0), z.reshape(N * S, -1))[i * S + s]`` gives with the same options, but the encoder, which never
        sees z, runs once per image; the mapping network, the styles and the synthesis network run once per sample."""
        assert noise_mode in ["random", "const", "none"]         # stylegan.py:280
        if truncation_cutoff is not None and (int(truncation_cutoff) != truncation_cutoff or truncation_cutoff < 0):
            raise ValueError(f"truncation_cutoff must be a non-negative integer or None, got {truncation_cutoff!r}")
        r = self.img_resolution
        if x.dim() != 4 or x.shape[1] != 4 or x.shape[2] != r or x.shape[3] != r:
            raise RuntimeError(f"expected input of shape [N, 4, {r}, {r}] (mask-0.5, img*mask), got {list(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"Input type ({x.dtype}) and weight type (torch.float32) should be the same")
        n = x.shape[0]
        if n == 0:
            raise RuntimeError("empty batch")
        if samples is not None and (int(samples) != samples or samples < 1):
            raise ValueError(f"samples must be a positive integer or None, got {samples!r}")
        if z is None:
            if samples is None:
                raise ValueError("forward_samples needs z of shape [N, S, z_dim], or samples=S to draw it")
        else:
            if z.dim() != 3 or z.shape[0] != n or z.shape[1] < 1 or z.shape[2] != self.z_dim:
                raise RuntimeError(f"expected z of shape [{n}, S, {self.z_dim}] (S latents per image), got {list(z.shape)}")
            if samples is not None and int(samples) != z.shape[1]:
                raise ValueError(f"samples={samples} contradicts z of shape {list(z.shape)}")
        s = int(samples) if z is None else int(z.shape[1])
        h = self._engine(x)
        x = x.contiguous()
        if z is None:
            z = torch.randn([n, s, self.z_dim]).to(x.device)
        z = z.to(device=x.device, dtype=torch.float32).contiguous()
        noise = None
        if noise_mode == "random":
            noise = torch.randn(n * s * h.noise_floats(), dtype=torch.float32, device=x.device)    # one draw per sample and layer
        cutoff = None if truncation_cutoff is None else int(truncation_cutoff)
        if cutoff != self._cutoff:                               # (part of the workspace layout: set before sizing it)
            h.set_truncation_cutoff(cutoff)
            self._cutoff = cutoff
        ws = self._workspace(h, n, x.device, s)
        if self._refreeze:                                       # as in forward(): the prepared weight planes do not depend on S
            h.assume_static_weights(self._frozen)
            self._refreeze = False
        y = torch.empty((n, s, 3, r, r), dtype=torch.float32, device=x.device)
        ms = h.forward_samples(x.data_ptr(), z.data_ptr(), y.data_ptr(), n, s, ws.data_ptr(), ws.numel(), float(truncation_psi), noise_mode,
                               None if noise is None else noise.data_ptr(), self._stream(x), timed=_timed)
        return (y, ms) if _timed else y

    # ------------------------------------------------------------------ uint8 in / uint8 out (include/comodgan_u8_hip.h)
    def _check_uint8(self, img_u8: torch.Tensor, mask_u8: torch.Tensor, what: str) -> None:
        r = self.img_resolution
        if not (img_u8.is_cuda and mask_u8.is_cuda):
            raise RuntimeError(f"mi-gan_amd comodgan.Generator.{what} needs tensors on an MI355X (HIP) device; there is no CPU path")
        if img_u8.dtype != torch.uint8 or mask_u8.dtype != torch.uint8:
            raise RuntimeError("image and mask must be uint8 (np.array of the PIL images, reference demo.py:59-60)")
        if img_u8.dim() != 4 or tuple(img_u8.shape[1:]) != (r, r, 3) or tuple(mask_u8.shape) != tuple(img_u8.shape[:3]):
            raise RuntimeError(f"expected image [N,{r},{r},3] and mask [N,{r},{r}], got {list(img_u8.shape)} and {list(mask_u8.shape)}")
        if img_u8.shape[0] == 0:
            raise RuntimeError("empty batch")

    def _forward_uint8(self, img_u8: torch.Tensor, mask_u8: torch.Tensor, z: torch.Tensor, truncation_psi, truncation_cutoff, noise_mode: str,
                       _timed: bool = False):
        """img [N,R,R,3], mask [N,R,R], z [N,S,z_dim] (checked by the callers) -> [N,S,R,R,3]; handle state as in forward_samples"""
        n, s, r = z.shape[0], z.shape[1], self.img_resolution
        h = self._engine(img_u8)
        img_u8, mask_u8 = img_u8.contiguous(), mask_u8.contiguous()
        z = z.to(device=img_u8.device, dtype=torch.float32).contiguous()
        noise = None
        if noise_mode == "random":
            noise = torch.randn(n * s * h.noise_floats(), dtype=torch.float32, device=img_u8.device)    # one draw per sample and layer
        cutoff = None if truncation_cutoff is None else int(truncation_cutoff)
        if cutoff != self._cutoff:                               # (part of the workspace layout: set before sizing it)
            h.set_truncation_cutoff(cutoff)
            self._cutoff = cutoff
        ws = self._workspace(h, n, img_u8.device, s)             # (the layout does not depend on the I/O mode)
        if self._refreeze:
            h.assume_static_weights(self._frozen)
            self._refreeze = False
        out = torch.empty((n, s, r, r, 3), dtype=torch.uint8, device=img_u8.device)
        ms = h.forward_u8(img_u8.data_ptr(), mask_u8.data_ptr(), z.data_ptr(), out.data_ptr(), n, s, ws.data_ptr(), ws.numel(),
                          float(truncation_psi), noise_mode, None if noise is None else noise.data_ptr(), self._stream(img_u8), timed=_timed)
        return (out, ms) if _timed else out

    def forward_uint8(self, img_u8: torch.Tensor, mask_u8: torch.Tensor, z: Optional[torch.Tensor] = None, truncation_psi: float = 1,
                      truncation_cutoff=None, noise_mode: str = "random", _timed: bool = False):
        """scripts/demo.py:56-66 + forward + :135-140 in one call, at network resolution: uint8 image [N,R,R,3] (HWC) and uint8 mask
        [N,R,R] (255 = known pixel, anything else = hole), z [N,z_dim] (drawn with torch.randn when None) -> composited uint8 image
        [N,R,R,3].  preprocess() runs inside the FromRGB kernel and the post-processing + composition inside the last ToRGB kernel: no
        fp32 network input or output tensor exists.  Bit-identical to pipeline.preprocess -> forward -> pipeline.compose with the same
        options (and, noise_mode "random", the same noise).  The inputs are not modified."""
        assert noise_mode in ["random", "const", "none"]         # stylegan.py:280
        if truncation_cutoff is not None and (int(truncation_cutoff) != truncation_cutoff or truncation_cutoff < 0):
            raise ValueError(f"truncation_cutoff must be a non-negative integer or None, got {truncation_cutoff!r}")
        self._check_uint8(img_u8, mask_u8, "forward_uint8")
        n = img_u8.shape[0]
        if z is None:
            z = torch.randn([n, self.z_dim]).to(img_u8.device)   # comodgan.py:439
        if z.shape != (n, self.z_dim):
            raise RuntimeError(f"expected z of shape [{n}, {self.z_dim}], got {list(z.shape)}")
        res = self._forward_uint8(img_u8, mask_u8, z.reshape(n, 1, self.z_dim), truncation_psi, truncation_cutoff, noise_mode, _timed)
        return (res[0][:, 0], res[1]) if _timed else res[:, 0]

    def forward_samples_uint8(self, img_u8: torch.Tensor, mask_u8: torch.Tensor, z: Optional[torch.Tensor] = None, samples: Optional[int] = None,
                              truncation_psi: float = 1, truncation_cutoff=None, noise_mode: str = "random", _timed: bool = False):
        """forward_samples on bytes: uint8 image [N,R,R,3] and mask [N,R,R]; z [N,S,z_dim], or None with ``samples=S`` -> uint8
        [N,S,R,R,3].  ``out[i, s]`` is ``compose(forward_samples(preprocess(img, mask), z)[i, s], img[i], mask[i])`` byte for byte with the
        same options: completion s of photo i pasted over photo i's known pixels, the encoder once per photo, nothing repeated by the
        caller and no fp32 image held."""
        assert noise_mode in ["random", "const", "none"]         # stylegan.py:280
        if truncation_cutoff is not None and (int(truncation_cutoff) != truncation_cutoff or truncation_cutoff < 0):
            raise ValueError(f"truncation_cutoff must be a non-negative integer or None, got {truncation_cutoff!r}")
        self._check_uint8(img_u8, mask_u8, "forward_samples_uint8")
        n = img_u8.shape[0]
        if samples is not None and (int(samples) != samples or samples < 1):
            raise ValueError(f"samples must be a positive integer or None, got {samples!r}")
        if z is None:
            if samples is None:
                raise ValueError("forward_samples_uint8 needs z of shape [N, S, z_dim], or samples=S to draw it")
            z = torch.randn([n, int(samples), self.z_dim]).to(img_u8.device)
        else:
            if z.dim() != 3 or z.shape[0] != n or z.shape[1] < 1 or z.shape[2] != self.z_dim:
                raise RuntimeError(f"expected z of shape [{n}, S, {self.z_dim}] (S latents per image), got {list(z.shape)}")
            if samples is not None and int(samples) != z.shape[1]:
                raise ValueError(f"samples={samples} contradicts z of shape {list(z.shape)}")
        return self._forward_uint8(img_u8, mask_u8, z, truncation_psi, truncation_cutoff, noise_mode, _timed)

    # ------------------------------------------------------------------ the stages (include/comodgan_stages_hip.h)
    def _stage_workspace(self, h: CoModGANHandle, batch: int, samples: int, device: torch.device) -> torch.Tensor:
        """One workspace for the stage calls and the fused forward: the prepared weight planes at its head serve all of them."""
        key = (id(h), batch, samples, self._fp16, self._fp16_storage_told, self._cutoff)
        need = self._stage_need.get(key)
        if need is None:
            if len(self._stage_need) > 64:
                self._stage_need.clear()
            need = self._stage_need[key] = h.stages_workspace_bytes(batch, samples)
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = None
            self._refreeze = True
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        if self._refreeze:
            h.assume_static_weights(self._frozen)
            self._refreeze = False
        return self._ws

    def _feat_dtype(self, res: int) -> torch.dtype:
        before = self._fp16[0]
        return torch.float16 if (self._fp16_storage_told and res > 4 and before is not None and res > before) else torch.float32

    def _resolutions(self) -> List[int]:
        return [1 << k for k in range(2, self.img_resolution.bit_length())]          # 4 ... R

    def _stage_mapping(self, z: torch.Tensor, c, truncation_psi, truncation_cutoff) -> torch.Tensor:
        if c is not None:
            raise NotImplementedError("c (class conditioning: c_dim = 0 in every published config) is not part of the MI355X inference path")
        if truncation_cutoff is not None and (int(truncation_cutoff) != truncation_cutoff or truncation_cutoff < 0):
            raise ValueError(f"truncation_cutoff must be a non-negative integer or None, got {truncation_cutoff!r}")
        if z.dim() != 2 or z.shape[1] != self.z_dim or z.shape[0] == 0:
            raise RuntimeError(f"expected z of shape [N, {self.z_dim}], got {list(z.shape)}")
        h = self._engine(z)
        z = z.to(torch.float32).contiguous()
        n = z.shape[0]
        wsp = self._stage_workspace(h, n, 1, z.device)
        ws = torch.empty((n, self.num_ws, self.w_dim), dtype=torch.float32, device=z.device)
        h.mapping(z.data_ptr(), ws.data_ptr(), n, wsp.data_ptr(), wsp.numel(), float(truncation_psi),
                  None if truncation_cutoff is None else int(truncation_cutoff), self._stream(z))
        return ws

    def _stage_encoder(self, img: torch.Tensor, c=None):
        if c is not None:
            raise NotImplementedError("c (class conditioning: c_dim = 0 in every published config) is not part of the MI355X inference path")
        r = self.img_resolution
        if img.dim() != 4 or img.shape[1] != 4 or img.shape[2] != r or img.shape[3] != r or img.shape[0] == 0:
            raise RuntimeError(f"expected input of shape [N, 4, {r}, {r}] (mask-0.5, img*mask), got {list(img.shape)}")
        if img.dtype != torch.float32:
            raise RuntimeError(f"Input type ({img.dtype}) and weight type (torch.float32) should be the same")
        h = self._engine(img)
        img = img.contiguous()
        n = img.shape[0]
        wsp = self._stage_workspace(h, n, 1, img.device)
        x = torch.empty((n, self._cfg.w0_dim), dtype=torch.float32, device=img.device)
        # NHWC memory under the reference's NCHW shape: the encoder kernels write the tensors the caller gets
        feats = {res: torch.empty((n, min(self._cfg.ch_base // res, self._cfg.ch_max), res, res), dtype=self._feat_dtype(res), device=img.device,
                                  memory_format=torch.channels_last) for res in reversed(self._resolutions())}
        h.encode(img.data_ptr(), x.data_ptr(), [feats[res].data_ptr() for res in self._resolutions()], n, wsp.data_ptr(), wsp.numel(),
                 self._stream(img))
        return x, feats

    def _stage_synthesis(self, x: torch.Tensor, feats, ws: torch.Tensor, noise_mode: str = "random", return_intermediate_outs: bool = False):
        assert noise_mode in ["random", "const", "none"]         # stylegan.py:280
        r, c = self.img_resolution, self._cfg
        if x.dim() != 2 or x.shape[1] != c.w0_dim or x.shape[0] == 0:
            raise RuntimeError(f"expected x (the encoder's global code) of shape [N, {c.w0_dim}], got {list(x.shape)}")
        n = x.shape[0]
        if ws.dim() != 3 or ws.shape[1] != self.num_ws or ws.shape[2] != self.w_dim or ws.shape[0] == 0:
            raise RuntimeError(f"expected ws of shape [N * S, {self.num_ws}, {self.w_dim}], got {list(ws.shape)}")
        b = ws.shape[0]
        if b % n:
            raise ValueError(f"ws has {b} rows for {n} encoded images (x: {list(x.shape)}): the rows must be a multiple of the images, "
                             f"row i * S + s completing image i")
        s = b // n
        h = self._engine(x)
        x = x.to(torch.float32).contiguous()
        ws = ws.to(device=x.device, dtype=torch.float32).contiguous()           # comodgan.py:397
        ptrs = []
        keep = []
        for res in self._resolutions():
            if res not in feats:
                raise ValueError(f"feats has no entry for resolution {res}: expected the keys {self._resolutions()}, got {sorted(feats)}")
            f = feats[res]
            want = (n, min(c.ch_base // res, c.ch_max), res, res)
            if tuple(f.shape) != want:
                raise RuntimeError(f"feats[{res}]: expected shape {list(want)}, got {list(f.shape)}")
            dt = self._feat_dtype(res)
            if f.dtype != dt or f.device != x.device or not f.is_contiguous(memory_format=torch.channels_last):
                f = f.to(device=x.device, dtype=dt).contiguous(memory_format=torch.channels_last)      # plumbing, off the hot path
            keep.append(f)
            ptrs.append(f.data_ptr())
        noise = None
        if noise_mode == "random":
            noise = torch.randn(b * h.noise_floats(), dtype=torch.float32, device=x.device)
        wsp = self._stage_workspace(h, n, s, x.device)
        y = torch.empty((b, 3, r, r), dtype=torch.float32, device=x.device)
        to_rgb = res_img = None
        outs = None
        if return_intermediate_outs:
            lower = [res for res in self._resolutions() if res < r]
            imgs = {res: torch.empty((b, 3, res, res), dtype=torch.float32, device=x.device) for res in lower}
            rgbs = {res: torch.empty((b, 3, res, res), dtype=torch.float32, device=x.device) for res in self._resolutions() if res > 4}
            res_img = [imgs[res].data_ptr() if res < r else 0 for res in self._resolutions()]
            to_rgb = [rgbs[res].data_ptr() if res > 4 else 0 for res in self._resolutions()]
            imgs[r] = y
            outs = {"res_to_rgb": {4: imgs[4], **rgbs}, "res_img": imgs}      # comodgan.py:410: one tensor under both keys at res 4
        h.synthesize(x.data_ptr(), ptrs, ws.data_ptr(), y.data_ptr(), n, s, wsp.data_ptr(), wsp.numel(), noise_mode,
                     None if noise is None else noise.data_ptr(), to_rgb, res_img, self._stream(x))
        return (y, outs) if return_intermediate_outs else y

    def forward_timed(self, x: torch.Tensor, z: torch.Tensor, noise_mode: str = "const"):
        """forward() with a hipEvent pair around every kernel launch: (y, [ms per launch])."""
        return self.forward(x, z, noise_mode=noise_mode, _timed=True)

    def launch_info(self):
        if self._handle is None:
            raise RuntimeError("launch_info() needs one forward first")
        return self._handle.launches()

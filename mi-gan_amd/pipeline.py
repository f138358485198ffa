"""GPU mirrors of the steps either side of ``Generator.forward`` in the reference's scripts/demo.py
(preprocess :56-66 and the result / composition lines :135-140), at network resolution, through the
C ABI (``migan_pack_input`` / ``migan_compose_output``).  Like the generator there is no CPU path."""
from __future__ import annotations

import math
import numbers

import torch

from .hipbind import load_library


def _check(img_u8: torch.Tensor, mask_u8: torch.Tensor):
    if not (img_u8.is_cuda and mask_u8.is_cuda):
        raise RuntimeError("mi-gan_amd.pipeline needs tensors on an MI355X (HIP) device; there is no CPU path")
    if img_u8.dtype != torch.uint8 or mask_u8.dtype != torch.uint8:
        raise RuntimeError("image and mask must be uint8 (np.array of the PIL images, reference demo.py:59-60)")
    if img_u8.dim() != 4 or img_u8.shape[-1] != 3 or img_u8.shape[1] != img_u8.shape[2]:
        raise RuntimeError(f"expected image batch [N,R,R,3], got {list(img_u8.shape)}")
    if tuple(mask_u8.shape) != tuple(img_u8.shape[:3]):
        raise RuntimeError(f"expected mask batch {list(img_u8.shape[:3])}, got {list(mask_u8.shape)}")
    return img_u8.contiguous(), mask_u8.contiguous()


def preprocess(img_u8: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """uint8 image [N,R,R,3] + mask [N,R,R] (255 = known) -> x [N,4,R,R] = cat([mask-0.5, img*mask])."""
    img_u8, mask_u8 = _check(img_u8, mask_u8)
    n, r = img_u8.shape[0], img_u8.shape[1]
    x = torch.empty((n, 4, r, r), dtype=torch.float32, device=img_u8.device)
    load_library().pack_input(img_u8.data_ptr(), mask_u8.data_ptr(), x.data_ptr(), n, r,
                              int(torch.cuda.current_stream(img_u8.device).cuda_stream))
    return x


def compose(y: torch.Tensor, img_u8: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """network output y [N,3,R,R] -> uint8 [N,R,R,3]: known pixels from the image, holes from the network."""
    img_u8, mask_u8 = _check(img_u8, mask_u8)
    n, r = img_u8.shape[0], img_u8.shape[1]
    if not y.is_cuda or y.dtype != torch.float32 or tuple(y.shape) != (n, 3, r, r):
        raise RuntimeError(f"expected y [N,3,R,R] float32 on the GPU, got {list(y.shape)} {y.dtype}")
    out = torch.empty((n, r, r, 3), dtype=torch.uint8, device=img_u8.device)
    load_library().compose_output(y.contiguous().data_ptr(), img_u8.data_ptr(), mask_u8.data_ptr(), out.data_ptr(), n, r,
                                  int(torch.cuda.current_stream(img_u8.device).cuda_stream))
    return out


class MIGAN_Pipeline(torch.nn.Module):
    """The reference's deployed pipeline, scripts/create_onnx_pipeline.py::MIGAN_Pipeline (:118-264, exported there as
    migan_pipeline_v2.onnx), on the GPU through the C ABI: masked bounding box -> crop -> resize to the network resolution ->
    generator -> resize back -> feathered blend into the image (``migan_pipeline_bbox / _pre / _post`` either side of
    ``migan_forward``).  Same constructor and ``forward(image, mask)`` contract as the reference module:

      image (1, 3, H, W) uint8, mask (1, 1, H, W) uint8 (255 = known pixel); the image is modified in place and returned.

    ``model_path`` is a reference ``migan_*.pt`` state dict, or an already built module: a ``mi-gan_amd`` Generator, or a
    ``comodgan.Generator`` of the pipeline's resolution (x [N, 4, R, R] -> y [N, 3, R, R]; ``forward_samples`` then gives several
    completions per image).  A mask of another size is resized to the image's size first (nearest), like the reference's first line
    (:256).  No CPU path.

    ``forward_batch(images, masks)`` is the same for N images of different sizes around ONE generator forward per ``max_batch``
    images, with the boxes kept on the device (``migan_pipeline_batch_pre / _post``): no host synchronisation in between.

    ``forward_samples(images, masks, z)`` leaves the images as they are and returns S completions of each, [S, 3, H_i, W_i], from one
    pass over the image per chunk (``migan_pipeline_batch_post_samples``).

    ``forward_patches(images, masks, z)`` returns the same completions as box-sized patches, [S, 3, ch_i, cw_i], and the boxes
    (``migan_pipeline_batch_post_patches``): the pixels outside a box are the photo's in every completion.

    ``forward_regions(images, masks)`` is ``forward_batch`` with one crop per hole region instead of one per image: a photo with
    several marked objects far apart gets each of them completed at its own scale (``migan_pipeline_regions_find / _pre / _post``).

    ``forward_native(images, masks)`` is ``forward_regions`` without the two resamplings: every crop is rounded up to the generator's
    granularity and completed at the photo's own scale by the fully convolutional forward (``migan_pipeline_native_pre / _post``
    around ``Generator.forward_any_size``).  Its effect on image quality has not been measured.

    ``forward_region_patches(images, masks, z)`` joins the two: S completions per hole region, returned as box-sized patches, with the
    photos left as they are; ``paste_patches`` writes the chosen completion of every region into its photo
    (``migan_pipeline_regions_post_patches / _paste``)."""

    def __init__(self, model_path, resolution: int, padding: int = 128, device="cuda"):
        super().__init__()
        from .migan_inference import Generator
        if isinstance(model_path, torch.nn.Module):
            self.model = model_path
        else:
            self.model = Generator(resolution=resolution)
            self.model.load_state_dict(torch.load(model_path, map_location="cpu"))
        self.model = self.model.to(device).eval()
        self.res = int(resolution)
        self.padding = int(padding)
        # GaussianSmoothing(channels=1, kernel_size=5, sigma=1.0, dim=2).weight (:63-85), in torch fp32 like the reference buffer
        ax = torch.arange(5, dtype=torch.float32)
        g = 1 / (1.0 * math.sqrt(2 * math.pi)) * torch.exp(-((ax - 2.0) / (2 * 1.0)) ** 2)
        k = g[:, None] * g[None, :]
        self.gaussian_weight = (k / k.sum()).contiguous()          # host side: handed to migan_pipeline_post by value
        self._gauss = self.gaussian_weight.flatten().tolist()
        self._scratch = None

    def _scratch_for(self, lib, h: int, w: int, device) -> torch.Tensor:
        """scratch of the bbox / post kernels, one buffer per (device, stream): two streams running the pipeline never share it"""
        return self._scratch_bytes(lib.pipeline_scratch_bytes(h, w), device)

    def _scratch_bytes(self, need: int, device) -> torch.Tensor:
        key = (device.index if device.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(device).cuda_stream))
        if self._scratch is None:
            self._scratch = {}
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < need:
            if len(self._scratch) >= 8:                    # (stream handles come and go: keep the cache bounded)
                self._scratch.clear()
            buf = torch.empty(need, dtype=torch.uint8, device=device)
            self._scratch[key] = buf
        return buf

    @staticmethod
    def _check_mask(mask: torch.Tensor) -> torch.Tensor:
        if not mask.is_cuda:
            raise RuntimeError("mi-gan_amd.pipeline needs tensors on an MI355X (HIP) device; there is no CPU path")
        if mask.dtype != torch.uint8:
            raise RuntimeError("mask must be uint8 (reference create_onnx_pipeline.py:254-255)")
        if mask.dim() != 4 or mask.shape[0] != 1 or mask.shape[1] != 1:
            raise RuntimeError(f"expected mask (1, 1, h, w), got {list(mask.shape)}")
        return mask.contiguous()

    def get_masked_bbox(self, mask: torch.Tensor):
        """(:132-231) -> x_min, x_max, y_min, y_max"""
        mask = self._check_mask(mask)
        lib = load_library()
        h, w = int(mask.shape[-2]), int(mask.shape[-1])
        with torch.cuda.device(mask.device):                      # the handle-free entry points launch on the CURRENT device
            scratch = self._scratch_for(lib, h, w, mask.device)
            return lib.pipeline_bbox(mask.data_ptr(), h, w, self.res, self.padding, scratch.data_ptr(),
                                     int(torch.cuda.current_stream(mask.device).cuda_stream))

    @torch.no_grad()
    def forward(self, image: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        if not (image.is_cuda and mask.is_cuda):
            raise RuntimeError("mi-gan_amd.pipeline needs tensors on an MI355X (HIP) device; there is no CPU path")
        if image.dtype != torch.uint8 or mask.dtype != torch.uint8:
            raise RuntimeError("image and mask must be uint8 (reference create_onnx_pipeline.py:254-255)")
        if image.dim() != 4 or image.shape[0] != 1 or image.shape[1] != 3 or not image.is_contiguous():
            raise RuntimeError(f"expected a contiguous image (1, 3, H, W), got {list(image.shape)}")
        h, w = int(image.shape[2]), int(image.shape[3])
        mask = self._check_mask(mask)
        if mask.device != image.device:
            raise RuntimeError("image and mask must be on the same device")
        with torch.cuda.device(image.device):                     # the handle-free entry points launch on the CURRENT device
            return self._forward_on_device(image, mask, h, w)

    def _forward_on_device(self, image: torch.Tensor, mask: torch.Tensor, h: int, w: int) -> torch.Tensor:
        lib = load_library()
        stream = int(torch.cuda.current_stream(image.device).cuda_stream)
        if tuple(mask.shape[2:]) != (h, w):                      # mask = tvF.resize(mask, image size, NEAREST) (:256)
            resized = torch.empty((1, 1, h, w), dtype=torch.uint8, device=image.device)
            lib.pipeline_mask_resize(mask.data_ptr(), int(mask.shape[2]), int(mask.shape[3]), resized.data_ptr(), h, w, stream)
            mask = resized
        scratch = self._scratch_for(lib, h, w, image.device)
        bbox = lib.pipeline_bbox(mask.data_ptr(), h, w, self.res, self.padding, scratch.data_ptr(), stream)
        x = torch.empty((1, 4, self.res, self.res), dtype=torch.float32, device=image.device)
        lib.pipeline_pre(image.data_ptr(), mask.data_ptr(), h, w, bbox, self.res, x.data_ptr(), stream)
        y = self.model(x).contiguous()
        lib.pipeline_post(image.data_ptr(), mask.data_ptr(), h, w, bbox, self.res, y.data_ptr(), scratch.data_ptr(),
                          gauss25=self._gauss, stream=stream)
        return image

    @staticmethod
    def _batch_items(images, masks):
        """the per-image input checks of forward_batch / forward_samples -> [(image ptr, mask ptr, H, W, h, w, the contiguous mask), ...], device"""
        items, device = [], None
        for image, mask in zip(images, masks):
            if not (image.is_cuda and mask.is_cuda):
                raise RuntimeError("mi-gan_amd.pipeline needs tensors on an MI355X (HIP) device; there is no CPU path")
            if image.dtype != torch.uint8 or mask.dtype != torch.uint8:
                raise RuntimeError("image and mask must be uint8 (reference create_onnx_pipeline.py:254-255)")
            if not ((image.dim() == 4 and image.shape[0] == 1 and image.shape[1] == 3) or (image.dim() == 3 and image.shape[0] == 3)) \
                    or not image.is_contiguous():
                raise RuntimeError(f"expected a contiguous image (1, 3, H, W), got {list(image.shape)}")
            if not ((mask.dim() == 4 and mask.shape[0] == 1 and mask.shape[1] == 1) or mask.dim() == 2):
                raise RuntimeError(f"expected mask (1, 1, h, w), got {list(mask.shape)}")
            device = image.device if device is None else device
            if mask.device != device or image.device != device:
                raise RuntimeError("image and mask must be on the same device")
            mask = mask.contiguous()
            items.append((image.data_ptr(), mask.data_ptr(), int(image.shape[-2]), int(image.shape[-1]), int(mask.shape[-2]),
                          int(mask.shape[-1]), mask))                # (the contiguous mask stays alive until the kernels are queued)
        return items, device

    @torch.no_grad()
    def forward_batch(self, images, masks, *, max_batch: int = 32, return_bbox: bool = False):
        """``forward`` for N images of different sizes: images[i] (1, 3, H_i, W_i) or (3, H_i, W_i) uint8, contiguous, masks[i]
        (1, 1, h_i, w_i) or (h_i, w_i) uint8, all on one device.  Per chunk of at most ``max_batch`` images: masks resized where
        needed -> boxes (on the device) -> x [n, 4, R, R] -> ONE ``self.model(x)`` -> blend, with no host synchronisation in
        between.  The images are modified in place and returned as a list; with ``return_bbox`` also the int32 [N, 4] device tensor
        of {x_min, x_max, y_min, y_max} rows.  Each image gets what ``forward`` gives it, up to the fp32 rounding by which the
        generator at batch n differs from batch 1.  Two entries that share memory are undefined."""
        images, masks = list(images), list(masks)
        if len(images) != len(masks) or not images:
            raise RuntimeError(f"expected as many masks as images and at least one, got {len(images)} images and {len(masks)} masks")
        if int(max_batch) < 1:
            raise RuntimeError(f"max_batch must be at least 1, got {max_batch}")
        items, device = self._batch_items(images, masks)
        lib = load_library()
        bbox = torch.empty((len(items), 4), dtype=torch.int32, device=device)
        with torch.cuda.device(device):                          # the handle-free entry points launch on the CURRENT device
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            for i0 in range(0, len(items), int(max_batch)):
                chunk = [it[:6] for it in items[i0:i0 + int(max_batch)]]
                scratch = self._scratch_bytes(lib.pipeline_batch_scratch_bytes(chunk), device)
                box = bbox[i0:i0 + len(chunk)]
                # A last chunk of ONE image of a longer list runs the generator at batch 2 (its x twice): an image of a batch of two
                # or more is bit-identical whatever the batch, a batch-1 forward only to fp32 rounding --
                # so the result of forward_batch does not depend on max_batch (max_batch=1 asks for batch 1 and gets it)
                pad = 1 if len(chunk) == 1 and len(items) > 1 and int(max_batch) > 1 else 0
                x = torch.empty((len(chunk) + pad, 4, self.res, self.res), dtype=torch.float32, device=device)
                lib.pipeline_batch_pre(chunk, self.res, self.padding, x.data_ptr(), box.data_ptr(), scratch.data_ptr(), stream)
                if pad:
                    x[1].copy_(x[0])
                y = self.model(x).contiguous()
                lib.pipeline_batch_post(chunk, self.res, y.data_ptr(), box.data_ptr(), scratch.data_ptr(), gauss25=self._gauss,
                                        stream=stream)
        return (images, bbox) if return_bbox else images

    def _samples_plan(self, images, masks, z, samples, max_rows, model_kwargs):
        """the argument checks forward_samples and forward_patches share -> items, device, the model's forward_samples or None, S,
        images per chunk, z (drawn here when the caller gave `samples` alone)"""
        if len(images) != len(masks) or not images:
            raise RuntimeError(f"expected as many masks as images and at least one, got {len(images)} images and {len(masks)} masks")
        if int(max_rows) < 1:
            raise RuntimeError(f"max_rows must be at least 1, got {max_rows}")
        items, device = self._batch_items(images, masks)
        n_img, max_rows = len(items), int(max_rows)
        sampler = getattr(self.model, "forward_samples", None)
        if samples is not None and (int(samples) != samples or samples < 1):
            raise ValueError(f"samples must be a positive integer or None, got {samples!r}")
        if sampler is None:
            if z is not None or (samples is not None and int(samples) != 1) or model_kwargs:
                raise ValueError(f"{type(self.model).__name__} has no forward_samples: it gives one completion per image, so z must be None, "
                                 f"samples None or 1, and there are no model options")
            s, per_chunk = 1, max_rows
        else:
            if z is None:
                if samples is None:
                    raise ValueError("forward_samples needs z of shape [N, S, z_dim], or samples=S to draw it")
                s = int(samples)
                z = torch.randn([n_img, s, self.model.z_dim]).to(device)
            else:
                if not z.is_cuda or z.device != device:
                    raise RuntimeError("mi-gan_amd.pipeline needs tensors on an MI355X (HIP) device; there is no CPU path (z must be on the images' device)")
                if not z.is_floating_point():
                    raise RuntimeError(f"z must be a floating-point tensor, got {z.dtype}")
                if z.dim() != 3 or z.shape[0] != n_img or z.shape[1] < 1:
                    raise ValueError(f"expected z of shape [{n_img}, S, z_dim] (S latents for each of the {n_img} images), got {list(z.shape)}")
                if samples is not None and int(samples) != z.shape[1]:
                    raise ValueError(f"samples={samples} contradicts z of shape {list(z.shape)}")
                s = int(z.shape[1])
            if s > max_rows:
                raise ValueError(f"{s} samples per image do not fit max_rows={max_rows} generator rows per chunk: raise max_rows")
            per_chunk = max_rows // s
        return items, device, sampler, s, per_chunk, z

    def _samples_pre(self, lib, items, i0, per_chunk, sampler, box, device, stream):
        """pipeline_batch_pre of the chunk that starts at image i0 -> its item tuples, scratch and x; `box` = its rows of the box table"""
        chunk = [it[:6] for it in items[i0:i0 + per_chunk]]
        scratch = self._scratch_bytes(lib.pipeline_batch_scratch_bytes(chunk), device)
        # (without a sampler: forward_batch's rule for a lone last chunk, so that the bytes are forward_batch's)
        pad = 1 if sampler is None and len(chunk) == 1 and len(items) > 1 and per_chunk > 1 else 0
        x = torch.empty((len(chunk) + pad, 4, self.res, self.res), dtype=torch.float32, device=device)
        lib.pipeline_batch_pre(chunk, self.res, self.padding, x.data_ptr(), box.data_ptr(), scratch.data_ptr(), stream)
        if pad:
            x[1].copy_(x[0])
        return chunk, scratch, x

    def _samples_generate(self, x, n, sampler, z, s, model_kwargs):
        """the generator on one chunk of n images -> y, contiguous, rows i * S + s"""
        if sampler is None:
            return self.model(x).contiguous()
        return sampler(x, z, **model_kwargs).reshape(n * s, 3, self.res, self.res).contiguous()

    @torch.no_grad()
    def forward_samples(self, images, masks, z=None, samples=None, *, max_rows: int = 32, return_bbox: bool = False, **model_kwargs):
        """S completions per image, written OUT OF PLACE: images and masks as for ``forward_batch`` and not modified -> a list of
        uint8 tensors [S, 3, H_i, W_i] (views of one allocation), with ``return_bbox`` also the int32 [N, 4] device tensor of boxes.

        A model with a ``forward_samples`` method (``comodgan.Generator``): ``z`` [N, S, z_dim], or ``samples=S`` draws it;
        ``model_kwargs`` (truncation_psi, truncation_cutoff, noise_mode) go to the model unchanged.  Per chunk of ``max_rows // S``
        images: boxes and x once per image -> ``model.forward_samples(x, z)``: the encoder once per image, [n * S, 3, R, R] ->
        ``migan_pipeline_batch_post_samples``: each image read once, its feathered mask built once, S images written.  No host
        synchronisation in between.

        Any other model (the MI-GAN generator) gives one completion: ``z`` must be None and S is 1; ``self.model(x)`` runs on
        ``forward_batch``'s chunks (``max_rows`` images, a lone last chunk at batch 2), so ``forward_samples(images, masks)[i][0]``
        holds the bytes ``forward_batch`` writes into a copy of images[i].

        Inside its box, sample s of image i is what ``forward_batch`` gives a copy of the image for that generator output; outside
        it is the image.  An image whose mask yields no usable box is returned as S plain copies."""
        images, masks = list(images), list(masks)
        items, device, sampler, s, per_chunk, z = self._samples_plan(images, masks, z, samples, max_rows, model_kwargs)
        n_img = len(items)
        lib = load_library()
        bbox = torch.empty((n_img, 4), dtype=torch.int32, device=device)
        sizes = [3 * it[2] * it[3] for it in items]
        flat = torch.empty(s * sum(sizes), dtype=torch.uint8, device=device)       # all S x N outputs; the list holds views
        outs, at = [], 0
        for it, size in zip(items, sizes):
            outs.append(flat[at:at + s * size].view(s, 3, it[2], it[3]))
            at += s * size
        with torch.cuda.device(device):                          # the handle-free entry points launch on the CURRENT device
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            for i0 in range(0, n_img, per_chunk):
                box = bbox[i0:i0 + per_chunk]
                chunk, scratch, x = self._samples_pre(lib, items, i0, per_chunk, sampler, box, device, stream)
                y = self._samples_generate(x, len(chunk), sampler, None if z is None else z[i0:i0 + len(chunk)], s, model_kwargs)
                lib.pipeline_batch_post_samples(chunk, s, self.res, y.data_ptr(), box.data_ptr(), scratch.data_ptr(),
                                                [o.data_ptr() for o in outs[i0:i0 + len(chunk)]], gauss25=self._gauss, stream=stream)
        return (outs, bbox) if return_bbox else outs

    @torch.no_grad()
    def forward_patches(self, images, masks, z=None, samples=None, *, max_rows: int = 32, **model_kwargs):
        """``forward_samples`` for a caller that wants only what differs between the completions: -> (patches, boxes), where
        patches[i] is uint8 [S, 3, ch_i, cw_i] on the device, the crop [y_min, y_max) x [x_min, x_max) of image i in every
        completion, and boxes the int32 CPU tensor [N, 4] of {x_min, x_max, y_min, y_max} rows.  Nothing outside the boxes is read
        or written, and the result takes S * 3 * ch * cw bytes per image instead of S * 3 * H * W.

        Arguments, checks, chunks (``max_rows // S`` images; for a model without ``forward_samples`` ``max_rows`` images and a lone
        last chunk at batch 2) and errors are ``forward_samples``'.  With the same model, z, ``model_kwargs`` (``noise_mode="const"``:
        random noise differs from call to call) and ``max_rows``, byte for byte:

            patches[i] == forward_samples(...)[i][:, :, y_min:y_max, x_min:x_max]

        Per chunk: boxes and x once per image -> the chunk's boxes are copied to the host, which sizes the result: ONE HOST
        SYNCHRONISATION PER CHUNK, the only one of this mode (``forward_samples`` has none) -> the generator ->
        ``migan_pipeline_batch_post_patches``.  patches[i] is a view of its chunk's one allocation; an image whose mask yields no
        usable box gets an empty patch, [S, 3, 0, 0].  Images and masks are not modified."""
        images, masks = list(images), list(masks)
        items, device, sampler, s, per_chunk, z = self._samples_plan(images, masks, z, samples, max_rows, model_kwargs)
        n_img = len(items)
        lib = load_library()
        bbox = torch.empty((n_img, 4), dtype=torch.int32, device=device)
        patches, boxes = [], []
        with torch.cuda.device(device):                          # the handle-free entry points launch on the CURRENT device
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            for i0 in range(0, n_img, per_chunk):
                box = bbox[i0:i0 + per_chunk]
                chunk, scratch, x = self._samples_pre(lib, items, i0, per_chunk, sampler, box, device, stream)
                rows = box.cpu()                                 # (waits for the boxes: the synchronisation of this mode)
                shapes = []
                for (x0, x1, y0, y1), it in zip(rows.tolist(), chunk):
                    # migan_pipeline.hpp: pipe_box_valid -- the kernel skips any other box, and an empty patch has nothing to skip
                    fits = x0 >= 0 and x1 <= it[3] and y0 >= 0 and y1 <= it[2] and x1 - x0 >= 3 and y1 - y0 >= 3
                    shapes.append((y1 - y0, x1 - x0) if fits else (0, 0))
                sizes = [s * 3 * h * w for h, w in shapes]
                flat = torch.empty(sum(sizes), dtype=torch.uint8, device=device)   # exactly the chunk's patches; the list holds views
                outs, at = [], 0
                for (h, w), size in zip(shapes, sizes):
                    outs.append(flat[at:at + size].view(s, 3, h, w))
                    at += size
                y = self._samples_generate(x, len(chunk), sampler, None if z is None else z[i0:i0 + len(chunk)], s, model_kwargs)
                lib.pipeline_batch_post_patches(chunk, s, self.res, y.data_ptr(), box.data_ptr(), scratch.data_ptr(),
                                                [o.data_ptr() if size else 0 for o, size in zip(outs, sizes)], sizes,
                                                gauss25=self._gauss, stream=stream)
                patches += outs
                boxes.append(rows)
        return patches, torch.cat(boxes)

    @torch.no_grad()
    def forward_regions(self, images, masks, *, gap=None, max_regions: int = 8, max_batch: int = 32, return_regions: bool = False):
        """``forward_batch`` with ONE CROP PER HOLE REGION.  ``forward_batch`` puts one box around every hole pixel of an image, so two
        small holes in opposite corners of a large photo share one crop squeezed to the network resolution; here the mask is split
        into regions on the device and every region gets a box of its own by the same box rule.  Arguments, checks and error types
        are ``forward_batch``'s; the images are modified in place and returned as a list.

        Regions: with hole pixel = ``mask != 255`` (the mask nearest-resized to the image first), D = every pixel within Chebyshev
        distance ``gap`` of a hole pixel, a region is an 8-connected component of D, numbered 1 ... K in raster order of its first
        pixel.  Region k's box is ``get_masked_bbox`` of its hole pixels, its network input is the crop with the FULL mask, and its
        result is ``forward_batch``'s post-processing of that crop stored only where the label is k.  ``gap`` defaults to
        ``max(2, padding // 4)`` and must be in 2 ... 64: the feathered mask at a pixel depends on the mask within 3 pixels of it and
        every other region's hole pixel is at least ``gap + 2`` away, so with ``gap >= 2`` a region's bytes are those a mask holding
        that region alone would give, and no pixel has two writers.

        When not to split: an image with K <= 1, with K > ``max_regions`` (1 ... 64), or whose single box has both sides <= the
        network resolution (its crop is not downscaled: splitting gains nothing) runs as one row with ``forward_batch``'s box, and
        its bytes are ``forward_batch``'s.  An image without a hole pixel has no row and is left untouched.

        Per call: ``migan_pipeline_regions_find`` for all images -> ONE copy of the counts and boxes to the host, which sizes the
        generator batch: ONE HOST SYNCHRONISATION PER CALL (``forward_batch`` has none) -> the rows of all images in one list -> the
        network input of ALL rows (an image's rows may straddle chunks, and every input must be formed before any result is stored
        into its image: ``rows * 4 * R * R * 4`` bytes are held at once) -> per chunk of at most ``max_batch`` rows ONE
        ``self.model(x)`` and ``migan_pipeline_regions_post``.  A lone last chunk runs at batch 2, as in ``forward_batch``, so the
        result does not depend on ``max_batch``.

        With ``return_regions`` also returns, per image, the int32 CPU tensor [rows_i, 4] of the boxes used ({x_min, x_max, y_min,
        y_max}; one row when not split, none without a hole) and the uint8 label map [H_i, W_i] on the device (unspecified for an
        image with more than ``max_regions`` regions)."""
        images, masks = list(images), list(masks)
        if len(images) != len(masks) or not images:
            raise RuntimeError(f"expected as many masks as images and at least one, got {len(images)} images and {len(masks)} masks")
        if int(max_batch) < 1:
            raise RuntimeError(f"max_batch must be at least 1, got {max_batch}")
        gap, max_regions, max_batch = *self._regions_args(gap, max_regions), int(max_batch)
        items, device = self._batch_items(images, masks)
        lib = load_library()
        res = self.res
        with torch.cuda.device(device):                          # the handle-free entry points launch on the CURRENT device
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            rows, _, used, labels, full = self._regions_rows(lib, items, device, stream, gap, max_regions)      # (`full` keeps the rows' masks alive)
            if rows:
                # forward_batch's rule for a lone last chunk: it runs at batch 2 (its x twice), so no row sees a batch-1 forward
                lone = len(rows) % max_batch == 1 and len(rows) > 1 and max_batch > 1
                x = torch.empty((len(rows) + (1 if lone else 0), 4, res, res), dtype=torch.float32, device=device)
                lib.pipeline_regions_pre(rows, res, x.data_ptr(), stream)
                if lone:
                    x[-1].copy_(x[-2])
                for r0 in range(0, len(rows), max_batch):
                    chunk = rows[r0:r0 + max_batch]
                    y = self.model(x[r0:r0 + len(chunk) + (1 if lone and len(chunk) == 1 else 0)]).contiguous()
                    lib.pipeline_regions_post(chunk, res, y.data_ptr(), gauss25=self._gauss, stream=stream)
        return (images, used, labels) if return_regions else images

    def native_window(self, box, H: int, W: int):
        """The window rule of ``forward_native``, a pure function of integers: ``box`` = (x_min, x_max, y_min, y_max), the
        reference's box inside an H x W photo -> ``((x0, x1, y0, y1), (Hc, Wc))``: the network window Hc x Wc, both sides the box's
        rounded up to a multiple of q = resolution / 4 (the granularity of ``Generator.forward_any_size``), and the part of it that
        lies inside the photo.

        Per axis (columns; rows alike): Wc = ceil(cw / q) q.  Wc <= W: the window lies inside the photo, the extra columns taken
        evenly from either side of the box and shifted back inside at a border, x0 = clamp(x_min - (Wc - cw) // 2, 0, W - Wc),
        x1 = x0 + Wc -- real photo context.  Wc > W (the photo is narrower than the window): x0 = 0, x1 = W, and columns W ... Wc - 1
        of the network input are unknown pixels.  The in-photo box always sits at the window's top-left corner; a box whose sides
        are multiples of q comes back unchanged."""
        q = self.res // 4
        x_min, x_max, y_min, y_max = (int(v) for v in box)

        def axis(lo, hi, n):
            side = hi - lo
            full = -(-side // q) * q
            if full > n:
                return 0, n, full
            at = min(max(lo - (full - side) // 2, 0), n - full)
            return at, at + full, full

        x0, x1, wc = axis(x_min, x_max, int(W))
        y0, y1, hc = axis(y_min, y_max, int(H))
        return (x0, x1, y0, y1), (hc, wc)

    @torch.no_grad()
    def forward_native(self, images, masks, *, max_side=None, gap=None, max_regions: int = 8, max_batch: int = 32,
                       return_rows: bool = False):
        """``forward_regions`` WITHOUT RESAMPLING: every row's crop goes through the generator at the photo's own scale
        (``Generator.forward_any_size``, the fully convolutional forward) instead of being squeezed to R x R and blown up again.
        Arguments, checks and error types are ``forward_regions``'; the images are modified in place and returned as a list.  The
        model must have ``forward_any_size`` (the MI-GAN ``Generator``): any other model (Co-Mod-GAN, whose encoder ends in a dense
        layer; ``NoiseSampler``) raises ``RuntimeError`` before anything is launched.

        WHAT IS AND IS NOT KNOWN ABOUT THIS MODE: it is an exact composition of pieces that are each tested -- the window rule, the
        network input and the blend of ``migan_pipeline_native_pre / _post``, ``forward_any_size`` -- and the tests hold it to that,
        byte for byte.  No trained checkpoint was at hand when it was written: what it does to IMAGE QUALITY (a generator trained
        at R x R, run on a larger window with its noise planes tiled) HAS NOT BEEN MEASURED.

        Rows and boxes are ``forward_regions``' (``_regions_rows``: the same one host synchronisation per call, the same "when not
        to split" rule; ``max_regions=1`` gives one box per photo).  Every box goes through ``native_window``: its sides rounded up
        to multiples of R / 4, grown into the photo around it; where the photo is smaller than the window the missing part of the
        network input is unknown pixels, mask 0 -- x = (-0.5, 0, 0, 0) -- not replicated or reflected photo.

        A row is a FALLBACK row, run resized at R exactly as ``forward_regions`` runs it, when its window has a side above
        ``max_side`` (default 4 R; must be in R ... 4096) or when Hc Wc max(4, 32768 // R) exceeds 2^30 - 1024, the extent limit of
        ``migan_forward_hw`` (32768 // R = the generator's channels at full resolution).

        Order of work: the network input of ALL rows first (``migan_pipeline_native_pre`` per window size,
        ``migan_pipeline_regions_pre`` for the fallback rows), as in ``forward_regions``.  Then, per window size in ascending
        (Hc, Wc) order, the rows in row order in calls of at most ``max(1, max_batch R^2 // (Hc Wc))`` rows -- no more activation
        memory than a ``forward_batch`` chunk -- each ONE ``model.forward_any_size(x)`` and one ``migan_pipeline_native_post``.
        The rows with an R x R window and the fallback rows run, at (R, R)'s place in that order, as ``forward_regions`` runs its
        rows: ``self.model(x)`` on chunks of ``max_batch``, a lone last chunk at batch 2.

        Consequences.  A call in which every row is a fallback or has an R x R window that lies inside its photo leaves
        ``forward_regions``' bytes (``torch.equal``).  In every other group a row's result may differ by fp32 rounding with the
        batch it shares a forward with, as ``forward`` differs from ``forward_batch``; a lone row of such a group runs at batch 1.

        With ``return_rows`` also returns the list of generator calls in the order they ran, each ``(Hc, Wc, [(image index, label,
        box), ...])`` with the rows in the order of x: box = the in-photo box of ``native_window``; a fallback row is listed in an
        (R, R) call with the reference's box."""
        images, masks = list(images), list(masks)
        any_size = getattr(self.model, "forward_any_size", None)
        if any_size is None:
            raise RuntimeError(f"forward_native needs a model with forward_any_size (the MI-GAN Generator's fully convolutional "
                               f"forward); {type(self.model).__name__} has none")
        if len(images) != len(masks) or not images:
            raise RuntimeError(f"expected as many masks as images and at least one, got {len(images)} images and {len(masks)} masks")
        if int(max_batch) < 1:
            raise RuntimeError(f"max_batch must be at least 1, got {max_batch}")
        res = self.res
        max_side = 4 * res if max_side is None else int(max_side)
        if not res <= max_side <= max(4096, 4 * res):
            raise ValueError(f"max_side must be in {res} ... 4096, got {max_side}")
        gap, max_regions, max_batch = *self._regions_args(gap, max_regions), int(max_batch)
        items, device = self._batch_items(images, masks)
        lib = load_library()
        calls = []
        with torch.cuda.device(device):                          # the handle-free entry points launch on the CURRENT device
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            rows, owner, _, labels, full = self._regions_rows(lib, items, device, stream, gap, max_regions)  # (`full`, `labels`: kept alive)
            # window size -> [(row as the kernels take it, its entry in a call's list, native or fallback), ...] in row order;
            # (R, R) also holds the fallback rows
            groups = {}
            for row, i in zip(rows, owner):
                win, (hc, wc) = self.native_window(row[6], row[3], row[4])
                if max(hc, wc) > max_side or hc * wc * max(4, 32768 // res) > 2 ** 30 - 1024:
                    groups.setdefault((res, res), []).append((row, (i, row[5], tuple(row[6])), False))
                else:
                    groups.setdefault((hc, wc), []).append((row[:6] + (win,), (i, row[5], win), True))

            def runs(group):
                """maximal runs of one kind: (first index, rows as the kernels take them, native or fallback)"""
                at = 0
                while at < len(group):
                    end = at
                    while end < len(group) and group[end][2] == group[at][2]:
                        end += 1
                    yield at, [g[0] for g in group[at:end]], group[at][2]
                    at = end

            xs = {}
            for (hc, wc), group in groups.items():
                square = (hc, wc) == (res, res)
                # forward_regions' rule for a lone last chunk: it runs at batch 2 (its x twice), so no row sees a batch-1 forward
                lone = square and len(group) % max_batch == 1 and len(group) > 1 and max_batch > 1
                x = torch.empty((len(group) + (1 if lone else 0), 4, hc, wc), dtype=torch.float32, device=device)
                for at, part, native in runs(group):
                    if native:
                        lib.pipeline_native_pre(part, hc, wc, x[at].data_ptr(), stream)
                    else:
                        lib.pipeline_regions_pre(part, res, x[at].data_ptr(), stream)
                if lone:
                    x[-1].copy_(x[-2])
                xs[(hc, wc)] = (x, lone)
            for (hc, wc) in sorted(groups):
                group, (x, lone) = groups[(hc, wc)], xs.pop((hc, wc))
                square = (hc, wc) == (res, res)
                per_call = max_batch if square else max(1, max_batch * res * res // (hc * wc))
                for r0 in range(0, len(group), per_call):
                    chunk = group[r0:r0 + per_call]
                    if square:
                        y = self.model(x[r0:r0 + len(chunk) + (1 if lone and len(chunk) == 1 else 0)]).contiguous()
                    else:
                        y = any_size(x[r0:r0 + len(chunk)]).contiguous()
                    for at, part, native in runs(chunk):
                        if native:
                            lib.pipeline_native_post(part, hc, wc, y[at].data_ptr(), gauss25=self._gauss, stream=stream)
                        else:
                            lib.pipeline_regions_post(part, res, y[at].data_ptr(), gauss25=self._gauss, stream=stream)
                    calls.append((hc, wc, [g[1] for g in chunk]))
            del full, labels                                     # (the masks and label maps lived until their readers were queued)
        return (images, calls) if return_rows else images

    def _regions_args(self, gap, max_regions):
        """the checks of ``gap`` and ``max_regions`` forward_regions and forward_region_patches share -> gap, max_regions"""
        gap = max(2, self.padding // 4) if gap is None else int(gap)
        max_regions = int(max_regions)
        if not 2 <= gap <= 64:
            raise ValueError(f"gap must be in 2 ... 64, got {gap}")
        if not 1 <= max_regions <= 64:
            raise ValueError(f"max_regions must be in 1 ... 64, got {max_regions}")
        return gap, max_regions

    def _regions_rows(self, lib, items, device, stream, gap, max_regions):
        """What forward_regions and forward_region_patches share, on the current device: ``migan_pipeline_regions_find`` for all images ->
        ONE copy of the counts and boxes to the host (the host synchronisation) -> the "when not to split" rule.  Returns the rows of
        all images in one list, (image ptr, mask ptr, labels ptr, H, W, label, box), the image every row belongs to, per image the
        int32 CPU tensor [rows_i, 4] of its boxes, the label maps, and the masks at the images' sizes (the rows hold their addresses:
        they must stay alive until the kernels that read them are queued)."""
        n, cap, res = len(items), max_regions + 1, self.res
        table = [it[:6] for it in items]
        scratch = self._scratch_bytes(lib.pipeline_regions_scratch_bytes(table, gap, max_regions), device)
        labels = [torch.empty((it[2], it[3]), dtype=torch.uint8, device=device) for it in items]
        found = torch.empty(n + n * cap * 4, dtype=torch.int32, device=device)       # the counts, then the boxes: one copy
        count, boxes = found[:n], found[n:]
        lib.pipeline_regions_find(table, res, self.padding, gap, max_regions, [t.data_ptr() for t in labels], count.data_ptr(),
                                  boxes.data_ptr(), scratch.data_ptr(), stream)
        host = found.cpu()                                   # (waits for the labelling: the synchronisation of this mode)
        counts, host_boxes = host[:n].tolist(), host[n:].view(n, cap, 4)
        full, rows, owner, used = [], [], [], []
        for i, it in enumerate(items):
            mask = it[6]
            if (it[4], it[5]) != (it[2], it[3]):             # the rows take the mask at the image's size (:256)
                mask = torch.empty((it[2], it[3]), dtype=torch.uint8, device=device)
                lib.pipeline_mask_resize(it[1], it[4], it[5], mask.data_ptr(), it[2], it[3], stream)
            full.append(mask)
            k, box = counts[i], host_boxes[i]
            single = box[0].tolist()
            if k == 0:
                mine = []
            elif k < 2 or k > max_regions or (single[1] - single[0] <= res and single[3] - single[2] <= res):
                mine = [(0, single)]
            else:
                mine = [(r, box[r].tolist()) for r in range(1, k + 1)]
            rows += [(it[0], mask.data_ptr(), labels[i].data_ptr(), it[2], it[3], label, b) for label, b in mine]
            owner += [i] * len(mine)
            used.append(torch.tensor([b for _, b in mine], dtype=torch.int32).view(len(mine), 4))
        return rows, owner, used, labels, full

    @torch.no_grad()
    def forward_region_patches(self, images, masks, z=None, samples=None, *, gap=None, max_regions: int = 8, max_rows: int = 32,
                               **model_kwargs):
        """S completions PER HOLE REGION, as box-sized patches: ``forward_regions``' crops (one per region) with ``forward_patches``'
        sample axis, written out of place -> ``(patches, boxes, labels)``.  An object-removal front end offers the S candidates of
        every object and lets the user pick one per object; ``paste_patches`` then writes the picks into the photo.

          patches[i]  a list with one uint8 [S, 3, ch, cw] device tensor per row of image i (views of one allocation per chunk);
                      empty for an image without a hole pixel
          boxes[i]    the int32 CPU tensor [rows_i, 4] of {x_min, x_max, y_min, y_max} rows ``forward_regions(return_regions=True)``
                      gives
          labels[i]   the uint8 [H_i, W_i] label map on the device (unspecified for an image with more than ``max_regions`` regions)

        The label of row j of image i is ``j + 1`` when the image has two or more rows (it was split: row j is region j + 1 of the
        label map) and 0 when it has one (a single-box row: no label test).  Inside its box, sample s of a row holds, where the label
        map equals the row's label, the bytes ``forward_regions`` would store there for that generator output, and the photo's bytes
        everywhere else -- also where the box covers a part of ANOTHER region: every patch is an opaque crop of the photo with one
        region completed.  Images and masks are only read.

        ``z``, ``samples``, ``max_rows`` and ``model_kwargs`` are ``forward_patches``' (checks and error types included), ``gap`` and
        ``max_regions`` ``forward_regions``'; region finding, the "when not to split" rule and the row list are ``forward_regions``'.
        Row j of image i uses the latents z[i] ([N, S, z_dim]): sample s of every region of a photo shares the photo's latent s.

        Per call: ``migan_pipeline_regions_find`` -> ONE HOST SYNCHRONISATION (counts and boxes) -> the rows.  A model with
        ``forward_samples`` then runs chunks of ``max_rows // S`` rows: ``migan_pipeline_regions_pre`` of the chunk ->
        ``model.forward_samples(x_rows, z_rows, **model_kwargs)`` -> ``migan_pipeline_regions_post_patches``.  Any other model (the
        MI-GAN generator, S = 1) runs ``self.model(x)`` on ``forward_regions``' chunks: ``max_rows`` rows, a lone last chunk at batch
        2, so ``paste_patches(copies, patches, boxes, labels, 0)`` leaves ``forward_regions``' bytes.  The photos are not written, so
        the network input is formed per chunk (``forward_regions`` holds the input of all rows at once)."""
        images, masks = list(images), list(masks)
        items, device, sampler, s, per_chunk, z = self._samples_plan(images, masks, z, samples, max_rows, model_kwargs)
        gap, max_regions = self._regions_args(gap, max_regions)
        lib = load_library()
        res = self.res
        patches = [[] for _ in items]
        with torch.cuda.device(device):                          # the handle-free entry points launch on the CURRENT device
            stream = int(torch.cuda.current_stream(device).cuda_stream)
            rows, owner, used, labels, full = self._regions_rows(lib, items, device, stream, gap, max_regions)
            # (without a sampler: forward_regions' rule for a lone last chunk, so that the bytes are forward_regions')
            lone = sampler is None and len(rows) % per_chunk == 1 and len(rows) > 1 and per_chunk > 1
            for r0 in range(0, len(rows), per_chunk):
                chunk = rows[r0:r0 + per_chunk]
                pad = 1 if lone and len(chunk) == 1 else 0
                x = torch.empty((len(chunk) + pad, 4, res, res), dtype=torch.float32, device=device)
                lib.pipeline_regions_pre(chunk, res, x.data_ptr(), stream)
                if pad:
                    x[1].copy_(x[0])
                z_rows = None if z is None else z[torch.tensor(owner[r0:r0 + len(chunk)], device=device)]
                y = self._samples_generate(x, len(chunk), sampler, z_rows, s, model_kwargs)
                shapes = [(row[6][3] - row[6][2], row[6][1] - row[6][0]) for row in chunk]
                sizes = [s * 3 * h * w for h, w in shapes]
                flat = torch.empty(sum(sizes), dtype=torch.uint8, device=device)   # exactly the chunk's patches; the lists hold views
                at = 0
                outs = []
                for (h, w), size in zip(shapes, sizes):
                    outs.append(flat[at:at + size].view(s, 3, h, w))
                    at += size
                lib.pipeline_regions_post_patches(chunk, s, res, y.data_ptr(), [o.data_ptr() for o in outs], sizes, gauss25=self._gauss,
                                                  stream=stream)
                for i, o in zip(owner[r0:r0 + len(chunk)], outs):
                    patches[i].append(o)
            del full                                             # (the resized masks lived until their readers were queued)
        return patches, used, labels

    @torch.no_grad()
    def paste_patches(self, images, patches, boxes, labels, choice):
        """The inverse step of ``forward_region_patches``: writes the chosen sample of every region into its photo, IN PLACE, and returns
        ``images``.  ``patches``, ``boxes``, ``labels`` are what ``forward_region_patches`` returned for these photos (or copies of
        them).  ``choice`` is one int for all rows, or per image a sequence with one entry per row (or one int for the image);
        ``None`` or -1 leaves that region untouched.

        Only the pixels of the row's own label are written (``migan_pipeline_regions_paste``; the whole box for the single row of an
        image that was not split), so the overlapping boxes of neighbouring regions do not disturb each other and the rows may be
        pasted in any order, or in several calls.  ``ValueError``: a patch whose shape is not [S, 3, ch, cw] of its box, a choice
        outside -1 ... S - 1, lists of the wrong length."""
        images, patches, boxes, labels = list(images), list(patches), list(boxes), list(labels)
        n = len(images)
        if not images or not (len(patches) == len(boxes) == len(labels) == n):
            raise ValueError(f"expected patches, boxes and labels for each of the {n} images and at least one image, got "
                             f"{len(patches)}, {len(boxes)} and {len(labels)}")
        if choice is None or isinstance(choice, numbers.Integral):
            choice = [choice] * n
        choice = list(choice)
        if len(choice) != n:
            raise ValueError(f"expected one choice, or one entry of choices per image ({n}), got {len(choice)}")
        rows, device = [], None
        for i, (image, mine, box, lab) in enumerate(zip(images, patches, boxes, labels)):
            if not (image.is_cuda and lab.is_cuda):
                raise RuntimeError("mi-gan_amd.pipeline needs tensors on an MI355X (HIP) device; there is no CPU path")
            if image.dtype != torch.uint8 or lab.dtype != torch.uint8:
                raise RuntimeError("image and label map must be uint8")
            if not ((image.dim() == 4 and image.shape[0] == 1 and image.shape[1] == 3) or (image.dim() == 3 and image.shape[0] == 3)) \
                    or not image.is_contiguous():
                raise RuntimeError(f"expected a contiguous image (1, 3, H, W), got {list(image.shape)}")
            device = image.device if device is None else device
            if image.device != device or lab.device != device:
                raise RuntimeError("images, patches and label maps must be on the same device")
            h, w = int(image.shape[-2]), int(image.shape[-1])
            mine = list(mine)
            box = torch.as_tensor(box).reshape(-1, 4).tolist()
            if len(mine) != len(box):
                raise ValueError(f"image {i}: {len(mine)} patches for {len(box)} boxes")
            if tuple(lab.shape) != (h, w) or not lab.is_contiguous():
                raise ValueError(f"image {i}: expected a contiguous label map [{h}, {w}], got {list(lab.shape)}")
            picks = choice[i]
            if picks is None or isinstance(picks, numbers.Integral):
                picks = [picks] * len(mine)
            picks = list(picks)
            if len(picks) != len(mine):
                raise ValueError(f"image {i}: {len(picks)} choices for {len(mine)} rows")
            for j, (patch, (x0, x1, y0, y1), pick) in enumerate(zip(mine, box, picks)):
                if patch.dim() != 4 or tuple(patch.shape[1:]) != (3, y1 - y0, x1 - x0) or patch.shape[0] < 1:
                    raise ValueError(f"image {i} row {j}: expected patches [S, 3, {y1 - y0}, {x1 - x0}] for box {[x0, x1, y0, y1]}, got {list(patch.shape)}")
                if patch.dtype != torch.uint8 or not patch.is_contiguous():
                    raise ValueError(f"image {i} row {j}: patches must be contiguous uint8")
                if not patch.is_cuda or patch.device != device:
                    raise RuntimeError("images, patches and label maps must be on the same device")
                pick = -1 if pick is None else int(pick)
                if not -1 <= pick < patch.shape[0]:
                    raise ValueError(f"image {i} row {j}: choice {pick} is outside -1 ... {patch.shape[0] - 1}")
                if pick < 0:
                    continue
                rows.append((image.data_ptr(), lab.data_ptr(), patch.data_ptr() + pick * 3 * (y1 - y0) * (x1 - x0), h, w,
                             j + 1 if len(mine) >= 2 else 0, (x0, x1, y0, y1)))
        if rows:
            with torch.cuda.device(device):                      # the handle-free entry points launch on the CURRENT device
                load_library().pipeline_regions_paste(rows, int(torch.cuda.current_stream(device).cuda_stream))
        return images

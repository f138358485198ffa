"""Shared by tests/test_emu_migan_layers.py (product kernel source on the fiber emulator) and tests/test_gpu_migan_layers.py (MI355X):
every launch of an MI-GAN plan checked in isolation.

One debug-plan forward keeps every layer's output (migan_set_debug).  Each reference-level unit is then recomputed by
oracle/migan_oracle.py FROM THE TENSOR THE DEVICE FED IT (the device's own tap, not the oracle's chained one), so no upstream error
enters a comparison, a failing unit names the faulty launch, and a unit is an operator call on a known input: it is held to the
operator-level bounds of tests/sepconv_case.py, in 16-bit storage too, where the chained per-layer test has to allow frac = 0.7.
The workspace and y are filled with NaN bytes (0xFF) before the forward: an unwritten tile edge shows.

Units, 5 per resolution level (R the network's resolution, r the block's):
  encoder.bR.conv1      from the network input x, with the FromRGB head: separable_conv(lrelu_agc(pointwise(x, fw, fb)))
  encoder.b{r}.conv1    r < R: from the tap encoder.b{2r}.conv2
  encoder.b{r}.conv2    from the tap encoder.b{r}.conv1; r > 4: down=2.  The unit is the WHOLE SeparableConv2d, the dwfir launch and the
                        pointwise GEMM together: dwfir_tmp, which carries the tensor between the two, is one buffer shared by all down=2
                        layers and overwritten by each, so after the forward only the last one's could be read and the two launches cannot
                        be split.  A failure names both symbols
  synthesis.b{r}.conv1  from encoder.b4.conv2 (r = 4) or synthesis.b{r/2}.conv2 (up=2, noise); the skip tap encoder.b{r}.conv1 is added
                        before the storage rounding: the stored tensor includes the skip
  synthesis.b{r}.conv2  from the tap synthesis.b{r}.conv1; noise for r > 4
  synthesis.b{r}.img    (y at r = R) pointwise(stored conv2 tap, tw, tb) + upsample2d(tap of synthesis.b{r/2}.img)

Arithmetic.  fp32 storage: want = the float64 oracle.  16-bit storage: the mode's oracle as tests/sepconv_case.py has it (float32; gemm16
when the GEMM variant is "f16"; round_storage on the stored feature map; images stay fp32).

Bounds: the operator-level constants, not new ones.
  feature maps  storage_close(got, want, storage, ulps=1, frac=0.05 if gemm16 else 0.02, top_ulps=0.5 if gemm16 else 0.0)
                (fp32: 2e-5 * max(1, |want|max))
  images        3e-5 * max(1, |want|max), plus the 16-bit term of sepconv_case.py (3 storage steps of the feature map x |tw|max)
Those constants were set on layers of at most 256 input channels and the units here sum over 512, so next to each unit a RULER is
evaluated: the same unit in float32 numpy on the same input against the float64 value (16-bit storage: the mode's float32 oracle against
the mode's oracle in float64 arithmetic).  Rulers and device errors per unit class: profiles/migan_layers.md.  Relative to
max(1, |want|max), over all fp32 cases on the MI355X: feature maps, largest ruler 9.9e-7, largest device error 1.0e-6; images, 1.7e-6 and
2.7e-7.  MARGIN x ruler as argued in tests/comodgan_layers_case.py (x 4 for the two-plane f16x2 product, 22 significant bits against
float32's 24; x 2 for summation order) would be 7.9e-6 and 1.4e-5: below the operator constants 2e-5 and 3e-5, which a correct kernel
therefore meets on the 512-channel units too.  No class needs its constant replaced and RULER_BOUND stays empty; a class listed there
is bound by MARGIN x its largest ruler of the case instead.  No bound comes from the kernels' own error.
The frac caps are conditions on the reference as well: in 16-bit storage the mode's float32 oracle is held against the mode's float64
oracle with the same storage_close arguments, so a seed whose reference alone leaves them fails here, on any machine.

Guards: every unit is finite everywhere; in fp32 storage a unit's optional terms (skip, noise, previous image) each exceed 10 x its bound,
so a launch that drops one fails; the unit count is 5 * (log2 R - 1).  Test infrastructure only."""
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import migan_oracle as orc
from tests.emu_util import from_storage, nchw, storage_close, storage_ulp
from tests.knobs import knobs as borrowed

MARGIN = 8.0
RULER_BOUND = ()           # unit classes whose operator constant a correct kernel cannot meet at 512 channels (none: see the docstring)
NAN_BYTE = 0xFF            # 0xFFFFFFFF, 0xFFFF: a NaN in fp32, bf16 and fp16

# The eleven MIGAN_GEOMETRIES_SMALL instantiations (migan_table.hpp), written out: MODE, MT, NT, KC, FROMRGB, NI, MINW, MAING, PERSIST
SMALL_TILES = (
    "0, 32, 128, 32, false, 3, 2, false, false",      # 32-row plain, KC 32
    "3, 32, 128, 32, false, 1, 2, false, false",      # 32-row pointwise, KC 32
    "2, 64, 128, 32, false, 4, 2, false, false",      # 64-row FIR-up, KC 32
    "0, 32, 128, 64, false, 5, 2, false, false",      # 32-row plain, KC 64
    "3, 32, 128, 64, false, 2, 2, false, false",      # 32-row pointwise, KC 64
    "2, 64, 128, 64, false, 7, 2, false, false",      # 64-row FIR-up, KC 64
    "2, 32, 128, 32, false, 2, 2, false, false",      # 32-row FIR-up, KC 32
    "2, 32, 128, 64, false, 4, 2, false, false",      # 32-row FIR-up, KC 64
    "0, 32, 32, 64, false, 5, 2, false, false",       # 32 x 32 K-split plain
    "3, 32, 32, 64, false, 2, 2, false, false",       # 32 x 32 K-split pointwise
    "2, 32, 32, 64, false, 4, 2, false, false",       # 32 x 32 K-split FIR-up
)


def small_symbols(gemmv, stv, tiles=SMALL_TILES):
    """the symbols of `tiles` in the slice (GEMM variant, storage format): (2, 0) fp32, (3, 1) bf16, (3, 2) fp16"""
    return {f"migan::sepconv_kernel<{t}, {gemmv}, false, {stv}>" for t in tiles}


def is_small(symbol):
    return any(symbol.startswith(f"migan::sepconv_kernel<{t}, ") for t in SMALL_TILES)


def levels(res):
    return res.bit_length() - 2            # blocks b4 .. bR


def unit_names(res):
    out = []
    r = res
    while r >= 4:
        out += [f"encoder.b{r}.conv1", f"encoder.b{r}.conv2"]
        r //= 2
    r = 4
    while r <= res:
        out += [f"synthesis.b{r}.conv1", f"synthesis.b{r}.conv2", f"synthesis.b{r}.img"]
        r *= 2
    return out


def _put_bytes(mem, nbytes, value):
    """`nbytes` bytes of `value` in the memory of `mem`, 256-byte aligned (as float32 elements: what both memories take)"""
    buf = np.full(nbytes + 512, value, np.uint8)
    off = (256 - buf.ctypes.data % 256) % 256
    return mem.put(buf[off:off + (nbytes + 3) // 4 * 4].view(np.float32))


class Taps:
    """what one debug-plan forward left: every debug tensor and y, as float32 NCHW arrays in the values the device stored"""

    def __init__(self, lib, pkg, mem, *, res, batch, storage, gemm, tune, hw, seed):
        self.res, self.batch, self.storage = res, batch, storage
        self.hh, self.ww = hw if hw is not None else (res, res)
        hh, ww = self.hh, self.ww
        self.sd = pkg.synth.make_state_dict(res, seed=seed)
        if hw is None:
            self.x = pkg.synth.make_input(batch, res, seed=seed)
        else:
            self.x = (pkg.synth.normal((batch, 4, hh, ww), seed, "xhw") * 0.7).astype(np.float32)
        # the plan's g_small lists are built from the tuning at plan time: create, bind and run inside the borrowed knobs
        with borrowed(lib, **tune):
            h = pkg.hipbind.MiganHandle(lib, res, dtype=storage)
            try:
                if gemm is not None:
                    h.set_gemm(gemm)
                h.set_streams(1)
                h.set_debug(True)
                self.gemm = h.gemm()
                keep = {k: mem.put(np.ascontiguousarray(v.reshape(1) if v.ndim == 0 else v)) for k, v in self.sd.items()}
                for name, shape, _ in h.weights():
                    h.set_weight(name, mem.ptr(keep[name]), shape)
                h.commit(mem.stream)
                need = h.workspace_bytes_hw(batch, hh, ww)
                if hw is None:
                    assert need == h.workspace_bytes(batch)
                xd = mem.put(np.ascontiguousarray(self.x))
                yd = _put_bytes(mem, batch * 3 * hh * ww * 4, NAN_BYTE)
                wd = _put_bytes(mem, need, NAN_BYTE)
                if hw is None:
                    h.forward(mem.ptr(xd), mem.ptr(yd), batch, mem.ptr(wd), need, mem.stream)
                else:
                    h.forward_hw(mem.ptr(xd), mem.ptr(yd), batch, hh, ww, mem.ptr(wd), need, mem.stream)
                mem.sync()
                # after a forward at the handle's own size launch_info names what it launched; forward_hw at another size does not change it
                self.launches = [(i["layer"], i["kernel"]) for i in h.launches()] if hw is None else []
                raw = np.asarray(mem.get(wd)).view(np.uint8)[:need]
                esz = 4 if storage == "f32" else 2
                self.t = {}
                for name in unit_names(res):
                    if name == f"synthesis.b{res}.img":
                        continue
                    off, shape = h.debug_tensor_hw(batch, hh, ww, name)
                    if hw is None:
                        assert (off, shape) == h.debug_tensor(batch, name), name      # the same answer at H = W = R
                    n = int(np.prod(shape))
                    if name.endswith(".img"):
                        self.t[name] = raw[off:off + 4 * n].view(np.float32).reshape(shape).copy()
                    else:
                        stored = raw[off:off + esz * n].view(np.float32 if esz == 4 else np.uint16).reshape(shape)
                        self.t[name] = nchw(from_storage(stored, storage))
                self.t[f"synthesis.b{res}.img"] = np.asarray(mem.get(yd)).view(np.float32)[:batch * 3 * hh * ww].reshape(batch, 3, hh, ww).copy()
            finally:
                h.close()

    # what a unit reads: whole tensors here; WindowTaps serves the rows under one strip of the unit's output instead
    def read(self, name, role, cls):
        """role "in": the unit's input (name None: the network input x); "out": a tensor of the unit's own size (skip, the feature map under
        an image); "prev": the previous, half-size image"""
        return self.x if name is None else self.t[name]

    def noise(self, p):
        return p

    def kernels_of(self, name):
        """the symbols launch_info gave for the unit: its SeparableConv2d entry and the dwfir entry in front of it; an image unit: the
        un-fused ToRGB entry, or the conv2 launch whose tail writes the image"""
        if name.endswith(".img"):
            block = name[:-4]
            return [k for l, k in self.launches if l == block + ".torgb"] or [k for l, k in self.launches if l == block + ".conv2"]
        return [k for l, k in self.launches if l in (name + ".dwfir", name)]


def _sub(sd, prefix, dt):
    """the parameters of one SeparableConv2d under the oracle's prefix "m", in dtype dt (the FIR taps are the reference's: outer([1,3,3,1]) /
    64, x 4 for up, exact in float32)"""
    out = {"m" + k[len(prefix):]: np.asarray(v).astype(dt) for k, v in sd.items() if k.startswith(prefix + ".")}
    cin = out["m.conv1.weight"].shape[0]
    cout = out["m.conv2.weight"].shape[0]
    if "m.downsample.filter.weight" in out:
        out["m.downsample.filter.weight"] = np.broadcast_to(orc.fir_taps(1.0), (cin, 1, 4, 4)).astype(dt)
    if "m.upsample.filter.weight" in out:
        out["m.upsample.filter.weight"] = np.broadcast_to(orc.fir_taps(4.0), (cout, 1, 4, 4)).astype(dt)
    out.pop("m.upsample.filter_const", None)
    return out


def units(T):
    """-> [(name, class, fn(dt) -> (value before the storage rounding, {term: max |term|}))] in launch order; dt the oracle's arithmetic"""
    R, sd = T.res, T.sd
    gemm16 = T.storage != "f32" and T.gemm == "f16"
    out = []

    def sep(name, src, cls, head=False, skip=None):
        def fn(dt):
            x = T.read(None if head else src, "in", cls).astype(dt)
            if head:
                x = orc.lrelu_agc(orc.pointwise(x, sd[f"encoder.b{R}.fromrgb.weight"].astype(dt), sd[f"encoder.b{R}.fromrgb.bias"].astype(dt)))
            p = T.noise(_sub(sd, name, dt))
            y = orc.separable_conv(x, p, "m", gemm16)
            terms = {}
            if "m.noise_const" in p:
                terms["noise"] = float(np.abs(p["m.noise_const"] * p["m.noise_strength"]).max())
            if skip is not None:
                sk = T.read(skip, "out", cls)
                y = y + sk.astype(dt)
                terms["skip"] = float(np.abs(sk).max())
            return y, terms
        fn.src = None if head else src
        out.append((name, cls, fn))

    r, prev = R, None
    while r >= 4:
        b = f"encoder.b{r}"
        sep(b + ".conv1", prev, "enc.conv1.fromrgb" if r == R else "enc.conv1", head=r == R)
        sep(b + ".conv2", b + ".conv1", "enc.conv2.down" if r > 4 else "enc.conv2.b4")
        prev = b + ".conv2"
        r //= 2
    r = 4
    while r <= R:
        b = f"synthesis.b{r}"
        sep(b + ".conv1", prev, "syn.conv1.up" if r > 4 else "syn.conv1.b4", skip=f"encoder.b{r}.conv1")
        sep(b + ".conv2", b + ".conv1", "syn.conv2")

        def img(dt, b=b, r=r):
            y = orc.pointwise(T.read(b + ".conv2", "out", "img").astype(dt), sd[b + ".torgb.weight"].astype(dt), sd[b + ".torgb.bias"].astype(dt))
            terms = {}
            if r > 4:
                up = orc.upsample2d(T.read(f"synthesis.b{r // 2}.img", "prev", "img").astype(dt))
                y = y + up
                terms["prev"] = float(np.abs(up).max())
            return y, terms
        img.src = b + ".conv2"
        out.append((b + ".img", "img", img))
        prev = b + ".conv2"
        r *= 2
    return out


def run_case(lib, pkg, mem, *, res, batch, storage="f32", gemm=None, knobs={}, hw=None, seed, report=None, tag=""):
    """One debug-plan forward of Generator(res) on `batch` images and every assertion of the layer test on it.  knobs: tuning knobs
    borrowed for the case; hw: (H, W) through migan_forward_hw.  -> the set of kernel symbols the forward launched (empty at H x W,
    where launch_info does not report them).  report: a dict that receives the per-unit rows and the wall time."""
    t0 = time.perf_counter()
    T = Taps(lib, pkg, mem, res=res, batch=batch, storage=storage, gemm=gemm, tune=knobs, hw=hw, seed=seed)
    t_device = time.perf_counter() - t0
    sixteen = storage != "f32"
    gemm16 = sixteen and T.gemm == "f16"
    close = dict(ulps=1, frac=0.05 if gemm16 else 0.02, top_ulps=0.5 if gemm16 else 0.0)
    us = units(T)
    assert len(us) == 5 * levels(res) == len(unit_names(res)), (tag, len(us))

    def reference(unit):
        name, cls, fn = unit
        w64, _ = fn(np.float64)
        w32, terms = fn(np.float32)
        if cls != "img":
            w64, w32 = orc.round_storage(w64, storage), orc.round_storage(w32, storage)
        want = w32 if sixteen else w64
        scale = max(1.0, float(np.abs(want).max()))
        ruler = float(np.abs(w32.astype(np.float64) - w64).max()) / scale
        return [name, cls, want, terms, scale, ruler, w32, w64]

    # the units are independent of each other (each reads the device's taps), and numpy releases the interpreter in its array loops:
    # the two oracle passes of every unit on a few threads, largest units first, keep the 256 x 256 case within seconds
    order = sorted(range(len(us)), key=lambda i: -T.t[us[i][0]].size)
    with ThreadPoolExecutor(max_workers=8) as pool:
        done = dict(zip(order, pool.map(reference, [us[i] for i in order])))
    res_rows = [done[i] for i in range(len(us))]
    failures, rows = [], []
    for name, cls, want, terms, scale, ruler, w32, w64 in res_rows:
        got = T.t[name]
        ks = T.kernels_of(name)
        who = f"{tag} {name} {ks}"
        is_img = cls == "img"
        const = 3e-5 if is_img else 2e-5
        if cls in RULER_BOUND:
            const = MARGIN * max(r[5] for r in res_rows if r[1] == cls)
        bound = const * scale
        if sixteen and not is_img:
            # (what storage_close grants the largest element; the guards below and the table use it)
            bound += (close["ulps"] + close["top_ulps"]) * float(storage_ulp(np.abs(want).max(), storage))
        if is_img and sixteen:
            feat = T.t[name[:-4] + ".conv2"]
            tw = T.sd[name[:-4] + ".torgb.weight"]
            bound += 3.0 * float(storage_ulp(np.abs(feat).max(), storage)) * float(np.abs(tw).max())
        assert got.shape == want.shape, (who, got.shape, want.shape)
        finite = bool(np.isfinite(got).all())
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        err = float(diff.max()) if finite else float("inf")
        moved = float((diff > 2e-5 * scale).mean()) if finite else 1.0
        rows.append(dict(case=tag, unit=name, cls=cls, wmax=float(np.abs(want).max()), ruler=ruler, err=err / scale, bound=bound / scale,
                         moved=moved, kernels=ks))
        if not finite:
            failures.append((name, ks, f"{int((~np.isfinite(got)).sum())} elements are not finite (unwritten output, or a read of unwritten memory)"))
            continue
        try:
            if is_img or (cls in RULER_BOUND and not sixteen):
                assert err <= bound, f"max abs error {err:.3e} over the bound {bound:.3e}"
            else:
                storage_close(got, want, storage, what=who, **close)
                if sixteen:
                    # the caps are conditions on the reference too: the mode's float32 oracle against the mode's float64 one
                    storage_close(w32, w64, storage, what=who + " (the reference alone: float32 oracle against float64)", **close)
        except AssertionError as e:
            failures.append((name, ks, str(e).strip().splitlines()[0] if not is_img else str(e), f"error/scale {err / scale:.3e} ruler {ruler:.3e}"))
        # a launch that drops an optional term must fail: the term is well above the bound (fp32 storage, whose bound is a fixed
        # constant; the same epilogues run in the 16-bit slices, where a storage step can exceed a small noise strength)
        for term, mag in terms.items():
            if not sixteen and not mag > 10 * bound:
                failures.append((name, ks, f"vacuous: the {term} term ({mag:.3e}) is below 10 x the bound ({bound:.3e})"))
    if report is not None:
        report.update(rows=rows, seconds=time.perf_counter() - t0, device_seconds=t_device,
                      kernels=sorted({k for _, k in T.launches}))
    print(format_rows(rows))
    assert not failures, (tag, "units over their bound (layer, kernel symbols, what)", failures)
    return {k for _, k in T.launches}


class WindowTaps(Taps):
    """A debug-plan forward whose taps stay on the device (GPU only, fp32 storage, batch 1): at the extent limit of the kernels the workspace
    is some 30 GiB.  x is drawn on the device; read() serves the rows of a tap under the current strip of the unit's output (self.strip =
    (o0, o1), set by run_window_case), with the rows of the input that strip depends on (tests/large_extent_case.py: in_rows, MARGIN)."""

    def __init__(self, lib, pkg, dev, *, res, hw, seed):
        import torch
        from tests.sepconv_case import CudaMem
        self.torch, mem = torch, CudaMem(dev)
        self.res, self.batch, self.storage = res, 1, "f32"
        self.hh, self.ww = hh, ww = hw
        self.sd = pkg.synth.make_state_dict(res, seed=seed)
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        self.xd = torch.empty((1, 4, hh, ww), device=dev).normal_(generator=g).mul_(0.7)
        h = pkg.hipbind.MiganHandle(lib, res, dtype="f32")
        try:
            h.set_streams(1)
            h.set_debug(True)
            self.gemm = h.gemm()
            keep = {k: mem.put(np.ascontiguousarray(v.reshape(1) if v.ndim == 0 else v)) for k, v in self.sd.items()}
            for name, shape, _ in h.weights():
                h.set_weight(name, mem.ptr(keep[name]), shape)
            h.commit(mem.stream)
            self.need = h.workspace_bytes_hw(1, hh, ww)
            print(f"workspace_bytes_hw(1, {hh}, {ww}) of the debug plan: {self.need} bytes ({self.need / 2 ** 30:.2f} GiB)")
            self.yd = torch.empty((1, 3, hh, ww), device=dev)
            self.yd.view(torch.uint8).fill_(NAN_BYTE)
            self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev).fill_(NAN_BYTE)
            assert self.ws.data_ptr() % 256 == 0
            h.forward_hw(self.xd.data_ptr(), self.yd.data_ptr(), 1, hh, ww, self.ws.data_ptr(), self.need, mem.stream)
            mem.sync()
            self.where = {n: h.debug_tensor_hw(1, hh, ww, n) for n in unit_names(res) if n != f"synthesis.b{res}.img"}
        finally:
            h.close()
        self.launches, self._local = [], threading.local()

    @property
    def strip(self):                      # per thread: run_window_case evaluates the units on a few threads
        return self._local.strip

    @strip.setter
    def strip(self, v):
        self._local.strip = v

    def dev_tensor(self, name):
        """(tensor on the device, True if NCHW): the network input, y and the images are planar, the feature maps NHWC"""
        if name is None:
            return self.xd, True
        if name == f"synthesis.b{self.res}.img":
            return self.yd, True
        off, shape = self.where[name]
        n = int(np.prod(shape))
        return self.ws[off:off + 4 * n].view(self.torch.float32).view(*[int(v) for v in shape]), name.endswith(".img")

    def rows(self, name, r0, r1):
        t, planar = self.dev_tensor(name)
        return t[:, :, r0:r1].cpu().numpy() if planar else nchw(t[:, r0:r1].cpu().numpy())

    def read(self, name, role, cls):
        from tests.large_extent_case import in_rows
        o0, o1 = self.strip
        if role == "in":
            o0, o1 = in_rows(o0, o1, 2 if cls == "enc.conv2.down" else 1, 2 if cls == "syn.conv1.up" else 1)
        elif role == "prev":
            o0, o1 = o0 // 2, (o1 + 1) // 2
        return self.rows(name, o0, o1)

    def noise(self, p):
        """noise_const [r][r] is tiled periodically down the layer (orc.noise_plane): the strip starts at row o0 of it"""
        if "m.noise_const" in p:
            p["m.noise_const"] = np.roll(p["m.noise_const"], -(self.strip[0] % p["m.noise_const"].shape[0]), axis=0)
        return p


WHOLE_BELOW = 1 << 22          # elements: smaller units are evaluated whole, the others on the row windows of tests/large_extent_case.py


def run_window_case(lib, pkg, dev, *, res, hw, seed, tag="", report=None):
    """run_case for a size whose taps cannot visit the host: one debug-plan forward through migan_forward_hw, then every unit on row
    windows of its output (the first rows, the last, the strips around byte 2^31 of its input and output, four seeded random strips), from
    the device's own input rows, under the same bounds and guards as run_case.  Every tap is finite everywhere (checked on the device)."""
    from tests.large_extent_case import all_finite, strips
    t0 = time.perf_counter()
    T = WindowTaps(lib, pkg, dev, res=res, hw=hw, seed=seed)
    us = units(T)
    assert len(us) == 5 * levels(res) == len(unit_names(res)), (tag, len(us))

    def check(k):
        name, cls, fn = us[k]
        failures = []
        t, planar = T.dev_tensor(name)
        ho = int(t.shape[2] if planar else t.shape[1])
        is_img = cls == "img"
        if not all_finite(t):
            return None, [(name, "elements are not finite (unwritten output, or a read of unwritten memory)")]
        if t.numel() < WHOLE_BELOW:
            ss = [(0, ho, 0, ho, "whole")]
        else:
            src, src_planar = T.dev_tensor(fn.src)
            xb, yb = (0 if src_planar else src.numel() * 4), (0 if planar else t.numel() * 4)
            ss = strips(ho, max(1, xb // ho), max(1, yb // ho), xb, yb, seed + k)
        worst, bound_max, wmax, seen = 0.0, 0.0, 0.0, {}
        for o0, o1, c0, c1, sname in ss:
            T.strip = (o0, o1)
            want, terms = fn(np.float64)
            if not is_img:
                want = orc.round_storage(want, "f32")
            got = T.rows(name, o0, o1)
            assert got.shape == want.shape, (name, sname, got.shape, want.shape)
            wv, gv = want[:, :, c0 - o0:c1 - o0], got[:, :, c0 - o0:c1 - o0]
            scale = max(1.0, float(np.abs(wv).max()))
            bound = (3e-5 if is_img else 2e-5) * scale
            err = float(np.abs(gv.astype(np.float64) - wv.astype(np.float64)).max())
            if not err <= bound:
                failures.append((name, sname, f"rows [{c0}, {c1}): max abs error {err:.3e} over the bound {bound:.3e}"))
            worst, bound_max, wmax = max(worst, err / bound), max(bound_max, bound), max(wmax, float(np.abs(wv).max()))
            for term, mag in terms.items():
                seen[term] = max(seen.get(term, 0.0), mag)
        for term, mag in seen.items():
            if not mag > 10 * bound_max:
                failures.append((name, f"vacuous: the {term} term ({mag:.3e}) is below 10 x the bound ({bound_max:.3e})"))
        return (tag, name, cls, tuple(t.shape), len(ss), f"{wmax:.3g}", f"{worst:.3f}"), failures

    # the units are independent of each other (each reads the device's taps): a few threads, as in run_case
    with ThreadPoolExecutor(max_workers=8) as pool:
        done = list(pool.map(check, range(len(us))))
    rows = [r for r, _ in done if r is not None]
    failures = [f for _, fs in done for f in fs]
    print("| case | unit | class | shape | windows | max abs want | error / bound |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print("| " + " | ".join(str(v) for v in r) + " |")
    if report is not None:
        report.update(rows=rows, seconds=time.perf_counter() - t0, workspace_bytes=T.need)
    assert not failures, (tag, "units over their bound (layer, window, what)", failures)


def format_rows(rows):
    out = ["| case | unit | class | max abs want | ruler | device error | bound | error / bound | moved | kernels |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r['unit']} | {r['cls']} | {r['wmax']:.3g} | {r['ruler']:.2e} | {r['err']:.2e} | {r['bound']:.2e} | "
                   f"{r['err'] / r['bound']:.2f} | {r['moved']:.2%} | {'; '.join(k.replace('migan::', '') for k in r['kernels'])} |")
    return "\n".join(out)


# ---- the cases: the smallest that select each form.  The channel count is fixed by the resolution (512 up to 64 x 64), so a small R is
# already the hard K.  name -> run_case's arguments
GPU_F32 = {
    # the K-split tiles <0|3|2, 32, 32, 64>, small dwfir chunks
    "r32_b1": dict(res=32, batch=1, seed=201),
    # the KC-64 32-row tiles, the 32-row FIR-up tile; two 4 x 4 images per small tile with an odd batch
    "r32_b3": dict(res=32, batch=3, seed=202),
    "r32_b1_noksplit": dict(res=32, batch=1, seed=203, knobs=dict(small_ksplit=0)),
    "r32_b1_kc32": dict(res=32, batch=1, seed=204, knobs=dict(small_kc=32)),
    "r32_b1_kc32_up64": dict(res=32, batch=1, seed=205, knobs=dict(small_kc=32, small_up32=0)),
    "r32_b1_kc64_up64": dict(res=32, batch=1, seed=206, knobs=dict(small_kc=64, small_up32=0)),
    # the control: the regular multi-image tiles at the same sizes
    "r32_b1_small0": dict(res=32, batch=1, seed=207, knobs=dict(small=0)),
    # the K-split tile exceeds small_max_wgs at 64 x 64: the plan falls through to the next small tile
    "r64_b1": dict(res=64, batch=1, seed=208),
    # the deployed single-image path: pipelined kernels at 256 x 256, wide, fused-ToRGB tiles, small tiles below
    "r256_b1": dict(res=256, batch=1, seed=209),
}
GPU_16BIT = {
    # the small tiles of the (3, 1) and (3, 2) slices
    "r32_b1_bf16": dict(res=32, batch=1, seed=211, storage="bf16"),
    "r32_b3_bf16": dict(res=32, batch=3, seed=212, storage="bf16"),
    "r32_b1_f16": dict(res=32, batch=1, seed=213, storage="f16"),
    "r32_b3_f16": dict(res=32, batch=3, seed=214, storage="f16"),
    # the f16x2 slice of 16-bit storage has no small tiles: the regular tiles in plan context
    "r32_b1_bf16_f16x2": dict(res=32, batch=1, seed=215, storage="bf16", gemm="f16x2"),
}
# knob variants of the 16-bit slices: the KC-32 tiles and the 64-row FIR-up tiles exist there too
GPU_16BIT_KNOBS = {
    "r32_b1_bf16_kc32": dict(res=32, batch=1, seed=216, storage="bf16", knobs=dict(small_kc=32)),
    "r32_b1_bf16_kc32_up64": dict(res=32, batch=1, seed=217, storage="bf16", knobs=dict(small_kc=32, small_up32=0)),
    "r32_b1_bf16_kc64_up64": dict(res=32, batch=1, seed=218, storage="bf16", knobs=dict(small_kc=64, small_up32=0, small_ksplit=0)),
    "r32_b1_f16_kc32": dict(res=32, batch=1, seed=219, storage="f16", knobs=dict(small_kc=32)),
    "r32_b1_f16_kc32_up64": dict(res=32, batch=1, seed=220, storage="f16", knobs=dict(small_kc=32, small_up32=0)),
    "r32_b1_f16_kc64_up64": dict(res=32, batch=1, seed=221, storage="f16", knobs=dict(small_kc=64, small_up32=0, small_ksplit=0)),
}
# other sizes: ragged FIR-up small tiles (3 x 5, 6 x 10, ...); the plain layers fall back to regular ragged tiles where w % 8 != 0
GPU_HW = {
    "r64_48x80_b1": dict(res=64, batch=1, seed=231, hw=(48, 80)),
    "r64_48x80_b2": dict(res=64, batch=2, seed=232, hw=(48, 80)),
}
GPU_CASES = {**GPU_F32, **GPU_16BIT, **GPU_16BIT_KNOBS, **GPU_HW}

EMU_CASES = {
    "r16_b1": dict(res=16, batch=1, seed=241),
    "r16_b2": dict(res=16, batch=2, seed=242),
    "r16_b3": dict(res=16, batch=3, seed=246),
    "r16_b1_bf16": dict(res=16, batch=1, seed=243, storage="bf16"),
    "r16_b3_bf16": dict(res=16, batch=3, seed=247, storage="bf16"),
    "r16_b1_f16": dict(res=16, batch=1, seed=248, storage="f16"),
    "r16_b1_kc32_up64": dict(res=16, batch=1, seed=244, knobs=dict(small_kc=32, small_up32=0)),
    "r16_12x20_b1": dict(res=16, batch=1, seed=245, hw=(12, 20)),
}

"""One SeparableConv2d through migan_sepconv_forward on tensors near the extent limit of the kernels (kMaxImageElems in migan_host.hpp:
2^30 - 1024 elements per image), which never visit the host.  GPU only: the emulator cannot run 2^30 elements.

x, skip, the noise plane and the previous image are drawn on the device from a seeded generator; y, img_out and scratch start as NaN bytes.
What comes back to the host are ROW WINDOWS, full width: a strip of output rows plus the rows of every input the strip depends on.  The
float64 oracle of tests/sepconv_case.py (16-bit storage: the mode's oracle) evaluates each window as an image of its own, and only the rows
whose support lies inside the strip -- or at a true image border, where the oracle's zero padding is the layer's own -- are compared, under
sepconv_case's bounds.  Every pixel in between is covered by `isfinite` on the device and by BAND CONSISTENCY: the same layer run on bands
of at most 2^29 bytes (sizes the rest of the suite ties to the oracle) must reproduce the big run within twice the bound, both runs being
within the bound of the exact value.  Test infrastructure only."""
import time

import numpy as np
import torch

from oracle import migan_oracle as orc
from tests.emu_util import nchw, storage_ulp, storage_close
from tests.sepconv_case import weights

# Rows of a strip, at each end that is not an image border, whose support may leave the strip (in OUTPUT rows; strips start on even
# output rows).  plain: the 3 x 3 taps reach 1 row.  FIR-up: output row o reads GEMM rows o/2 - 1 .. o/2 + 1 (4 x 4 FIR on the zero-
# inserted grid), each 3 x 3 rows of x: 2 input rows = 4 output rows.  down=2: output row o reads depthwise rows 2o - 1 .. 2o + 2, each
# 3 x 3 rows of x: input rows 2o - 2 .. 2o + 3, that is 1 output row before and 2 after (1.5 rounded up).  The previous image of a
# ToRGB tail is half size: output row o reads rows o/2 - 1 .. o/2 + 1 of it, 2 output rows.  One margin for all: the largest, 4.
MARGIN = 4
ROWS = 8                  # compared rows of an interior strip
BAND_BYTES = 1 << 29
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def out_size(h, w, down, up):
    return (h // 2, w // 2) if down == 2 else ((h * 2, w * 2) if up == 2 else (h, w))


def in_rows(o0, o1, down, up):
    """input rows under the output rows [o0, o1) (o0 even; o1 even or the last row)"""
    if down == 2:
        return 2 * o0, 2 * o1
    if up == 2:
        return o0 // 2, (o1 + 1) // 2
    return o0, o1


class Layer:
    """weights on the device plus everything the oracle needs, for one layer shape"""

    def __init__(self, pkg, dev, *, cin, cout, down, up, noise, fromrgb, torgb, seed):
        self.cin, self.cout, self.down, self.up, self.noise, self.fromrgb, self.torgb = cin, cout, down, up, noise, fromrgb, torgb
        sd = weights(pkg, cin, cout, seed, (1, 1), False)
        self.sd = sd
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.w1, self.b1, self.w2 = put(sd["m.conv1.weight"]), put(sd["m.conv1.bias"]), put(sd["m.conv2.weight"])
        self.strength = np.asarray(0.37, dtype=np.float32)
        self.ns = put(self.strength.reshape(1))
        wsp_n = (3 * cin * cout + 1) // 2 + 8
        self.wsp = torch.full((wsp_n,), float("nan"), device=dev)
        if fromrgb:
            self.fw = (pkg.synth.normal((cin, 4, 1, 1), seed, "fw") * 0.7).astype(np.float32)
            self.fb = (pkg.synth.normal((cin,), seed, "fb") * 0.3).astype(np.float32)
            self.fw_d, self.fb_d = put(self.fw), put(self.fb)
        if torgb:
            self.tw = (pkg.synth.normal((3, cout, 1, 1), seed, "tw") / np.sqrt(cout)).astype(np.float32)
            self.tb = (pkg.synth.normal((3,), seed, "tb") * 0.2).astype(np.float32)
            self.tw_d, self.tb_d = put(self.tw), put(self.tb)

    def want(self, x, noise, skip, prev, storage):
        """the oracle on one window taken as an image of its own: x NCHW (fromrgb: the raw 4-channel input), noise [ho][wo], skip NCHW,
        prev NCHW [.,3,ho/2,wo/2]; returns (feature map rounded to storage, ToRGB image or None)"""
        odt = np.float64 if storage == "f32" else np.float32
        osd = dict(self.sd)
        if self.down == 2:
            osd["m.downsample.filter.weight"] = np.broadcast_to(orc.fir_taps(1.0), (self.cin, 1, 4, 4)).astype(np.float32)
        if self.up == 2:
            osd["m.upsample.filter.weight"] = np.broadcast_to(orc.fir_taps(4.0), (self.cout, 1, 4, 4)).astype(np.float32)
        if noise is not None:
            osd["m.noise_const"], osd["m.noise_strength"] = noise, self.strength
        if self.fromrgb:
            x = orc.lrelu_agc(orc.pointwise(x.astype(odt), self.fw, self.fb))
        want = orc.separable_conv(x.astype(odt), osd, "m", storage != "f32")
        if skip is not None:
            want = want + skip
        want = orc.round_storage(want, storage)
        img = None
        if self.torgb:
            img = orc.pointwise(want, self.tw, self.tb)
            if prev is not None:
                img = img + orc.upsample2d(prev.astype(odt))
        return want, img


def nan_bytes(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.int8).fill_(-1)                   # 0xff bytes: a NaN in fp32, bf16 and fp16
    return t


def all_finite(t):
    """isfinite(t).all() on the device, in pieces (no boolean copy of a 4 GiB tensor)"""
    flat = t.reshape(-1)
    step = 1 << 28
    return all(bool(torch.isfinite(flat[i:i + step]).all()) for i in range(0, flat.numel(), step))


def call(lib, L, storage, *, x, y, skip, noise, prev, img_out, scratch, batch, h, w, samples=None):
    ho, wo = out_size(h, w, L.down, L.up)
    p = lambda t: None if t is None else t.data_ptr()
    kw = {}
    if L.fromrgb:
        kw.update(fromrgb_weight=p(L.fw_d), fromrgb_bias=p(L.fb_d))
    if L.torgb:
        kw.update(torgb_weight=p(L.tw_d), torgb_bias=p(L.tb_d), img_out=p(img_out), img_prev=p(prev))
    lib.sepconv_forward(stream=int(torch.cuda.current_stream().cuda_stream), samples=samples, x=p(x), y=p(y), skip=p(skip),
                        conv1_weight=p(L.w1), conv1_bias=p(L.b1), conv2_weight=p(L.w2), noise_const=p(noise),
                        noise_strength=p(L.ns) if noise is not None else None, batch=batch, cin=L.cin, cout=L.cout, res_in=h, width_in=w,
                        down=L.down, up=L.up, scratch=p(scratch), scratch_bytes=0 if scratch is None else scratch.numel() * 4,
                        wsplit=p(L.wsp), wsplit_bytes=L.wsp.numel() * 4, dtype={"f32": 0, "bf16": 1, "f16": 2}[storage], gemm=-1, **kw)


def strips(ho, row_bytes_x_per_out_row, row_bytes_y, x_bytes, y_bytes, seed):
    """output-row strips (o0, o1, first compared row, end of compared rows, name) of one case"""
    def around(r, name):                       # compared rows [r - ROWS/2, r + ROWS/2): row r and the row before it are both in
        c0 = max(0, min(r - ROWS // 2, ho - ROWS)) & ~1
        return interior(c0, name)

    def interior(c0, name):
        c0 = max(0, min(c0, ho - ROWS)) & ~1
        c1 = min(ho, c0 + ROWS)
        o0 = 0 if c0 < MARGIN else c0 - MARGIN
        o1 = ho if c1 + MARGIN >= ho else c1 + MARGIN
        return (o0, o1, 0 if o0 == 0 else c0, ho if o1 == ho else c1, name)

    out = [interior(0, "first"), interior(ho, "last")]
    if x_bytes > 1 << 31:
        out.append(around((1 << 31) // row_bytes_x_per_out_row, "x@2^31"))
    if y_bytes > 1 << 31:
        s = around((1 << 31) // row_bytes_y, "y@2^31")
        r = (1 << 31) // row_bytes_y
        assert s[2] <= r - 1 and r < s[3], "a compared row on each side of byte 2^31 of y"
        out.append(s)
    rng = np.random.default_rng(seed)
    out += [interior(int(r), f"random{i}") for i, r in enumerate(rng.integers(0, max(1, ho - ROWS), 4))]
    seen, uniq = {}, []
    for s in out:                              # a plain layer's x and y cross byte 2^31 in the same row: one window, both names
        if s[:4] in seen:
            uniq[seen[s[:4]]] = s[:4] + (uniq[seen[s[:4]]][4] + " = " + s[4],)
        else:
            seen[s[:4]] = len(uniq)
            uniq.append(s)
    return uniq


def run_large_case(lib, pkg, dev, *, cin, cout, h, w, down=1, up=1, noise=False, skip=False, fromrgb=False, torgb=False, with_prev=False,
                   storage="f32", seed=41, kernel=None, kernel_prefix=None, bands=True, rows=0):
    """rows = S > 0: the per-row form (migan_sepconv_forward_samples) at n = 1: S rows of x, y and noise planes, one skip tensor; every row
    gets the windows and the bands (the bands run the per-row form too, at S = 1 with the row's own plane).
    Returns the report row: kernel, bytes per image, worst window error / bound, worst band error / bound, seconds"""
    nb = rows or 1
    t0 = time.time()
    tdt, esz = TORCH_DT[storage], 4 if storage == "f32" else 2
    ho, wo = out_size(h, w, down, up)
    L = Layer(pkg, dev, cin=cin, cout=cout, down=down, up=up, noise=noise, fromrgb=fromrgb, torgb=torgb, seed=seed)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    draw = lambda shape, scale: torch.empty(shape, device=dev, dtype=torch.float32).normal_(generator=g).mul_(scale)
    if fromrgb:
        x = draw((nb, 4, h, w), 0.8)
    else:
        x = draw((nb, h, w, cin), 1.5).to(tdt)           # 16-bit storage: rounded on the device
    sk = draw((1, ho, wo, cout), 1.0).to(tdt) if skip else None
    nzs = draw((nb, ho, wo), 1.0) if noise else None
    prev = draw((nb, 3, ho // 2, wo // 2), 1.0) if (torgb and with_prev) else None
    y = nan_bytes((nb, ho, wo, cout), tdt, dev)
    img_out = nan_bytes((nb, 3, ho, wo), torch.float32, dev) if torgb else None
    scratch = nan_bytes((1, ho, wo, cin), torch.float32, dev) if down == 2 else None
    call(lib, L, storage, x=x, y=y, skip=sk, noise=nzs, prev=prev, img_out=img_out, scratch=scratch, batch=nb, h=h, w=w, samples=rows or None)
    torch.cuda.synchronize()
    ran = lib.last_kernel()
    if kernel is not None:
        assert ran == kernel, (ran, kernel)
    if kernel_prefix is not None:
        assert ran.startswith(kernel_prefix), (ran, kernel_prefix)
    assert all_finite(y), "the kernel left NaNs (unwritten output) or produced one"
    if torgb:
        assert all_finite(img_out), "img_out holds NaNs"

    x_bytes = x[0].numel() * x.element_size()
    y_bytes = y[0].numel() * esz
    X, Y, PREV, IMG = x, y, prev, img_out
    x_row_per_out = x_bytes // ho if not fromrgb else (1 << 62)      # (the NCHW input of FromRGB has no byte 2^31: 4 channels)
    host = lambda t: t.float().cpu().numpy()
    worst_w, top, guard = 0.0, 1.0, {"skip": 0.0, "noise": 0.0, "prev": 0.0}
    for row, (o0, o1, c0, c1, name) in ((r, s) for r in range(nb)
                                        for s in strips(ho, x_row_per_out, wo * cout * esz, 0 if fromrgb else x_bytes, y_bytes, seed + r)):
        x, y, nz = X[row:row + 1], Y[row:row + 1], nzs[row] if noise else None
        prev, img_out = PREV[row:row + 1] if PREV is not None else None, IMG[row:row + 1] if IMG is not None else None
        name = f"{name}" if not rows else f"row {row} {name}"
        i0, i1 = in_rows(o0, o1, down, up)
        xs = host(x[:, :, i0:i1]) if fromrgb else nchw(host(x[:, i0:i1]))
        want, want_img = L.want(xs, host(nz[o0:o1]) if noise else None, nchw(host(sk[:, o0:o1])) if skip else None,
                                host(prev[:, :, o0 // 2:(o1 + 1) // 2]) if prev is not None else None, storage)
        got = nchw(host(y[:, o0:o1]))
        a, b = c0 - o0, c1 - o0
        assert b > a
        gemm16 = storage != "f32"
        wv, gv = want[:, :, a:b], got[:, :, a:b]
        atol = 2e-5 * max(1.0, float(np.abs(wv).max()))
        print(f"  window {name}: rows [{c0}, {c1}) max err {float(np.abs(gv - wv).max()):.3e} bound {atol:.3e}")
        storage_close(gv, wv, storage, ulps=1, frac=0.05 if gemm16 else 0.02, top_ulps=0.5 if gemm16 else 0.0, what=name)
        if storage == "f32":
            worst_w = max(worst_w, float(np.abs(gv - wv).max()) / atol)
        top = max(top, float(np.abs(wv).max()))
        if skip:
            guard["skip"] = max(guard["skip"], float(np.abs(host(sk[:, c0:c1])).max()) / atol)
        if noise:       # added before the activation, whose slope is at least 0.2 * sqrt(2) below the clamp
            guard["noise"] = max(guard["noise"], 0.2 * np.sqrt(2) * 0.37 * float(np.abs(host(nz[c0:c1])).max()) / atol)
        if torgb:
            iv, gi = want_img[:, :, a:b], host(img_out[:, :, o0:o1])[:, :, a:b]
            iatol = 3e-5 * max(1.0, float(np.abs(iv).max()))
            if storage != "f32":
                iatol += 3.0 * float(storage_ulp(np.abs(wv).max(), storage)) * float(np.abs(L.tw).max())
            print(f"  window {name}: img max err {float(np.abs(gi - iv).max()):.3e} bound {iatol:.3e}")
            np.testing.assert_allclose(gi, iv, rtol=0, atol=iatol, err_msg=name)
            worst_w = max(worst_w, float(np.abs(gi - iv).max()) / iatol)
            if prev is not None:        # interior rows of the window: every tap of the FIR lands on drawn values
                guard["prev"] = max(guard["prev"], float(np.abs(orc.upsample2d(host(prev[:, :, o0 // 2:(o1 + 1) // 2]).astype(np.float64))
                                                               [:, :, a:b]).max()) / iatol)
    if storage == "f32":        # vacuity guard: a kernel that dropped the term would be far outside the bound
        for term, on in (("skip", skip), ("noise", noise), ("prev", prev is not None)):
            assert not on or guard[term] > 10.0, f"the {term} term never exceeds 10 x the bound inside the compared rows"

    worst_b = 0.0
    for row in range(nb if bands else 0):
        worst_b = max(worst_b, band_consistency(lib, L, storage, x=X[row:row + 1], y=Y[row:row + 1], sk=sk, nz=nzs[row] if noise else None,
                                                prev=PREV[row:row + 1] if PREV is not None else None,
                                                img_out=IMG[row:row + 1] if IMG is not None else None, h=h, w=w, top=top,
                                                samples=1 if rows else None))
    del x, y, X, Y, sk, nzs, nz, prev, PREV, img_out, IMG, scratch
    torch.cuda.empty_cache()
    return dict(kernel=ran, image_bytes=max(x_bytes, y_bytes), window=worst_w, band=worst_b, seconds=time.time() - t0)


def band_consistency(lib, L, storage, *, x, y, sk, nz, prev, img_out, h, w, top, samples=None):
    """the layer again on bands of at most 2^29 bytes (first row a multiple of 64) plus halo, each a tensor of its own; the band's interior
    rows against the big run, on the device.  Returns the worst error over its bound (twice the operator's)."""
    dev, tdt, esz = y.device, y.dtype, y.element_size()
    down, up, cin, cout = L.down, L.up, L.cin, L.cout
    ho, wo = out_size(h, w, down, up)
    in_per_out = (h * w * (4 if L.fromrgb else cin) * (4 if L.fromrgb else esz)) // ho
    rows = max(64, (BAND_BYTES // max(in_per_out, wo * cout * esz)) // 64 * 64 - 64)      # (the halo stays inside the 2^29 bytes)
    halo = 8                                                                                # output rows, even, >= MARGIN
    bound = 2.0 * 2e-5 * top
    ibound = 2.0 * 3e-5 * top
    if storage != "f32":        # the two runs may round an element to neighbouring storage values
        bound += 2.0 * 1.5 * float(storage_ulp(top, storage))
        ibound += 2.0 * 3.0 * float(storage_ulp(top, storage)) * float(np.abs(L.tw).max()) if L.torgb else 0.0
    worst = 0.0
    for b0 in range(0, ho, rows):
        b1 = min(ho, b0 + rows)
        o0, o1 = max(0, b0 - halo), (ho if b1 + halo >= ho else b1 + halo)
        i0, i1 = in_rows(o0, o1, down, up)
        xb = x[:, :, i0:i1].contiguous() if L.fromrgb else x[:, i0:i1]          # NHWC row slices are contiguous: no copy
        skb = sk[:, o0:o1] if sk is not None else None
        nzb = nz[o0:o1] if nz is not None else None
        pb = prev[:, :, o0 // 2:(o1 + 1) // 2].contiguous() if prev is not None else None
        yb = nan_bytes((1, o1 - o0, wo, cout), tdt, dev)
        ib = nan_bytes((1, 3, o1 - o0, wo), torch.float32, dev) if L.torgb else None
        sb = nan_bytes((1, o1 - o0, wo, cin), torch.float32, dev) if down == 2 else None
        assert all(t is None or t.is_contiguous() for t in (xb, skb, nzb))
        call(lib, L, storage, x=xb, y=yb, skip=skb, noise=nzb, prev=pb, img_out=ib, scratch=sb, batch=1, h=i1 - i0, w=w, samples=samples)
        torch.cuda.synchronize()
        assert samples is None or "_rows_kernel<" in lib.last_kernel(), lib.last_kernel()
        d = float((yb[:, b0 - o0:b1 - o0].float() - y[:, b0:b1].float()).abs().max())
        assert d == d and d <= bound, f"band rows [{b0}, {b1}): {d:.3e} apart from the big run, bound {bound:.3e}"
        worst = max(worst, d / bound)
        if L.torgb:
            d = float((ib[:, :, b0 - o0:b1 - o0] - img_out[:, :, b0:b1]).abs().max())
            assert d == d and d <= ibound, f"band rows [{b0}, {b1}): img {d:.3e} apart from the big run, bound {ibound:.3e}"
            worst = max(worst, d / ibound)
        del xb, yb, ib, sb, pb
    return worst


def run_batch_case(lib, pkg, dev, *, cin, cout, h, w, batch, noise=False, skip=False, fromrgb=False, torgb=False, with_prev=False, seed=43,
                   kernel=None, kernel_prefix=None, **_):
    """small images, a whole batch above 2^32 bytes (fp32 storage, plain layers): the windows are whole images -- the first, the last, and
    those that contain byte 2^31 and byte 2^32 of x and of y (and their neighbours, so that both sides of each boundary are compared).
    Band consistency: the same layer on sub-batches of at most 2^29 bytes, each a tensor of its own."""
    t0 = time.time()
    L = Layer(pkg, dev, cin=cin, cout=cout, down=1, up=1, noise=noise, fromrgb=False, torgb=False, seed=seed)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    draw = lambda shape, scale: torch.empty(shape, device=dev, dtype=torch.float32).normal_(generator=g).mul_(scale)
    x = draw((batch, h, w, cin), 1.5)
    sk = draw((batch, h, w, cout), 1.0) if skip else None
    nz = draw((h, w), 1.0) if noise else None
    y = nan_bytes((batch, h, w, cout), torch.float32, dev)
    call(lib, L, "f32", x=x, y=y, skip=sk, noise=nz, prev=None, img_out=None, scratch=None, batch=batch, h=h, w=w)
    torch.cuda.synchronize()
    ran = lib.last_kernel()
    assert kernel is None or ran == kernel, (ran, kernel)
    assert kernel_prefix is None or ran.startswith(kernel_prefix), (ran, kernel_prefix)
    assert all_finite(y), "the kernel left NaNs (unwritten output) or produced one"
    xi, yi = h * w * cin * 4, h * w * cout * 4
    picks = {0, batch - 1}
    for per_image in (xi, yi):
        for edge in (1 << 31, 1 << 32):
            if per_image * batch > edge:
                picks.update(i for i in (edge // per_image - 1, edge // per_image) if 0 <= i < batch)
    assert yi * batch > 1 << 32 and (1 << 32) // yi in picks
    host = lambda t: t.float().cpu().numpy()
    worst_w, top, gs, gn = 0.0, 1.0, 0.0, 0.0
    for i in sorted(picks):
        want, _ = L.want(nchw(host(x[i:i + 1])), host(nz) if noise else None, nchw(host(sk[i:i + 1])) if skip else None, None, "f32")
        got = nchw(host(y[i:i + 1]))
        atol = 2e-5 * max(1.0, float(np.abs(want).max()))
        print(f"  image {i}: max err {float(np.abs(got - want).max()):.3e} bound {atol:.3e}")
        storage_close(got, want, "f32", ulps=1, frac=0.02, what=f"image {i}")
        worst_w, top = max(worst_w, float(np.abs(got - want).max()) / atol), max(top, float(np.abs(want).max()))
        gs = max(gs, float(sk[i].abs().max()) / atol) if skip else gs
        gn = max(gn, 0.2 * np.sqrt(2) * 0.37 * float(nz.abs().max()) / atol) if noise else gn
    assert (not skip or gs > 10.0) and (not noise or gn > 10.0), "a term never exceeds 10 x the bound"
    step = max(1, BAND_BYTES // max(xi, yi))
    bound, worst_b = 2.0 * 2e-5 * top, 0.0
    for b0 in range(0, batch, step):
        b1 = min(batch, b0 + step)
        yb = nan_bytes((b1 - b0, h, w, cout), torch.float32, dev)
        call(lib, L, "f32", x=x[b0:b1], y=yb, skip=sk[b0:b1] if skip else None, noise=nz, prev=None, img_out=None, scratch=None,
             batch=b1 - b0, h=h, w=w)
        torch.cuda.synchronize()
        d = float((yb - y[b0:b1]).abs().max())
        assert d == d and d <= bound, f"images [{b0}, {b1}): {d:.3e} apart from the big run, bound {bound:.3e}"
        worst_b = max(worst_b, d / bound)
        del yb
    del x, y, sk, nz
    torch.cuda.empty_cache()
    return dict(kernel=ran, image_bytes=max(xi, yi), batch_bytes=max(xi, yi) * batch, window=worst_w, band=worst_b, seconds=time.time() - t0)

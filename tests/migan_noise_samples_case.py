"""MI-GAN: S completions per image from per-row noise (include/migan_noise_samples_hip.h), through the C ABI.  Shared by
tests/test_emu_migan_noise_samples.py (product kernel source on the CPU emulator, host memory) and tests/test_gpu_migan_noise_samples.py
(libmigan_hip.so on an MI355X).  Test infrastructure only.

What is checked, and against what:
  * const noise: every row's blob = the model's own noise_const planes (tiled and cropped at H x W) -> every row i * S + s holds the BITS of
    migan_forward_hw's row i.  Any wrong row / S, skip image, noise stride or row copy shows here.
  * independence: swapping the blobs of two samples of an image swaps exactly those two output rows; changing one row's blob changes no
    other row; different blobs give different rows.  Always within one batch shape (the plan picks kernel forms by batch).
  * one SeparableConv2d through migan_sepconv_forward_samples against oracle/migan_oracle.py, evaluated row by row at batch 1 with that
    row's plane as noise_const and image row // S of the skip tensor; bounds: tests/sepconv_case.py's (storage_close, the ToRGB atol).
  * host guards: every MIGAN_EINVAL leaves y and the workspace untouched."""
import numpy as np
import pytest

from oracle import migan_oracle as orc
from tests.emu_util import aligned, from_storage, nchw, nhwc, storage_close, storage_ulp, to_storage
from tests.last_store_case import FILL, Bound
from tests.sepconv_case import weights


def noise_layers(res, hw=None):
    """[(state_dict key, h, w)] of the noisy layers in blob order"""
    hh, ww = hw or (res, res)
    out, r = [], 8
    while r <= res:
        out += [(f"synthesis.b{r}.{c}.noise_const", hh * r // res, ww * r // res) for c in ("conv1", "conv2")]
        r *= 2
    return out


def const_blob(sd, res, hw=None):
    """the model's own planes as one blob: noise_const tiled periodically and cropped to its layer's size (migan_forward_hw's rule)"""
    planes = []
    for key, h, w in noise_layers(res, hw):
        c = sd[key]
        r = c.shape[0]
        planes.append(np.tile(c, ((h + r - 1) // r, (w + r - 1) // r))[:h, :w].reshape(-1))
    return np.concatenate(planes).astype(np.float32)


class SamplesBound(Bound):
    """tests/last_store_case.py's Generator behind the C ABI, with the samples forward"""

    def __init__(self, pkg, lib, mem, res, seed, dtype=0, streams=2):
        """streams = 2 is the library's default (and the Python Generator's): from 16 rows on the rows then run in two sub-batches"""
        super().__init__(pkg, lib, mem, res, seed, dtype=dtype)
        self.h.set_streams(streams)

    def forward_samples_hw(self, x, noise, ws_bytes=None, y_fill=np.nan):
        """x [n,4,H,W], noise [n,S,F] -> (y [n*S,3,H,W], workspace bytes after the call)"""
        n, _, hh, ww = x.shape
        s = noise.shape[1]
        need = self.h.workspace_bytes_samples_hw(n, s, hh, ww)
        xd, nd = self.mem.put(aligned(x)), self.mem.put(aligned(noise))
        yd = self.mem.put(aligned(np.full((n * s, 3, hh, ww), y_fill, np.float32)))
        wd = self.mem.put(np.full(need + 256, FILL, np.uint8).view(np.float32))
        try:
            self.h.forward_samples_hw(self.mem.ptr(xd), self.mem.ptr(nd), self.mem.ptr(yd), n, s, hh, ww, self.mem.ptr(wd),
                                      need if ws_bytes is None else ws_bytes, self.mem.stream)
        finally:
            self.mem.sync()
            self.last_y = np.array(self.mem.get(yd))
            self.last_ws = np.array(self.mem.get(wd)).view(np.uint8)
        return self.last_y, self.last_ws


def check_const_noise_gives_forward_bits(pkg, lib, mem, res, hw, n, s, dtype="f32", seed=31, streams=2):
    """-> the bound generator, x and forward_hw's y, for further checks on the same batch"""
    hh, ww = hw
    g = SamplesBound(pkg, lib, mem, res, seed, dtype=pkg.hipbind.dtype_code(dtype), streams=streams)
    f = g.h.noise_floats_hw(hh, ww)
    blob = const_blob(g.sd, res, hw)
    assert f == blob.size == sum(h * w for _, h, w in noise_layers(res, hw)), (f, blob.size)
    x = (pkg.synth.normal((n, 4, hh, ww), seed, "xns") * 0.7).astype(np.float32)
    want, _, _ = g.forward_hw(x)
    assert np.isfinite(want).all()
    noise = np.broadcast_to(blob, (n, s, f)).copy()
    y, _ = g.forward_samples_hw(x, noise)
    assert np.isfinite(y).all(), "the samples forward left rows unwritten"
    for i in range(n):
        for k in range(s):
            np.testing.assert_array_equal(y[i * s + k], want[i], err_msg=f"row {i * s + k} (image {i}, sample {k}) of {res} at {hw}, {dtype}")
    # and the plain forward afterwards is what it was (the samples call shares the handle, the planes and the kernels' tables with it)
    again, _, _ = g.forward_hw(x)
    np.testing.assert_array_equal(again, want)
    return g, x, want


K_SPLIT_ROWS = r"migan::sepconv_rows_kernel<[^,]+, 32, 32, "       # the 32 x 32 K-split tile (four partial sums over K), per-row form


def check_single_image_runs_the_k_split_rows_form(pkg, lib, mem, res, s, dtype="f32"):
    """n = 1 (the pipeline's ordinary last chunk) with S > 1: the only call in which the K-split tiles, which a forward picks for a single
    image alone, run their per-row form with several rows.  Bits of forward's single image, the symbol among the launches, independence."""
    import re
    g, x, _ = check_const_noise_gives_forward_bits(pkg, lib, mem, res, (res, res), 1, s, dtype=dtype)
    check_rows_are_independent(pkg, g, x, s)
    launches = g.h.launches()                                # (of the call made last: a samples call)
    names = [d["kernel"] for d in launches]
    assert any(re.match(K_SPLIT_ROWS, k) for k in names), names
    assert not any("_rows_kernel<" in d["kernel"] for d in launches if d["layer"].startswith("encoder.")), names
    return names


def check_rows_are_independent(pkg, g, x, s, seed=37):
    """on the batch of `x` with S = s >= 2 samples: swap, single-row change, distinct rows"""
    n, _, hh, ww = x.shape
    f = g.h.noise_floats_hw(hh, ww)
    noise = pkg.synth.normal((n, s, f), seed, "blobs").astype(np.float32)
    y0, _ = g.forward_samples_hw(x, noise)
    assert np.isfinite(y0).all()
    for r in range(n * s):
        for q in range(r + 1, n * s):
            assert not np.array_equal(y0[r], y0[q]), f"rows {r} and {q} are the same image although their blobs differ"
    # swap the blobs of samples 0 and s - 1 of the last image: exactly those two output rows swap
    i, a, b = n - 1, 0, s - 1
    swapped = noise.copy()
    swapped[i, a], swapped[i, b] = noise[i, b], noise[i, a]
    y1, _ = g.forward_samples_hw(x, swapped)
    want = y0.copy()
    want[i * s + a], want[i * s + b] = y0[i * s + b], y0[i * s + a]
    np.testing.assert_array_equal(y1, want)
    # change one row's blob (first image, last sample): every other row keeps its bits
    changed = noise.copy()
    changed[0, s - 1] = pkg.synth.normal((f,), seed + 1, "other").astype(np.float32)
    y2, _ = g.forward_samples_hw(x, changed)
    for r in range(n * s):
        if r == s - 1:
            assert not np.array_equal(y2[r], y0[r]), "the changed blob did not change its row"
        else:
            np.testing.assert_array_equal(y2[r], y0[r], err_msg=f"row {r} changed with the blob of row {s - 1}")


def run_rows_sepconv_case(lib, pkg, mem, *, cin, cout, h, w=None, n=2, s=2, up=1, noise=True, skip=False, seed=5, storage="f32", gemm=-1,
                          torgb=False, with_prev=False, symbol=None):
    """one plain / FIR-up SeparableConv2d at batch n * s through migan_sepconv_forward_samples: noise_const [n*s][ho][wo], skip [n]..."""
    w = w or h
    batch = n * s
    ho, wo = (h * 2, w * 2) if up == 2 else (h, w)
    sd = weights(pkg, cin, cout, seed, (ho, wo), noise)
    planes = pkg.synth.normal((batch, ho, wo), seed, "row planes").astype(np.float32) if noise else None
    keep = []

    def dev(a):
        keep.append(mem.put(aligned(a) if a.dtype == np.float32 else a))
        return keep[-1]

    x = orc.round_storage((pkg.synth.normal((batch, cin, h, w), seed, "x") * 1.5).astype(np.float32), storage)
    sk = orc.round_storage(pkg.synth.normal((n, cout, ho, wo), seed, "skip").astype(np.float32), storage) if skip else None
    gemm16 = storage != "f32" and gemm != 2
    want = np.empty((batch, cout, ho, wo), np.float32)
    for b in range(batch):                                   # the oracle row by row, with that row's plane as the layer's noise_const
        osd = dict(sd)
        if up == 2:
            osd["m.upsample.filter.weight"] = np.broadcast_to(orc.fir_taps(4.0), (cout, 1, 4, 4)).astype(np.float32)
        if noise:
            osd["m.noise_const"] = planes[b]
        row = orc.separable_conv(x[b:b + 1], osd, "m", gemm16)
        if skip:
            row = row + sk[b // s:b // s + 1]
        want[b] = orc.round_storage(row, storage)[0]
    xin = dev(to_storage(nhwc(x), storage))
    y = dev(to_storage(np.full((batch, ho, wo, cout), np.nan, dtype=np.float32), storage))
    skh = dev(to_storage(nhwc(sk), storage)) if skip else None
    w1, b1, w2 = dev(sd["m.conv1.weight"]), dev(sd["m.conv1.bias"]), dev(sd["m.conv2.weight"])
    nc = dev(planes) if noise else None
    ns = dev(sd["m.noise_strength"].reshape(1)) if noise else None
    wsp_n = (3 * cin * cout + 1) // 2 + 8
    wsp = dev(np.full(wsp_n, np.nan, dtype=np.float32))
    kw, img_out, want_img, tw = {}, None, None, None
    if torgb:
        tw = (pkg.synth.normal((3, cout, 1, 1), seed, "tw") / np.sqrt(cout)).astype(np.float32)
        tb = (pkg.synth.normal((3,), seed, "tb") * 0.2).astype(np.float32)
        img_out = dev(np.full((batch, 3, ho, wo), np.nan, np.float32))
        want_img = orc.pointwise(want, tw, tb)
        kw.update(torgb_weight=mem.ptr(dev(tw)), torgb_bias=mem.ptr(dev(tb)), img_out=mem.ptr(img_out))
        if with_prev:                                        # the previous image is per ROW (it already differs between the samples)
            prev = pkg.synth.normal((batch, 3, ho // 2, wo // 2), seed, "prev").astype(np.float32)
            want_img = want_img + orc.upsample2d(prev)
            kw.update(img_prev=mem.ptr(dev(prev)))
    lib.sepconv_forward(samples=s, stream=mem.stream, x=mem.ptr(xin), y=mem.ptr(y), skip=mem.ptr(skh), conv1_weight=mem.ptr(w1),
                        conv1_bias=mem.ptr(b1), conv2_weight=mem.ptr(w2), noise_const=mem.ptr(nc), noise_strength=mem.ptr(ns), batch=batch,
                        cin=cin, cout=cout, res_in=h, width_in=w, down=1, up=up, wsplit=mem.ptr(wsp), wsplit_bytes=wsp_n * 4,
                        dtype=pkg.hipbind.dtype_code(storage), gemm=gemm, **kw)
    mem.sync()
    name = lib.last_kernel()
    if symbol is not None:
        assert name.startswith(symbol), name
    assert "_rows_kernel<" in name, name
    got = nchw(from_storage(mem.get(y), storage))
    assert np.isfinite(got).all(), "kernel left NaNs (unwritten output or read of unwritten LDS)"
    storage_close(got, want, storage, ulps=1, frac=0.05 if gemm16 else 0.02, top_ulps=0.5 if gemm16 else 0.0)      # tests/sepconv_case.py
    if torgb:
        atol = 3e-5 * max(1.0, float(np.abs(want_img).max()))
        if storage != "f32":
            atol += 3.0 * float(storage_ulp(np.abs(want).max(), storage)) * float(np.abs(tw).max())
        np.testing.assert_allclose(mem.get(img_out), want_img, rtol=0, atol=atol)
    return name


def check_host_guards(pkg, lib, mem, res=16, hw=None):
    """every MIGAN_EINVAL of migan_forward_samples_hw: refused with y and the workspace untouched; then a good call, then migan_forward's bits"""
    Err = ValueError                       # what hipbind raises for MIGAN_EINVAL
    hh, ww = hw or (res, res)
    g = SamplesBound(pkg, lib, mem, res, seed=41)
    h = g.h
    f = h.noise_floats_hw(hh, ww)
    n, s = 2, 2
    x = (pkg.synth.normal((n, 4, hh, ww), 41, "xg") * 0.7).astype(np.float32)
    noise = pkg.synth.normal((n, s, f), 41, "ng").astype(np.float32)
    before, _, _ = g.forward_hw(x)
    need = h.workspace_bytes_samples_hw(n, s, hh, ww)
    assert need > h.workspace_bytes_hw(n, hh, ww)
    xd, nd = mem.put(aligned(x)), mem.put(aligned(noise))
    yd = mem.put(aligned(np.full((n * s, 3, hh, ww), np.nan, np.float32)))
    wd = mem.put(np.full(need + 256, FILL, np.uint8).view(np.float32))
    px, pn, py, pw = mem.ptr(xd), mem.ptr(nd), mem.ptr(yd), mem.ptr(wd)
    q = res // 4
    bad = [
        ("samples < 1", dict(samples=0)), ("samples < 1", dict(samples=-3)), ("null noise", dict(noise=None)), ("null x", dict(x=None)),
        ("null y", dict(y=None)), ("empty batch", dict(n=0)), ("bad height", dict(height=hh + 1)), ("bad width", dict(width=q // 2 if q > 1 else 0)),
        ("null workspace", dict(ws=None)), ("workspace one byte short", dict(ws_bytes=need - 1)),
        ("workspace of the plain forward", dict(ws_bytes=h.workspace_bytes_hw(n, hh, ww))),
    ]
    for what, change in bad:
        a = dict(x=px, noise=pn, y=py, n=n, samples=s, height=hh, width=ww, ws=pw, ws_bytes=need)
        a.update(change)
        with pytest.raises(Err):
            h.forward_samples_hw(a["x"] or 0, a["noise"] or 0, a["y"] or 0, a["n"], a["samples"], a["height"], a["width"], a["ws"] or 0,
                                 a["ws_bytes"], mem.stream)
        mem.sync()
        assert np.isnan(np.array(mem.get(yd))).all(), f"{what}: the refused call wrote y"
        assert (np.array(mem.get(wd)).view(np.uint8) == FILL).all(), f"{what}: the refused call wrote the workspace"
    for what, args in [("samples", (2, 0, hh, ww)), ("batch", (0, 2, hh, ww)), ("height", (2, 2, hh + 1, ww))]:
        with pytest.raises(Err):
            h.workspace_bytes_samples_hw(*args)
    with pytest.raises(Err):
        h.noise_floats_hw(hh + 1, ww)
    h.forward_samples_hw(px, pn, py, n, s, hh, ww, pw, need, mem.stream)
    mem.sync()
    assert np.isfinite(np.array(mem.get(yd))).all()
    after, _, _ = g.forward_hw(x)
    np.testing.assert_array_equal(after, before)

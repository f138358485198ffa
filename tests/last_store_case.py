"""The last SeparableConv2d of a generator keeps its feature map in registers for the fused ToRGB tail and does not write it: what
tests/test_emu_last_store.py (CPU emulator) and tests/test_gpu_last_store.py (MI355X) check, through the C ABI.  Test infrastructure only.

How the missing store is seen.  The caller owns the workspace, so the test fills it with a byte pattern before the forward and looks for
the longest run of pattern bytes afterwards.  One stream, so the sub-batch is the whole batch of n images.  At H x W, Generator(512):
  * act0's largest tenant is the last feature map, n * H*W*64*4 bytes; the next largest (the 128-channel map at half resolution) is half of
    that, so without the last store the upper half of act0 is never written: a run of at least n * H*W*64*4 / 2 bytes (the threshold);
  * with the store (the parent, or a debug plan) every byte of act0 is written and the longest run is the unused part of dwfir_tmp.
Measured on the CPU emulator at 128 x 128, per image, pipe_min_tiles = 1: threshold 2 097 152 bytes; longest run with the store (the parent
commit) 786 432 bytes, 3/8 of the threshold (the part of dwfir_tmp that the fused down=2 kernels leave unused); without it 2 097 152 bytes.
On the MI355X at batch 5: 10 485 760 bytes at 128 x 128 and 20 971 520 at 128 x 256, the threshold exactly in both."""
import numpy as np

from oracle import migan_torch_cpu as torc
from tests.emu_util import aligned
from tests.knobs import knobs

PIPE = "migan::sepconv_pipe_kernel<"
FILL = 0xA5
TOL = 1e-4                 # tests/test_gpu_round2.py: forward_any_size against the oracle, fp32 storage
TAP_TOL = 3e-5             # tests/test_emu_generator.py: a layer tap against the oracle, times max(1, |tap|max)


def longest_run(raw, value=FILL):
    """length of the longest run of `value` in the uint8 array `raw`"""
    hit = np.flatnonzero(raw != value)
    if hit.size == 0:
        return int(raw.size)
    edges = np.concatenate(([-1], hit, [raw.size]))
    return int(np.diff(edges).max()) - 1


class Bound:
    """Generator(res) behind the C ABI with synthetic weights: one handle, one stream, workspaces owned by the caller"""

    def __init__(self, pkg, lib, mem, res, seed, dtype=0):
        self.pkg, self.lib, self.mem, self.res = pkg, lib, mem, res
        self.h = pkg.hipbind.MiganHandle(lib, res, dtype=dtype)
        self.h.set_streams(1)
        self.sd = pkg.synth.make_state_dict(res, seed=seed)
        self.keep = {k: mem.put(aligned(v.reshape(1) if v.ndim == 0 else v)) for k, v in self.sd.items()}
        for name, shape, _ in self.h.weights():
            self.h.set_weight(name, mem.ptr(self.keep[name]), shape)
        self.h.commit(mem.stream)

    def forward_hw(self, x):
        """-> (y, workspace bytes after the forward, symbol of the last SeparableConv2d launch)"""
        n, _, hh, ww = x.shape
        need = self.h.workspace_bytes_hw(n, hh, ww)
        xd = self.mem.put(aligned(x))
        yd = self.mem.put(aligned(np.full((n, 3, hh, ww), np.nan, np.float32)))
        wd = self.mem.put(np.full(need + 256, FILL, np.uint8).view(np.float32))        # (float32 view: 4-byte elements, aligned)
        self.h.forward_hw(self.mem.ptr(xd), self.mem.ptr(yd), n, hh, ww, self.mem.ptr(wd), need, self.mem.stream)
        self.mem.sync()
        return np.array(self.mem.get(yd)), np.array(self.mem.get(wd)).view(np.uint8)[:need], self.lib.last_kernel()


def check_hw_case(pkg, lib, mem, hw, batch, grid, symbol, seed=23, res=512):
    """Generator(res) at H x W: the last layer runs `symbol` (a pipelined ToRGB form), equals the oracle, equals the storing debug plan bit
    for bit, leaves the upper half of act0 untouched, and the debug plan still holds the last feature map."""
    hh, ww = hw
    cl = 32768 // res
    x = (pkg.synth.normal((batch, 4, hh, ww), seed, "xhw") * 0.7).astype(np.float32)
    last = f"synthesis.b{res}.conv2"
    tune = dict(pipe_min_tiles=1)
    if grid:
        tune["pipe_grid"] = grid
    with knobs(lib, **tune):
        g = Bound(pkg, lib, mem, res, seed)
        taps = {}
        want = torc.generator(x, g.sd, res, taps=taps).numpy()
        tap = taps[last].numpy()
        y, raw, name = g.forward_hw(x)
        assert name.startswith(symbol), name
        err = float(np.abs(y - want).max())
        run = longest_run(raw)
        threshold = batch * hh * ww * cl * 4 // 2
        print(f"last store {hh}x{ww} batch {batch}: {name} max_abs_err {err:.3e} longest untouched run {run} threshold {threshold}")
        assert err <= TOL
        assert run >= threshold, (run, threshold)
        # the same handle with every layer kept: the last launch stores, the image is the same bits, the map equals the oracle's tap
        g.h.set_debug(True)
        yd, rawd, named = g.forward_hw(x)
        assert named == name, (named, name)
        np.testing.assert_array_equal(yd, y)
        # (migan_debug_tensor_hw: the plan at H x W.  By layout the map is the last buffer of the workspace -- a debug plan gives every
        # layer a buffer of its own in launch order -- and the two must agree.)
        nbytes = batch * hh * ww * cl * 4
        off, shape = g.h.debug_tensor_hw(batch, hh, ww, last)
        assert shape == (batch, hh, ww, cl) and off == rawd.size - (nbytes + 255) // 256 * 256, (off, shape, rawd.size)
        got = rawd[off:off + nbytes].view(np.float32).reshape(batch, hh, ww, cl)
        np.testing.assert_allclose(np.transpose(got, (0, 3, 1, 2)), tap, rtol=0, atol=TAP_TOL * max(1.0, float(np.abs(tap).max())), err_msg=last)
        g.h.set_debug(False)
    return y

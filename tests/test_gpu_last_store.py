"""The dead store of the last layer's feature map (tests/last_store_case.py) on a real MI355X."""
import numpy as np
import pytest
import torch

from oracle import migan_torch_cpu as torc
from tests.emu_util import aligned
from tests.last_store_case import FILL, PIPE, TAP_TOL, TOL, Bound, check_hw_case, longest_run
from tests.sepconv_case import CudaMem

pytestmark = pytest.mark.gpu
TORGB_64 = PIPE + "0, 64, 64, false, true"


def longest_untouched(ws, block=256):
    """bytes of the longest run of whole `block`-byte blocks of the device tensor `ws` that still hold the fill pattern: a lower bound of the
    longest run of pattern bytes, and equal to it where the run starts and ends on workspace buffers (they are 256-byte aligned)"""
    whole = ws[:ws.numel() // block * block].view(-1, block).eq(FILL).all(dim=1)
    return longest_run(whole.cpu().numpy().view(np.uint8), 1) * block


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


# Generator(512) at 128 x 128: 128 tiles per image in the last layer.  Batch 5 on the default 256 persistent workgroups: 640 tiles, so 128
# workgroups walk 3 tiles and 128 walk 2 (peeled first tile, steady-state loop, last tile, uneven share).  128 x 256: a non-square tile grid.
@pytest.mark.parametrize("hw,batch", [((128, 128), 5), ((128, 256), 5)])
def test_last_feature_map_is_not_written(pkg, lib, dev, hw, batch):
    check_hw_case(pkg, lib, CudaMem(dev), hw, batch, 0, TORGB_64)


def test_fixed_size_plan_reports_the_symbol_and_the_debug_plan_keeps_the_map(pkg, lib, dev):
    """Generator(512) at its own size, default tuning: migan_launch_info names the pipelined ToRGB symbol for the last launch, the forward
    leaves the upper half of the last map's slot untouched (threshold n * 512*512*64*4 / 2 = 67 108 864 bytes at n = 2; a forward that
    stores leaves 3/8 of that, as at the smaller sizes of tests/last_store_case.py) while the debug plan does not, the two images are the
    same bits, and the debug plan's synthesis.b512.conv2 read through migan_debug_tensor equals the oracle's tap."""
    mem = CudaMem(dev)
    g = Bound(pkg, lib, mem, 512, seed=29)
    n = 2
    x = pkg.synth.make_input(n, 512, seed=29)
    taps = {}
    want = torc.generator(x, g.sd, 512, taps=taps)
    xd = mem.put(aligned(x))
    out = []
    for debug in (False, True):
        g.h.set_debug(debug)
        need = g.h.workspace_bytes(n)
        yd = torch.full((n, 3, 512, 512), float("nan"), device=dev)
        ws = torch.full((need,), FILL, dtype=torch.uint8, device=dev)
        g.h.forward(mem.ptr(xd), yd.data_ptr(), n, ws.data_ptr(), need, mem.stream)
        mem.sync()
        last = g.h.launches()[-1]
        assert last["layer"] == "synthesis.b512.conv2" and last["kernel"].startswith(TORGB_64), last
        out.append((yd.cpu(), ws))
    (y, ws), (ydbg, wsd) = out
    threshold = n * 512 * 512 * 64 * 4 // 2
    run, rund = longest_untouched(ws), longest_untouched(wsd)
    print(f"last store 512x512 batch {n}: longest untouched run {run}, debug plan {rund}, threshold {threshold}")
    assert run >= threshold, (run, threshold)
    assert rund < threshold, (rund, threshold)
    assert torch.equal(y, ydbg)
    assert float((y - want).abs().max()) <= TOL
    off, shape = g.h.debug_tensor(n, "synthesis.b512.conv2")
    assert shape == (n, 512, 512, 64)
    t = wsd[off:off + 4 * int(np.prod(shape))].view(torch.float32).reshape(shape).permute(0, 3, 1, 2).cpu()
    tap = taps["synthesis.b512.conv2"]
    assert float((t - tap).abs().max()) <= TAP_TOL * max(1.0, float(tap.abs().max()))
    g.h.set_debug(False)


@pytest.mark.parametrize("batch", [5])
def test_uint8_forward_composes_the_same_image(pkg, lib, dev, batch):
    """forward_uint8 (the same last launch, composing bytes in its tail; the uint8 path exists at the network's own size only) equals
    compose(forward) bit for bit, and does not write the last feature map either: the module's workspace, filled with the pattern before
    the call, keeps a run of batch * 512*512*64*4 / 2 bytes (a batch below 16 runs as one sub-batch)"""
    res, seed = 512, 31
    sd = pkg.synth.make_state_dict(res, seed=seed)
    m = pkg.Generator(resolution=res)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(rng.integers(0, 256, size=(batch, res, res, 3), dtype=np.uint8)).to(dev)
    mask = torch.from_numpy(np.where(rng.random((batch, res, res)) < 0.4, 0, 255).astype(np.uint8)).to(dev)
    with torch.no_grad():
        y = m(pkg.pipeline.preprocess(img, mask))
        want = pkg.pipeline.compose(y, img, mask)
        m._ws.fill_(FILL)
        got = m.forward_uint8(img, mask)
    torch.cuda.synchronize()
    need = m._handle.workspace_bytes(batch)
    assert m._handle.forward_split(batch) == [batch] and m._ws.numel() >= need
    run, threshold = longest_untouched(m._ws[:need]), batch * res * res * 64 * 4 // 2
    print(f"last store uint8 {res}x{res} batch {batch}: longest untouched run {run} threshold {threshold}")
    assert run >= threshold, (run, threshold)
    assert m._handle.launches()[-1]["kernel"].startswith(TORGB_64), m._handle.launches()[-1]
    assert torch.equal(got, want)

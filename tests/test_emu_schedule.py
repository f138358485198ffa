"""The tile schedule every MI-GAN kernel shares (mi-gan_amd/csrc/migan_kernels.hpp: MIGAN_XCD_RANGE, MIGAN_XCD_TILES, xcd_remap;
migan_pipe.hpp: MIGAN_TILE_WALK), run on the host through an export of the emulator library: which workgroup owns which tile, and in which
order it walks them.

The schedule gives every XCD (workgroup number mod 8) one range of tiles, walked by the workgroups of that XCD only.  Its precondition,
stated on the macro, is nblk >= 8 or nblk >= ntiles: a smaller grid has no workgroup on some XCDs.  The host launches no such grid
(one workgroup per tile, or min(ntiles, knob) with the knob a multiple of 8: test_host_never_launches_a_grid_outside_the_precondition).
Every case runs the same checks; what differs is the set of tiles that must have been walked once: all of them inside the
precondition, and outside it exactly the ranges of the XCDs that have a workgroup (grid 1: 2 of 12, 6 of 48, 256 of 2048 tiles; grid 7:
11 of 12, 42 of 48, 1792 of 2048) -- the other ranges are walked by nobody, which is why the precondition is one."""
import ctypes

import numpy as np
import pytest

from tests.emu.build_emu import build
from tests.emu_util import emu_lib
from tests.knobs import knobs

# (tiles_x, tiles_y, nchunks, B): one tile; a carry through every digit of the cursor; a remainder in the XCD split; a production-size grid
EXTENTS = [(1, 1, 1, 1), (3, 2, 2, 1), (4, 4, 1, 3), (32, 32, 1, 2)]
# fewer workgroups than XCDs, one per XCD, a remainder, one CU's worth around 256; None = one workgroup per tile
GRIDS = [1, 7, 8, 9, 255, 256, 257, None]


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(build())
    lib.hipemu_tile_walk.restype = ctypes.c_int
    lib.hipemu_tile_walk.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [ctypes.c_int]
    lib.hipemu_xcd_remap.restype = ctypes.c_int
    lib.hipemu_xcd_remap.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


def decode(t, tiles_x, tiles_y, nchunks):
    """logical tile numbers -> rows (n, x, y, b): column chunk fastest, then x, y, image"""
    t = np.asarray(t)
    return np.stack([t % nchunks, t // nchunks % tiles_x, t // (nchunks * tiles_x) % tiles_y, t // (nchunks * tiles_x * tiles_y)], axis=-1)


def xcd_ranges(ntiles):
    """[(first tile, tile count)] of the 8 XCDs, written out independently of the code under test"""
    q, r = divmod(ntiles, 8)
    counts = [q + (x < r) for x in range(8)]
    return [(sum(counts[:x]), counts[x]) for x in range(8)]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("extents", EXTENTS)
def test_every_tile_once_in_the_decoded_order(emu, extents, grid):
    tiles_x, tiles_y, nchunks, batch = extents
    ntiles = tiles_x * tiles_y * nchunks * batch
    nblk = ntiles if grid is None else grid
    ranges = xcd_ranges(ntiles)
    on_xcd = [len(range(x, nblk, 8)) for x in range(8)]           # workgroups per XCD
    rng = np.zeros(4, dtype=np.int32)
    cur = np.empty((ntiles + 1, 4), dtype=np.int32)
    walked = np.zeros(ntiles, dtype=np.int64)                     # how often each logical tile was walked
    idle = 0
    for bid in range(nblk):
        cur[...] = -1
        T = emu.hipemu_tile_walk(tiles_x, tiles_y, nchunks, batch, bid, nblk, rng.ctypes.data, cur.ctypes.data, ntiles + 1)
        tbase, tcnt, tstep, tl0 = (int(v) for v in rng)
        assert (tbase, tcnt) == ranges[bid % 8] and tstep == on_xcd[bid % 8] >= 1 and tl0 == bid // 8, (bid, tbase, tcnt, tstep, tl0)
        mine = tbase + np.arange(tl0, tcnt, tstep)
        assert T == len(mine), (bid, T, tbase, tcnt, tstep, tl0)
        assert (cur[T:] == -1).all(), f"workgroup {bid} walked past its {T} tiles"          # T == 0: walks nothing
        if T == 0:
            idle += 1
            continue
        assert (cur[:T] == decode(mine, tiles_x, tiles_y, nchunks)).all(), (bid, cur[:T])      # k-th cursor = decode(tbase + tl0 + k tstep)
        walked[mine] += 1
        if nblk == ntiles:
            assert T == 1 and mine[0] == emu.hipemu_xcd_remap(bid, nblk), (bid, tbase, tl0)     # one tile each: xcd_remap's order
    assert idle == sum(max(0, on_xcd[x] - ranges[x][1]) for x in range(8))        # workgroups beyond their XCD's tiles leave at once
    expect = np.ones(ntiles, dtype=np.int64)
    if nblk < 8 and nblk < ntiles:
        # outside the precondition: the ranges of the XCDs without a workgroup are walked by nobody (figures in the docstring)
        for first, count in ranges[nblk:]:
            expect[first:first + count] = 0
        assert expect.sum() < ntiles
    assert (walked == expect).all(), f"walked {int(walked.sum())} tiles, {int((walked > 1).sum())} more than once, expected {int(expect.sum())} once each"


def test_xcd_remap_is_a_bijection(emu):
    for nblk in (1, 7, 8, 9, 63, 64, 65, 257):
        assert sorted(emu.hipemu_xcd_remap(b, nblk) for b in range(nblk)) == list(range(nblk))


def test_host_never_launches_a_grid_outside_the_precondition():
    """the persistent-grid knobs are rounded to a multiple of 8, at least 8, whatever is asked for; every other launch is one workgroup per tile"""
    lib = emu_lib()
    for key in ("pipe_grid", "persist_grid"):
        for asked in (0, 1, 7, 9, 255):
            with knobs(lib, **{key: asked}):
                got = lib.get_tuning(key)
                assert got >= 8 and got % 8 == 0, (key, asked, got)

"""The split of a call's items into launches (mi-gan_amd/csrc/migan_host.hpp: table_split), the host half of every kernel that takes a
table of items by value, run on the host through hipemu_table_split of the emulator library.  The rule: a launch takes the next item
while it holds fewer than max_items and the item's workgroups still fit under max_groups; an item that alone exceeds max_groups is
refused.  Every expected list below is written out by hand from that rule."""
import ctypes

import numpy as np
import pytest

from tests.emu.build_emu import build


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(build())
    lib.hipemu_table_split.restype = ctypes.c_int
    lib.hipemu_table_split.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_int]
    lib.migan_last_error.restype = ctypes.c_char_p
    return lib


def split(emu, tiles, max_items, max_groups=0):
    """-> [(i0, k, total)], or the refusal's text.  max_groups = 0: the split's default, 2^31 - 1"""
    t = np.asarray(tiles, dtype=np.uint64)
    out = np.full((len(tiles) + 1, 3), 0xEEEE, dtype=np.uint64)
    n = emu.hipemu_table_split(t.ctypes.data, len(tiles), max_items, max_groups, out.ctypes.data, len(out))
    if n < 0:
        return emu.migan_last_error().decode()
    assert 0 <= n <= len(tiles) and (out[n:] == 0xEEEE).all()
    return [tuple(int(v) for v in row) for row in out[:n]]


def test_the_workgroup_cap_ends_a_launch(emu):
    """4 + 4 fit, the third 4 does not; the item without workgroups rides along; 9 would pass the cap; an item that alone equals the
    cap is a launch of its own, and the 1 behind it another"""
    assert split(emu, [4, 4, 4, 0, 9, 10, 1], 8, 10) == [(0, 2, 8), (2, 2, 4), (4, 1, 9), (5, 1, 10), (6, 1, 1)]


def test_an_item_above_the_cap_is_refused_with_its_index(emu):
    msg = split(emu, [1, 11, 1], 8, 10)
    assert isinstance(msg, str) and "item 1" in msg and "too large" in msg
    msg = split(emu, [3, 0, 1 << 31], 8)
    assert isinstance(msg, str) and "item 2" in msg


def test_the_table_fills_before_the_cap_is_reached(emu):
    """three items fill the table at 3 workgroups; then 6 + 6 pass the cap with one item in the launch; 6 + 1 fit"""
    assert split(emu, [1, 1, 1, 6, 6, 1], 3, 10) == [(0, 3, 3), (3, 1, 6), (4, 2, 7)]
    assert split(emu, [1, 1, 1, 9, 1, 1], 2, 10) == [(0, 2, 2), (2, 2, 10), (4, 2, 2)]        # (1 + 9 is exactly the cap)


def test_the_cap_is_reached_before_the_table_fills(emu):
    """4 + 4 + 4 pass the cap with two of three slots used; the next launch fills its three slots at 6 workgroups"""
    assert split(emu, [4, 4, 4, 1, 1, 1, 1], 3, 10) == [(0, 2, 8), (2, 3, 6), (5, 2, 2)]


def test_the_default_cap_is_a_one_dimensional_grid(emu):
    assert split(emu, [1] * 33, 32) == [(0, 32, 32), (32, 1, 1)]
    top = (1 << 31) - 1
    assert split(emu, [top, 1, top - 1, 1, 1], 32) == [(0, 1, top), (1, 2, top), (3, 2, 2)]
    assert split(emu, [0, 0, 0], 2) == [(0, 2, 0), (2, 1, 0)]                                  # launches without workgroups: nothing to launch
    assert split(emu, [], 4) == []

"""The dead store of the last layer's feature map (tests/last_store_case.py) on the CPU emulator of the product's kernel source."""
import pytest

from tests.emu_util import emu_lib
from tests.last_store_case import PIPE, check_hw_case
from tests.sepconv_case import HostMem


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


# Generator(512) at 128 x 128 (its smallest input) has 128 tiles per image in its last layer; 48 persistent workgroups walk them 3, 3, 3 ...
# 2, 2 -- the mix of batch 5 on the GPU's 256: the peeled first tile, the steady-state loop, the last tile and an uneven share.  128 x 256: a
# non-square tile grid, 6 or 5 tiles each.  One image: the emulator takes 9 s and 13 s for the two cases, twice that at batch 2; the kernel
# forms of batch >= 2 in the other layers are what tests/test_gpu_last_store.py runs.
@pytest.mark.parametrize("hw", [(128, 128), (128, 256)])
def test_last_feature_map_is_not_written(pkg, lib, hw):
    check_hw_case(pkg, lib, HostMem(), hw, 1, 48, PIPE + "0, 64, 64, false, true")

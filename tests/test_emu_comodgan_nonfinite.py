"""CPU execution (fiber SIMT emulator, tests/emu) of the Co-Mod-GAN NaN policy of the default build (tests/comodgan_nonfinite_case.py).
The emulator has the default policy only; the nan_policy="clamp" build is tested on the GPU (tests/test_gpu_comodgan_nonfinite.py)."""
from tests.comodgan_layers_case import HostMem
from tests.comodgan_nonfinite_case import check_default
from tests.emu_util import emu_lib


def test_nan_mask_of_the_default_library_is_the_float32_oracles():
    check_default(emu_lib(), HostMem())

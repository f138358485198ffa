"""CPU execution (fiber SIMT emulator, tests/emu) of the Co-Mod-GAN layer-isolating check (tests/comodgan_layers_case.py): every
layer's launch against the float64 oracle on the device's own input tap, in every kernel form the cases reach.  No GPU involved.
Run with -s for the per-unit table; measured figures: profiles/comodgan_layers.md."""
import pytest

from tests.comodgan_layers_case import CASES, HostMem, run_case
from tests.emu_util import emu_lib


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_layer_in_isolation(name, monkeypatch):
    run_case(name, emu_lib(), HostMem(), monkeypatch)

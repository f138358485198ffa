"""Every Co-Mod-GAN layer's launch on a real MI355X against the float64 oracle on the device's own input tap
(tests/comodgan_layers_case.py; the same cases run through the emulator in tests/test_emu_comodgan_layers.py).
Run with -s for the per-unit table; measured figures: profiles/comodgan_layers.md."""
import pytest
import torch

from tests.comodgan_layers_case import CASES, GPU_CASES, TorchMem, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", sorted(CASES) + sorted(GPU_CASES))
def test_every_layer_in_isolation(pkg, dev, name, monkeypatch):
    lib = pkg.hipbind.load_library()
    assert lib.backend() == "hip:gfx950"
    run_case(name, lib, TorchMem(dev), monkeypatch)

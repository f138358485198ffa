"""The Co-Mod-GAN NaN policy of both builds on a real MI355X (tests/comodgan_nonfinite_case.py): the default library leaves NaNs
where the float32 oracle has them; load_library(nan_policy="clamp") stays finite, and agrees with the default bit for bit on a
finite input and on one with infinite and huge pixels."""
import numpy as np
import pytest
import torch

from tests.comodgan_layers_case import TorchMem
from tests.comodgan_nonfinite_case import check_default, forwards, huge_input, inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def test_nan_mask_of_the_default_library_and_a_finite_clamp_build(pkg, dev):
    default = pkg.hipbind.load_library()
    assert default.backend() == "hip:gfx950"
    y_default, mask = check_default(default, TorchMem(dev))
    clamp = pkg.hipbind.load_library(nan_policy="clamp")
    assert clamp.backend() == "hip:gfx950" and clamp.nan_policy() == "clamp"
    cfg, sd, x, bad, z = inputs()
    huge = huge_input(x)
    y_bad, y, y_huge = forwards(clamp, TorchMem(dev), cfg, sd, [bad, x, huge], z)
    assert mask.any() and np.isfinite(y_bad).all()                  # where the default build has NaNs, this one has numbers
    assert y.tobytes() == y_default.tobytes()                       # finite input: the two builds give the same bytes
    # +-inf and 3e38 pixels are +-256 behind FromRGB's clamp in either build (every layer of the default build on this kind of input:
    # the per-layer case r16_huge): finite, and the same bytes
    y_huge_default, = forwards(default, TorchMem(dev), cfg, sd, [huge], z)
    assert np.isfinite(y_huge).all() and np.abs(y_huge - y).max() > 0 and y_huge.tobytes() == y_huge_default.tobytes()

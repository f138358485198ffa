"""The operator table of tests/sepconv_matrix.py on the MI355X: every kernel family behind migan_sepconv_forward, crossed with skip x noise
x ToRGB x FromRGB and the storage formats, against the numpy oracle (float64 for fp32 storage); the refusals of missing companion
pointers; and a coverage check -- every kernel the default generators launch in a forward is reported by some case of the table."""
import numpy as np
import pytest
import torch

from tests import sepconv_matrix as mx
from tests.sepconv_case import CudaMem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def mem():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return CudaMem(torch.device("cuda", 0))


CASES = mx.cases()


@pytest.mark.parametrize("row,flags,storage", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_sepconv_matrix(lib, pkg, mem, row, flags, storage):
    mx.run_matrix_case(lib, pkg, mem, row, flags, storage)


@pytest.mark.parametrize("row", mx.COMPANION_ROWS)
@pytest.mark.parametrize("name,flags,drop,fragment", mx.COMPANIONS, ids=[c[0] for c in mx.COMPANIONS])
def test_missing_companion_pointer_is_refused(lib, pkg, mem, row, name, flags, drop, fragment):
    mx.run_companion_case(lib, pkg, mem, row, flags, drop, fragment)


@pytest.fixture(scope="module")
def table_names(lib, pkg, mem):
    return mx.table_kernels(lib, pkg, mem)


@pytest.mark.parametrize("res,storage,batch", [(256, "f32", 1), (256, "f32", 32), (256, "bf16", 32), (512, "f32", 1), (512, "f32", 32),
                                               (512, "bf16", 32), (1024, "f32", 1), (2048, "f32", 1)])
def test_table_covers_the_generator_forwards(pkg, mem, table_names, res, storage, batch):
    """one forward of the default Generator(res): the kernel each launch ran (migan_launch_info after a forward names what the forward's
    last sub-batch launched: the pipelined / pipedown forms depend on the batch) must be reported by some case of the table"""
    dev = torch.device("cuda", 0)
    sd = pkg.synth.make_state_dict(res, seed=5)
    m = pkg.Generator(resolution=res, activation_dtype=storage)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to(dev).eval()
    x = torch.from_numpy(pkg.synth.make_input(batch, res, seed=5)).to(dev)
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    plan = {l["kernel"] for l in m.launch_info()}
    assert not mx.uncovered(plan, table_names), mx.uncovered(plan, table_names)

"""The operator table of tests/sepconv_matrix.py on the CPU fiber emulator: every kernel family behind migan_sepconv_forward, crossed with
skip x noise x ToRGB x FromRGB and the storage formats, against the numpy oracle (float64 for fp32 storage); the refusals of missing
companion pointers; and a coverage check -- every kernel the Generator(1024 / 2048 / 4096) plans name is reported by some case of the table."""
import importlib

import pytest

from tests import sepconv_matrix as mx
from tests.emu_util import emu_lib
from tests.sepconv_case import HostMem


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("mi-gan_amd")


CASES = mx.cases()


@pytest.mark.parametrize("row,flags,storage", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_sepconv_matrix(lib, pkg, row, flags, storage):
    mx.run_matrix_case(lib, pkg, HostMem(), row, flags, storage)


@pytest.mark.parametrize("row", mx.COMPANION_ROWS)
@pytest.mark.parametrize("name,flags,drop,fragment", mx.COMPANIONS, ids=[c[0] for c in mx.COMPANIONS])
def test_missing_companion_pointer_is_refused(lib, pkg, row, name, flags, drop, fragment):
    mx.run_companion_case(lib, pkg, HostMem(), row, flags, drop, fragment)


def test_narrow_fir_up_takes_its_registered_dynamic_lds(lib, pkg):
    """the narrow FIR-up layer with 64 output channels takes 81 KiB of dynamic LDS: prepare_kernels() registers it (above the 64 KiB
    default), so the launch goes through -- and its output matches the oracle"""
    mx.run_matrix_case(lib, pkg, HostMem(), "narrow_up", mx.FLAGS[0], "f32")
    assert lib.last_kernel() == "migan::narrow_sepconv_kernel<2, false>"


@pytest.fixture(scope="module")
def table_names(lib, pkg):
    return mx.table_kernels(lib, pkg, HostMem())


@pytest.mark.parametrize("res", [1024, 2048, 4096])
def test_table_covers_the_generator_plans(lib, pkg, table_names, res):
    """the kernels a default Generator(res) plan names before any forward: the table kernels of its own tile geometry.  (The pipelined /
    pipedown / small-tile forms depend on the batch, Plan::resolve picks them per forward: tests/test_emu_launch_stream.py lists what
    production forwards launch, the GPU test runs forwards.)  Each must be reported by a case of the table"""
    h = pkg.hipbind.MiganHandle(lib, res, 0)
    plan = {l["kernel"] for l in h.launches()}
    assert not mx.uncovered(plan, table_names), mx.uncovered(plan, table_names)

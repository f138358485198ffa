"""Dry runs of the emulator library: what a forward launches -- kernel symbol, grid, block, LDS bytes, argument bytes -- at sizes the
emulator could never execute (tests/emu/hip_emu.h: rt::launch logs instead of running, nothing is dereferenced).  Which kernel runs where
is a pure host decision (migan_host.hpp: resolve_layer), so it is checked here, without a GPU.  Test infrastructure only."""
import contextlib
import ctypes as C
import importlib

import numpy as np

FAKE = 1 << 40          # any non-null address will do for tensors and workspaces: a dry run never reads them


def load(path):
    pkg = importlib.import_module("mi-gan_amd")
    return pkg.hipbind.MiganLib(path, allow_test_backend=True)


@contextlib.contextmanager
def dry_run(lib):
    lib.lib.hipemu_set_dry_run.restype = None
    lib.lib.hipemu_set_dry_run(1)
    try:
        yield
    finally:
        lib.lib.hipemu_set_dry_run(0)


def take_log(lib, with_args=False):
    """the launches logged since the last call: [symbol, grid, block, lds_bytes(, argument bytes)]"""
    L = lib.lib
    out = []
    name, args = C.c_char_p(), C.c_void_p()
    grid, block = C.c_uint(), C.c_uint()
    lds, nbytes = C.c_size_t(), C.c_size_t()
    for i in range(L.hipemu_log_size()):
        assert L.hipemu_log_entry(i, C.byref(name), C.byref(grid), C.byref(block), C.byref(lds), C.byref(args), C.byref(nbytes)) == 0
        row = [name.value.decode(), grid.value, block.value, lds.value]
        if with_args:
            row.append(C.string_at(args.value, nbytes.value))
        out.append(row)
    L.hipemu_set_dry_run(1)      # (empties the log)
    return out


class Weights:
    """state_dict stand-in for a handle: real memory only where migan_commit reads it (the FIR taps and zero-insertion masks), a distinct fake
    address for everything else"""

    def __init__(self):
        self.keep, self.fake = {}, {}
        self.next = FAKE + (1 << 36)

    def bind(self, handle):
        taps = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0]).astype(np.float32) / 64.0
        for name, shape, _ in handle.weights():
            if name.endswith("filter.weight"):
                key = (name.split(".")[-3], shape)
                if key not in self.keep:
                    self.keep[key] = np.ascontiguousarray(np.broadcast_to(taps * (4.0 if key[0] == "upsample" else 1.0), shape))
                ptr = self.keep[key].ctypes.data
            elif name.endswith("filter_const"):
                if shape not in self.keep:
                    m = np.zeros(shape, np.float32)
                    m[..., ::2, ::2] = 1.0
                    self.keep[shape] = m
                ptr = self.keep[shape].ctypes.data
            else:                    # (the same address whenever the same tensor is bound again: argument bytes stay comparable)
                if (name, shape) not in self.fake:
                    self.fake[name, shape] = self.next
                    self.next += (4 * int(np.prod(shape, dtype=np.int64)) + 4095) // 4096 * 4096
                ptr = self.fake[name, shape]
            handle.set_weight(name, ptr, shape)
        handle.commit()
        return handle


def generator(lib, weights, res, storage="f32", gemm=None, streams=2, debug=False):
    pkg = importlib.import_module("mi-gan_amd")
    h = pkg.hipbind.MiganHandle(lib, res, dtype=storage)
    if gemm is not None:
        h.set_gemm(gemm)
    h.set_streams(streams)
    if debug:
        h.set_debug(True)
    return weights.bind(h)


def step(lib, h, kind, batch, with_args=False, hw=None):
    """one forward of `kind` on fake tensors: what it launched and what the handle reports around it.  Raises what the library raises."""
    x, y, ws = FAKE, FAKE + (1 << 32), FAKE + (1 << 37)
    before = h.launches()
    if kind == "hw":
        nbytes = h.workspace_bytes_hw(batch, *hw)
        h.forward_hw(x, y, batch, hw[0], hw[1], ws, nbytes)
    else:
        nbytes = h.workspace_bytes(batch)
        if kind == "forward":
            h.forward(x, y, batch, ws, nbytes)
        elif kind == "timed":
            h.forward_timed(x, y, batch, ws, nbytes)
        elif kind == "u8":
            h.forward_u8(x, x + (1 << 30), y, batch, ws, nbytes)
        elif kind == "parts":
            h.forward_parts(x, [y + (k << 28) for k in range(4)], batch, ws, nbytes, 0, [0x10, 0x20, 0x30])
        else:
            raise ValueError(kind)
    return dict(before=before, launches=take_log(lib, with_args), after=h.launches(), workspace_bytes=nbytes, last_kernel=lib.last_kernel())

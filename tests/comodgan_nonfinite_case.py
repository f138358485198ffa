"""Shared by tests/test_emu_comodgan_nonfinite.py and tests/test_gpu_comodgan_nonfinite.py: what a Co-Mod-GAN forward does with a NaN
in its input, against what oracle/comodgan_oracle.py (float32, the reference's arithmetic) does with the same input.  The oracle
decides the mask: nothing here states where the NaNs go.  Huge and infinite pixels are finite behind FromRGB's clamp, so they are a
case of the per-layer check (tests/comodgan_layers_case.py, "r16_huge").  Test infrastructure only."""
import numpy as np

from oracle import comodgan_oracle as orc
from tests.comodgan_layers_case import HUGE_PIXELS, R16, config, hb, pkg

N, SEED = 3, 161
NAN_AT = (1, 2, 6, 9)             # image, plane, row, column


def inputs():
    cfg = config(*R16)
    sd = pkg.synth.make_comodgan_state_dict(cfg, SEED)
    x, z = pkg.synth.make_input(N, cfg.resolution, SEED), pkg.synth.make_latent(N, cfg.z_dim, SEED)
    bad = x.copy()
    bad[NAN_AT] = np.nan
    return cfg, sd, x, bad, z


def huge_input(x):
    """x with the +inf, -inf and 3e38 pixels of the per-layer case r16_huge"""
    out = x.copy()
    for b, ch, iy, ix, v in HUGE_PIXELS:
        out[b, ch, iy, ix] = v
    return out


def forwards(lib, mem, cfg, sd, xs, z):
    """one handle, one forward per input -> [y [N,3,R,R] float32]"""
    R = cfg.resolution
    h = hb.CoModGANHandle(lib, R, cfg.num_ws, cfg.ch_base, cfg.ch_max, cfg.z_dim, cfg.w_dim, cfg.w0_dim, cfg.map_layers)
    keep = {k: mem.put(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    for name, shape, _ in h.weights():
        h.set_weight(name, mem.ptr(keep[name]), shape)
    h.commit(mem.stream)
    zd = mem.put(np.asarray(z, dtype=np.float32))
    out = []
    for x in xs:
        n = x.shape[0]
        xd = mem.put(np.asarray(x, dtype=np.float32))
        nbytes = h.workspace_bytes(n)
        ws, y = mem.zeros(nbytes), mem.zeros(n * 3 * R * R * 4)
        h.forward(mem.ptr(xd), mem.ptr(zd), mem.ptr(y), n, mem.ptr(ws), nbytes, 1.0, "const", None, mem.stream)
        mem.sync()
        out.append(mem.get(y).view(np.float32).reshape(n, 3, R, R).copy())
    h.close()
    return out


def reference(cfg, sd, x, z):
    return orc.generator(x, z, sd, cfg.resolution, cfg.num_ws)


def check_default(lib, mem):
    """the default library: NaN exactly where the float32 oracle has one, and the oracle's values everywhere on the finite input"""
    assert lib.nan_policy() == "propagate"
    cfg, sd, x, bad, z = inputs()
    want_bad, want = reference(cfg, sd, bad, z), reference(cfg, sd, x, z)
    assert np.isnan(want_bad).any() and np.isfinite(want).all()         # the test is about something
    y_bad, y = forwards(lib, mem, cfg, sd, [bad, x], z)
    assert np.array_equal(np.isnan(y_bad), np.isnan(want_bad)), (int(np.isnan(y_bad).sum()), int(np.isnan(want_bad).sum()))
    # 1e-3: the whole-generator tolerance of every end-to-end Co-Mod-GAN test against this oracle (tests/test_gpu_comodgan_fp16.py,
    # tests/test_emu_comodgan.py), not a figure taken from this run; the issue asks for the mask only
    ok = ~np.isnan(want_bad)
    assert np.isfinite(y_bad[ok]).all() and (not ok.any() or np.abs(y_bad[ok] - want_bad[ok]).max() <= 1e-3)
    assert np.abs(y - want).max() <= 1e-3
    return y, np.isnan(want_bad)

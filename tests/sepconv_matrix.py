"""Every kernel family behind migan_sepconv_forward crossed with every optional input: skip x noise x ToRGB {none, plain, with_prev}
x FromRGB, in each storage format a family takes.  One row per family (the geometry, batch and tuning knobs that select it); the expected
outcome of every case is written out below as a small rule table -- the exact kernel `last_kernel()` reports plus an oracle match, or a
refusal -- not derived from the host code.  Shared by the CPU test (product kernel source on the fiber emulator) and the GPU test.
Test infrastructure only."""
import itertools
import re
from dataclasses import dataclass, field

from tests.knobs import knobs
from tests.sepconv_case import run_sepconv_case

STORAGES = ("f32", "bf16", "f16")
STV = {"f32": 0, "bf16": 1, "f16": 2}
# the emulator cases have a few dozen tiles: let the persistent kernels take them, a few tiles per workgroup (as test_emu_pipe / _wide2 do)
PERSISTENT = dict(pipe_min_tiles=1, pipe_grid=8, w2_min_tiles=1)

# launches of a generator plan that are not a SeparableConv2d layer (nor part of one): nothing in the operator table reports them
NON_SEPCONV = (
    "migan::split_weights_kernel",          # fp16 weight planes, once per handle
    "migan::weight_absmax_kernel",
)
# SeparableConv2d forms the generator picks per launch size that migan_sepconv_forward does not offer: the small-launch tiles of
# MIGAN_GEOMETRIES_SMALL (32-row tiles of plain / pointwise / FIR-up layers, the 32 x 32 K-split tile, the 64-row FIR-up tile), chosen for
# launches of few workgroups.  No operator case can reach them; tests/migan_layers_case.py checks each of their launches in isolation, in
# plan context, and asserts that all 11 of every slice that has them run.
PLAN_ONLY = re.compile(r"^migan::sepconv_kernel<(\d, 32|2, 64), ")


def tile(mode, nt, fromrgb, ni, minw, maing, torgb, stv, persist=False):
    """symbol of the one-tile kernel sepconv_kernel<MODE, MT, NT, KC, FROMRGB, NI, MINW, MAING, PERSIST, GEMMV, TORGB, STV>
    (default GEMM variant: f16x2 for fp32 storage, f16 for 16-bit storage)"""
    b = lambda v: "true" if v else "false"
    return (f"migan::sepconv_kernel<{mode}, 128, {nt}, 32, {b(fromrgb)}, {ni}, {minw}, {b(maing)}, {b(persist)}, {3 if stv else 2}, {b(torgb)}, "
            f"{stv}>")


def pipe(mode, nt, cin, fromrgb, torgb, r, na):
    b = lambda v: "true" if v else "false"
    return f"migan::sepconv_pipe_kernel<{mode}, {nt}, {cin}, {b(fromrgb)}, {b(torgb)}, {r}, {na}>"


def wide(torgb, stv):
    # f32: waves 4-7 run the MFMAs and LDS-DMA staging (tuning wide = 3); 16-bit: the "f16" GEMM variant on the register path
    return f"migan::sepconv_wide_kernel<{'true' if torgb else 'false'}, {stv}, {'true' if stv else 'false'}, true, {'false' if stv else 'true'}, false>"


def dwfir(maing, stv):
    # 16-bit storage: the variant that hands the "f16" pointwise GEMM its A operand ready-made (stv + 2)
    return f"migan::dwfir_kernel<{'7, true' if maing else '9, false'}, {stv + 2 if stv else 0}>"


WIDE_UP = "migan::sepconv_wide_kernel<false, 0, false, true, true, true>"
WIDE2 = "migan::sepconv_wide2_kernel<1>"
WIDE2_PW = "migan::sepconv_wide2_kernel<3>"
PIPEDOWN = "migan::sepconv_pipedown_kernel<128, 64, 2, 12, 4>"
PIPEDOWN256 = "migan::sepconv_pipedown_kernel<256, 128, 2, 12, 4>"


def torgb_kernel(stv):
    return f"migan::torgb_kernel<{stv}>"


@dataclass(frozen=True)
class Row:
    name: str
    kw: dict                       # cin, cout, h, w, batch, down, up
    storages: tuple = STORAGES
    knobs: dict = field(default_factory=dict)
    fused: bool = True             # one workgroup owns all output channels: a ToRGB tail is fused (else torgb_kernel runs after it)
    dw_maing: bool = False         # down=2 rows: whole 4 x 16 tiles for dwfir_kernel

    @property
    def down(self):
        return self.kw.get("down", 1) == 2

    @property
    def up(self):
        return self.kw.get("up", 1) == 2

    @property
    def narrow(self):
        return self.name.startswith("narrow")


ROWS = (
    # narrow_sepconv_kernel<mode, fromrgb>: fewer than 64 channels (cin % 32 or cout % 64), fp32 storage only
    Row("narrow_plain", dict(cin=32, cout=32, h=12, w=20, batch=3)),
    Row("narrow_min", dict(cin=4, cout=4, h=1, w=1, batch=1)),                       # the smallest legal layer
    Row("narrow_down", dict(cin=16, cout=32, h=8, w=12, batch=1, down=2)),
    Row("narrow_up", dict(cin=16, cout=64, h=6, w=10, batch=2, up=2)),               # 18 x 18 x 64 floats = 81 KiB of dynamic LDS
    # the one-tile kernel: ragged sizes (no whole 8 x 16 tiles), plain / FIR-up / smallest sizes
    Row("tile_plain", dict(cin=64, cout=64, h=12, w=20, batch=1)),
    Row("tile_min", dict(cin=32, cout=64, h=1, w=1, batch=1)),
    Row("tile_up", dict(cin=64, cout=128, h=6, w=10, batch=3, up=2)),
    Row("tile_min_up", dict(cin=32, cout=64, h=1, w=1, batch=1, up=2)),
    Row("tile_up64", dict(cin=128, cout=64, h=8, w=16, batch=1, up=2)),              # synthesis.b512.conv1 below the pipelined kernel's threshold
    # two images per tile (8 x 8 layers, 4 x 4 FIR-up inputs), an odd batch leaves the second half of the last tile empty
    Row("tile_imgs", dict(cin=64, cout=128, h=8, w=8, batch=3)),
    Row("tile_up_imgs", dict(cin=64, cout=128, h=4, w=4, batch=3, up=2)),
    # ToRGB on a layer wider than one column tile: torgb_kernel on y afterwards
    Row("torgb_unfused", dict(cin=64, cout=192, h=8, w=16, batch=1), fused=False),
    # down=2 without a fused form: dwfir_kernel + the pointwise GEMM
    Row("dwfir_pw", dict(cin=64, cout=64, h=12, w=20, batch=2, down=2)),
    Row("dwfir_min", dict(cin=32, cout=64, h=2, w=2, batch=1, down=2)),
    # the persistent form of the one-tile pointwise GEMM (a fixed grid of workgroups walks the tiles)
    Row("persist_pw", dict(cin=128, cout=256, h=32, w=64, batch=2, down=2), knobs=dict(persist_min=2, persist_grid=8), fused=False,
        dw_maing=True),
    Row("dwfir_pw_whole", dict(cin=32, cout=64, h=16, w=32, batch=1, down=2), dw_maing=True),     # encoder.b1024.conv2: whole tiles both halves
    # the software-pipelined persistent kernels (fp32 storage)
    Row("pipe64", dict(cin=64, cout=64, h=8, w=16, batch=2), knobs=PERSISTENT),
    Row("pipe128", dict(cin=128, cout=128, h=8, w=16, batch=5), knobs=PERSISTENT),
    Row("pipe_up", dict(cin=128, cout=64, h=6, w=14, batch=2, up=2), knobs=PERSISTENT),
    Row("pipedown", dict(cin=64, cout=128, h=8, w=32, batch=1, down=2), knobs=PERSISTENT, dw_maing=True),
    Row("pipedown256", dict(cin=128, cout=256, h=8, w=32, batch=1, down=2), knobs=PERSISTENT, fused=False, dw_maing=True),
    # 256-column tiles: wide, wide FIR-up, the persistent 256 x 256 tile (plain and pointwise)
    Row("wide", dict(cin=64, cout=256, h=8, w=16, batch=1)),
    Row("wide_up", dict(cin=64, cout=256, h=6, w=10, batch=1, up=2)),
    Row("wide2", dict(cin=64, cout=256, h=16, w=16, batch=1), knobs=PERSISTENT),
    Row("wide2_pw", dict(cin=64, cout=256, h=32, w=32, batch=1, down=2), knobs=PERSISTENT, fused=False, dw_maing=True),
)
ROW = {r.name: r for r in ROWS}

FLAGS = tuple(dict(skip=s, noise=n, torgb=t != "none", with_prev=t == "prev", fromrgb=f)
              for s, n, t, f in itertools.product((False, True), (False, True), ("none", "plain", "prev"), (False, True)))


def flag_id(f):
    t = "prev" if f["with_prev"] else ("rgb" if f["torgb"] else "-")
    return f"{'skip' if f['skip'] else '-'}.{'noise' if f['noise'] else '-'}.{t}.{'frgb' if f['fromrgb'] else '-'}"


def one_tile(row, f, stv):
    """the one-tile kernel each row falls back to (the row's geometry decides NT / NI / MINW / whole tiles)"""
    fr, t = f["fromrgb"], f["torgb"] and row.fused
    return {
        "tile_plain": lambda: tile(0, 64, fr, 9, 2, False, t, stv),
        "tile_min": lambda: tile(0, 64, fr, 9, 2, False, t, stv),
        "tile_up": lambda: tile(2, 128, False, 6, 2, True, False, stv),
        "tile_min_up": lambda: tile(2, 64, False, 9, 2, False, False, stv),
        "tile_up64": lambda: tile(2, 64, False, 6, 2, True, False, stv),
        "tile_imgs": lambda: tile(0, 128, fr, 9, 2, False, t, stv),
        "tile_up_imgs": lambda: tile(2, 128, False, 9, 2, False, False, stv),
        "persist_pw": lambda: tile(3, 128, False, 4, 2, True, False, stv, persist=True),
        "dwfir_pw_whole": lambda: tile(3, 64, False, 4, 2, True, t, stv),
        "torgb_unfused": lambda: tile(0, 64, fr, 6, 3, True, False, stv),
        "dwfir_pw": lambda: tile(3, 64, False, 4, 2, False, t, stv),
        "dwfir_min": lambda: tile(3, 64, False, 4, 2, False, t, stv),
        "pipe64": lambda: tile(0, 64, fr, 6, 3, True, t, stv),
        "pipe128": lambda: tile(0, 128, fr, 6, 2, True, t, stv),
        "pipe_up": lambda: tile(2, 64, False, 6, 2, True, False, stv),
        "pipedown": lambda: tile(3, 128, False, 4, 2, False, False, stv),
        "pipedown256": lambda: tile(3, 128, False, 4, 2, False, False, stv),
        "wide": lambda: tile(0, 128, fr, 6, 2, True, False, stv),
        "wide_up": lambda: tile(2, 128, False, 6, 2, True, False, stv),
        "wide2": lambda: tile(0, 128, fr, 6, 2, True, False, stv),
        "wide2_pw": lambda: tile(3, 128, False, 4, 2, True, False, stv),
    }[row.name]()


def expected(row, f, storage):
    """("refused", exception type, message fragment) or ("ran", last_kernel, [other kernels the call launched])"""
    stv = STV[storage]
    plain = not row.down and not row.up
    if row.narrow:
        mode = 1 if row.down else (2 if row.up else 0)
        if stv:
            return ("refused", NotImplementedError, "fp32 activation storage only")
        if f["torgb"] and not plain:
            return ("refused", ValueError, "ToRGB needs up == down == 1")
        if f["fromrgb"] and not plain:
            return ("refused", ValueError, "fromrgb is only fused into plain layers")
        return ("ran", f"migan::narrow_sepconv_kernel<{mode}, {'true' if f['fromrgb'] else 'false'}>", [])
    if f["torgb"] and row.up:
        return ("refused", ValueError, "ToRGB needs up == 1")
    if f["fromrgb"] and not plain:
        return ("refused", ValueError, "fromrgb is only fused into plain layers")
    # a fused ToRGB tail exists for plain layers without the FromRGB head only; an un-fused one (torgb_kernel) for any layer
    if f["torgb"] and row.fused and (f["fromrgb"] or row.down):
        return ("refused", ValueError, "ToRGB can only be fused into a plain layer whose output channels fit one column tile")
    fused_rgb = f["torgb"] and row.fused
    extra = [torgb_kernel(stv)] if f["torgb"] and not row.fused else []
    f32 = stv == 0
    n = row.name
    if n == "pipe64" and f32 and not f["skip"]:           # (the pipelined plain epilogue has no skip add)
        k = pipe(0, 64, 64, f["fromrgb"], fused_rgb, 2, 4) if f["fromrgb"] else pipe(0, 64, 64, False, fused_rgb, 3, 8)
    elif n == "pipe128" and f32 and not f["skip"] and not f["fromrgb"]:
        k = pipe(0, 128, 128, False, fused_rgb, 2, 4)
    elif n == "pipe_up" and f32:
        k = pipe(2, 64, 128, False, False, 2, 4)
    elif n in ("pipedown", "pipedown256") and f32 and not f["skip"] and not f["noise"] and not f["torgb"]:
        return ("ran", PIPEDOWN if n == "pipedown" else PIPEDOWN256, [])      # one launch: no dwfir_kernel
    elif n == "wide" and not f["fromrgb"]:
        k = wide(fused_rgb, stv)
    elif n == "wide_up" and f32:
        k = WIDE_UP
    elif n == "wide2" and not f["fromrgb"]:
        k = WIDE2 if f32 and not f["skip"] and not f["torgb"] else wide(fused_rgb, stv)
    elif n == "wide2_pw" and f32 and not f["skip"]:
        k = WIDE2_PW
    else:
        k = one_tile(row, f, stv)
    if row.down:
        extra.append(dwfir(row.dw_maing, stv))
    return ("ran", k, extra)


def cases(rows=ROWS):
    """(id, row name, flags, storage) of the whole table (ToRGB with_prev needs an even output size: img_prev is half of it)"""
    out = []
    for row in rows:
        ho = row.kw["h"] // 2 if row.down else (row.kw["h"] * 2 if row.up else row.kw["h"])
        wo = row.kw["w"] // 2 if row.down else (row.kw["w"] * 2 if row.up else row.kw["w"])
        for storage in row.storages:
            for f in FLAGS:
                if f["with_prev"] and (ho % 2 or wo % 2):
                    continue
                out.append((f"{row.name}-{storage}-{flag_id(f)}", row.name, f, storage))
    return out


# missing companion pointers: refused on both branches of migan_sepconv_forward, before anything is launched
COMPANIONS = (
    ("fromrgb_no_bias", dict(fromrgb=True), ("fromrgb_bias",), "fromrgb_weight without fromrgb_bias"),
    ("torgb_no_bias", dict(torgb=True), ("torgb_bias",), "ToRGB needs"),
    ("torgb_no_img_out", dict(torgb=True, with_prev=True), ("img_out",), "ToRGB needs"),
    ("noise_no_strength", dict(noise=True), ("noise_strength",), "noise_const without noise_strength"),
)
COMPANION_ROWS = ("narrow_plain", "tile_plain", "pipe64", "wide")


def run_matrix_case(lib, pkg, mem, row_name, f, storage, seed=29):
    """run one case of the table; returns the kernel names it launched (for the coverage checks), [] for a refusal"""
    row = ROW[row_name]
    want = expected(row, f, storage)
    with knobs(lib, **row.knobs):
        if want[0] == "refused":
            run_sepconv_case(lib, pkg, mem, seed=seed, storage=storage, oracle_f64=True, refused=(want[1], want[2]), **row.kw, **f)
            return []
        run_sepconv_case(lib, pkg, mem, seed=seed, storage=storage, oracle_f64=True, **row.kw, **f)
        assert lib.last_kernel() == want[1], (lib.last_kernel(), want[1])
        return [want[1]] + want[2]


def run_companion_case(lib, pkg, mem, row_name, flags, drop, fragment):
    row = ROW[row_name]
    with knobs(lib, **row.knobs):
        run_sepconv_case(lib, pkg, mem, seed=31, oracle_f64=True, drop=drop, refused=(ValueError, fragment), **row.kw, **flags)


def table_kernels(lib, pkg, mem):
    """every kernel name the passing cases of the table launch"""
    names = set()
    for _, row_name, f, storage in cases():
        names.update(run_matrix_case(lib, pkg, mem, row_name, f, storage))
    return names


def uncovered(plan_names, table_names):
    """names a generator plan launches that no case of the table reports and that are not on the NON_SEPCONV list"""
    return sorted({n for n in plan_names if n not in table_names and not n.startswith(NON_SEPCONV) and not PLAN_ONLY.match(n)})

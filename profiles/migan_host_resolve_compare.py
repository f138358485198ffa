"""Two builds of the emulator library (tests/emu) in one process, dry run, on the same bound tensors and the same workspace address: every
launch (symbol, grid, block, LDS bytes, argument bytes), migan_launch_info before / after each forward, workspace bytes, migan_last_kernel,
return codes and messages are compared over the matrix of profiles/migan_host_resolve.md.

    python profiles/migan_host_resolve_compare.py path/to/the/other/libmigan_emu.so

The other build needs the dry-run switch of tests/emu/hip_emu.h + migan_emu.cpp (copy the two files into its tree and run its
tests/emu/build_emu.py).  Prints the totals and a classification of whatever differs."""
import itertools
import json
import sys
import time

import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import launch_stream as ls          # noqa: E402
from tests import sepconv_matrix as sm         # noqa: E402
from tests.knobs import knobs                  # noqa: E402

from tests.emu.build_emu import build          # noqa: E402

libs = [ls.load(sys.argv[1]), ls.load(build())]      # [the other build ("parent" below), this tree ("branch")]
W = ls.Weights()
rows = []          # (section, case, outcome, launches)
bad = []


def both(fn):
    """run fn(lib) on both libraries; result or (exception type, message)"""
    out = []
    for lib in libs:
        try:
            out.append(("ok", fn(lib)))
        except Exception as e:                       # noqa: BLE001
            ls.take_log(lib)
            out.append(("raised", type(e).__name__, str(e)))
    return out


def record(section, case, res):
    same = res[0] == res[1]
    n = "-"
    if res[0][0] == "ok":
        n = sum(len(s["launches"]) for s in res[0][1]) if isinstance(res[0][1], list) else len(res[0][1]["launches"])
        outcome = "equal" if same else "DIFFERENT"
    else:
        outcome = ("both refuse: " + res[0][2][:60]) if same else "DIFFERENT"
    rows.append((section, case, outcome, n))
    if not same:
        bad.append((section, case, res))
        print("DIFF", section, case, flush=True)


def gen_case(res, storage, gemm, streams, steps, debug=False, **kw):
    def run(lib):
        h = ls.generator(lib, W, res, storage, gemm, streams, debug)
        out = []
        for st in steps:
            out.append(ls.step(lib, h, st[0], st[1], with_args=True, hw=st[2] if len(st) > 2 else None))
        h.close()
        return out
    return both(run)


GEMMS = {"f32": ("f32", "bf16x3", "f16x2"), "bf16": ("f16x2", "f16"), "f16": ("f16x2", "f16")}
t0 = time.time()
with ls.dry_run(libs[0]), ls.dry_run(libs[1]):
    for res, storage in itertools.product((256, 512), ("f32", "bf16", "f16")):
        for gemm, streams, batch in itertools.product(GEMMS[storage], (1, 2), (1, 2, 8, 16, 32, 40)):
            record("migan_forward", f"{res} {storage} {gemm} streams={streams} batch={batch}",
                   gen_case(res, storage, gemm, streams, [("forward", batch)]))
    record("entry points", "migan_forward_timed 512 f32 batch 32", gen_case(512, "f32", None, 2, [("timed", 32)]))
    record("entry points", "migan_forward_timed 256 bf16 batch 32", gen_case(256, "bf16", None, 2, [("timed", 32)]))
    record("entry points", "migan_forward_u8 512 f32 batch 32", gen_case(512, "f32", None, 2, [("u8", 32)]))
    record("entry points", "migan_forward_u8 256 f32 batch 1", gen_case(256, "f32", None, 2, [("u8", 1)]))
    record("entry points", "migan_forward_u8 1024 batch 1 (refused)", gen_case(1024, "f32", None, 2, [("u8", 1)]))
    record("entry points", "migan_forward_parts 512 f32 batch 32", gen_case(512, "f32", None, 2, [("parts", 32)]))
    record("entry points", "migan_forward_parts 512 f32 batch 40 streams 4", gen_case(512, "f32", None, 4, [("parts", 40)]))
    record("entry points", "migan_forward_hw 192x320 on Generator(256), then migan_forward 256",
           gen_case(256, "f32", None, 2, [("forward", 8), ("hw", 2, (192, 320)), ("forward", 1)]))
    record("entry points", "debug plan 256 f32 batch 16", gen_case(256, "f32", None, 2, [("forward", 16)], debug=True))
    record("entry points", "debug plan 512 bf16 batch 1", gen_case(512, "bf16", None, 2, [("forward", 1)], debug=True))
    record("entry points", "Generator(1024) batch 1", gen_case(1024, "f32", None, 2, [("forward", 1)]))
    record("entry points", "Generator(2048) batch 1", gen_case(2048, "f32", None, 2, [("forward", 1)]))
    record("entry points", "512 f32: batch 32 then batch 1", gen_case(512, "f32", None, 2, [("forward", 32), ("forward", 1)]))
    record("entry points", "256 bf16: batch 32 then batch 1 then timed 16", gen_case(256, "bf16", None, 2, [("forward", 32), ("forward", 1), ("timed", 16)]))

    KNOBS = dict(kc16=7, kc16_minw=4, w3=0, wide=2, wide_up=0, small=0, small_max_wgs=128, small_kc=32, small_up32=0, small_dwfir=0,
                 small_ksplit=0, nt256=0, persist_min=1024, persist_grid=256, streams=4, stagger=5, single_b=1, debug_split=1, stagger_pct=40,
                 pipe=0, pipe_grid=128, pipe_na=8, pipe_na8=0, pipe_dna=8, pipe_min_tiles=4096, pipe_min_batch=2, w2=1, w2_min_tiles=4096, w2_pw=0)
    assert sorted(KNOBS) == sorted(libs[0].tuning_keys()), set(libs[0].tuning_keys()) ^ set(KNOBS)
    for key, value in list(KNOBS.items()) + [("wide", 0), ("w2", 0), ("pipe", 7), ("pipe", 8)]:
        for res, storage in ((512, "f32"), (256, "f32"), (256, "bf16")):
            with knobs(libs[0], **{key: value}), knobs(libs[1], **{key: value}):
                # knob set before the plan is made (plan-time knobs) ...
                record("knobs", f"{key}={value} {res} {storage}: batch 32, batch 1", gen_case(res, storage, None, 2, [("forward", 32), ("forward", 1)]))

                # ... and between two forwards of one handle (knobs the resolved path reads per forward)
            def flip(lib, key=key, value=value, res=res, storage=storage):
                h = ls.generator(lib, W, res, storage)
                out = [ls.step(lib, h, "forward", 32, with_args=True)]
                with knobs(lib, **{key: value}):
                    out.append(ls.step(lib, h, "forward", 32, with_args=True))
                    out.append(ls.step(lib, h, "forward", 1, with_args=True))
                out.append(ls.step(lib, h, "forward", 32, with_args=True))
                h.close()
                return out
            record("knobs", f"{key}: default -> {value} -> default on one handle, {res} {storage}", both(flip))

    # migan_sepconv_forward: every row x flag combination x storage of tests/sepconv_matrix.py
    for cid, row_name, f, storage in sm.cases():
        row = sm.ROW[row_name]
        kw = dict(row.kw)
        h, w, n, cin, cout = kw["h"], kw["w"], kw["batch"], kw["cin"], kw["cout"]
        down, up = kw.get("down", 1), kw.get("up", 1)
        a = ls.FAKE
        args = dict(x=a, y=a + (1 << 30), conv1_weight=a + (2 << 30), conv1_bias=a + (3 << 30), conv2_weight=a + (4 << 30), batch=n, cin=cin, cout=cout,
                    res_in=h, width_in=w, down=down, up=up, dtype=sm.STV[storage], scratch=a + (5 << 30), scratch_bytes=1 << 30, wsplit=a + (6 << 30),
                    wsplit_bytes=1 << 30)
        if f["skip"]:
            args["skip"] = a + (7 << 30)
        if f["noise"]:
            args.update(noise_const=a + (8 << 30), noise_strength=a + (9 << 30))
        if f["fromrgb"]:
            args.update(fromrgb_weight=a + (10 << 30), fromrgb_bias=a + (11 << 30))
        if f["torgb"]:
            args.update(torgb_weight=a + (12 << 30), torgb_bias=a + (13 << 30), img_out=a + (14 << 30))
        if f["with_prev"]:
            args["img_prev"] = a + (15 << 30)

        def run(lib, args=args, row=row):
            with knobs(lib, **row.knobs):
                try:
                    lib.sepconv_forward(**args)
                    rc = ("ok",)
                except Exception as e:             # noqa: BLE001
                    rc = (type(e).__name__, str(e))
            return dict(rc=rc, launches=ls.take_log(lib, with_args=True), last_kernel=lib.last_kernel())
        res = both(run)
        want = sm.expected(row, f, storage)
        got = res[1][1]
        if want[0] == "ran":
            ok = got["rc"] == ("ok",) and got["last_kernel"] == want[1]
        else:
            ok = got["rc"][0] == want[1].__name__ and want[2] in got["rc"][1]
        if not ok:
            print("UNEXPECTED (branch vs rule table)", cid, got["rc"], got["last_kernel"], want, flush=True)
            bad.append(("sepconv-expected", cid, got["rc"]))
        same = res[0] == res[1]
        rows.append(("migan_sepconv_forward", cid, "equal" if same else "DIFFERENT", len(got["launches"])))
        if not same:
            bad.append(("migan_sepconv_forward", cid, res))

print("seconds", time.time() - t0)
print("cases", len(rows), "different", sum(1 for r in rows if r[2] == "DIFFERENT"))
for sec in dict.fromkeys(r[0] for r in rows):
    sub = [r for r in rows if r[0] == sec]
    print(f"{sec}: {len(sub)} cases, {sum(r[3] for r in sub if isinstance(r[3], int))} launches, "
          f"{sum(1 for r in sub if r[2] == 'DIFFERENT')} different")

# ---- classify the differences
kinds = {}
for sec, case, res in bad:
    if sec == "migan_sepconv_forward":
        p, b = res[0][1], res[1][1]
        if p["rc"] == b["rc"] and p["rc"] != ("ok",) and b["launches"] == [] and p["launches"] and p["last_kernel"] == b["last_kernel"]:
            k = "refusal: parent launched %s first, branch nothing" % "+".join(sorted({l[0].split("<")[0].split("::")[1] for l in p["launches"]}))
        else:
            k = "OTHER"
        kinds.setdefault(k, []).append(case)
    elif sec == "knobs":
        ps, bs = res[0][1], res[1][1]
        what = set()
        for si, (p, b) in enumerate(zip(ps, bs)):
            for key in p:
                if p[key] != b[key]:
                    if key in ("after", "before"):
                        for i, (x, y) in enumerate(zip(p[key], b[key])):
                            if x != y:
                                what.add(f"{key}[{x['layer']}]: parent {x['kernel'][:45]} / branch {y['kernel'][:45]} / launched {bs[si]['launches'] and ''}")
                    else:
                        what.add(key)
        kinds.setdefault(" ; ".join(sorted(what))[:600], []).append(case)
    else:
        kinds.setdefault("OTHER " + sec, []).append(case)
for k, v in kinds.items():
    print(len(v), k, v[:3])

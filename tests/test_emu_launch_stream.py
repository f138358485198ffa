"""What a generator forward launches at production sizes, launch by launch, against a recorded list: kernel symbol, grid, block and LDS
bytes of every launch, and the names migan_launch_info reports before and after.  Which kernel runs where is a host decision
(migan_host.hpp: resolve_layer, Plan::resolve), so a dry run of the emulator library sees it without a GPU -- migan-512 at batch 32 takes
milliseconds -- and a change that is meant to leave it alone can prove that it did.

tests/golden/migan_launch_streams.json was recorded from the commit BEFORE the host learned to resolve a forward's launches up front
(its emulator given the same dry-run switch), so it pins that refactor to the launches of the code it replaced.  A change that moves a
launch on purpose records the file again from its own build and says so:
    python -m tests.test_emu_launch_stream --record [path/to/libmigan_emu.so]
"""
import json
import os
import sys

import pytest

from tests import launch_stream as ls

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "migan_launch_streams.json")

# id -> (resolution, activation storage, [(kind, batch), ...] on one handle); two streams, default knobs
CASES = {f"forward-{res}-{storage}-b{batch}": (res, storage, [("forward", batch)])
         for res in (256, 512) for storage in ("f32", "bf16") for batch in (1, 8, 32)}
CASES["timed-512-f32-b32"] = (512, "f32", [("timed", 32)])                          # whole-batch launches, the forms of a 16-image sub-batch
CASES["sequence-512-f32-b32-b1"] = (512, "f32", [("forward", 32), ("forward", 1)])   # the second forward's names replace the first's
CASES["forward-1024-f32-b1"] = (1024, "f32", [("forward", 1)])                      # narrow layers at both ends


def run_case(lib, weights, case):
    res, storage, steps = CASES[case]
    with ls.dry_run(lib):
        h = ls.generator(lib, weights, res, storage, streams=2)
        out = []
        for kind, batch in steps:
            s = ls.step(lib, h, kind, batch)
            out.append(dict(before=[l["kernel"] for l in s["before"]], launches=s["launches"], after=[l["kernel"] for l in s["after"]]))
        h.close()
    return out


def record(path):
    lib, weights = ls.load(path), ls.Weights()
    symbols, cases = [], {}

    def idx(name):
        if name not in symbols:
            symbols.append(name)
        return symbols.index(name)

    for case in CASES:
        cases[case] = [dict(before=[idx(n) for n in s["before"]], launches=[[idx(l[0])] + l[1:] for l in s["launches"]],
                            after=[idx(n) for n in s["after"]]) for s in run_case(lib, weights, case)]
    with open(GOLDEN, "w") as f:
        json.dump(dict(symbols=symbols, cases=cases), f, separators=(",", ":"))
        f.write("\n")
    return GOLDEN


@pytest.fixture(scope="module")
def env():
    from tests.emu.build_emu import build
    with open(GOLDEN) as f:
        golden = json.load(f)
    return ls.load(build()), ls.Weights(), golden


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_stream(env, case):
    lib, weights, golden = env
    sym = golden["symbols"]
    got, want = run_case(lib, weights, case), golden["cases"][case]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["before"] == [sym[k] for k in w["before"]], f"step {i}: migan_launch_info before the forward"
        wl = [[sym[l[0]]] + l[1:] for l in w["launches"]]
        assert len(g["launches"]) == len(wl), f"step {i}: {len(g['launches'])} launches, recorded {len(wl)}"
        for j, (a, b) in enumerate(zip(g["launches"], wl)):
            assert a == b, f"step {i}, launch {j}: [symbol, grid, block, LDS bytes] {a}, recorded {b}"
        assert g["after"] == [sym[k] for k in w["after"]], f"step {i}: migan_launch_info after the forward"


def test_golden_covers_the_cases(env):
    assert sorted(env[2]["cases"]) == sorted(CASES)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        from tests.emu.build_emu import build
        print(record(sys.argv[2] if len(sys.argv) > 2 else build()))

"""The process-wide tuning knobs (migan_set_tuning / migan_get_tuning / migan_tuning_key over the one knob table of
mi-gan_amd/csrc/migan_host.hpp), through the CPU emulator build of the same host code: the keys, defaults, normalisation
and environment variables are what they were when each was a branch of an if-chain, and tests/knobs.py puts back what it
borrowed.  The two tests that need a fresh process (the environment is read once) start a new Python with the emulator
library; everything else runs inside the helper and leaves nothing behind."""
import json
import os
import subprocess
import sys

import pytest

from tests.emu_util import ROOT, emu_lib
from tests.knobs import knobs

# key -> default initialiser of struct Tuning.  The one place that lists the knobs: adding, dropping or re-defaulting one shows up here.
DEFAULTS = dict(kc16=0, kc16_minw=3, w3=3, wide=3, wide_up=1, small=1, small_max_wgs=512, small_kc=64, small_up32=1, small_dwfir=1,
                small_ksplit=1, nt256=1, persist_min=8192, persist_grid=512, streams=2, stagger=-1, single_b=0, debug_split=0,
                stagger_pct=15, pipe=15, pipe_grid=256, pipe_na=4, pipe_na8=9, pipe_dna=12, pipe_min_tiles=256, pipe_min_batch=1,
                w2=2, w2_min_tiles=256, w2_pw=1)

# (key, requested, stored)
NORMALISED = [("kc16_minw", 1, 2), ("kc16_minw", 7, 4), ("nt256", 5, 1), ("single_b", -3, 1), ("debug_split", 2, 1), ("w2_pw", 9, 1),
              ("persist_min", 0, 1), ("pipe_min_tiles", -4, 1), ("pipe_min_batch", 0, 1), ("w2_min_tiles", 0, 1), ("persist_grid", 13, 8),
              ("persist_grid", 519, 512), ("pipe_grid", 3, 8), ("pipe_grid", 70, 64), ("streams", 0, 1), ("streams", 9, 4),
              ("stagger_pct", -5, 0), ("stagger_pct", 150, 100), ("pipe_na", 8, 8), ("pipe_na", 5, 4), ("w2", -1, 0), ("w2", 5, 2)]
UNTOUCHED = ["kc16", "w3", "wide", "wide_up", "small", "small_max_wgs", "small_kc", "small_up32", "small_dwfir", "small_ksplit", "stagger",
             "pipe", "pipe_na8", "pipe_dna"]


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def _fresh_process(env_vars):
    """knobs and GEMM variant a new process reports whose only MIGAN_* variables are `env_vars`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIGAN_")}
    env.update(env_vars)
    code = ("import json; from tests.emu_util import emu_lib; lib = emu_lib(); "
            "print(json.dumps(dict(knobs={k: lib.get_tuning(k) for k in lib.tuning_keys()}, gemm=lib.gemm_variant())))")
    emu_lib()                                              # (built here, once, not by the child)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("key,requested,stored", NORMALISED)
def test_normalisation_is_what_it_was(lib, key, requested, stored):
    with knobs(lib, **{key: requested}):
        assert lib.get_tuning(key) == stored


@pytest.mark.parametrize("key", UNTOUCHED)
@pytest.mark.parametrize("value", [-7, 1000])
def test_keys_without_a_normaliser_store_the_request(lib, key, value):
    with knobs(lib, **{key: value}):
        assert lib.get_tuning(key) == value


def test_the_key_set_is_the_parents(lib):
    keys = lib.tuning_keys()
    assert len(keys) == 29 and sorted(keys) == sorted(DEFAULTS), keys
    assert lib.lib.migan_tuning_key(-1) is None and lib.lib.migan_tuning_key(len(keys)) is None
    for key in ("gemm", "nope"):                           # (MIGAN_GEMM is a string and environment-only)
        with pytest.raises(ValueError, match=f"unknown tuning key: {key}"):
            lib.set_tuning(key, 0)
        with pytest.raises(ValueError, match=f"unknown tuning key: {key}"):
            lib.get_tuning(key)
    assert lib.lib.migan_get_tuning(b"pipe", None) != 0    # MIGAN_EINVAL for a null pointer, not a crash


def test_defaults_are_the_structs():
    got = _fresh_process({})
    assert got["knobs"] == DEFAULTS
    assert got["gemm"] == "f16x2"


@pytest.mark.parametrize("key", sorted(DEFAULTS))
def test_setting_back_a_stored_value_changes_nothing(lib, key):
    """what tests/knobs.py rests on: every normaliser is a clamp or a rounding, so a stored value normalises to itself"""
    with knobs(lib, **{key: lib.get_tuning(key)}):
        for requested in (None, -7, -1, 0, 1, 2, 5, 8, 9, 13, 70, 150, 519, 1000):
            if requested is not None:
                lib.set_tuning(key, requested)
            first = lib.get_tuning(key)
            lib.set_tuning(key, first)
            assert lib.get_tuning(key) == first, (key, requested)


def test_the_environment_pass_is_what_it_was():
    env = dict(MIGAN_PERSIST_GRID="13", MIGAN_PIPE_GRID="70", MIGAN_STREAMS="9", MIGAN_KC16_MINW="1", MIGAN_NT256="5", MIGAN_SINGLE_B="2",
               MIGAN_W2="7", MIGAN_PERSIST_MIN="0", MIGAN_KC16="5", MIGAN_W3="1", MIGAN_WIDE="2", MIGAN_STAGGER="9", MIGAN_PIPE="7",
               MIGAN_GEMM="bf16x3", MIGAN_STAGGER_PCT="50")       # (the last one is not a variable the library reads)
    got = _fresh_process(env)
    want = dict(persist_grid=8, pipe_grid=64, streams=4, kc16_minw=2, nt256=1, single_b=1, w2=2, persist_min=1, kc16=5, w3=1, wide=2,
                stagger=9, pipe=7)
    assert {k: got["knobs"][k] for k in want} == want
    assert got["gemm"] == "bf16x3"
    assert {k: v for k, v in got["knobs"].items() if k not in want} == {k: v for k, v in DEFAULTS.items() if k not in want}


def test_the_helper_restores_when_the_body_raises(lib):
    before = {k: lib.get_tuning(k) for k in lib.tuning_keys()}
    with pytest.raises(RuntimeError, match="body failed"):
        with knobs(lib, pipe=0, persist_grid=13, stagger_pct=70, w2=1):
            assert (lib.get_tuning("pipe"), lib.get_tuning("persist_grid"), lib.get_tuning("stagger_pct"), lib.get_tuning("w2")) == (0, 8, 70, 1)
            raise RuntimeError("body failed")
    assert {k: lib.get_tuning(k) for k in lib.tuning_keys()} == before
    with pytest.raises(ValueError):                        # a key the library refuses: nothing was set, nothing is left behind
        with knobs(lib, pipe=0, nope=1):
            pass
    assert {k: lib.get_tuning(k) for k in lib.tuning_keys()} == before

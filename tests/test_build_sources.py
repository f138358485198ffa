"""The freshness lists of the two in-tree builds (mi-gan_amd/build.py, tests/emu/build_emu.py) are read from the directories: every
file a library is built from is watched, so editing one can never leave a stale library that the tests then pass against."""
import importlib.util
import os
import re

from tests.emu import build_emu
from tests.emu_util import ROOT

CSRC = os.path.join(ROOT, "mi-gan_amd", "csrc")


def _product_build():
    spec = importlib.util.spec_from_file_location("migan_build", os.path.join(ROOT, "mi-gan_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _included(path, seen):
    """the quoted includes of `path`, followed"""
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
        _included(os.path.normpath(os.path.join(os.path.dirname(path), inc)), seen)
    return seen


def test_every_file_the_libraries_include_is_watched():
    product = set(_product_build().sources())
    units = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip")]
    assert units
    for unit in units:
        missing = _included(unit, set()) - product
        assert not missing, f"{os.path.basename(unit)} includes files the product build does not watch: {sorted(missing)}"
    emu = set(build_emu.sources())
    missing = _included(build_emu.SRC, set()) - emu
    assert not missing, f"the emulator includes files its build does not watch: {sorted(missing)}"
    for name in ("migan_pipeline_regions.inc", "migan_pipeline_region_patches.inc", "migan_pipeline_pool_body.inc",
                 "migan_pipeline_samples_body.inc", "migan_metrics.hpp", "migan_photo.hpp", "migan_masks.hpp", "migan_masks_host.hpp"):
        assert os.path.join(CSRC, name) in emu and os.path.join(CSRC, name) in product, name


def test_only_sources_are_watched():
    """no build product or cache among them: touching no file means no rebuild"""
    for path in set(_product_build().sources()) | set(build_emu.sources()):
        assert path.endswith((".hip", ".hpp", ".inc", ".h", ".cpp")) and os.path.isfile(path), path

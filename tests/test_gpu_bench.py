"""bench.py on an MI355X: a plain run times exactly --steps steps and prints the headline figure only; --dump-outputs writes what the
timed path computed in its last step, the same from run to run, and that is the generator's image of the seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import migan_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("gpu tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "migan-64", "--batch", "16", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_the_last_step_and_measures_nothing_else(pkg, dev, tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["max_abs_vs_ref"] is None
    for key in ("secondary", "latency_b1_ms", "rccl_world1", "value_exact_f32"):
        assert key not in line
    y = np.load(tmp_path / "a" / "output.npy")
    assert y.dtype == np.float32 and y.shape == (16, 3, 64, 64)
    # the inputs bench.py builds (seeded): the dumped images are the generator's output on them
    sd = pkg.synth.make_state_dict(64, seed=0, regime="export")
    x = pkg.synth.make_input(16, 64, seed=100, kind="demo")
    want = orc.generator(x[:2], sd, 64)
    assert float(np.abs(y[:2] - want).max()) <= 1e-3
    # a second run on the same arguments computes the same images
    _bench(tmp_path / "b")
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "output.npy"), y)


def test_plain_run_makes_warmup_plus_steps_forwards_and_times_them(pkg, dev, monkeypatch):
    """--steps sets the number of timed steps: a plain run calls the generator exactly warmup + steps times (no other forward anywhere:
    no roofline, latency or parity pass), and ms_per_step is the timed region divided by --steps"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_gpu_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    calls = []
    real = pkg.Generator.forward

    def counted(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)

    monkeypatch.setattr(pkg.Generator, "forward", counted)
    for steps in (3, 6):
        calls.clear()
        args = b.parse(["--model", "migan-64", "--batch", "16", "--steps", str(steps), "--warmup", "2"])
        line = b.run_workload(args, 0, 0, 1, None, dev)
        assert len(calls) == 2 + steps, (steps, len(calls))
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert abs(line["value"] - 16 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]

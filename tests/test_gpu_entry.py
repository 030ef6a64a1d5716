"""The driver's entry points in ONE fresh process, in the order that used to fail: build() loads libinpaintnet_hip.so before
anything has touched the GPU; smoke() then runs a training step.  (PyTorch-ROCm ships its own HIP runtime: the library must bind
to that one -- inpaintnet_amd/_lib.py imports torch before it loads the library; loaded first it pulled in /opt/rocm's copy as a
second runtime and the first launch failed with hipErrorNoDevice.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loaded_before_torch_then_smoke():
    code = ("from inpaintnet_amd import _lib\n"
            "L = _lib.lib()\n"                       # (what build() does after compiling; without the rebuild: seconds, not minutes)
            "assert L.inet_abi_version() == 1\n"
            "import __graft_entry__ as g\n"
            "g.smoke()\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[smoke] ok" in r.stdout


def test_bench_prints_exactly_one_small_line(tmp_path):
    """The driver's command with --full (short form: no extras, no CPU baseline) in a subprocess: stdout is ONE JSON line under
    bench.py's 4 KB limit with the contract's keys; the detail went to bench_detail.json (round 5's 20 KB line was dropped by the
    driver)."""
    import json
    detail = str(tmp_path / "bench_detail_test.json")
    env = dict(os.environ, INET_BENCH_DETAIL=detail)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full",
                        "--no-extras", "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[:2000]
    assert len(lines[0]) < 4096
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["steps"] == 20 and line["warmup"] == 5 and line["n_gpus"] == 1 and line["chain_timeouts"] == 0
    assert line["parity_checked"] is True
    assert "priming_steps" not in line["config"]               # --warmup 5 means five
    assert line["roofline"]["bound"] in ("mfma", "hbm") and 0.0 < line["roofline"]["frac"] < 1.0
    full = json.load(open(detail))
    assert full["value"] == line["value"] and len(full["roofline"]["kernels"]) >= 4


def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """The plain command (no --full) prints the headline line and nothing it did not measure; --dump-outputs writes the last
    timed step's loss, accuracy and the fixed samples of the trained weights and their gradients.  Two runs with the same
    arguments compute the same outputs to round-off: every step starts from the seeded weights, so the last bits in which the
    kernels' atomics differ from run to run are not amplified by training (they were, to ~5e-2 of the gradients' norm, after
    45 steps of training on their own results)."""
    import json
    import numpy as np

    def run(tag):
        out = tmp_path / tag
        env = dict(os.environ, INET_BENCH_DETAIL=str(tmp_path / f"{tag}_detail.json"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5",
                            "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == 1, r.stdout[:2000]
        line = json.loads(lines[0])
        assert not os.path.exists(env["INET_BENCH_DETAIL"]) and "detail" not in line
        return line, {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}

    line, a = run("a")
    assert line["steps"] == 40 and line["warmup"] == 5 and line["n_gpus"] == 1 and line["chain_timeouts"] == 0
    assert line["unit"] == "measures/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(256 * 1e3 / line["ms_per_step"], rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and "parity_checked" not in line and "extras" not in line
    assert "first_steps_ms" not in line
    assert sorted(a) == ["accuracy", "grads_sample", "loss", "params_sample"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["params_sample"].shape == a["grads_sample"].shape == (1 << 22,)
    assert all(np.isfinite(v).all() for v in a.values()) and 0.0 <= float(a["accuracy"][0]) <= 1.0
    assert float(a["loss"][0]) == pytest.approx(line["config"]["final_loss"], abs=1e-5)
    _, b = run("b")
    assert float(b["loss"][0]) == pytest.approx(float(a["loss"][0]), rel=1e-6)
    assert np.linalg.norm(b["grads_sample"] - a["grads_sample"]) <= 1e-6 * np.linalg.norm(a["grads_sample"])
    assert np.abs(b["params_sample"] - a["params_sample"]).max() <= 1e-6 * np.abs(a["params_sample"]).max()

"""bench.py driver contract: one JSON line on stdout with the agreed
fields (the round-end harness parses exactly this)."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract_cpu():
    r = subprocess.run(
        [sys.executable, "bench.py", "--batch", "8", "--steps", "2",
         "--warmup", "1"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for key in ["metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"]:
        assert key in d, key
    assert d["unit"] == "images/sec"
    assert d["scaling"] == "weak"
    assert d["higher_is_better"] is True
    assert d["data"] == "synthetic"
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["config"]["model"] == "resnet18"
    assert d["config"]["global_batch"] == 8
    assert d["value"] > 0


def _run_dump(outdir, extra=(), model="net", batch=8):
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--model", model,
         "--batch", str(batch), "--steps", "3", "--warmup", "1",
         "--dump-outputs", str(outdir), *extra],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _loss_from_dumped_logits(outdir, batch, steps=3):
    """Mean cross-entropy, in float64, of the dumped logits against the
    labels of the LAST timed step (step i uses pool batch i % N_POOL; the
    pool is rebuilt here from the benchmark's own seeded generator). It
    equals loss.npy only if both come from that one step."""
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    _, ys = bench.synthetic_pool(batch, 32, 10)
    logits = torch.from_numpy(np.load(os.path.join(outdir, "logits.npy")))
    return float(torch.nn.functional.cross_entropy(
        logits.double(), ys[(steps - 1) % bench.N_POOL]))


# fp32 loss kernel vs float64 on the same logits: per sample, 10 fast-math
# exps and one log at a few 2^-22 relative each on a loss near 2.3, then an
# fp32 mean -- under 1e-5 in all; 1e-4 leaves a decade of room and is two
# decades under the step-to-step change of the loss (1e-2 and more)
_LOSS_TOL = 1e-4


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 .npy,
    identically from run to run; --full is accepted and keeps the result
    line's fields."""
    import numpy as np
    d1 = _run_dump(tmp_path / "a")
    d2 = _run_dump(tmp_path / "b", extra=("--full",))
    assert d1["steps"] == 3 and d1["ms_per_step"] > 0
    assert set(d1) == set(d2)
    total = 0
    for name in ["loss", "logits", "params", "grads"]:
        a = np.load(tmp_path / "a" / f"{name}.npy")
        b = np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 2**20
    assert np.load(tmp_path / "a" / "logits.npy").shape == (8, 10)
    assert abs(float(np.load(tmp_path / "a" / "loss.npy"))
               - d1["config"]["loss_final"]) < 1e-3
    assert abs(float(np.load(tmp_path / "a" / "loss.npy"))
               - _loss_from_dumped_logits(tmp_path / "a", 8)) < _LOSS_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["0", "1"])
def test_bench_dump_outputs_gpu(tmp_path, graph):
    """ResNet-18 on the GPU, eager and hipGraph-replayed: the dump holds
    the last step's loss and logits in full and the seeded 7M-element
    sample of the 11.2M-element flat parameter / gradient buffers."""
    import numpy as np
    d = _run_dump(tmp_path, extra=("--graph", graph), model="resnet18",
                  batch=64)
    assert d["config"]["hip_graph"] is (graph == "1")
    got = {n: np.load(tmp_path / f"{n}.npy")
           for n in ["loss", "logits", "params", "grads"]}
    for name, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert got["logits"].shape == (64, 10)
    assert got["params"].shape == got["grads"].shape == (7_000_000,)
    assert np.abs(got["grads"]).max() > 0
    assert abs(float(got["loss"]) - d["config"]["loss_final"]) < 1e-3
    # logits and loss come from the same (last) step, graph replay included
    assert abs(float(got["loss"])
               - _loss_from_dumped_logits(tmp_path, 64)) < _LOSS_TOL
    assert sum(a.nbytes for a in got.values()) <= 64 * 2**20


@pytest.mark.gpu
def test_bench_dump_repeats_gpu(tmp_path):
    """Two runs with the same arguments dump bit-identical arrays: the
    kernels' split reductions fold their partials in a fixed order."""
    import numpy as np
    _run_dump(tmp_path / "a", model="resnet18", batch=64)
    _run_dump(tmp_path / "b", model="resnet18", batch=64)
    for name in ["loss", "logits", "params", "grads"]:
        a = np.load(tmp_path / "a" / f"{name}.npy")
        b = np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b), name

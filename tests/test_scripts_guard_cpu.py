"""The training scripts' MI355X_CLIP_NORM / MI355X_DEVICE_SCALER knobs run
end to end on CPU (the guarded step's plain-torch fallbacks; gloo for DDP)."""

import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = {
    "MI355X_SYNTHETIC": "1",
    "MI355X_STEPS": "3",
    "MI355X_EPOCHS": "1",
    "MI355X_BATCH": "8",
    "MI355X_CLIP_NORM": "0.5",
    "MI355X_FP16": "1",
    "MI355X_DEVICE_SCALER": "1",
}


def _run(cmd, extra_env, timeout=300):
    env = dict(os.environ)
    env.update(extra_env)
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=timeout)


def test_serial_script_with_clipping_and_device_scaler(tmp_path):
    r = _run([sys.executable, "cifar_example.py"],
             dict(KNOBS, MI355X_CKPT=str(tmp_path / "net.pth")))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert (tmp_path / "net.pth").exists()


def test_device_scaler_knob_needs_fp16(tmp_path):
    env = dict(KNOBS, MI355X_CKPT=str(tmp_path / "net.pth"))
    env["MI355X_FP16"] = "0"
    r = _run([sys.executable, "cifar_example.py"], env)
    assert r.returncode != 0
    assert "MI355X_DEVICE_SCALER=1 needs MI355X_FP16=1" in r.stderr


def test_ddp_script_with_clipping_and_device_scaler(tmp_path):
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
              "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29619", "cifar_example_ddp.py"],
             dict(KNOBS, MI355X_CKPT=str(tmp_path / "net_ddp.pth")),
             timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert (tmp_path / "net_ddp.pth").exists()

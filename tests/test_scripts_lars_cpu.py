"""The training scripts' MI355X_OPTIM / MI355X_WD / MI355X_LARS_ETA knobs
run end to end on CPU (the LARS plain-torch fallbacks; gloo for DDP), and
the optimizer the scripts report is the one the knobs ask for."""

import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = {
    "MI355X_SYNTHETIC": "1",
    "MI355X_STEPS": "3",
    "MI355X_EPOCHS": "1",
    "MI355X_BATCH": "8",
    "MI355X_OPTIM": "lars",
    "MI355X_WD": "5e-4",
}
GUARDED = {
    "MI355X_FP16": "1",
    "MI355X_DEVICE_SCALER": "1",
    "MI355X_CLIP_NORM": "0.5",
}


def _run(cmd, extra_env, timeout=300):
    env = dict(os.environ)
    env.update(extra_env)
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _trains(r, ckpt, optimizer_line):
    assert r.returncode == 0, r.stderr[-2000:]
    assert optimizer_line in r.stdout.splitlines(), r.stdout[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert ckpt.exists()


def test_serial_script_with_lars(tmp_path):
    ckpt = tmp_path / "net.pth"
    _trains(_run([sys.executable, "cifar_example.py"],
                 dict(KNOBS, MI355X_CKPT=str(ckpt))), ckpt,
            "optimizer: LARS lr=0.001 momentum=0.9 weight_decay=0.0005 "
            "trust_coefficient=0.001")


def test_serial_script_with_lars_clipping_and_device_scaler(tmp_path):
    ckpt = tmp_path / "net.pth"
    _trains(_run([sys.executable, "cifar_example.py"],
                 dict(KNOBS, **GUARDED, MI355X_LARS_ETA="0.002",
                      MI355X_CKPT=str(ckpt))), ckpt,
            "optimizer: LARS lr=0.001 momentum=0.9 weight_decay=0.0005 "
            "trust_coefficient=0.002")


def test_serial_script_passes_weight_decay_to_sgd(tmp_path):
    ckpt = tmp_path / "net.pth"
    env = dict(KNOBS, MI355X_WD="0.01", MI355X_CKPT=str(ckpt))
    del env["MI355X_OPTIM"]
    _trains(_run([sys.executable, "cifar_example.py"], env), ckpt,
            "optimizer: SGD lr=0.001 momentum=0.9 weight_decay=0.01")


def test_ddp_script_with_lars(tmp_path):
    ckpt = tmp_path / "net_ddp.pth"
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
              "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29741", "cifar_example_ddp.py"],
             dict(KNOBS, **GUARDED, MI355X_LARS_ETA="0.002",
                  MI355X_CKPT=str(ckpt)), timeout=600)
    _trains(r, ckpt,
            "optimizer: LARS lr=0.001 momentum=0.9 weight_decay=0.0005 "
            "trust_coefficient=0.002")


def test_unknown_optimizer_names_the_valid_ones(tmp_path):
    r = _run([sys.executable, "cifar_example.py"],
             dict(KNOBS, MI355X_OPTIM="adam",
                  MI355X_CKPT=str(tmp_path / "net.pth")))
    assert r.returncode != 0
    assert "MI355X_OPTIM=adam: expected sgd or lars" in r.stderr
    assert "Traceback" not in r.stderr
    assert not (tmp_path / "net.pth").exists()

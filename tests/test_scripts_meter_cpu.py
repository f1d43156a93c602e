"""The training scripts' MI355X_DEVICE_METER knob end to end on CPU (the
meter's plain-torch twin; gloo for DDP): the runs finish and checkpoint, the
reference accuracy line keeps its format, the test-loss/top-5 and per-class
lines appear, and with the knob unset nothing new is printed."""

import math
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = {
    "MI355X_SYNTHETIC": "1",
    "MI355X_STEPS": "3",
    "MI355X_EPOCHS": "1",
    "MI355X_BATCH": "8",
}
METER = {"MI355X_DEVICE_METER": "1"}

ACC = re.compile(r"Accuracy of the network on the 10000 test images: \d+ %")
ACC_EMA = re.compile(
    r"Accuracy of the EMA weights on the 10000 test images: \d+ %")
LOSS = re.compile(r"Test loss: (\S+), top-5 accuracy: (\S+) %")
PER_CLASS = re.compile(r"Per-class accuracy:(?: \d+: \S+ %){10}")


def _run(cmd, extra_env, timeout=300):
    env = dict(os.environ)
    env.pop("MI355X_DEVICE_METER", None)
    env.update(extra_env)
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _count(pattern, lines):
    return sum(1 for l in lines if pattern.fullmatch(l))


def _metered(r, ckpt, evaluations=1):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert "Finished Training (3 steps" in r.stdout
    assert ckpt.exists()
    assert _count(ACC, lines) == 1, r.stdout[-2000:]
    assert _count(PER_CLASS, lines) == evaluations, r.stdout[-2000:]
    found = [m for m in map(LOSS.fullmatch, lines) if m]
    assert len(found) == evaluations, r.stdout[-2000:]
    for m in found:
        loss, top5 = float(m.group(1)), float(m.group(2))
        assert math.isfinite(loss) and loss > 0
        assert 0.0 <= top5 <= 100.0
    # the new lines follow the accuracy line they belong to
    at = next(i for i, l in enumerate(lines) if ACC.fullmatch(l))
    assert LOSS.fullmatch(lines[at + 1]) and PER_CLASS.fullmatch(lines[at + 2])
    return lines


def test_serial_script_with_the_meter_and_an_ema(tmp_path):
    ckpt = tmp_path / "net.pth"
    r = _run([sys.executable, "cifar_example.py"],
             dict(KNOBS, **METER, MI355X_EMA="0.9", MI355X_CKPT=str(ckpt)))
    lines = _metered(r, ckpt, evaluations=2)
    at = next(i for i, l in enumerate(lines) if ACC_EMA.fullmatch(l))
    assert LOSS.fullmatch(lines[at + 1]) and PER_CLASS.fullmatch(lines[at + 2])
    assert (tmp_path / "net_ema.pth").exists()


def test_serial_script_meters_the_cutmix_loss_it_already_has(tmp_path):
    ckpt = tmp_path / "net.pth"
    mix = {"MI355X_DEVICE_DATA": "1", "MI355X_CUTMIX": "0.5",
           "MI355X_LABEL_SMOOTH": "0.1"}
    r = _run([sys.executable, "cifar_example.py"],
             dict(KNOBS, **METER, **mix, MI355X_CKPT=str(ckpt)))
    _metered(r, ckpt)
    # the end-of-run line is read from the meter: the mean of the losses
    # the loop handed it
    head = ("soft-target loss: label_smoothing=0.1 cutmix=0.5 mixup=0, "
            "mean over the run ")
    line = [l for l in r.stdout.splitlines() if l.startswith(head)]
    assert len(line) == 1, r.stdout[-2000:]
    mean = float(line[0][len(head):])
    assert math.isfinite(mean) and mean > 0


def test_ddp_script_with_the_meter(tmp_path):
    ckpt = tmp_path / "net_ddp.pth"
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
              "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29747", "cifar_example_ddp.py"],
             dict(KNOBS, **METER, MI355X_LABEL_SMOOTH="0.1",
                  MI355X_CKPT=str(ckpt)), timeout=600)
    _metered(r, ckpt)
    assert "soft-target loss: label_smoothing=0.1 " in r.stdout


def test_without_the_knob_nothing_new_is_printed(tmp_path):
    ckpt = tmp_path / "net.pth"
    r = _run([sys.executable, "cifar_example.py"],
             dict(KNOBS, MI355X_CKPT=str(ckpt)))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert _count(ACC, lines) == 1
    assert "Test loss" not in r.stdout and "Per-class" not in r.stdout
    assert ckpt.exists()

"""cifar_example.py trains end to end on the CPU with MI355X_OPTIM=lamb (the
plain-torch twin of ops.lamb_step) and reports the optimizer it built."""

import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_serial_script_with_lamb(tmp_path):
    ckpt = tmp_path / "net.pth"
    env = dict(os.environ, MI355X_SYNTHETIC="1", MI355X_STEPS="3",
               MI355X_EPOCHS="1", MI355X_BATCH="8", MI355X_OPTIM="lamb",
               MI355X_WD="5e-4", MI355X_BETA2="0.99", MI355X_CLIP_NORM="0.5",
               MI355X_CKPT=str(ckpt))
    r = subprocess.run([sys.executable, "cifar_example.py"], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("optimizer: LAMB lr=0.001 betas=(0.9, 0.99) eps=1e-08 "
            "weight_decay=0.0005") in r.stdout.splitlines(), r.stdout[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert ckpt.exists()

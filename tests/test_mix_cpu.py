"""CutMix / Mixup and the soft-target loss on the CPU: the numpy twin of the
draws against a plain Python loop, the CPU pair builder against a float32
loop over the existing gather_augment, the soft loss against torch, the
loader's off case, and both training scripts with the new switches."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.data import (MIX_CUT, MIX_NONE, MIX_UP, Augment, DeviceLoader,
                         SyntheticImageDataset, mix_params)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9

# the (seed, epoch) of the every-mode case below, chosen on the CPU so that
# its assertions hold; the GPU tests mix with the same pair
SEED, EPOCH = 3, 1


def _mix32(h):
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def _loop_params(seed, epoch, i, H, W, cutmix, mixup):
    """One sample's draw in plain Python integers: (mode, box, keep, u,
    unclipped box)."""
    key = _mix32(((seed & M32) * GOLDEN + (epoch & M32)) & M32)
    h = _mix32(i ^ key)
    h2 = _mix32((h + GOLDEN) & M32)
    h3 = _mix32((h2 + GOLDEN) & M32)
    h4 = _mix32((h3 + GOLDEN) & M32)
    tc, tm = round(cutmix * 65536), round(mixup * 65536)
    r, u = h3 & 0xFFFF, h3 >> 16
    mode = MIX_CUT if r < tc else MIX_UP if r < tc + tm else MIX_NONE
    ch = math.isqrt((H * H * (65536 - u)) >> 16)
    cw = math.isqrt((W * W * (65536 - u)) >> 16)
    cy, cx = ((h4 & 0xFFFF) * H) >> 16, ((h4 >> 16) * W) >> 16
    raw = (cy - ch // 2, cy - ch // 2 + ch, cx - cw // 2, cx - cw // 2 + cw)
    box = (max(raw[0], 0), min(raw[1], H), max(raw[2], 0), min(raw[3], W))
    keep = H * W - (box[1] - box[0]) * (box[3] - box[2])
    return mode, box, keep, u, raw


@pytest.mark.parametrize("H,W", [(5, 7), (32, 32), (7, 5), (224, 224),
                                 (1, 1)])
def test_mix_params_against_python_loop(H, W):
    idx = list(range(40)) + [49999, 2 ** 31 - 1, 0xFFFFFFFF]
    for seed, epoch in [(0, 0), (SEED, EPOCH), (2 ** 40 + 5, 7)]:
        mode, box, lam = mix_params(seed, epoch, idx, H, W, 0.4, 0.4)
        assert mode.dtype == torch.int64 and box.shape == (len(idx), 4)
        assert lam.dtype == torch.float32
        for k, i in enumerate(idx):
            m, b, keep, u, _ = _loop_params(seed, epoch, i, H, W, 0.4, 0.4)
            assert int(mode[k]) == m
            if m == MIX_CUT:
                y0, y1, x0, x1 = box[k].tolist()
                assert (y0, y1, x0, x1) == b
                assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
                want = np.float32(keep) * np.float32(1.0 / (H * W))
                assert lam[k].item() == float(want)
            elif m == MIX_UP:
                assert box[k].tolist() == [0, 0, 0, 0]
                assert lam[k].item() == u / 65536
            else:
                assert box[k].tolist() == [0, 0, 0, 0]
                assert lam[k].item() == 1.0
        assert float(lam.min()) >= 0.0 and float(lam.max()) <= 1.0


def test_isqrt_is_exact():
    from mi355x.data import _isqrt

    vals = [0, 1, 2, 3, 4, 8, 9, 15, 16, 17, 224 * 224, 224 * 224 - 1,
            2 ** 31, 2 ** 46 - 1, 2 ** 46, (2 ** 23) ** 2 - 1]
    vals += [k * k + d for k in (3037000499, 94906265, 94906266, 67108864,
                                 12345677) for d in (-1, 0, 1)
             if k * k + d < 2 ** 62]
    got = _isqrt(np.array(vals, dtype=np.int64))
    assert got.tolist() == [math.isqrt(v) for v in vals]


def test_probabilities_are_checked():
    for c, m in [(0.6, 0.5), (-0.1, 0.0), (0.0, 1.5)]:
        with pytest.raises(ValueError):
            mix_params(0, 0, [0], 4, 4, c, m)
        with pytest.raises(ValueError):
            Augment(cutmix=c, mixup=m)
    # the extremes are fine: every sample cutmix, every sample mixup
    assert bool((mix_params(0, 0, range(50), 4, 4, 1.0, 0.0)[0]
                 == MIX_CUT).all())
    assert bool((mix_params(0, 0, range(50), 4, 4, 0.0, 1.0)[0]
                 == MIX_UP).all())
    assert bool((mix_params(0, 0, range(50), 4, 4, 0.0, 0.0)[0]
                 == MIX_NONE).all())


def test_fixed_seed_has_every_mode_and_a_clipped_box():
    """The (SEED, EPOCH) the other tests mix with really mixes: no later
    test can pass by mixing nothing."""
    H = W = 32
    mode, box, lam = mix_params(SEED, EPOCH, range(64), H, W, 0.4, 0.4)
    counts = np.bincount(mode.numpy(), minlength=3)
    assert counts.min() >= 8, counts
    clipped = 0
    for i in range(64):
        m, b, _, _, raw = _loop_params(SEED, EPOCH, i, H, W, 0.4, 0.4)
        if m == MIX_CUT and tuple(raw) != tuple(b):
            clipped += 1
            assert box[i].tolist() == list(b)
    assert clipped >= 1
    # mixing changes the weights: cutmix and mixup rows are not all 1
    assert float(lam[mode != MIX_NONE].min()) < 1.0


def _dataset(n, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8)
    targets = torch.randint(0, 10, (n,), generator=g, dtype=torch.int64)
    scale = torch.tensor([0.017, 0.0081, 0.0123, 0.02][:C])
    shift = torch.tensor([-1.9, -2.1, 0.3, 1.7][:C])
    return data, targets, scale, shift


@pytest.mark.parametrize("N,H,W,C,pad,flip,B", [
    (37, 32, 32, 3, 4, True, 19),
    (6, 5, 7, 3, 2, True, 4),
    (6, 5, 7, 1, 8, True, 1),
    (6, 5, 7, 4, 0, False, 5),
])
@pytest.mark.parametrize("cutmix,mixup", [(1.0, 0.0), (0.0, 1.0), (0.4, 0.4)])
def test_cpu_op_against_numpy_loop(N, H, W, C, pad, flip, B, cutmix, mixup):
    data, targets, scale, shift = _dataset(N, H, W, C)
    g = torch.Generator().manual_seed(B)
    idx = torch.randint(0, N, (B,), generator=g).to(torch.int32)
    if B > 2:
        idx[1] = idx[0]  # a repeated index
    kw = dict(pad=pad, flip=flip, seed=SEED, epoch=EPOCH)
    x, y_a, y_b, lam = ops.gather_augment_mix(
        data, targets, idx, scale, shift, cutmix=cutmix, mixup=mixup, **kw)
    assert x.dtype == torch.float32 and x.shape == (B, H, W, C)
    assert y_a.dtype == torch.int64 and lam.dtype == torch.float32

    # the existing op: normalized A, and raw A through scale 1, shift 0
    norm, want_ya = ops.gather_augment(data, targets, idx, scale, shift, **kw)
    raw, _ = ops.gather_augment(data, targets, idx, torch.ones(C),
                                torch.zeros(C), **kw)
    norm, raw = norm.numpy(), raw.numpy()
    sc, sf = scale.numpy(), shift.numpy()
    mode, box, want_lam = mix_params(SEED, EPOCH, idx, H, W, cutmix, mixup)
    want = np.empty((B, H, W, C), dtype=np.float32)
    want_yb = want_ya.clone()
    for b in range(B):
        p = B - 1 - b
        if mode[b] == MIX_NONE:
            want[b] = norm[b]
            continue
        want_yb[b] = want_ya[p]
        if mode[b] == MIX_CUT:
            y0, y1, x0, x1 = box[b].tolist()
            want[b] = norm[b]
            want[b, y0:y1, x0:x1] = norm[p, y0:y1, x0:x1]
        else:
            w = np.float32(want_lam[b].item())
            v = raw[b] * w + raw[p] * (np.float32(1) - w)
            want[b] = v * sc + sf
    assert torch.equal(x, torch.from_numpy(want))
    assert torch.equal(y_a, want_ya) and torch.equal(y_b, want_yb)
    assert torch.equal(lam, want_lam)


def test_cpu_op_off_equals_gather_augment_and_checks_indices():
    data, targets, scale, shift = _dataset(6, 5, 7, 3)
    idx = torch.tensor([1, 5, 0, 1], dtype=torch.int32)
    kw = dict(pad=2, flip=True, seed=4, epoch=1)
    x, y_a, y_b, lam = ops.gather_augment_mix(data, targets, idx, scale,
                                              shift, **kw)
    want_x, want_y = ops.gather_augment(data, targets, idx, scale, shift, **kw)
    assert torch.equal(x, want_x) and torch.equal(y_a, want_y)
    assert torch.equal(y_b, want_y) and torch.equal(lam, torch.ones(4))
    for bad in ([1, 6, 0], [1, -1, 0]):
        with pytest.raises(IndexError):
            ops.gather_augment_mix(
                data, targets, torch.tensor(bad, dtype=torch.int32), scale,
                shift, cutmix=0.5, mixup=0.5, **kw)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("B,C", [(1, 10), (33, 65), (5, 2)])
def test_cpu_soft_loss_and_gradient_against_torch(B, C, eps, mixed):
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = (torch.randn(B, C, generator=g) * 3).requires_grad_()
    y_a = torch.randint(0, C, (B,), generator=g)
    y_b = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    lam[0] = 1.0
    target = ops.MixTarget(y_a, y_b, lam) if mixed else y_a
    loss = ops.cross_entropy(logits, target, label_smoothing=eps)
    (grad,) = torch.autograd.grad(loss, logits)

    ref_in = logits.detach().clone().requires_grad_()
    rows = F.cross_entropy(ref_in, y_a, label_smoothing=eps, reduction="none")
    if mixed:
        rows = lam * rows + (1 - lam) * F.cross_entropy(
            ref_in, y_b, label_smoothing=eps, reduction="none")
    want = rows.mean()
    (want_grad,) = torch.autograd.grad(want, ref_in)
    # rtol for both; the gradient also gets an absolute floor of one fp32
    # ulp of its own largest entry (a softmax minus a target, |.| <= 1/B):
    # entries that cancel to near zero carry the rounding of that scale
    torch.testing.assert_close(loss, want, rtol=1e-6, atol=0)
    torch.testing.assert_close(
        grad, want_grad, rtol=1e-6,
        atol=float(want_grad.abs().max()) * 2.0 ** -23)


def test_soft_loss_rejects_bad_smoothing():
    with pytest.raises(ValueError):
        ops.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64),
                          label_smoothing=1.5)


def test_mix_target_moves_as_a_whole():
    t = ops.MixTarget(torch.zeros(2, dtype=torch.int64),
                      torch.ones(2, dtype=torch.int64), torch.ones(2))
    moved = t.to("cpu")
    assert isinstance(moved, ops.MixTarget) and torch.equal(moved.y_b, t.y_b)


def test_loader_with_mixing_off_is_the_loader_without_it():
    ds = SyntheticImageDataset(45, seed=3)
    kw = dict(batch_size=16, shuffle=True, seed=2)
    plain = DeviceLoader(ds, augment=Augment(), **kw)
    off = DeviceLoader(ds, augment=Augment(cutmix=0.0, mixup=0.0), **kw)
    assert repr(Augment(cutmix=0.0, mixup=0.0)) == repr(Augment())
    n = 0
    for (px, py), (ox, oy) in zip(plain, off):
        assert torch.is_tensor(oy) and not isinstance(oy, ops.MixTarget)
        assert torch.equal(ox, px) and torch.equal(oy, py)
        n += 1
    assert n == 3


def test_loader_with_mixing_on_yields_mix_targets():
    ds = SyntheticImageDataset(45, seed=3)
    dl = DeviceLoader(ds, batch_size=16, shuffle=True, seed=SEED,
                      augment=Augment(cutmix=0.4, mixup=0.4))
    sizes, mixed = [], 0
    for x, t in dl:
        assert isinstance(t, ops.MixTarget)
        assert x.shape[1:] == (3, 32, 32) and t.lam.shape == (x.shape[0],)
        sizes.append(x.shape[0])
        mixed += int((t.lam < 1).sum())
    assert sizes == [16, 16, 13] and mixed >= 8


# -- the scripts ------------------------------------------------------------

KNOBS = {
    "MI355X_SYNTHETIC": "1",
    "MI355X_STEPS": "3",
    "MI355X_EPOCHS": "1",
    "MI355X_BATCH": "8",
}
MIX = {
    "MI355X_DEVICE_DATA": "1",
    "MI355X_CUTMIX": "0.5",
    "MI355X_LABEL_SMOOTH": "0.1",
}


def _run(cmd, extra_env, timeout=300):
    env = dict(os.environ)
    env.update(extra_env)
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _trains(r, ckpt):
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    head = ("soft-target loss: label_smoothing=0.1 cutmix=0.5 mixup=0, "
            "mean over the run ")
    line = [l for l in r.stdout.splitlines() if l.startswith(head)]
    assert len(line) == 1, r.stdout[-2000:]
    mean = float(line[0][len(head):])
    assert math.isfinite(mean) and mean > 0, line
    assert ckpt.exists()


def test_serial_script_with_cutmix_and_label_smoothing(tmp_path):
    ckpt = tmp_path / "net.pth"
    _trains(_run([sys.executable, "cifar_example.py"],
                 dict(KNOBS, **MIX, MI355X_CKPT=str(ckpt))), ckpt)


def test_ddp_script_with_cutmix_and_label_smoothing(tmp_path):
    ckpt = tmp_path / "net_ddp.pth"
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
              "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29743", "cifar_example_ddp.py"],
             dict(KNOBS, **MIX, MI355X_CKPT=str(ckpt)), timeout=600)
    _trains(r, ckpt)


@pytest.mark.parametrize("script", ["cifar_example.py",
                                    "cifar_example_ddp.py"])
@pytest.mark.parametrize("knob", ["MI355X_CUTMIX", "MI355X_MIXUP"])
def test_mixing_without_device_data_exits_with_the_message(tmp_path, script,
                                                           knob):
    env = dict(KNOBS, MI355X_CKPT=str(tmp_path / "net.pth"))
    env[knob] = "0.5"
    r = _run([sys.executable, script], env)
    assert r.returncode != 0
    assert f"{knob}=0.5 needs MI355X_DEVICE_DATA=1" in r.stderr
    assert "Traceback" not in r.stderr
    assert not (tmp_path / "net.pth").exists()

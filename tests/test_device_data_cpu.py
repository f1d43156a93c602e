"""Device-resident data path, CPU side: the counter-based augmentation draws
(augment_params), the plain-torch gather_augment op against an independent
F.pad/slice/flip construction, and DeviceLoader against DataLoader."""

import math
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.data import (CIFAR10, Augment, DataLoader, DeviceLoader,
                         DistributedSampler, SyntheticImageDataset,
                         augment_params)
from mi355x.models.layers import to_model_layout


# ---------------------------------------------------------------------------
# augment_params
# ---------------------------------------------------------------------------

def _sd(n, p):
    return math.sqrt(n * p * (1 - p))


def test_augment_params_statistics():
    n, pad = 65536, 4
    dy, dx, f = augment_params(1234, 3, torch.arange(n), pad, True)
    k = 2 * pad + 1
    assert int(dy.min()) >= 0 and int(dy.max()) <= 2 * pad
    assert int(dx.min()) >= 0 and int(dx.max()) <= 2 * pad
    assert set(f.tolist()) <= {0, 1}
    for name, d in (("dy", dy), ("dx", dx)):
        cnt = torch.bincount(d, minlength=k)
        assert cnt.numel() == k
        dev = (cnt - n / k).abs().max().item() / _sd(n, 1 / k)
        print(f"{name}: worst cell {dev:.2f} sd")
        assert dev <= 4.0
    dev = abs(int(f.sum()) - n / 2) / _sd(n, 0.5)
    print(f"flip: {dev:.2f} sd")
    assert dev <= 4.0
    cells = k * k * 2
    assert cells == 162
    joint = torch.bincount((dy * k + dx) * 2 + f, minlength=cells)
    dev = (joint - n / cells).abs().max().item() / _sd(n, 1 / cells)
    print(f"joint: worst cell {dev:.2f} sd")
    assert dev <= 4.5


def test_augment_params_basic_properties():
    idx = torch.arange(4096)
    a = augment_params(7, 2, idx, 4, True)
    b = augment_params(7, 2, idx, 4, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for t in augment_params(7, 2, idx, 0, False):
        assert t.dtype == torch.int64 and not t.any()
    c = augment_params(7, 3, idx, 4, True)
    changed = (a[0] != c[0]) | (a[1] != c[1]) | (a[2] != c[2])
    assert changed.float().mean().item() > 0.95  # expectation 1-1/162
    # keyed on the index value, not its position
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(0))
    p = augment_params(7, 2, idx[perm], 4, True)
    for u, v in zip(a, p):
        assert torch.equal(u[perm], v)


# ---------------------------------------------------------------------------
# CPU op vs an independent construction
# ---------------------------------------------------------------------------

def _dataset(n, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8)
    targets = torch.randint(0, 10, (n,), generator=g, dtype=torch.int64)
    scale = torch.tensor([0.017, 0.0081, 0.0123, 0.02][:C])
    shift = torch.tensor([-1.9, -2.1, 0.3, 1.7][:C])
    return data, targets, scale, shift


def _expected(data, idx, scale, shift, pad, flip, seed, epoch):
    """pad the uint8 image -> slice at (dy,dx) -> flip -> normalize"""
    _, H, W, C = data.shape
    dy, dx, f = augment_params(seed, epoch, idx, pad, flip)
    out = []
    for b, i in enumerate(idx.tolist()):
        img = data[i].permute(2, 0, 1)                       # CHW uint8
        img = F.pad(img, (pad, pad, pad, pad), value=0)
        y0, x0 = int(dy[b]), int(dx[b])
        img = img[:, y0:y0 + H, x0:x0 + W]
        if int(f[b]):
            img = torch.flip(img, dims=[2])
        out.append(img.permute(1, 2, 0).to(torch.float32) * scale + shift)
    return torch.stack(out)


@pytest.mark.parametrize("H,W,C,pad", [
    (32, 32, 3, 4),   # the CIFAR case
    (5, 7, 3, 2),     # non-square
    (5, 7, 1, 8),     # pad >= W: all-padding crops occur
    (5, 7, 3, 0),     # no crop
])
def test_cpu_op_vs_pad_slice_flip(H, W, C, pad):
    n = 37
    data, targets, scale, shift = _dataset(n, H, W, C)
    idx = torch.tensor([0, n - 1, 5, 5, 17, 0, 36, 9, 23, 23, 11, 30, 2],
                       dtype=torch.int32)
    all_padding = 0
    for epoch in range(4):
        x, y = ops.gather_augment(data, targets, idx, scale, shift, pad=pad,
                                  flip=True, seed=11, epoch=epoch)
        want = _expected(data, idx, scale, shift, pad, True, 11, epoch)
        assert x.dtype == torch.float32 and x.shape == (len(idx), H, W, C)
        assert torch.equal(x, want)
        assert torch.equal(y, targets[idx.long()])
        # padded pixels equal shift[c]
        dy, dx, _ = augment_params(11, epoch, idx, pad, True)
        for b in range(len(idx)):
            oy, ox = int(dy[b]) - pad, int(dx[b]) - pad
            if oy <= -H or oy >= H or ox <= -W or ox >= W:
                all_padding += 1
                assert torch.equal(x[b], shift.expand(H, W, C))
            if oy < 0:
                k = min(-oy, H)
                assert torch.equal(x[b, :k], shift.expand(k, W, C))
    if pad >= W:
        assert all_padding > 0


def test_cpu_op_eval_path_is_gather_normalize():
    data, targets, scale, shift = _dataset(9, 5, 7, 3)
    idx = torch.tensor([8, 0, 3], dtype=torch.int32)
    x, y = ops.gather_augment(data, targets, idx, scale, shift)
    assert torch.equal(x, data[idx.long()].float() * scale + shift)
    assert torch.equal(y, targets[idx.long()])


def test_index_keying_across_batches():
    data, targets, scale, shift = _dataset(37, 32, 32, 3)
    kw = dict(pad=4, flip=True, seed=5, epoch=2)
    a = torch.tensor([3, 20, 7, 36], dtype=torch.int32)
    b = torch.tensor([36, 1, 3, 3, 7], dtype=torch.int32)
    xa, _ = ops.gather_augment(data, targets, a, scale, shift, **kw)
    xb, _ = ops.gather_augment(data, targets, b, scale, shift, **kw)
    assert torch.equal(xa[0], xb[2]) and torch.equal(xa[0], xb[3])  # 3
    assert torch.equal(xa[2], xb[4])                                # 7
    assert torch.equal(xa[3], xb[0])                                # 36
    assert not torch.equal(xa[0], xa[1])


# ---------------------------------------------------------------------------
# DeviceLoader
# ---------------------------------------------------------------------------

def _write_fake_cifar(root):
    base = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(base, exist_ok=True)
    rng = np.random.RandomState(0)
    for name, n in [("data_batch_1", 20), ("test_batch", 10)]:
        d = {b"data": rng.randint(0, 256, (n, 3072), dtype=np.uint8),
             b"labels": [int(v) for v in rng.randint(0, 10, n)]}
        with open(os.path.join(base, name), "wb") as f:
            pickle.dump(d, f)
    for i in range(2, 6):
        d = {b"data": rng.randint(0, 256, (5, 3072), dtype=np.uint8),
             b"labels": [0, 1, 2, 3, 4]}
        with open(os.path.join(base, f"data_batch_{i}"), "wb") as f:
            pickle.dump(d, f)


def test_normalize_constants_match_reader():
    u8 = np.arange(256, dtype=np.uint8)
    reader = torch.from_numpy(u8.astype(np.float32) * (2.0 / 255.0) - 1.0)
    s = torch.from_numpy(np.float32(1.0 / (255.0 * 0.5)).reshape(1))
    ours = torch.from_numpy(u8).float() * s + torch.tensor([-1.0])
    assert torch.equal(reader, ours)


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_device_loader_equals_dataloader_on_cifar(tmp_path, shuffle,
                                                  drop_last):
    _write_fake_cifar(str(tmp_path))
    ds = CIFAR10(str(tmp_path), train=True)
    assert ds.data_u8.shape == (40, 32, 32, 3)
    assert ds.data_u8.dtype == torch.uint8 and ds.data_u8.is_contiguous()
    kw = dict(batch_size=12, shuffle=shuffle, drop_last=drop_last, seed=3)
    ref, dev = DataLoader(ds, **kw), DeviceLoader(ds, augment=None, **kw)
    assert len(dev) == len(ref) == (3 if drop_last else 4)
    for _ in range(2):  # the per-epoch reshuffle matches too
        rb, db = list(ref), list(dev)
        assert len(rb) == len(db) == len(ref)
        for (rx, ry), (dx, dy) in zip(rb, db):
            assert dx.dtype == torch.float32 and dx.shape == rx.shape
            assert torch.equal(dx, rx)   # bit-equal fp32
            assert torch.equal(dy, ry)


def test_device_loader_synthetic_quantization_gap():
    ds = SyntheticImageDataset(50, seed=4)
    before = ds.data.clone()
    tbefore = ds.targets.clone()
    again = SyntheticImageDataset(50, seed=4)
    u8 = ds.data_u8
    assert u8.shape == (50, 32, 32, 3) and u8.dtype == torch.uint8
    assert ds.data_u8 is u8  # derived once
    assert torch.equal(ds.data, before) and torch.equal(ds.data, again.data)
    assert torch.equal(ds.targets, tbefore)
    for (rx, ry), (dx, dy) in zip(DataLoader(ds, batch_size=16),
                                  DeviceLoader(ds, batch_size=16)):
        gap = (dx - rx).abs().max().item()
        assert gap <= 1 / 255 + 1e-6
        assert torch.equal(dy, ry)


def test_zero_copy_through_to_model_layout():
    ds = SyntheticImageDataset(10, seed=0)
    for x, _ in DeviceLoader(ds, batch_size=4, augment=Augment()):
        assert x.shape[1:] == (3, 32, 32)
        assert x.permute(0, 2, 3, 1).is_contiguous()
        assert to_model_layout(x).data_ptr() == x.data_ptr()


def _by_index(ds, world, rank, epoch, batch):
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank,
                                 shuffle=True, seed=0)
    sampler.set_epoch(epoch)
    dl = DeviceLoader(ds, batch_size=batch, sampler=sampler,
                      augment=Augment(), seed=9)
    order = list(iter(sampler))
    out, k = {}, 0
    for x, y in dl:
        for b in range(x.shape[0]):
            i = order[k]
            k += 1
            assert int(y[b]) == int(ds.targets[i])
            if i in out:  # duplicated by the sampler's padding
                assert torch.equal(out[i], x[b])
            out[i] = x[b]
    assert k == len(order)
    return out


def test_rank_independence_and_set_epoch():
    ds = SyntheticImageDataset(37, seed=1)
    w1 = _by_index(ds, 1, 0, 0, 8)
    assert sorted(w1) == list(range(37))
    w2 = {}
    for rank in range(2):
        part = _by_index(ds, 2, rank, 0, 5)
        for i, img in part.items():
            assert torch.equal(img, w1[i])
        w2.update(part)
    assert sorted(w2) == list(range(37))
    e1 = _by_index(ds, 1, 0, 1, 8)
    differ = sum(not torch.equal(e1[i], w1[i]) for i in range(37))
    assert differ > 0.8 * 37  # expectation 1-1/162 per image


def test_loader_epoch_counter_drives_augmentation_without_sampler():
    ds = SyntheticImageDataset(8, seed=1)
    dl = DeviceLoader(ds, batch_size=8, augment=Augment())
    (x0, _), = list(dl)
    (x1, _), = list(dl)
    assert not torch.equal(x0, x1)
    want, _ = ops.gather_augment(ds.data_u8, ds.targets,
                                 torch.arange(8, dtype=torch.int32),
                                 dl.scale, dl.shift, pad=4, flip=True,
                                 seed=0, epoch=1)
    assert torch.equal(x1.permute(0, 2, 3, 1), want)


def test_out_of_range_index_raises_on_host():
    ds = SyntheticImageDataset(10, seed=0)
    for bad in ([0, 3, 10], [2, -1]):
        dl = DeviceLoader(ds, batch_size=2, sampler=bad)
        with pytest.raises(IndexError):
            next(iter(dl))


def test_mean_std_are_parameters():
    ds = SyntheticImageDataset(6, seed=2)
    mean, std = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)
    (x, _), = list(DeviceLoader(ds, batch_size=6, mean=mean, std=std))
    want = (ds.data_u8.double() / 255 - torch.tensor(mean, dtype=torch.float64)) \
        / torch.tensor(std, dtype=torch.float64)
    torch.testing.assert_close(x.permute(0, 2, 3, 1).double(), want,
                               rtol=0, atol=2e-6)
    with pytest.raises(ValueError):
        DeviceLoader(ds, batch_size=2, mean=(0.5,), std=(0.5,))


# ---------------------------------------------------------------------------
# scripts: MI355X_DEVICE_DATA / MI355X_AUGMENT
# ---------------------------------------------------------------------------

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_script(script, tmp_path, **extra):
    import subprocess
    import sys

    env = dict(os.environ)
    env.update({"MI355X_SYNTHETIC": "1", "MI355X_STEPS": "3",
                "MI355X_EPOCHS": "1", "MI355X_BATCH": "8",
                "MI355X_CKPT": str(tmp_path / "net.pth"),
                "MASTER_PORT": "29631"})
    env.update(extra)
    return subprocess.run([sys.executable, script], cwd=REPO, env=env,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("script", ["cifar_example.py",
                                    "cifar_example_ddp.py"])
def test_scripts_run_with_device_data_and_augment(script, tmp_path):
    r = _run_script(script, tmp_path, MI355X_DEVICE_DATA="1",
                    MI355X_AUGMENT="1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (3 steps" in r.stdout
    assert "Accuracy of the network" in r.stdout
    assert (tmp_path / "net.pth").exists()


def test_script_refuses_augment_without_device_data(tmp_path):
    r = _run_script("cifar_example.py", tmp_path, MI355X_AUGMENT="1")
    assert r.returncode != 0
    assert "MI355X_DEVICE_DATA" in r.stderr

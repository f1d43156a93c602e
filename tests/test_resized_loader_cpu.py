"""Random resized crop + bilinear resize on the CPU: the draws
(rrc_params), the integer twin of gather_resize_kernel against a float64
F.interpolate reference, the identity with the pad-crop path, DeviceLoader
and the scripts."""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x.data import (Augment, DeviceLoader, SyntheticImageDataset,
                         rrc_params)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO = (3 / 4, 4 / 3)


def _dataset(n, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8)
    targets = torch.randint(0, 10, (n,), generator=g, dtype=torch.int64)
    scale = torch.tensor([0.017, 0.0081, 0.0123, 0.02][:C])
    shift = torch.tensor([-1.9, -2.1, 0.3, 1.7][:C])
    return data, targets, scale, shift


def _reference(data, idx, size, box, norm_scale, shift):
    """Cut each sample's box, resample it in float64, flip, normalize."""
    out = []
    for i, y0, x0, ch, cw, f in zip(idx.tolist(), *(t.tolist() for t in box)):
        crop = data[i, y0:y0 + ch, x0:x0 + cw].double().permute(2, 0, 1)
        v = F.interpolate(crop[None], size=size, mode="bilinear",
                          align_corners=False)[0].permute(1, 2, 0)
        out.append(v.flip(1) if f else v)
    return torch.stack(out) * norm_scale.double() + shift.double()


@pytest.mark.parametrize("H,W,C,size,scale", [
    (32, 32, 3, (224, 224), (0.08, 1.0)),
    (32, 32, 3, (37, 53), (0.08, 1.0)),
    (40, 24, 1, (16, 16), (0.08, 1.0)),    # downsample
    (9, 9, 4, (50, 50), (0.005, 0.2)),     # boxes down to 1x1
    (32, 32, 3, (224, 224), None),         # evaluation: the whole image
    (40, 24, 1, (16, 16), None),
])
def test_twin_against_float64_interpolate(H, W, C, size, scale):
    """The twin differs from exact bilinear resampling only in its weights:
    fy and fx are the fractions truncated to 8 bits, so each is below the
    exact weight by less than 2^-8, and moving a weight by d between two
    taps moves the value by d * |tap difference| <= d * 255 raw levels. Two
    weights: below 2 * 255 * 2^-8 raw levels, times |scale[c]|. On top, the
    twin's normalize rounds twice in fp32 (the product, then the sum), each
    by at most 2^-24 of a magnitude below 255*|scale[c]| + |shift[c]|."""
    data, targets, ns, shift = _dataset(11, H, W, C)
    idx = torch.tensor([0, 10, 3, 3, 7, 1, 9, 5], dtype=torch.int32)
    x, y = ops.gather_augment(data, targets, idx, ns, shift, flip=True,
                              seed=5, epoch=2, size=size, scale=scale,
                              ratio=RATIO)
    assert x.dtype == torch.float32 and x.shape == (8, *size, C)
    assert torch.equal(y, targets[idx.long()])
    if scale is None:
        z = torch.zeros(8, dtype=torch.int64)
        box = (z, z, z + H, z + W, z)
    else:
        box = rrc_params(5, 2, idx, H, W, scale, RATIO)
    want = _reference(data, idx, size, box, ns, shift)
    bound = (2 * 255 / 256 * ns.abs().double()
             + 2.0 ** -23 * (255 * ns.abs() + shift.abs()).double())
    err = (x.double() - want).abs().amax(dim=(0, 1, 2))
    print("max error per channel", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all()


def test_identity_with_the_pad_crop_path():
    data, targets, ns, shift = _dataset(9, 12, 12, 3)
    idx = torch.arange(9, dtype=torch.int32)
    kw = dict(flip=True, seed=3, epoch=4)
    x, y = ops.gather_augment(data, targets, idx, ns, shift, size=12,
                              scale=(1, 1), ratio=(1, 1), **kw)
    want_x, want_y = ops.gather_augment(data, targets, idx, ns, shift, pad=0,
                                        **kw)
    assert torch.equal(x, want_x) and torch.equal(y, want_y)


@pytest.mark.parametrize("H,W", [(32, 32), (40, 24), (9, 9), (1, 7)])
def test_draw_properties(H, W):
    idx = torch.arange(400)
    y0, x0, ch, cw, f = rrc_params(1, 0, idx, H, W, (0.02, 1.0), RATIO)
    assert (ch >= 1).all() and (cw >= 1).all() and (y0 >= 0).all()
    assert (x0 >= 0).all() and (y0 + ch <= H).all() and (x0 + cw <= W).all()
    assert set(f.tolist()) <= {0, 1}
    # keyed on the dataset index: the same box in any batch
    sub = torch.tensor([399, 7, 7, 120])
    for a, b in zip(rrc_params(1, 0, sub, H, W, (0.02, 1.0), RATIO),
                    (y0, x0, ch, cw, f)):
        assert torch.equal(a, b[sub])
    if H * W > 1:
        other = rrc_params(1, 1, idx, H, W, (0.02, 1.0), RATIO)
        assert any(not torch.equal(a, b)
                   for a, b in zip(other, (y0, x0, ch, cw, f)))
    # full area at ratio 1 is the whole of a square image
    y0, x0, ch, cw, _ = rrc_params(1, 0, idx, H, H, (1, 1), (1, 1))
    assert not y0.any() and not x0.any()
    assert (ch == H).all() and (cw == H).all()


@pytest.mark.parametrize("augment", [None, Augment(scale=(0.08, 1.0))])
@pytest.mark.parametrize("size,want", [(48, (48, 48)), ((20, 36), (20, 36))])
def test_device_loader_size(augment, size, want):
    ds = SyntheticImageDataset(10, seed=3)
    dl = DeviceLoader(ds, batch_size=4, augment=augment, size=size, seed=2)
    shapes = []
    for x, y in dl:
        assert x.shape[1:] == (3, *want) and y.shape == (x.shape[0],)
        assert x.permute(0, 2, 3, 1).is_contiguous()
        shapes.append(x.shape[0])
    assert shapes == [4, 4, 2]
    idx = torch.arange(4, dtype=torch.int32)
    kw = dict(scale=augment.scale, flip=True) if augment else {}
    ref, _ = ops.gather_augment(ds.data_u8, ds.targets, idx, dl.scale,
                                dl.shift, seed=2, epoch=0, size=size, **kw)
    first = next(iter(DeviceLoader(ds, batch_size=4, augment=augment,
                                   size=size, seed=2)))[0]
    assert torch.equal(first.permute(0, 2, 3, 1), ref)


def test_rrc_without_size_keeps_the_source_size():
    ds = SyntheticImageDataset(6, seed=3, size=20)
    x, _ = next(iter(DeviceLoader(ds, batch_size=6,
                                  augment=Augment(scale=(0.3, 1.0)))))
    assert x.shape == (6, 3, 20, 20)


@pytest.mark.parametrize("make,needle", [
    (lambda ds: Augment(scale=(0.0, 1.0)), "0.0"),
    (lambda ds: Augment(scale=(0.5, 0.25)), "0.25"),
    (lambda ds: Augment(scale=(0.5, 1.5)), "1.5"),
    (lambda ds: Augment(scale=(0.5, 1.0), ratio=(0.0, 1.0)), "0.0"),
    (lambda ds: Augment(scale=(0.5, 1.0), ratio=(2.0, 1.0)), "2.0"),
    (lambda ds: Augment(scale=(0.5, 1.0), cutmix=0.5), "does not resample"),
    (lambda ds: DeviceLoader(ds, size=64, augment=Augment(mixup=0.25)),
     "does not resample"),
    (lambda ds: DeviceLoader(ds, size=64, augment=Augment(pad=4)), "pad=4"),
    (lambda ds: DeviceLoader(ds, size=5000), "5000"),
    (lambda ds: DeviceLoader(ds, size=(0, 8)), "(0, 8)"),
    (lambda ds: ops.gather_augment(ds.data_u8, ds.targets,
                                   torch.zeros(1, dtype=torch.int32),
                                   torch.ones(3), torch.zeros(3),
                                   scale=(0.5, 1.0)), "(0.5, 1.0)"),
])
def test_value_errors_name_the_value(make, needle):
    with pytest.raises(ValueError) as e:
        make(SyntheticImageDataset(4, seed=0))
    assert needle in str(e.value)
    assert "pad" not in repr(Augment(scale=(0.08, 1.0)))


def test_script_trains_at_another_size(tmp_path):
    """MI355X_LABEL_SMOOTH is there because the script prints no loss
    within two steps otherwise (its progress line comes every 2000)."""
    env = dict(os.environ, MI355X_SYNTHETIC="1", MI355X_DEVICE_DATA="1",
               MI355X_AUGMENT="1", MI355X_SIZE="64", MI355X_MODEL="resnet18",
               MI355X_STEPS="2", MI355X_LABEL_SMOOTH="0.1",
               MI355X_CKPT=str(tmp_path / "net.pth"))
    r = subprocess.run([sys.executable, "cifar_example.py"], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Finished Training (2 steps" in r.stdout
    loss = float(r.stdout.split("mean over the run")[1].split()[0])
    assert loss == loss and abs(loss) != float("inf")
    r = subprocess.run([sys.executable, "cifar_example.py"], cwd=REPO,
                       env=dict(env, MI355X_DEVICE_DATA="0",
                                MI355X_AUGMENT="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "MI355X_SIZE needs" in r.stderr

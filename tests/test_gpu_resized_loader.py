"""gather_resize_kernel on the GPU: bit-equal to the CPU twin rounded to the
compute dtype, tied to the pad-crop kernel by the identity case, and feeding
the 224-px ViT through DeviceLoader."""

import pytest
import torch

import mi355x.ops as ops
from mi355x import amp, optim
from mi355x.data import (Augment, DeviceLoader, SyntheticImageDataset,
                         rrc_params)
from mi355x.models import build_model
from mi355x.parallel.flat import FlatState
from test_resized_loader_cpu import RATIO, _dataset

pytestmark = pytest.mark.gpu


@pytest.fixture
def compute_dtype(request):
    prev = amp.get_compute_dtype()
    amp.set_compute_dtype(request.param)
    yield request.param
    amp.set_compute_dtype(prev)


@pytest.mark.parametrize("compute_dtype,N,H,W,C,size,scale,B,bad", [
    (torch.bfloat16, 37, 32, 32, 3, 224, (0.08, 1.0), 5, True),
    (torch.bfloat16, 37, 32, 32, 3, (37, 53), (0.08, 1.0), 4, False),  # 159
    (torch.bfloat16, 6, 40, 24, 1, 16, (0.08, 1.0), 4, False),
    (torch.bfloat16, 6, 9, 9, 4, 224, (0.005, 0.2), 16, False),  # 1x1 boxes
    (torch.float16, 37, 32, 32, 3, 224, (0.08, 1.0), 3, False),
    (torch.bfloat16, 37, 32, 32, 3, 96, (0.08, 1.0), 40, False),  # 6 bands
    (torch.bfloat16, 37, 32, 32, 3, 224, None, 4, False),  # evaluation
], indirect=["compute_dtype"])
def test_kernel_bit_exact_vs_cpu_twin(compute_dtype, N, H, W, C, size, scale,
                                      B, bad):
    data, targets, ns, shift = _dataset(N, H, W, C)
    g = torch.Generator().manual_seed(B)
    idx = torch.randint(0, N, (B,), generator=g).to(torch.int32)
    idx[0], idx[-1] = 0, N - 1
    if bad:
        idx[2] = N  # outside the dataset: reads nothing
    good = idx < N
    if C == 4:
        _, _, ch, cw, _ = rrc_params(21, 1, idx, H, W, scale, RATIO)
        assert ((ch == 1) & (cw == 1)).any()
    kw = dict(flip=True, seed=21, epoch=1, size=size, scale=scale,
              ratio=RATIO)
    want_x, want_y = ops.gather_augment(data, targets, idx[good], ns, shift,
                                        **kw)
    dev = [t.cuda() for t in (data, targets, idx, ns, shift)]
    x, y = ops.gather_augment(*dev, **kw)
    x2, y2 = ops.gather_augment(*dev, **kw)
    assert x.dtype == compute_dtype and x.is_contiguous()
    assert x.shape == (B, *want_x.shape[1:])
    assert torch.equal(x, x2) and torch.equal(y, y2)
    assert torch.equal(x[good.cuda()].cpu(), want_x.to(compute_dtype))
    assert torch.equal(y[good.cuda()].cpu(), want_y)
    if bad:
        assert int(y[2]) == -1
        assert torch.equal(x[2].cpu(),
                           shift.to(compute_dtype).expand(*x.shape[1:]))


def test_identity_with_the_pad_crop_kernel():
    data, targets, ns, shift = _dataset(9, 12, 12, 3)
    idx = torch.arange(9, dtype=torch.int32)
    dev = [t.cuda() for t in (data, targets, idx, ns, shift)]
    kw = dict(flip=True, seed=3, epoch=4)
    x, y = ops.gather_augment(*dev, size=12, scale=(1, 1), ratio=(1, 1), **kw)
    want_x, want_y = ops.gather_augment(*dev, pad=0, **kw)
    assert torch.equal(x, want_x) and torch.equal(y, want_y)


def test_domain_errors_name_the_value():
    data, targets, ns, shift = _dataset(2, 2, 2049, 4)  # W*C = 8196 bytes
    idx = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="8196"):
        ops.gather_augment(*(t.cuda() for t in (data, targets, idx, ns,
                                                shift)), size=8)


def test_vit_s8_trains_from_the_resized_loader():
    torch.manual_seed(0)
    dev = torch.device("cuda")
    ds = SyntheticImageDataset(64, seed=7)
    dl = DeviceLoader(ds, batch_size=4, shuffle=True, device=dev, size=224,
                      augment=Augment(scale=(0.08, 1.0)))
    net = build_model("vit_s8").to(dev)
    opt = optim.SGD(FlatState(net), lr=0.01, momentum=0.9)
    losses, batches = [], []
    for x, y in dl:
        assert x.shape == (4, 3, 224, 224)
        opt.zero_grad()
        loss = ops.cross_entropy(net(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        batches.append(x)
        if len(losses) == 2:
            break
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert not torch.equal(batches[0], batches[1])

"""Device-resident data path on the GPU: the gather_augment kernel is
bit-exact against the CPU op (same draws, non-contracted mul+add, one
rounding to 16 bits), and DeviceLoader feeds the models end to end."""

import pytest
import torch

import mi355x.ops as ops
from mi355x import amp, optim
from mi355x.data import (Augment, DeviceLoader, DistributedSampler,
                         SyntheticImageDataset)
from mi355x.models import Net, build_model
from mi355x.models.layers import to_model_layout
from mi355x.parallel.flat import FlatState

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture
def compute_dtype(request):
    prev = amp.get_compute_dtype()
    amp.set_compute_dtype(request.param)
    yield request.param
    amp.set_compute_dtype(prev)


def _dataset(n, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8)
    targets = torch.randint(0, 10, (n,), generator=g, dtype=torch.int64)
    scale = torch.tensor([0.017, 0.0081, 0.0123, 0.02][:C])
    shift = torch.tensor([-1.9, -2.1, 0.3, 1.7][:C])
    return data, targets, scale, shift


def _indices(n, B):
    # first and last sample, repeats
    base = [0, n - 1, 2, 2, n - 1, 1, 3, 0]
    g = torch.Generator().manual_seed(B)
    more = torch.randint(0, n, (max(B - len(base), 0),), generator=g).tolist()
    return torch.tensor((base + more)[:B] if B > 1 else [n - 1],
                        dtype=torch.int32)


@pytest.mark.parametrize("compute_dtype", DTYPES, indirect=True)
@pytest.mark.parametrize("N,H,W,C,pad,flip,B", [
    (37, 32, 32, 3, 4, True, 19),   # repeats, first and last index
    (6, 5, 7, 3, 2, True, 4),       # small non-square
    (6, 5, 7, 1, 8, True, 1),       # B=1, 35 elements, all-padding crops
    (6, 5, 7, 4, 0, False, 5),      # C=4, no crop
])
def test_kernel_bit_exact_vs_cpu_op(compute_dtype, N, H, W, C, pad, flip, B):
    data, targets, scale, shift = _dataset(N, H, W, C)
    idx = _indices(N, B)
    dev = [t.cuda() for t in (data, targets, idx, scale, shift)]
    for epoch in range(3):
        kw = dict(pad=pad, flip=flip, seed=21, epoch=epoch)
        want_x, want_y = ops.gather_augment(data, targets, idx, scale, shift,
                                            **kw)
        x, y = ops.gather_augment(*dev, **kw)
        assert x.dtype == compute_dtype and x.shape == (B, H, W, C)
        assert x.is_contiguous() and y.dtype == torch.int64
        assert torch.equal(x.cpu(), want_x.to(compute_dtype))
        assert torch.equal(y.cpu(), want_y)


def test_kernel_reads_nothing_for_out_of_range_index():
    """The kernel cannot raise: an index outside [0,N) must not be used as
    an address. It yields an all-padding image and label -1."""
    N, H, W, C = 6, 5, 7, 3
    data, targets, scale, shift = _dataset(N, H, W, C)
    idx = torch.tensor([1, N, -1, 0], dtype=torch.int32)
    good = torch.tensor([1, 0], dtype=torch.int32)
    kw = dict(pad=2, flip=True, seed=4, epoch=1)
    x, y = ops.gather_augment(*(t.cuda() for t in (data, targets, idx, scale,
                                                   shift)), **kw)
    want_x, want_y = ops.gather_augment(data, targets, good, scale, shift,
                                        **kw)
    dt = ops.compute_dtype()
    assert torch.equal(x[[0, 3]].cpu(), want_x.to(dt))
    pad_img = shift.to(dt).expand(H, W, C)
    assert torch.equal(x[1].cpu(), pad_img) and torch.equal(x[2].cpu(), pad_img)
    assert y.cpu().tolist() == [int(want_y[0]), -1, -1, int(want_y[1])]
    with pytest.raises(IndexError):
        ops.gather_augment(data, targets, idx, scale, shift, **kw)


@pytest.mark.parametrize("compute_dtype", DTYPES, indirect=True)
def test_device_loader_cifar_mean_std_bit_equal(compute_dtype):
    ds = SyntheticImageDataset(45, seed=3)
    kw = dict(batch_size=16, shuffle=True, augment=Augment(), seed=2,
              mean=(0.4914, 0.4822, 0.4465), std=(0.2470, 0.2435, 0.2616))
    cpu, gpu = DeviceLoader(ds, **kw), DeviceLoader(ds, device="cuda", **kw)
    batches = 0
    for (cx, cy), (gx, gy) in zip(cpu, gpu):
        assert gx.is_cuda and gx.dtype == compute_dtype
        assert torch.equal(gx.cpu(), cx.to(compute_dtype))
        assert torch.equal(gy.cpu(), cy)
        batches += 1
    assert batches == 3


def test_device_loader_on_cuda_epochs_layout_zero_copy():
    ds = SyntheticImageDataset(100, seed=5)
    sampler = DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True)
    dl = DeviceLoader(ds, batch_size=32, sampler=sampler, device="cuda",
                      augment=Augment())
    assert len(dl) == 4
    first = None
    for epoch in range(2):
        sampler.set_epoch(epoch)
        order = list(iter(sampler))
        sizes, labels = [], []
        for x, y in dl:
            assert x.is_cuda and x.dtype == ops.compute_dtype()
            assert x.shape[1:] == (3, 32, 32)
            assert x.permute(0, 2, 3, 1).is_contiguous()
            assert to_model_layout(x).data_ptr() == x.data_ptr()
            sizes.append(x.shape[0])
            labels.append(y.cpu())
        assert sizes == [32, 32, 32, 4]
        # index coverage equals the sampler's: labels arrive in its order
        assert sorted(order) == list(range(100))
        assert torch.equal(torch.cat(labels), ds.targets[order])
        if first is None:
            first = order
    assert first != order  # set_epoch reshuffled


@pytest.mark.parametrize("make", [lambda: build_model("resnet18"), Net],
                         ids=["resnet18", "net"])
def test_models_train_from_device_loader(make):
    torch.manual_seed(0)
    dev = torch.device("cuda")
    ds = SyntheticImageDataset(48, seed=7)
    dl = DeviceLoader(ds, batch_size=16, shuffle=True, device=dev,
                      augment=Augment())
    net = make().to(dev)
    flat = FlatState(net)
    opt = optim.SGD(flat, lr=0.05, momentum=0.9)
    before = flat.flat_param.detach().clone()
    losses = []
    for x, y in dl:
        opt.zero_grad()
        loss = ops.cross_entropy(net(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert len(losses) == 3
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert not torch.equal(flat.flat_param.detach(), before)

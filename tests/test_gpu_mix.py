"""CutMix / Mixup and the soft-target loss on the GPU: gather_mix_kernel is
bit-exact against the CPU op, the soft loss pair is as close to an fp64
oracle as the hard-label pair is (within a factor of two), the default loss
path still is the hard-label pair, and the whole thing trains under fp16
with the device-side scaler and replays from a captured graph."""

import pytest
import torch
import torch.nn.functional as F

import mi355x.ops as ops
from mi355x import amp, optim
from mi355x.data import (MIX_NONE, Augment, DeviceLoader,
                         SyntheticImageDataset, mix_params)
from mi355x.models import Net, build_model
from mi355x.ops import MixTarget, ext
from mi355x.parallel.flat import FlatState

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]

# every mode occurs and a box is clipped under this pair with
# cutmix = mixup = 0.4 (asserted in tests/test_mix_cpu.py)
SEED = 3


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


SHAPES = [
    (37, 32, 32, 3, 4, True, 19),   # odd B: self-paired middle; repeats
    (6, 5, 7, 3, 2, True, 4),       # 105 elements a sample: lanes cross
    (6, 5, 7, 1, 8, True, 1),       # B=1, 35 elements: the sub-8 store tail
    (6, 5, 7, 4, 0, False, 5),      # C=4, no crop
]


@pytest.mark.parametrize("compute_dtype", DTYPES, indirect=True)
@pytest.mark.parametrize("cutmix,mixup", [(1.0, 0.0), (0.0, 1.0), (0.4, 0.4)])
@pytest.mark.parametrize("N,H,W,C,pad,flip,B", SHAPES)
def test_kernel_bit_exact_vs_cpu_op(compute_dtype, N, H, W, C, pad, flip, B,
                                    cutmix, mixup):
    data, targets, scale, shift = _dataset(N, H, W, C)
    idx = _indices(N, B)
    dev = [t.cuda() for t in (data, targets, idx, scale, shift)]
    mixed = 0
    for epoch in range(3):
        kw = dict(pad=pad, flip=flip, cutmix=cutmix, mixup=mixup, seed=SEED,
                  epoch=epoch)
        want = ops.gather_augment_mix(data, targets, idx, scale, shift, **kw)
        x, y_a, y_b, lam = ops.gather_augment_mix(*dev, **kw)
        assert x.dtype == compute_dtype and x.shape == (B, H, W, C)
        assert x.is_contiguous() and y_a.dtype == torch.int64
        assert y_b.dtype == torch.int64 and lam.dtype == torch.float32
        assert torch.equal(x.cpu(), want[0].to(compute_dtype))
        assert torch.equal(y_a.cpu(), want[1])
        assert torch.equal(y_b.cpu(), want[2])
        assert torch.equal(lam.cpu(), want[3])
        mode, _, _ = mix_params(SEED, epoch, idx, H, W, cutmix, mixup)
        mixed += int((mode != MIX_NONE).sum())
    assert mixed >= 1  # the comparison above was of mixed samples


@pytest.mark.parametrize("compute_dtype", DTYPES, indirect=True)
@pytest.mark.parametrize("N,H,W,C,pad,flip,B", SHAPES)
def test_mix_kernel_with_both_off_is_gather_augment(compute_dtype, N, H, W, C,
                                                    pad, flip, B):
    data, targets, scale, shift = _dataset(N, H, W, C)
    dev = [t.cuda() for t in (data, targets, _indices(N, B), scale, shift)]
    kw = dict(pad=pad, flip=flip, seed=21, epoch=1)
    x, y_a, y_b, lam = ops.gather_augment_mix(*dev, cutmix=0.0, mixup=0.0,
                                              **kw)
    want_x, want_y = ops.gather_augment(*dev, **kw)
    assert torch.equal(x, want_x)
    assert torch.equal(y_a, want_y) and torch.equal(y_b, want_y)
    assert torch.equal(lam, torch.ones(B, device="cuda"))


# -- soft loss ----------------------------------------------------------------

LOSS_SHAPES = [(1, 10), (257, 10), (33, 65), (5, 2), (64, 1000)]


def _loss_inputs(B, C, dtype):
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = (torch.randn(B, C, generator=g) * 3).to(dtype)
    y_a = torch.randint(0, C, (B,), generator=g)
    y_b = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    lam[0] = 1.0
    return logits, y_a, y_b, lam


def _oracle(logits16, y_a, y_b, lam, eps):
    """fp64 loss and dlogits from the 16-bit logits upcast (CPU)."""
    z = logits16.double().requires_grad_()
    rows = F.cross_entropy(z, y_a, label_smoothing=eps, reduction="none")
    if y_b is not None:
        lam = lam.double()
        rows = lam * rows + (1 - lam) * F.cross_entropy(
            z, y_b, label_smoothing=eps, reduction="none")
    loss = rows.mean()
    (grad,) = torch.autograd.grad(loss, z)
    return loss.detach(), grad


def _errors(loss, grad, want_loss, want_grad):
    """(relative error of the loss, largest error of dlogits relative to
    the oracle's largest entry)."""
    el = abs(loss.double().item() - want_loss.item()) / abs(want_loss.item())
    eg = ((grad.double().cpu() - want_grad).abs().max()
          / want_grad.abs().max()).item()
    return el, eg


def _run_gpu(logits, target, eps):
    z = logits.cuda().requires_grad_()
    loss = ops.cross_entropy(z, target, label_smoothing=eps)
    (grad,) = torch.autograd.grad(loss, z)
    return loss, grad


@pytest.fixture(scope="module")
def hard_error():
    """Per dtype: the largest (loss, dlogits) error of the existing
    hard-label kernels against the fp64 oracle over LOSS_SHAPES, on the
    logits the soft tests use (target y_a). Computed once."""
    out = {}
    for dtype in DTYPES:
        worst_l = worst_g = 0.0
        for B, C in LOSS_SHAPES:
            logits, y_a, _, _ = _loss_inputs(B, C, dtype)
            loss, grad = _run_gpu(logits, y_a.cuda(), 0.0)
            el, eg = _errors(loss, grad, *_oracle(logits, y_a, None, None, 0.0))
            print(f"hard  {str(dtype):15s} B={B:<4d} C={C:<5d} "
                  f"loss_err={el:.3e} grad_err={eg:.3e}")
            worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
        out[dtype] = (worst_l, worst_g)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", LOSS_SHAPES)
def test_soft_loss_fwd_bwd_against_fp64_oracle(hard_error, B, C, eps, mixed,
                                               dtype):
    """The bound is measured, not chosen: twice the error of the existing
    hard-label kernels against the same fp64 oracle on the same logits
    (largest over LOSS_SHAPES, per dtype), since the soft kernels use the
    same __expf/__logf and one more reduction. Loss: relative error of the
    mean. dlogits: largest error over the oracle's largest entry (the
    16-bit rounding of the output dominates it).

    Measured on an MI355X (hard-label pair, largest over the five shapes):
      bf16  loss 4.29e-08   dlogits 1.96e-03
      fp16  loss 4.66e-08   dlogits 2.44e-04
    and the soft pair's largest over all its cases:
      bf16  loss 3.95e-08   dlogits 2.16e-03
      fp16  loss 5.30e-08   dlogits 2.62e-04
    The loss bound (8.6e-08 / 9.3e-08) is below one fp32 ulp of the loss,
    which is why the soft forward forms each row's loss and the mean over
    rows in double and rounds once: with both in fp32 the (33, 65) bf16
    mix case came out 1.5 ulp off (1.55e-07).
    """
    logits, y_a, y_b, lam = _loss_inputs(B, C, dtype)
    if mixed:
        target = MixTarget(y_a.cuda(), y_b.cuda(), lam.cuda())
        want = _oracle(logits, y_a, y_b, lam, eps)
    else:
        target = y_a.cuda()
        want = _oracle(logits, y_a, None, None, eps)
    if not mixed and eps == 0.0:
        # the default path is the hard pair (its own test below); drive the
        # soft kernels with a plain target directly
        z = logits.cuda()
        loss, lse = ext().cross_entropy_soft_fwd(z, target, None, None, 0.0)
        grad = ext().cross_entropy_soft_bwd(
            z, target, None, None, lse, torch.ones((), device="cuda"), 0.0)
    else:
        loss, grad = _run_gpu(logits, target, eps)
    assert loss.dtype == torch.float32 and grad.dtype == dtype
    el, eg = _errors(loss, grad, *want)
    bound_l, bound_g = (2 * e for e in hard_error[dtype])
    print(f"soft  {str(dtype):15s} B={B:<4d} C={C:<5d} eps={eps} "
          f"mixed={mixed} loss_err={el:.3e} (bound {bound_l:.3e}) "
          f"grad_err={eg:.3e} (bound {bound_g:.3e})")
    assert el <= bound_l
    assert eg <= bound_g


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_path_is_the_hard_label_pair(dtype):
    logits, y_a, _, _ = _loss_inputs(257, 10, dtype)
    z, t = logits.cuda(), y_a.cuda()
    want_loss, lse = ext().cross_entropy_fwd(z, t)
    want_grad = ext().cross_entropy_bwd(z, t, lse,
                                        torch.ones((), device="cuda"))
    for kw in ({}, {"label_smoothing": 0.0}):
        zz = z.clone().requires_grad_()
        loss = ops.cross_entropy(zz, t, **kw)
        assert loss.grad_fn.name().startswith("_CEFn")
        (grad,) = torch.autograd.grad(loss, zz)
        assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)


@pytest.mark.parametrize("slot", ["y_a", "y_b"])
def test_bad_target_in_either_slot_poisons_the_loss(slot):
    logits, y_a, y_b, lam = _loss_inputs(33, 65, torch.bfloat16)
    good = ops.cross_entropy(logits.cuda(),
                             MixTarget(y_a.cuda(), y_b.cuda(), lam.cuda()),
                             label_smoothing=0.1)
    assert torch.isfinite(good)
    (y_a if slot == "y_a" else y_b)[7] = -1
    bad = ops.cross_entropy(logits.cuda(),
                            MixTarget(y_a.cuda(), y_b.cuda(), lam.cuda()),
                            label_smoothing=0.1)
    assert torch.isnan(bad)
    # and a plain target through the soft kernels
    assert torch.isnan(ops.cross_entropy(
        logits.cuda(), torch.full((33,), 65).cuda(), label_smoothing=0.1))


def test_soft_loss_replays_from_a_captured_graph():
    B, C, eps = 33, 65, 0.1
    first = _loss_inputs(B, C, torch.bfloat16)
    g = torch.Generator().manual_seed(99)
    second = ((torch.randn(B, C, generator=g) * 3).to(torch.bfloat16),
              torch.randint(0, C, (B,), generator=g),
              torch.randint(0, C, (B,), generator=g),
              torch.rand(B, generator=g))
    static = [t.cuda() for t in first]
    static[0].requires_grad_()

    def step():
        static[0].grad = None
        loss = ops.cross_entropy(static[0], MixTarget(*static[1:]),
                                 label_smoothing=eps)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one chain: fwd, mean, bwd
        static_loss = step()
    static_grad = static[0].grad
    # new logits, targets and weights, in place; one replay
    with torch.no_grad():
        for dst, src in zip(static, second):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()

    z = second[0].cuda().requires_grad_()
    loss = ops.cross_entropy(z, MixTarget(*(t.cuda() for t in second[1:])),
                             label_smoothing=eps)
    (grad,) = torch.autograd.grad(loss, z)
    assert torch.equal(static_loss, loss) and torch.equal(static_grad, grad)
    # and the replay did follow the new batch
    old = ops.cross_entropy(first[0].cuda(),
                            MixTarget(*(t.cuda() for t in first[1:])),
                            label_smoothing=eps)
    assert not torch.equal(static_loss, old)


# -- end to end ---------------------------------------------------------------


@pytest.mark.parametrize("compute_dtype", [torch.float16], indirect=True)
@pytest.mark.parametrize("make", [lambda: build_model("resnet18"), Net],
                         ids=["resnet18", "net"])
def test_models_train_on_mixed_batches_with_smoothing(compute_dtype, make):
    torch.manual_seed(0)
    dev = torch.device("cuda")
    ds = SyntheticImageDataset(48, seed=7)
    dl = DeviceLoader(ds, batch_size=16, shuffle=True, device=dev, seed=SEED,
                      augment=Augment(cutmix=0.4, mixup=0.4))
    net = make().to(dev)
    flat = FlatState(net)
    opt = optim.SGD(flat, lr=0.05, momentum=0.9)
    scaler = amp.DeviceGradScaler(init_scale=2.0 ** 10, device=dev)
    before = flat.flat_param.detach().clone()
    losses, mixed = [], 0
    for x, t in dl:
        assert isinstance(t, MixTarget) and x.dtype == torch.float16
        mixed += int((t.lam < 1).sum())
        opt.zero_grad()
        loss = ops.cross_entropy(net(x), t, label_smoothing=0.1)
        scaler.scale(loss).backward()
        opt.step(scaler=scaler)
        losses.append(loss.item())
    assert len(losses) == 3 and mixed >= 8
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert not torch.equal(flat.flat_param.detach(), before)
    assert scaler.skipped_steps == 0

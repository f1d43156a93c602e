"""GPU end-to-end: full models train on the HIP kernel path, loss falls."""

import pytest
import torch

from mi355x import optim
from mi355x.models import Net, build_model
from mi355x.ops import cross_entropy, have_ext
from mi355x.parallel.flat import FlatState

pytestmark = pytest.mark.gpu


def _train(model, batch=16, size=32, classes=10, steps=8, lr=0.05):
    dev = torch.device("cuda")
    net = model.to(dev)
    flat = FlatState(net)
    opt = optim.SGD(flat, lr=lr, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, 3, size, size, generator=g).to(dev)
    y = torch.randint(0, classes, (batch,), generator=g).to(dev)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = cross_entropy(net(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def test_extension_is_required():
    assert have_ext(), "HIP extension must be present on the GPU box"


def test_net_trains_on_gpu():
    torch.manual_seed(0)
    losses = _train(Net(), steps=20, lr=0.05)
    assert all(l == l for l in losses), losses  # no NaN
    assert losses[-1] < losses[0]


def test_resnet18_trains_on_gpu():
    torch.manual_seed(0)
    losses = _train(build_model("resnet18"), steps=8)
    assert all(l == l for l in losses), losses
    assert losses[-1] < losses[0] * 0.8, losses


def test_resnet50_trains_on_gpu():
    torch.manual_seed(0)
    losses = _train(build_model("resnet50", num_classes=1000), batch=4,
                    size=64, classes=1000, steps=4, lr=0.01)
    assert all(l == l for l in losses), losses


def test_gpu_matches_cpu_model_output():
    """Same weights: GPU bf16 forward tracks the CPU fp32 forward."""
    torch.manual_seed(1)
    net = Net()
    x = torch.randn(4, 3, 32, 32)
    y_cpu = net(x)
    net_gpu = Net()
    net_gpu.load_state_dict(net.state_dict())
    y_gpu = net_gpu.cuda()(x.cuda())
    torch.testing.assert_close(y_gpu.float().cpu(), y_cpu, rtol=5e-2,
                               atol=5e-2)


def test_checkpoint_gpu_cpu_interchange(tmp_path):
    torch.manual_seed(2)
    net = Net().cuda()
    p = tmp_path / "ck.pth"
    torch.save(net.state_dict(), p)
    net2 = Net()
    net2.load_state_dict(
        {k: v.cpu() for k, v in torch.load(p, weights_only=True).items()})
    x = torch.randn(2, 3, 32, 32)
    torch.testing.assert_close(net2(x), net.cpu()(x), rtol=1e-4, atol=1e-5)


def test_resnet18_fp16_trains_on_gpu():
    from mi355x import amp
    torch.manual_seed(0)
    with amp.autocast(torch.float16):
        losses = _train(build_model("resnet18"), steps=6)
    assert all(l == l for l in losses), losses
    assert losses[-1] < losses[0] * 1.05, losses


def test_fp16_dynamic_scaling_overflow_recovery():
    """BASELINE config 5 on hardware: start with an absurd loss scale so the
    fp32 flat grads overflow; the scaler must skip those steps (params
    untouched), halve down to a workable scale, then train normally."""
    from mi355x import amp

    dev = torch.device("cuda")
    torch.manual_seed(0)
    with amp.autocast(torch.float16):
        net = build_model("resnet18").to(dev)
        flat = FlatState(net)
        opt = optim.SGD(flat, lr=0.05, momentum=0.9)
        scaler = amp.GradScaler(init_scale=2.0**40, growth_interval=10_000)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(16, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (16,), generator=g).to(dev)
        p0 = flat.flat_param.clone()
        skips = 0
        losses = []
        for _ in range(30):
            opt.zero_grad()
            used = scaler.scale_value
            loss = cross_entropy(net(x), y)
            (loss * used).backward()
            if scaler.step_ok(flat.flat_grad):
                opt.grad_scale = 1.0 / used
                opt.step()
                losses.append(loss.item())
            else:
                skips += 1
                if not losses:  # nothing applied yet: params must be frozen
                    torch.testing.assert_close(flat.flat_param, p0,
                                               rtol=0, atol=0)
    assert skips >= 1, "2^40 scale should overflow fp32 grads at least once"
    assert scaler.scale_value < 2.0**40
    assert len(losses) >= 5 and losses[-1] < losses[0], (skips, losses)


def test_device_dataloader_prefetch_roundtrip():
    """The prefetching H2D loader (mi355x/data.py device= path) delivers
    exactly the dataset's tensors, in sampler order, on the GPU."""
    from mi355x.data import DataLoader, SyntheticImageDataset

    ds = SyntheticImageDataset(67, seed=9)
    dl = DataLoader(ds, batch_size=16, shuffle=False, device="cuda")
    seen_x, seen_y = [], []
    for x, y in dl:
        assert x.is_cuda and y.is_cuda
        seen_x.append(x.cpu())
        seen_y.append(y.cpu())
    torch.cuda.synchronize()
    torch.testing.assert_close(torch.cat(seen_x), ds.data)
    torch.testing.assert_close(torch.cat(seen_y), ds.targets)


def _grad_parity(model, size, env, off, on):
    """Compare the flat gradient between two kernel-path modes against the
    SAME-MODE rounding-noise floor. The reductions add in a fixed order, so
    a repeated run is bit-identical and shows no noise; the floor is
    instead how far the gradient moves when a handful of roundings fall the
    other way: the baseline mode rerun on the input scaled by (1 + 2^-20),
    which flips the bf16 rounding of about one input element in 2000 and
    changes nothing else (what the fp32 reduction-order differences of the
    earlier atomic reductions did: ~0.11 max-abs on the r18 stem wgrad).
    bf16 re-rounding in every layer amplifies either to the same scale.

    Measured on one MI355X, max-abs over the flat gradient, four draws each
    (old: rerun noise of the atomic reductions; new: this floor at scalings
    2^-20..2^-17, which all land alike): resnet18 old 0.10-0.14, new
    0.12-0.15; resnet50/64px/batch 8 old 39-59, new 48-77. The mode deltas
    themselves, no longer buried in rerun noise: TAP 0.005 (r18) and 0.85
    (r50), lazy BN 0.0 exactly."""
    import os

    torch.manual_seed(3)
    classes = 10 if model == "resnet18" else 1000
    net = build_model(model, num_classes=classes).cuda()
    flat = FlatState(net)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, size, size, generator=g).cuda()
    yl = torch.randint(0, classes, (8,), generator=g).cuda()

    def run(v, xin=x):
        os.environ[env] = v
        flat.zero_grad()
        cross_entropy(net(xin), yl).backward()
        torch.cuda.synchronize()
        return flat.flat_grad.clone()

    try:
        g0a = run(off)
        assert torch.equal(run(off), g0a), "same-mode rerun is not bitwise"
        g0b = run(off, x * (1.0 + 2.0 ** -20))
        g1 = run(on)
    finally:
        os.environ.pop(env, None)
    noise = (g0b - g0a).abs().max().item()
    delta = (g1 - g0a).abs().max().item()
    # floor covers the case where the two baseline runs happen to agree
    # closely while the mode under test legitimately rounds differently
    assert delta <= max(4 * noise, 2e-2), (
        f"{env}: delta {delta:.5f} vs noise floor {noise:.5f}")


@pytest.mark.parametrize("model,size", [("resnet18", 32), ("resnet50", 64)])
def test_residual_tap_grad_parity(model, size):
    """The residual-tap fusion (junction gradient added in the dgrad
    epilogue, mi355x/ops/functional._ConvTapFn) produces the same flat
    gradient as the plain double-use path (MI355X_TAP=0), to within the
    reduction-order noise floor."""
    _grad_parity(model, size, "MI355X_TAP", "0", "1")


@pytest.mark.parametrize("model,size", [("resnet18", 32), ("resnet50", 64)])
def test_lazy_bn_grad_parity(model, size):
    """Lazy BN (apply fused into the consuming conv's A-loads with
    mask-recompute backward, ops.functional._BNConvFn) matches the
    materialized-apply path to within the reduction-order noise floor
    (both all-consumer and gather-only modes)."""
    _grad_parity(model, size, "MI355X_LAZY_BN", "0", "1")
    _grad_parity(model, size, "MI355X_LAZY_BN", "0", "g")


def test_ddp_world2_single_gpu_fallback():
    """Oversubscribed layout (2 ranks sharing cuda:0 over gloo): the
    collective feasibility agreement must detect the duplicate device and
    fall back to torch.distributed instead of hanging in native RCCL
    init (parallel/ddp.py::_native_feasible_everywhere; the torch-DDP
    contract of /root/reference/cifar_example_ddp.py:83)."""
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(__file__), "_ddp_gpu_worker.py")
    env = dict(os.environ, MI355X_BACKEND="gloo",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--standalone",
         "--local-addr", "127.0.0.1", "--nproc-per-node", "2", worker],
        capture_output=True, text=True, timeout=300, env=env,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, (r.stdout[-1500:] + "\n" + r.stderr[-2500:])
    assert "DDP_GPU_OK native=False" in r.stdout

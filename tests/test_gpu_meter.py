"""The meter kernels (mi355x/csrc/meter.hip) against the plain-torch twin on
the same 16-bit logits: counts, bad rows, updates and the confusion matrix
are equal, the computed loss is as close to fp64 cross-entropy as the
existing hard-label kernel is (within a factor of two), the state is
bit-identical from run to run, and an update replays from a captured
graph."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _meter_common import (K, SHAPES, bad_rows, inputs, planted, reference,
                           state_dict)
from mi355x.metrics import DeviceMeter
from mi355x.ops import MixTarget, ext

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]

# C <= 16 packs 16 rows into a block and the grid stops at 2048 blocks: one
# pass covers 32768 rows. This B needs a second pass of one partial block.
B_TWO_PASSES = 2048 * 16 + 5
GPU_SHAPES = SHAPES + [(B_TWO_PASSES, 10)]


def _cpu_meter(C, logits, target, loss=None, k=K):
    m = DeviceMeter(C, topk=k, confusion=True)
    m.update(logits, target, loss=loss)
    return m


def _gpu_meter(C, logits, target, loss=None, k=K):
    m = DeviceMeter(C, topk=k, confusion=True, device="cuda")
    m.update(logits, target, loss=loss)
    return m


def _to_cuda(target):
    return target.to("cuda") if isinstance(target, MixTarget) else target.cuda()


def _same_counts(gpu, cpu):
    g, c = state_dict(gpu.state), state_dict(cpu.state)
    for key in ("rows", "correct1", "correctk", "bad", "updates"):
        assert g[key] == c[key], key
    assert torch.equal(gpu.confusion.cpu(), cpu.confusion)
    return g, c


def _fp64_loss(logits16, y):
    return F.cross_entropy(logits16.double(), y).item()


def _rel(got, want):
    return abs(got - want) / (abs(want) if want != 0 else 1.0)


@pytest.fixture(scope="module")
def hard_error():
    """Per dtype: the largest relative error of the existing
    ext().cross_entropy_fwd mean against fp64 cross-entropy over GPU_SHAPES,
    on the logits the meter tests use. Computed once."""
    out = {}
    for dtype in DTYPES:
        worst = 0.0
        for B, C in GPU_SHAPES:
            logits, y, _, _ = inputs(B, C, dtype)
            loss, _ = ext().cross_entropy_fwd(logits.cuda(), y.cuda())
            e = _rel(loss.double().item(), _fp64_loss(logits, y))
            print(f"hard  {str(dtype):15s} B={B:<6d} C={C:<5d} err={e:.3e}")
            worst = max(worst, e)
        out[dtype] = worst
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,C", GPU_SHAPES)
def test_kernel_equals_twin_and_loss_is_close_to_fp64(hard_error, B, C, dtype):
    """Counts and matrix: equal. The loss bound is measured, not chosen:
    twice the error of the hard-label kernel's mean against the same fp64
    value (largest over GPU_SHAPES, per dtype). A row's nll here is that
    kernel's row loss bit for bit (same tree), and the rows are added in
    double, so the meter should not be worse.

    Measured on an MI355X (largest over the six shapes):
      hard-label mean  bf16 8.68e-08  fp16 8.11e-08
      meter            bf16 3.67e-08  fp16 1.17e-08
    (the meter's largest is the B = 1 row, where both are the same fp32
    number; from 33 rows up it stays below 1.2e-08)
    """
    logits, y, _, _ = inputs(B, C, dtype)
    before = (logits.clone(), y.clone())
    z, t = logits.cuda(), y.cuda()
    gpu = _gpu_meter(C, z, t)
    g, _ = _same_counts(gpu, _cpu_meter(C, logits, y))
    assert g["bad"] == 0 and g["rows"] == B
    # the inputs are untouched
    assert torch.equal(z.cpu(), before[0]) and torch.equal(t.cpu(), before[1])
    r = gpu.compute()
    e = _rel(r["loss"], _fp64_loss(logits, y))
    bound = 2 * hard_error[dtype]
    print(f"meter {str(dtype):15s} B={B:<6d} C={C:<5d} err={e:.3e} "
          f"(bound {bound:.3e})")
    assert e <= bound
    # two runs on the same inputs: the same bits
    assert torch.equal(_gpu_meter(C, z, t).state, gpu.state)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,C", [(33, 10), (33, 65)])
def test_logits_one_element_into_their_storage(B, C, dtype):
    logits, y, _, _ = inputs(B, C, dtype)
    buf = torch.zeros(B * C + 1, dtype=dtype, device="cuda")
    z = buf[1:].view(B, C)
    z.copy_(logits)
    assert z.is_contiguous() and z.data_ptr() % 16 != 0
    _same_counts(_gpu_meter(C, z, y.cuda()), _cpu_meter(C, logits, y))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_planted_ties_on_the_device(dtype):
    logits, labels, want1, want5, untied = planted(dtype)
    assert untied != (want1, want5)
    for k, wantk in ((1, want1), (5, want5)):
        gpu = _gpu_meter(10, logits.cuda(), labels.cuda(), k=k)
        g, _ = _same_counts(gpu, _cpu_meter(10, logits, labels, k=k))
        assert (g["correct1"], g["correctk"]) == (want1, wantk)
        conf = gpu.compute()["confusion"]
        assert conf[7, 2] == 1 and conf[2, 2] == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bad_rows_on_the_device(dtype):
    logits, y, where = bad_rows(dtype)
    gpu = _gpu_meter(10, logits.cuda(), y.cuda())
    g, _ = _same_counts(gpu, _cpu_meter(10, logits, y))
    want = reference(logits, y)
    assert g["bad"] == want["bad"] == len(where) == 4
    assert (g["correct1"], g["correctk"]) == (want["correct1"],
                                              want["correctk"])
    r = gpu.compute()
    assert math.isnan(r["loss"]) and r["bad_rows"] == 4
    assert np.array_equal(r["confusion"].numpy(), want["confusion"])
    assert math.isfinite(g["loss_sum"])  # the good rows' nll only


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,C", [(33, 10), (33, 65), (7, 1000)])
def test_mix_target_on_the_device(B, C, dtype):
    logits, y_a, y_b, lam = inputs(B, C, dtype)
    target = MixTarget(y_a, y_b, lam)
    gpu = _gpu_meter(C, logits.cuda(), _to_cuda(target))
    g, _ = _same_counts(gpu, _cpu_meter(C, logits, target))
    want = reference(logits, y_a, y_b, lam)
    assert lam[0] == 0.5 and want["labels"][0] == int(y_a[0])
    assert (g["correct1"], g["correctk"]) == (want["correct1"],
                                              want["correctk"])
    assert np.array_equal(gpu.confusion.cpu().numpy(), want["confusion"])


def test_external_loss_sum_equals_the_twin_to_the_bit():
    gpu = DeviceMeter(10, device="cuda")
    cpu = DeviceMeter(10)
    for seed, B in enumerate((33, 8, 1)):
        logits, y, _, _ = inputs(B, 10, torch.bfloat16, seed=seed)
        loss = torch.tensor(0.1 + 1.7 * seed, dtype=torch.float32)
        gpu.update(logits.cuda(), y.cuda(), loss=loss.cuda())
        cpu.update(logits, y, loss=loss)
    assert torch.equal(gpu.state.cpu(), cpu.state)
    # fp32 logits on the GPU take the twin there: the same numbers again
    twin = DeviceMeter(10, confusion=True, device="cuda")
    logits, y, _, _ = inputs(33, 10, torch.bfloat16)
    twin.update(logits.cuda().float(), y.cuda())
    _same_counts(twin, _cpu_meter(10, logits, y))


def test_update_replays_from_a_captured_graph():
    B, C = 33, 10
    batches = [inputs(B, C, torch.bfloat16, seed=s) for s in range(3)]
    static = [t.cuda() for t in batches[0]]
    meter = DeviceMeter(C, topk=K, confusion=True, device="cuda")

    def step():
        meter.update(static[0], MixTarget(*static[1:]))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one chain: rows, finalise
        step()
    meter.reset()
    for batch in batches:
        with torch.no_grad():
            for dst, src in zip(static, batch):
                dst.copy_(src)
        graph.replay()
    torch.cuda.synchronize()

    eager = DeviceMeter(C, topk=K, confusion=True, device="cuda")
    for batch in batches:
        z, y_a, y_b, lam = (t.cuda() for t in batch)
        eager.update(z, MixTarget(y_a, y_b, lam))
    assert torch.equal(meter.state, eager.state)
    assert torch.equal(meter.confusion, eager.confusion)
    assert state_dict(meter.state)["rows"] == 3 * B
    assert state_dict(meter.state)["updates"] == 3

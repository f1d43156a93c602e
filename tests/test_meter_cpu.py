"""metrics.DeviceMeter and ops.meter_update on the CPU: the plain-torch twin
of the meter kernels against an independent numpy/fp64 computation of the
definitions (label choice, rank with its tie rule, bad rows), the external
loss path, accumulation, reset, and the sum over ranks."""

import math

import numpy as np
import pytest
import torch

from _meter_common import (K, SHAPES, bad_rows, inputs, planted, reference,
                           state_dict)
from mi355x import ops
from mi355x.metrics import DeviceMeter
from mi355x.ops import MixTarget
from tests.test_ddp_cpu import run_distributed

DTYPES = [torch.bfloat16, torch.float16, torch.float32]

# |loss - fp64 loss| allowed for the twin's fp32 rows: a row's lse is
# mx + log(sum) with the sum of C <= 1000 terms <= 1 in fp32 (relative error
# <= ~log2(C) eps, the same absolute error after the log), rounded once more
# by the addition and once by lse - z_t: (log2(C) + 2 + |lse| + |nll|) eps
# with |lse|, |nll| < 30 on these logits (|z| < 15) and eps = 2^-23 is below
# 1e-5. The mean over rows cannot exceed the largest row error.
LOSS_ATOL = 1e-5


def _meter(C, logits, target, confusion=True, k=K, loss=None):
    m = DeviceMeter(C, topk=k, confusion=confusion)
    m.update(logits, target, loss=loss)
    return m


def _check(meter, want, k=K):
    r = meter.compute()
    got = state_dict(meter.state)
    assert got["rows"] == r["rows"] == want["rows"]
    assert got["correct1"] == want["correct1"]
    assert got["correctk"] == want["correctk"]
    assert got["bad"] == r["bad_rows"] == want["bad"]
    assert r["top1"] == want["correct1"] / want["rows"]
    assert r[f"top{k}"] == want["correctk"] / want["rows"]
    assert np.array_equal(r["confusion"].numpy(), want["confusion"])
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,C", SHAPES)
def test_twin_matches_fp64_definitions(B, C, dtype):
    logits, y_a, _, _ = inputs(B, C, dtype)
    want = reference(logits, y_a)
    r = _check(_meter(C, logits, y_a), want)
    assert want["bad"] == 0
    assert abs(r["loss"] - want["nll_sum"] / B) <= LOSS_ATOL
    assert r["updates"] == 1
    if K >= C:  # k >= C: every good row is correct
        assert r[f"top{K}"] == 1.0
    seen = want["confusion"].sum(1)
    for c in range(C):
        if seen[c] == 0:
            assert math.isnan(r["per_class"][c])
        else:
            assert r["per_class"][c] == want["confusion"][c, c] / seen[c]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_planted_ties_decide_the_counts(dtype):
    logits, labels, want1, want5, untied = planted(dtype)
    want = reference(logits, labels)
    # the planted rows are there: ranks straight from the definition
    assert want["ranks"] == [1, 0, 5, 4, 0, 9]
    assert (logits[0, 2] == logits[0, 7] == logits[0].max()
            and logits[2, 3] == logits[2, 8])
    assert (want["correct1"], want["correctk"]) == (want1, want5)
    # ... and they decide: a rule blind to ties would count differently
    z = logits.double().numpy()
    zt = z[np.arange(6), labels.numpy()][:, None]
    blind = (z > zt).sum(1)
    assert (int((blind == 0).sum()), int((blind < 5).sum())) == untied
    assert untied != (want1, want5)
    for k, wantk in ((1, want1), (5, want5)):
        m = _meter(10, logits, labels, k=k)
        s = state_dict(m.state)
        assert s["correct1"] == want1 and s["correctk"] == wantk
        # column = pred = first index of the maximum: rows 0 and 1 -> 2
        conf = m.compute()["confusion"]
        assert conf[7, 2] == 1 and conf[2, 2] == 1
        assert np.array_equal(conf.numpy(), want["confusion"])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,C", [(33, 10), (33, 65), (7, 1000)])
def test_mix_target_takes_the_heavier_label(B, C, dtype):
    logits, y_a, y_b, lam = inputs(B, C, dtype)
    want = reference(logits, y_a, y_b, lam)
    # lam == 0.5 takes y_a, just below takes y_b
    assert lam[0] == 0.5 and want["labels"][0] == int(y_a[0])
    assert lam[1] < 0.5 and want["labels"][1] == int(y_b[1])
    assert want["labels"] != y_a.tolist() and want["labels"] != y_b.tolist()
    r = _check(_meter(C, logits, MixTarget(y_a, y_b, lam)), want)
    assert abs(r["loss"] - want["nll_sum"] / B) <= LOSS_ATOL


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bad_rows_are_counted_and_poison_only_the_loss(dtype):
    logits, y, where = bad_rows(dtype)
    want = reference(logits, y)
    assert want["bad"] == 4
    assert [i for i, r in enumerate(want["ranks"]) if r is None] == where
    r = _check(_meter(10, logits, y), want)
    assert math.isnan(r["loss"]) and r["bad_rows"] == 4
    # the counts are those of the 29 good rows alone
    keep = [i for i in range(33) if i not in where]
    good = reference(logits[keep], y[keep])
    assert (want["correct1"], want["correctk"]) == (good["correct1"],
                                                    good["correctk"])
    assert np.array_equal(want["confusion"], good["confusion"])
    assert r["confusion"].sum() == 29
    # the loss sum itself only holds the good rows' nll
    s = state_dict(_meter(10, logits, y).state)
    assert abs(s["loss_sum"] - good["nll_sum"]) <= 29 * LOSS_ATOL


def test_external_loss_accumulation_reset_and_keys():
    m = DeviceMeter(10, topk=3, confusion=True)
    total, rows, want_c1 = 0.0, 0, 0
    for seed, B in enumerate((33, 8, 1)):
        logits, y, _, _ = inputs(B, 10, torch.float32, seed=seed)
        loss = torch.tensor(0.1 + seed, dtype=torch.float32)
        m.update(logits, y, loss=loss)
        total += float(loss.double()) * B   # (double)loss * B, in turn
        rows += B
        want_c1 += reference(logits, y, k=3)["correct1"]
    r = m.compute()
    assert set(r) == {"rows", "top1", "top3", "loss", "bad_rows", "updates",
                      "confusion", "per_class"}
    assert r["rows"] == rows == 42 and r["updates"] == 3
    assert state_dict(m.state)["loss_sum"] == total      # to the bit
    assert r["loss"] == total / rows
    assert r["top1"] == want_c1 / rows
    assert r["confusion"].dtype == torch.int64 and r["confusion"].sum() == rows
    assert set(DeviceMeter(10, topk=5).compute()) == {
        "rows", "top1", "top5", "loss", "bad_rows", "updates"}
    m.reset()
    r = m.compute()
    assert r["rows"] == r["updates"] == r["bad_rows"] == 0
    assert r["confusion"].sum() == 0 and math.isnan(r["loss"])
    # a computed-nll update after the reset starts from zero
    logits, y, _, _ = inputs(33, 10, torch.float32)
    m.update(logits, y)
    want = reference(logits, y, k=3)
    assert abs(m.compute()["loss"] - want["nll_sum"] / 33) <= LOSS_ATOL


def test_merge_adds_a_window_into_a_total():
    run, win = DeviceMeter(10), DeviceMeter(10)
    both = DeviceMeter(10)
    for seed in range(3):
        logits, y, _, _ = inputs(8, 10, torch.float32, seed=seed)
        loss = torch.tensor(1.5 * seed, dtype=torch.float32)
        win.update(logits, y, loss=loss)
        both.update(logits, y, loss=loss)
        if seed == 1:
            run.merge(win)
            win.reset()
    run.merge(win)
    assert torch.equal(run.state, both.state)


def test_update_changes_neither_logits_nor_targets():
    logits, y_a, y_b, lam = inputs(33, 10, torch.bfloat16)
    keep = [t.clone() for t in (logits, y_a, y_b, lam)]
    _meter(10, logits, MixTarget(y_a, y_b, lam))
    for a, b in zip(keep, (logits, y_a, y_b, lam)):
        assert torch.equal(a, b)


def test_ops_meter_update_is_exported_and_checks_its_arguments():
    state = torch.zeros(8, dtype=torch.int64)
    logits, y, _, _ = inputs(7, 10, torch.float32)
    ops.meter_update(state, None, logits, y, k=1)
    s = state_dict(state)
    assert s["rows"] == 7 and s["correct1"] == s["correctk"]
    with pytest.raises(ValueError):
        ops.meter_update(state, None, logits, y, k=0)
    with pytest.raises(ValueError):
        ops.meter_update(state, None, logits, y, y, None, k=1)
    with pytest.raises(ValueError):
        DeviceMeter(10).update(torch.zeros(4, 11), y[:4])


def _two_ranks(rank):
    from mi355x.parallel import comm

    comm.init_process_group(backend="gloo")
    m = DeviceMeter(10, topk=K, confusion=True)
    for seed in (rank, rank + 2):       # different batches on each rank
        logits, y, _, _ = inputs(9 + rank, 10, torch.bfloat16, seed=seed)
        if seed == 3:
            y[0] = 10                   # one bad row, on rank 1 only
        m.update(logits, y)
    local = m.compute(sync=False)
    return m.compute(), local, m.state.clone()


def test_compute_sums_over_two_gloo_ranks():
    res = run_distributed(_two_ranks)
    one = DeviceMeter(10, topk=K, confusion=True)
    batches = []
    for rank in (0, 1):
        for seed in (rank, rank + 2):
            logits, y, _, _ = inputs(9 + rank, 10, torch.bfloat16, seed=seed)
            if seed == 3:
                y[0] = 10
            batches.append((logits, y))
            one.update(logits, y)
    want = reference(torch.cat([b[0] for b in batches]),
                     torch.cat([b[1] for b in batches]))
    single = one.compute()
    assert single["rows"] == 38 and single["bad_rows"] == want["bad"] == 1
    for rank in (0, 1):
        summed, local, _ = res[rank]
        assert local["rows"] == 2 * (9 + rank) and local["updates"] == 2
        for key in ("rows", "top1", f"top{K}", "bad_rows", "updates"):
            assert summed[key] == single[key], key
        assert summed["top1"] == want["correct1"] / 38
        assert math.isnan(summed["loss"]) and math.isnan(single["loss"])
        assert torch.equal(summed["confusion"], single["confusion"])
        assert np.array_equal(summed["confusion"].numpy(), want["confusion"])
        assert torch.equal(summed["per_class"].isnan(),
                           single["per_class"].isnan())
        assert torch.equal(summed["per_class"].nan_to_num(-1),
                           single["per_class"].nan_to_num(-1))
    # the loss sums add up exactly as doubles (two terms: commutative)
    s0, s1 = (state_dict(res[r][2])["loss_sum"] for r in (0, 1))
    assert math.isnan(res[0][0]["loss"]) and not math.isnan(res[0][1]["loss"])
    assert abs((s0 + s1) - state_dict(one.state)["loss_sum"]) <= 38 * LOSS_ATOL

"""Shared by the CPU and GPU meter tests: the inputs, the planted rows and
an independent numpy/fp64 computation of what ops.meter_update defines."""

import numpy as np
import torch

from mi355x.ops import functional as fn

SHAPES = [(1, 10), (33, 10), (33, 65), (7, 1000), (5, 1)]
K = 5


def inputs(B, C, dtype, seed=0):
    """(logits in `dtype`, y_a, y_b, lam) on the CPU. Rows 0/1/2 of a mixed
    batch get lam 0.5 (takes y_a), just below it (y_b) and 1."""
    g = torch.Generator().manual_seed(B * 1000 + C + 7919 * seed)
    logits = (torch.randn(B, C, generator=g) * 3).to(dtype)
    y_a = torch.randint(0, C, (B,), generator=g)
    y_b = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    for i, v in enumerate((0.5, 0.49999997, 1.0)[:B]):
        lam[i] = v
    return logits, y_a, y_b, lam


def reference(logits, y_a, y_b=None, lam=None, k=K):
    """Row by row in Python and fp64, straight from the definitions."""
    z = logits.double().numpy()
    B, C = z.shape
    out = {"rows": B, "correct1": 0, "correctk": 0, "bad": 0, "nll_sum": 0.0,
           "confusion": np.zeros((C, C), dtype=np.int64), "labels": [],
           "ranks": []}
    for b in range(B):
        t = int(y_a[b])
        if y_b is not None and not float(lam[b]) >= 0.5:
            t = int(y_b[b])
        row = z[b]
        with np.errstate(all="ignore"):
            m = row.max()
            lse = m + np.log(np.exp(row - m).sum())
        out["labels"].append(t)
        if not (0 <= t < C) or not np.isfinite(lse):
            out["bad"] += 1
            out["ranks"].append(None)
            continue
        rank = int((row > row[t]).sum() + (row[:t] == row[t]).sum())
        pred = next(c for c in range(C) if row[c] == m)
        out["ranks"].append(rank)
        out["correct1"] += rank == 0
        out["correctk"] += rank < k
        out["nll_sum"] += lse - row[t]
        out["confusion"][t, pred] += 1
    return out


def planted(dtype):
    """C = 10 rows whose label ties a decision boundary: (logits, labels,
    expected correct@1, expected correct@5, the counts a rule that ignores
    ties (rank = #{z_c > z_t}) would give).

      row 0  label 7 ties the maximum with index 2 (lower)   -> wrong @1
      row 1  label 2 ties the maximum with index 7 (higher)  -> right @1
      row 2  four larger logits; label 8 ties 5th place with
             index 3 (lower)                                 -> wrong @5
      row 3  the same with label 3 and the tie at 8 (higher) -> right @5
      row 4  a plain row, label is the single maximum        -> right
      row 5  a plain row, label is the single minimum        -> wrong
    """
    base = torch.tensor([-4., -3.5, -3., -2.5, -2., -1.5, -1., -0.5, 0., 0.5])
    rows = []
    r = base.clone(); r[2] = 3.0; r[7] = 3.0; rows.append(r)          # 0
    rows.append(r.clone())                                           # 1
    r = base.clone()
    r[[0, 1, 5, 9]] = torch.tensor([5., 6., 7., 8.]); r[3] = 1.25; r[8] = 1.25
    rows.append(r)                                                   # 2
    rows.append(r.clone())                                           # 3
    rows.append(base.clone())                                        # 4
    rows.append(base.clone())                                        # 5
    logits = torch.stack(rows).to(dtype)
    labels = torch.tensor([7, 2, 8, 3, 9, 0])
    return logits, labels, 2, 4, (3, 5)


def bad_rows(dtype):
    """(33, 10) inputs with four bad rows: label -1, label C, a NaN logit,
    an all -inf row. Returns (logits, labels, indices of the bad rows)."""
    logits, y, _, _ = inputs(33, 10, dtype)
    y = y.clone()
    logits = logits.clone()
    y[3] = -1
    y[11] = 10
    logits[20, 4] = float("nan")
    logits[32, :] = float("-inf")
    return logits, y, [3, 11, 20, 32]


def state_dict(state):
    """The meter state tensor as Python numbers."""
    s = state.cpu()
    return {
        "rows": int(s[fn.MT_ROWS]), "correct1": int(s[fn.MT_CORRECT1]),
        "correctk": int(s[fn.MT_CORRECTK]), "bad": int(s[fn.MT_BAD]),
        "loss_sum": float(s[fn.MT_LOSS_SUM:fn.MT_LOSS_SUM + 1]
                          .view(torch.float64)),
        "updates": int(s[fn.MT_UPDATES]),
    }

"""Shared by the LARS tests: the synthetic tensor table, a module that lays
it out in a FlatState, and the per-tensor fp64 reference (plain torch,
independent of mi355x.ops)."""

import torch
from torch import nn

from mi355x.parallel.flat import FlatState

TILE = 4096
# one tile, one tile + 1, two tiles - 1, two tiles + 7, between tiny ones;
# starts modulo 4: 0,1,0,0,1,1,1,2,1,0
SIZES = [1, 3, 4, 5, 64, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 7, 10]
EXCLUDE = [False, False, False, False, True, False, False, False, False, True]
ZERO_W, ZERO_G = 2, 3            # tensor 3: weights 0; tensor 4: gradient 0
HP = dict(lr=0.1, mu=0.9, wd=1e-4, eta=1e-3, eps=1e-8, grad_scale=0.5)
TRUST_RTOL = 32 * 2.0 ** -24     # two norms at 8 ulp + product, sum, quotient
ULP8 = 8 * 2.0 ** -24


def offsets_of(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + n)
    return out


def spans(offsets):
    return list(zip(offsets, offsets[1:]))


def synthetic(steps=3, seed=0, sizes=SIZES):
    """-> (w0, m0, [g_1..g_steps]) float32 on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    off = offsets_of(sizes)
    n = off[-1]
    w = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(steps)]
    if sizes is SIZES:
        w[off[ZERO_W]:off[ZERO_W + 1]] = 0
        for g in grads:
            g[off[ZERO_G]:off[ZERO_G + 1]] = 0
    return w, m, grads


class Table(nn.Module):
    """Parameters that a FlatState lays out as SIZES in order: excluded
    tensors 1-D, the others 2-D, so LARS' default predicate gives EXCLUDE."""

    def __init__(self, sizes=SIZES, exclude=EXCLUDE):
        super().__init__()
        shapes = [(n,) if e else (n, 1) for n, e in zip(sizes, exclude)]
        # FlatState lays parameters out in reverse registration order
        self.ps = nn.ParameterList(
            [nn.Parameter(torch.zeros(s)) for s in reversed(shapes)])


def table_flat(w, m, device="cpu"):
    flat = FlatState(Table().to(device))
    assert [p.numel() for p in flat.params] == SIZES
    flat.flat_param.copy_(w)
    flat.flat_momentum.copy_(m)
    return flat


def ref_step(w, m, g, offsets, exclude, *, lr, mu, wd, eta, eps, grad_scale,
             inv_scale=1.0, max_norm=None):
    """One LARS step on float64 w, m in place, g the raw gradient. Returns
    (trust ratios [S] float64, norm of the true gradient)."""
    k = grad_scale * inv_scale
    norm = float(g.norm()) * k
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    eff = k * coef
    trust = []
    for (a, b), ex in zip(spans(offsets), exclude):
        ws, gs, ms = w[a:b], g[a:b], m[a:b]
        wn, gn = float(ws.norm()), float(gs.norm()) * eff
        wd_s = 0.0 if ex else wd
        t = 1.0
        if not ex and wn > 0 and gn > 0:
            t = eta * wn / (gn + wd * wn + eps)
        gr = gs * eff + wd_s * ws
        ms.mul_(mu).add_(t * gr)
        ws.sub_(lr * ms)
        trust.append(t)
    return torch.tensor(trust, dtype=torch.float64), norm


def ref_trajectory(w, m, grads, offsets, exclude, **kw):
    """-> [(w, m, trust, norm) after each step], float64 copies."""
    w, m = w.double().clone(), m.double().clone()
    out = []
    for g in grads:
        trust, norm = ref_step(w, m, g.double(), offsets, exclude, **kw)
        out.append((w.clone(), m.clone(), trust, norm))
    return out


def assert_trust(got, ref, label=""):
    """Relative TRUST_RTOL; an exact 1.0 in the reference must be exact."""
    got = got.detach().cpu().double()
    rel = ((got - ref).abs() / ref.abs()).max().item()
    print(f"trust ratios {label}: max rel err {rel:.3e} "
          f"(bound {TRUST_RTOL:.3e})")
    assert rel <= TRUST_RTOL
    ones = ref == 1.0
    assert torch.equal(got[ones], torch.ones(int(ones.sum()),
                                             dtype=torch.float64))

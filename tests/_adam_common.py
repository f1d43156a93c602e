"""Shared by the AdamW/LAMB tests: the cases on _lars_common's tensor table,
the float64 references (torch.optim.AdamW where nothing is excluded, a plain
loop otherwise) and the comparison at the tolerances the kernels are held
to. Independent of mi355x.ops."""

import torch

from _lars_common import EXCLUDE, SIZES, offsets_of, spans, synthetic, table_flat
from mi355x import optim

OFF = offsets_of(SIZES)
KINDS = {"adamw": optim.AdamW, "lamb": optim.LAMB}
HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, grad_scale=0.5)
# about 20 fp32 roundings of 2^-24 per element and step over three steps
RTOL, ATOL = 4e-6, 4e-7
TRUST_RTOL = 1e-5   # two norms at <= 10 ulp, a quotient, 5x margin
NOTHING = [False] * len(SIZES)

# id: (optimizer, max_grad_norm, weight decay, exclusions)
CASES = {
    "adamw-noclip": ("adamw", None, 1e-2, EXCLUDE),
    "adamw-clip": ("adamw", 1.0, 1e-2, EXCLUDE),
    "lamb-noclip": ("lamb", None, 1e-2, EXCLUDE),
    "lamb-clip": ("lamb", 1.0, 1e-2, EXCLUDE),
    "adamw-torch": ("adamw", 1.0, 1e-2, NOTHING),  # torch.optim.AdamW
    "lamb-wd0": ("lamb", None, 0.0, EXCLUDE),      # g == 0 gives u == 0
}


def start(steps=3):
    """-> (w0, [g_1..g_steps]) float32 on the CPU; m and v start at 0."""
    w, _, grads = synthetic(steps=steps)
    return w, grads


def make(kind, w0, device, max_norm, wd, exclude, **kw):
    flat = table_flat(w0, torch.zeros_like(w0), device)
    flags = dict(zip(map(id, flat.params), exclude))
    return KINDS[kind](flat, weight_decay=wd, max_grad_norm=max_norm,
                       exclude=lambda p: flags[id(p)], **{**HP, **kw})


def snapshot(opt):
    """-> [w, m, v, trust or None] as CPU clones."""
    out = [opt.flat.flat_param, opt.flat.flat_momentum, opt.exp_avg_sq]
    out.append(opt.last_trust_ratios if isinstance(opt, optim.LAMB) else None)
    return [None if t is None else t.detach().cpu().clone() for t in out]


def run(opt, grads):
    out = []
    for g in grads:
        opt.flat.flat_grad.copy_(g)
        opt.step()
        out.append(snapshot(opt))
    return out


def _eff(g, max_norm):
    norm = float(g.norm()) * HP["grad_scale"]
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    return HP["grad_scale"] * coef


def reference(kind, w0, grads, max_norm, wd, exclude):
    """-> [[w, m, v, trust] after each step] in float64."""
    lr, (b1, b2), eps = HP["lr"], HP["betas"], HP["eps"]
    w = w0.double().clone()
    out = []
    if kind == "adamw" and not any(exclude):
        p = torch.nn.Parameter(w)
        o = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps,
                              weight_decay=wd)
        for g in grads:
            p.grad = g.double() * _eff(g.double(), max_norm)
            o.step()
            out.append([p.detach().clone(), o.state[p]["exp_avg"].clone(),
                        o.state[p]["exp_avg_sq"].clone(), None])
        return out
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    for t, g in enumerate(grads, 1):
        g = g.double() * _eff(g.double(), max_norm)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
        trust = []
        for (a, b), ex in zip(spans(OFF), exclude):
            us = u[a:b] + (0.0 if ex else wd) * w[a:b]
            wn, un = float(w[a:b].norm()), float(us.norm())
            lamb = kind == "lamb" and not ex and wn > 0 and un > 0
            trust.append(wn / un if lamb else 1.0)
            w[a:b] -= lr * trust[-1] * us
        out.append([w.clone(), m.clone(), v.clone(),
                    torch.tensor(trust, dtype=torch.float64)])
    return out


def compare(got, ref, label):
    """One step's [w, m, v, trust] against the reference: prints every worst
    error as a fraction of its line, then asserts."""
    for name, a, r in zip("wmv", got, ref):
        frac = ((a.double() - r).abs() / (ATOL + RTOL * r.abs())).max()
        print(f"{label} {name}: worst error {float(frac):.3f} of the line")
    if got[3] is not None:
        rel = ((got[3].double() - ref[3]).abs() / ref[3].abs()).max()
        print(f"{label} trust: max rel err {float(rel):.3e} "
              f"(line {TRUST_RTOL:.0e})")
    for a, r in zip(got[:3], ref[:3]):
        torch.testing.assert_close(a.double(), r, rtol=RTOL, atol=ATOL)
    if got[3] is not None:
        torch.testing.assert_close(got[3].double(), ref[3], rtol=TRUST_RTOL,
                                   atol=0)
        ones = ref[3] == 1.0
        assert bool((got[3][ones] == 1.0).all()), label

"""What CutMix / Mixup and the soft-target loss cost on one GPU.

Every variant of a group is timed in the same process, interleaved, --reps
times, with HIP events around --calls back-to-back calls after a warmup, so
the run-to-run spread stands next to the differences:

  (g) batch building at --batch x 32x32x3: the plain gather_augment kernel
      against gather_mix_kernel at (cutmix, mixup) = (0,0), (1,0), (0,1) and
      (0.5,0.5), all with pad-4 crop + flip
  (l) the loss at (--batch, 10) and (--batch, 1000): the hard-label
      forward + backward pair, the soft pair (label smoothing 0.1 and a
      MixTarget), and the same soft loss built from torch ops on the GPU
      (log_softmax, gather, mean and the mix; backward through autograd),
      and, with --launches, the number of kernels each launches per
      forward + backward (counted with the torch profiler, in a run of its
      own: no times are taken then)

Each line also gives the time as a share of --step-ms (the ResNet-18 step
the shares in profiles/ refer to). Prints one JSON line per measurement.
Needs a GPU; there is no CPU fallback.

    python benchmarks/mix_bench.py --batch 8192 --reps 3
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mi355x import ops  # noqa: E402
from mi355x.data import DeviceLoader, SyntheticImageDataset  # noqa: E402

STEP_MS = 51.0


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, calls):
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    for k in range(calls):
        fn(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls  # us per call


def interleaved(group, variants, reps, calls, **tags):
    """variants: name -> fn(k). Warm each, then reps rounds over all."""
    for fn in variants.values():
        for k in range(5):
            fn(k)
    torch.cuda.synchronize()
    for rep in range(reps):
        for name, fn in variants.items():
            us = timed(fn, calls)
            emit(what=group, variant=name, rep=rep, us_per_call=round(us, 2),
                 pct_of_step=round(us / (STEP_MS * 1e3) * 100, 4), **tags)


def gather_group(n, batch, dev, reps, calls):
    ds = SyntheticImageDataset(n, seed=1)
    dl = DeviceLoader(ds, batch_size=batch, device=dev)
    g = torch.Generator().manual_seed(0)
    idx = torch.randperm(n, generator=g)[:batch].to(torch.int32).to(dev)
    args = (dl.data_u8, dl.targets, idx, dl.scale, dl.shift)
    variants = {"gather_augment": lambda k: ops.gather_augment(
        *args, pad=4, flip=True, epoch=k)}
    for cm, mu in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5)):
        variants[f"mix({cm:g},{mu:g})"] = (
            lambda k, cm=cm, mu=mu: ops.gather_augment_mix(
                *args, pad=4, flip=True, cutmix=cm, mixup=mu, epoch=k))
    interleaved("gather", variants, reps, calls, batch=batch)


def torch_soft_loss(z, t, eps):
    """The soft loss a user can build today from torch ops on the GPU."""
    lp = F.log_softmax(z.float(), dim=1)
    smooth = -lp.mean(dim=1)
    na = (1 - eps) * -lp.gather(1, t.y_a[:, None])[:, 0] + eps * smooth
    nb = (1 - eps) * -lp.gather(1, t.y_b[:, None])[:, 0] + eps * smooth
    return (t.lam * na + (1 - t.lam) * nb).mean()


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile

    fn(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(0)
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages()
               if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.key.lower())


def loss_group(batch, classes, dev, reps, calls, launches, eps=0.1):
    g = torch.Generator().manual_seed(classes)
    z = (torch.randn(batch, classes, generator=g) * 3).to(
        ops.compute_dtype()).to(dev).requires_grad_()
    t = ops.MixTarget(
        torch.randint(0, classes, (batch,), generator=g).to(dev),
        torch.randint(0, classes, (batch,), generator=g).to(dev),
        torch.rand(batch, generator=g).to(dev))

    def fwd_bwd(loss_fn):
        def run(k):
            torch.autograd.grad(loss_fn(), z)
        return run

    variants = {
        "hard": fwd_bwd(lambda: ops.cross_entropy(z, t.y_a)),
        "soft": fwd_bwd(lambda: ops.cross_entropy(z, t, label_smoothing=eps)),
        "torch_soft": fwd_bwd(lambda: torch_soft_loss(z, t, eps)),
    }
    if launches:
        for name, fn in variants.items():
            emit(what="loss_launches", classes=classes, variant=name,
                 kernels_per_fwd_bwd=count_kernels(fn))
        return
    # the loss value must agree before the times are worth comparing
    ours = ops.cross_entropy(z, t, label_smoothing=eps).item()
    theirs = torch_soft_loss(z, t, eps).item()
    emit(what="loss_check", classes=classes, soft=ours, torch_soft=theirs)
    interleaved("loss_fwd_bwd", variants, reps, calls, batch=batch,
                classes=classes)


def main():
    global STEP_MS
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--step-ms", type=float, default=STEP_MS)
    ap.add_argument("--launches", action="store_true",
                    help="only count the kernels of each loss variant (torch "
                         "profiler); times taken in such a run mean nothing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench.py measures on a GPU; none found")
    STEP_MS = args.step_ms
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if not args.launches:
        gather_group(args.n, args.batch, dev, args.reps, args.calls)
    for classes in (10, 1000):
        loss_group(args.batch, classes, dev, args.reps, args.calls,
                   args.launches)


if __name__ == "__main__":
    main()

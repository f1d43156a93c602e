"""A/B of the two real-data input paths on one GPU (synthetic 50k x 32x32x3):

  host    DataLoader(device=) + to_model_layout: fp32 fancy-index gather on
          the CPU, pinned staging, H2D on a copy stream, then a permute +
          cast + contiguous on the GPU
  device  DeviceLoader: uint8 dataset resident in HBM, one gather_augment
          kernel per batch (with or without pad-4 crop + flip)

Measurements, each repeated --reps times with the variants interleaved in
the same process so run-to-run spread is visible next to the difference:

  (k) the kernel alone: HIP-event time per gather_augment call and the
      achieved GB/s over the bytes the algorithm needs (1 B in + 2 B out per
      element, plus index and label traffic)
  (a) loader only: one epoch of batches through to_model_layout, no model;
      images/s from HIP events around the epoch, median step time from
      events between steps
  (b) ResNet-18 training: wall time of one epoch with the train loop of
      cifar_example.py (zero_grad, forward, cross_entropy, backward, SGD
      step, loss.item()), host clock around a device synchronise

Prints one JSON line per measurement. Needs a GPU; there is no CPU fallback.

    python benchmarks/loader_bench.py --batches 8192,256 --reps 3
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mi355x import ops, optim  # noqa: E402
from mi355x.data import (Augment, DataLoader, DeviceLoader,  # noqa: E402
                         SyntheticImageDataset)
from mi355x.models import build_model  # noqa: E402
from mi355x.models.layers import to_model_layout  # noqa: E402
from mi355x.parallel.flat import FlatState  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make_loader(kind, ds, batch, dev):
    if kind == "host":
        return DataLoader(ds, batch_size=batch, shuffle=True, device=dev)
    aug = Augment() if kind == "device+aug" else None
    return DeviceLoader(ds, batch_size=batch, shuffle=True, device=dev,
                        augment=aug)


def kernel_alone(ds, batch, dev, reps, calls=50):
    dl = DeviceLoader(ds, batch_size=batch, device=dev)
    g = torch.Generator().manual_seed(0)
    idx = torch.randperm(len(ds), generator=g)[:batch].to(torch.int32).to(dev)
    H, W, C = dl.data_u8.shape[1:]
    nbytes = batch * (H * W * C * 3 + 4 + 8 + 8)
    for pad, flip in ((0, False), (4, True)):
        for _ in range(5):
            ops.gather_augment(dl.data_u8, dl.targets, idx, dl.scale,
                               dl.shift, pad=pad, flip=flip, epoch=1)
        for rep in range(reps):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for k in range(calls):
                ops.gather_augment(dl.data_u8, dl.targets, idx, dl.scale,
                                   dl.shift, pad=pad, flip=flip, epoch=k)
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / calls
            emit(what="kernel", batch=batch, pad=pad, flip=flip, rep=rep,
                 us_per_call=round(us, 2),
                 gb_per_s=round(nbytes / us / 1e3, 1))


def loader_epoch(dl):
    """One epoch through to_model_layout; (images, epoch ms, step ms list)."""
    evs = [torch.cuda.Event(enable_timing=True)]
    evs[0].record()
    n = 0
    for x, y in dl:
        x = to_model_layout(x)
        n += x.shape[0]
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        evs.append(ev)
    evs[-1].synchronize()
    steps = [a.elapsed_time(b) for a, b in zip(evs[:-1], evs[1:])]
    return n, evs[0].elapsed_time(evs[-1]), steps


def loader_only(ds, batch, dev, reps, kinds):
    loaders = {k: make_loader(k, ds, batch, dev) for k in kinds}
    for k in kinds:
        loader_epoch(loaders[k])  # warmup: pinned buffers, code objects
    for rep in range(reps):
        for k in kinds:
            n, ms, steps = loader_epoch(loaders[k])
            emit(what="loader_only", batch=batch, loader=k, rep=rep,
                 images=n, epoch_ms=round(ms, 2),
                 img_per_s=round(n / ms * 1e3),
                 step_ms_median=round(statistics.median(steps), 3))


def train_epoch(net, opt, dl, dev):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 0
    for inputs, labels in dl:
        inputs, labels = inputs.to(dev), labels.to(dev)
        opt.zero_grad()
        loss = ops.cross_entropy(net(inputs), labels)
        loss.backward()
        opt.step()
        loss.item()
        steps += 1
    torch.cuda.synchronize()
    return steps, time.perf_counter() - t0


def train(ds, batch, dev, reps, kinds):
    torch.manual_seed(0)
    net = build_model("resnet18").to(dev)
    opt = optim.SGD(FlatState(net), lr=0.001, momentum=0.9)
    loaders = {k: make_loader(k, ds, batch, dev) for k in kinds}
    for k in kinds:
        train_epoch(net, opt, loaders[k], dev)  # warmup epoch per loader
    for rep in range(reps):
        for k in kinds:
            steps, s = train_epoch(net, opt, loaders[k], dev)
            emit(what="train_epoch", batch=batch, loader=k, rep=rep,
                 steps=steps, epoch_s=round(s, 4),
                 img_per_s=round(len(ds) / s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--batches", default="8192,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench.py measures on a GPU; none found")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ds = SyntheticImageDataset(args.n, seed=1)
    kinds = ("host", "device", "device+aug")
    for batch in (int(b) for b in args.batches.split(",")):
        kernel_alone(ds, batch, dev, args.reps)
        loader_only(ds, batch, dev, args.reps, kinds)
        if not args.skip_train:
            train(ds, batch, dev, args.reps, kinds)


if __name__ == "__main__":
    main()

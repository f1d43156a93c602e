"""Flagship benchmark: ResNet-18 CIFAR-10 DDP training throughput (images/sec,
whole node) on MI355X — the BASELINE.json north-star metric.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
the driver launches it under torch.distributed.run with one rank per GPU
(RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* in env). W untimed warmup steps, then
exactly K timed steps bracketed by barrier + torch.cuda.synchronize on both
sides; elapsed is MAX over ranks; rank 0 prints ONE JSON line.

A plain run does only that: setup, warmup, the timed steps, the optional
`--dump-outputs DIR` (the last timed step's results as .npy, for comparing
two builds on identical seeded inputs), the result line. Any measurement
beyond the headline figure belongs behind `--full`.

The inputs repeat exactly, and so do the outputs: every split reduction
in the kernels (BN statistics, wgrads) stores per-block partials and folds
them in a fixed order, so two runs of one build with the same arguments
dump bit-identical arrays.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch

from mi355x import optim
from mi355x.models import build_model
from mi355x.ops import cross_entropy
from mi355x.parallel import DistributedDataParallel, comm
from mi355x.parallel.flat import FlatState


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int,
                    default=int(os.environ["MI355X_BENCH_BATCH"])
                    if "MI355X_BENCH_BATCH" in os.environ else None,
                    help="per-GPU batch size; default 8192 for 32-px "
                         "models, 2048 at 224 px (measured sweep: 94.5k "
                         "img/s at b1024 -> 107.6k at b4096 -> 111.5k at "
                         "b8192 eager on 1xMI355X)")
    ap.add_argument("--model", default=os.environ.get("MI355X_BENCH_MODEL",
                                                      "resnet18"))
    ap.add_argument("--size", type=int,
                    default=int(os.environ.get("MI355X_BENCH_SIZE", "32")),
                    help="image side (32 CIFAR, 224 config 4)")
    ap.add_argument("--classes", type=int, default=None)
    ap.add_argument("--sync-bn", action="store_true",
                    default=os.environ.get("MI355X_SYNC_BN", "0") == "1")
    ap.add_argument("--fp16", action="store_true",
                    default=os.environ.get("MI355X_FP16", "0") == "1")
    ap.add_argument("--graph", default=os.environ.get("MI355X_GRAPH", "auto"),
                    help="hipGraph-capture the train step: 1/0/auto. Auto "
                         "enables it only below batch 2048 — at large "
                         "batches the step is no longer launch-bound and "
                         "the graph's static-input copies are a net tax "
                         "(measured 109.9k eager vs 108.4k graphed at "
                         "b4096+)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, rank 0 writes what the last "
                         "timed step computed as DIR/<name>.npy (float32): "
                         "loss, logits, and the flat parameter and gradient "
                         "buffers the step updated (a fixed seeded sample "
                         "of the large ones, 64 MB at most in all)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (baselines, other configs, per-kernel "
                         "figures). None exist yet, so today this changes "
                         "nothing; later ones go behind it")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (ms_per_step is elapsed / steps)")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


# --dump-outputs element caps: 2 x 7M + 1M fp32 values stay under 64 MB
_DUMP_CAP = {"loss": 1, "logits": 1 << 20, "params": 7_000_000,
             "grads": 7_000_000}


N_POOL = 8  # synthetic batches, cycled: step i uses batch i % N_POOL


def synthetic_pool(batch, size, num_classes, rank=0):
    """The benchmark's inputs: N_POOL (images, labels) batches on the CPU,
    from one generator seeded by the rank alone, so they are the same in
    every run with the same arguments."""
    g = torch.Generator(device="cpu").manual_seed(4321 + rank)
    xs = [torch.randn(batch, 3, size, size, generator=g)
          for _ in range(N_POOL)]
    ys = [torch.randint(0, num_classes, (batch,), generator=g)
          for _ in range(N_POOL)]
    return xs, ys


def dump_outputs(dirname, tensors):
    """Write each tensor as <dirname>/<name>.npy in float32. Tensors larger
    than their cap are sampled at fixed seeded flat indices (sorted), so two
    builds run with the same arguments dump the same elements."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, t in tensors.items():
        flat = t.detach().reshape(-1)
        cap = _DUMP_CAP[name]
        if flat.numel() > cap:
            g = torch.Generator(device="cpu").manual_seed(97)
            idx = torch.randperm(flat.numel(), generator=g)[:cap].sort().values
            arr = flat[idx.to(flat.device)].float().cpu().numpy()
        else:
            arr = t.detach().float().cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), arr)


def main():
    args = parse_args()
    if args.batch is None:
        args.batch = 8192 if args.size < 224 else 2048
    use_cuda = torch.cuda.is_available()
    world = comm.env_world_size()
    distributed = world > 1
    if distributed:
        rank, world, local = comm.init_process_group()
    else:
        rank, local = 0, 0
    # modulo so oversubscribed layouts (more ranks than GPUs — rehearsal
    # on a 1-GPU box with gloo) land on a valid ordinal instead of dying
    # with "invalid device ordinal"
    device = (torch.device("cuda", local % torch.cuda.device_count())
              if use_cuda else torch.device("cpu"))
    if args.fp16:
        from mi355x import amp
        amp.set_compute_dtype(torch.float16)

    # conv->BN stats fusion (MI355X_FUSE_BN) defaults ON since round 2
    # (+0.9% r18 / +2.8% r50 after the shuffle stats fold + two-level
    # slab reduce; MI355X_FUSE_BN=0 disables)
    num_classes = args.classes or (1000 if args.size >= 224 else 10)
    model_name = args.model if args.size < 224 or args.model != "resnet18" \
        else "resnet18_imagenet"
    torch.manual_seed(1234)
    net = build_model(model_name, num_classes=num_classes).to(device)
    if args.sync_bn and distributed:
        from mi355x.parallel import sync_bn
        sync_bn.enable(net)
    if distributed:
        net = DistributedDataParallel(net)
        flat = net.flat
        gscale = net.grad_scale
    else:
        flat = FlatState(net)
        gscale = 1.0

    # graph decision up front: dynamic loss scaling takes a host-side
    # branch per step, so the graphed path keeps a static scale instead
    want_graph = (str(args.graph) == "1"
                  or (str(args.graph) == "auto" and args.batch < 2048))
    if distributed and os.environ.get("MI355X_GRAPH_DIST", "0") != "1":
        # world>1 graph capture (RCCL collectives inside hipGraph) is
        # untested on this pool — off unless explicitly requested
        want_graph = False
    use_graph = want_graph and use_cuda

    # fp16 (BASELINE config 5): DYNAMIC loss scaling via amp.GradScaler
    # (halve on overflow, grow on clean streaks), inf/nan scan over the
    # flat fp32 grad buffer post-all-reduce; 1/scale folds into the fused
    # SGD grad_scale. Graphed runs fall back to a static 256.0 scale.
    scaler = None
    loss_scale = 1.0
    if args.fp16:
        if use_graph:
            loss_scale = 256.0
        else:
            from mi355x import amp
            scaler = amp.GradScaler(
                init_scale=float(os.environ.get("MI355X_INIT_SCALE", 2.0**14)),
                growth_interval=int(os.environ.get("MI355X_GROWTH_INTERVAL",
                                                   "200")))
    optimizer = optim.SGD(flat, lr=0.1, momentum=0.9,
                          grad_scale=gscale / loss_scale)

    # synthetic on-device data pool (new batch each step, cycling)
    n_pool = N_POOL
    pool_x, pool_y = synthetic_pool(args.batch, args.size, num_classes, rank)
    pool_x = [t.to(device) for t in pool_x]
    pool_y = [t.to(device) for t in pool_y]

    # --dump-outputs: the step leaves its logits here (graphed runs: the
    # static tensor the replay writes)
    kept = {} if args.dump_outputs else None

    def run_step(x, y):
        optimizer.zero_grad()
        out = net(x)
        if kept is not None:
            kept["logits"] = out
        loss = cross_entropy(out, y)
        if scaler is not None:
            used = scaler.scale_value  # capture: step_ok may grow it
            (loss * used).backward()
            if distributed:
                net.finish_grad_sync()
            if scaler.step_ok(flat.flat_grad):
                optimizer.grad_scale = gscale / used
                optimizer.step()
            return loss
        (loss * loss_scale).backward() if loss_scale != 1.0 else loss.backward()
        if distributed:
            net.finish_grad_sync()
        optimizer.step()
        return loss

    if use_graph:
      try:
        # capture one full train step (launch-bound at CIFAR sizes: ~200
        # kernels/step; replay removes per-launch host cost + gaps). New
        # data each step is copied into the static input buffers.
        static_x = pool_x[0].clone()
        static_y = pool_y[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for i in range(3):  # warm up allocator/caches pre-capture
                run_step(static_x, static_y)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = run_step(static_x, static_y)

        def step(i):
            static_x.copy_(pool_x[i % n_pool])
            static_y.copy_(pool_y[i % n_pool])
            graph.replay()
            return static_loss
      except Exception as e:
        print(f"# graph capture failed ({e!r}); falling back to eager",
              flush=True)
        use_graph = False
    if not use_graph:
        def step(i):
            return run_step(pool_x[i % n_pool], pool_y[i % n_pool])

    for i in range(args.warmup):
        step(i)
    if distributed:
        comm.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(i)
    if use_cuda:
        torch.cuda.synchronize()
    if distributed:
        comm.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    t = torch.tensor([elapsed], dtype=torch.float64,
                     device=device if (distributed and use_cuda) else "cpu")
    if distributed:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {
            "loss": loss, "logits": kept["logits"],
            "params": flat.flat_param, "grads": flat.flat_grad})

    n_gpus = world if use_cuda else 0
    global_batch = args.batch * world
    images_per_sec = global_batch * args.steps / elapsed
    if rank == 0:
        print(json.dumps({
            "metric": ("images/sec (whole node), ResNet-18 CIFAR-10"
                       if args.model == "resnet18" and args.size == 32
                       else f"images/sec (whole node), {args.model} "
                            f"{args.size}x{args.size}"),
            "value": round(images_per_sec, 1),
            "unit": "images/sec",
            "n_gpus": n_gpus if use_cuda else world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp16" if args.fp16 else "bf16",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": global_batch,
                "image_size": args.size,
                "num_classes": num_classes,
                "parallelism": f"dp{world}",
                "sync_bn": bool(args.sync_bn),
                "hip_graph": bool(use_graph),
                "loss_scaling": (None if not args.fp16 else
                                 "static256" if scaler is None else
                                 f"dynamic(final={scaler.scale_value:g})"),
                "loss_final": round(float(loss.item()), 4),
            },
        }))
    if distributed:
        comm.destroy()


if __name__ == "__main__":
    main()

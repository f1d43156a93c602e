"""Distributed CIFAR-10 training — the reference's DDP script surface
(/root/reference/cifar_example_ddp.py) on the mi355x framework.

Same launcher env contract (RANK/LOCAL_RANK/WORLD_SIZE read from the
environment, MASTER_ADDR/PORT pinned to 127.0.0.1:29500 — single node,
like the reference's init_distributed at cifar_example_ddp.py:42-58), the
same --world_size CLI flag (env wins, as in the reference), per-rank batch
4, DistributedSampler with per-epoch set_epoch, our DDP wrap (flat-bucket
RCCL reducer), 'module.'-prefixed checkpoint keys. Conscious fixes of
reference bugs: eval tensors are moved to the device
(quirk 6), the checkpoint write is rank-0-gated (quirk 7), and the dead
`dataiter.next()` call is dropped (quirk 1), and a launcher-less run
works as world-1 instead of crashing in DistributedSampler (quirk 2 —
comm.init_process_group builds a 1-rank group).

Launch:  python -m mi355x.launcher --nproc-per-node 8 cifar_example_ddp.py
   (or)  torchrun --nproc-per-node 8 cifar_example_ddp.py

Env overrides (benchmark configs; CLI shape unchanged): MI355X_MODEL
(net, resnet18, resnet50, or mobilenet, which is CPU-only for now),
MI355X_SYNTHETIC, MI355X_BATCH, MI355X_EPOCHS, MI355X_STEPS, MI355X_LR,
MI355X_SYNC_BN=1, MI355X_FP16=1 (fp16 compute + dynamic loss scaling),
MI355X_CKPT (checkpoint path, default ./cifar_net.pth),
MI355X_DEVICE_DATA=1 (device-resident dataset for train and test),
MI355X_AUGMENT=1 (pad-4 random crop + flip on the train loader; needs
MI355X_DEVICE_DATA), MI355X_CLIP_NORM=<float> (global-norm gradient
clipping in the fused step; unset or 0 = off), MI355X_DEVICE_SCALER=1
(with MI355X_FP16=1: amp.DeviceGradScaler, loss scaling without a host
sync per step), MI355X_OPTIM=sgd|lars (default sgd; lars is optim.LARS, for
large batches), MI355X_LARS_ETA=<float> (LARS trust coefficient, default
0.001), MI355X_WD=<float> (weight decay of either optimizer, default 0),
MI355X_LABEL_SMOOTH=<float> (label smoothing of the training loss, default
0), MI355X_CUTMIX=<p> / MI355X_MIXUP=<p> (probability that a train sample
is cutmixed / mixed up with its partner in the rank's batch, default 0;
need MI355X_DEVICE_DATA, and the two sum to at most 1),
MI355X_SCHED=const|cosine|poly (learning-rate schedule over epochs *
len(train loader) steps with peak MI355X_LR, advanced on the device; default
const), MI355X_WARMUP_EPOCHS=<float> (linear warm-up from 0 in front of
cosine / poly, default 0), MI355X_EMA=<decay> (weight EMA in the fused step:
a second accuracy line, and rank 0 saves <ckpt stem>_ema.pth; unset or 0 =
off), MI355X_DEVICE_METER=1 (metrics.DeviceMeter: the training loss is read
from the device only where a line is printed, with no loss.item() per step
and no collective; an evaluation is one all-reduce and one read-back instead
of one per batch, and also prints test loss, top-5 and per-class accuracy).
"""

import argparse
import os
import time

import torch

from mi355x import optim
from mi355x.data import (CIFAR10, Augment, DataLoader, DeviceLoader,
                         DistributedSampler, SyntheticImageDataset)
from mi355x.metrics import DeviceMeter, DistAccuracy
from mi355x.models import build_model
from mi355x.ops import cross_entropy
from mi355x.parallel import DistributedDataParallel, comm, sync_bn


def init_distributed(args):
    # env contract, reference cifar_example_ddp.py:43-45; single-node
    # MASTER hard-wire, :55-56
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ.setdefault("MASTER_PORT", "29500")
    args.rank, args.world_size, args.gpu = comm.init_process_group()
    args.distributed = args.world_size > 1
    comm.barrier()


def get_datasets(args):
    if os.environ.get("MI355X_SYNTHETIC", "0") == "1":
        return (SyntheticImageDataset(50000, seed=1),
                SyntheticImageDataset(10000, seed=2))
    # rank-0-gated download + barrier — a conscious fix of reference quirk
    # 11, where every rank races on the download because dataset setup
    # precedes init_distributed (/root/reference/cifar_example_ddp.py:67-69)
    if args.rank == 0:
        from mi355x.data import download_cifar10
        download_cifar10("./data")
    comm.barrier()
    return CIFAR10("./data", train=True), CIFAR10("./data", train=False)


def main(args):
    init_distributed(args)
    trainset, testset = get_datasets(args)
    use_cuda = torch.cuda.is_available()
    device = (torch.device("cuda", args.gpu % torch.cuda.device_count())
              if use_cuda else torch.device("cpu"))

    batch = int(os.environ.get("MI355X_BATCH", "4"))
    epochs = int(os.environ.get("MI355X_EPOCHS", "2"))
    lr = float(os.environ.get("MI355X_LR", "0.001"))
    max_steps = int(os.environ.get("MI355X_STEPS", "0"))
    label_smooth = float(os.environ.get("MI355X_LABEL_SMOOTH", "0"))
    cutmix = float(os.environ.get("MI355X_CUTMIX", "0"))
    mixup = float(os.environ.get("MI355X_MIXUP", "0"))
    soft_loss = label_smooth > 0 or cutmix + mixup > 0

    sampler_train = DistributedSampler(trainset, num_replicas=args.world_size,
                                       rank=args.rank, shuffle=True)
    sampler_test = DistributedSampler(testset, num_replicas=args.world_size,
                                      rank=args.rank, shuffle=False)
    dev_for_loader = device if use_cuda else None
    if os.environ.get("MI355X_DEVICE_DATA", "0") == "1":
        # dataset resident on the device as uint8; one fused kernel per
        # batch. The draws key on the dataset index and the sampler's
        # epoch, so a sample augments the same on every rank.
        crop = os.environ.get("MI355X_AUGMENT", "0") == "1"
        augment = None
        if crop or cutmix + mixup > 0:
            # cutmix/mixup alone mix uncropped, unflipped samples
            try:
                augment = Augment(pad=4 if crop else 0, flip=crop,
                                  cutmix=cutmix, mixup=mixup)
            except ValueError as e:
                raise SystemExit(str(e))
        trainloader = DeviceLoader(trainset, batch_size=batch,
                                   sampler=sampler_train,
                                   device=dev_for_loader, augment=augment)
        testloader = DeviceLoader(testset, batch_size=batch,
                                  sampler=sampler_test, device=dev_for_loader)
    else:
        if os.environ.get("MI355X_AUGMENT", "0") == "1":
            raise SystemExit("MI355X_AUGMENT=1 needs MI355X_DEVICE_DATA=1")
        for knob, p in (("MI355X_CUTMIX", cutmix), ("MI355X_MIXUP", mixup)):
            if p > 0:
                raise SystemExit(f"{knob}={p:g} needs MI355X_DEVICE_DATA=1")
        trainloader = DataLoader(trainset, batch_size=batch,
                                 sampler=sampler_train, device=dev_for_loader)
        testloader = DataLoader(testset, batch_size=batch,
                                sampler=sampler_test, device=dev_for_loader)

    net = build_model(os.environ.get("MI355X_MODEL", "net")).to(device)
    if os.environ.get("MI355X_SYNC_BN", "0") == "1":
        sync_bn.enable(net)
    net = DistributedDataParallel(net)
    # BASELINE config 5: fp16 compute + dynamic loss scaling (overflow
    # skips the step and halves the scale; clean streaks grow it)
    scaler = None
    dev_scaler = None
    if os.environ.get("MI355X_FP16", "0") == "1":
        from mi355x import amp
        amp.set_compute_dtype(torch.float16)
        if os.environ.get("MI355X_DEVICE_SCALER", "0") == "1":
            # scale, overflow check and skip decision stay on the device:
            # no host sync in the step
            dev_scaler = amp.DeviceGradScaler(device=device)
        else:
            scaler = amp.GradScaler()
    elif os.environ.get("MI355X_DEVICE_SCALER", "0") == "1":
        raise SystemExit("MI355X_DEVICE_SCALER=1 needs MI355X_FP16=1")
    clip_norm = float(os.environ.get("MI355X_CLIP_NORM", "0")) or None
    try:
        ema = optim.ema_from_env()
        optimizer = optim.from_env(
            net.flat,
            lr=optim.schedule_from_env(lr, len(trainloader), epochs),
            momentum=0.9, grad_scale=net.grad_scale, max_grad_norm=clip_norm,
            ema=ema)
    except ValueError as e:
        raise SystemExit(str(e))
    if args.rank == 0 and any(k in os.environ for k in (
            "MI355X_OPTIM", "MI355X_WD", "MI355X_SCHED", "MI355X_EMA")):
        print("optimizer:", optim.describe(optimizer))

    meter = None
    if os.environ.get("MI355X_LOG_SPEED", "0") == "1":
        from mi355x.utils import SpeedMeter
        meter = SpeedMeter(print_every=100)

    # MI355X_DEVICE_METER=1: the loss window of the progress line and the
    # whole-run total live on the device; nothing is read back per step and
    # the reads are local (rank 0 prints its own loss, as below)
    device_meter = os.environ.get("MI355X_DEVICE_METER", "0") == "1"
    win_meter = run_meter = None

    t0 = time.time()
    steps = 0
    loss_sum = 0.0
    for epoch in range(epochs):
        sampler_train.set_epoch(epoch)
        running_loss = 0.0
        if win_meter is not None:
            # a new epoch starts a new window, as running_loss does
            run_meter.merge(win_meter)
            win_meter.reset()
        for i, (inputs, labels) in enumerate(trainloader):
            inputs, labels = inputs.to(device), labels.to(device)
            optimizer.zero_grad()
            outputs = net(inputs)
            # labels: a tensor, or a MixTarget under cutmix/mixup
            loss = cross_entropy(outputs, labels,
                                 label_smoothing=label_smooth)
            if scaler is not None:
                used = scaler.scale_value
                (loss * used).backward()
                net.finish_grad_sync()
                if scaler.step_ok(net.flat.flat_grad):
                    optimizer.grad_scale = net.grad_scale / used
                    optimizer.step()
            elif dev_scaler is not None:
                dev_scaler.scale(loss).backward()
                net.finish_grad_sync()
                optimizer.step(scaler=dev_scaler)
            else:
                loss.backward()
                net.finish_grad_sync()
                optimizer.step()

            if meter is not None:
                meter.step(inputs.shape[0])
            if device_meter:
                if win_meter is None:
                    win_meter, run_meter = (
                        DeviceMeter(outputs.shape[1], device=device)
                        for _ in range(2))
                win_meter.update(outputs, labels, loss=loss.detach())
                if i % 2000 == 1999:
                    if args.rank == 0:
                        print("[%d, %5d] loss: %.3f" %
                              (epoch + 1, i + 1,
                               win_meter.compute(sync=False)["loss"]))
                    run_meter.merge(win_meter)
                    win_meter.reset()
            else:
                step_loss = loss.item()
                running_loss += step_loss
                loss_sum += step_loss
                if i % 2000 == 1999 and args.rank == 0:
                    print("[%d, %5d] loss: %.3f" %
                          (epoch + 1, i + 1, running_loss / 2000))
                    running_loss = 0.0
            steps += 1
            if max_steps and steps >= max_steps:
                break
        if max_steps and steps >= max_steps:
            break
    if args.rank == 0:
        print(f"Finished Training ({steps} steps, {time.time() - t0:.1f}s)")
    if soft_loss and args.rank == 0:
        if run_meter is not None:
            # the one read of the run's total (row-weighted over the steps)
            run_meter.merge(win_meter)
            mean_loss = run_meter.compute(sync=False)["loss"]
        else:
            mean_loss = loss_sum / max(steps, 1)
        print("soft-target loss: label_smoothing=%g cutmix=%g mixup=%g, "
              "mean over the run %.4f" %
              (label_smooth, cutmix, mixup, mean_loss))

    PATH = os.environ.get("MI355X_CKPT", "./cifar_net.pth")
    if args.rank == 0:  # rank-gated (fixes reference quirk 7); keys keep
        torch.save(net.state_dict(), PATH)  # the 'module.' prefix

    def evaluate():
        accuracy = DistAccuracy(dist_sync_on_step=True, device=device)
        with torch.no_grad():
            for n, (images, labels) in enumerate(testloader):
                images, labels = images.to(device), labels.to(device)
                outputs = net(images)
                _, predicted = torch.max(outputs, 1)
                accuracy.update(predicted, labels)
                if max_steps and n >= max_steps:
                    break
        return accuracy.compute()

    meter_result = {}

    def evaluate_metered():
        # one meter per evaluation: one all-reduce and one read-back at its
        # end instead of one of each per batch
        meter = None
        with torch.no_grad():
            for n, (images, labels) in enumerate(testloader):
                images, labels = images.to(device), labels.to(device)
                outputs = net(images)
                if meter is None:
                    meter = DeviceMeter(outputs.shape[1], topk=5,
                                        confusion=True, device=device)
                meter.update(outputs, labels)
                if max_steps and n >= max_steps:
                    break
        meter_result.clear()
        meter_result.update(meter.compute())
        return meter_result["top1"]

    def print_meter_lines():
        r = meter_result
        print("Test loss: %.3f, top-5 accuracy: %.2f %%" %
              (r["loss"], 100 * r["top5"]))
        print("Per-class accuracy: " + " ".join(
            "%d: %.1f %%" % (c, 100 * a)
            for c, a in enumerate(r["per_class"].tolist())))

    run_eval = evaluate_metered if device_meter else evaluate

    net.eval()
    acc = run_eval()
    if args.rank == 0:
        # reference print format (/root/reference/cifar_example_ddp.py:135)
        print("Accuracy of the network on the 10000 test images: %d %%" %
              (100 * acc))
        if device_meter:
            print_meter_lines()
    if ema is not None:
        # the averaged weights, with the live BN running statistics; every
        # rank holds the same average, rank 0 saves it
        with ema.swapped():
            acc = run_eval()
            if args.rank == 0:
                print("Accuracy of the EMA weights on the 10000 test "
                      "images: %d %%" % (100 * acc))
                if device_meter:
                    print_meter_lines()
                stem, ext = os.path.splitext(PATH)
                torch.save(net.state_dict(), stem + "_ema" + ext)
    comm.destroy()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--world_size", default=None,
                        help="unused in distributed mode (env wins, as in "
                             "the reference)")
    main(parser.parse_args())

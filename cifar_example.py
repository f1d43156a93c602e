"""Single-process CIFAR-10 training — the reference's serial script surface
(/root/reference/cifar_example.py) on the mi355x framework.

Same CLI (no args), hyperparameters (batch 4, SGD lr=0.001 momentum=0.9,
2 epochs), print cadence (running loss every 2000 minibatches), checkpoint
path/format ('./cifar_net.pth', plain state_dict keys), and final accuracy
print. Differences are conscious fixes of reference bugs:
no dead `dataiter.next()` (removed API), no dead imshow/matplotlib.

Env overrides (benchmark configs; CLI shape unchanged):
  MI355X_MODEL=net|resnet18|resnet50|mobilenet  (default net; mobilenet
                                            is CPU-only: no depthwise GPU
                                            kernel yet)
  MI355X_SYNTHETIC=1                        synthetic 32x32 data (no download)
  MI355X_BATCH / MI355X_EPOCHS / MI355X_STEPS / MI355X_LR
  MI355X_DEVICE=cpu|cuda                    (default cpu, like the reference)
  MI355X_CKPT=path                          checkpoint path (default the
                                            reference's ./cifar_net.pth)
  MI355X_DEVICE_DATA=1                      device-resident dataset
                                            (DeviceLoader) for train and test
  MI355X_AUGMENT=1                          pad-4 random crop + flip on the
                                            train loader (needs DEVICE_DATA)
  MI355X_CLIP_NORM=<float>                  global-norm gradient clipping in
                                            the fused step (unset or 0 = off)
  MI355X_FP16=1 MI355X_DEVICE_SCALER=1      fp16 compute with
                                            amp.DeviceGradScaler: dynamic loss
                                            scaling, no host sync per step
  MI355X_OPTIM=sgd|lars                     optimizer (default sgd); lars is
                                            optim.LARS, for large batches
  MI355X_LARS_ETA=<float>                   LARS trust coefficient (default
                                            0.001)
  MI355X_WD=<float>                         weight decay of either optimizer
                                            (default 0)
  MI355X_LABEL_SMOOTH=<float>               label smoothing of the training
                                            loss (default 0)
  MI355X_CUTMIX=<p> MI355X_MIXUP=<p>        probability that a train sample is
                                            cutmixed / mixed up with its
                                            partner in the batch (default 0;
                                            need DEVICE_DATA, p's sum <= 1)
  MI355X_SCHED=const|cosine|poly            learning-rate schedule over
                                            epochs * len(train loader) steps,
                                            peak MI355X_LR, advanced on the
                                            device (default const)
  MI355X_WARMUP_EPOCHS=<float>              linear warm-up from 0 in front of
                                            cosine / poly (default 0)
  MI355X_EMA=<decay>                        weight EMA in the fused step; a
                                            second accuracy line and
                                            <ckpt stem>_ema.pth (unset or 0 =
                                            off)
  MI355X_DEVICE_METER=1                     metrics.DeviceMeter: the training
                                            loss is read from the device only
                                            where a line is printed (no
                                            loss.item() per step); evaluation
                                            reads back once and also prints
                                            test loss, top-5 and per-class
                                            accuracy
"""

import os
import time

import torch

from mi355x import optim
from mi355x.data import (CIFAR10, Augment, DataLoader, DeviceLoader,
                         SyntheticImageDataset)
from mi355x.metrics import DeviceMeter
from mi355x.models import build_model
from mi355x.ops import cross_entropy
from mi355x.parallel.flat import FlatState


def get_datasets():
    if os.environ.get("MI355X_SYNTHETIC", "0") == "1":
        return (SyntheticImageDataset(50000, seed=1),
                SyntheticImageDataset(10000, seed=2))
    # download=True bootstraps a clean box, like the reference's
    # torchvision.datasets.CIFAR10(root='./data', download=True)
    # (/root/reference/cifar_example.py:40-44)
    return (CIFAR10("./data", train=True, download=True),
            CIFAR10("./data", train=False, download=True))


def main():
    device = torch.device(os.environ.get("MI355X_DEVICE", "cpu"))
    batch = int(os.environ.get("MI355X_BATCH", "4"))
    epochs = int(os.environ.get("MI355X_EPOCHS", "2"))
    lr = float(os.environ.get("MI355X_LR", "0.001"))
    max_steps = int(os.environ.get("MI355X_STEPS", "0"))  # 0 = full epochs
    label_smooth = float(os.environ.get("MI355X_LABEL_SMOOTH", "0"))
    cutmix = float(os.environ.get("MI355X_CUTMIX", "0"))
    mixup = float(os.environ.get("MI355X_MIXUP", "0"))
    soft_loss = label_smooth > 0 or cutmix + mixup > 0

    trainset, testset = get_datasets()
    # num_workers=2 mirrors the reference surface (cifar_example.py:47,52);
    # our loader needs no worker processes (see mi355x/data.py)
    if os.environ.get("MI355X_DEVICE_DATA", "0") == "1":
        # dataset resident on the device as uint8; one fused kernel per
        # batch builds it (gather + crop/flip + normalize + NHWC 16-bit)
        crop = os.environ.get("MI355X_AUGMENT", "0") == "1"
        augment = None
        if crop or cutmix + mixup > 0:
            # cutmix/mixup alone mix uncropped, unflipped samples
            try:
                augment = Augment(pad=4 if crop else 0, flip=crop,
                                  cutmix=cutmix, mixup=mixup)
            except ValueError as e:
                raise SystemExit(str(e))
        trainloader = DeviceLoader(trainset, batch_size=batch, shuffle=True,
                                   device=device, augment=augment)
        testloader = DeviceLoader(testset, batch_size=batch, shuffle=False,
                                  device=device)
    else:
        if os.environ.get("MI355X_AUGMENT", "0") == "1":
            raise SystemExit("MI355X_AUGMENT=1 needs MI355X_DEVICE_DATA=1")
        for knob, p in (("MI355X_CUTMIX", cutmix), ("MI355X_MIXUP", mixup)):
            if p > 0:
                raise SystemExit(f"{knob}={p:g} needs MI355X_DEVICE_DATA=1")
        trainloader = DataLoader(trainset, batch_size=batch, shuffle=True,
                                 num_workers=2,
                                 device=device if device.type == "cuda" else None)
        testloader = DataLoader(testset, batch_size=batch, shuffle=False,
                                num_workers=2,
                                device=device if device.type == "cuda" else None)

    net = build_model(os.environ.get("MI355X_MODEL", "net")).to(device)
    flat = FlatState(net)
    clip_norm = float(os.environ.get("MI355X_CLIP_NORM", "0")) or None
    try:
        ema = optim.ema_from_env()
        optimizer = optim.from_env(
            flat, lr=optim.schedule_from_env(lr, len(trainloader), epochs),
            momentum=0.9, max_grad_norm=clip_norm, ema=ema)
    except ValueError as e:
        raise SystemExit(str(e))
    if any(k in os.environ for k in ("MI355X_OPTIM", "MI355X_WD",
                                     "MI355X_SCHED", "MI355X_EMA")):
        print("optimizer:", optim.describe(optimizer))
    dev_scaler = None
    if os.environ.get("MI355X_DEVICE_SCALER", "0") == "1":
        if os.environ.get("MI355X_FP16", "0") != "1":
            raise SystemExit("MI355X_DEVICE_SCALER=1 needs MI355X_FP16=1")
        # fp16 compute; scale, overflow check and skip decision stay on the
        # device: no host sync in the step
        from mi355x import amp
        amp.set_compute_dtype(torch.float16)
        dev_scaler = amp.DeviceGradScaler(device=device)

    meter = None
    if os.environ.get("MI355X_LOG_SPEED", "0") == "1":
        from mi355x.utils import SpeedMeter
        meter = SpeedMeter(print_every=100)

    # MI355X_DEVICE_METER=1: the loss window of the progress line and the
    # whole-run total live on the device; nothing is read back per step
    device_meter = os.environ.get("MI355X_DEVICE_METER", "0") == "1"
    win_meter = run_meter = None

    t0 = time.time()
    steps = 0
    loss_sum = 0.0
    for epoch in range(epochs):
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
            if dev_scaler is not None:
                dev_scaler.scale(loss).backward()
                optimizer.step(scaler=dev_scaler)
            else:
                loss.backward()
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
                    print("[%d, %5d] loss: %.3f" %
                          (epoch + 1, i + 1,
                           win_meter.compute(sync=False)["loss"]))
                    run_meter.merge(win_meter)
                    win_meter.reset()
            else:
                step_loss = loss.item()
                running_loss += step_loss
                loss_sum += step_loss
                if i % 2000 == 1999:
                    print("[%d, %5d] loss: %.3f" %
                          (epoch + 1, i + 1, running_loss / 2000))
                    running_loss = 0.0
            steps += 1
            if max_steps and steps >= max_steps:
                break
        if max_steps and steps >= max_steps:
            break
    print(f"Finished Training ({steps} steps, {time.time() - t0:.1f}s)")
    if soft_loss:
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
    torch.save(net.state_dict(), PATH)

    def evaluate_metered():
        # one meter per evaluation, one read-back at its end
        meter = None
        total = 0
        with torch.no_grad():
            for images, labels in testloader:
                images, labels = images.to(device), labels.to(device)
                outputs = net(images)
                if meter is None:
                    meter = DeviceMeter(outputs.shape[1], topk=5,
                                        confusion=True, device=device)
                meter.update(outputs, labels)
                total += labels.size(0)
                if max_steps and total >= max_steps * batch:
                    break
        r = meter.compute()
        # 100 * correct / total from the integer counts, as below
        r["accuracy"] = 100 * round(r["top1"] * r["rows"]) / max(r["rows"], 1)
        return r

    def print_meter_lines(r):
        print("Test loss: %.3f, top-5 accuracy: %.2f %%" %
              (r["loss"], 100 * r["top5"]))
        print("Per-class accuracy: " + " ".join(
            "%d: %.1f %%" % (c, 100 * a)
            for c, a in enumerate(r["per_class"].tolist())))

    def evaluate():
        correct = 0
        total = 0
        with torch.no_grad():
            for images, labels in testloader:
                images, labels = images.to(device), labels.to(device)
                outputs = net(images)
                _, predicted = torch.max(outputs, 1)
                total += labels.size(0)
                correct += (predicted == labels).sum().item()
                if max_steps and total >= max_steps * batch:
                    break
        return 100 * correct / max(total, 1)

    net.eval()
    if device_meter:
        r = evaluate_metered()
        print("Accuracy of the network on the 10000 test images: %d %%" %
              r["accuracy"])
        print_meter_lines(r)
    else:
        print("Accuracy of the network on the 10000 test images: %d %%" %
              evaluate())
    if ema is not None:
        # the averaged weights, with the live BN running statistics
        with ema.swapped():
            if device_meter:
                r = evaluate_metered()
                print("Accuracy of the EMA weights on the 10000 test images: "
                      "%d %%" % r["accuracy"])
                print_meter_lines(r)
            else:
                print("Accuracy of the EMA weights on the 10000 test images: "
                      "%d %%" % evaluate())
            stem, ext = os.path.splitext(PATH)
            torch.save(net.state_dict(), stem + "_ema" + ext)


if __name__ == "__main__":
    main()

"""Data pipeline.

MI355X-native replacements for the torchvision/torch.utils.data slice the
reference scripts pull in (reference: cifar_example.py:38-52,
cifar_example_ddp.py:61-76 — torchvision is not installed in this image, so
these are mandatory, not convenience):

  CIFAR10                on-disk-compatible reader of the cifar-10-batches-py
                         python-pickle batches, normalized (x/255-0.5)/0.5 to
                         float32 CHW exactly like the reference's
                         transforms.Compose([ToTensor, Normalize(.5,.5)])
                         (cifar_example.py:38-40).
  SyntheticImageDataset  CIFAR-shaped random data for benchmarks (no network
                         for the real set; BASELINE.json says synthetic).
  DistributedSampler     element-for-element parity with
                         torch.utils.data.distributed.DistributedSampler
                         (rank shard, pad-by-duplication, set_epoch reseed —
                         cifar_example_ddp.py:70-76,92).
  DataLoader             batching + per-epoch reshuffle; with device= it
                         stages batches through pinned host memory and copies
                         H2D asynchronously on a dedicated HIP stream one
                         batch ahead of consumption (the MI355X replacement
                         for worker processes + pin_memory: CIFAR batches are
                         tiny, so prefetch depth 1 on a copy stream hides the
                         whole transfer behind compute).
  DeviceLoader           the dataset lives in HBM as uint8 NHWC; each batch
                         is one fused HIP kernel (gather by sampler index,
                         pad-4 random crop + flip per Augment, normalize,
                         16-bit NHWC out) — no host work or H2D per step.
"""

from __future__ import annotations

import math
import os
import pickle
from typing import Optional, Sequence

import numpy as np
import torch

__all__ = [
    "CIFAR10",
    "download_cifar10",
    "SyntheticImageDataset",
    "DistributedSampler",
    "DataLoader",
    "augment_params",
    "mix_params",
    "MIX_NONE",
    "MIX_CUT",
    "MIX_UP",
    "Augment",
    "DeviceLoader",
]


# ---------------------------------------------------------------------------
# Datasets
# ---------------------------------------------------------------------------

_CIFAR_DIR = "cifar-10-batches-py"
_TRAIN_BATCHES = [f"data_batch_{i}" for i in range(1, 6)]
_TEST_BATCHES = ["test_batch"]

CIFAR10_URL = "https://www.cs.toronto.edu/~kriz/cifar-10-python.tar.gz"
CIFAR10_MD5 = "c58f30108f718f92721af3b95e74349a"

CIFAR10_CLASSES = (
    "plane", "car", "bird", "cat", "deer",
    "dog", "frog", "horse", "ship", "truck",
)


def _md5(path: str) -> str:
    import hashlib
    h = hashlib.md5()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def _batches_present(base: str) -> bool:
    return all(os.path.exists(os.path.join(base, n))
               for n in _TRAIN_BATCHES + _TEST_BATCHES)


def download_cifar10(root: str, url: str = CIFAR10_URL,
                     md5: str = CIFAR10_MD5) -> None:
    """Fetch + verify + extract CIFAR-10 into the torchvision on-disk layout
    (``<root>/cifar-10-batches-py/``) — the bootstrap the reference gets
    from torchvision.datasets.CIFAR10(download=True)
    (/root/reference/cifar_example.py:40-44). No-op if the batches are
    already in place. Callers in distributed jobs must gate this on rank 0
    and barrier (consciously fixing reference quirk 11: all ranks racing on
    the download, /root/reference/cifar_example_ddp.py:67-69)."""
    import tarfile
    import urllib.request

    base = os.path.join(root, _CIFAR_DIR)
    if _batches_present(base):
        return
    os.makedirs(root, exist_ok=True)
    tgz = os.path.join(root, os.path.basename(url) or "cifar-10-python.tar.gz")
    if not (os.path.exists(tgz) and _md5(tgz) == md5):
        part = tgz + ".part"
        urllib.request.urlretrieve(url, part)
        os.replace(part, tgz)
    got = _md5(tgz)
    if got != md5:
        raise RuntimeError(
            f"CIFAR-10 archive checksum mismatch at {tgz}: got {got}, "
            f"expected {md5} — delete the file and retry")
    with tarfile.open(tgz, "r:gz") as tf:
        try:
            tf.extractall(root, filter="data")
        except TypeError:  # tarfile without extraction filters
            for m in tf.getmembers():
                if m.name.startswith(("/", "..")) or ".." in m.name.split("/"):
                    raise RuntimeError(f"unsafe path in archive: {m.name}")
            tf.extractall(root)
    if not _batches_present(base):
        raise RuntimeError(
            f"CIFAR-10 archive extracted but batches missing under {base}")


class CIFAR10:
    """Reader for the standard CIFAR-10 python-pickle batch files.

    Accepts the same on-disk layout torchvision downloads
    (``<root>/cifar-10-batches-py/data_batch_{1..5}``, ``test_batch``; each a
    pickle with ``b"data"`` as (N, 3072) uint8 row-major RRR...GGG...BBB and
    ``b"labels"`` a list of ints).  ``download=True`` bootstraps a clean box
    via :func:`download_cifar10` (reference surface:
    torchvision.datasets.CIFAR10(root, download=True),
    /root/reference/cifar_example.py:40-44).  Samples come back as float32
    (3, 32, 32) tensors normalized to [-1, 1] — identical math to the
    reference's ToTensor + Normalize((0.5,)*3, (0.5,)*3)
    (cifar_example.py:38-40).
    """

    def __init__(self, root: str, train: bool = True, download: bool = False):
        if download:
            download_cifar10(root)
        base = os.path.join(root, _CIFAR_DIR)
        names = _TRAIN_BATCHES if train else _TEST_BATCHES
        datas, labels = [], []
        for name in names:
            path = os.path.join(base, name)
            with open(path, "rb") as f:
                d = pickle.load(f, encoding="bytes")
            datas.append(np.asarray(d[b"data"], dtype=np.uint8))
            labels.extend(int(v) for v in d[b"labels"])
        raw = np.concatenate(datas, axis=0).reshape(-1, 3, 32, 32)
        # (x/255 - 0.5)/0.5 == x * (2/255) - 1 : one fused pass, float32 CHW
        self.data = torch.from_numpy(raw.astype(np.float32) * (2.0 / 255.0) - 1.0)
        # the raw bytes as NHWC, for DeviceLoader (device-resident dataset)
        self.data_u8 = torch.from_numpy(
            np.ascontiguousarray(raw.transpose(0, 2, 3, 1)))
        self.targets = torch.tensor(labels, dtype=torch.int64)
        self.classes = list(CIFAR10_CLASSES)

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int):
        return self.data[i], self.targets[i]


class SyntheticImageDataset:
    """Random CIFAR-shaped data (float32 (3,32,32) in [-1,1], labels 0..9).

    Deterministic per seed so multi-process ranks materialize identical
    datasets without any exchange (BASELINE.json benchmarks run synthetic).
    """

    def __init__(self, n: int, seed: int = 0, size: int = 32,
                 channels: int = 3, num_classes: int = 10):
        g = torch.Generator().manual_seed(seed)
        self.data = torch.rand((n, channels, size, size), generator=g) * 2 - 1
        self.targets = torch.randint(0, num_classes, (n,), generator=g,
                                     dtype=torch.int64)
        self.classes = [str(i) for i in range(num_classes)]
        self._data_u8 = None

    @property
    def data_u8(self) -> torch.Tensor:
        """(N,H,W,C) uint8 view of ``.data`` for DeviceLoader, derived on
        first use as round((data+1)*127.5) — no generator call, so ``.data``
        and ``.targets`` are exactly what they were without it."""
        if self._data_u8 is None:
            q = torch.round((self.data + 1) * 127.5).clamp_(0, 255)
            self._data_u8 = q.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return self._data_u8

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int):
        return self.data[i], self.targets[i]


# ---------------------------------------------------------------------------
# DistributedSampler — torch-parity semantics
# ---------------------------------------------------------------------------

class DistributedSampler:
    """Rank-sharded epoch-seeded sampler, element-for-element equal to
    ``torch.utils.data.distributed.DistributedSampler`` (verified by
    tests/test_sampler.py): shuffled via ``torch.randperm`` seeded
    ``seed + epoch``, padded by duplication to a multiple of world size
    (reference behavior at cifar_example_ddp.py:70-76), strided subsample
    ``indices[rank::num_replicas]``.
    """

    def __init__(self, dataset, num_replicas: Optional[int] = None,
                 rank: Optional[int] = None, shuffle: bool = True,
                 seed: int = 0, drop_last: bool = False):
        if num_replicas is None:
            import torch.distributed as dist
            num_replicas = dist.get_world_size() if dist.is_initialized() else 1
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_initialized() else 0
        if not 0 <= rank < num_replicas:
            raise ValueError(f"rank {rank} out of range for world {num_replicas}")
        self.dataset = dataset
        self.num_replicas = num_replicas
        self.rank = rank
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        self.epoch = 0
        n = len(self.dataset)
        if self.drop_last and n % self.num_replicas != 0:
            self.num_samples = math.ceil((n - self.num_replicas) / self.num_replicas)
        else:
            self.num_samples = math.ceil(n / self.num_replicas)
        self.total_size = self.num_samples * self.num_replicas

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self) -> int:
        return self.num_samples

    def __iter__(self):
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            indices = torch.randperm(n, generator=g).tolist()
        else:
            indices = list(range(n))
        if not self.drop_last:
            pad = self.total_size - len(indices)
            if pad > 0:
                if pad <= len(indices):
                    indices += indices[:pad]
                else:
                    indices += (indices * math.ceil(pad / len(indices)))[:pad]
        else:
            indices = indices[: self.total_size]
        assert len(indices) == self.total_size
        return iter(indices[self.rank: self.total_size: self.num_replicas])


# ---------------------------------------------------------------------------
# DataLoader — batching + async H2D staging
# ---------------------------------------------------------------------------

class DataLoader:
    """Minimal loader over map-style datasets with tensor ``.data``/
    ``.targets`` fast path.

    * ``shuffle=True`` reshuffles every epoch (each ``__iter__`` advances an
      internal epoch counter — matches the reference DataLoader's fresh
      permutation per epoch, cifar_example.py:46-47).
    * ``sampler=`` takes precedence over ``shuffle`` (DDP path,
      cifar_example_ddp.py:69-76); ``set_epoch`` on the sampler is the
      caller's job, as in the reference (:92).
    * ``device=`` enables prefetch: the next batch is gathered into a pinned
      staging buffer and copied H2D on a dedicated stream while the current
      batch is being consumed, then handed over with a stream-wait (no sync).
    """

    def __init__(self, dataset, batch_size: int = 1, shuffle: bool = False,
                 sampler: Optional[Sequence[int]] = None,
                 drop_last: bool = False, device=None, seed: int = 0,
                 num_workers: int = 0):
        # num_workers is accepted for reference-surface parity
        # (cifar_example.py:47,52 passes num_workers=2). Worker PROCESSES
        # are deliberately not spawned: our datasets are fully materialized
        # tensors (no per-item decode), so batch gathering is one indexed
        # copy and the GPU path overlaps H2D on a copy stream instead —
        # there is no decode work to parallelize.
        self.num_workers = num_workers
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.sampler = sampler
        self.drop_last = drop_last
        self.device = torch.device(device) if device is not None else None
        self.seed = seed
        self._epoch = 0
        self._fast = hasattr(dataset, "data") and hasattr(dataset, "targets") \
            and isinstance(getattr(dataset, "data"), torch.Tensor)
        self._pinned = None  # (x, y) pinned staging buffers, lazily sized

    def __len__(self) -> int:
        if self.sampler is not None:
            n = len(self.sampler)
        else:
            n = len(self.dataset)
        if self.drop_last:
            return n // self.batch_size
        return math.ceil(n / self.batch_size)

    # -- index plan for this epoch ------------------------------------
    def _indices(self):
        if self.sampler is not None:
            return list(iter(self.sampler))
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self._epoch)
            return torch.randperm(n, generator=g).tolist()
        return list(range(n))

    def _gather(self, idx):
        if self._fast:
            t = torch.as_tensor(idx, dtype=torch.int64)
            return self.dataset.data[t], self.dataset.targets[t]
        xs, ys = zip(*(self.dataset[i] for i in idx))
        return torch.stack(xs), torch.as_tensor(ys, dtype=torch.int64)

    def __iter__(self):
        indices = self._indices()
        self._epoch += 1
        bs = self.batch_size
        batches = [indices[i: i + bs] for i in range(0, len(indices), bs)]
        if self.drop_last and batches and len(batches[-1]) < bs:
            batches.pop()
        if self.device is None or self.device.type != "cuda":
            for b in batches:
                yield self._gather(b)
            return
        yield from self._iter_device(batches)

    def _iter_device(self, batches):
        """Depth-1 pipelined H2D: gather batch k+1 into pinned staging and
        launch its copy on the copy stream while batch k computes.  Two
        pinned slots alternate; a slot is rewritten only after its previous
        H2D copy's event has completed (host-side sync on a copy that is
        already one full batch in the past, so it never actually blocks)."""
        stream = torch.cuda.Stream(device=self.device)
        if self._pinned is None:
            self._pinned = [None, None]
        slot_ev = [None, None]

        def stage(b, s):
            x, y = self._gather(b)
            if slot_ev[s] is not None:
                slot_ev[s].synchronize()  # pinned slot free for reuse?
            if self._pinned[s] is None or self._pinned[s][0].shape[0] < x.shape[0]:
                self._pinned[s] = (torch.empty_like(x).pin_memory(),
                                   torch.empty(y.shape, dtype=y.dtype).pin_memory())
            px = self._pinned[s][0][: x.shape[0]]
            py = self._pinned[s][1][: y.shape[0]]
            px.copy_(x)
            py.copy_(y)
            with torch.cuda.stream(stream):
                dx = px.to(self.device, non_blocking=True)
                dy = py.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            slot_ev[s] = ev
            return dx, dy, ev

        def handover(p):
            dx, dy, ev = p
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            # dx/dy were allocated on the copy stream; tell the caching
            # allocator they are consumed on the compute stream, else a
            # freed batch could be reused (and overwritten by a later H2D
            # copy) while compute still reads it.
            dx.record_stream(cur)
            dy.record_stream(cur)
            return dx, dy

        pending = None
        for k, b in enumerate(batches):
            nxt = stage(b, k & 1)
            if pending is not None:
                yield handover(pending)
            pending = nxt
        if pending is not None:
            yield handover(pending)


# ---------------------------------------------------------------------------
# Device-resident dataset: one fused gather/crop/flip/normalize kernel/batch
# ---------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)
_GOLDEN = 0x9E3779B9


def _mix32(h: np.ndarray) -> np.ndarray:
    """uint32 avalanche hash on uint64 carriers (products masked to 32 bits;
    uint64 multiplication wraps, so the low 32 bits are exact)."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & _M32
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & _M32
    h = h ^ (h >> np.uint64(16))
    return h


def augment_params(seed: int, epoch: int, indices, pad: int, flip: bool):
    """Crop offsets and flip bits of the samples ``indices`` in ``epoch``:
    ``(dy, dx, f)`` int64 tensors, dy/dx in [0, 2*pad], f in {0, 1}.

    Counter-based and keyed on the dataset index, so a sample's augmentation
    in an epoch is the same at any batch size, world size or rank. This is
    the CPU twin of the device function in csrc/augment.hip (uint32
    arithmetic throughout) and the oracle of its tests.
    """
    if not 0 <= pad <= 32767:  # dy/dx are 16.16 fixed-point uint32 products
        raise ValueError(f"pad must be in [0, 32767], got {pad}")
    i = np.asarray(torch.as_tensor(indices, dtype=torch.int64).numpy())
    if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
        raise ValueError("augment_params: index outside uint32 range")
    i = i.astype(np.uint64)
    key0 = ((int(seed) & 0xFFFFFFFF) * _GOLDEN + (int(epoch) & 0xFFFFFFFF)) \
        & 0xFFFFFFFF
    key = _mix32(np.array(key0, dtype=np.uint64))
    h = _mix32(i ^ key)
    h2 = _mix32((h + np.uint64(_GOLDEN)) & _M32)
    span = np.uint64(2 * pad + 1)
    dy = (((h & np.uint64(0xFFFF)) * span) & _M32) >> np.uint64(16)
    dx = (((h >> np.uint64(16)) * span) & _M32) >> np.uint64(16)
    f = (h2 & np.uint64(1)) if flip else np.zeros_like(h2)
    return tuple(torch.from_numpy(a.astype(np.int64)) for a in (dy, dx, f))


MIX_NONE, MIX_CUT, MIX_UP = 0, 1, 2


def _isqrt(n: np.ndarray) -> np.ndarray:
    """Exact floor square root of non-negative int64 values below 2^62: a
    double guess, off by at most one, then an integer correction."""
    s = np.sqrt(n.astype(np.float64)).astype(np.int64)
    s = s - (s * s > n)
    s = s + ((s + 1) * (s + 1) <= n)
    return s


def mix_params(seed: int, epoch: int, indices, H: int, W: int,
               cutmix: float, mixup: float):
    """CutMix / Mixup draws of the samples ``indices`` in ``epoch``, for
    H x W images: ``(mode, box, lam)``.

      mode  int64 (B,)    MIX_NONE, MIX_CUT or MIX_UP
      box   int64 (B,4)   cutmix rows [y0,y1) and columns [x0,x1), clipped
                          to the image; zeros for the other modes
      lam   float32 (B,)  weight of the sample's own image and label: 1 for
                          none, u/65536 for mixup, kept area/(H*W) for cutmix

    The draws continue augment_params' hash chain of the dataset index
    (h, h2 -> h3, h4), so they too are the same at any batch size, world
    size or rank; which sample is mixed IN is the loader's business (batch
    position B-1-b). lam is uniform: Beta(1,1), the setting both papers use
    on CIFAR; a general Beta(alpha) is not supported. This is the CPU twin
    of mix_draw in csrc/augment.hip and the oracle of its tests.
    """
    from mi355x.ops.functional import mix_thresholds

    tc, tm = mix_thresholds(cutmix, mixup)
    H, W = int(H), int(W)
    if not (1 <= H <= 1 << 23 and 1 <= W <= 1 << 23):
        raise ValueError("mix_params: H and W must be in [1, 2^23]")
    i = np.asarray(torch.as_tensor(indices, dtype=torch.int64).numpy())
    if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
        raise ValueError("mix_params: index outside uint32 range")
    i = i.astype(np.uint64)
    key0 = ((int(seed) & 0xFFFFFFFF) * _GOLDEN + (int(epoch) & 0xFFFFFFFF)) \
        & 0xFFFFFFFF
    key = _mix32(np.array(key0, dtype=np.uint64))
    h = _mix32(i ^ key)
    h2 = _mix32((h + np.uint64(_GOLDEN)) & _M32)
    h3 = _mix32((h2 + np.uint64(_GOLDEN)) & _M32)
    h4 = _mix32((h3 + np.uint64(_GOLDEN)) & _M32)
    r = (h3 & np.uint64(0xFFFF)).astype(np.int64)
    u = (h3 >> np.uint64(16)).astype(np.int64)
    mode = np.where(r < tc, MIX_CUT, np.where(r < tc + tm, MIX_UP, MIX_NONE))
    ch = _isqrt((H * H * (65536 - u)) >> 16)
    cw = _isqrt((W * W * (65536 - u)) >> 16)
    cy = ((h4 & np.uint64(0xFFFF)).astype(np.int64) * H) >> 16
    cx = ((h4 >> np.uint64(16)).astype(np.int64) * W) >> 16
    y0 = np.maximum(cy - ch // 2, 0)
    y1 = np.minimum(cy - ch // 2 + ch, H)
    x0 = np.maximum(cx - cw // 2, 0)
    x1 = np.minimum(cx - cw // 2 + cw, W)
    cut = mode == MIX_CUT
    box = np.stack([y0, y1, x0, x1], axis=1) * cut[:, None]
    keep = H * W - (y1 - y0) * (x1 - x0)
    # one float32 multiply by the rounded reciprocal, as the kernel does
    lam_cut = keep.astype(np.float32) * np.float32(1.0 / (H * W))
    lam_up = u.astype(np.float32) * np.float32(1.0 / 65536.0)
    lam = np.where(cut, lam_cut,
                   np.where(mode == MIX_UP, lam_up, np.float32(1.0)))
    return (torch.from_numpy(mode.astype(np.int64)),
            torch.from_numpy(box.astype(np.int64)),
            torch.from_numpy(lam.astype(np.float32)))


class Augment:
    """Train-time augmentation settings: zero-pad by ``pad`` and take a
    random crop of the original size, then flip horizontally with
    probability 1/2 (the torchvision RandomCrop(padding=pad) +
    RandomHorizontalFlip recipe). ``augment=None`` on a loader means none.

    ``cutmix`` / ``mixup`` are the probabilities that a sample is mixed with
    its partner in the batch (``ops.gather_augment_mix``); they must sum to
    at most 1. With either above 0 a DeviceLoader yields ``(x, MixTarget)``
    for ``ops.cross_entropy``; with both 0 nothing changes."""

    def __init__(self, pad: int = 4, flip: bool = True, cutmix: float = 0.0,
                 mixup: float = 0.0):
        self.pad = int(pad)
        self.flip = bool(flip)
        self.cutmix = float(cutmix)
        self.mixup = float(mixup)
        if not (0.0 <= self.cutmix <= 1.0 and 0.0 <= self.mixup <= 1.0
                and self.cutmix + self.mixup <= 1.0):
            raise ValueError(
                "cutmix and mixup must be probabilities with cutmix + mixup "
                f"<= 1, got {self.cutmix} and {self.mixup}")

    @property
    def mixes(self) -> bool:
        return self.cutmix + self.mixup > 0

    def __repr__(self) -> str:
        mix = (f", cutmix={self.cutmix}, mixup={self.mixup}"
               if self.mixes else "")
        return f"Augment(pad={self.pad}, flip={self.flip}{mix})"


class DeviceLoader:
    """Loader over a dataset that lives on the device as uint8 NHWC.

    Construction uploads ``dataset.data_u8`` / ``.targets`` once (CIFAR-10
    train is 150 MB). Each ``__iter__`` uploads the epoch's indices once as
    int32; every batch is then one ``ops.gather_augment`` call on the current
    stream over a slice of them: gather, pad+crop, flip, normalize with
    ``mean``/``std``, convert to the compute dtype, write NHWC. No host
    sync, H2D copy or pinned staging per batch.

    Same index plan as :class:`DataLoader` (sampler wins over ``shuffle``;
    ``randperm`` seeded ``seed + epoch``; ``drop_last``; ``__len__``). The
    augmentation epoch is the sampler's ``epoch`` when it has one (so
    ``set_epoch`` drives shuffle and augmentation together), else the
    loader's own counter.

    Yields ``(x, y)`` with x the NHWC buffer viewed as logical NCHW, so the
    models' ``to_model_layout`` permute back is contiguous already and
    copies nothing. ``device=None`` or a CPU device runs the CPU op (fp32).

    With ``Augment(cutmix=..., mixup=...)`` above 0 the batch is built by
    ``ops.gather_augment_mix`` instead (still one kernel) and the loader
    yields ``(x, MixTarget(y_a, y_b, lam))``; the partner of batch position
    b is position B-1-b of the same batch.
    """

    def __init__(self, dataset, batch_size: int = 1, shuffle: bool = False,
                 sampler: Optional[Sequence[int]] = None,
                 drop_last: bool = False, device=None,
                 augment: Optional[Augment] = None,
                 mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), seed: int = 0):
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.sampler = sampler
        self.drop_last = drop_last
        self.device = torch.device(device) if device is not None \
            else torch.device("cpu")
        self.augment = augment
        self.seed = seed
        self._epoch = 0
        data_u8 = dataset.data_u8
        C = data_u8.shape[3]
        mean64 = np.asarray(mean, dtype=np.float64).reshape(-1)
        std64 = np.asarray(std, dtype=np.float64).reshape(-1)
        if mean64.size != C or std64.size != C:
            raise ValueError(
                f"mean/std need one value per channel ({C}), got "
                f"{mean64.size}/{std64.size}")
        # (u8/255 - mean)/std == u8 * scale + shift
        self.scale = torch.from_numpy(
            (1.0 / (255.0 * std64)).astype(np.float32)).to(self.device)
        self.shift = torch.from_numpy(
            (-mean64 / std64).astype(np.float32)).to(self.device)
        self.data_u8 = data_u8.contiguous().to(self.device)
        self.targets = dataset.targets.to(torch.int64).to(self.device)

    def __len__(self) -> int:
        n = len(self.sampler) if self.sampler is not None \
            else len(self.dataset)
        if self.drop_last:
            return n // self.batch_size
        return math.ceil(n / self.batch_size)

    def _indices(self):
        if self.sampler is not None:
            return list(iter(self.sampler))
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self._epoch)
            return torch.randperm(n, generator=g).tolist()
        return list(range(n))

    def __iter__(self):
        from mi355x import ops

        idx = torch.as_tensor(self._indices(), dtype=torch.int64)
        aug_epoch = int(getattr(self.sampler, "epoch", self._epoch))
        self._epoch += 1
        n = self.data_u8.shape[0]
        # host-side bounds check, before anything is launched
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            bad = idx[(idx < 0) | (idx >= n)][0].item()
            raise IndexError(
                f"DeviceLoader: sampler index {bad} outside dataset of {n}")
        idx_dev = idx.to(torch.int32).to(self.device)
        pad = self.augment.pad if self.augment is not None else 0
        flip = self.augment.flip if self.augment is not None else False
        mixes = self.augment is not None and self.augment.mixes
        bs = self.batch_size
        total = idx.numel()
        for s in range(0, total, bs):
            e = min(s + bs, total)
            if self.drop_last and e - s < bs:
                break
            if mixes:
                # the pair kernel in place of the plain one: still one
                # launch per batch, and two labels plus a weight per row
                x, y_a, y_b, lam = ops.gather_augment_mix(
                    self.data_u8, self.targets, idx_dev[s:e], self.scale,
                    self.shift, pad=pad, flip=flip,
                    cutmix=self.augment.cutmix, mixup=self.augment.mixup,
                    seed=self.seed, epoch=aug_epoch)
                yield x.permute(0, 3, 1, 2), ops.MixTarget(y_a, y_b, lam)
                continue
            x, y = ops.gather_augment(
                self.data_u8, self.targets, idx_dev[s:e], self.scale,
                self.shift, pad=pad, flip=flip, seed=self.seed,
                epoch=aug_epoch)
            yield x.permute(0, 3, 1, 2), y

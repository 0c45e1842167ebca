"""Image dataset for the ResNet workloads: a directory of ``.npy`` files turned into
training batches on the device by one kernel launch per step (``ops/image.py``).

Format (``docs/get_started.md``): ``train_images.npy`` uint8 ``[N, Hs, Ws, 3]`` (NHWC,
RGB), ``train_labels.npy`` int64 ``[N]``, optional ``val_images.npy`` /
``val_labels.npy`` of the same ``Hs x Ws``, optional ``meta.json`` with
``num_classes``, ``mean`` and ``std`` (per channel, 0-255 units).

Batches are stateless: ``batch_at(step)`` is a pure function of ``(seed, step, B,
rank, world)`` and an image's augmentation in an epoch a function of ``(seed, epoch,
dataset index)`` only, so a resumed or re-sharded job sees the same crops.

A split is resident on the device when it fits the budget, otherwise staged: one
background thread gathers the next batch's images into a pinned buffer (two
buffers, one batch ahead), a non-blocking copy moves it up, and the same kernel
reads the staging buffer with ``index = 0..B-1``.
"""
from __future__ import annotations

import json
import math
import os
import queue
import threading
import weakref
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from ..ops.image import IMAGENET_MEAN, IMAGENET_STD, image_batch

AUGMENTS = ("rrc", "crop", "none")
RRC_SCALE = (0.08, 1.0)
RRC_RATIO = (3.0 / 4.0, 4.0 / 3.0)
RRC_TRIES = 10
CPU_RESIDENT_BYTES = 1 << 30  # automatic budget of a CPU run: keep splits up to 1 GiB in memory

_M64 = (1 << 64) - 1


def _mix_int(x: int) -> int:
    x &= _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _mix(x: np.ndarray) -> np.ndarray:
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def uniforms(seed: int, epoch: int, index: np.ndarray, streams: int) -> np.ndarray:
    """``[len(index), streams]`` uniforms in [0, 1): a counter hash (splitmix64
    finaliser) of ``(seed, epoch, dataset index, stream)`` and nothing else."""
    key = _mix_int(_mix_int(seed) ^ ((epoch + 1) * 0x9E3779B97F4A7C15))
    with np.errstate(over="ignore"):
        base = _mix(np.asarray(index, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + np.uint64(key))
        k = np.arange(1, streams + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        h = _mix(base[:, None] + k[None, :])
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def rrc_boxes(seed: int, epoch: int, index: np.ndarray, Hs: int, Ws: int):
    """Random-resized-crop boxes (torchvision's rule: scale (0.08, 1), log-uniform
    ratio (3/4, 4/3), 10 tries, then the centre fallback) and flips with p = 0.5.
    Returns int arrays ``(y0, x0, h, w, flip)`` and ``accepted`` (False: fallback)."""
    index = np.asarray(index)
    u = uniforms(seed, epoch, index, 4 * RRC_TRIES + 1)
    t = u[:, :4 * RRC_TRIES].reshape(-1, RRC_TRIES, 4)
    area = Hs * Ws * (RRC_SCALE[0] + (RRC_SCALE[1] - RRC_SCALE[0]) * t[:, :, 0])
    lr0, lr1 = math.log(RRC_RATIO[0]), math.log(RRC_RATIO[1])
    ratio = np.exp(lr0 + (lr1 - lr0) * t[:, :, 1])
    w = np.rint(np.sqrt(area * ratio)).astype(np.int64)
    h = np.rint(np.sqrt(area / ratio)).astype(np.int64)
    ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)
    first = np.argmax(ok, axis=1)
    accepted = ok.any(axis=1)
    rows = np.arange(len(index))
    h, w = h[rows, first], w[rows, first]
    y0 = np.floor(t[rows, first, 2] * (Hs - h + 1)).astype(np.int64)
    x0 = np.floor(t[rows, first, 3] * (Ws - w + 1)).astype(np.int64)
    in_ratio = Ws / Hs  # the fallback: the largest centred box whose ratio is in range
    if in_ratio < RRC_RATIO[0]:
        fw, fh = Ws, int(round(Ws / RRC_RATIO[0]))
    elif in_ratio > RRC_RATIO[1]:
        fh, fw = Hs, int(round(Hs * RRC_RATIO[1]))
    else:
        fw, fh = Ws, Hs
    fh, fw = min(fh, Hs), min(fw, Ws)
    h = np.where(accepted, h, fh)
    w = np.where(accepted, w, fw)
    y0 = np.where(accepted, np.minimum(y0, Hs - h), (Hs - fh) // 2)
    x0 = np.where(accepted, np.minimum(x0, Ws - w), (Ws - fw) // 2)
    flip = (u[:, -1] < 0.5).astype(np.int64)
    return y0, x0, h, w, flip, accepted


def _load_split(data_dir: str, split: str):
    pi, pl = (os.path.join(data_dir, f"{split}_{k}.npy") for k in ("images", "labels"))
    if not os.path.exists(pi):
        return None
    if not os.path.exists(pl):
        raise ValueError(f"{pi} has no {split}_labels.npy beside it")
    img, lab = np.load(pi, mmap_mode="r"), np.load(pl, mmap_mode="r")
    if img.dtype != np.uint8 or img.ndim != 4 or img.shape[3] != 3 or min(img.shape[:3]) < 1:
        raise ValueError(f"{pi}: expected uint8 [N, Hs, Ws, 3] (NHWC, RGB), got {img.dtype} {img.shape}")
    if not img.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{pi}: expected a C-contiguous array")
    if lab.dtype != np.int64 or lab.ndim != 1:
        raise ValueError(f"{pl}: expected int64 [N], got {lab.dtype} {lab.shape}")
    if lab.shape[0] != img.shape[0]:
        raise ValueError(f"{pl}: {lab.shape[0]} labels for {img.shape[0]} images")
    return img, np.array(lab)  # the labels are small: in memory


def has_dataset(data_dir: str) -> bool:
    return bool(data_dir) and os.path.exists(os.path.join(data_dir, "train_images.npy"))


def _stage_loop(images, req: "queue.Queue", done: "queue.Queue") -> None:
    """The prefetch thread: gather ``images[idx]`` into the buffer of each request.
    It holds the arrays and the queues, never the dataset, so the dataset can be
    collected while the thread waits; ``None`` ends it."""
    while True:
        item = req.get()
        if item is None:
            return
        key, idx, buf = item
        try:
            np.take(images, idx, axis=0, out=buf)
            done.put((key, None))
        except Exception as e:  # handed to the consumer
            done.put((key, e))


def _stop_stager(req: "queue.Queue", thread: threading.Thread) -> None:
    req.put(None)
    if thread is not threading.current_thread():
        thread.join(timeout=10.0)


class _Split:
    """One split's images either resident on the device or gathered per batch."""

    def __init__(self, images: np.ndarray, labels: np.ndarray):
        self.images, self.labels_np = images, labels
        self.N, self.Hs, self.Ws = images.shape[:3]
        self.nbytes = int(images.size)
        self.store = None      # resident: uint8 [N, Hs, Ws, 3] on the device
        self.labels = None     # resident: int64 [N] on the device
        self.device = torch.device("cpu")
        self.thread = None
        self._req = self._done = self._finalizer = None
        self._bufs, self._events, self._pending, self._slot = [], [None, None], None, 0

    def place(self, device: torch.device, resident: bool) -> None:
        self.close()
        self.device = device
        self.store = self.labels = None
        if not resident:
            return
        self.labels = torch.from_numpy(self.labels_np).to(device)
        self.store = torch.empty(self.images.shape, dtype=torch.uint8, device=device)
        rows = max(1, (256 << 20) // max(1, self.Hs * self.Ws * 3))  # upload in 256 MiB pieces
        for a in range(0, self.N, rows):
            self.store[a:a + rows].copy_(torch.from_numpy(np.array(self.images[a:a + rows])))

    # ---- staged
    def _buffers(self, B: int):
        if not self._bufs or self._bufs[0].shape[0] != B:
            pin = self.device.type == "cuda"
            self._bufs = [torch.empty((B, self.Hs, self.Ws, 3), dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
            self._events, self._pending = [None, None], None
        return self._bufs

    def _start(self) -> None:
        if self.thread is None:
            self._req, self._done = queue.Queue(), queue.Queue()
            self.thread = threading.Thread(target=_stage_loop, args=(self.images, self._req, self._done),
                                           name="kfa-image-stage", daemon=True)
            self.thread.start()
            self._finalizer = weakref.finalize(self, _stop_stager, self._req, self.thread)

    def _submit(self, key, idx: np.ndarray, B: int) -> None:
        slot = self._slot
        ev = self._events[slot]
        if ev is not None:  # the upload that last read this buffer has finished
            ev.synchronize()
            self._events[slot] = None
        self._req.put((key, idx, self._buffers(B)[slot].numpy()))
        self._pending = (key, slot)

    def _collect(self) -> int:
        key, slot = self._pending
        got, err = self._done.get()
        self._pending = None
        assert got == key, (got, key)
        if err is not None:
            raise err
        return slot

    def staged(self, key, idx: np.ndarray, next_key, next_idx: Optional[np.ndarray]):
        """``(store, labels)`` of the batch ``idx`` (identified by ``key``), prefetched
        if the previous call announced it; then the announced next batch is started."""
        B = len(idx)
        self._buffers(B)
        self._start()
        if self._pending is not None and self._pending[0] != key:
            self._collect()  # a jump (set_step): drop the stale prefetch
        if self._pending is None:
            self._submit(key, idx, B)
        slot = self._collect()
        self._slot = 1 - slot
        if next_idx is not None and len(next_idx) == B:
            self._submit(next_key, next_idx, B)
        buf = self._bufs[slot]
        lab = torch.from_numpy(self.labels_np[idx])
        if self.device.type != "cuda":
            return buf, lab
        lab = lab.pin_memory().to(self.device, non_blocking=True)
        dev = buf.to(self.device, non_blocking=True)
        self._events[slot] = torch.cuda.Event()
        self._events[slot].record()
        return dev, lab

    def close(self) -> None:
        if self._finalizer is not None:
            self._finalizer()  # stops and joins the thread (once)
        self.thread = self._finalizer = self._pending = None
        self._bufs, self._events = [], [None, None]


class ImageDataset:
    """See the module docstring.  ``out_hw``: the network's input size; ``augment``:
    ``rrc`` | ``crop`` (after ``crop_pad`` zero padding) | ``none`` (centre crop), the
    first two with a horizontal flip; ``data_resident_gb``: device budget in GB for
    resident splits (``None``: automatic, at most half of the free device memory at
    ``to()`` time; ``0`` forces staging)."""

    def __init__(self, data_dir: str, out_hw, augment: str = "rrc", crop_pad: int = 0, seed: int = 0,
                 rank: int = 0, world: int = 1, data_resident_gb: Optional[float] = None,
                 dtype: Optional[torch.dtype] = None):
        if augment not in AUGMENTS:
            raise ValueError(f"augment must be one of {AUGMENTS}, got {augment!r}")
        train = _load_split(data_dir, "train")
        if train is None:
            raise ValueError(f"{data_dir}: no train_images.npy")
        self.data_dir = data_dir
        self.train = _Split(*train)
        val = _load_split(data_dir, "val")
        self.val = _Split(*val) if val is not None else None
        if self.val is not None and (self.val.Hs, self.val.Ws) != (self.train.Hs, self.train.Ws):
            raise ValueError(f"{data_dir}: val images are {self.val.Hs}x{self.val.Ws}, train images "
                             f"{self.train.Hs}x{self.train.Ws}")
        meta = {}
        if os.path.exists(os.path.join(data_dir, "meta.json")):
            with open(os.path.join(data_dir, "meta.json")) as f:
                meta = json.load(f)
        top = int(self.train.labels_np.max()) if self.val is None else \
            max(int(self.train.labels_np.max()), int(self.val.labels_np.max()))
        self.num_classes = int(meta.get("num_classes", top + 1))
        if self.train.labels_np.min() < 0 or top >= self.num_classes:
            raise ValueError(f"{data_dir}: labels must lie in [0, {self.num_classes})")
        self.mean = tuple(float(v) for v in meta.get("mean", IMAGENET_MEAN))
        self.std = tuple(float(v) for v in meta.get("std", IMAGENET_STD))
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.augment, self.crop_pad, self.seed = augment, int(crop_pad), int(seed)
        self.rank, self.world = int(rank), int(world)
        self.data_resident_gb = data_resident_gb
        self.dtype = dtype
        self.device = torch.device("cpu")
        self._step = 0
        self._perms = {}
        self._placed = False

    # ---- placement
    @property
    def N(self) -> int:
        return self.train.N

    def set_shard(self, rank: int, world: int) -> "ImageDataset":
        self.rank, self.world = int(rank), int(world)
        return self

    def to(self, device) -> "ImageDataset":
        """Place the splits: resident while they fit the budget (train first), else staged."""
        self.device = torch.device(device)
        if self.data_resident_gb is not None and self.data_resident_gb >= 0:
            budget = int(self.data_resident_gb * 1e9)
        elif self.device.type == "cuda":
            budget = torch.cuda.mem_get_info(self.device)[0] // 2
        else:
            budget = CPU_RESIDENT_BYTES
        for sp in (self.train, self.val):
            if sp is None:
                continue
            resident = sp.nbytes <= budget
            sp.place(self.device, resident)
            if resident:
                budget -= sp.nbytes
        self._placed = True
        return self

    @property
    def resident(self) -> bool:
        self._ensure_placed()
        return self.train.store is not None

    def _ensure_placed(self) -> None:
        if not self._placed:
            self.to(self.device)

    def _out_dtype(self) -> torch.dtype:
        if self.dtype is not None:
            return self.dtype
        return torch.bfloat16 if self.device.type == "cuda" else torch.float32

    # ---- order
    def steps_per_epoch(self, B: int, world: Optional[int] = None) -> int:
        world = self.world if world is None else world
        if self.N < B * world:
            raise ValueError(f"{self.N} training images are fewer than one global batch ({B} x {world} replicas)")
        return self.N // (B * world)

    def _perm(self, epoch: int) -> np.ndarray:
        p = self._perms.get(epoch)
        if p is None:
            if len(self._perms) >= 2:
                self._perms.pop(min(self._perms))
            p = self._perms[epoch] = np.random.default_rng([self.seed, epoch]).permutation(self.N)
        return p

    def indices_at(self, step: int, B: int, rank: Optional[int] = None, world: Optional[int] = None):
        """``(epoch, dataset indices [B])`` of this rank's batch at ``step``."""
        rank = self.rank if rank is None else rank
        world = self.world if world is None else world
        spe = self.steps_per_epoch(B, world)
        epoch, s = divmod(int(step), spe)
        a = s * B * world + rank * B
        return epoch, self._perm(epoch)[a:a + B]

    # ---- augmentation tables
    def train_boxes(self, epoch: int, index: np.ndarray) -> np.ndarray:
        """``[len(index), 5]`` int64 rows ``(y0, x0, h, w, flip)``: a function of
        ``(seed, epoch, dataset index)`` only."""
        Hs, Ws = self.train.Hs, self.train.Ws
        Ho, Wo = self.out_hw
        n = len(index)
        if self.augment == "rrc":
            y0, x0, h, w, flip, _ = rrc_boxes(self.seed, epoch, index, Hs, Ws)
        elif self.augment == "crop":
            u = uniforms(self.seed, epoch, index, 3)
            P = self.crop_pad
            y0 = np.floor(u[:, 0] * (Hs + 2 * P - Ho + 1)).astype(np.int64) - P if Hs + 2 * P >= Ho \
                else np.full(n, (Hs - Ho) // 2)
            x0 = np.floor(u[:, 1] * (Ws + 2 * P - Wo + 1)).astype(np.int64) - P if Ws + 2 * P >= Wo \
                else np.full(n, (Ws - Wo) // 2)
            h, w, flip = np.full(n, Ho), np.full(n, Wo), (u[:, 2] < 0.5).astype(np.int64)
        else:
            return self.centre_boxes(n)
        return np.stack([y0, x0, h, w, flip], axis=1).astype(np.int64)

    def centre_boxes(self, n: int) -> np.ndarray:
        Ho, Wo = self.out_hw
        row = [(self.train.Hs - Ho) // 2, (self.train.Ws - Wo) // 2, Ho, Wo, 0]
        return np.tile(np.array(row, dtype=np.int64), (n, 1))

    # ---- batches
    def _build(self, sp: _Split, idx: np.ndarray, boxes: np.ndarray, key, next_key, next_idx):
        self._ensure_placed()
        B = len(idx)
        pin = self.device.type == "cuda"
        table = torch.empty((B, 6), dtype=torch.int32, pin_memory=pin)  # one small upload per step
        t = table.numpy()
        t[:, 1:] = boxes
        if sp.store is not None:
            t[:, 0] = idx
            store, labels = sp.store, sp.labels
        else:
            t[:, 0] = np.arange(B)
            store, labels = sp.staged(key, idx, next_key, next_idx)
        return image_batch(store, labels, table, self.mean, self.std, self.out_hw, self._out_dtype())

    def batch_at(self, step: int, B: int, rank: Optional[int] = None, world: Optional[int] = None):
        """The training batch ``(x, y)`` of ``step``: a pure function of ``(seed, step, B, rank, world)``."""
        self._ensure_placed()
        epoch, idx = self.indices_at(step, B, rank, world)
        nxt = None
        if self.train.store is None:  # staged: announce the next batch to the prefetch thread
            _, nxt = self.indices_at(step + 1, B, rank, world)
        key = (int(step), B, rank, world)
        return self._build(self.train, idx, self.train_boxes(epoch, idx), key, (int(step) + 1, B, rank, world), nxt)

    def next_batch(self, B: int):
        out = self.batch_at(self._step, B)
        self._step += 1
        return out

    def set_step(self, k: int) -> None:
        self._step = int(k)

    def eval_batches(self, B: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """Centre-crop batches over the val split in order; the last one may be partial."""
        if self.val is None:
            return
        self._ensure_placed()
        M = self.val.N
        for a in range(0, M, B):
            idx = np.arange(a, min(a + B, M))
            nxt = np.arange(a + B, min(a + 2 * B, M)) if a + B < M else None
            yield self._build(self.val, idx, self.centre_boxes(len(idx)), ("val", a), ("val", a + B), nxt)

    def describe(self) -> str:
        m = self.val.N if self.val is not None else 0
        return f"{self.data_dir}, {self.N} training images {self.train.Hs}x{self.train.Ws}, {m} validation images"

    def close(self) -> None:
        for sp in (self.train, self.val):
            if sp is not None:
                sp.close()


@torch.no_grad()
def evaluate(model, batches) -> Tuple[float, float, int]:
    """``(top-1 accuracy, mean cross entropy, images)`` over ``(x, y)`` batches, each
    batch weighted by its size."""
    import torch.nn.functional as F
    hit, ce, m = 0, 0.0, 0
    for x, y in batches:
        z = model(x).float()
        hit += int((z.argmax(1) == y).sum())
        ce += float(F.cross_entropy(z, y, reduction="sum"))
        m += int(y.shape[0])
    return (hit / m, ce / m, m) if m else (0.0, 0.0, 0)


# ---------------------------------------------------------------- synthetic directory
def class_colours(classes: int) -> np.ndarray:
    """``[classes, 3]`` RGB means in 0-255: a cubic grid, one point per class."""
    L = max(2, math.ceil(round(classes ** (1.0 / 3.0), 6)))
    c = np.arange(classes)
    grid = np.stack([c % L, (c // L) % L, (c // (L * L)) % L], axis=1)
    return 32.0 + grid * (192.0 / (L - 1))


def write_synthetic_dataset(out: str, n: int, size: int, classes: int, seed: int, n_val: Optional[int] = None) -> None:
    """A dataset directory from a seed: every image is its class colour plus
    zero-mean pixel noise, so the label can be read off the mean pixel."""
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(seed)
    pal = class_colours(classes)
    n_val = max(1, n // 4) if n_val is None else n_val
    for split, m in (("train", n), ("val", n_val)):
        if m <= 0:
            continue
        y = rng.integers(0, classes, size=m, dtype=np.int64)
        y[:min(m, classes)] = np.arange(min(m, classes))  # every class that fits appears
        x = np.lib.format.open_memmap(os.path.join(out, f"{split}_images.npy"), mode="w+", dtype=np.uint8,
                                      shape=(m, size, size, 3))
        rows = max(1, (32 << 20) // (size * size * 3))  # 32 MiB of pixels at a time
        for a in range(0, m, rows):
            noise = rng.integers(-8, 9, size=(len(y[a:a + rows]), size, size, 3), dtype=np.int16)
            x[a:a + rows] = np.clip(pal[y[a:a + rows]][:, None, None, :] + noise, 0, 255).astype(np.uint8)
        x.flush()
        del x
        np.save(os.path.join(out, f"{split}_labels.npy"), y)
    with open(os.path.join(out, "meta.json"), "w") as f:
        json.dump({"num_classes": classes, "mean": list(IMAGENET_MEAN), "std": list(IMAGENET_STD)}, f)

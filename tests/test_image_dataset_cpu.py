"""``ImageDataset`` on the CPU path: format errors, the stateless batch order,
random-resized-crop boxes, staged against resident batches, evaluation, and a
replica run on a dataset directory."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kubeflow_controller_amd.models import imagenet
from kubeflow_controller_amd.models.imagenet import ImageDataset, evaluate, rrc_boxes, write_synthetic_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SIZE, CLASSES = 103, 40, 10


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("images"))
    write_synthetic_dataset(d, N, SIZE, CLASSES, seed=3, n_val=21)
    return d


def _write(d, images, labels, split="train"):
    np.save(os.path.join(d, f"{split}_images.npy"), images)
    np.save(os.path.join(d, f"{split}_labels.npy"), labels)


def test_tool_writes_the_documented_format(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_dataset.py"), "--out", str(tmp_path),
                        "--n", "24", "--size", "16", "--classes", "5", "--seed", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    x, y = np.load(tmp_path / "train_images.npy"), np.load(tmp_path / "train_labels.npy")
    assert x.dtype == np.uint8 and x.shape == (24, 16, 16, 3) and y.dtype == np.int64 and y.shape == (24,)
    assert np.load(tmp_path / "val_images.npy").shape[1:] == (16, 16, 3)
    pal = imagenet.class_colours(5)
    mean = x.reshape(24, -1, 3).mean(1)
    assert np.array_equal(((mean[:, None] - pal[None]) ** 2).sum(2).argmin(1), y)  # label from the mean pixel
    assert ImageDataset(str(tmp_path), (16, 16)).num_classes == 5


@pytest.mark.parametrize("images, labels, what", [
    (np.zeros((4, 8, 8, 3), np.float32), np.zeros(4, np.int64), "uint8"),
    (np.zeros((4, 8, 8), np.uint8), np.zeros(4, np.int64), "NHWC"),
    (np.zeros((4, 3, 8, 8), np.uint8), np.zeros(4, np.int64), "NHWC"),
    (np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int32), "int64"),
    (np.zeros((4, 8, 8, 3), np.uint8), np.zeros(5, np.int64), "5 labels for 4 images"),
])
def test_format_errors_are_clear(tmp_path, images, labels, what):
    _write(str(tmp_path), images, labels)
    with pytest.raises(ValueError, match=what):
        ImageDataset(str(tmp_path), (8, 8))


def test_val_split_of_another_size_is_refused(tmp_path):
    _write(str(tmp_path), np.zeros((4, 8, 8, 3), np.uint8), np.zeros(4, np.int64))
    _write(str(tmp_path), np.zeros((2, 8, 9, 3), np.uint8), np.zeros(2, np.int64), "val")
    with pytest.raises(ValueError, match="8x9"):
        ImageDataset(str(tmp_path), (8, 8))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_an_epoch_is_one_permutation_split_over_the_ranks(data_dir, world):
    B = 8
    ds = ImageDataset(data_dir, (32, 32), seed=5)
    spe = ds.steps_per_epoch(B, world)
    assert spe == N // (B * world)
    seen = []
    for epoch in (0, 1):
        per_rank = [np.concatenate([ds.indices_at(epoch * spe + s, B, r, world)[1] for s in range(spe)])
                    for r in range(world)]
        flat = np.concatenate(per_rank)
        assert len(set(flat.tolist())) == len(flat) == spe * B * world  # disjoint over ranks and steps
        perm = np.random.default_rng([5, epoch]).permutation(N)
        tail = perm[spe * B * world:]
        assert sorted(flat.tolist() + tail.tolist()) == list(range(N))  # with the dropped tail: a permutation
        assert all(ds.indices_at(epoch * spe + s, B, 0, world)[0] == epoch for s in range(spe))
        seen.append(flat)
    assert not np.array_equal(seen[0], seen[1])


def test_batches_do_not_depend_on_the_sharding(data_dir):
    B = 6
    one = ImageDataset(data_dir, (32, 32), seed=9)
    two = [ImageDataset(data_dir, (32, 32), seed=9, rank=r, world=2) for r in range(2)]
    for step in (0, 3, N // (2 * B) + 1):  # the last one is in the second epoch
        x, y = one.batch_at(step, 2 * B)
        parts = [d.batch_at(step, B) for d in two]
        assert torch.equal(x, torch.cat([p[0] for p in parts])) and torch.equal(y, torch.cat([p[1] for p in parts]))
        again = ImageDataset(data_dir, (32, 32), seed=9).batch_at(step, 2 * B)
        assert torch.equal(x, again[0]) and torch.equal(y, again[1])  # the same seed repeats bit for bit
    other = ImageDataset(data_dir, (32, 32), seed=10).batch_at(0, 2 * B)
    assert not torch.equal(other[0], one.batch_at(0, 2 * B)[0])
    assert x.dtype == torch.float32 and x.shape == (2 * B, 3, 32, 32)
    assert x.is_contiguous(memory_format=torch.channels_last)


def test_set_step_then_next_batch_is_batch_at(data_dir):
    ds = ImageDataset(data_dir, (32, 32), seed=2)
    ds.set_step(7)
    a, b = ds.next_batch(8), ds.next_batch(8)
    assert torch.equal(a[0], ds.batch_at(7, 8)[0]) and torch.equal(b[0], ds.batch_at(8, 8)[0])
    assert torch.equal(b[1], ds.batch_at(8, 8)[1])


def test_fewer_images_than_one_global_batch_raises(data_dir):
    with pytest.raises(ValueError, match="fewer"):
        ImageDataset(data_dir, (32, 32), world=2).batch_at(0, 52)
    ImageDataset(data_dir, (32, 32), world=2, rank=1).batch_at(0, 51)


def test_augment_modes(data_dir):
    none = ImageDataset(data_dir, (32, 32), augment="none")
    assert np.array_equal(none.train_boxes(0, np.arange(5)), np.tile([4, 4, 32, 32, 0], (5, 1)))
    crop = ImageDataset(data_dir, (32, 32), augment="crop", crop_pad=4)
    b = crop.train_boxes(1, np.arange(4000))
    assert b[:, 0].min() == -4 and b[:, 0].max() == SIZE + 4 - 32 and b[:, 1].min() == -4
    assert (b[:, 2] == 32).all() and (b[:, 3] == 32).all() and 0.4 < b[:, 4].mean() < 0.6
    assert np.array_equal(b[100:200], crop.train_boxes(1, np.arange(100, 200)))  # a function of the index alone
    assert not np.array_equal(b, crop.train_boxes(2, np.arange(4000)))
    x, _ = crop.batch_at(0, 8)
    assert torch.isfinite(x).all()
    with pytest.raises(ValueError):
        ImageDataset(data_dir, (32, 32), augment="mixup")


def test_random_resized_crop_boxes():
    n, H, W = 100_000, 256, 256
    y0, x0, h, w, flip, accepted = rrc_boxes(11, 0, np.arange(n), H, W)
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    assert accepted.mean() > 0.99
    ha, wa = h[accepted].astype(float), w[accepted].astype(float)
    # h = round(sqrt(area / ratio)), w = round(sqrt(area * ratio)): each within 0.5 of its real value
    assert ((ha + 0.5) * (wa + 0.5) >= 0.08 * H * W).all() and ((ha - 0.5) * (wa - 0.5) <= H * W).all()
    assert ((wa + 0.5) / (ha - 0.5) >= 3 / 4).all() and ((wa - 0.5) / (ha + 0.5) <= 4 / 3).all()
    assert abs(flip.mean() - 0.5) <= 4 * 0.5 / np.sqrt(n)
    assert len(np.unique(h)) > 100 and len(np.unique(y0)) > 100
    again = rrc_boxes(11, 0, np.arange(500, 600), H, W)
    assert np.array_equal(again[2], h[500:600]) and np.array_equal(again[0], y0[500:600])
    # 300 x 10: no try fits (w >= round(sqrt(240 * 3/4)) = 13 > 10), so every box is the centre fallback
    y0, x0, h, w, flip, accepted = rrc_boxes(11, 0, np.arange(1000), 300, 10)
    assert not accepted.any()
    assert (w == 10).all() and (h == 13).all() and (x0 == 0).all() and (y0 == (300 - 13) // 2).all()
    assert 0.4 < flip.mean() < 0.6


def test_staged_batches_equal_resident_ones(data_dir):
    B = 8
    res = ImageDataset(data_dir, (32, 32), seed=4)
    stg = ImageDataset(data_dir, (32, 32), seed=4, data_resident_gb=0)
    assert res.resident and not stg.resident
    for step in range(2 * (N // B)):
        a, b = res.batch_at(step, B), stg.next_batch(B)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), step
    b = stg.batch_at(3, B)  # a jump drops the prefetched batch
    assert torch.equal(res.batch_at(3, B)[0], b[0])
    for a, b in zip(res.eval_batches(B), stg.eval_batches(B)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    thread = stg.train.thread
    assert thread is not None and thread.is_alive() and res.train.thread is None
    stg.close()
    assert not thread.is_alive()


def test_prefetch_thread_exits_on_garbage_collection(data_dir):
    ds = ImageDataset(data_dir, (32, 32), data_resident_gb=0)
    ds.next_batch(8)
    thread = ds.train.thread
    assert thread.is_alive()
    del ds
    gc.collect()
    thread.join(timeout=10)
    assert not thread.is_alive()


class _MeanColour(torch.nn.Module):
    """Logits = minus the squared distance of the mean pixel to each class colour."""

    def __init__(self, ds, classes):
        super().__init__()
        m, s = torch.tensor(ds.mean), torch.tensor(ds.std)
        self.pal = (torch.tensor(imagenet.class_colours(classes), dtype=torch.float32) - m) / s

    def forward(self, x):
        return -((x.float().mean((2, 3))[:, None] - self.pal[None]) ** 2).sum(2)


def test_eval_accuracy_and_cross_entropy(data_dir):
    ds = ImageDataset(data_dir, (32, 32))
    model = _MeanColour(ds, CLASSES)
    sizes = [y.shape[0] for _, y in ds.eval_batches(8)]
    assert sizes == [8, 8, 5]  # 21 validation images: the last batch is partial
    acc, ce, m = evaluate(model, ds.eval_batches(8))
    assert acc == 1.0 and m == 21
    xs, ys = zip(*ds.eval_batches(21))
    want = float(F.cross_entropy(model(xs[0]), ys[0]))
    assert ce == pytest.approx(want, rel=1e-5)
    # weighted by size: the plain mean of the three batch means is something else
    per = [float(F.cross_entropy(model(x), y)) for x, y in ds.eval_batches(8)]
    assert abs(np.mean(per) - want) > 1e-4 * want
    wrong = torch.nn.Sequential(model)
    model.pal = model.pal.roll(1, 0)
    assert evaluate(wrong, ds.eval_batches(8))[0] == 0.0
    assert ImageDataset(data_dir, (32, 32)).val.N == 21


def _replica(*args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "kubeflow_controller_amd.trainer.replica", "--device", "cpu", "--model",
           "resnet_tiny", "--train_steps", "4", "--batch_size", "8", "--optimizer", "sgd", "--learning_rate", "0.05",
           *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)


def test_replica_trains_on_a_dataset_directory(data_dir, tmp_path):
    r = _replica("--data_dir", data_dir)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"data ready: {data_dir}, {N} training images {SIZE}x{SIZE}, 21 validation images" in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("Validation: top-1 accuracy = ")]
    assert len(line) == 1 and line[0].endswith("over 21 images"), r.stdout
    assert "Final loss" in r.stdout
    d = _replica("--data_dir", data_dir, "--download_only")
    assert d.returncode == 0 and d.stdout.strip() == \
        f"data ready: {data_dir}, {N} training images {SIZE}x{SIZE}, 21 validation images"
    # an empty directory, or none, keeps the synthetic batch and today's log
    for extra in (["--data_dir", str(tmp_path)], []):
        s = _replica(*extra)
        assert s.returncode == 0, s.stdout + s.stderr
        assert "data ready" not in s.stdout and "Validation:" not in s.stdout and "Final loss" in s.stdout

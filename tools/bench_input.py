"""Input pipeline on one MI355X (profiles/input_pipeline.md):

1. ``kfa_image_batch`` time per batch at B = 256, 256x256 -> 224x224, direct
   (random crop + flip) and resample (random-resized-crop + flip) mode, against the
   bytes it must move: 77 MB of bf16 written plus the crop regions read;
2. the same batch built by the torch-op chain (gather, slice, flip, float,
   normalise, cast, channels-last; for resample ``F.interpolate`` per distinct box),
   the two sides alternated round by round;
3. with ``--replica``: ``resnet50`` replica images/s from a resident dataset, a
   staged one and the synthetic batch, interleaved (each a fresh process).

  python tools/bench_input.py [--rounds 5] [--replica --steps 40 --images 2048]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kubeflow_controller_amd.models.imagenet import rrc_boxes, write_synthetic_dataset  # noqa: E402
from kubeflow_controller_amd.ops.image import (IMAGENET_MEAN, IMAGENET_STD, _norm_consts, image_batch,  # noqa: E402
                                              launch)

B, HS, HO = 256, 256, 224


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def torch_chain(src, table, mean, inv):
    """The batch of ``table`` by torch ops; one slice per sample because every
    sample has its own box."""
    out = torch.empty((table.shape[0], 3, HO, HO), dtype=torch.bfloat16, device=src.device,
                      memory_format=torch.channels_last)
    for b, (idx, y0, x0, h, w, flip) in enumerate(table.tolist()):
        v = src[idx, y0:y0 + h, x0:x0 + w].permute(2, 0, 1).unsqueeze(0).float()
        if (h, w) != (HO, HO):
            v = F.interpolate(v, size=(HO, HO), mode="bilinear", align_corners=False)
        if flip:
            v = v.flip(3)
        out[b] = ((v - mean) * inv).to(torch.bfloat16)[0]
    return out


def torch_chain_batched(src, table, mean, inv):
    """Direct mode, the whole batch at once: one gather of the crop windows."""
    idx, y0, x0, flip = (table[:, k].long() for k in (0, 1, 2, 5))
    ar = torch.arange(HO, device=src.device)
    yy = (y0[:, None] + ar)[:, :, None]
    xx = torch.where(flip[:, None] != 0, x0[:, None] + HO - 1 - ar, x0[:, None] + ar)[:, None, :]
    v = src[idx[:, None, None], yy, xx].float()  # [B, HO, HO, 3]
    return ((v - mean.view(1, 1, 1, 3)) * inv.view(1, 1, 1, 3)).to(torch.bfloat16).permute(0, 3, 1, 2)


def kernels(rounds: int) -> None:
    d = torch.device("cuda")
    n = 1024
    src = torch.randint(0, 256, (n, HS, HS, 3), dtype=torch.uint8, device=d)
    labels = torch.arange(n, device=d)
    rng = np.random.default_rng(0)
    idx = rng.permutation(n)[:B]
    direct = np.stack([idx, rng.integers(0, HS - HO + 1, B), rng.integers(0, HS - HO + 1, B), np.full(B, HO),
                       np.full(B, HO), rng.integers(0, 2, B)], 1)
    y0, x0, h, w, flip, _ = rrc_boxes(0, 0, idx, HS, HS)
    resample = np.stack([idx, y0, x0, h, w, flip], 1)
    mean = torch.tensor(IMAGENET_MEAN, device=d).view(1, 3, 1, 1)
    inv = torch.tensor(IMAGENET_STD, device=d).reciprocal().view(1, 3, 1, 1)
    written = B * HO * HO * 3 * 2
    m32, i32 = (t.tolist() for t in _norm_consts(IMAGENET_MEAN, IMAGENET_STD))
    for name, tab in (("direct", direct), ("resample", resample)):
        host = torch.tensor(tab, dtype=torch.int32)
        dev = host.to(d)
        read = int((tab[:, 3] * tab[:, 4]).sum()) * 3
        x, y = image_batch(src, labels, host, IMAGENET_MEAN, IMAGENET_STD, (HO, HO))
        # the raw entry on a table already on the device: the launch alone, as the timed region
        ours = lambda: launch(src, labels, dev, host, x, y, m32, i32, HO, HO)  # noqa: E731
        chain = (lambda: torch_chain_batched(src, dev, mean, inv)) if name == "direct" else \
            (lambda: torch_chain(src, host, mean, inv))  # noqa: E731
        ours(), chain()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(rounds):  # sides alternated
            tk.append(timeit(ours, 20))
            tc.append(timeit(chain, 2))
        k, c = float(np.median(tk)), float(np.median(tc))
        print(f"{name}: kernel {k * 1e3:.1f} us per batch (min {min(tk) * 1e3:.1f}, max {max(tk) * 1e3:.1f}; "
              f"{(written + read) / k / 1e6:.0f} GB/s over {written / 1e6:.1f} MB written + {read / 1e6:.1f} MB read); "
              f"torch chain {c * 1e3:.1f} us (min {min(tc) * 1e3:.1f}, max {max(tc) * 1e3:.1f}); "
              f"ratio {c / k:.1f}x", flush=True)


def replica(steps: int, images: int, rounds: int) -> None:
    with tempfile.TemporaryDirectory() as tmp:
        write_synthetic_dataset(tmp, images, HS, 1000, seed=0, n_val=0)
        base = [sys.executable, "-m", "kubeflow_controller_amd.trainer.replica", "--model", "resnet50", "--batch_size",
                str(B), "--optimizer", "sgd", "--learning_rate", "0.1", "--momentum", "0.9", "--train_steps",
                str(steps), "--log_every", "0", "--graph", "off"]
        sides = {"resident": ["--data_dir", tmp], "staged": ["--data_dir", tmp, "--data_resident_gb", "0"],
                 "synthetic": []}
        got = {k: [] for k in sides}
        for _ in range(rounds):
            for name, extra in sides.items():
                r = subprocess.run(base + extra, capture_output=True, text=True, cwd=ROOT,
                                   env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
                m = re.search(r"Steady-state: .* ([\d.]+) examples/s", r.stdout)
                if r.returncode != 0 or not m:
                    raise SystemExit(f"{name} replica failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                got[name].append(float(m.group(1)))
                print(f"replica {name}: {got[name][-1]:.0f} images/s", flush=True)
        for name, v in got.items():
            print(f"replica {name}: median {np.median(v):.0f} images/s over {len(v)} runs (min {min(v):.0f}, "
                  f"max {max(v):.0f})")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replica", action="store_true", help="also time resnet50 replicas (three processes per round)")
    ap.add_argument("--replica_rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--no_kernels", action="store_true")
    a = ap.parse_args()
    if not a.no_kernels:
        kernels(a.rounds)
    if a.replica:
        replica(a.steps, a.images, a.replica_rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())

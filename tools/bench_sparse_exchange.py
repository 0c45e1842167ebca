"""Time the device-side embedding exchange kernels (csrc/kernels/sparse_exchange.hip)
against the ATen ops they replace, at the Wide&Deep workload's own shape.

One process, one GPU: n = 65,536 x 26 ids of ``synthetic_batch`` over ``CRITEO_LIKE``
(global rows), D = 72, world 8, owners 4.  After a warm-up every pair is timed with
device events, one repetition of each side in turn (``--reps`` of them, 50 by default):

* plan     vs  device ``torch.unique(sorted, return_inverse)`` + ``bincount``
* expand   vs  ``back.index_select(0, inv)``
* pre-sum  vs  ``zeros`` + ``index_add_(dout.float())`` + cast to bf16

and the host wall time of the CPU work in ``ShardedEmbedding.plan`` (key, ``torch.unique``,
``bincount``) on the same ids.  Prints a markdown table (median and minimum, us).
"""
import argparse
import statistics
import time

import torch

from kubeflow_controller_amd.models.wide_deep import CRITEO_LIKE, WideDeepConfig, synthetic_batch
from kubeflow_controller_amd.parallel import sparse_exchange as X


def alternate(sides, reps, warmup=5):
    """Per-repetition device times (us) of each callable, taken in turn."""
    for _ in range(warmup):
        for fn in sides:
            fn()
    torch.cuda.synchronize()
    evs = [[] for _ in sides]
    for _ in range(reps):
        for k, fn in enumerate(sides):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) * 1000 for a, b in e] for e in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dim", type=int, default=72)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--owners", type=int, default=4)
    args = ap.parse_args()
    cfg = WideDeepConfig()
    _, ids, _ = synthetic_batch(cfg, args.batch, torch.Generator().manual_seed(0))
    offs = torch.tensor([0] + list(CRITEO_LIKE[:-1])).cumsum(0)
    gids_cpu = (ids + offs.view(1, -1)).reshape(-1)
    n, D, W, O = gids_cpu.numel(), args.dim, args.world, args.owners
    num_rows = sum(CRITEO_LIKE)
    R = -(-num_rows // O)
    gids = gids_cpu.cuda()

    def aten_plan():
        key = (gids % O) * R + torch.div(gids, O, rounding_mode="floor")
        ukey, inv = torch.unique(key, sorted=True, return_inverse=True)
        return ukey, inv, torch.bincount(torch.div(ukey, R, rounding_mode="floor"), minlength=W)

    plan = X.build_plan(gids, W, O, R, num_rows).finish()
    ukey, inv64, counts = aten_plan()
    U = plan.U
    ok = (U == ukey.numel() and torch.equal(plan.inv.long(), inv64) and torch.equal(plan.counts.long(), counts)
          and torch.equal(plan.rows, ukey - torch.div(ukey, R, rounding_mode="floor") * R))
    g = torch.Generator().manual_seed(1)
    back = torch.randn(U, D, generator=g).to(torch.bfloat16).cuda()
    dout = torch.randn(n, D, generator=g).to(torch.bfloat16).cuda()

    def aten_presum():
        gu = torch.zeros(U, D, dtype=torch.float32, device="cuda")
        gu.index_add_(0, inv64, dout.float())
        return gu.to(torch.bfloat16)

    ok = ok and torch.equal(X.expand_rows(back, plan), back.index_select(0, inv64))
    diff = float((X.presum_rows(dout, plan).float() - aten_presum().float()).abs().max())
    rows = []
    for name, ours, aten in (
            ("plan", lambda: X.build_plan(gids, W, O, R, num_rows), aten_plan),
            ("expand", lambda: X.expand_rows(back, plan), lambda: back.index_select(0, inv64)),
            ("pre-sum", lambda: X.presum_rows(dout, plan), aten_presum)):
        a, b = alternate([ours, aten], args.reps)
        rows.append((name, statistics.median(a), min(a), statistics.median(b), min(b)))
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        key = (gids_cpu % O) * R + torch.div(gids_cpu, O, rounding_mode="floor")
        uk, _ = torch.unique(key, sorted=True, return_inverse=True)
        torch.bincount(torch.div(uk, R, rounding_mode="floor"), minlength=W)
        host.append((time.perf_counter() - t0) * 1e6)
    print(f"n = {n} ids ({args.batch} x {len(CRITEO_LIKE)}), {U} distinct ({100.0 * U / n:.1f} %), D = {D}, "
          f"world {W}, owners {O}; {args.reps} repetitions per side, taken in turn; outputs match: {ok}; "
          f"pre-sum max |HIP - ATen| = {diff:.3g}")
    print()
    print("| step | HIP median us | HIP min us | ATen median us | ATen min us | ATen / HIP (median) |")
    print("|---|---|---|---|---|---|")
    for name, am, amin, bm, bmin in rows:
        print(f"| {name} | {am:.1f} | {amin:.1f} | {bm:.1f} | {bmin:.1f} | {bm / am:.2f} |")
    print()
    print(f"host plan (CPU key + torch.unique + bincount, wall): median {statistics.median(host) / 1000:.1f} ms, "
          f"min {min(host) / 1000:.1f} ms")


if __name__ == "__main__":
    main()

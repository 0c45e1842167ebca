"""Device-side dedup / expand / pre-sum of the sharded embedding exchange
(``csrc/kernels/sparse_exchange.hip``, ``parallel/sparse_exchange.py``) against torch
on the CPU, and the ``exchange="device"`` lookup with two ranks sharing the GPU over
gloo (RCCL refuses two ranks on one device; ``tests/test_dp_gpu.py``).

The sizes cross the structures that can go wrong: the 64-entry pre-sum chunk, the
4096-entry radix and scan tiles, more than one radix pass, more than 64 K entries.
"""
import datetime
import functools
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

# name -> (n, num_rows, world, owners, ids)
CASES = {
    "n1": (1, 10, 2, 2, "zipf"),
    "n63": (63, 1000, 2, 2, "zipf"),
    "n64": (64, 1000, 2, 2, "zipf"),
    "n65": (65, 1000, 2, 2, "zipf"),
    "n4095": (4095, 1001, 3, 2, "zipf"),
    "n4096": (4096, 1001, 3, 2, "zipf"),
    "n4097": (4097, 1001, 3, 2, "zipf"),
    "equal": (12305, 1001, 4, 3, "equal"),
    "perm": (12305, 50000, 3, 3, "perm"),
    "even": (12305, 1000, 2, 2, "even"),
    "n70001": (70001, 5_000_000, 8, 4, "zipf"),
}
ROW_CASES = ("n4097", "equal", "n70001")   # expand / pre-sum: a tile edge, one run of 12305, 3 radix passes
DIMS = (8, 72, 248)


def _zipf(n, c, seed):
    """Power-law ids as ``models.wide_deep.synthetic_batch`` draws them."""
    u = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    return torch.clamp((c ** u).long() - 1, 0, c - 1)


def _ids(name):
    n, rows, _, _, kind = CASES[name]
    g = torch.Generator().manual_seed(11)
    if kind == "zipf":
        return _zipf(n, rows, 7)
    if kind == "equal":
        return torch.full((n,), 777, dtype=torch.int64)
    if kind == "perm":
        return torch.randperm(rows, generator=g)[:n]
    return torch.randint(0, rows // 2, (n,), generator=g) * 2


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ids, CPU reference, device plan) of a case, computed once and shared."""
    from kubeflow_controller_amd.parallel import sparse_exchange as X
    n, rows, world, owners, _ = CASES[name]
    R = -(-rows // owners)
    ids = _ids(name)
    key = (ids % owners) * R + ids // owners
    ukey, inv = torch.unique(key, sorted=True, return_inverse=True)
    ref = {"rows": ukey - (ukey // R) * R, "inv": inv, "counts": torch.bincount(ukey // R, minlength=world),
           "U": ukey.numel()}
    plan = X.build_plan(ids.cuda(), world, owners, R, rows).finish()
    return ids, ref, plan


def _grid(n, D, seed):
    """Values k / 8, |k| <= 16: exact in bf16, and every fp32 partial sum of up to 2^20 of
    them is exact in any order (16 n units of 1/8 stay below 2^24)."""
    k = torch.randint(-16, 17, (n, D), generator=torch.Generator().manual_seed(seed))
    return (k.float() / 8).to(torch.bfloat16)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_matches_torch_unique(name):
    ids, ref, plan = _case(name)
    n, _, world, _, _ = CASES[name]
    rows, inv, counts, seg = plan.rows, plan.inv, plan.counts, plan.seg_start
    torch.cuda.synchronize()
    assert plan.U == ref["U"]
    assert torch.equal(rows.cpu(), ref["rows"])
    assert torch.equal(inv.cpu().long(), ref["inv"])
    assert torch.equal(counts.cpu().long(), ref["counts"])
    seg = seg[:plan.U + 1].cpu().long()   # run bounds: the distinct keys' occurrence counts, in key order
    assert int(seg[0]) == 0 and int(seg[-1]) == n
    assert torch.equal(seg[1:] - seg[:-1], torch.bincount(ref["inv"], minlength=ref["U"]))
    send, recv = plan.split_sizes()
    assert send == ref["counts"].tolist() and len(recv) == world


def test_plan_of_no_ids_is_empty():
    from kubeflow_controller_amd.parallel import sparse_exchange as X
    plan = X.build_plan(torch.empty(0, dtype=torch.int64, device="cuda"), 2, 2, 500, 1000)
    assert plan.ws is None and plan.U == 0 and plan.rows.numel() == 0 and plan.inv.numel() == 0
    assert plan.split_sizes() == ([0, 0], [0, 0])
    back = torch.empty(0, 72, dtype=torch.bfloat16, device="cuda")
    assert tuple(X.expand_rows(back, plan).shape) == (0, 72)
    assert tuple(X.presum_rows(back, plan).shape) == (0, 72)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", ROW_CASES)
def test_expand_is_index_select(name, D):
    from kubeflow_controller_amd.parallel import sparse_exchange as X
    _, ref, plan = _case(name)
    back = torch.randn(ref["U"], D, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    got = X.expand_rows(back.cuda(), plan)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().view(torch.int16), back.index_select(0, ref["inv"]).view(torch.int16))


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", ROW_CASES)
def test_presum_exact_on_grid_values(name, D):
    from kubeflow_controller_amd.parallel import sparse_exchange as X
    n = CASES[name][0]
    _, ref, plan = _case(name)
    dout = _grid(n, D, 4)
    want = torch.zeros(ref["U"], D).index_add_(0, ref["inv"], dout.float()).to(torch.bfloat16)
    got = X.presum_rows(dout.cuda(), plan)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (ref["U"], D)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("name", ROW_CASES)
def test_presum_random_data_within_rounding_and_reproducible(name):
    """|got - ref| <= 2^-7 |ref| + 2^-20 sum|g| per element (one bf16 ulp + the fp32
    accumulation), fp64 reference; two calls give the same bits."""
    from kubeflow_controller_amd.parallel import sparse_exchange as X
    n, D = CASES[name][0], 72
    _, ref, plan = _case(name)
    dout = torch.randn(n, D, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    want = torch.zeros(ref["U"], D, dtype=torch.float64).index_add_(0, ref["inv"], dout.double())
    mag = torch.zeros(ref["U"], D, dtype=torch.float64).index_add_(0, ref["inv"], dout.double().abs())
    d = dout.cuda()
    a = X.presum_rows(d, plan).clone()
    b = X.presum_rows(d, plan)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    err = (a.cpu().double() - want).abs()
    tol = 2.0 ** -7 * want.abs() + 2.0 ** -20 * mag
    print(f"{name}: worst err/tol {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all()), float((err - tol).max())


def test_out_of_range_ids_raise_index_error():
    """Input validation: the plan kernels index by position, the bad ids only set the flag."""
    from kubeflow_controller_amd.parallel import sparse_exchange as X
    n, rows, world, owners = 4097, 1001, 3, 2
    ids = _zipf(n, rows, 9)
    ids[100], ids[3000] = rows, -1
    plan = X.build_plan(ids.cuda(), world, owners, -(-rows // owners), rows)
    with pytest.raises(IndexError, match=r"\[0, 1001\)"):
        plan.split_sizes()


# ------------------------------------------------------------------ two ranks on one GPU
N2, ROWS2, D2, LR2 = 4097, 1001, 72, 2.0 ** -6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    import torch.distributed as dist
    os.environ["KFA_COMM"] = "torch"
    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    # a failing rank ends the test instead of hanging it
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    return d


def _table_worker(rank, world, port, out):
    import torch.distributed as dist
    from kubeflow_controller_amd.parallel.comm import TorchComm
    from kubeflow_controller_amd.parallel.embedding import ShardedEmbedding
    d = _init(rank, world, port)
    emb = ShardedEmbedding(ROWS2, D2, owners=2, optimizer="sgd", lr=LR2, weight_decay=0.0, device=d,
                           exchange="device")
    emb.comm = TorchComm()
    w0 = emb.weight.detach().cpu().clone()
    ids = _zipf(N2, ROWS2, 300 + rank).to(d)
    rows = emb(ids)
    rows.backward(_grid(N2, D2, 400 + rank).to(d))
    torch.cuda.synchronize()
    torch.save({"w0": w0, "w": emb.weight.detach().cpu(), "rows": rows.detach().cpu(), "xb": emb.exchange_bytes},
               f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_table_lookup_and_update_exact(tmp_path):
    """Each rank looks up its own ids and pushes grid-valued gradients: the looked-up rows
    are the bf16 of the table's rows, and each owner's shard is, bit for bit, the CPU model
    w - lr * grad_scale * sum over senders of bf16(exact per-row sum)."""
    out = str(tmp_path / "t")
    mp.start_processes(_table_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = [torch.load(f"{out}.{r}", weights_only=True) for r in range(2)]
    full = torch.empty(ROWS2, D2)
    for r in range(2):
        full[r::2] = got[r]["w0"]
    total = torch.zeros(ROWS2, D2)
    for r in range(2):
        xb = got[r]["xb"]
        assert xb["path"] == "device" and xb["sent_ids"] < xb["lookups"] == N2, xb
        ids = _zipf(N2, ROWS2, 300 + r)
        assert torch.equal(got[r]["rows"].view(torch.int16), full[ids].to(torch.bfloat16).view(torch.int16))
        g = torch.zeros(ROWS2, D2).index_add_(0, ids, _grid(N2, D2, 400 + r).float())
        total += g.to(torch.bfloat16).float()
    want = full - (LR2 * total) * 0.5
    for r in range(2):
        assert torch.equal(got[r]["w"], want[r::2]), float((got[r]["w"] - want[r::2]).abs().max())


def _model_worker(rank, world, port, out, exchange):
    import torch.distributed as dist
    from kubeflow_controller_amd.models.wide_deep import (WideDeep, WideDeepConfig, prepare_batch, synthetic_batch,
                                                          wide_deep_loss)
    from kubeflow_controller_amd.trainer.engine import DistInfo, Engine
    d = _init(rank, world, port)
    cfg = WideDeepConfig.tiny()
    cfg.exchange, cfg.embed_lr = exchange, 1.0
    torch.manual_seed(0)
    m = WideDeep(cfg, device=d)
    m.tables.optimizer = "sgd"
    e = Engine(m, wide_deep_loss, optimizer="sgd", lr=0.05, momentum=0.0, weight_decay=0.0,
               compute_dtype=torch.bfloat16, channels_last=False, dist_info=DistInfo(rank=rank, world=world, device=d))
    init = [m.tables.full_table().cpu()] + [g.fp32.float().cpu().clone() for g in e.groups]
    dense, ids, labels = synthetic_batch(cfg, 512, torch.Generator().manual_seed(5))
    sl = slice(rank * 256, (rank + 1) * 256)
    for _ in range(2):
        batch = prepare_batch(m, dense[sl], ids[sl], labels[sl], d)
        assert hasattr(batch[1], "_kfa_plan") == (exchange == "host")
        e.train_step(*batch)
        assert m.tables.exchange_bytes["path"] == exchange, m.tables.exchange_bytes
    e.wait()
    torch.cuda.synchronize()
    end = [m.tables.full_table().cpu()] + [g.fp32.float().cpu() for g in e.groups]
    if rank == 0:
        torch.save({"init": init, "end": end}, out)
    dist.barrier()
    dist.destroy_process_group()


def _run_model(tmp_path, exchange, tag):
    out = str(tmp_path / f"m_{tag}.pt")
    mp.start_processes(_model_worker, args=(2, _free_port(), out, exchange), nprocs=2, join=True,
                       start_method="spawn")
    return torch.load(out, weights_only=True)


def _update_mismatch(a, b):
    """Worst |da - db| / (2 % of the element's own update + 1 % of the largest update)
    over the table and the dense groups (the bound of ``tests/test_dp_gpu.py`` for the
    same sums rounded to bf16 at different points)."""
    worst = 0.0
    for ia, ea, ib, eb in zip(a["init"], a["end"], b["init"], b["end"]):
        assert torch.equal(ia, ib)
        da, db = ea - ia, eb - ib
        assert float(db.abs().max()) > 0
        tol = 2e-2 * db.abs() + 1e-2 * float(db.abs().max())
        worst = max(worst, float(((da - db).abs() / tol).max()))
    return worst


def test_two_ranks_model_device_matches_host(tmp_path):
    """Wide&Deep (tiny) through the Engine, bf16 compute, SGD tables, two steps: the table
    and the dense weights move as with ``exchange="host"``.  Both paths send the same
    per-row sums, rounded to bf16 once; the host path's ``index_add_`` adds them in an
    arbitrary order.  Measured on an MI355X, worst mismatch as a fraction of the bound:
    host vs host 0.71 (``index_add_``'s atomics alone stay inside it, so the bound
    stands), device vs device 0, device vs host 0 (``profiles/sparse_exchange_b65536.md``)."""
    dev = _run_model(tmp_path, "device", "dev")
    host = _run_model(tmp_path, "host", "host")
    worst = _update_mismatch(dev, host)
    print(f"device vs host: worst mismatch / bound = {worst:.4f}")
    assert worst <= 1.0, worst

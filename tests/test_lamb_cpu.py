"""FusedLAMB and global-norm gradient clipping on the CPU path: against an fp64
reference of the formulas, across two gloo ranks, through a checkpoint round
trip, and the configurations that are refused."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

import _optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES_W = [(5,), (768,), (64, 33), (40, 41)]
SHAPES_B = [(11,), (768,)]


def _ref_adam_step(w, m, v, g, t, *, lr, b1, b2, eps, wd, gs):
    g = g.double() * gs
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    w.mul_(1 - lr * wd).sub_(lr * (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps))


def _groups():
    return R.cpu_groups(SHAPES_W, SHAPES_B)


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_cpu_lamb_matches_fp64_reference(max_norm):
    from kubeflow_controller_amd.ops.optim import FusedLAMB
    gw, gb = _groups()
    hp = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-6, wd=0.01)
    opt = FusedLAMB([gw, gb], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"],
                    max_grad_norm=max_norm)
    ref = [[p.detach().double().clone() for p in g.params] for g in (gw, gb)]
    rm = [[torch.zeros_like(x) for x in r] for r in ref]
    rv = [[torch.zeros_like(x) for x in r] for r in ref]
    gen = torch.Generator().manual_seed(11)
    for t in range(1, 5):
        grads = [[torch.randn(p.shape, generator=gen) for p in g.params] for g in (gw, gb)]
        R.set_grads((gw, gb), grads)
        opt.step(grad_scale=0.5)
        norm, coef = R.ref_clip([x for gs in grads for x in gs], 0.5, max_norm)
        for gi in range(2):
            for k in range(len(ref[gi])):
                R.ref_lamb_step(ref[gi][k], rm[gi][k], rv[gi][k], grads[gi][k], t,
                                **{**hp, "wd": hp["wd"] if gi == 0 else 0.0}, adapt=gi == 0, gs=0.5 * coef)
        if max_norm is not None:
            assert coef < 1.0  # the clip is active
            torch.testing.assert_close(opt.last_grad_norm.double(), norm, rtol=1e-5, atol=0)
    assert opt.last_grad_norm is None or opt.last_grad_norm.dim() == 0
    R.check_against((gw, gb), ([gw.fp32, gb.fp32], opt.m, opt.v),
                    [[[x.flatten() for x in r] for r in rs] for rs in (ref, rm, rv)])


def test_cpu_clipped_adam_matches_fp64_reference():
    from kubeflow_controller_amd.ops.optim import FusedAdam
    gw, gb = _groups()
    hp = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
    opt = FusedAdam([gw, gb], lr=hp["lr"], weight_decay=hp["wd"], max_grad_norm=1.0)
    ref = [[p.detach().double().clone() for p in g.params] for g in (gw, gb)]
    rm = [[torch.zeros_like(x) for x in r] for r in ref]
    rv = [[torch.zeros_like(x) for x in r] for r in ref]
    gen = torch.Generator().manual_seed(12)
    for t in range(1, 5):
        grads = [[torch.randn(p.shape, generator=gen) for p in g.params] for g in (gw, gb)]
        R.set_grads((gw, gb), grads)
        opt.step()
        norm, coef = R.ref_clip([x for gs in grads for x in gs], 1.0, 1.0)
        assert coef < 0.1
        torch.testing.assert_close(opt.last_grad_norm.double(), norm, rtol=1e-5, atol=0)
        for gi in range(2):
            for k in range(len(ref[gi])):
                _ref_adam_step(ref[gi][k], rm[gi][k], rv[gi][k], grads[gi][k], t,
                               **{**hp, "wd": hp["wd"] if gi == 0 else 0.0}, gs=coef)
    for gi, g in enumerate((gw, gb)):
        for k, p in enumerate(g.params):
            torch.testing.assert_close(p.detach().double(), ref[gi][k], atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------ two gloo ranks == one process
# the clip is active on every step: the gradient norm of this model stays above 0.3
DP_CLIP = 0.05


def _dp_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from kubeflow_controller_amd.ops.optim import FusedLAMB
    from kubeflow_controller_amd.parallel.ddp import GradSync, broadcast_params
    from kubeflow_controller_amd.parallel.flat import split_params
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = R.model()
    groups = split_params(model, None, pad_to=8 * world)
    broadcast_params(groups)
    sync = GradSync(groups, bucket_mb=0.0005)  # several buckets
    opt = FusedLAMB(sync.spaces(), lr=0.01, max_grad_norm=DP_CLIP)
    x, y = R.data()
    n = x.shape[0] // world
    norms = R.train(model, opt, sync, x[rank * n:(rank + 1) * n], y[rank * n:(rank + 1) * n], 5)
    torch.save({"sd": {k: v.clone() for k, v in model.state_dict().items()}, "norms": norms,
                "buckets": len(sync.buckets)}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_dp_lamb_clip_matches_single_process(tmp_path):
    from kubeflow_controller_amd.ops.optim import FusedLAMB
    from kubeflow_controller_amd.parallel.ddp import GradSync
    from kubeflow_controller_amd.parallel.flat import split_params
    out = str(tmp_path / "res")
    mp.start_processes(_dp_worker, args=(2, R.free_port(), out), nprocs=2, join=True, start_method="spawn")
    model = R.model()
    sync = GradSync(split_params(model, None))
    opt = FusedLAMB(sync.spaces(), lr=0.01, max_grad_norm=DP_CLIP)
    norms = R.train(model, opt, sync, *R.data(), 5)
    assert min(norms) > 2 * DP_CLIP, norms
    for r in range(2):
        got = torch.load(f"{out}.{r}", weights_only=True)
        assert got["buckets"] > 2
        torch.testing.assert_close(torch.tensor(got["norms"]), torch.tensor(norms), atol=2e-5, rtol=1e-4)
        for k, v in model.state_dict().items():
            torch.testing.assert_close(got["sd"][k], v, atol=2e-5, rtol=1e-4)


# ------------------------------------------------------------------ engine: checkpoint, refusals, flags
def _engine(**kw):
    from kubeflow_controller_amd.trainer.engine import DistInfo, Engine
    import torch.nn.functional as F
    kw.setdefault("optimizer", "lamb")
    return Engine(R.model(), lambda m, x, y: F.cross_entropy(m(x), y), lr=0.01, weight_decay=0.01, compute_dtype=None,
                  channels_last=False, dist_info=kw.pop("dist_info", DistInfo()), **kw)


def test_lamb_engine_checkpoint_round_trip_continues_bit_identically(tmp_path):
    from kubeflow_controller_amd.ops.optim import FusedLAMB
    x, y = R.data()
    a = _engine(max_grad_norm=DP_CLIP)
    assert isinstance(a.opt, FusedLAMB) and a.opt.max_grad_norm == DP_CLIP and not a.opt_overlap
    for _ in range(3):
        a.train_step(x, y)
    a.save(str(tmp_path), 3)
    b = _engine(max_grad_norm=DP_CLIP)
    assert b.restore(str(tmp_path)) == 3 and b.opt.step_count == 3
    for _ in range(2):
        a.train_step(x, y)
        b.train_step(x, y)
    for ga, gb in zip(a.groups, b.groups):
        assert torch.equal(ga.fp32, gb.fp32)
    for name in ("m", "v"):
        for ta, tb in zip(getattr(a.opt, name), getattr(b.opt, name)):
            assert torch.equal(ta, tb)
    assert torch.equal(a.opt.last_grad_norm, b.opt.last_grad_norm)


def test_overlap_is_off_for_lamb_and_clipping():
    assert _engine(optimizer="adam", opt_overlap=True).opt_overlap
    assert not _engine(optimizer="adam", opt_overlap=True, max_grad_norm=1.0).opt_overlap
    assert not _engine(optimizer="lamb", opt_overlap=True).opt_overlap


@pytest.mark.parametrize("kw", [dict(optimizer="lamb"), dict(optimizer="adam", max_grad_norm=1.0)])
def test_sharded_layout_refuses_lamb_and_clipping(kw):
    """ps > 0 at world > 1: refused before any collective (no process group exists here)."""
    from kubeflow_controller_amd.trainer.engine import DistInfo
    with pytest.raises(ValueError, match="shard"):
        _engine(ps=1, dist_info=DistInfo(rank=0, world=2), **kw)


def test_sgd_refuses_clipping():
    from kubeflow_controller_amd.ops.optim import FusedSGD
    gw, gb = _groups()
    with pytest.raises(ValueError, match="not built"):
        FusedSGD([gw, gb], lr=0.1, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="not built"):
        _engine(optimizer="sgd", max_grad_norm=1.0)
    FusedSGD([gw, gb], lr=0.1, max_grad_norm=None)


def test_lamb_refuses_a_space_without_segments():
    from kubeflow_controller_amd.ops.optim import FusedLAMB, OptSpace
    gw, _ = _groups()
    assert OptSpace.of_group(gw).segments == [(o, p.numel()) for o, p in zip(gw.offsets, gw.params)]
    shard = OptSpace("weights", torch.zeros(64), None, torch.zeros(64))
    assert shard.segments is None
    with pytest.raises(ValueError, match="segments"):
        FusedLAMB([shard])


@pytest.mark.parametrize("flags", [["--optimizer", "lamb"], ["--max_grad_norm", "1.0"]])
def test_async_ps_mode_refuses_lamb_and_clipping(flags):
    """mnist without --sync_replicas and with PS tasks is the async mode; refused before any connection."""
    from kubeflow_controller_amd.trainer import replica
    with pytest.raises(ValueError, match="async"):
        replica.main(["--model", "mnist_mlp", "--worker_hosts", "127.0.0.1:1,127.0.0.1:2", "--ps_hosts", "127.0.0.1:3",
                      "--job_name", "worker", "--task_index", "0", "--device", "cpu", *flags])


def test_replica_flags_parse():
    from kubeflow_controller_amd.trainer import replica
    ap = replica.build_parser()
    a = ap.parse_args(["--optimizer", "lamb", "--max_grad_norm", "1.0"])
    assert a.optimizer == "lamb" and a.max_grad_norm == 1.0
    a = ap.parse_args([])
    assert a.optimizer == "adam" and a.max_grad_norm is None


def test_replica_local_lamb_clip_trains(tmp_path):
    """A local replica with both flags runs the engine's LAMB step end to end (in process, CPU)."""
    from kubeflow_controller_amd.trainer import replica
    assert replica.main(["--model", "mnist_mlp", "--device", "cpu", "--optimizer", "lamb", "--max_grad_norm", "1.0",
                         "--train_steps", "3", "--batch_size", "16", "--log_every", "0"]) == 0

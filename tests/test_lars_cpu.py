"""FusedLARS on the CPU path: against an fp64 reference of its formula, across two gloo
ranks, through a checkpoint round trip, through the replica's flags, and the
configurations that are refused."""
import os
import re
import sys

import pytest
import torch
import torch.multiprocessing as mp

import _optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES_W = [(5,), (768,), (64, 33), (40, 41)]
SHAPES_B = [(11,), (768,)]
# lr and trust large enough that a wrong rate moves the weights far past the tolerance
HP = dict(lr=0.1, momentum=0.9, wd=0.01, trust=0.1, eps=1e-8)


def _groups():
    return R.cpu_groups(SHAPES_W, SHAPES_B)


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
def test_cpu_lars_matches_fp64_reference(max_norm, nesterov):
    from kubeflow_controller_amd.ops.optim import FusedLARS
    gw, gb = _groups()
    opt = FusedLARS([gw, gb], lr=HP["lr"], momentum=HP["momentum"], weight_decay=HP["wd"], trust=HP["trust"],
                    eps=HP["eps"], nesterov=nesterov, max_grad_norm=max_norm)
    assert opt.adapt_groups == {"weights"} and opt.trust_ratios[1] is None
    ref = [[p.detach().double().clone().flatten() for p in g.params] for g in (gw, gb)]
    rm = [[torch.zeros_like(x) for x in r] for r in ref]
    gen = torch.Generator().manual_seed(11)
    for _ in range(4):
        grads = [[torch.randn(p.shape, generator=gen) for p in g.params] for g in (gw, gb)]
        R.set_grads((gw, gb), grads)
        opt.step(grad_scale=0.5)
        norm, coef = R.ref_clip([x for gs in grads for x in gs], 0.5, max_norm)
        lams = [R.ref_lars_step(ref[0][k], rm[0][k], grads[0][k].flatten(), **HP, nesterov=nesterov, adapt=True,
                                gs=0.5 * coef) for k in range(len(ref[0]))]
        for k in range(len(ref[1])):
            R.ref_lars_step(ref[1][k], rm[1][k], grads[1][k].flatten(), **{**HP, "wd": 0.0}, nesterov=nesterov,
                            adapt=False, gs=0.5 * coef)
        torch.testing.assert_close(opt.trust_ratios[0].double(), torch.tensor(lams, dtype=torch.float64),
                                   rtol=1e-5, atol=0)
        if max_norm is not None:
            assert coef < 1.0  # the clip is active
            torch.testing.assert_close(opt.last_grad_norm.double(), norm, rtol=1e-5, atol=0)
    assert opt.step_count == 4
    assert opt.last_grad_norm is None or opt.last_grad_norm.dim() == 0
    R.check_against((gw, gb), ([gw.fp32, gb.fp32], opt.mom), (ref, rm))


def test_cpu_lars_without_adapting_groups_is_clipped_momentum_sgd():
    """adapt_groups=() under the clip threshold: FusedSGD(dampening=0)'s trajectory."""
    from kubeflow_controller_amd.ops.optim import FusedLARS, FusedSGD
    a, b = _groups(), _groups()
    lars = FusedLARS(a, lr=0.1, momentum=0.9, weight_decay=0.01, adapt_groups=(), max_grad_norm=1e4)
    sgd = FusedSGD(b, lr=0.1, momentum=0.9, weight_decay=0.01)
    assert lars.trust_ratios == [None, None]
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        for ga, gb in zip(a, b):
            ga.zero_grad()
            gb.zero_grad()
            for pa, pb in zip(ga.params, gb.params):
                x = torch.randn(pa.shape, generator=gen)
                pa.grad.copy_(x)
                pb.grad.copy_(x)
        lars.step()
        sgd.step()
    assert 1.0 < float(lars.last_grad_norm) < 1e4
    for ga, gb, ma, mb in zip(a, b, lars.mom, sgd.mom):
        torch.testing.assert_close(ga.fp32, gb.fp32, atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(ma, mb, atol=1e-6, rtol=1e-6)


# ------------------------------------------------------------------ two gloo ranks == one process
# the clip is active on every step: the gradient norm of this model stays above 0.3
DP_CLIP = 0.05
DP_HP = dict(lr=0.05, momentum=0.9, weight_decay=0.01, trust=0.1)


def _dp_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from kubeflow_controller_amd.ops.optim import FusedLARS
    from kubeflow_controller_amd.parallel.ddp import GradSync, broadcast_params
    from kubeflow_controller_amd.parallel.flat import split_params
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = R.model()
    groups = split_params(model, None, pad_to=8 * world)
    broadcast_params(groups)
    sync = GradSync(groups, bucket_mb=0.0005)  # several buckets
    opt = FusedLARS(sync.spaces(), max_grad_norm=DP_CLIP, **DP_HP)
    x, y = R.data()
    n = x.shape[0] // world
    norms = R.train(model, opt, sync, x[rank * n:(rank + 1) * n], y[rank * n:(rank + 1) * n], 5)
    torch.save({"sd": {k: v.clone() for k, v in model.state_dict().items()}, "norms": norms,
                "ratios": [r.clone() for r in opt.trust_ratios if r is not None],
                "buckets": len(sync.buckets)}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_dp_lars_clip_matches_single_process(tmp_path):
    from kubeflow_controller_amd.ops.optim import FusedLARS
    from kubeflow_controller_amd.parallel.ddp import GradSync
    from kubeflow_controller_amd.parallel.flat import split_params
    out = str(tmp_path / "res")
    mp.start_processes(_dp_worker, args=(2, R.free_port(), out), nprocs=2, join=True, start_method="spawn")
    model = R.model()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    sync = GradSync(split_params(model, None))
    opt = FusedLARS(sync.spaces(), max_grad_norm=DP_CLIP, **DP_HP)
    norms = R.train(model, opt, sync, *R.data(), 5)
    assert min(norms) > 2 * DP_CLIP, norms
    ratios = [r for r in opt.trust_ratios if r is not None]
    assert ratios and all(float((r - 1).abs().min()) > 0.1 for r in ratios)  # the rates are not the neutral 1
    for k, v in model.state_dict().items():  # the run moved every tensor well past the tolerance below
        assert float((v - before[k]).abs().max()) > 1e-3, k
    for r in range(2):
        got = torch.load(f"{out}.{r}", weights_only=True)
        assert got["buckets"] > 2
        torch.testing.assert_close(torch.tensor(got["norms"]), torch.tensor(norms), atol=2e-5, rtol=1e-4)
        for a, b in zip(got["ratios"], ratios):
            torch.testing.assert_close(a, b, atol=0, rtol=1e-4)
        for k, v in model.state_dict().items():
            torch.testing.assert_close(got["sd"][k], v, atol=2e-5, rtol=1e-4)


# ------------------------------------------------------------------ engine: checkpoint, refusals, flags
def _engine(**kw):
    from kubeflow_controller_amd.trainer.engine import DistInfo, Engine
    import torch.nn.functional as F
    kw.setdefault("optimizer", "lars")
    return Engine(R.model(), lambda m, x, y: F.cross_entropy(m(x), y), lr=0.05, weight_decay=0.01, compute_dtype=None,
                  channels_last=False, dist_info=kw.pop("dist_info", DistInfo()), **kw)


def test_lars_engine_checkpoint_round_trip_continues_bit_identically(tmp_path):
    from kubeflow_controller_amd.ops.optim import FusedLARS
    x, y = R.data()
    kw = dict(max_grad_norm=DP_CLIP, trust_coefficient=0.1, nesterov=True)
    a = _engine(**kw)
    assert isinstance(a.opt, FusedLARS) and a.opt.max_grad_norm == DP_CLIP and not a.opt_overlap
    assert a.opt.trust == 0.1 and a.opt.nesterov and a.opt.momentum == 0.9
    for _ in range(3):
        a.train_step(x, y)
    a.save(str(tmp_path), 3)
    b = _engine(**kw)
    assert b.restore(str(tmp_path)) == 3 and b.opt.step_count == 3
    for _ in range(2):
        a.train_step(x, y)
        b.train_step(x, y)
    for ga, gb in zip(a.groups, b.groups):
        assert torch.equal(ga.fp32, gb.fp32)
    assert any(float(m.abs().max()) > 0 for m in a.opt.mom)
    for ta, tb in zip(a.opt.mom, b.opt.mom):
        assert torch.equal(ta, tb)
    for ta, tb in zip(a.opt.trust_ratios, b.opt.trust_ratios):
        assert (ta is None and tb is None) or torch.equal(ta, tb)
    assert torch.equal(a.opt.last_grad_norm, b.opt.last_grad_norm)


def test_overlap_is_off_for_lars():
    assert _engine(optimizer="sgd", opt_overlap=True).opt_overlap
    assert not _engine(optimizer="lars", opt_overlap=True).opt_overlap


@pytest.mark.parametrize("kw", [dict(), dict(max_grad_norm=1.0)], ids=["noclip", "clip"])
def test_sharded_layout_refuses_lars(kw):
    """ps > 0 at world > 1: refused before any collective (no process group exists here)."""
    from kubeflow_controller_amd.trainer.engine import DistInfo
    with pytest.raises(ValueError, match="shard"):
        _engine(ps=1, dist_info=DistInfo(rank=0, world=2), **kw)


def test_lars_refuses_a_space_without_segments():
    from kubeflow_controller_amd.ops.optim import FusedLARS, OptSpace
    shard = OptSpace("weights", torch.zeros(64), None, torch.zeros(64))
    assert shard.segments is None
    with pytest.raises(ValueError, match="segments"):
        FusedLARS([shard])
    with pytest.raises(ValueError, match="positive"):
        FusedLARS(_groups(), max_grad_norm=0.0)


CLUSTER = ["--model", "mnist_mlp", "--worker_hosts", "127.0.0.1:1,127.0.0.1:2", "--ps_hosts", "127.0.0.1:3",
           "--job_name", "worker", "--task_index", "0", "--device", "cpu"]


def test_async_ps_mode_refuses_lars():
    """mnist without --sync_replicas and with PS tasks is the async mode; refused before any connection."""
    from kubeflow_controller_amd.trainer import replica
    with pytest.raises(ValueError, match="async"):
        replica.main([*CLUSTER, "--optimizer", "lars"])


def test_collective_layout_with_ps_tasks_refuses_lars():
    """--sync_replicas with PS tasks is the sharded collective layout; refused before any connection."""
    from kubeflow_controller_amd.trainer import replica
    with pytest.raises(ValueError, match="whole gradient"):
        replica.main([*CLUSTER, "--sync_replicas", "--optimizer", "lars"])


def test_replica_flags_parse():
    from kubeflow_controller_amd.trainer import replica
    ap = replica.build_parser()
    a = ap.parse_args(["--optimizer", "lars", "--trust_coefficient", "0.02", "--max_grad_norm", "1.0"])
    assert a.optimizer == "lars" and a.trust_coefficient == 0.02 and a.max_grad_norm == 1.0
    a = ap.parse_args([])
    assert a.optimizer == "adam" and a.trust_coefficient == 0.001
    with pytest.raises(ValueError, match="not built"):
        replica.main(["--model", "mnist_mlp", "--device", "cpu", "--optimizer", "sgd", "--max_grad_norm", "1.0"])


def _replica_validation_loss(capsys, steps):
    from kubeflow_controller_amd.trainer import replica
    assert replica.main(["--model", "mnist_mlp", "--device", "cpu", "--optimizer", "lars", "--max_grad_norm", "1.0",
                         "--learning_rate", "0.1", "--momentum", "0.9", "--trust_coefficient", "0.1",
                         "--train_steps", str(steps), "--batch_size", "32", "--log_every", "0"]) == 0
    m = re.search(r"validation cross entropy = ([0-9.eE+-]+)", capsys.readouterr().out)
    assert m, "the replica printed no validation loss"
    return float(m.group(1))


def test_replica_local_lars_clip_trains(capsys):
    """A local replica with the flags runs the engine's LARS step end to end (in process, CPU):
    the validation loss after 30 steps is below the one after 1 step of the same run."""
    first = _replica_validation_loss(capsys, 1)
    later = _replica_validation_loss(capsys, 30)
    assert later < 0.9 * first, (first, later)

"""FusedLAMB and device-side global-norm clipping on the GPU (csrc/kernels/optim.hip)
against an fp64 reference of the formulas written here.

Tolerances are those of tests/test_kernels_gpu.py::test_fused_adam_bf16_master: fp32
master weights atol = rtol = 1e-4, the bf16 compute copy atol 2e-2 / rtol 1e-2."""
import copy

import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

# 5: under one vector; 64x33: numel % 8 != 0; 300x300: several chunks and a ragged last one
# for any chunk size up to 64 K elements
SHAPES_W = [(5,), (768,), (64, 33), (300, 300)]
SHAPES_B = [(11,), (768,)]
HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-6, wd=0.01)


def _groups(wdtype, seed=7, shapes_w=SHAPES_W, init=None):
    """Two flat groups with a group tail (pad_to=64): "weights" in ``wdtype`` (bf16: with an
    fp32 master and a bf16 compute copy, bf16 gradients) and fp32 1-D "norms_biases"."""
    torch.manual_seed(seed)
    pw = [torch.nn.Parameter(torch.randn(*s, device=R.dev()).to(wdtype)) for s in shapes_w]
    pb = [torch.nn.Parameter(torch.randn(*s, device=R.dev())) for s in SHAPES_B]
    if init is not None:
        init(pw)
    return R.flat_pair(pw, pb)


def _rand_grads(groups, gen, scale=1.0):
    """Per group, per tensor: random gradients already rounded to the group's gradient dtype."""
    return [[(torch.randn(p.shape, generator=gen, device=R.dev()) * scale).to(g.grad.dtype) for p in g.params]
            for g in groups]


def _run_vs_reference(groups, opt, grads_per_step, *, wd, gscale=1.0, max_norm=None):
    """Step ``opt`` and the fp64 reference through the same gradients; compare w, m, v per
    tensor, the bf16 copy where there is one, and the padding, which must hold exact zeros."""
    ref = [[(g.fp32[o:o + p.numel()]).double().clone() for o, p in zip(g.offsets, g.params)] for g in groups]
    rm = [[torch.zeros_like(x) for x in r] for r in ref]
    rv = [[torch.zeros_like(x) for x in r] for r in ref]
    for t, grads in enumerate(grads_per_step, start=1):
        R.set_grads(groups, grads)
        opt.step(grad_scale=gscale)
        _, coef = R.ref_clip([x for gs in grads for x in gs], gscale, max_norm)
        for gi in range(len(groups)):
            for k in range(len(ref[gi])):
                R.ref_lamb_step(ref[gi][k], rm[gi][k], rv[gi][k], grads[gi][k].flatten(), t, lr=HP["lr"], b1=HP["b1"],
                                b2=HP["b2"], eps=HP["eps"], wd=wd if gi == 0 else 0.0, adapt=gi == 0,
                                gs=gscale * coef)
    torch.cuda.synchronize()
    R.check_against(groups, ([g.fp32 for g in groups], opt.m, opt.v), (ref, rm, rv))


@pytest.mark.parametrize("wdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
def test_lamb_matches_fp64_reference(wdtype, max_norm):
    from kubeflow_controller_amd.ops.optim import CHUNK, FusedLAMB
    assert CHUNK <= 65536 and 300 * 300 > CHUNK and (300 * 300) % CHUNK
    groups = _groups(wdtype)
    assert groups[0].numel > groups[0].offsets[-1] + 300 * 300  # a group tail exists
    assert groups[0].grad.dtype == wdtype
    opt = FusedLAMB(groups, lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"],
                    max_grad_norm=max_norm)
    gen = torch.Generator(device=R.dev()).manual_seed(5)
    steps = [_rand_grads(groups, gen) for _ in range(4)]
    _run_vs_reference(groups, opt, steps, wd=HP["wd"], gscale=0.5, max_norm=max_norm)
    if max_norm is not None:
        norm, coef = R.ref_clip([x for gs in steps[-1] for x in gs], 0.5, max_norm)
        assert coef < 0.1  # the clip was active
        torch.testing.assert_close(opt.last_grad_norm.double(), norm, rtol=1e-5, atol=0)


def test_lamb_trust_ratio_edge_cases():
    """|w| = 0 (an all-zero tensor) and |u| = 0 (zero gradient, wd = 0) both take r = 1."""
    from kubeflow_controller_amd.ops.optim import FusedLAMB

    def init(pw):
        pw[0].data.zero_()

    shapes = [(40, 9), (129,), (64, 33)]
    groups = _groups(torch.float32, seed=9, shapes_w=shapes, init=init)
    opt = FusedLAMB(groups, lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=0.0)
    gen = torch.Generator(device=R.dev()).manual_seed(6)
    steps = [_rand_grads(groups, gen) for _ in range(3)]
    for grads in steps:
        grads[0][1].zero_()  # tensor 1 of "weights": no gradient ever, so m = v = u = 0
    w1 = groups[0].params[1].detach().clone()
    _run_vs_reference(groups, opt, steps, wd=0.0)
    assert torch.equal(groups[0].params[1].detach(), w1)
    assert groups[0].params[0].detach().abs().max() > 0  # the zero tensor did move, with r = 1


def _state(groups, opt):
    return [g.fp32.clone() for g in groups] + [x.clone() for x in opt.m + opt.v] + [opt.last_grad_norm.clone()]


def test_lamb_step_is_bit_repeatable():
    from kubeflow_controller_amd.ops.optim import FusedLAMB
    gen = torch.Generator(device=R.dev()).manual_seed(8)
    out = []
    steps = None
    for _ in range(2):
        groups = _groups(torch.bfloat16)
        opt = FusedLAMB(groups, lr=HP["lr"], eps=HP["eps"], weight_decay=HP["wd"], max_grad_norm=1.0)
        if steps is None:
            steps = [_rand_grads(groups, gen) for _ in range(3)]
        for grads in steps:
            R.set_grads(groups, grads)
            opt.step()
        torch.cuda.synchronize()
        assert float(opt.last_grad_norm) > 10.0  # clipping active
        out.append(_state(groups, opt))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_adam_clipping_matches_torch():
    from kubeflow_controller_amd.ops.optim import FusedAdam
    groups = _groups(torch.float32)
    refs = [[torch.nn.Parameter(p.detach().clone()) for p in g.params] for g in groups]
    opt = FusedAdam(groups, lr=1e-2, weight_decay=0.1, max_grad_norm=1.0)
    topt = torch.optim.AdamW([{"params": refs[0], "weight_decay": 0.1}, {"params": refs[1], "weight_decay": 0.0}],
                             lr=1e-2)
    gen = torch.Generator(device=R.dev()).manual_seed(4)
    for _ in range(4):
        grads = _rand_grads(groups, gen)
        R.set_grads(groups, grads)
        for rs, gs in zip(refs, grads):
            for r, x in zip(rs, gs):
                r.grad = x.clone()
        tnorm = torch.nn.utils.clip_grad_norm_([r for rs in refs for r in rs], 1.0)
        assert float(tnorm) > 10.0  # well above max_grad_norm
        opt.step()
        topt.step()
        torch.testing.assert_close(opt.last_grad_norm, tnorm, rtol=1e-5, atol=0)
    for g, rs in zip(groups, refs):
        for p, r in zip(g.params, rs):
            torch.testing.assert_close(p.detach(), r.detach(), atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("wdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_adam_under_the_threshold_is_bit_identical_to_unclipped(wdtype):
    from kubeflow_controller_amd.ops.optim import FusedAdam
    gen = torch.Generator(device=R.dev()).manual_seed(3)
    out, steps = [], None
    for max_norm in (1e4, None):
        groups = _groups(wdtype)
        opt = FusedAdam(groups, lr=1e-2, weight_decay=0.1, max_grad_norm=max_norm)
        if steps is None:
            steps = [_rand_grads(groups, gen) for _ in range(3)]
        for grads in steps:
            R.set_grads(groups, grads)
            opt.step()
        torch.cuda.synchronize()
        if max_norm is not None:
            assert 10.0 < float(opt.last_grad_norm) < max_norm
        out.append([g.fp32.clone() for g in groups] + [g.data.clone() for g in groups]
                   + [x.clone() for x in opt.m + opt.v])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_graph_replay_lamb_clip_matches_eager():
    """One eager step, a capture (its warm-up step trains too) and 3 replays against the same 5
    steps run eagerly, with the tolerances of test_graph_gpu.py::test_graph_adam_mlp_matches_eager."""
    from kubeflow_controller_amd.models.mnist import MnistMLP
    from kubeflow_controller_amd.ops.loss import cross_entropy
    from kubeflow_controller_amd.trainer.engine import DistInfo, Engine
    torch.manual_seed(2)
    base = MnistMLP(100)
    d = R.dev()

    def mk(optimizer="lamb", max_grad_norm=1.0):
        return Engine(copy.deepcopy(base), lambda m, x, y: cross_entropy(m(x).float(), y), optimizer=optimizer,
                      lr=0.01, weight_decay=0.01, compute_dtype=None, channels_last=False,
                      dist_info=DistInfo(device=d), max_grad_norm=max_grad_norm)
    ea, eg = mk(), mk()
    xs = [torch.rand(100, 784, device=d) for _ in range(5)]
    ys = [torch.randint(0, 10, (100,), device=d) for _ in range(5)]
    la = [float(ea.train_step(x, y)) for x, y in zip(xs, ys)]
    lg = [float(eg.train_step(xs[0], ys[0]))]
    assert eg.graph_ok() is None
    lg.append(float(eg.capture(xs[1].clone(), ys[1].clone())))
    lg += [float(eg.train_step(x, y)) for x, y in zip(xs[2:], ys[2:])]
    torch.cuda.synchronize()
    assert eg.opt.step_count == ea.opt.step_count == 5
    assert int(eg.opt._t.item()) == 5
    for a, g in zip(la, lg):
        assert abs(a - g) < 1e-4 * max(1.0, abs(a)), (la, lg)
    for ga, gg in zip(ea.groups, eg.groups):
        torch.testing.assert_close(gg.master if gg.master is not None else gg.data,
                                   ga.master if ga.master is not None else ga.data, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(eg.opt.last_grad_norm, ea.opt.last_grad_norm, atol=1e-5, rtol=1e-4)
    # no per-element scratch: LAMB keeps what Adam keeps (m and v), within 1 %
    assert eg.optimizer_bytes() <= 1.01 * mk("adam", None).optimizer_bytes()

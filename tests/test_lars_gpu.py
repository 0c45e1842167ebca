"""FusedLARS on the GPU (csrc/kernels/optim.hip: lars_norms / lars_ratio / lars_apply)
against an fp64 reference of the formula written here, and bit for bit against itself and
against FusedSGD where the two must agree.

Tolerances are those of tests/test_lamb_gpu.py: fp32 master weights and momentum
atol = rtol = 1e-4, the bf16 compute copy atol 2e-2 / rtol 1e-2, device norms and rates
against fp64 rtol 1e-5.  Weights and gradients come from a CPU generator, so the inputs do
not depend on the device's random stream."""
import copy
import functools

import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

# 5: under one vector; 63x33: several vectors and numel % 8 != 0 (64x33, from the LAMB tests, is a
# multiple of 8); 128x128: exactly one chunk; 300x300: several chunks and a ragged last one;
# 1040x1024: 65 chunks, so the rate kernel's 64-lane loop over chunks wraps
SHAPES_W = [(5,), (64, 33), (63, 33), (128, 128), (300, 300), (1040, 1024)]
SHAPES_B = [(11,), (768,)]
# lr and trust large enough that a wrong rate shows: at trust = 0.001 a whole update is below atol
HP = dict(lr=0.1, momentum=0.9, wd=0.01, trust=0.1, eps=1e-8)
ATOL = RTOL = 1e-4


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


@functools.lru_cache(maxsize=None)
def _inputs(seed, shapes_w, nsteps):
    """fp32 CPU tensors: initial weights of both groups and ``nsteps`` gradients of each."""
    gen = torch.Generator().manual_seed(seed)
    init = [[torch.randn(*s, generator=gen) for s in shapes] for shapes in (shapes_w, tuple(SHAPES_B))]
    steps = [[[torch.randn(*s, generator=gen) for s in shapes] for shapes in (shapes_w, tuple(SHAPES_B))]
             for _ in range(nsteps)]
    return init, steps


def _groups(wdtype, init, edit=None):
    """Two flat groups with a group tail (pad_to=64): "weights" in ``wdtype`` (bf16: with an
    fp32 master and a bf16 compute copy, bf16 gradients) and fp32 1-D "norms_biases"."""
    pw = [torch.nn.Parameter(x.to(R.dev()).to(wdtype)) for x in init[0]]
    pb = [torch.nn.Parameter(x.to(R.dev())) for x in init[1]]
    if edit is not None:
        edit(pw)
    return R.flat_pair(pw, pb)


def _cast_grads(groups, grads):
    """Per group, per tensor: the gradients rounded to the group's gradient dtype, on the device."""
    return [[x.to(R.dev()).to(g.grad.dtype) for x in gs] for g, gs in zip(groups, grads)]


def _reference(w0, steps, *, wd, nesterov, gscale, max_norm, lam_scale=1.0):
    """The fp64 run from the weights ``w0`` (per group, per tensor, flat) through the gradients
    ``steps`` (already in their dtype).  Returns w, mom, the rates of group 0 per step and the norms."""
    w = [[x.double().clone() for x in ws] for ws in w0]
    mom = [[torch.zeros_like(x) for x in ws] for ws in w]
    lams, norms = [], []
    for grads in steps:
        norm, coef = R.ref_clip([x for gs in grads for x in gs], gscale, max_norm)
        norms.append(norm)
        lams.append([R.ref_lars_step(w[0][k], mom[0][k], grads[0][k].flatten(), **{**HP, "wd": wd}, nesterov=nesterov,
                                     adapt=True, gs=gscale * coef, lam_scale=lam_scale) for k in range(len(w[0]))])
        for k in range(len(w[1])):
            R.ref_lars_step(w[1][k], mom[1][k], grads[1][k].flatten(), **{**HP, "wd": 0.0}, nesterov=nesterov,
                            adapt=False, gs=gscale * coef)
    return w, mom, lams, norms


def _flat_weights(groups):
    return [[g.fp32[o:o + p.numel()].clone() for o, p in zip(g.offsets, g.params)] for g in groups]


def _check_against(groups, opt, ref_w, ref_mom):
    R.check_against(groups, ([g.fp32 for g in groups], opt.mom), (ref_w, ref_mom), atol=ATOL, rtol=RTOL)


def _opt(groups, **kw):
    from kubeflow_controller_amd.ops.optim import FusedLARS
    kw = {**dict(lr=HP["lr"], momentum=HP["momentum"], weight_decay=HP["wd"], trust=HP["trust"], eps=HP["eps"]), **kw}
    return FusedLARS(groups, **kw)


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("wdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_lars_matches_fp64_reference(wdtype, max_norm, nesterov):
    from kubeflow_controller_amd.ops.optim import CHUNK
    want_chunks = [1, 1, 1, 1, 6, 65]
    assert [-(-_numel(s) // CHUNK) for s in SHAPES_W] == want_chunks
    assert _numel(SHAPES_W[3]) == CHUNK and _numel(SHAPES_W[4]) % CHUNK and _numel(SHAPES_W[2]) % 8 == 7
    init, raw = _inputs(7, tuple(SHAPES_W), 4)
    groups = _groups(wdtype, init)
    assert groups[0].numel > groups[0].offsets[-1] + _numel(SHAPES_W[-1])  # a group tail exists
    assert groups[0].grad.dtype == wdtype
    opt = _opt(groups, nesterov=nesterov, max_grad_norm=max_norm)
    assert opt._tables()[0].tens[:, 1].tolist() == want_chunks and opt._tables()[0].nchunks == sum(want_chunks)
    assert opt.trust_ratios[1] is None and opt.trust_ratios[0].shape == (len(SHAPES_W),)
    steps = [_cast_grads(groups, g) for g in raw]
    w0 = _flat_weights(groups)
    kw = dict(wd=HP["wd"], nesterov=nesterov, gscale=0.5, max_norm=max_norm)
    ref_w, ref_mom, lams, norms = _reference(w0, steps, **kw)
    # the check is sharp: a rate off by 2 % moves every adapting tensor more than 10 x atol away
    off_w = _reference(w0, steps, lam_scale=1.02, **kw)[0]
    for k, (a, b) in enumerate(zip(off_w[0], ref_w[0])):
        assert float((a - b).abs().max()) > 10 * ATOL, (k, float((a - b).abs().max()))
    got_lams, got_norms = [], []
    for grads in steps:
        R.set_grads(groups, grads)
        opt.step(grad_scale=0.5)
        got_lams.append(opt.trust_ratios[0].clone())
        got_norms.append(opt.last_grad_norm.clone() if max_norm is not None else None)
    torch.cuda.synchronize()
    assert opt.step_count == 4
    _check_against(groups, opt, ref_w, ref_mom)
    for got, want in zip(got_lams, lams):
        print("rates", got.tolist(), want)
        torch.testing.assert_close(got.double().cpu(), torch.tensor(want, dtype=torch.float64), rtol=1e-5, atol=0)
    if max_norm is None:
        assert opt.last_grad_norm is None
    else:
        assert R.ref_clip([x for gs in steps[-1] for x in gs], 0.5, max_norm)[1] < 0.1  # the clip was active
        for got, want in zip(got_norms, norms):
            torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=0)


def test_lars_rate_edge_cases():
    """|w| = 0 (an all-zero tensor) and |g| = 0 (no gradient ever) both take the rate 1: the zero
    tensor still moves, and the tensor without gradient, at wd = 0, does not move bit for bit."""
    def edit(pw):
        pw[0].data.zero_()

    shapes = ((40, 9), (129,), (64, 33))
    init, raw = _inputs(9, shapes, 3)
    groups = _groups(torch.float32, init, edit=edit)
    opt = _opt(groups, weight_decay=0.0)
    steps = [_cast_grads(groups, g) for g in raw]
    for grads in steps:
        grads[0][1].zero_()
    w0 = _flat_weights(groups)
    w1 = groups[0].params[1].detach().clone()
    ref_w, ref_mom, lams, _ = _reference(w0, steps, wd=0.0, nesterov=False, gscale=1.0, max_norm=None)
    assert lams[0][0] == 1.0 and all(l[1] == 1.0 for l in lams) and all(l[2] != 1.0 for l in lams)
    for i, grads in enumerate(steps):
        R.set_grads(groups, grads)
        opt.step()
        got = opt.trust_ratios[0].tolist()
        assert got[1] == 1.0 and (i > 0 or got[0] == 1.0)
        torch.testing.assert_close(torch.tensor(got, dtype=torch.float64),
                                   torch.tensor(lams[i], dtype=torch.float64), rtol=1e-5, atol=0)
    torch.cuda.synchronize()
    _check_against(groups, opt, ref_w, ref_mom)
    assert torch.equal(groups[0].params[1].detach(), w1)
    assert torch.count_nonzero(opt.mom[0][groups[0].offsets[1]:groups[0].offsets[1] + 129]) == 0
    assert groups[0].params[0].detach().abs().max() > 0  # the zero tensor did move, with the rate 1


def test_lars_step_is_bit_repeatable():
    init, raw = _inputs(8, tuple(SHAPES_W), 3)
    out = []
    for _ in range(2):
        groups = _groups(torch.bfloat16, init)
        opt = _opt(groups, max_grad_norm=1.0)
        for grads in [_cast_grads(groups, g) for g in raw]:
            R.set_grads(groups, grads)
            opt.step()
        torch.cuda.synchronize()
        assert float(opt.last_grad_norm) > 10.0  # clipping active
        out.append([g.fp32.clone() for g in groups] + [g.data.clone() for g in groups]
                   + [x.clone() for x in opt.mom] + [opt.trust_ratios[0].clone(), opt.last_grad_norm.clone()])
    assert float((out[0][-2] - 1).abs().min()) > 0.01  # the rates are not the neutral 1
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("max_norm", [None, 1e4], ids=["noclip", "under_threshold"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("wdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_lars_without_adapting_groups_is_bit_identical_to_sgd(wdtype, nesterov, max_norm):
    """FusedLARS(adapt_groups=()) is FusedSGD(dampening=0), also with a clip threshold well above the norm."""
    from kubeflow_controller_amd.ops.optim import FusedSGD
    init, raw = _inputs(3, tuple(SHAPES_W), 3)
    out = []
    for kind in ("lars", "sgd"):
        groups = _groups(wdtype, init)
        start = groups[0].fp32.clone()
        if kind == "lars":
            opt = _opt(groups, nesterov=nesterov, adapt_groups=(), max_grad_norm=max_norm)
            assert opt.trust_ratios == [None, None]
        else:
            opt = FusedSGD(groups, lr=HP["lr"], momentum=HP["momentum"], dampening=0.0, weight_decay=HP["wd"],
                           nesterov=nesterov)
        for grads in [_cast_grads(groups, g) for g in raw]:
            R.set_grads(groups, grads)
            opt.step(grad_scale=0.5)
        torch.cuda.synchronize()
        if kind == "lars" and max_norm is not None:
            assert 10.0 < float(opt.last_grad_norm) < max_norm
        out.append([g.fp32.clone() for g in groups] + [g.data.clone() for g in groups] + [x.clone() for x in opt.mom])
        assert float((groups[0].fp32 - start).abs().max()) > 0.1  # the steps moved the weights
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_graph_replay_lars_clip_matches_eager():
    """One eager step, a capture (its warm-up step trains too) and 3 replays against the same 5 steps
    run eagerly, with the tolerances of test_lamb_gpu.py::test_graph_replay_lamb_clip_matches_eager."""
    from kubeflow_controller_amd.models.mnist import MnistMLP
    from kubeflow_controller_amd.ops.loss import cross_entropy
    from kubeflow_controller_amd.ops.optim import FusedLARS
    from kubeflow_controller_amd.trainer.engine import DistInfo, Engine
    torch.manual_seed(2)
    base = MnistMLP(100)
    d = R.dev()

    def mk(optimizer="lars", max_grad_norm=1.0, **kw):
        return Engine(copy.deepcopy(base), lambda m, x, y: cross_entropy(m(x).float(), y), optimizer=optimizer,
                      lr=0.05, weight_decay=0.01, compute_dtype=None, channels_last=False,
                      dist_info=DistInfo(device=d), max_grad_norm=max_grad_norm, **kw)
    ea, eg = mk(trust_coefficient=0.1), mk(trust_coefficient=0.1)
    assert isinstance(eg.opt, FusedLARS) and eg.opt.trust == 0.1 and not eg.opt_overlap
    xs = [torch.rand(100, 784, device=d) for _ in range(5)]
    ys = [torch.randint(0, 10, (100,), device=d) for _ in range(5)]
    la = [float(ea.train_step(x, y)) for x, y in zip(xs, ys)]
    lg = [float(eg.train_step(xs[0], ys[0]))]
    assert eg.graph_ok() is None
    lg.append(float(eg.capture(xs[1].clone(), ys[1].clone())))
    lg += [float(eg.train_step(x, y)) for x, y in zip(xs[2:], ys[2:])]
    torch.cuda.synchronize()
    assert eg.opt.step_count == ea.opt.step_count == 5
    for a, g in zip(la, lg):
        assert abs(a - g) < 1e-4 * max(1.0, abs(a)), (la, lg)
    for ga, gg in zip(ea.groups, eg.groups):
        torch.testing.assert_close(gg.master if gg.master is not None else gg.data,
                                   ga.master if ga.master is not None else ga.data, atol=1e-5, rtol=1e-4)
    for ma, mg in zip(ea.opt.mom, eg.opt.mom):
        torch.testing.assert_close(mg, ma, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(eg.opt.last_grad_norm, ea.opt.last_grad_norm, atol=1e-5, rtol=1e-4)
    ra, rg = ea.opt.trust_ratios[0], eg.opt.trust_ratios[0]
    assert float((ra - 1).abs().min()) > 0.01  # the rates are at work
    torch.testing.assert_close(rg, ra, atol=1e-5, rtol=1e-4)
    # no per-element scratch: LARS keeps what momentum SGD keeps (mom), within 1 %
    assert eg.optimizer_bytes() <= 1.01 * mk("sgd", None).optimizer_bytes()

"""One-pass bn3 backward + conv3 dgrad / wgrad (``conv3_bwd_fused_kernel``, ``kfa_conv3_bwd_fused``).

Kernel level, against fp32 references formed from the bf16-rounded dx3 (the tensor the separate
path writes): dX2 with ``test_conv_halo_gpu.py``'s dgrad tolerance, bn2's backward statistics as
``test_halo_dgrad_with_fused_bn_backward_statistics`` compares them, dW with ``test_conv_gpu.py``'s
wgrad tolerances (overwrite / accumulate, fp32 / bf16 flat gradients), and the BatchNorm slots clean
after the backward that consumes them.

Pixel counts: 1x5x5 (25 pixels: less than one 64-pixel tile, one block), 2x9x9 (162: two tiles and
a 34-row tail), 3x20x20 with ``max_blocks=3`` (19 tiles dealt 7/6/6: multi-tile ranges, a tail,
three partial slabs) and with the default grid (one tile per block, 19 slabs).

Shapes: (Co, Ci) = (256, 64) and (512, 128), the two identity-tail shapes of ResNet-50 stages 1 and 2.

Block level: ``Bottleneck`` at 2x12x12 with the switch on and off from the same seeds, every
gradient within ``test_conv_gpu.py``'s block tolerance; with conv3's weight frozen the link takes
the materialise fallback and still matches.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(256, 64), (512, 128)]
PIXELS = [(1, 5, 5, 0), (2, 9, 9, 0), (3, 20, 20, 3), (3, 20, 20, 0)]


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(t):  # [Nb, C, H, W] channels-last -> [K, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class _Bn:  # the fields of a BnBwdLink the fused entry reads
    def __init__(self, x, mean, ss):
        self.x, self.mean, self.ss, self.mb, self.y, self.relu, self.prestats = x, mean, ss, None, None, True, False


@functools.lru_cache(maxsize=None)
def _case(Nb, H, W, Co, Ci):
    """Inputs and fp32 references of one geometry, computed once and shared (never modified)."""
    from kubeflow_controller_amd.ops import _lib, batchnorm, conv  # noqa: F401  (register the signatures)
    torch.manual_seed(Nb * 1000 + H * 10 + Co)
    d = torch.device("cuda")
    K = Nb * H * W
    g = _nhwc(torch.randn(Nb, Co, H, W, device=d).to(torch.bfloat16))
    x3 = _nhwc((torch.randn(Nb, Co, H, W, device=d) * 1.5 + 0.3).to(torch.bfloat16))
    y2 = _nhwc(torch.relu(torch.randn(Nb, Ci, H, W, device=d)).to(torch.bfloat16))
    w = _nhwc((torch.randn(Co, Ci, 1, 1, device=d) / Ci ** 0.5).to(torch.bfloat16))
    mb = torch.randint(0, 256, (K * Co // 8,), dtype=torch.uint8, device=d)  # random ReLU bits
    gamma = torch.rand(Co, device=d) + 0.5
    gamma[::7] = 0.0  # bn3 is zero-initialised in the model
    xr = _rows(x3).float()
    mean = xr.mean(0).contiguous()
    invstd = torch.rsqrt(xr.var(0, unbiased=False) + 1e-5).contiguous()
    # coef from the project's own finalize (statistics by its partial pass)
    slots = torch.zeros(_lib.lib().kfa_bn_slot_floats(Co), dtype=torch.float32, device=d)
    coef = torch.empty(3 * Co, dtype=torch.float32, device=d)
    dgam, dbet = torch.empty(Co, device=d), torch.empty(Co, device=d)
    _lib.call("kfa_bn_bwd_finalize_only", _lib.ptr(g), _lib.ptr(x3), None, _lib.ptr(gamma), _lib.ptr(mean),
              _lib.ptr(invstd), _lib.ptr(dgam), _lib.ptr(dbet), _lib.ptr(slots), _lib.ptr(coef), K, Co, 1, 0, None,
              _lib.ptr(mb), 0, _lib.stream())
    torch.cuda.synchronize()
    assert slots.abs().max().item() == 0  # finalize leaves bn3's slots clean
    # dx3 = bf16(fmaf(a, dz, fmaf(b, x, k))): each fma is one fp32 rounding of the exact value
    shifts = torch.arange(8, device=d, dtype=torch.uint8)
    mask = ((mb.view(-1, 1) >> shifts) & 1).view(K, Co).bool()
    dz = torch.where(mask, _rows(g).float(), torch.zeros((), device=d))
    a, b, k = coef[:Co].double(), coef[Co:2 * Co].double(), coef[2 * Co:].double()
    inner = (b * xr.double() + k).float()
    dx3 = (a * dz.double() + inner.double()).float().to(torch.bfloat16).float()  # [K, Co]
    wm = w.view(Co, Ci).float()
    ref_dx2 = dx3 @ wm                       # [K, Ci]
    ref_dw = dx3.t() @ _rows(y2).float()     # [Co, Ci]
    # bn2 (BatchNorm + ReLU, mask recomputed from x2 with its scale / shift)
    x2 = _nhwc(torch.randn(Nb, Ci, H, W, device=d).to(torch.bfloat16))
    mean2 = torch.randn(Ci, device=d) * 0.1
    ss2 = torch.cat([torch.rand(Ci, device=d) + 0.5, torch.randn(Ci, device=d) * 0.3]).contiguous()
    return dict(g=g, x3=x3, y2=y2, w=w, mb=mb, coef=coef, ref_dx2=ref_dx2, ref_dw=ref_dw, x2=x2, mean2=mean2,
                ss2=ss2, K=K)


def _slot_sums(Ci, d):
    from kubeflow_controller_amd.ops import _lib
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    n = _lib.lib().kfa_bn_slot_floats(Ci)
    return bn_slot_workspace(Ci, d).view(torch.float32)[:n].view(-1, 2, Ci).sum(0)


@pytest.mark.parametrize("Co,Ci", SHAPES)
@pytest.mark.parametrize("Nb,H,W,max_blocks", PIXELS)
def test_fused_dx2_statistics_dw_and_clean_slots(Nb, H, W, max_blocks, Co, Ci):
    from kubeflow_controller_amd.ops import _lib, conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    c = _case(Nb, H, W, Co, Ci)
    d = c["g"].device
    K = c["K"]
    bn_slot_workspace(Ci, d).zero_()
    bn = _Bn(c["x2"], c["mean2"], c["ss2"])
    grad = torch.full((Co, Ci, 1, 1), float("nan"), device=d).contiguous(memory_format=torch.channels_last)
    dx2 = convmod.conv3_bwd_fused(c["g"], c["x3"], c["mb"], c["coef"], c["y2"], c["w"], grad, False, bn, max_blocks)
    torch.cuda.synchronize()
    assert bn.prestats
    # splits = blocks with a non-empty range
    tiles = (K + 63) // 64
    per_cu = 2 if Ci == 64 else 1  # resident blocks per CU = the default grid's cap
    want = min(tiles, max_blocks or per_cu * torch.cuda.get_device_properties(d).multi_processor_count)
    assert _lib.lib().kfa_conv3_bwd_part_floats(Nb, H, W, Co, Ci, max_blocks) == want * Co * Ci
    # dX2
    got = _rows(dx2).float()
    ref = c["ref_dx2"]
    err = (got - ref).abs().max().item()
    print(f"dX2 max err {err:.4g} (|ref|max {ref.abs().max().item():.4g})")
    assert err < 2e-2 * max(1.0, ref.abs().max().item()), err
    # bn2's backward statistics of the bf16 dX2 the kernel wrote (order-dependent atomics)
    xr = _rows(c["x2"])
    mask = (xr.double() * c["ss2"][:Ci].double() + c["ss2"][Ci:].double()) > 0
    dz = got * mask
    sums = _slot_sums(Ci, d).clone()
    torch.testing.assert_close(sums[0], dz.sum(0), rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(sums[1], (dz * (xr.float() - c["mean2"])).sum(0), rtol=1e-3, atol=1e-1)
    # dW (fp32 gradient, overwrite)
    ref = c["ref_dw"]
    err = (grad.view(Co, Ci) - ref).abs().max().item()
    print(f"dW max err {err:.4g} (|ref|max {ref.abs().max().item():.4g})")
    assert err < 1e-2 * ref.abs().max().item(), err
    # the BN backward that consumes the slots leaves them clean
    dxb = torch.empty_like(c["x2"])
    dg, db = torch.empty(Ci, device=d), torch.empty(Ci, device=d)
    coefws = torch.empty(3 * Ci, device=d)
    _lib.call("kfa_bn_bwd_prestats", _lib.ptr(dx2), _lib.ptr(c["x2"]), None, _lib.ptr(torch.ones(Ci, device=d)),
              _lib.ptr(c["mean2"]), _lib.ptr(torch.ones(Ci, device=d)), _lib.ptr(dxb), None, _lib.ptr(dg), _lib.ptr(db),
              _lib.ptr(bn_slot_workspace(Ci, d)), _lib.ptr(coefws), K, Ci, 1, 0, _lib.ptr(c["ss2"]), None, _lib.stream())
    torch.cuda.synchronize()
    assert bn_slot_workspace(Ci, d).abs().max().item() == 0
    torch.testing.assert_close(db, sums[0], rtol=1e-4, atol=1e-3)  # dbeta = the slots' sum(dz)


@pytest.mark.parametrize("Co,Ci", SHAPES)
@pytest.mark.parametrize("dtype,accumulate", [(torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)])
def test_fused_dw_into_flat_gradient(dtype, accumulate, Co, Ci):
    """dW through wgrad_reduce_kernel into an fp32 / bf16 gradient, overwriting or accumulating."""
    from kubeflow_controller_amd.ops import conv as convmod
    c = _case(3, 20, 20, Co, Ci)
    d = c["g"].device
    ref = c["ref_dw"]
    torch.manual_seed(5)
    init = (torch.randn(Co, Ci, 1, 1, device=d) * ref.abs().max().item() * 0.5).to(dtype)
    grad = init.clone().contiguous(memory_format=torch.channels_last)
    convmod.conv3_bwd_fused(c["g"], c["x3"], c["mb"], c["coef"], c["y2"], c["w"], grad, accumulate, None, 3)
    torch.cuda.synchronize()
    want = ref + init.view(Co, Ci).float() if accumulate else ref
    err = (grad.view(Co, Ci).float() - want).abs().max().item()
    print(f"dW {dtype} accumulate={accumulate}: max err {err:.4g} (|ref|max {ref.abs().max().item():.4g})")
    assert err < 2e-2 * ref.abs().max().item(), err


def test_fused_entry_refuses_other_geometries():
    """An error, not a fallback: stride 2, a 3x3, Co != 4 Ci."""
    from kubeflow_controller_amd.ops import conv as convmod
    c = _case(1, 5, 5, 256, 64)
    d = c["g"].device
    grad = torch.zeros(256, 64, 1, 1, device=d).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        convmod.conv3_bwd_fused(c["g"], c["x3"], c["mb"], c["coef"], c["y2"], c["w"], grad, False, stride=2)
    w3 = _nhwc(torch.zeros(256, 64, 3, 3, device=d, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        convmod.conv3_bwd_fused(c["g"], c["x3"], c["mb"], c["coef"], c["y2"], w3, grad, False, pad=1)
    w128 = _nhwc(torch.zeros(128, 64, 1, 1, device=d, dtype=torch.bfloat16))  # Co = 2 Ci
    g128 = _nhwc(torch.zeros(1, 128, 5, 5, device=d, dtype=torch.bfloat16))
    grad128 = torch.zeros(128, 64, 1, 1, device=d).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        convmod.conv3_bwd_fused(g128, g128, c["mb"], c["coef"], c["y2"], w128, grad128, False)
    torch.cuda.synchronize()


def _block_run(blk, x, g, convmod, monkeypatch, on):
    monkeypatch.setattr(convmod.CONV3_BWD, "enabled", on)
    xr = x.clone().requires_grad_()
    y = blk(xr)
    y.backward(g)
    torch.cuda.synchronize()
    return y.float(), xr.grad.float(), [None if p.grad is None else p.grad.float().clone() for p in blk.parameters()]


@pytest.mark.parametrize("freeze_conv3", [False, True])
@pytest.mark.parametrize("cin,mid", [(256, 64), (512, 128)])
def test_bottleneck_grads_fused_vs_separate(cin, mid, freeze_conv3, monkeypatch):
    import copy
    from kubeflow_controller_amd.models import resnet as R
    from kubeflow_controller_amd.ops import conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    torch.manual_seed(0)
    d = torch.device("cuda")
    blk = R.Bottleneck(cin, mid, 1).to(d)
    for m in blk.modules():
        if isinstance(m, convmod.Conv2d):
            m.weight.data = m.weight.data.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        if hasattr(m, "running_var"):  # non-trivial BN parameters, some exact zeros in bn3's gamma
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.5, 0.5)
    blk.bn3.weight.data[::5] = 0.0
    if freeze_conv3:
        blk.conv3.weight.requires_grad_(False)
    blk2 = copy.deepcopy(blk)
    x = torch.randn(2, cin, 12, 12, device=d).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    g = torch.randn(2, cin, 12, 12, device=d).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(convmod.CONV3_BWD, "route", lambda *a, **k: True)  # the route says fused
    calls = {"fused": 0, "materialize": 0}
    real_fused, real_mat = convmod.TailBwd.fused, convmod.TailBwdLink.materialize

    def fused(self, *a, **k):  # (counted for conv3's record only)
        calls["fused"] += self is convmod.CONV3_BWD
        return real_fused(self, *a, **k)

    def materialize(self):
        calls["materialize"] += self.state == "deferred" and self.rec is convmod.CONV3_BWD
        return real_mat(self)

    monkeypatch.setattr(convmod.TailBwd, "fused", fused)
    monkeypatch.setattr(convmod.TailBwdLink, "materialize", materialize)
    ya, ga, pa = _block_run(blk, x, g, convmod, monkeypatch, True)
    covered = convmod.conv3_bwd_shape_ok((2, mid, 12, 12), (cin, mid, 1, 1), 1, 0)
    assert calls == {"fused": int(covered and not freeze_conv3), "materialize": int(covered and freeze_conv3)}
    yb, gb, pb = _block_run(blk2, x, g, convmod, monkeypatch, False)
    assert calls["fused"] + calls["materialize"] == int(covered)  # the switch off: neither
    # (the forward is the same code both times; its fused BatchNorm statistics are order-dependent atomics)
    assert (ya - yb).abs().max().item() <= 2e-2 * max(1.0, yb.abs().max().item())
    err = (ga - gb).abs().max().item()
    print(f"input gradient: max diff {err:.4g} (|ref|max {gb.abs().max().item():.4g})")
    assert err <= 3e-2 * max(1.0, gb.abs().max().item())
    for u, v in zip(pa, pb):
        assert (u is None) == (v is None)
        if u is not None:
            assert (u - v).abs().max().item() <= 3e-2 * max(1.0, v.abs().max().item())
    for C in (mid, 4 * mid):
        assert bn_slot_workspace(C, d).abs().max().item() == 0

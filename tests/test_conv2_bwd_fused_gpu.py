"""One-pass bn2 backward + conv2 dgrad / wgrad (``conv2_bwd_fused_kernel``, ``kfa_conv2_bwd_fused``).

Kernel level, against the project's separate path on the same inputs (``kfa_bn_bwd_apply_only`` ->
halo dgrad -> ``kfa_conv_wgrad``, with the coefficients of one ``kfa_bn_bwd_finalize_only``):
dX1 bit-equal; bn1's slot sums, dW, and dW into an fp32 / bf16 flat gradient with and without
accumulate within ``test_conv3_bwd_fused_gpu.py``'s tolerances for the same quantities; bn2's
dgamma / dbeta equal to ``kfa_bn_bwd``'s; the BatchNorm slots clean after the backward that consumes
them; a relaunch on the same buffers gives the same dX1.

Pixel cases (Nb, H, W, max_blocks), C = 64: 2x6x5 (60 pixels: less than one 256-pixel tile, every
image border inside one tile), 3x9x7 in one block, 2x16x16 (two exact tiles), 5x12x10 in ONE block
(three tiles, the last partial: dW carried across tiles, the prefetch past the end), 1x56x56 over
two blocks (the real W + 1 = 57 halo, 12.25 tiles).

Block level: ``Bottleneck(256, 64)`` at 2x12x12 with ``CONV2_BWD.enabled`` on and off from the same
seeds, every gradient within ``test_bottleneck_grads_fused_vs_separate``'s tolerances; with conv2's
weight frozen the link takes the materialise fallback and still matches.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
PIXELS = [(2, 6, 5, 0), (3, 9, 7, 1), (2, 16, 16, 0), (5, 12, 10, 1), (1, 56, 56, 2)]


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(t):  # [Nb, C, H, W] channels-last -> [M, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class _Bn:  # the fields of a BnBwdLink the entries read
    def __init__(self, x, mean, ss):
        self.x, self.mean, self.ss, self.mb, self.y, self.relu, self.prestats = x, mean, ss, None, None, True, False


def _slot_sums(d):
    from kubeflow_controller_amd.ops import _lib
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    n = _lib.lib().kfa_bn_slot_floats(C)
    return bn_slot_workspace(C, d).view(torch.float32)[:n].view(-1, 2, C).sum(0)


@functools.lru_cache(maxsize=None)
def _case(Nb, H, W):
    """Inputs of one geometry and the separate path's results, computed once and shared (never modified)."""
    from kubeflow_controller_amd.ops import _lib, batchnorm, conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    torch.manual_seed(Nb * 1000 + H * 10 + W)
    d = torch.device("cuda")
    M = Nb * H * W
    g2 = _nhwc(torch.randn(Nb, C, H, W, device=d).to(torch.bfloat16))
    x2 = _nhwc((torch.randn(Nb, C, H, W, device=d) * 1.5 + 0.3).to(torch.bfloat16))
    y1 = _nhwc(torch.relu(torch.randn(Nb, C, H, W, device=d)).to(torch.bfloat16))
    w = _nhwc((torch.randn(C, C, 3, 3, device=d) / (9 * C) ** 0.5).to(torch.bfloat16))
    gamma = torch.rand(C, device=d) + 0.5
    xr = _rows(x2).float()
    mean = xr.mean(0).contiguous()
    invstd = torch.rsqrt(xr.var(0, unbiased=False) + 1e-5).contiguous()
    ss2 = torch.cat([gamma * invstd, 0.2 - mean * gamma * invstd]).contiguous()  # bn2's forward [scale | shift]
    # bn2: finalize only (its own statistics pass), as the hand-off runs it ...
    slots = bn_slot_workspace(C, d)
    slots.zero_()
    coef = torch.empty(3 * C, dtype=torch.float32, device=d)
    dgam, dbet = torch.empty(C, device=d), torch.empty(C, device=d)
    _lib.call("kfa_bn_bwd_finalize_only", _lib.ptr(g2), _lib.ptr(x2), None, _lib.ptr(gamma), _lib.ptr(mean),
              _lib.ptr(invstd), _lib.ptr(dgam), _lib.ptr(dbet), _lib.ptr(slots), _lib.ptr(coef), M, C, 1, 0,
              _lib.ptr(ss2), None, 0, _lib.stream())
    torch.cuda.synchronize()
    assert slots.abs().max().item() == 0  # finalize leaves bn2's slots clean
    # ... and the ordinary backward: its dgamma / dbeta are the separate path's
    dx2_full = torch.empty_like(x2)
    dgam_sep, dbet_sep = torch.empty(C, device=d), torch.empty(C, device=d)
    coefws = torch.empty(3 * C, device=d)
    _lib.call("kfa_bn_bwd", _lib.ptr(g2), _lib.ptr(x2), None, _lib.ptr(gamma), _lib.ptr(mean), _lib.ptr(invstd),
              _lib.ptr(dx2_full), None, _lib.ptr(dgam_sep), _lib.ptr(dbet_sep), _lib.ptr(slots), _lib.ptr(coefws), M, C,
              1, 0, _lib.ptr(ss2), None, _lib.stream())
    # bn1 (BatchNorm + ReLU, mask recomputed from x1 with its scale / shift)
    x1 = _nhwc(torch.randn(Nb, C, H, W, device=d).to(torch.bfloat16))
    mean1 = torch.randn(C, device=d) * 0.1
    ss1 = torch.cat([torch.rand(C, device=d) + 0.5, torch.randn(C, device=d) * 0.3]).contiguous()
    # the separate path: apply pass -> halo dgrad (with bn1's backward statistics) -> wgrad
    dx2 = torch.empty_like(x2)
    _lib.call("kfa_bn_bwd_apply_only", _lib.ptr(g2), _lib.ptr(x2), None, _lib.ptr(coef), _lib.ptr(dx2), M, C, 1,
              _lib.ptr(ss2), None, _lib.stream())
    (geo, taps), = convmod.dgrad_geometries(tuple(dx2.shape), tuple(w.shape), tuple(y1.shape), 1, 1)
    wt = convmod._transposed_weight(w, *taps)
    dx1 = torch.empty_like(y1)
    slots.zero_()
    launch = geo.replace(variant=7, st=_lib.stream(), T=_lib.ptr(dx2), B=_lib.ptr(wt), D=_lib.ptr(dx1),
                         stats=_lib.ptr(slots), bn_x=_lib.ptr(x1), bn_mean=_lib.ptr(mean1), bn_relu=1,
                         bn_ss=_lib.ptr(ss1))
    assert launch.halo_ok
    launch.launch()
    torch.cuda.synchronize()
    sums = _slot_sums(d).clone()
    slots.zero_()
    dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=d).contiguous(memory_format=torch.channels_last)
    convmod.wgrad_into(y1, dx2, dw, Nb, H, W, C, H, W, C, 3, 3, 1, 1, accumulate=False)
    torch.cuda.synchronize()
    return dict(g2=g2, x2=x2, y1=y1, w=w, ss2=ss2, coef=coef, x1=x1, mean1=mean1, ss1=ss1, M=M, dx1=dx1, sums=sums,
                dw=dw, dgam=dgam, dbet=dbet, dgam_sep=dgam_sep, dbet_sep=dbet_sep)


@pytest.mark.parametrize("Nb,H,W,max_blocks", PIXELS)
def test_fused_matches_the_separate_path(Nb, H, W, max_blocks):
    from kubeflow_controller_amd.ops import _lib, conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    c = _case(Nb, H, W)
    d = c["g2"].device
    M = c["M"]
    slots = bn_slot_workspace(C, d)
    slots.zero_()
    bn = _Bn(c["x1"], c["mean1"], c["ss1"])
    grad = torch.full((C, C, 3, 3), float("nan"), device=d).contiguous(memory_format=torch.channels_last)
    dx1 = convmod.conv2_bwd_fused(c["g2"], c["x2"], c["ss2"], c["coef"], c["y1"], c["w"], grad, False, bn, max_blocks)
    torch.cuda.synchronize()
    assert bn.prestats
    tiles = (M + 255) // 256
    want = min(tiles, max_blocks or torch.cuda.get_device_properties(d).multi_processor_count)
    assert _lib.lib().kfa_conv2_bwd_part_floats(Nb, H, W, C, C, max_blocks) == want * 9 * C * C
    # dX1: bit-equal
    diff = (dx1.view(torch.int16) != c["dx1"].view(torch.int16)).sum().item()
    print(f"dX1: {diff} of {dx1.numel()} elements differ")
    assert diff == 0
    # bn1's backward statistics (order-dependent atomics)
    sums = _slot_sums(d).clone()
    print(f"slot sums: max diff {(sums - c['sums']).abs().max().item():.4g}")
    torch.testing.assert_close(sums[0], c["sums"][0], rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(sums[1], c["sums"][1], rtol=1e-3, atol=1e-1)
    # dW (fp32 gradient, overwrite)
    ref = c["dw"]
    err = (grad - ref).abs().max().item()
    print(f"dW max err {err:.4g} (|ref|max {ref.abs().max().item():.4g})")
    assert err < 1e-2 * ref.abs().max().item(), err
    # bn2's dgamma / dbeta: finalize-only against the ordinary backward
    assert torch.equal(c["dgam"], c["dgam_sep"]) and torch.equal(c["dbet"], c["dbet_sep"])
    # the BN backward that consumes the slots leaves them clean
    dxb = torch.empty_like(c["x1"])
    dg, db = torch.empty(C, device=d), torch.empty(C, device=d)
    coefws = torch.empty(3 * C, device=d)
    _lib.call("kfa_bn_bwd_prestats", _lib.ptr(dx1), _lib.ptr(c["x1"]), None, _lib.ptr(torch.ones(C, device=d)),
              _lib.ptr(c["mean1"]), _lib.ptr(torch.ones(C, device=d)), _lib.ptr(dxb), None, _lib.ptr(dg), _lib.ptr(db),
              _lib.ptr(slots), _lib.ptr(coefws), M, C, 1, 0, _lib.ptr(c["ss1"]), None, _lib.stream())
    torch.cuda.synchronize()
    assert slots.abs().max().item() == 0
    torch.testing.assert_close(db, sums[0], rtol=1e-4, atol=1e-3)  # dbeta = the slots' sum(dz)
    # a relaunch on the same buffers
    again = convmod.conv2_bwd_fused(c["g2"], c["x2"], c["ss2"], c["coef"], c["y1"], c["w"], grad, False, None,
                                    max_blocks)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int16), dx1.view(torch.int16))
    assert slots.abs().max().item() == 0  # no statistics asked for: none written


@pytest.mark.parametrize("dtype,accumulate", [(torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)])
def test_fused_dw_into_flat_gradient(dtype, accumulate):
    """dW through wgrad_reduce_kernel into an fp32 / bf16 gradient, overwriting or accumulating."""
    from kubeflow_controller_amd.ops import conv as convmod
    c = _case(5, 12, 10)
    d = c["g2"].device
    ref = c["dw"]
    torch.manual_seed(5)
    init = (torch.randn(C, C, 3, 3, device=d) * ref.abs().max().item() * 0.5).to(dtype)
    grad = init.clone().contiguous(memory_format=torch.channels_last)
    convmod.conv2_bwd_fused(c["g2"], c["x2"], c["ss2"], c["coef"], c["y1"], c["w"], grad, accumulate, None, 1)
    torch.cuda.synchronize()
    want = ref + init.float() if accumulate else ref
    err = (grad.float() - want).abs().max().item()
    print(f"dW {dtype} accumulate={accumulate}: max err {err:.4g} (|ref|max {ref.abs().max().item():.4g})")
    assert err < 2e-2 * ref.abs().max().item(), err


def test_fused_entry_refuses_other_geometries():
    """An error code and no launch: a 1x1, stride 2, C = 128, an oversize W."""
    from kubeflow_controller_amd.ops import _lib, conv as convmod  # noqa: F401  (registers the signature)
    c = _case(2, 6, 5)
    d = c["g2"].device
    grad = torch.zeros(C, C, 3, 3, device=d).contiguous(memory_format=torch.channels_last)
    dx1 = torch.full_like(c["y1"], 7.0)
    part = torch.zeros(9 * C * C, device=d)
    fn = _lib.lib().kfa_conv2_bwd_fused

    def run(Nb, H, W, Cc, Co, R, S, stride, pad):
        return fn(_lib.ptr(c["g2"]), _lib.ptr(c["x2"]), _lib.ptr(c["ss2"]), _lib.ptr(c["coef"]), _lib.ptr(c["y1"]),
                  _lib.ptr(c["w"]), _lib.ptr(dx1), _lib.ptr(grad), 1, 0, _lib.ptr(part), Nb, H, W, Cc, Co, R, S,
                  stride, pad, None, None, None, 0, None, None, 1, _lib.stream())

    assert run(2, 6, 5, 64, 64, 1, 1, 1, 0) == -1
    assert run(2, 6, 5, 64, 64, 3, 3, 2, 1) == -1
    assert run(2, 6, 5, 128, 128, 3, 3, 1, 1) == -1
    assert run(1, 2, 80, 64, 64, 3, 3, 1, 1) == -4
    torch.cuda.synchronize()
    assert (dx1.float() == 7.0).all() and grad.abs().max().item() == 0  # nothing was launched
    w1 = _nhwc(torch.zeros(C, C, 1, 1, device=d, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        convmod.conv2_bwd_fused(c["g2"], c["x2"], c["ss2"], c["coef"], c["y1"], w1, grad, False, pad=0)


def _block_run(blk, x, g, convmod, monkeypatch, on):
    monkeypatch.setattr(convmod.CONV2_BWD, "enabled", on)
    xr = x.clone().requires_grad_()
    y = blk(xr)
    y.backward(g)
    torch.cuda.synchronize()
    return y.float(), xr.grad.float(), [None if p.grad is None else p.grad.float().clone() for p in blk.parameters()]


@pytest.mark.parametrize("freeze_conv2", [False, True])
def test_bottleneck_grads_fused_vs_separate(freeze_conv2, monkeypatch):
    import copy
    from kubeflow_controller_amd.models import resnet as R
    from kubeflow_controller_amd.ops import conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    torch.manual_seed(0)
    d = torch.device("cuda")
    cin, mid = 256, 64
    blk = R.Bottleneck(cin, mid, 1).to(d)
    for m in blk.modules():
        if isinstance(m, convmod.Conv2d):
            m.weight.data = m.weight.data.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        if hasattr(m, "running_var"):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.5, 0.5)
    if freeze_conv2:
        blk.conv2.weight.requires_grad_(False)
    blk2 = copy.deepcopy(blk)
    x = torch.randn(2, cin, 12, 12, device=d).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    g = torch.randn(2, cin, 12, 12, device=d).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(convmod.CONV2_BWD, "route", lambda *a, **k: True)   # the route says fused
    monkeypatch.setattr(convmod.CONV3_BWD, "route", lambda *a, **k: False)  # conv3: the separate path both times
    calls = {"fused": 0, "materialize": 0}
    real_fused, real_mat = convmod.TailBwd.fused, convmod.TailBwdLink.materialize

    def fused(self, *a, **k):  # (counted for conv2's record only)
        calls["fused"] += self is convmod.CONV2_BWD
        return real_fused(self, *a, **k)

    def materialize(self):
        calls["materialize"] += self.state == "deferred" and self.rec is convmod.CONV2_BWD
        return real_mat(self)

    monkeypatch.setattr(convmod.TailBwd, "fused", fused)
    monkeypatch.setattr(convmod.TailBwdLink, "materialize", materialize)
    ya, ga, pa = _block_run(blk, x, g, convmod, monkeypatch, True)
    assert convmod.conv2_bwd_shape_ok((2, mid, 12, 12), (mid, mid, 3, 3), 1, 1)
    assert calls == {"fused": int(not freeze_conv2), "materialize": int(freeze_conv2)}
    yb, gb, pb = _block_run(blk2, x, g, convmod, monkeypatch, False)
    assert calls["fused"] + calls["materialize"] == 1  # the switch off: neither
    # (the forward is the same code both times; its fused BatchNorm statistics are order-dependent atomics)
    assert (ya - yb).abs().max().item() <= 2e-2 * max(1.0, yb.abs().max().item())
    err = (ga - gb).abs().max().item()
    print(f"input gradient: max diff {err:.4g} (|ref|max {gb.abs().max().item():.4g})")
    assert err <= 3e-2 * max(1.0, gb.abs().max().item())
    for u, v in zip(pa, pb):
        assert (u is None) == (v is None)
        if u is not None:
            assert (u - v).abs().max().item() <= 3e-2 * max(1.0, v.abs().max().item())
    for Cc in (mid, 4 * mid):
        assert bn_slot_workspace(Cc, d).abs().max().item() == 0

"""Halo-staged 3x3 implicit GEMM (``conv_halo_kernel``, ``kfa_conv_igemm`` variant 7):
bit-equal to the default tile variant, within the fp32-reference tolerance of
``tests/test_conv_gpu.py``, fused forward / BatchNorm-backward statistics included.

Shapes: the smallest at which the staging can go wrong —
3x10x12 (one full 256-row tile plus a tail; image boundaries and row edges inside a tile),
1x6x56 (the stage-1 halo width; the tile's halo reaches before and past the tensor),
2x9x28 (the stage-2 width; a tile boundary in mid-row), 1x1x5 (only the row's own taps are real)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HALO = 7  # kfa_conv_igemm variant
SHAPES = [(3, 10, 12), (1, 6, 56), (2, 9, 28), (1, 1, 5)]


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _launch(T, Bw, Nb, H, W, C, N, ra, variant, stats=None, bn=None):
    """One kfa_conv_igemm launch of a 3x3 stride-1 'same' conv over the channels-last
    tensor T (ra = +1 forward, -1 the dgrad orientation); returns D as [Nb, N, H, W]."""
    from kubeflow_controller_amd.ops import _lib, conv  # noqa: F401  (conv registers the signature)
    D = torch.empty((Nb, N, H, W), dtype=torch.bfloat16, device=T.device).contiguous(memory_format=torch.channels_last)
    bn_args = (None, None, None, 0, None, None) if bn is None else \
        (_lib.ptr(bn["x"]), None, _lib.ptr(bn["mean"]), 1, _lib.ptr(bn["ss"]), None)
    _lib.call("kfa_conv_igemm", _lib.ptr(T), _lib.ptr(Bw), _lib.ptr(D), None, Nb, H, W, C, H, W, 3, 3, 1, ra, -ra, -ra,
              N, H, W, 1, 0, 0, N, variant, _lib.ptr(stats), *bn_args, None, _lib.stream())
    return D


def _slots(N, d):
    from kubeflow_controller_amd.ops import _lib
    return torch.zeros(_lib.lib().kfa_bn_slot_floats(N), dtype=torch.float32, device=d)


def _inputs(Nb, H, W, C):
    torch.manual_seed(Nb * 1000 + H * 100 + W + C)
    d = torch.device("cuda")
    x = _nhwc(torch.randn(Nb, C, H, W, device=d).to(torch.bfloat16))
    w = _nhwc((torch.randn(C, C, 3, 3, device=d) / (9 * C) ** 0.5).to(torch.bfloat16))  # memory [Co][R][S][Ci]
    return x, w


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Nb,H,W", SHAPES)
def test_halo_forward_with_fused_statistics(Nb, H, W, C):
    from kubeflow_controller_amd.ops import conv as convmod
    x, w = _inputs(Nb, H, W, C)
    default = convmod._variant(Nb * H * W, C, 9 * C)
    assert default != HALO
    s_ref, s_halo = _slots(C, x.device), _slots(C, x.device)
    y_ref = _launch(x, w, Nb, H, W, C, C, 1, default, s_ref)
    y = _launch(x, w, Nb, H, W, C, C, 1, HALO, s_halo)
    assert torch.equal(y, y_ref)
    yf = torch.nn.functional.conv2d(x.float(), w.float(), None, 1, 1)
    err = (y.float() - yf).abs().max().item()
    assert err < 2e-2 * max(1.0, yf.abs().max().item()), err
    # order-dependent atomics: test_conv_gpu.py's tolerance for fused statistics
    got = s_halo.view(-1, 2, C).sum(0)
    yb = y.float().permute(0, 2, 3, 1).reshape(-1, C)
    torch.testing.assert_close(got[0], yb.sum(0), rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(got[1], (yb * yb).sum(0), rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(got, s_ref.view(-1, 2, C).sum(0), rtol=1e-3, atol=1e-1)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Nb,H,W", SHAPES)
def test_halo_dgrad_with_fused_bn_backward_statistics(Nb, H, W, C):
    """The dgrad orientation (flipped taps, transposed weight) with the backward
    statistics of the BatchNorm + ReLU it feeds, ReLU mask recomputed from x / ss."""
    from kubeflow_controller_amd.ops import conv as convmod
    dy, w = _inputs(Nb, H, W, C)
    d = dy.device
    wt = w.permute(1, 2, 3, 0).contiguous()  # [Ci][R][S][Co]
    xbn = _nhwc(torch.randn(Nb, C, H, W, device=d).to(torch.bfloat16))
    mean = torch.randn(C, device=d) * 0.1
    ss = torch.cat([torch.rand(C, device=d) + 0.5, torch.randn(C, device=d) * 0.3]).contiguous()
    bn = {"x": xbn, "mean": mean, "ss": ss}
    default = convmod._variant(Nb * H * W, C, 9 * C)
    s_ref, s_halo = _slots(C, d), _slots(C, d)
    dx_ref = _launch(dy, wt, Nb, H, W, C, C, -1, default, s_ref, bn)
    dx = _launch(dy, wt, Nb, H, W, C, C, -1, HALO, s_halo, bn)
    assert torch.equal(dx, dx_ref)
    dxf = torch.nn.grad.conv2d_input((Nb, C, H, W), w.float(), dy.float(), 1, 1)
    err = (dx.float() - dxf).abs().max().item()
    assert err < 2e-2 * max(1.0, dxf.abs().max().item()), err
    # dz = dx * (fma(x, scale, shift) > 0); the sign of the exact value (float64) is the fma's
    xr = xbn.permute(0, 2, 3, 1).reshape(-1, C)
    mask = (xr.double() * ss[:C].double() + ss[C:].double()) > 0
    dz = dx.float().permute(0, 2, 3, 1).reshape(-1, C) * mask
    got = s_halo.view(-1, 2, C).sum(0)
    torch.testing.assert_close(got[0], dz.sum(0), rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(got[1], (dz * (xr.float() - mean)).sum(0), rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(got, s_ref.view(-1, 2, C).sum(0), rtol=1e-3, atol=1e-1)


def test_halo_variant_refuses_other_geometries():
    """Variant 7 is an error, not a fallback, outside 3x3 / stride 1 / C in {64, 128}."""
    x, _ = _inputs(1, 4, 4, 64)
    d = x.device
    x256 = _nhwc(torch.zeros(1, 256, 4, 4, device=d, dtype=torch.bfloat16))
    w256 = torch.zeros(64, 3, 3, 256, device=d, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _launch(x256, w256, 1, 4, 4, 256, 64, 1, HALO)

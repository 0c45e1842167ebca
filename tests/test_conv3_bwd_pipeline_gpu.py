"""The pipelined one-pass conv3 backward (``conv3_bwd_fused_kernel``) against the separate path.

The kernel keeps the next tile's loads in flight across its own epilogue and, in both forms, stages
dX2 through LDS with its own waits.  What must not move: dX2 is the separate path's, bit for bit (the
same bf16 dx3, the same k order, the same rounding); dW is the same fp32 sum in another order; bn2's
slot sums are those of the dX2 written; nothing survives a launch.

Per case, on the operands of ``test_conv3_bwd_fused_gpu._case``:

1. dX2 == ``kfa_bn_bwd_apply_only`` + ``conv_dgrad`` (same bn2 link) on every row < K; the output is
   over-allocated by one 64-pixel unit of sentinel rows, which stay untouched.
2. dW within 1e-2 |ref|max of the fp32 reference (the existing file's tolerance).
3. dW within 2e-2 |ref|max of the separate path's ``conv_wgrad`` (two fp32 sums in different orders,
   each within 1e-2 of the reference).
4. bn2's slot sums against the reference (rtol 1e-3, atol 1e-1), and zero once
   ``kfa_bn_bwd_prestats`` consumed them.
5. A second launch on the same operands writes the identical dX2.

Geometries: 25 pixels (less than a 32-pixel half unit), 36 (a half unit plus 4 rows), 64 (one unit, no
tail), 162 (two units and a 34-row tail), 1200 pixels = 19 units in one block (the prefetch wraps
across many tiles), dealt 10 / 9, and one per block.
"""
import pytest
import torch

from test_conv3_bwd_fused_gpu import _Bn, _case, _rows, _slot_sums

pytestmark = pytest.mark.gpu

SHAPES = [(256, 64), (512, 128)]
GEOMETRIES = [(1, 5, 5, 0), (1, 6, 6, 0), (1, 8, 8, 0), (2, 9, 9, 0), (3, 20, 20, 1), (3, 20, 20, 2), (3, 20, 20, 0)]
SENTINEL = -7.0  # exactly representable in bf16
PAD_ROWS = 64


def _launch_fused(c, Co, Ci, Nb, H, W, grad, bn, max_blocks):
    """``ops.conv.conv3_bwd_fused`` with an output over-allocated by PAD_ROWS sentinel rows."""
    from kubeflow_controller_amd.ops import _lib, conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    d = c["g"].device
    K = c["K"]
    out = torch.full((K + PAD_ROWS, Ci), SENTINEL, dtype=torch.bfloat16, device=d)
    wt = convmod._transposed_weight(convmod._cl(c["w"]), 0, 1, 1, 0, 1, 1)
    nfl = _lib.lib().kfa_conv3_bwd_part_floats(Nb, H, W, Co, Ci, max_blocks)
    part = torch.empty(max(nfl, 1), dtype=torch.float32, device=d)
    ws = bn_slot_workspace(Ci, d)
    _lib.call("kfa_conv3_bwd_fused", _lib.ptr(c["g"]), _lib.ptr(c["x3"]), _lib.ptr(c["mb"]), _lib.ptr(c["coef"]),
              _lib.ptr(c["y2"]), _lib.ptr(wt), _lib.ptr(out), _lib.ptr(grad), 1, 0, _lib.ptr(part), Nb, H, W, Ci, Co,
              1, 1, 1, 0, _lib.ptr(ws), _lib.ptr(bn.x), _lib.ptr(bn.mean), int(bn.relu), _lib.ptr(bn.ss),
              _lib.ptr(bn.mb), max_blocks, _lib.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Co,Ci", SHAPES)
@pytest.mark.parametrize("Nb,H,W,max_blocks", GEOMETRIES)
def test_pipelined_kernel_against_the_separate_path(Nb, H, W, max_blocks, Co, Ci, monkeypatch):
    from kubeflow_controller_amd.ops import _lib, conv as convmod
    from kubeflow_controller_amd.ops.batchnorm import bn_slot_workspace
    monkeypatch.setattr(convmod, "TUNE", False)  # the project's own dgrad / wgrad kernels, nothing timed
    c = _case(Nb, H, W, Co, Ci)
    d = c["g"].device
    K = c["K"]
    ws = bn_slot_workspace(Ci, d)

    # the separate path: bn3's apply pass into dx3, conv3's dgrad with bn2's statistics, conv3's wgrad
    ws.zero_()
    dx3 = torch.empty_like(c["x3"])
    _lib.call("kfa_bn_bwd_apply_only", _lib.ptr(c["g"]), _lib.ptr(c["x3"]), None, _lib.ptr(c["coef"]), _lib.ptr(dx3),
              K, Co, 1, None, _lib.ptr(c["mb"]), _lib.stream())
    sep_dx2 = _rows(convmod.conv_dgrad(dx3, c["w"], c["y2"].shape, 1, 0, None, _Bn(c["x2"], c["mean2"], c["ss2"])))
    sep_dw = convmod.conv_wgrad(c["y2"], dx3, c["w"].float(), 1, 0)
    torch.cuda.synchronize()
    assert sep_dw.dtype == torch.float32
    sep_dw = sep_dw.view(Co, Ci)

    # the one-pass kernel, twice
    ws.zero_()
    bn = _Bn(c["x2"], c["mean2"], c["ss2"])
    grad = torch.full((Co, Ci), float("nan"), device=d)
    out = _launch_fused(c, Co, Ci, Nb, H, W, grad, bn, max_blocks)
    sums = _slot_sums(Ci, d).clone()
    ws.zero_()
    out2 = _launch_fused(c, Co, Ci, Nb, H, W, torch.empty_like(grad), bn, max_blocks)

    # 1. dX2: every row < K, bit for bit; the rows past K untouched
    got = out[:K]
    assert got.shape == sep_dx2.shape == (K, Ci)
    differ = (got.view(torch.int16) != sep_dx2.contiguous().view(torch.int16)).sum().item()
    print(f"dX2: {differ} of {K * Ci} elements differ from the separate path")
    assert differ == 0
    assert (out[K:] == SENTINEL).all().item()
    # 5. no state survives a launch
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))

    # 2. / 3. dW
    ref = c["ref_dw"]
    scale = ref.abs().max().item()
    err = (grad - ref).abs().max().item()
    err_sep = (grad - sep_dw).abs().max().item()
    print(f"dW: max err {err:.4g} against the reference, {err_sep:.4g} against conv_wgrad (|ref|max {scale:.4g})")
    assert err < 1e-2 * scale, err
    assert err_sep < 2e-2 * scale, err_sep

    # 4. bn2's backward statistics of the dX2 written
    xr = _rows(c["x2"])
    mask = (xr.double() * c["ss2"][:Ci].double() + c["ss2"][Ci:].double()) > 0
    dz = got.float() * mask
    torch.testing.assert_close(sums[0], dz.sum(0), rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(sums[1], (dz * (xr.float() - c["mean2"])).sum(0), rtol=1e-3, atol=1e-1)
    dx2 = got.view(Nb, H, W, Ci).permute(0, 3, 1, 2)  # channels-last [Nb, Ci, H, W]
    dxb = torch.empty_like(c["x2"])
    dg, db = torch.empty(Ci, device=d), torch.empty(Ci, device=d)
    coefws = torch.empty(3 * Ci, device=d)
    ones = torch.ones(Ci, device=d)
    _lib.call("kfa_bn_bwd_prestats", _lib.ptr(dx2), _lib.ptr(c["x2"]), None, _lib.ptr(ones), _lib.ptr(c["mean2"]),
              _lib.ptr(ones), _lib.ptr(dxb), None, _lib.ptr(dg), _lib.ptr(db), _lib.ptr(ws), _lib.ptr(coefws), K, Ci, 1,
              0, _lib.ptr(c["ss2"]), None, _lib.stream())
    torch.cuda.synchronize()
    assert ws.abs().max().item() == 0

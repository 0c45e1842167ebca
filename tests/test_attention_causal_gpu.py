"""Causal packed attention (csrc/kernels/attention.hip: attn_causal_*) against the plain fp32
reference ops.transformer.attention_varlen_reference(causal=True), computed from the same bf16
bits the kernels receive; checks and tolerances are those of test_attention_varlen_gpu.py."""
import math

import numpy as np
import pytest
import torch

from test_attention_gpu import _close, _t16
from test_attention_varlen_gpu import HEADS, HD, PAD, _keep_masks

D = torch.device("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [[1], [15, 16, 17], [31, 33], [127, 128, 129], [257, 1, 384], [400]],
                         ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_causal_fwd_bwd(p, lens):
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    H, own = HEADS * HD, sum(lens)
    T_ = own + PAD
    qkv = torch.randn(T_, 3 * H, device=D).to(torch.bfloat16)
    dout = torch.randn(T_, H, device=D).to(torch.bfloat16)
    qkv[own:] = float("nan")    # unowned rows: never read into anything
    dout[own:] = float("nan")
    bqkv = torch.randn(3 * H, device=D) * 0.1
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    seed = 987654321
    out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, HEADS, p, seed, causal=True)
    db = torch.zeros(3 * H, device=D)
    dqkv = T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, db, HEADS, p, seed, causal=True)

    xr = qkv.float().nan_to_num(0.0).requires_grad_()
    br = bqkv.clone().requires_grad_()
    keep = [torch.tril(k) for k in _keep_masks(seed, lens, T_, seqs.max_seqlen, p)] if p > 0 else None
    ref = T.attention_varlen_reference(xr, br, seqs, HEADS, keep, 1.0 / (1.0 - _t16(p) / 65536.0), causal=True)
    ref.backward(dout.float().nan_to_num(0.0))
    for name, t in (("out", out[:own]), ("lse", lse[:, :own]), ("dqkv", dqkv[:own]), ("dbqkv", db)):
        assert torch.isfinite(t.float()).all(), name
    _close(out[:own], ref[:own], 2e-2, "ctx")
    _close(dqkv[:own], xr.grad[:own], 3e-2, "dqkv")
    _close(db, br.grad, 3e-2, "dbqkv")
    assert not out[own:].any() and not dqkv[own:].any(), "unowned rows must be written as zeros"
    x = xr.detach() + bqkv
    for i, n in enumerate(lens):
        s0 = int(seqs.cu_host[i])
        q, k, _ = x[s0:s0 + n].view(n, 3, HEADS, HD).permute(1, 2, 0, 3)
        sc = ((q @ k.transpose(-1, -2)) / math.sqrt(HD)).masked_fill(~torch.ones(n, n, device=D).tril().bool(), -math.inf)
        _close(lse[:, s0:s0 + n], torch.logsumexp(sc, -1), 2e-2, "lse")


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 128, 129, 299])
def test_causal_no_look_ahead(t):
    """Queries before the cut never see rows at or past it: same shape, same work split, so
    the same operations in the same order — bit-identical."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(1)
    n, H = 300, HEADS * HD
    qkv = torch.randn(n, 3 * H, device=D).to(torch.bfloat16)
    seqs = T.PackedSeqs([0, n], n, device=D)
    out0, lse0 = T.attn_varlen_fwd(qkv, None, seqs, HEADS, causal=True)
    qkv[t:] = torch.randn(n - t, 3 * H, device=D).to(torch.bfloat16)
    out1, lse1 = T.attn_varlen_fwd(qkv, None, seqs, HEADS, causal=True)
    assert torch.equal(out0[:t], out1[:t]) and torch.equal(lse0[:, :t], lse1[:, :t])
    assert not torch.equal(out0[t:], out1[t:])


@pytest.mark.parametrize("cu,rows,max_seqlen", [
    ([0, 4, 4, 9], 16, 8),   # a zero-length sequence
    ([0, 8, 16], 12, 8),     # cu[B] > rows
    ([0, 4, 13], 16, 8),     # a length over max_seqlen
])
def test_causal_wrapper_refuses(cu, rows, max_seqlen, monkeypatch):
    """A table that went bad after construction never reaches kfa_attn_causal_*, and causal
    attention without a packed table is refused by the layer."""
    from kubeflow_controller_amd.ops import _lib
    from kubeflow_controller_amd.ops import transformer as T
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("launched"))
    seqs = T.PackedSeqs([0, 4, 9], 16, 8)
    qkv = torch.zeros(16, 3 * 2 * 64, dtype=torch.bfloat16)
    out, lse = torch.zeros(16, 128, dtype=torch.bfloat16), torch.zeros(2, 16)
    seqs.cu_host.copy_(torch.tensor(cu, dtype=torch.int32)[:3])
    seqs.rows, seqs.max_seqlen = rows, max_seqlen
    with pytest.raises(ValueError):
        T.attn_varlen_fwd(qkv[:rows], None, seqs, 2, causal=True)
    with pytest.raises(ValueError):
        T.attn_varlen_bwd(qkv[:rows], None, seqs, out[:rows], lse[:, :rows], out[:rows], None, 2, causal=True)
    x = torch.zeros(16, 128)
    prm = [torch.zeros(1)] * 12
    for fn in (T.EncoderLayerFn.apply, T.encoder_layer_reference):
        with pytest.raises(ValueError, match="packed"):
            fn(x, None, (2, 8, 2, 0.0, 0.0, 0, 1e-5, None, None, None, True), *prm)
